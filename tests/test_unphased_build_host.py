"""The unphased row builder without a device: the Python statement of the unphased genotype rule against
variant._genotypes_to_samples, the host twin (hawk_host_unphased_rows through workload.unphased_rows_host) against
haplotypes.add_variants_unphased on the seam panel and on the g4_unphased* fixtures - whose whole-region haplotypes the reference
itself produced - the declines, the new parameter, and the sanitizer build of the twin as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import unphased_build_refs as ub
from crisprhawk_hip import _lib, pipeline, workload
from crisprhawk_hip.variant import _genotypes_to_samples
from resolve_refs import G4_FIXTURES
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANEL = ub.panel()
DECLINES = ub.declines()


def test_exports_exist():
    L = _lib.lib()
    for name in ("hawk_gt_parse_unphased", "hawk_ubuild_lists", "hawk_ubuild_lists_download", "hawk_ubuild_signatures", "hawk_ubuild_fill",
                 "hawk_ubuild_free", "hawk_hapset_pack_ascii_rows", "hawk_host_unphased_rows"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_genotype_rule_agrees_with_the_reference_on_unflagged_fields():
    samples = ["s"]
    for g in ub.PLAIN:
        flags, a, b = ub.gt_rule(g)
        assert flags == 0, g
        n_alleles = 300
        sets = _genotypes_to_samples([g], samples, n_alleles, False, True)
        for k in range(1, 254):   # (254 is where allele numbers clamp)
            assert (k in (a, b)) == ("s" in sets[k - 1][0]), (g, k)
    assert ub.gt_rule("0/300:7:x")[1:] == (0, 254) and ub.gt_rule("./.")[1:] == (255, 255)


def test_genotype_rule_flags_exactly_the_malformed_fields():
    assert {g: ub.gt_rule(g)[0] for g in ub.FLAGGED} == {"1": 1, "0/1/1": 1, "0|1": 5, "0/1|2": 5, "": 5, "a/1": 4, "/1": 4}
    c = ub.Case("short", 300, 3).snv(100, {0: "0/1"})
    c.rows[0] = c.rows[0][:-1]
    assert ub.record_codes(c.rows, 3)[1].tolist() == [2]
    for g in ub.PLAIN:
        assert ub.gt_rule(g)[0] == 0


def _twin(c):
    codes, flags = ub.record_codes(c.rows, len(c.samples))
    assert not flags.any()
    return workload.unphased_rows_host(c.seq, c.coord.start, c.block(), c.samples, codes)


@pytest.mark.parametrize("name", sorted(PANEL))
def test_twin_equals_the_host_builder_on_the_panel(name):
    c = PANEL[name]
    region, haps = c.host()   # (never raises on the panel's inputs)
    whole = ub.whole_region_rows(haps)
    rows, labels, alleles, (sample_off, idx), sig, groups = _twin(c)
    assert rows == [h.sequence.sequence for h in whole]
    ub.assert_labels_equal(labels, whole)
    ub.assert_alleles_equal(alleles, [haps[0]] + whole)
    # members: first carrier first, ascending; a sample is in one row at the most; equal rows have equal signatures
    assert all(m == sorted(m) for m in groups) and len({s for m in groups for s in m}) == sum(len(m) for m in groups)
    for m in groups:
        assert len({(int(sig[s, 0]), int(sig[s, 1])) for s in m}) == 1
    assert len({(int(sig[m[0], 0]), int(sig[m[0], 1])) for m in groups}) == len(groups)


def test_panel_has_the_shapes_it_claims():
    assert len(ub.whole_region_rows(PANEL["interleaved_and_equal"].host()[1])) == 5
    labels = _twin(PANEL["interleaved_and_equal"])[1]
    assert sorted(len(l.samples.split(",")) for l in labels) == [1, 1, 1, 2, 5]
    assert [l.samples.count(",") + 1 for l in _twin(PANEL["all_equal"])[1]] == [6]
    dup = _twin(PANEL["duplicate_record"])
    assert len(dup[1]) == 1 and dup[1][0].samples == "S000,S002" and dup[3][1].tolist() == [0, 2, 1, 2]   # each carries its own copy
    assert _twin(PANEL["indels_without_snvs"])[0] == [] and len(PANEL["indels_without_snvs"].host()[1]) > 1
    assert any("n" in r for r in _twin(PANEL["multi_alts"])[0])   # three alts at one position: all four bases


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_twin_on_the_reference_fixtures(fixture):
    fx = load_golden(f"{fixture}.json.gz")
    c = ub.g4_case(fx)
    region, haps = c.host()
    whole = ub.whole_region_rows(haps)
    rows, labels, alleles, _, _, _ = _twin(c)
    assert rows == [h.sequence.sequence for h in whole] and len(rows) > 0
    ub.assert_labels_equal(labels, whole)
    ub.assert_alleles_equal(alleles, [haps[0]] + whole)
    # the fixture's whole-region haplotypes are the reference's own
    want = [w for w in fx["haplotypes"] if w["coord"] == fx["haplotypes"][0]["coord"]][1:]
    assert rows == [w["seq"] for w in want]
    assert [sorted(l.samples.split(",")) for l in labels] == [sorted(w["samples"].split(",")) for w in want]
    assert [sorted(l.variants.split(",")) for l in labels] == [sorted(w["variants"].split(",")) for w in want]


@pytest.mark.parametrize("name", sorted(n for n, (_, r) in DECLINES.items() if r != 1))
def test_twin_declines(name):
    c, reason = DECLINES[name]
    codes, flags = ub.record_codes(c.rows, len(c.samples))
    with pytest.raises(_lib.UnphasedBuildDeclined) as e:
        workload.unphased_rows_host(c.seq, c.coord.start, c.block(), c.samples, codes)
    assert e.value.reason == reason


def test_genotype_declines_are_flagged_records():
    for name, (c, reason) in DECLINES.items():
        if reason == 1:
            assert ub.record_codes(c.rows, len(c.samples))[1].any(), name


def test_an_alt_carried_twice_is_where_the_host_builder_raises():
    """the one decline that is not in the records alone: the host builder's sequential IUPAC look-up has no key for it"""
    from crisprhawk_hip.crisprhawk_error import CrisprHawkIupacTableError
    with pytest.raises(CrisprHawkIupacTableError):
        DECLINES["alt_carried_twice"][0].host()


def test_parameter_values(tmp_path):
    with pytest.raises(ValueError, match="unphased_haplotypes"):
        pipeline.search_files("x.fa", "x.bed", [], "NGG", 20, False, str(tmp_path), unphased_haplotypes="gpu")
    assert pipeline.UNPHASED_HAPLOTYPES == (None, "host", "device")


def test_phased_entry_points_at_the_unphased_builder():
    with pytest.raises(ValueError, match="expand_unphased_from_vcf"):
        workload.expand_from_vcf("ACGT", 1, 4, ub.block_of([]), [], 3, phased=False)


def test_ubuild_check_builds_and_passes(tmp_path):
    """the stand-alone program with the twin compiled under -fsanitize=address,undefined (its objects go to the test's directory)"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "crispr-hawk_amd", "csrc"), "asan-ubuild", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ubuild_check: ok" in r.stdout
