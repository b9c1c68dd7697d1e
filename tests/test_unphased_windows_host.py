"""The unphased indel-window builder without a device: the host twin (hawk_host_unphased_windows through
workload.unphased_windows_host) against haplotypes.unphased_indel_windows on the seam panel and on the g4_unphased* fixtures - rows,
members, labels, segments, scan bounds and the allele table - the header's geometry and survival rules against
Haplotype.add_variants_unphased on single cases, the grouping under forged signatures, the declines, the new parameter, and the
sanitizer build of the twin as a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import unphased_build_refs as ub
import unphased_window_refs as uw
from crisprhawk_hip import _lib, pipeline, search_guides as sg, workload
from resolve_refs import G4_FIXTURES
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANEL = uw.panel()
DECLINES = uw.declines()
PAMLEN = 3


def _twin(c, n_whole=0, **kw):
    codes, flags = ub.record_codes(c.rows, len(c.samples))
    assert not flags.any()
    return workload.unphased_windows_host(c.seq, c.coord.start, c.block(), c.samples, codes, c.coord, PAMLEN, row_base=1 + n_whole, **kw)


def _assert_twin_equals_host(c):
    region, haps, wins = uw.host_windows(c)   # (asserted here: a panel case builds under the host builder without raising)
    n_whole = len(haps) - 1 - len(wins)
    t = _twin(c, n_whole)
    assert t["rows"] == [h.sequence.sequence for h in wins]
    assert t["hap_len"].tolist() == [len(h.sequence) for h in wins]
    ub.assert_labels_equal(t["labels"], wins)   # samples, variants, ids, afs (values and order), segments
    key, off, ref = sg.flatten_variant_alleles(haps)
    first = int(np.searchsorted(key, np.uint64((1 + n_whole) << 32)))
    assert np.array_equal(t["alleles"][0], key[first:])
    assert np.array_equal(t["alleles"][1].astype(np.int64), off[first:].astype(np.int64) - int(off[first]))
    assert np.array_equal(t["alleles"][2], ref[int(off[first]):])
    for m, h in zip(t["meta"], wins):
        assert m.scan == sg.compute_scan_start_stop(h, region.start, region.stop, PAMLEN) and not m.is_ref
    # members: the instances of a row carry the row's sample names, and the head is the first of them in NAME order
    head = t["head"].astype(np.int64)
    for r, k in enumerate(t["row_inst"].tolist()):
        members = [c.samples[int(s)] for s in t["inst_sample"][head == k]]
        assert members == sorted(members) and ",".join(members) == wins[r].samples
        assert members[0] == c.samples[int(t["inst_sample"][k])]
    # equal rows of one indel have equal signatures; different rows of one indel different ones
    indel = np.repeat(np.arange(len(t["table"])), np.diff(t["inst_off"].astype(np.int64)))
    sig = [(int(a), int(b)) for a, b in t["sig"]]
    for k in range(len(head)):
        assert sig[k] == sig[head[k]]
    heads = t["row_inst"].tolist()
    assert len({(int(indel[k]), sig[k]) for k in heads}) == len(heads)
    return t, wins


def test_exports_exist():
    L = _lib.lib()
    for name in ("hawk_uwin_instances", "hawk_uwin_download", "hawk_uwin_signatures", "hawk_uwin_group", "hawk_uwin_fill", "hawk_uwin_free",
                 "hawk_host_unphased_windows"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert 8 in _lib.UBUILD_REASONS and 9 in _lib.UBUILD_REASONS


@pytest.mark.parametrize("name", sorted(PANEL))
def test_twin_equals_the_host_builder_on_the_panel(name):
    _assert_twin_equals_host(PANEL[name])


@pytest.mark.parametrize("fixture", G4_FIXTURES)
def test_twin_on_the_reference_fixtures(fixture):
    fx = load_golden(f"{fixture}.json.gz")
    t, wins = _assert_twin_equals_host(ub.g4_case(fx))
    assert len(wins) > 0
    # the fixture's window haplotypes are the reference's own (it walks an indel's carriers in hash order: the same rows with the
    # same carriers, not always in the same order)
    want = [w for w in fx["haplotypes"] if w["coord"] != fx["haplotypes"][0]["coord"]]
    mine = sorted((r, sorted(l.samples.split(","))) for r, l in zip(t["rows"], t["labels"]))
    assert mine == sorted((w["seq"], sorted(w["samples"].split(","))) for w in want)


def test_panel_has_the_shapes_it_claims():
    for name, c in PANEL.items():
        assert c.samples != sorted(c.samples) or len(c.samples) == 1, name   # names do not sort in column order
        assert len(c.seq) <= 1300 and len(c.samples) <= 129
    t = _twin(PANEL["starts_unclamped"])
    assert sorted(set((t["table"].a % 32).tolist())) == [0, 1, 31] and (t["table"].rowlen == 201).all()
    assert t["table"].a.tolist() == [0, 31, 32, 33]
    t = _twin(PANEL["starts_clamped"])
    assert t["table"].o.tolist() == [0, 1, 31, 32, 33, 99] and not t["table"].a.any()
    t = _twin(PANEL["right_clamp"])
    assert len(t["table"]) == 4   # the insertion on the last base is outside indel_in_region
    assert t["table"].b.tolist() == [597, 599, 599, 599]   # three windows clamped at the region's last base
    assert int(t["table"].o[3]) + int(t["table"].span[3]) - 1 == 599   # the deletion's ref ends on it
    lens = set(_twin(PANEL["row_lengths"])["hap_len"].tolist())
    assert {127, 128, 129, 159, 160, 161} <= lens
    assert sorted(set(_twin(PANEL["sizes_insertions"])["table"].grow.tolist())) == [1, 31, 32, 33, 64, 100]
    assert sorted(set(_twin(PANEL["sizes_deletions"])["table"].grow.tolist())) == [-64, -33, -32, -31, -1]
    for n in (1, 63, 64, 65, 129):
        assert int(_twin(PANEL[f"carriers_{n}"])["inst_off"][-1]) == n
    t = _twin(PANEL["equal_rows_apart"])
    assert sorted(l.samples.count(",") + 1 for l in t["labels"]) == [1, 1, 1, 4]
    big = [l for l in t["labels"] if l.samples.count(",") == 3][0]
    ranks = sorted(sorted(PANEL["equal_rows_apart"].samples).index(s) for s in big.samples.split(","))
    assert any(b - a > 1 for a, b in zip(ranks, ranks[1:]))   # its members are not neighbours in name order
    t = _twin(PANEL["all_carriers_equal"])
    assert len(t["rows"]) == 1 and t["labels"][0].samples.count(",") == 4
    assert len(_twin(PANEL["overlapping_windows"])["table"]) == 4 and int(_twin(PANEL["overlapping_windows"])["inst_off"][-1]) == 4
    t = _twin(PANEL["multi_allelic"])
    assert t["table"].o.tolist() == [300, 302] and t["table"].grow.tolist() == [-2, 2]


def test_carriers_that_differ_by_unwritten_snvs_merge_with_their_labels_joined():
    c = PANEL["merged_over_unwritten_snvs"]
    t, wins = _assert_twin_equals_host(c)
    (label,) = t["labels"]
    assert len(label.samples.split(",")) == 4
    # four members, four different variants strings: with the anchor SNV, the SNV inside the span, the SNV in the tail, without
    ids = label.variants.split(",")
    assert len([i for i in ids if "/" in i and len(i.split("-")[2].split("/")[0]) > 1]) == 4   # the deletion closes each string
    assert len(set(t["sig"][:, 0].tolist())) == 1


# ---- the header's rules on single cases, against Haplotype.add_variants_unphased
def _single(n_del=None, n_ins=None, snv_offs=(), length=700, off=300):
    c = uw.wcase("single", length, 2, 99)
    (c.deletion(off, n_del, {0: "0/1"}) if n_del else uw.ins(c, off, n_ins, {0: "0/1"}))
    for s in snv_offs:
        c.snv(s, {0: "0/1"})
    return c.sort()


@pytest.mark.parametrize("n_del,n_ins", [(1, None), (7, None), (40, None), (None, 1), (None, 9), (None, 100)])
def test_geometry_against_the_host_builder(n_del, n_ins):
    for off, length in ((300, 700), (20, 700), (650, 700), (100, 230)):
        if n_ins and n_ins > off:
            continue   # (the window would end before the scan of an unpadded region starts)
        c = _single(n_del, n_ins, length=length, off=off)
        t, wins = _assert_twin_equals_host(c)
        (w,), tab = wins, t["table"]
        assert (w.coordinates.start - c.startp, w.coordinates.stop - c.startp) == (int(tab.a[0]), int(tab.b[0]))
        assert len(w.sequence) == int(tab.rowlen[0]) and w.sequence.sequence[int(tab.i[0])].islower()
        if off >= 100 and off + (n_del or 0) + 100 < length:
            assert len(w.sequence) == 201


def test_survival_rule_against_the_host_builder():
    """every SNV offset of a deletion's and an insertion's window, one at a time: applied, covered or skipped as the builder does"""
    for n_del, n_ins in ((5, None), (None, 4)):
        for s in list(range(200, 206)) + list(range(297, 309)) + list(range(394, 407)):
            c = _single(n_del, n_ins, snv_offs=(s,))
            t, wins = _assert_twin_equals_host(c)
            g = t["table"]
            inside = int(g.a[0]) <= s <= int(g.b[0])
            assert (int(t["inst_hi"][0]) - int(t["inst_lo"][0]) == 1) == inside
            row = wins[0].sequence.sequence
            lowered = sum(ch.islower() for ch in row) - int(g.alt_len[0])
            survives = inside and s - int(g.a[0]) < int(g.rowlen[0]) and not (300 <= s < 300 + int(g.span[0]))
            assert lowered == int(survives), (n_del, n_ins, s)
            assert (tuple(t["sig"][0]) != (0, 0)) == survives


def test_grouping_splits_rows_under_forged_signatures():
    """a signature may propose a row, the comparison decides: with every signature forced equal the rows stay what the sites say"""
    for name in ("equal_rows_apart", "carriers_65", "snvs_around_a_deletion", "multi_allelic"):
        t = _twin(PANEL[name])
        forged = np.zeros_like(t["sig"])
        f = _twin(PANEL[name], forged_sig=forged)
        assert np.array_equal(f["head"], t["head"]) and f["rows"] == t["rows"] and np.array_equal(f["sig"], t["sig"])
        assert len(set(t["head"].tolist())) > 1


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_twin_declines(name):
    c, reason = DECLINES[name]
    with pytest.raises(_lib.UnphasedBuildDeclined) as e:
        _twin(c)
    assert e.value.reason == reason and "chrU-" in str(e.value)


def test_an_uncarried_indel_never_declines():
    c = uw.wcase("uncarried", 500, 2, 98)
    uw.ins(c, 250, 150, {})
    c.insertion(260, "NN", {}).deletion(300, 2, {1: "0/1"})
    t, wins = _assert_twin_equals_host(c.sort())
    assert len(wins) == 1


def test_parameter_values(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="unphased_indel_windows"):
        pipeline.search_files("x.fa", "x.bed", [], "NGG", 20, False, str(tmp_path), unphased_indel_windows="gpu")
    monkeypatch.setenv("HAWK_UNPHASED_INDEL_WINDOWS", "gpu")
    with pytest.raises(ValueError, match="HAWK_UNPHASED_INDEL_WINDOWS"):
        pipeline.search_files("x.fa", "x.bed", [], "NGG", 20, False, str(tmp_path))
    assert pipeline.UNPHASED_INDEL_WINDOWS == (None, "host", "device")
    c = PANEL["indels_alone"]
    with pytest.raises(ValueError, match="indel_windows"):
        workload.expand_unphased_from_vcf(c.seq, c.coord.start, c.coord.stop, c.block(), c.samples, PAMLEN, coord=c.coord, indel_windows="gpu")


def test_uwin_check_builds_and_passes(tmp_path):
    """the stand-alone program with the twin compiled under -fsanitize=address,undefined (its objects go to the test's directory)"""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "crispr-hawk_amd", "csrc"), "asan-uwin", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "uwin_check: ok" in r.stdout
