"""Variant effects on unphased report groups, without a GPU: the new C-ABI entry is exported, declared and bound; the host chain
(rows from the strings -> hawk_host_resolve_unphased -> hawk_host_unphased_groups -> GroupEffects(engine="host")) against what the
reference's stage computed on the two unphased reports (tests/golden/g16_effects_unphased.json.gz) under effects_refs' comparison
rule; and Haplotype.add_variants_unphased with its insertion-ordered site list against a restatement of the loop it replaces."""
import os
import re
import subprocess

import numpy as np
import pytest

import effects_refs as refs
import unphased_effects_refs as ur
from crisprhawk_hip import _lib, graphical_reports as gr, haplotype as hm, reports
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.haplotype import Haplotype
from crisprhawk_hip.sequence import Sequence
from crisprhawk_hip.variant import VariantRecord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_entry_is_exported_declared_and_bound():
    L = _lib.lib()
    assert "hawk_effects_create_ugroups" in _lib.EXPORTS and hasattr(L, "hawk_effects_create_ugroups")
    hdr = open(os.path.join(ROOT, "include", "hawk.h")).read()
    decl = re.search(r"int hawk_effects_create_ugroups\(([^;]*)\);", hdr)
    assert decl and decl.group(1).count(",") == 7   # g, rank, hap_off, sample_id, n_hap, n_sample_ids, out, timing
    declared = set(re.findall(r"\b(hawk_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert set(_lib.EXPORTS) <= declared and len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) >= 114


def test_public_header_compiles_as_plain_cpp_and_as_c(tmp_path):
    for ext, cc, std in (("cpp", "g++", "-std=c++17"), ("c", "gcc", "-std=c99")):
        src = tmp_path / f"h.{ext}"
        src.write_text('#include "hawk.h"\nint main(void) { return HAWK_FX_SAMPLE_CAP == 65536 ? 0 : 1; }\n')
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / f"h_{ext}")])
        subprocess.check_call([str(tmp_path / f"h_{ext}")])


# ------------------------------------------------------------------------------------------------- the host chain against g16
def _table(name, key):
    fx, g, lab, columns = ur.host_report(name)
    rec = ur.g16()["fixtures"][name]
    cg, score = ur.table_args(name, key)
    scores = {"score_azimuth": refs.group_scores(rec["score_azimuth"], columns[1])} if score == "score_azimuth" else None
    df = gr.compute_delta_table(g, lab, cg, score, engine="host", columns=columns, scores=scores)
    return df, rec["tables"][key], len(cg), fx["report_tsv"]


@pytest.mark.parametrize("name", ur.INPUTS)
def test_host_chain_writes_the_references_report(name, tmp_path):
    """(the synthetic score column is stored per report row: the rows must be the reference's, in its order)"""
    fx, g, lab, columns = ur.host_report(name)
    path = str(tmp_path / "report.tsv")
    reports.write_report_tsv(path, *columns)
    ur.assert_report_equals_reference(open(path).read(), fx)
    assert g.n_groups == fx["report_tsv"].count("\n") - 1 and g.engine == "host"


@pytest.mark.parametrize("key", ur.TABLES)
def test_host_delta_tables_match_the_reference(key):
    split, exact = 0, 0
    for name in ur.INPUTS:
        s, e = refs.compare_table(*_table(name, key))   # (asserts at most one split run per table)
        split += s
        exact += e
    if key in ("cfdon", "azimuth"):
        assert split <= 1   # at most one of a score's two no-candidate tables holds a split run
    assert exact > 0


def test_fixture_conditions_hold_for_the_reference_alone():
    fx = ur.g16()
    assert fx["k"] == 25 and all(v <= 1 for v in fx["split_tables"].values())
    t = fx["fixtures"]
    assert t["unphased"]["tables"]["cfdon"]["n_positions"] == 370 and t["unphased_dense"]["tables"]["cfdon"]["n_positions"] == 905
    cut = t["unphased_dense"]["tables"]["cfdon"]["cut"]
    assert cut["split"] and len(cut["run_ids"]) == 3 and not t["unphased"]["tables"]["cfdon"]["cut"]["split"]
    dense = t["unphased_dense"]["fixture"]
    assert dense["unphased"] and len(dense["haplotypes"]) == 121 and dense["report_tsv"].count("\n") - 1 == 1994
    assert sum(len(v[1]) == len(v[2]) for v in dense["variants"]) == 227 and len(dense["variants"]) == 260
    for name in ur.INPUTS:
        assert sum(h["samples"] == "REF" for h in ur.fixture(name)["haplotypes"]) == 1   # more would be declined: MULTI_REF
        w = t[name]["tables"]["azimuth_nans"]["worst"]
        assert w[0] is None and w[1] is not None and w[2] is None


@pytest.mark.parametrize("name", ur.INPUTS)
def test_host_guide_type_counts_match_the_reference(name):
    fx, g, lab, columns = ur.host_report(name)
    assert gr.guide_type_counts(g, lab, columns[1], engine="host") == ur.g16()["fixtures"][name]["type_counts"]


def test_groups_without_a_device_result_stay_group_columns():
    """an UnphasedGroups of the host twin holds no handle: GroupEffects takes it as columns on either engine's column entry"""
    fx, g, lab, columns = ur.host_report("unphased")
    assert g._ug is None
    g.close()   # nothing to give back; the columns stay
    st = gr.GroupEffects(g, lab.samples, lab.is_ref, columns[1], engine="host")
    assert st._fx is None and st.n_groups == g.n_groups


# -------------------------------------------------------------------------------------------------------------- the site list
def _parent_add_variants_unphased(self, variants, sample):
    """Haplotype.add_variants_unphased as it stood with the list rebuilt for every SNV - this project's own loop, kept here as the
    yardstick of the insertion-ordered mapping that replaced the rebuild"""
    variants = hm._sort_variants(variants)
    start = self.coordinates.start
    cur, sites, va, off, deleted = {}, [], {}, 0, []
    map_keys = len(self.sequence.sequence) + sum(len(v.alt[0]) - len(v.ref) for v in variants)
    for v in variants:
        pos, ref, alt = v.position, v.ref, v.alt[0]
        if any(a < pos <= b for a, b in deleted):
            continue
        chain = len(alt) - len(ref)
        posrel = pos - start + off
        if posrel >= map_keys:
            continue
        stop = posrel + abs(chain) + 1 if chain < 0 else posrel + 1
        ref_seq = self.sequence.sequence
        refnt = "".join(cur.get(pos + i, ref_seq[pos - start + i: pos - start + i + 1]) for i in range(stop - posrel))
        if not hm.match_iupac(ref, refnt):
            raise ValueError(f"Mismatching reference alleles in VCF and reference sequence at position {pos} ({refnt} - {ref})")
        if posrel in va:
            if pos == va[posrel][0][2]:
                va[posrel].append((ref, alt, pos))
        else:
            va[posrel] = [(ref, alt, pos)]
        if v.vtype[0] == hm.VTYPES[0]:
            letter = hm.IUPAC_ENCODER["".join({hm.IUPACTABLE[refnt.upper()], alt})]
            cur[pos] = letter.lower()
            sites = [x for x in sites if x[0] != pos] + [(pos, ref.encode(), letter.encode())]
        else:
            va = {p_: a_ for p_, a_ in va.items() if p_ <= posrel or p_ >= stop}
            va = {(p_ + chain if p_ > posrel else p_): a_ for p_, a_ in va.items()}
            sites.append((pos, ref.encode(), alt.encode()))
            if chain < 0:
                deleted.append((pos, pos - chain))
            off += chain
    try:
        arr, seg = hm.expand_haplotype(self._arr, start, sites)
    except hm.HaplotypeBuildError as e:
        raise ValueError(str(e)) from e
    self._arr, self._seg = arr, seg
    self.sequence = Sequence(arr.tobytes().decode("ascii"), self._debug, allow_lower_case=True)
    self._variant_alleles = va
    self._samples = sample
    self._variants = ",".join(v.id[0] for v in variants)
    self._afs = {v.id[0]: v.afs[0] for v in variants}


START = 1000


def _records(seq, specs):
    """specs: (genomic position, ref, 'alt[,alt]') -> split VariantRecords, in the order given"""
    out = []
    for pos, ref, alt in specs:
        r = VariantRecord(True)
        n = alt.count(",") + 1
        r.read_vcf_line(["chrT", str(pos), ".", ref, alt, ".", "PASS", "AF=" + ",".join(["0.25"] * n), "GT", "0/1"], ["S1"], False)
        out += r.split()
    return out


def _hand_made(seq):
    at = lambda p, n=1: seq[p - START:p - START + n]
    other = lambda b, k=1: "ACGT"[("ACGT".index(b) + k) % 4]
    snv = lambda p, k=1: (p, at(p), other(at(p), k))
    multi = lambda p: (p, at(p), other(at(p), 1) + "," + other(at(p), 2))
    dele = lambda p, n: (p, at(p, n + 1), at(p))
    ins = lambda p, s: (p, at(p), at(p) + s)
    return {
        "multi-allelic splits at two positions": [multi(1040), snv(1050), multi(1060), snv(1061)],
        "the same position three times, other records between": [snv(1030, 1), snv(1045), snv(1030, 2), snv(1090), snv(1030, 3)],
        "records arriving unsorted": [snv(1200), dele(1150, 2), snv(1020), ins(1100, "GG"), multi(1010), snv(1199)],
        "SNVs next to a deletion": [snv(1079), snv(1080), dele(1080, 3), snv(1084), snv(1085)],
        "SNVs inside a deletion": [dele(1120, 4), snv(1121), multi(1123), snv(1124), snv(1125)],
        "an indel and a SNV at one position": [snv(1070), ins(1070, "T"), dele(1130, 1), snv(1130)],
        "a SNV in the tail a deletion shortens": [dele(1100, 5), snv(START + len(seq) - 2)],
    }


def _seeded(seq, seed, n=40):
    rng = np.random.default_rng(seed)
    specs = []
    for p in sorted(rng.choice(np.arange(START + 5, START + len(seq) - 12), size=n, replace=False).tolist()):
        b = seq[p - START]
        kind = rng.random()
        if kind < 0.55:
            specs.append((p, b, "ACGT"[("ACGT".index(b) + int(rng.integers(1, 4))) % 4]))
        elif kind < 0.75:
            specs.append((p, b, "ACGT"[("ACGT".index(b) + 1) % 4] + "," + "ACGT"[("ACGT".index(b) + 2) % 4]))
        elif kind < 0.9:
            specs.append((p, seq[p - START:p - START + 1 + int(rng.integers(1, 4))], b))
        else:
            specs.append((p, b, b + "".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4))))))
    return [specs[i] for i in rng.permutation(len(specs))]


def _run(method, seq, recs, monkeypatch):
    h = Haplotype(Sequence(seq, True), Coordinate("chrT", START, START + len(seq) - 1, 0), False, 0, True)
    handed = []
    real = hm.expand_haplotype
    monkeypatch.setattr(hm, "expand_haplotype", lambda arr, start, sites: handed.append(list(sites)) or real(arr, start, sites))
    try:
        method(h, list(recs), "S1")
    except ValueError as e:
        return ("ValueError", str(e)), handed
    finally:
        monkeypatch.setattr(hm, "expand_haplotype", real)
    seg = h.segments
    return (h.sequence.sequence, {k: list(v) for k, v in h.variant_alleles.items()}, seg.full().tolist(), seg.length, h.samples, h.variants,
            {k: v for k, v in h.afs.items()}), handed


def test_site_list_mapping_equals_the_rebuilt_list(monkeypatch):
    seq = "".join("ACGT"[int(x)] for x in np.random.default_rng(77).integers(0, 4, 260))
    cases = dict(_hand_made(seq))
    for seed in range(12):
        cases[f"seeded {seed}"] = _seeded(seq, 500 + seed)
    built = 0
    for label, specs in cases.items():
        recs = _records(seq, specs)
        want, want_sites = _run(_parent_add_variants_unphased, seq, recs, monkeypatch)
        got, got_sites = _run(Haplotype.add_variants_unphased, seq, recs, monkeypatch)
        assert got_sites == want_sites, label   # the list handed to expand_haplotype, element for element
        assert got == want, label
        built += want[0] != "ValueError"
        if label.startswith(("multi", "the same")):   # the yardstick itself keeps one entry per position, the last, at the end
            pos = [s[0] for s in want_sites[0]]
            assert len(pos) == len(set(pos)) and want[0] != "ValueError"
    assert built >= len(_hand_made(seq))   # (seeded sets may hold overlapping indels, which the builder refuses - either way alike)
