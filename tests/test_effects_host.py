"""The variant-effect data stage on the host (csrc/hawk_effects.h through hawk_host_effects) against what the reference's
graphical_reports.py / candidate_guides.py computed (tests/golden/g14_effects.json.gz, made by tests/golden/make_golden_effects.py
with the reference's stale REPORTCOLS index re-pointed - see its docstring), the rounding against Python's round(x, 4), the
refusals.  The comparison rule is stated in effects_refs.py."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

from crisprhawk_hip import _lib, candidate_guides, graphical_reports as gr
from crisprhawk_hip.crisprhawk_error import CrisprHawkCandidateGuideError, CrisprHawkGraphicalReportsError
import effects_refs as refs

TABLES = ["cfdon", "cfdon_two", "cfdon_none_valid", "azimuth", "azimuth_two", "azimuth_nans"]


def _table(name, key, engine="host"):
    fx, G, lab, columns = refs.host_report(name)
    rec = refs.g14()["fixtures"][name]
    score = "score_cfdon" if key.startswith("cfdon") else "score_azimuth"
    cg = rec["candidates"][key.split("_", 1)[1]] if "_" in key else []
    scores = {"score_azimuth": refs.group_scores(rec["score_azimuth"], columns[1])} if score == "score_azimuth" else None
    df = gr.compute_delta_table(G, lab, cg, score, engine=engine, columns=columns, scores=scores)
    return df, rec["tables"][key], len(cg), fx["report_tsv"]


@pytest.mark.parametrize("key", TABLES)
def test_host_delta_tables_match_the_reference(key):
    split, exact = 0, 0
    for name in refs.FIXTURES:
        s, e = refs.compare_table(*_table(name, key))
        split += s
        exact += e
    if key in ("cfdon", "azimuth"):
        assert split <= 1  # at most one of a score's three tables holds a split run
    assert exact > 0       # rows outside runs of equal worst deltas were compared exactly (CFDon ties a lot: most rows sit in runs)


def test_fixture_conditions_hold_for_the_reference_alone():
    fx = refs.g14()
    assert fx["k"] == 25 and all(v <= 1 for v in fx["split_tables"].values())
    t = fx["fixtures"]
    assert t["phased16"]["tables"]["cfdon"]["n_positions"] == 3729 and t["phased4"]["tables"]["cfdon"]["n_positions"] == 381
    assert t["indel_dense"]["tables"]["cfdon"]["n_positions"] == 99 and t["indel_dense"]["tables"]["cfdon"]["cut"]["split"]
    for name in refs.FIXTURES:  # the NaN cases the synthetic column was given are in it, and in a stored table as candidates:
        assert set(t[name]["score_azimuth_nans"]) == {"first_alt_nan", "later_alt_nan", "ref_nan"}
        w = t[name]["tables"]["azimuth_nans"]["worst"]  # the reference's own worst deltas - NaN, the maximum of the rest, NaN
        assert w[0] is None and w[1] is not None and w[2] is None
        row = dict(zip(t[name]["tables"]["azimuth_nans"]["columns"], t[name]["tables"]["azimuth_nans"]["rows"][0]))
        assert row["alt1_abs_delta"] is None and row["alt2_abs_delta"] is not None  # the FIRST alternative is the NaN one


@pytest.mark.parametrize("name", refs.FIXTURES)
def test_nan_first_rule_matches_the_references_worst_deltas(name):
    """pos_worst of the three planted positions against the worst deltas the reference ranked them by"""
    fx, G, lab, columns = refs.host_report(name)
    rec = refs.g14()["fixtures"][name]
    st = gr.GroupEffects(G, lab.samples, lab.is_ref, columns[1], engine="host")
    r = st.rank(gr.ABSOLUTE, refs.group_scores(rec["score_azimuth"], columns[1]), gr.parse_candidate_ids(rec["candidates"]["nans"]), 25)
    got = [None if v != v else float(v) for v in r.pos_worst[r.chosen[:3]].tolist()]
    assert [refs.bits(v) for v in got] == [refs.bits(v) for v in rec["tables"]["azimuth_nans"]["worst"][:3]]


@pytest.mark.parametrize("name", refs.FIXTURES)
def test_host_guide_type_counts_match_the_reference(name):
    fx, G, lab, columns = refs.host_report(name)
    assert gr.guide_type_counts(G, lab, columns[1], engine="host") == refs.g14()["fixtures"][name]["type_counts"]


def _round4(x):
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(a)
    _lib.check(_lib.lib().hawk_host_round4(a.ctypes.data_as(C.c_void_p), C.c_uint64(len(a)), out.ctypes.data_as(C.c_void_p)), "hawk_host_round4")
    return out


def test_round4_is_pythons_round_bit_for_bit():
    x = np.array(refs.round4_values(), dtype=np.float64)   # (the list is shared with the device's round panel)
    got = _round4(x)
    want = np.array([round(v, 4) for v in x.tolist()], dtype=np.float64)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, [(x[i], got[i], want[i]) for i in bad[:10]]
    nan = _round4(np.array([np.nan]))
    assert math.isnan(nan[0])
    # and the naive rint(x * 1e4) / 1e4 is NOT it: some product rounds across a tie
    naive = np.rint(x * 1e4) / 1e4
    assert (naive.view(np.uint64) != want.view(np.uint64)).any()


def test_refusals():
    fx, G, lab, columns = refs.host_report("phased4")
    rec = refs.g14()["fixtures"]["phased4"]
    with pytest.raises(CrisprHawkGraphicalReportsError, match="score_elevationon"):
        gr.compute_delta_table(G, lab, [], "score_elevationon", engine="host", columns=columns)
    with pytest.raises(CrisprHawkGraphicalReportsError, match="26 candidate"):
        gr.compute_delta_table(G, lab, [rec["candidates"]["two"][0]] * 26, "score_cfdon", engine="host", columns=columns)
    missing = f"{fx['contig']}_1_+"
    with pytest.raises(CrisprHawkGraphicalReportsError, match=missing.replace("+", r"\+")):
        gr.compute_delta_table(G, lab, [missing], "score_cfdon", engine="host", columns=columns)
    # a position with alternatives but no REF group is no candidate either
    import io
    import pandas as pd
    rep = pd.read_csv(io.StringIO(fx["report_tsv"]), sep="\t")
    gid = rep["chr"] + "_" + rep["start"].astype(str) + "_" + rep["strand"]
    has_ref = set(gid[rep["origin"] == "ref"])
    orphans = [g for g in gid.unique() if g not in has_ref]
    assert orphans  # phased4 has positions that only an alternative shows
    with pytest.raises(CrisprHawkGraphicalReportsError, match="no reference guide"):
        gr.compute_delta_table(G, lab, [orphans[0]], "score_cfdon", engine="host", columns=columns)
    # the library's own refusals: K out of range, more candidates than K, a sample id space above the cap
    st = gr.GroupEffects(G, lab.samples, lab.is_ref, columns[1], engine="host")
    for K, cands in ((0, ()), (65, ()), (1, ((1, 0), (2, 0)))):
        with pytest.raises(_lib.HawkStatusError) as e:
            st.rank(gr.SIGNED, None, cands, K)
        assert e.value.status == _lib.HAWK_E_INVALID
    st._cols.n_sample_ids = 65537
    with pytest.raises(_lib.HawkStatusError) as e:
        st.rank(gr.SIGNED, None, (), 25)
    assert e.value.status == _lib.HAWK_E_UNSUPPORTED


def test_panel_rules_on_the_host():
    """what the fixtures cannot show: duplicates under a flank, right=True and strand 1 type bits, an unknown type, a position
    without REF, the NaN-first rule in report order, ties in report order"""
    p = refs.rules_panel()
    order = np.arange(p.n_groups)
    st = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, engine="host")
    r = st.rank(gr.SIGNED, None, (), 25)
    assert r.type.tolist() == [0, 2, 2, 3, 0, 3, 1, 0, 255]
    assert r.dup.tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert r.counts[:6].tolist() == [3, 1, 1, 2, 1, 4]
    assert r.n_samples.tolist() == [0, 1, 3, 3, 0, 1, 1, 0, 3]
    assert r.position.tolist() == [0, 0, 0, 0, 4, 4, 6, 7, 7]
    assert r.delta[6] == 0.0 and r.pos_ref[6] == gr.FX_NONE
    assert r.pos_nvalid[[0, 4, 7]].tolist() == [3, 1, 0] and r.pos_worst[0] == 0.2 - 0.9
    assert r.chosen.tolist() == [0, 4, 7]  # -0.7, -0.6, 0.0
    assert r.alt_group[r.alt_off[0]:r.alt_off[1]].tolist() == [1, 2, 3]
    with pytest.raises(CrisprHawkGraphicalReportsError, match="Unknown guide type"):
        gr.guide_type_counts(p, None, order, engine="host", stage=st)
    # the same groups, the report in reverse: the duplicate is now the other one, the alternatives come in the other order
    st2 = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order[::-1].copy(), engine="host")
    r2 = st2.rank(gr.SIGNED, None, (), 25)
    assert r2.dup.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert r2.alt_group[r2.alt_off[0]:r2.alt_off[1]].tolist() == [3, 2, 1]
    # absolute family: NaN iff the FIRST alternative in report order is NaN
    sc = np.array([0.5, np.nan, 0.9, 0.1, 0.5, 0.6, 0.3, np.nan, 0.2])
    ra = st.rank(gr.ABSOLUTE, sc, (), 25)
    assert math.isnan(ra.pos_worst[0]) and ra.pos_worst[4] == abs(0.6 - 0.5) and math.isnan(ra.pos_worst[7])
    rb = st2.rank(gr.ABSOLUTE, sc, (), 25)
    assert rb.pos_worst[0] == 0.4  # first in (reversed) report order is group 3; the NaN comes later and is skipped
    assert ra.chosen.tolist() == [4, 0, 7]  # NaN last, then by first appearance
    st.close(); st2.close()
    pr = refs.right_panel()
    st3 = gr.GroupEffects(pr, pr.hap_samples, pr.is_ref_hap, np.arange(3), engine="host")
    assert st3.rank(gr.SIGNED, None, (), 1).type.tolist() == [0, 3, 2]  # right: the PAM comes first


@pytest.mark.parametrize("name", refs.FIXTURES)
def test_subset_reports_match_the_reference(tmp_path, name):
    fx, G, lab, columns = refs.host_report(name)
    rec = refs.g14()["fixtures"][name]
    cgs = candidate_guides.initialize_candidate_guides(rec["candidate_strings"], fx["guidelen"], True)
    from crisprhawk_hip.coordinate import Coordinate
    region = Coordinate(fx["contig"], fx["bed_start"], fx["bed_stop"], 0)
    made = candidate_guides.subset_reports(cgs, {region: columns}, refs.fixture_pam(fx), fx["guidelen"], str(tmp_path), True)
    assert len(made) == len(cgs)
    got = {os.path.basename(p): open(p).read() for p in made.values()}
    assert got == rec["subreports"]
    # ... which is the written report's header and the rows whose start is the candidate's position, byte for byte
    lines = fx["report_tsv"].splitlines(keepends=True)
    for cg, p in made.items():
        assert open(p).read() == lines[0] + "".join(ln for ln in lines[1:] if ln.split("\t")[1] == str(cg.position))
    starts = {int(ln.split("\t")[1]) for ln in lines[1:]}
    absent = next(p for p in range(fx["bed_start"], fx["bed_stop"] - fx["guidelen"]) if p not in starts)  # inside the region, no guide starts there
    bad = candidate_guides.initialize_candidate_guides([f"{fx['contig']}:{absent}:+"], fx["guidelen"], True)
    with pytest.raises(CrisprHawkCandidateGuideError, match="not found. Is the candidate guide correct"):
        candidate_guides.subset_reports(bad, {region: columns}, refs.fixture_pam(fx), fx["guidelen"], str(tmp_path), True)


def test_seam_panels_on_the_host():
    """the panels of tests/test_gpu_effects.py have the answers they were built for (there the device must give the same bits)"""
    p, want = refs.samples_panel()
    st = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, np.arange(p.n_groups), engine="host")
    r = st.rank(gr.SIGNED, None, (), 25)
    assert r.n_samples.tolist() == want and int(r.counts[6]) == 6  # past FX_SHORT_LIST: 63, 64, 65, 4097, 17 and 38 entries
    p, sizes = refs.positions_panel()
    st = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, np.arange(p.n_groups)[::-1].copy(), engine="host")
    r = st.rank(gr.SIGNED, None, (), 64)
    heads = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    assert np.array_equal(np.unique(r.position), heads) and int(r.counts[5]) == len(sizes)
    assert len(r.chosen) == 64 and set(r.chosen.tolist()) <= set(heads.tolist())
    keys = [(r.pos_worst[h], r.pos_first_rank[h]) for h in r.chosen.tolist()]
    assert keys == sorted(keys)
    p, order = refs.tie_panel()
    st = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, engine="host")
    r = st.rank(gr.SIGNED, None, (), 25)
    assert len(set(r.pos_worst[r.chosen].tolist())) == 1
    fr = r.pos_first_rank[r.chosen].tolist()
    assert fr == sorted(r.pos_first_rank[r.position == np.arange(p.n_groups)].tolist())[:25]


# ---- the plain reference (effects_refs.plain_effects: Python floats, sets and sorted(), nothing of the library) against the host
# twin: the independent check of the shared rule header, on the seam panels of tests/test_gpu_effects_seams.py and the older ones
def _host_equals_plain(p, order, calls):
    st = gr.GroupEffects(p, p.hap_samples, p.is_ref_hap, order, engine="host")
    assert st.perm is None  # the panels are built in collapse order: group numbers mean the same to both
    for family, score, cands, K in calls:
        refs.results_equal(st.rank(family, score, cands, K), refs.plain_effects(p, order, family, score, cands, K))


def test_plain_reference_restates_the_products_constants():
    assert refs.PlainResult.ARRAYS == gr.EffectsResult.ARRAYS
    assert (refs.FX_NONE, refs.FX_TYPE_UNKNOWN, refs.SIGNED, refs.ABSOLUTE, refs.FX_MAX_K) == (gr.FX_NONE, gr.FX_TYPE_UNKNOWN, gr.SIGNED, gr.ABSOLUTE, 64)
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "hawk_effects.hip")).read()
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "hawk_effects.h")).read()
    dev = open(os.path.join(os.path.dirname(_lib.__file__), "..", "csrc", "hawk_device.h")).read()
    assert f"#define FX_BLOCK {refs.FX_BLOCK}\n" in src and f"G < {refs.FX_LONG_WAVES} ? G : {refs.FX_LONG_WAVES}" in src
    assert f"#define FX_MAX_K {refs.FX_MAX_K} " in hdr and f"#define FX_SHORT_LIST {refs.FX_SHORT_LIST}u" in hdr
    assert f"#define FX_TOPK_MAX_BLOCKS {refs.FX_TOPK_MAX_BLOCKS}u" in dev


@pytest.mark.parametrize("name", refs.SEAM_CASES)
def test_seam_panels_are_on_their_seams_and_the_host_twin_equals_the_plain_reference(name):
    p, order, calls, n_long = refs.seam_case(name)
    refs.check_required(p)
    _host_equals_plain(p, order, calls)


def test_older_panels_host_twin_equals_the_plain_reference():
    p = refs.rules_panel()
    nan_scores = np.array([0.5, np.nan, 0.9, 0.1, 0.5, 0.6, 0.3, np.nan, 0.2])
    for order in (np.arange(p.n_groups), np.arange(p.n_groups)[::-1].copy()):
        _host_equals_plain(p, order, [(gr.SIGNED, None, (), 25), (gr.ABSOLUTE, nan_scores, (), 25), (gr.SIGNED, None, ((100, 1), (200, 0)), 2)])
    pr = refs.right_panel()
    _host_equals_plain(pr, np.arange(3), [(gr.SIGNED, None, (), 1), (gr.ABSOLUTE, None, (), 25)])
    p, sizes = refs.positions_panel()
    n = p.n_groups
    rng = np.random.default_rng(10)
    az = np.round(rng.random(n), 4)
    az[rng.random(n) < 0.1] = np.nan
    for order in (np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(9).permutation(n)):
        _host_equals_plain(p, order, [(gr.SIGNED, None, (), K) for K in (1, 25, 64)] + [(gr.ABSOLUTE, az, (), K) for K in (1, 25, 64)]
                           + [(gr.ABSOLUTE, az, ((int(p.start[0]), int(p.strand[0])), (1, 0)), 64)])
    p, want = refs.samples_panel()
    _host_equals_plain(p, np.arange(p.n_groups), [(gr.SIGNED, None, (), 25)])
    p, order = refs.tie_panel()
    _host_equals_plain(p, order, [(gr.SIGNED, None, (), 25), (gr.ABSOLUTE, None, (), 64)])
