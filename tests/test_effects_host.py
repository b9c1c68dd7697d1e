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
    vals = []
    for name in refs.FIXTURES:  # the fixtures' distinct unrounded scores
        _, G, _, _ = refs.host_report(name)
        vals += np.unique(G.cfdon[~np.isnan(G.cfdon)]).tolist()
    # (the issue speaks of 4x10^3 distinct scores; the three reports hold 5731 rows but only these few hundred distinct unrounded
    # CFDon values - all of them are used, and the ties, their neighbours and the random values below carry the coverage)
    assert len(set(vals)) >= 400
    ties = [0.03125, 0.09375, 0.15625, -0.03125, -0.09375]                   # k / 2^n with five decimals: exact ties
    ties += [(2 * k + 1) / 32.0 for k in range(0, 160)]                      # x.xxxx5 exactly when representable (odd / 32 has 5 decimals)
    ties += [k / 2.0 ** n for n in (5, 6, 7, 8) for k in range(1, 2 ** n, 2)]
    near = [f(t, d) for t in ties for f, d in ((math.nextafter, math.inf), (math.nextafter, -math.inf))]
    rng = np.random.default_rng(14)
    rand = rng.random(20000).tolist() + (rng.random(2000) * 200 - 100).tolist() + (rng.integers(0, 10 ** 6, 5000) / 1e5).tolist()
    decimal_ties = [(2 * k + 1) / 20000.0 for k in range(0, 3000)]           # nearest doubles to x.xxxx5: never exact, either side
    special = [0.0, -0.0, 1.0, -1.0, 1e-5, -1e-5, 5e-5, -5e-5, 4.9999e-5, 1e-300, 123456.78905, 0.99995, 0.00005, 2.5e-5]
    x = np.array(vals + ties + near + rand + decimal_ties + special, dtype=np.float64)
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
