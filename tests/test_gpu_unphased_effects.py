"""Variant effects on the report groups of an unphased interval while they are still in HBM (hawk_effects_create_ugroups behind
hapset.UnphasedGroups kept resident): the new entry against hawk_effects_create_columns on the same groups downloaded and against
the host twin, bit for bit; origin and lifetime; the empty result, groups without CFD tables, the refusals; and
pipeline.search_files(unphased_effects=True) from files against the reference's stage (tests/golden/g16_effects_unphased.json.gz)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import effects_refs as refs
import ugroups_refs as ug
import unphased_effects_refs as ur
from crisprhawk_hip import _lib, graphical_reports as gr, pipeline, readers, reports, scoring, search_guides as sg, synth
from crisprhawk_hip.hapset import _p

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ helpers
def _resident(region, haps, pam, guidelen, right, flank=(0, 0), tables=ur.CFD):
    """-> (set, table, UnphasedGroups that still hold their device result); the caller closes all three"""
    ds = sg._device_set(region, haps, len(pam))
    tab = ds.search(pam.bits, pam.bitsrc, len(pam), guidelen, right, download=False)
    g = tab.resolve_unphased_groups(haps, pam, tables, flank, "device", keep_resident=True)
    assert g._ug is not None and g.n_hap == len(haps)
    return ds, tab, g


def _downloaded(g):
    """the same groups as columns alone"""
    d = copy.copy(g)
    d._ug = None
    return d


def _labels(haps):
    return reports.HapLabels.from_objects(haps), np.array([h.samples == "REF" for h in haps], dtype=bool)


class _Calls:
    """counts what GroupEffects calls of the two create entries that take group columns or resident groups"""

    def __init__(self, monkeypatch):
        L = _lib.lib()
        self.columns = self.ugroups = 0
        real_c, real_u = L.hawk_effects_create_columns, L.hawk_effects_create_ugroups

        def columns(*a):
            self.columns += 1
            return real_c(*a)

        def ugroups(*a):
            self.ugroups += 1
            return real_u(*a)
        monkeypatch.setattr(L, "hawk_effects_create_columns", columns)
        monkeypatch.setattr(L, "hawk_effects_create_ugroups", ugroups)


def _orphans(g):
    """positions (start, strand) no REF group sits at"""
    pos = list(zip(np.asarray(g.start).tolist(), np.asarray(g.strand).tolist()))
    with_ref = {p for p, r in zip(pos, np.asarray(g.is_ref).tolist()) if r}
    return [p for p in dict.fromkeys(pos) if p not in with_ref]


def _create(g_handle, rank, hap_off, sid, n_hap, n_ids):
    fx, tm = C.c_void_p(), _lib.EffectsTiming()
    rc = _lib.lib().hawk_effects_create_ugroups(g_handle, _p(rank), _p(hap_off), _p(sid), C.c_uint32(n_hap), C.c_uint32(n_ids), C.byref(fx), C.byref(tm))
    return rc, fx, tm


# ------------------------------------------------------------------------------------------------- three routes, bit for bit
@pytest.mark.parametrize("flank", ur.FLANKS)
@pytest.mark.parametrize("name", ur.INPUTS)
def test_resident_groups_columns_route_and_host_twin_agree_bit_for_bit(name, flank, monkeypatch):
    fx, region, haps, pam = ur.built(name)
    rec = ur.g16()["fixtures"][name]
    ds, tab, g = _resident(region, haps, pam, fx["guidelen"], fx["right"], flank)
    try:
        lab, is_ref = _labels(haps)
        ng = g.n_groups
        if flank == (0, 0):
            assert ng == fx["report_tsv"].count("\n") - 1
        order = np.asarray(reports.group_columns(g, lab, pam, fx["contig"], fx["target"], with_cfdon=True, is_ref_hap=is_ref)[1])
        calls = _Calls(monkeypatch)
        res = gr.GroupEffects(g, lab.samples, is_ref, order, "device")
        assert (calls.ugroups, calls.columns) == (1, 0) and res.timing["n_groups"] == ng and res.perm is None
        down = _downloaded(g)
        cols = gr.GroupEffects(down, lab.samples, is_ref, order, "device")
        host = gr.GroupEffects(down, lab.samples, is_ref, order, "host")
        assert (calls.ugroups, calls.columns) == (1, 1) and cols.perm is None and host.perm is None
        rng = np.random.default_rng(160 + len(name) + flank[0])
        az = np.round(rng.random(ng), 4)
        az[rng.random(ng) < 0.1] = np.nan
        present = gr.parse_candidate_ids(rec["candidates"]["two"])
        orphan = _orphans(g)
        assert orphan and all(any(s == int(a) and t == int(b) for a, b in zip(g.start, g.strand)) for s, t in present)
        cand_sets = [(), tuple(present), ((1, 0),), (orphan[0],), (present[0], (1, 0), orphan[-1], present[1])]
        checked = 0
        for family, score in ((gr.SIGNED, None), (gr.ABSOLUTE, az)):
            for K in (1, 25, 64):
                for cands in cand_sets:
                    cands = cands[:K]
                    r = res.rank(family, score, cands, K)
                    refs.results_equal(r, cols.rank(family, score, cands, K))
                    refs.results_equal(r, host.rank(family, score, cands, K))
                    assert len(r.chosen) == K   # (hundreds of positions have a REF group)
                    if cands == (orphan[0],) or cands == ((1, 0),):
                        assert r.chosen[0] == gr.FX_NONE
                    checked += 1
        assert checked == 30
        # the origin the handle took from the groups: k_fx_isref_gather's on the set's flags and the first members (the columns
        # route runs it), and the groups' own column
        r = res.rank(gr.SIGNED, None, (), 25)
        first = np.asarray(g.member_hap)[np.asarray(g.member_off).astype(np.int64)[:-1]]
        assert np.array_equal(r.type == 0, np.asarray(g.is_ref).astype(bool)) and np.array_equal(np.asarray(g.is_ref).astype(bool), is_ref[first])
        assert np.array_equal(r.type == 0, cols.rank(gr.SIGNED, None, (), 25).type == 0)
        for st in (res, cols, host):
            st.close()
    finally:
        g.close(); tab.close(); ds.close()


def test_the_handle_outlives_groups_resolution_table_and_set():
    fx, region, haps, pam = ur.built("unphased")
    rec = ur.g16()["fixtures"]["unphased"]
    ds, tab, g = _resident(region, haps, pam, fx["guidelen"], fx["right"])   # (the hawk_resolve handle is freed in there already)
    lab, is_ref = _labels(haps)
    order = np.asarray(reports.group_columns(g, lab, pam, fx["contig"], fx["target"], with_cfdon=True, is_ref_hap=is_ref)[1])
    early = gr.GroupEffects(g, lab.samples, is_ref, order, "device")
    late = gr.GroupEffects(g, lab.samples, is_ref, order, "device")    # created before the frees, first ranked after them
    cands = gr.parse_candidate_ids(rec["candidates"]["two"])
    az = np.round(np.random.default_rng(5).random(g.n_groups), 4)
    before = [early.rank(gr.SIGNED, None, cands, 25), early.rank(gr.ABSOLUTE, az, (), 64)]
    g.close(); tab.close(); ds.close()
    assert g._ug is None
    g.close()   # twice is fine
    # memory the pool hands out again: another set, table and groups take the place of the freed ones
    ds2, tab2, g2 = _resident(region, haps, pam, fx["guidelen"], fx["right"], (4, 3))
    try:
        for st in (early, late):
            after = [st.rank(gr.SIGNED, None, cands, 25), st.rank(gr.ABSOLUTE, az, (), 64)]
            for a, b in zip(before, after):
                refs.results_equal(a, b)
    finally:
        g2.close(); tab2.close(); ds2.close()
        early.close(); late.close()


# ------------------------------------------------------------------------------------------------ edge cases and refusals
def test_zero_kept_guides_give_a_handle_of_zero_groups(tmp_path):
    """REF alone, its one row not valid: a table of one row that keeps nothing (ugroups_refs.short_ref_rows)"""
    region, haps, pam, t = ug.short_ref_rows()
    ds, tab, g = _resident(region, haps[:1], pam, 20, False, (4, 3))
    try:
        assert (g.n_kept, g.n_groups, g.n_members) == (0, 0, 0) and tab.n_rows == 1
        lab, is_ref = _labels(haps[:1])
        st = gr.GroupEffects(g, lab.samples, is_ref, np.zeros(0, np.int64), "device")
        assert st._fx is not None and st.n_groups == 0 and st.timing["n_groups"] == 0
        r = st.rank(gr.SIGNED, None, (), 25)
        assert len(r.chosen) == 0 and r.alt_off.tolist() == [0] and r.counts.tolist() == [0] * 8
        st.close()
        columns = reports.group_columns(g, lab, pam, "chrP", "chrP:1-2", with_cfdon=True, is_ref_hap=is_ref)
        from types import SimpleNamespace
        made = gr.compute_graphical_reports(g, lab, columns, SimpleNamespace(contig="chrP", start=900, stop=2100), str(tmp_path), [], None,
                                            is_ref_hap=is_ref)
        assert [os.path.basename(p) for p in made] == ["chrP_1000_2000_guides_type.tsv"]   # the type table, no delta table
        assert open(made[0]).read() == ur.type_table_text({label: 0 for label in gr.GUIDETYPES.values()})
    finally:
        g.close(); tab.close(); ds.close()


def test_groups_made_without_cfd_tables_need_scores():
    fx, region, haps, pam = ur.built("unphased")
    ds, tab, g = _resident(region, haps, pam, fx["guidelen"], fx["right"], (0, 0), None)
    try:
        assert np.all(np.isnan(g.cfdon))
        lab, is_ref = _labels(haps)
        order = np.arange(g.n_groups)
        res = gr.GroupEffects(g, lab.samples, is_ref, order, "device")
        with pytest.raises(_lib.HawkStatusError) as e:
            res.rank(gr.SIGNED, None, (), 25)
        assert e.value.status == _lib.HAWK_E_INVALID
        az = np.round(np.random.default_rng(6).random(g.n_groups), 4)
        host = gr.GroupEffects(_downloaded(g), lab.samples, is_ref, order, "host")
        for family in (gr.SIGNED, gr.ABSOLUTE):
            refs.results_equal(res.rank(family, az, (), 25), host.rank(family, az, (), 25))
        res.close()
    finally:
        g.close(); tab.close(); ds.close()


def test_refusals_leave_nothing_behind_and_the_next_call_succeeds():
    fx, region, haps, pam = ur.built("unphased")
    ds, tab, g = _resident(region, haps, pam, fx["guidelen"], fx["right"])
    try:
        L = _lib.lib()
        ng, n_hap = g.n_groups, len(haps)
        lab, _ = _labels(haps)
        hap_off, sid, n_ids = gr.sample_csr(lab.samples)
        assert n_ids == len(fx["samples"]) and len(sid) > 0
        rank = np.arange(ng, dtype=np.uint32)[::-1].copy()

        def good():
            rc, fx_h, tm = _create(g._ug, rank, hap_off, sid, n_hap, n_ids)
            assert rc == _lib.HAWK_OK and fx_h.value and tm.n_groups == ng
            L.hawk_effects_free(fx_h)
        good()
        twice = rank.copy(); twice[1] = twice[0]
        beyond = rank.copy(); beyond[0] = ng
        bad_sid = sid.copy(); bad_sid[-1] = n_ids
        longer = np.concatenate([hap_off, hap_off[-1:]])
        refusals = [
            ("wrong n_hap", (g._ug, rank, longer, sid, n_hap + 1, n_ids), _lib.HAWK_E_INVALID),
            ("rank with a value twice", (g._ug, twice, hap_off, sid, n_hap, n_ids), _lib.HAWK_E_INVALID),
            ("rank with a value out of range", (g._ug, beyond, hap_off, sid, n_hap, n_ids), _lib.HAWK_E_INVALID),
            ("a sample id >= n_sample_ids", (g._ug, rank, hap_off, bad_sid, n_hap, n_ids), _lib.HAWK_E_INVALID),
            ("n_sample_ids above the cap", (g._ug, rank, hap_off, sid, n_hap, 65537), _lib.HAWK_E_UNSUPPORTED),
            ("no groups handle", (None, rank, hap_off, sid, n_hap, n_ids), _lib.HAWK_E_INVALID),
        ]
        for label, args, status in refusals:
            rc, fx_h, _ = _create(*args)
            assert rc == status and not fx_h.value, label
            good()
        rc, fx_h, _ = _create(g._ug, rank, hap_off, sid, n_hap, 65536)   # the cap itself is served
        assert rc == _lib.HAWK_OK and fx_h.value
        L.hawk_effects_free(fx_h)
    finally:
        g.close(); tab.close(); ds.close()


def test_keep_resident_is_the_device_engines():
    fx, region, haps, pam = ur.built("unphased")
    ds = sg._device_set(region, haps, len(pam))
    tab = ds.search(pam.bits, pam.bitsrc, len(pam), fx["guidelen"], fx["right"], download=False)
    try:
        with pytest.raises(ValueError, match="keep_resident"):
            tab.resolve_unphased_groups(haps, pam, ur.CFD, (0, 0), "host", keep_resident=True)
        g = tab.resolve_unphased_groups(haps, pam, ur.CFD, (0, 0), "device")   # the default gives the handle back at once
        assert g._ug is None
    finally:
        tab.close(); ds.close()


# ------------------------------------------------------------------------------------------------------------- from files
def _spy(monkeypatch, fail=None):
    from test_gpu_unphased_groups import _Spy
    return _Spy(monkeypatch, fail=fail)


def _files_of(root):
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("key", ["cfdon", "cfdon_two", "cfdon_none_valid"])
@pytest.mark.parametrize("name", ur.INPUTS)
def test_search_files_runs_the_stage_on_resident_groups(name, key, tmp_path, monkeypatch):
    import pandas as pd
    fx = ur.fixture(name)
    rec = ur.g16()["fixtures"][name]
    fa, bed, vcf = ur.write_files(fx, tmp_path / "in")
    cg, _ = ur.table_args(name, key)
    cstr = [f"{fx['contig']}:{c.split('_')[-2]}:{c.split('_')[-1]}" for c in cg]
    spy, calls, figures = _spy(monkeypatch), _Calls(monkeypatch), {}
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=ur.CFD,
                                    unphased_effects=True, graphical_reports=True, candidate_guides=cstr, figures=figures).values()
    assert spy.took_the_device_route()                       # no Guide object
    assert (calls.ugroups, calls.columns) == (1, 0)          # the groups were ranked where they lay
    assert spy.groups[0]._ug is None                         # ... and given back
    ur.assert_report_equals_reference(open(path).read(), fx)
    (made,) = figures.values()
    base = {os.path.basename(p): p for p in made}
    prefix = f"{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}"
    subs = {f"crisprhawk_candidate_guides__{fx['contig']}_{c.split(':')[1]}_{fx['pam']}_{fx['guidelen']}.tsv" for c in cstr}
    assert set(base) == {f"{prefix}_score_cfdon_delta.tsv", f"{prefix}_guides_type.tsv"} | subs and len(subs) == len(cstr)
    df = pd.read_csv(base[f"{prefix}_score_cfdon_delta.tsv"], sep="\t", float_precision="round_trip")
    refs.compare_table(df, rec["tables"][key], len(cg), fx["report_tsv"])
    assert open(base[f"{prefix}_guides_type.tsv"]).read() == ur.type_table_text(rec["type_counts"])
    for k in subs:
        ur.assert_subreport_equals_reference(open(base[k]).read(), rec["subreports"][k], open(path).read(), fx)


def test_search_files_candidates_alone_need_no_resident_groups(tmp_path, monkeypatch):
    fx = ur.fixture("unphased")
    rec = ur.g16()["fixtures"]["unphased"]
    fa, bed, vcf = ur.write_files(fx, tmp_path / "in")
    spy, calls, figures = _spy(monkeypatch), _Calls(monkeypatch), {}
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"), cfd_tables=ur.CFD,
                                    unphased_effects=True, candidate_guides=rec["candidate_strings"], figures=figures).values()
    assert spy.took_the_device_route() and (calls.ugroups, calls.columns) == (0, 0)
    (made,) = figures.values()
    assert {os.path.basename(p) for p in made} == set(rec["subreports"]) and len(made) == 3
    for p in made:
        ur.assert_subreport_equals_reference(open(p).read(), rec["subreports"][os.path.basename(p)], open(path).read(), fx)


class _Panel:
    """an UnphasedGroups as effects_refs.plain_effects reads a panel"""

    def __init__(self, g, hap_samples, is_ref_hap):
        self.guidelen, self.pamlen, self.right, self.n_groups = g.guidelen, g.pamlen, g.right, g.n_groups
        self.start, self.stop, self.strand = np.asarray(g.start, np.int64), np.asarray(g.stop, np.int64), np.asarray(g.strand, np.uint8)
        self.cfdon, self.wins = np.asarray(g.cfdon, np.float64), g.windows()
        off = np.asarray(g.member_off).astype(np.int64)
        self.members = [np.asarray(g.member_hap)[off[i]:off[i + 1]].tolist() for i in range(g.n_groups)]
        self.hap_samples, self.is_ref_hap = list(hap_samples), list(is_ref_hap)


def test_search_files_with_deepcpf1_ranks_the_flanked_groups(tmp_path, monkeypatch):
    """Cpf1 with DeepCpf1 on: groups keyed on the scorer's k-mer, no CFDon - the file set is the score's delta table and the type
    table, and what the stage computed is the plain restatement (effects_refs.plain_effects) on the downloaded groups"""
    from test_gpu_unphased_groups import _g4_files
    fx, reg, fa, bed, vcf = _g4_files(tmp_path, "g4_unphased_cpf1")
    spy, calls, figures, seen = _spy(monkeypatch), _Calls(monkeypatch), {}, []
    real_init, real_rank = gr.GroupEffects.__init__, gr.GroupEffects.rank

    def init(self, groups, hap_samples, is_ref_hap, order, engine="device"):
        real_init(self, groups, hap_samples, is_ref_hap, order, engine)
        self._seen = dict(samples=list(hap_samples), is_ref=np.asarray(is_ref_hap).tolist(), order=np.asarray(order).copy())

    def rank(self, family, score=None, candidates=(), K=gr.TOPK):
        r = real_rank(self, family, score, candidates, K)
        seen.append((self._seen, family, None if score is None else np.asarray(score, np.float64).copy(), tuple(candidates), K, r))
        return r
    monkeypatch.setattr(gr.GroupEffects, "__init__", init)
    monkeypatch.setattr(gr.GroupEffects, "rank", rank)
    (path,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "out"),
                                    deepcpf1_weights=synth.deepcpf1_weights(), unphased_effects=True, graphical_reports=True, figures=figures).values()
    assert spy.took_the_device_route() and (calls.ugroups, calls.columns) == (1, 0)
    (made,) = figures.values()
    prefix = f"{reg.contig}_{reg.bed_start}_{reg.bed_stop}"
    assert {os.path.basename(p) for p in made} == {f"{prefix}_score_deepcpf1_delta.tsv", f"{prefix}_guides_type.tsv"}
    groups = spy.groups[0]
    (how, family, score, cands, K, got), = seen
    assert family == gr.ABSOLUTE and K == 25 and cands == () and score is not None
    want_scores = np.asarray(scoring.deepcpf1(reports.group_kmers(groups), True), dtype=np.float64)
    assert score.tobytes() == want_scores.tobytes()
    panel = _Panel(groups, how["samples"], how["is_ref"])
    refs.results_equal(got, refs.plain_effects(panel, how["order"], refs.ABSOLUTE, score, (), 25))
    assert len(got.chosen) == 25 or len(got.chosen) == int((got.pos_ref[got.position == np.arange(groups.n_groups)] != gr.FX_NONE).sum())


# ----------------------------------------------------------------------------------------------------- the ValueError cases
def test_the_stage_that_cannot_run_is_a_value_error_before_any_file(tmp_path, monkeypatch):
    fx = ur.fixture("unphased")
    fa, bed, vcf = ur.write_files(fx, tmp_path / "in")
    def run(out, **kw):
        kw = dict(dict(cfd_tables=ur.CFD, graphical_reports=True, haplotype_table=True), **kw)
        return pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / out), **kw)
    with pytest.raises(ValueError, match="graphical_reports.*unphased_effects"):   # without the switch: as before, and the text names it
        run("a")
    with pytest.raises(ValueError, match="graphical_reports.*objects"):
        run("b", unphased_effects=True, unphased_report="objects")
    with pytest.raises(ValueError, match="graphical_reports.*host engine"):
        run("c", unphased_effects=True, unphased_engine="host")
    monkeypatch.setenv("HAWK_UNPHASED_ENGINE", "host")
    with pytest.raises(ValueError, match="graphical_reports.*host engine"):
        run("d", unphased_effects=True)
    monkeypatch.delenv("HAWK_UNPHASED_ENGINE")
    monkeypatch.setenv("HAWK_UNPHASED_REPORT", "objects")
    with pytest.raises(ValueError, match="graphical_reports.*objects"):
        run("e", unphased_effects=True, candidate_guides=[f"{fx['contig']}:{fx['bed_start'] + 5}:+"], graphical_reports=False)
    monkeypatch.delenv("HAWK_UNPHASED_REPORT")
    spy = _spy(monkeypatch, fail=_lib.HawkStatusError(_lib.HAWK_E_UNSUPPORTED, "hawk_resolve_groups"))
    with pytest.raises(ValueError, match=r"graphical_reports.*hawk_resolve_groups.*status -7"):
        run("f", unphased_effects=True)
    assert spy.groups == [None] and spy.guides == 0   # no retreat to the object route
    for out in "abcdef":
        assert _files_of(str(tmp_path / out)) == [], out


def test_a_recordless_interval_takes_the_variant_free_route(tmp_path, monkeypatch):
    """an unphased VCF whose one record lies behind the interval: report and figures of the run without a VCF, byte for byte"""
    fx = ur.fixture("unphased")
    fa, bed, _ = ur.write_files(fx, tmp_path / "in")
    contig_seq = "N" * (fx["startp"] - 1) + fx["region_seq"] + "ACGT" * 10
    pos = fx["startp"] + len(fx["region_seq"]) + 8
    base = contig_seq[pos - 1]
    vcf = str(tmp_path / "in" / "far.vcf")
    readers.write_vcf(vcf, fx["contig"], fx["samples"], [[fx["contig"], str(pos), ".", base, "A" if base != "A" else "C", ".", "PASS", "AF=0.5", "GT"]
                                                         + ["0/1"] * len(fx["samples"])], False)
    spy = _spy(monkeypatch)
    kw = dict(cfd_tables=ur.CFD, graphical_reports=True)
    f_with, f_none = {}, {}
    (a,) = pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "with"), unphased_effects=True, figures=f_with,
                                 **kw).values()
    (b,) = pipeline.search_files(fa, bed, [], fx["pam"], fx["guidelen"], fx["right"], str(tmp_path / "none"), figures=f_none, **kw).values()
    assert spy.groups == [] and spy.guides == 0
    assert open(a, "rb").read() == open(b, "rb").read() and open(a).read().count("\n") > 1
    (ma,), (mb,) = f_with.values(), f_none.values()
    assert [os.path.basename(p) for p in ma] == [os.path.basename(p) for p in mb] and len(ma) == 2
    for p, q in zip(ma, mb):
        assert open(p, "rb").read() == open(q, "rb").read()
