"""hawk_table_collapse_ex against a dictionary grouping of the table's own rows (tests/collapse_refs.py), array for array: the
number of groups, the row permutation, the CSR offsets, the G/C counts and the representative columns of the export - under the
sort path, the forced hash-table path and HAWK_COLLAPSE_EXACT=1, which must also agree with one another.  The cases sit on the
seams the builders prove on the CPU (tests/test_collapse_refs.py): one key field at a time, a flank base in and just outside the
compared slice on either strand, position-map spans at the steps of the sort key, thousands of different rows under one start,
the template path of a cluster-search table, and the hash table's memory of its last size."""
import numpy as np
import pytest

import collapse_refs as cr
from crisprhawk_hip import _lib
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

MODES = (("sort", "0"), ("hash", "0"), ("sort", "1"))  # HAWK_COLLAPSE_MODE, HAWK_COLLAPSE_EXACT
ARRAYS = ("perm", "off", "gc_num", "gc_den", "rep_row", "pos", "strand", "start", "stop", "flags", "win", "member_hap")


def _snap(tab):
    g = tab.export_groups()
    return dict(n=tab.n_groups, perm=tab.group_perm.astype(np.int64), off=np.asarray(tab.group_off).astype(np.int64),
                gc_num=tab.gc_num.copy(), gc_den=tab.gc_den.copy(), rep_row=np.array(g.rep_row).astype(np.int64), pos=np.array(g.pos),
                strand=np.array(g.strand), start=np.array(g.start), stop=np.array(g.stop), flags=np.array(g.flags),
                cfdon=np.array(g.cfdon), win=np.array(g.win), member_hap=np.array(g.member_hap))


def _collapse_modes(tab, flanks, monkeypatch, modes=MODES):
    """{flank: {mode: arrays}} of a device-resident table"""
    out = {}
    for flank in flanks:
        out[flank] = {}
        for mode, exact in modes:
            monkeypatch.setenv("HAWK_COLLAPSE_MODE", mode)
            monkeypatch.setenv("HAWK_COLLAPSE_EXACT", exact)
            tab.collapse(flank=flank)
            assert tab.collapse_flank == flank
            out[flank][(mode, exact)] = _snap(tab)
    return out


def _against_reference(tab, isref_row, snaps):
    """`tab` downloaded: every snapshot against the reference grouping of the table's rows, and the modes against each other"""
    wins = tab.windows()
    counts = {}
    for flank, by_mode in snaps.items():
        groups, gc = cr.group_rows(tab.start, tab.stop, tab.strand, isref_row, wins, tab.guidelen, tab.pamlen, tab.right, flank)
        counts[flank] = len(groups)
        first = None
        for mode, s in by_mode.items():
            assert s["n"] == len(groups), (flank, mode, s["n"], len(groups))
            assert sorted(s["perm"].tolist()) == list(range(tab.n_rows))
            perm, off, gc_num, gc_den = cr.reference_arrays(groups, gc, s["perm"], s["off"])
            assert np.array_equal(s["perm"], perm), (flank, mode, "members")
            assert np.array_equal(s["off"], off), (flank, mode, "offsets")
            assert np.array_equal(s["gc_num"], gc_num) and np.array_equal(s["gc_den"], gc_den), (flank, mode, "gc")
            heads = s["perm"][s["off"][:-1]]
            assert np.array_equal(s["rep_row"], heads), (flank, mode, "rep_row")
            for col in ("pos", "strand", "start", "stop", "flags"):
                assert np.array_equal(s[col], getattr(tab, col)[heads]), (flank, mode, col)
            assert np.array_equal(s["cfdon"], tab.cfdon[heads], equal_nan=True)
            assert np.array_equal(s["win"], tab.win[:, heads]), (flank, mode, "win")
            assert np.array_equal(s["member_hap"], tab.hap[s["perm"]]), (flank, mode, "member_hap")
            if first is None:
                first = s
            for k in ARRAYS:
                assert np.array_equal(s[k], first[k]), (flank, mode, k, "the modes disagree")
    return counts


def _same_rows_as_oracle(case, tab):
    g, wins = case.rows()
    want = sorted(zip(g["hap"].tolist(), g["pos"].tolist(), g["strand"].tolist(), g["start"].tolist(), g["stop"].tolist(), wins))
    got = sorted(zip(tab.hap.tolist(), tab.pos.tolist(), tab.strand.tolist(), tab.start.tolist(), tab.stop.tolist(), tab.windows()))
    assert got == want, f"{case.name}: the device table is not the table the seam was proven on"


def _run(case, monkeypatch, modes=MODES, ds=None):
    bits, bitsrc, _, _ = ora.pam_encode(case.pam)
    own = ds is None
    ds = case.device_set() if own else ds
    try:
        tab = ds.search(bits, bitsrc, case.pamlen, case.guidelen, case.right, download=False)
        snaps = _collapse_modes(tab, case.flanks, monkeypatch, modes)
        tab.download()
        _same_rows_as_oracle(case, tab)
        return _against_reference(tab, np.asarray(case.is_ref)[tab.hap], snaps), snaps
    finally:
        if own:
            ds.close()


# ---- A: key fields one at a time ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cr.CASES_A)))
def test_key_fields_one_at_a_time(i, monkeypatch):
    case = cr.CASES_A[i]()
    counts, _ = _run(case, monkeypatch)
    assert counts[(0, 0)] == len(case.reference()[0])


# ---- B: flanks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(8))
def test_flanks_against_the_reference(i, monkeypatch):
    case = cr.flank_cases()[i]
    counts, _ = _run(case, monkeypatch)
    for flank in case.flanks:  # the split counts the builder proved guide by guide
        assert counts[flank] == len(case.reference(flank)[0])
    assert counts[(10, 10)] > counts[(4, 3)] >= counts[(0, 0)]


def test_flank_beyond_the_stored_pad_is_refused():
    case = cr.case_stop_only(0)
    bits, bitsrc, _, _ = ora.pam_encode(case.pam)
    ds = case.device_set()
    tab = ds.search(bits, bitsrc, case.pamlen, case.guidelen, case.right, download=False)
    for flank in ((11, 0), (0, 11), (11, 11)):
        with pytest.raises(_lib.HawkStatusError) as e:
            tab.collapse(flank=flank)
        assert e.value.status == _lib.HAWK_E_UNSUPPORTED
    tab.collapse(flank=(10, 10))
    assert tab.n_groups == len(case.reference((10, 10))[0])
    tab.close()
    ds.close()


# ---- C: key width ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", cr.SPANS, ids=[hex(s) for s in cr.SPANS])
def test_key_width_steps(span, monkeypatch):
    # (at 0xffffffff the forced hash mode has no table to offer and must answer through the sort)
    case = cr.case_span(span)
    counts, _ = _run(case, monkeypatch)
    assert counts[(0, 0)] == len(case.reference()[0])


def test_span_beyond_the_key_is_refused():
    case = cr.case_span(0x100000000)
    bits, bitsrc, _, _ = ora.pam_encode(case.pam)
    ds = case.device_set()
    tab = ds.search(bits, bitsrc, case.pamlen, case.guidelen, case.right, download=False)
    with pytest.raises(_lib.HawkStatusError) as e:
        tab.collapse()
    assert e.value.status == _lib.HAWK_E_UNSUPPORTED
    tab.download()
    _same_rows_as_oracle(case, tab)
    ds.close()


# ---- D: many distinct rows under one (start, strand) ------------------------------------------------------------------------
def test_many_distinct_rows_under_one_start(monkeypatch):
    """8192 different rows at each of four (start, strand) with 24 hash bits in the sort key: about two colliding pairs per start
    under ANY seed, so the four seeds of the usual path are used up and the exact path has to group rows that share a key.
    Before its rows were sorted by identity below the key this came back as HAWK_E_UNSUPPORTED."""
    # (No counter or timing field tells which path answered.  That the usual path's seeds are used up shows in the parent of this
    # change, which returned the error for exactly this table; likewise nothing but the result arrays shows that forced hash mode
    # fell through to the sort at span 0xffffffff and in the "all" step of the table-memory case.)
    case = cr.case_many_distinct()
    counts, _ = _run(case, monkeypatch)
    assert counts[(0, 0)] == len(case.rows()[0])


# ---- E: the template path ------------------------------------------------------------------------------------------------------
def _view_case(reg, pam_s, guidelen, right, flanks, monkeypatch, prove=None, want_r0_off_block=False):
    """The set of `reg` searched from its planes (table a) and through the plan's view per distinct cluster (table c, v_path 2,
    grouped by collapse_by_templates): both against the reference on their own rows under every mode, and c's groups against a's,
    in order, rows mapped through (haplotype, strand, position).  `prove(st, info, a, is_ref_row_a, reference counts)` holds the
    case to its seam.  The seam "REF's row count is no multiple of 256" is asserted where a case asks for it
    (`want_r0_off_block`: test_template_path_clusters_without_rows) and in the case without a prove step
    (test_template_path_dense_region).  -> {flank: groups}"""
    from crisprhawk_hip.workload import expand_on_device
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    bits, bitsrc, _, _ = ora.pam_encode(pam_s)
    ds, info, _ms, _kept = expand_on_device(reg, len(pam_s), keep_plan=True)
    try:
        a = ds.search(bits, bitsrc, len(pam_s), guidelen, right, download=False)
        sa = _collapse_modes(a, flanks, monkeypatch)
        a.download()
        view = ds.plan.view()
        st = ds.plan.cluster_stats()
        c = view.search(bits, bitsrc, len(pam_s), guidelen, right, download=False)
        assert c.timing["v_path"] == 2 and c.layout() == "rows" and st["usable"] and st["status"] == 0, st
        sc = _collapse_modes(c, flanks, monkeypatch)
        c.download()
        is_ref = np.asarray(ds.is_ref, dtype=bool)
        na = _against_reference(a, is_ref[a.hap], sa)
        nc = _against_reference(c, is_ref[c.hap], sc)
        assert na == nc and c.n_rows == a.n_rows > 0
        r0 = int(is_ref[c.hap].sum())
        assert 0 < r0 < c.n_rows and is_ref[c.hap[:r0]].all()  # REF's rows lead the table
        if prove is None or want_r0_off_block:
            assert r0 % 256 != 0  # ... and end inside a 256-row block of k_cc_refgid / k_cc_mini

        def parts(t, s):
            ident = list(zip(t.hap.tolist(), t.strand.tolist(), t.pos.tolist()))
            return [frozenset(ident[r] for r in s["perm"][x:y]) for x, y in zip(s["off"][:-1], s["off"][1:])]
        for flank in flanks:
            assert parts(a, sa[flank][MODES[0]]) == parts(c, sc[flank][MODES[0]]), flank  # the same groups in the same order
        if prove is not None:
            prove(st, info, a, is_ref[a.hap])
        return nc
    finally:
        ds.plan.close()
        ds.close()


def _host_instances(info):
    """inst_uid's order restated: per searched non-REF row its clusters in position order (True), then the closing instance, which
    belongs to no cluster (False = CL_NONE).  Isolated SNVs only: every carried variant is a cluster of its own."""
    out = []
    for inf in info:
        k = len(inf.variant_idx)
        if k:
            out += [True] * k + [False]
    return out


def _nonref_cover(reg, a, isref_row, index):
    """non-REF rows of the plane table whose guide spans region index `index` (SNV-only panels: the position map is the identity)"""
    g = reg.startp + index
    return int(((~isref_row) & (a.start <= g) & (g < a.start + a.guidelen + a.pamlen)).sum())


def test_template_path_dense_region(monkeypatch):
    from crisprhawk_hip import synth
    # common variants every ~60 bases: most guides have a variant within ten bases of their core on some copy
    reg = synth.make_region(7511, "chrC", 40_000, 1_000, 38_000)
    synth.add_phased_variants(reg, 7512, 600, 6, af_min=0.3, af_max=0.8)
    n = _view_case(reg, "NGG", 20, False, ((0, 0), (4, 3), (10, 10)), monkeypatch)
    assert n[(10, 10)] >= n[(4, 3)] > n[(0, 0)]


def test_template_path_clusters_without_rows(monkeypatch):
    """distinct clusters with zero kept rows first, last, and two in a row between full ones (k_cc_ucnt's zero counts under the scan
    and both binary searches: equal offsets side by side)"""
    from test_gpu_clusters import Panel
    p = Panel(9801, 60_000, 2)
    sites = cr.panel_zero_rows(p)
    reg = p.region()

    def prove(st, info, a, isref_row):
        assert st["distinct"] == len(sites) == 8 and [k for _, k in sites] == list("ZFFZZFFZ")
        assert [i for i, _ in sites] == sorted(i for i, _ in sites)  # cluster numbers of single variants follow the positions
        for i, kind in sites:
            n = _nonref_cover(reg, a, isref_row, i)
            assert (n == 0) == (kind == "Z"), (i, kind, n)
    _view_case(reg, "NGG", 20, False, ((0, 0), (4, 3)), monkeypatch, prove, want_r0_off_block=True)


@pytest.mark.parametrize("n_uniq", [255, 256, 257, 1023, 1024, 1025])
def test_template_path_distinct_cluster_counts(n_uniq, monkeypatch):
    from test_gpu_clusters import Panel
    p = Panel(9810 + n_uniq, 150 * n_uniq + 1500, 2)
    cr.panel_distinct(p, n_uniq)
    reg = p.region()

    def prove(st, info, a, isref_row):
        assert st["distinct"] == n_uniq, st
    _view_case(reg, "NGG", 20, False, ((0, 0),), monkeypatch, prove)


@pytest.mark.parametrize("per_col,none_at", [((62,), None), ((63,), None), ((64,), 64), ((64, 64), 64), ((254,), None), ((255,), None),
                                             ((256,), 256), ((64, 190), None)],
                         ids=["63", "64", "65", "130-wave-starts-on-none", "255", "256", "257", "256-two-rows"])
def test_template_path_instance_counts(per_col, none_at, monkeypatch):
    """instance counts at the wave (64) and workgroup (256) seams of k_cs_gid; a wave whose FIRST instance is a row's closing
    instance (CL_NONE), with and without instances behind it"""
    from test_gpu_clusters import Panel
    total = sum(per_col) + len(per_col)
    p = Panel(9830 + total, 150 * sum(per_col) + 1500, 2)
    cr.panel_isolated(p, per_col)
    reg = p.region()

    def prove(st, info, a, isref_row):
        inst = _host_instances(info)
        assert st["instances"] == len(inst) == total and st["distinct"] == sum(per_col), (st, total)
        if none_at is not None:
            assert none_at % 64 == 0 and inst[none_at] is False
            if per_col == (64, 64):
                assert inst[none_at + 1] is True  # cluster instances follow in the same wave
    _view_case(reg, "NGG", 20, False, ((0, 0),), monkeypatch, prove)


def test_template_path_reservation_longer_than_live_rows(monkeypatch):
    from test_gpu_clusters import Panel
    p = Panel(9802, 30_000, 6)
    sites = cr.panel_reservation(p, 12)
    reg = p.region()

    def prove(st, info, a, isref_row):
        # every cluster is carried by one copy alone, so the live template rows are the table's non-REF rows
        live = int((~isref_row).sum())
        assert st["distinct"] == len(sites) and st["template_slots"] > live > 0, (st, live)
    _view_case(reg, "NGG", 20, False, ((0, 0), (4, 3)), monkeypatch, prove)


@pytest.mark.parametrize("pam_s,guidelen,right,places", [
    ("NGG", 20, False, (("5", 4), ("5", 5), ("3", 3), ("3", 4))), ("TTTV", 20, True, (("5", 4), ("5", 5), ("3", 3), ("3", 4))),
    ("NGG", 41, False, (("5", 10), ("3", 10), ("5", 4), ("3", 4))), ("TTTV", 40, True, (("5", 10), ("3", 10), ("5", 4), ("3", 4)))],
    ids=["NGG-20", "TTTV-20", "NGG-41-core44", "TTTV-40-core44"])
def test_flanks_on_the_view_path(pam_s, guidelen, right, places, monkeypatch):
    """The flank seams of case B through the plan: a second SNV d bases outside the core on the guide's 5' or 3' side, on either
    strand, splits the four copies' group iff the flank on that side reaches it - on the plane table and on the view's."""
    from test_gpu_clusters import Panel
    p = Panel(9850 + guidelen, 40_000, 2)
    guides = cr.panel_flanks(p, pam_s, guidelen, right, places)
    reg = p.region()

    def prove(st, info, a, isref_row):
        wins = a.windows()
        for flank in cr.FLANKS:
            groups, _ = cr.group_rows(a.start, a.stop, a.strand, isref_row, wins, guidelen, len(pam_s), right, flank)
            for c0, strand, side, d in guides:
                mine = [v for k, v in groups.items() if k[0] == reg.startp + c0 and k[2] == strand and not k[3]]
                assert sum(len(v) for v in mine) == 4, (c0, strand, "four non-REF copies of the planted guide")
                reach = flank[0] if side == "5" else flank[1]
                assert len(mine) == (2 if d <= reach else 1), (c0, strand, side, d, flank, len(mine))
    _view_case(reg, pam_s, guidelen, right, cr.FLANKS, monkeypatch, prove)


# ---- F: the memory of the hash table's size -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["hash", None])
def test_table_size_memory_few_all_few(mode, monkeypatch):
    """`last_groups` of the set sizes the next call's hash table: few groups, then every row its own group (rows find no slot in a
    table sized for six groups: the call must answer through the sort), then few again - each against the reference."""
    from crisprhawk_hip.hapset import HostHaplotype, PosSegments, segments_from_posmap
    few, every = cr.case_table_memory()
    ds = few.device_set()
    want_groups = []
    for case in (few, every, few):
        ds.set_meta([HostHaplotype(seq, PosSegments(*segments_from_posmap(pm), len(seq)), r, sc)
                     for seq, pm, r, sc in zip(case.seqs, case.posmaps, case.is_ref, case.scan)])
        modes = ((mode, "0"),) if mode else ((None, None),)
        bits, bitsrc, _, _ = ora.pam_encode(case.pam)
        tab = ds.search(bits, bitsrc, case.pamlen, case.guidelen, case.right, download=False)
        if mode:
            monkeypatch.setenv("HAWK_COLLAPSE_MODE", mode)
        else:
            monkeypatch.delenv("HAWK_COLLAPSE_MODE", raising=False)
        monkeypatch.setenv("HAWK_COLLAPSE_EXACT", "0")
        tab.collapse()
        snaps = {(0, 0): {modes[0]: _snap(tab)}}
        tab.download()
        _same_rows_as_oracle(case, tab)
        want_groups.append(_against_reference(tab, np.asarray(case.is_ref)[tab.hap], snaps)[(0, 0)])
    assert want_groups[0] == want_groups[2] == 6 and want_groups[1] > 4096
    ds.close()
