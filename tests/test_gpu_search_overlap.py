"""The cluster search of a plan view runs REF's plane passes on the context's side stream, beside the cluster passes on the main
stream (search_count / search_emit in hawk_api_search.hip: a fork behind the misc memset, a join in front of the offset scan; a
fork behind the scan, a join in front of whatever reads the status block or the table).  A missing or misplaced join shows where one
side is much longer than the other, where an attempt is repeated inside one call, and where the next call follows at once - the
shapes below.  Every table is compared with the plane search of the materialised set and with the ORACLE's rows and totals, and
every search asserts that it ran per cluster (timing v_path 2).  Each case prints the row counts of both sides (-s)."""
import math

import numpy as np
import pytest

from crisprhawk_hip import _lib, synth
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora
from test_gpu_clusters import BASES, Panel, _same_rows, _view_check
from test_gpu_vsearch import _oracle_rows, _table_rows
from util import oracle_haplotypes

pytestmark = pytest.mark.gpu

REF = ("REF",)


@pytest.fixture(autouse=True)
def _cluster_path_for_small_panels(monkeypatch):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_ROWS0", "HAWK_CLUSTER_MAX_SLOTS"):
        monkeypatch.delenv(k, raising=False)


# ---- panels and the comparison -------------------------------------------------------------------------------------------
def _panel(seed, length, n_samples, edit=None):
    """test_gpu_clusters.Panel, its contig rewritten by `edit(bases: list, base: int)` first (`base`: contig index of region index 0)"""
    p = Panel(seed, length, n_samples)
    if edit is not None:
        s = list(p.reg.contig_seq)
        edit(s, p.reg.startp - 1)
        p.reg.contig_seq = "".join(s)
        p.seq = p.reg.sequence.upper()
    return p


def _scrub(s, lo, hi):
    """no GG and no CC in s[lo:hi] (nor across its edges): NGG has no hit there on either strand"""
    for i in range(max(lo, 1), min(hi + 1, len(s))):
        if s[i] in "GC" and s[i] == s[i - 1]:
            s[i] = "A" if s[i] == "G" else "T"


def _oracle_rows_scanned_as(reg, pam_s, guidelen, scan_pamlen):
    """test_gpu_vsearch._oracle_rows (left PAM, no scores) for a PAM searched on a plan whose scan ranges were laid out for
    another PAM length: the rows' scan bounds come from the plan, not from the search"""
    fx = dict(region_seq=reg.sequence, startp=reg.startp, samples=reg.samples,
              variants=[[v.pos, v.ref, v.alt, v.af, ["".join(str(int(x)) for x in row) for row in v.gt]] for v in reg.variants])
    haps = oracle_haplotypes(fx)
    scan = [ora.scan_bounds(h["posmap"], reg.startp, reg.stopp, scan_pamlen) for h in haps]
    hs = ora.HapSet([h["seq"] for h in haps], [h["posmap"] for h in haps], [h["samples"] == ["REF"] for h in haps], scan)
    want = ora.search(hs, pam_s, guidelen, False)
    g, wins = want.guides, want.windows
    lab = [tuple(sorted(h["samples"])) for h in haps]
    rows = sorted((lab[int(g["hap"][i])], int(g["start"][i]), int(g["stop"][i]), int(g["strand"][i]), int(g["pos"][i]), wins[i], None)
                  for i in range(len(g)))
    return rows, want.n_candidates, want.n_hits


def _sides(want, name):
    """rows of REF (the side stream's) and of every other haplotype (the main stream's) in the oracle's table"""
    n_ref = sum(1 for r in want if r[0] == REF)
    print(f"{name}: REF rows {n_ref}, cluster rows {len(want) - n_ref}")
    return n_ref, len(want) - n_ref


class _Both:
    """A panel's materialised set and the view of its plan, side by side; the oracle's rows once per PAM."""

    def __init__(self, reg, pamlen=3):
        self.reg, self.pamlen = reg, pamlen
        self.ds, self.info, _ms, self.kept = expand_on_device(reg, pamlen, keep_plan=True)
        self.view = self.ds.plan.view()
        assert self.ds.plan.cluster_stats()["usable"]
        self._want = {}

    def args(self, pam_s, guidelen=20):
        bits, bitsrc, _, _ = ora.pam_encode(pam_s)
        mm, pt = synth.cfd_tables() if len(pam_s) >= 2 else (None, None)
        return bits, bitsrc, len(pam_s), guidelen, False, mm, pt

    def want(self, pam_s):
        """(the oracle scores strictly: a reference with an N is compared without the scores)"""
        if pam_s not in self._want:
            a = self.args(pam_s)
            mm, pt = (a[5], a[6]) if self.scored(pam_s) else (None, None)
            self._want[pam_s] = (_oracle_rows(self.reg, pam_s, 20, False, mm, pt) if len(pam_s) == self.pamlen else
                                 _oracle_rows_scanned_as(self.reg, pam_s, 20, self.pamlen))
        return self._want[pam_s]

    def scored(self, pam_s):
        return len(pam_s) >= 2 and "N" not in self.reg.sequence.upper()

    def planes(self, pam_s, **kw):
        return self.ds.search(*self.args(pam_s), **kw)

    def search(self, pam_s, **kw):
        t = self.view.search(*self.args(pam_s), **kw)
        assert t.timing["v_path"] == 2
        return t

    def check(self, pam_s, t, na_on_ambiguous=False):
        """a downloaded table of the view against the plane search and the oracle"""
        rows, n_cand, n_hits = self.want(pam_s)
        _same_rows(self.planes(pam_s, cfd_na_on_ambiguous=na_on_ambiguous), t)
        assert (t.n_rows, t.n_candidates, t.n_hits) == (len(rows), n_cand, n_hits)
        assert _table_rows(t, self.info, self.kept, self.scored(pam_s)) == rows

    def close(self):
        self.ds.plan.close()
        self.ds.close()


def _identical(t, want):
    assert (t.n_rows, t.n_candidates, t.n_hits) == (want.n_rows, want.n_candidates, want.n_hits)
    for c in ("hap", "pos", "strand", "start", "stop", "flags", "win"):
        assert np.array_equal(getattr(t, c), getattr(want, c)), c
    assert np.array_equal(t.cfdon, want.cfdon, equal_nan=True)


def _few_variants_panel(seed=9101, length=6_000, n_samples=3):
    """a dozen SNVs and two indels on three samples: REF and cluster rows of the same order"""
    p = _panel(seed, length, n_samples)
    for k in range(12):
        p.snv(1_300 + 350 * k, {k % (2 * n_samples), (k + 3) % (2 * n_samples)})
    p.deletion(1_475, 3, {1, 4})
    p.insertion(3_925, 2, {0, 5})
    return p.region()


# ---- 1: the side stream outlasts the main one -------------------------------------------------------------------------------
def test_side_outlasts_main_and_the_next_call_follows_at_once():
    """60 kb of REF (thousands of rows through k_emit_list / k_search_emit / k_rows_pack) against two private SNVs (a handful of rows
    through k_cs_emit_rows): the emit join is what the main stream waits for.  collapse() and export_groups() follow the search
    without a download in between - they read REF's staged rows and the packed table on the main stream."""
    p = _panel(9001, 60_000, 2)
    p.snv(20_000, {0})
    p.snv(41_000, {3})
    b = _Both(p.region())
    try:
        n_ref, n_cl = _sides(b.want("NGG")[0], "side outlasts main")
        assert n_cl > 0 and n_ref > 50 * n_cl and n_ref > 2_000
        t = b.search("NGG", download=False)
        t.collapse(download_perm=False)
        g = t.export_groups()
        t.download()
        b.check("NGG", t)
        a = b.planes("NGG", download=False)
        a.collapse(download_perm=False)
        ga = a.export_groups()
        a.close()
        assert t.n_groups == a.n_groups
        for col in ("pos", "strand", "start", "stop", "flags", "member_hap", "member_off", "gc_num", "gc_den"):
            assert np.array_equal(getattr(g, col), getattr(ga, col)), col
        assert np.array_equal(g.win, ga.win) and np.array_equal(g.cfdon, ga.cfdon, equal_nan=True)
    finally:
        b.close()


# ---- 2: the main stream outlasts the side one -------------------------------------------------------------------------------
def _crowded_panel():
    """3 kb, 64 samples: an SNV every 70 nt on ALL 128 copies.  Identical copies would collapse onto one row, so half way between two
    of them copy c also carries an SNV wherever bit (slot % 8) of c + 1 is set: 128 different rows, each with rows of its own"""
    p = _panel(9002, 3_000, 64)
    every = set(range(128))
    for k in range(40):
        p.snv(120 + 70 * k, every)
        p.snv(155 + 70 * k, {c for c in range(128) if (c + 1) >> (k % 8) & 1}, shift=2)
    return p.region()


def test_main_outlasts_side():
    reg = _crowded_panel()
    a = synth.cfd_tables()
    n_ref, n_cl = _sides(_oracle_rows(reg, "NGG", 20, False, *a)[0], "main outlasts side")
    assert n_ref > 0 and n_cl > 50 * n_ref
    _view_check(reg, "NGG", 20, False, 2, words=False)


# ---- 3: the three paths of the table reservation on one view ----------------------------------------------------------------
def test_first_speculative_and_refused_emit_on_one_view():
    """first search: the table is reserved behind the read-back, one emit; second: the emit is speculative; `N` (every position of
    both strands a hit): the speculative emit - both of its streams - is refused for capacity and runs again; NGG after it fits"""
    b = _Both(_few_variants_panel())
    try:
        _sides(b.want("NGG")[0], "reservation NGG")
        _sides(b.want("N")[0], "reservation N")
        assert len(b.want("N")[0]) > 4 * len(b.want("NGG")[0])
        # REF's rows alone outnumber the table NGG reserved, by more than the 255 rows a launch is rounded up by: the packing of REF's
        # staged rows (k_rows_pack) has to refuse too, not only k_cs_emit_rows
        assert sum(1 for r in b.want("N")[0] if r[0] == REF) > len(b.want("NGG")[0]) + 256
        first = b.search("NGG")
        b.check("NGG", first)
        second = b.search("NGG")
        _identical(second, first)
        b.check("NGG", second)
        wide = b.search("N")
        assert wide.n_rows > first.n_rows
        b.check("N", wide)
        again = b.search("NGG")
        _identical(again, first)
        b.check("NGG", again)
    finally:
        b.close()


# ---- 4: two attempts in one call --------------------------------------------------------------------------------------------
def test_template_retry_forks_and_joins_twice(monkeypatch):
    b = _Both(_few_variants_panel())
    try:
        n_ref, n_cl = _sides(b.want("NGG")[0], "template retry")
        assert n_cl > 1  # more template rows than the one reserved
        monkeypatch.setenv("HAWK_CLUSTER_ROWS0", "1")
        t = b.search("NGG")
        b.check("NGG", t)
        monkeypatch.delenv("HAWK_CLUSTER_ROWS0")
        t2 = b.search("NGG")
        _identical(t2, t)
        b.check("NGG", t2)
    finally:
        b.close()


# ---- 5: the benchmark's step, back to back ----------------------------------------------------------------------------------
def test_rebuild_and_search_back_to_back():
    b = _Both(_few_variants_panel(seed=9105))
    try:
        _sides(b.want("NGG")[0], "repeat")
        tabs = []
        for it in range(10):
            b.ds.plan.rebuild_dictionary()
            t = b.search("NGG", download=False)
            if it == 0:
                t.download()  # (the first iteration's rows: a later search overwrites the table)
            elif it < 9:
                t.close()
            tabs.append(t)
        last = tabs[-1].download()
        _identical(last, tabs[0])
        b.check("NGG", last)
    finally:
        b.close()


# ---- 6: one side writes nothing ---------------------------------------------------------------------------------------------
def _no_ref_rows_panel():
    p = _panel(9006, 4_000, 2, edit=lambda s, base: _scrub(s, 0, len(s)))
    made, i = 0, 1_200
    while made < 4:
        if p.seq[i] == "G" and p.seq[i + 1] in "AT":
            p.snv(i + 1, {made}, shift=(2 - BASES.index(p.seq[i + 1])) % 4)
            made, i = made + 1, i + 500
        i += 1
    return p.region()


def test_no_ref_rows():
    """no GG and no CC anywhere in the contig: REF has no NGG hit on either strand; four SNVs turn a G[AT] into GG"""
    reg = _no_ref_rows_panel()
    n_ref, n_cl = _sides(_oracle_rows(reg, "NGG", 20, False, *synth.cfd_tables())[0], "no REF rows")
    assert n_ref == 0 and n_cl > 0
    _view_check(reg, "NGG", 20, False, 2, words=False)


def _no_cluster_rows_panel():
    sites = (1_500, 2_600)

    def edit(s, base):
        for i in sites:
            _scrub(s, base + i - 150, base + i + 150)
            s[base + i] = "A"
    p = _panel(9007, 4_000, 2, edit=edit)
    for k, i in enumerate(sites):
        p.snv(i, {k, 3 - k}, shift=3)
    return p.region()


def test_no_cluster_rows():
    """the SNVs (A -> T) lie in the middle of 300 nt without GG / CC: no window of a guide reaches them, the cluster side writes nothing"""
    reg = _no_cluster_rows_panel()
    n_ref, n_cl = _sides(_oracle_rows(reg, "NGG", 20, False, *synth.cfd_tables())[0], "no cluster rows")
    assert n_ref > 0 and n_cl == 0
    _view_check(reg, "NGG", 20, False, 2, words=False)


# ---- 7: a status raised on the side stream ----------------------------------------------------------------------------------
def _n_under_a_guide_panel():
    at = []

    def edit(s, base):
        i = next(j for j in range(base + 2_000, base + 2_400) if s[j + 1] == "G" and s[j + 2] == "G")
        s[i - 5] = "N"
        at.append(i - 5 - base)
    p = _panel(9008, 4_000, 2, edit=edit)
    assert p.seq[at[0]] == "N"
    p.snv(1_300, {0})
    p.snv(3_300, {2, 3})
    return p.region()


def test_cfd_error_of_refs_pass_reaches_the_caller():
    """an N five bases in front of one of REF's NGG hits, far from every variant: only REF's plane pass looks it up.  Strict scoring
    refuses - on a fresh view (no table reserved) and behind a successful search (speculative emit) - and the view stays usable."""
    b = _Both(_n_under_a_guide_panel())
    try:
        _sides(b.want("NGG")[0], "status travels")
        for _round in range(2):
            with pytest.raises(_lib.HawkStatusError) as e:
                b.search("NGG", cfd_na_on_ambiguous=False)
            assert e.value.status == _lib.HAWK_E_CFD
            t = b.search("NGG", cfd_na_on_ambiguous=True)
            assert np.isnan(t.cfdon).any()
            b.check("NGG", t, na_on_ambiguous=True)
    finally:
        b.close()


# ---- 8: the timing block keeps its meanings ---------------------------------------------------------------------------------
@pytest.mark.parametrize("speculative", [False, True])
def test_timing_brackets(speculative):
    b = _Both(_few_variants_panel(seed=9108))
    try:
        t = b.search("NGG")
        if speculative:
            t = b.search("NGG")
        assert t.n_rows > 0
        tm = t.timing
        print({k: round(tm[k], 4) for k in ("count_ms", "offsets_ms", "emit_ms", "emit_list_ms", "total_ms", "v_count_ms", "v_templates_ms",
                                            "v_emit_ms", "v_emit_rows_ms")})
        for k in ("count_ms", "offsets_ms", "emit_ms", "emit_list_ms", "total_ms", "v_count_ms", "v_templates_ms", "v_emit_rows_ms"):
            assert math.isfinite(tm[k]) and tm[k] > 0, k
        assert tm["v_emit_rows_ms"] <= tm["emit_ms"]
        assert tm["v_templates_ms"] <= tm["v_count_ms"] <= tm["count_ms"]
    finally:
        b.close()
