"""The per-cluster search of a plan view (hawk_csearch.hip; its dictionary: hawk_cldict.hip, xplan_build_dict in hawk_api_cldict.hip) at the limits it hard-codes:
the 44-base core and one-base / sixteen-base PAMs, the 64-position link between records, the 4096-record chain cap, the row-bound
classes of an instance, the seams of the cutting passes (wave, slice, chunk), the head launch and the bitmap read from HBM,
the default sharing and template-slot thresholds.  Every case compares the view's table with the ORACLE's rows (carrier
labels, coordinates, strand, padded window, CFDon) and the job totals, and asserts which path ran (timing v_path: 2 per distinct
cluster, 1 per dirty word).  Panels are placed by hand so that each limit is met at the offsets where an off-by-one would show."""
import os
import subprocess
import sys

import numpy as np
import pytest

from crisprhawk_hip import _lib, synth
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora
from test_gpu_vsearch import _canonical, _oracle_rows, _same_table, _table_rows, COLS

pytestmark = pytest.mark.gpu

HAWK_PAD = 10  # the padded window's flank (hawk_device.h)
BASES = "ACGT"


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_MIN_SHARE", "HAWK_CLUSTER_MAX_SLOTS", "HAWK_CLUSTER_WEAK_HASH"):
        monkeypatch.delenv(k, raising=False)


# ---- panels ------------------------------------------------------------------------------------------------------------
class Panel:
    """Hand-placed variant sites on a synthetic region: indices are 0-based into the region string (reg.sequence), carriers are
    chromosome-copy columns (2 * sample + copy)."""

    def __init__(self, seed, length, n_samples, flank=1000):
        self.reg = synth.make_region(seed, "chrL", length + 2 * flank, flank, flank + length - 201)
        self.seq = self.reg.sequence.upper()
        self.n_samples = n_samples
        self.sites = {}  # (index, ref, alt) -> set of columns

    def _add(self, i, ref, alt, cols):
        assert 0 < i and i + len(ref) < len(self.seq)
        self.sites.setdefault((i, ref, alt), set()).update(cols)
        return i + len(ref)  # the index behind the REF allele

    def snv(self, i, cols, shift=1):
        r = self.seq[i]
        return self._add(i, r, BASES[(BASES.index(r) + shift) % 4], cols)

    def deletion(self, i, k, cols):
        return self._add(i, self.seq[i:i + k + 1], self.seq[i], cols)

    def insertion(self, i, k, cols):
        return self._add(i, self.seq[i], self.seq[i] + "".join(BASES[(i + 3 * t) % 4] for t in range(k)), cols)

    def region(self):
        reg = self.reg
        reg.samples = [f"S{s:04d}" for s in range(self.n_samples)]
        out = []
        for (i, ref, alt), cols in sorted(self.sites.items()):
            gt = np.zeros((self.n_samples, 2), dtype=np.uint8)
            for c in cols:
                gt[c // 2, c % 2] = 1
            out.append(synth.VariantSite(reg.startp + i, ref, alt, float(gt.mean()), gt))
        reg.variants = out
        reg.gt_matrix = None
        return reg


def _cfd(reg, pam_s, right):
    # scored wherever the plane sweep scores it: a left PAM of two bases or more, a reference without N
    return (not right) and len(pam_s) >= 2 and "N" not in reg.sequence.upper()


def _host_clusters(reg, info):
    """the dictionary's instances counted on the host (test_gpu_vsearch.test_cluster_dictionary_against_a_host_count): a row's
    carried variants sorted by position, a new cluster wherever more than 64 reference bases separate one variant's end from the
    next one's start, + one closing instance per searched row; and the distinct variant tuples"""
    pos = np.array([v.pos for v in reg.variants], dtype=np.int64)
    end = pos + np.array([len(v.ref) for v in reg.variants], dtype=np.int64)
    inst, distinct = 0, set()
    for inf in info:
        idx = np.sort(np.asarray(inf.variant_idx, dtype=np.int64))
        if len(idx) == 0:
            continue  # REF
        brk = np.flatnonzero(pos[idx[1:]] - end[idx[:-1]] > 64) + 1
        for part in np.split(idx, brk):
            distinct.add(tuple(part.tolist()))
        inst += len(brk) + 2
    return inst, distinct


def _same_rows(a, c):
    assert (c.n_rows, c.n_candidates, c.n_hits) == (a.n_rows, a.n_candidates, a.n_hits)
    ca, cc = _canonical(a), _canonical(c)
    for k in COLS:
        assert np.array_equal(ca[k], cc[k]), k
    assert np.array_equal(ca["win"], cc["win"])
    assert np.array_equal(ca["cfdon"], cc["cfdon"], equal_nan=True)


def _view_check(reg, pam_s, guidelen, right, path, words=True, stats=None):
    """The default search of the plan's view takes `path`; its table, the per-word search's and the plane search's hold the
    oracle's rows and totals.  `stats(st, plan, info, kept)` sees the dictionary before the search.  -> cluster_stats()"""
    bits, bitsrc, _, _ = ora.pam_encode(pam_s)
    cfd = _cfd(reg, pam_s, right)
    mm, pt = synth.cfd_tables() if cfd else (None, None)
    ds, info, _ms, kept = expand_on_device(reg, len(pam_s), keep_plan=True)
    try:
        a = ds.search(bits, bitsrc, len(pam_s), guidelen, right, mm, pt)
        view = ds.plan.view()
        st = ds.plan.cluster_stats()
        if stats is not None:
            stats(st, ds.plan, info, kept)
        c = view.search(bits, bitsrc, len(pam_s), guidelen, right, mm, pt)
        assert c.timing["v_path"] == path, (c.timing["v_path"], st)
        assert st["usable"] == (path == 2), st
        tables = [c]
        if words and path == 2:
            os.environ["HAWK_VIEW_SEARCH"] = "words"
            try:
                b = view.search(bits, bitsrc, len(pam_s), guidelen, right, mm, pt)
            finally:
                del os.environ["HAWK_VIEW_SEARCH"]
            assert b.timing["v_path"] == 1
            tables.append(b)
        want, n_cand, n_hits = _oracle_rows(reg, pam_s, guidelen, right, mm, pt)
        for t in tables:
            _same_rows(a, t)
            assert (t.n_candidates, t.n_hits) == (n_cand, n_hits)
            assert _table_rows(t, info, kept, cfd) == want
        assert len(want) > 0
        return st
    finally:
        ds.plan.close()
        ds.close()


# ---- A: shapes at the length limit ---------------------------------------------------------------------------------------
def _indel_panel(seed):
    reg = synth.make_region(seed, "chrA", 30_000, 1_000, 27_000)
    synth.add_phased_variants(reg, seed + 1, 1_400, 6, frac_snv=0.5, frac_del=0.25, max_indel=8, af_min=0.2, af_max=0.8)
    return reg


@pytest.mark.parametrize("pam_s,guidelen,right", [("NRG", 41, False), ("TTTV", 40, True), ("NGNNNNNNNNNNNNGN", 28, False), ("N", 20, False)])
def test_view_shapes_at_the_length_limit(monkeypatch, pam_s, guidelen, right):
    # guide + PAM of 44 bases (the core limit the cluster classes hard-code), a 16-base PAM, a one-base PAM; SNVs, insertions and
    # deletions a few bases apart
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _indel_panel(9101)
    _same_table(reg, pam_s, guidelen, right, cfd=_cfd(reg, pam_s, right), oracle=True)


def test_view_refuses_beyond_the_length_limit(monkeypatch):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _indel_panel(9111)
    ds, _info, _ms, _kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        view = ds.plan.view()
        b3, r3, _, _ = ora.pam_encode("NGG")
        b16, r16, _, _ = ora.pam_encode("NGNNNNNNNNNNNNGN")
        for hs in (ds, view):
            # (a PAM is 4 bits per base in one 64-bit word each way: 17 bases cannot be encoded, so the 17-base case passes 16 bases'
            # codes with pamlen 17 - the length check has to refuse it before anything reads the codes)
            for bits, bitsrc, pamlen, guidelen in ((b3, r3, 3, 42), (b16, r16, 16, 29), (b16, r16, 17, 20)):
                with pytest.raises(_lib.HawkStatusError) as e:
                    hs.search(bits, bitsrc, pamlen, guidelen, False)
                assert e.value.status == _lib.HAWK_E_UNSUPPORTED, (pamlen, guidelen)
        # nothing is left behind: the next search on the same view runs and gives the plane search's rows
        a = ds.search(b3, r3, 3, 20, False)
        c = view.search(b3, r3, 3, 20, False)
        assert c.timing["v_path"] == 2 and c.n_rows > 0
        _same_rows(a, c)
    finally:
        ds.plan.close()
        ds.close()


# ---- B: the link seam ------------------------------------------------------------------------------------------------------
def _link_panel(seed):
    """pairs SNV-SNV, insertion-SNV and deletion-SNV whose alleles are 62..66 reference bases apart, one pair per kilobase; some
    copies carry both records, some one of them"""
    rng = np.random.default_rng(seed)
    n_samples = 8
    p = Panel(seed, 34_000, n_samples)
    i = 400
    for rep in range(2):
        for kind in ("snv", "ins", "del"):
            for gap in (62, 63, 64, 65, 66):
                pick = rng.choice(4, size=2 * n_samples, p=[0.4, 0.15, 0.15, 0.3])  # both, first only, second only, neither
                pick[:2], pick[2], pick[3] = 0, 1, 2
                rng.shuffle(pick)
                first, second = np.flatnonzero((pick == 0) | (pick == 1)), np.flatnonzero((pick == 0) | (pick == 2))
                k = 2 + 5 * rep
                e = {"snv": lambda: p.snv(i, first), "ins": lambda: p.insertion(i, k, first), "del": lambda: p.deletion(i, k, first)}[kind]()
                p.snv(e + gap, second)
                i += 1000
    return p.region()


@pytest.mark.parametrize("pam_s,guidelen,right", [("NGG", 20, False), ("NRG", 41, False), ("TTTV", 40, True)])
def test_link_seam(monkeypatch, pam_s, guidelen, right):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _link_panel(9201)

    def counts(st, plan, info, kept):
        inst, distinct = _host_clusters(reg, info)
        assert st["status"] == 0 and st["instances"] == inst and st["distinct"] == len(distinct), (st, inst, len(distinct))
        assert any(len(d) == 2 for d in distinct) and any(len(d) == 1 for d in distinct)
    _view_check(reg, pam_s, guidelen, right, 2, stats=counts)


# ---- C: the chain cap ------------------------------------------------------------------------------------------------------
def _chain_panel(seed, chain):
    """copies 0..3 carry 500 isolated shared SNVs, then a chain of `chain` SNVs 20 nt apart (starting at record 500: across the
    chunk seams), then a private SNV; copies 4, 5 carry the isolated SNVs and a private SNV only"""
    p = Panel(seed, 50_000 + 20 * chain + 2_000, 3)
    i = 300
    for _ in range(500):
        p.snv(i, range(6))
        i += 100
    for _ in range(chain):
        p.snv(i, range(4))
        i += 20
    for c in range(6):
        p.snv(i + 100 * (c + 1), [c])
    return p.region()


@pytest.mark.parametrize("chain", [4096, 4097])
def test_chain_cap(monkeypatch, chain):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _chain_panel(9301 + chain, chain)

    def cap(st, plan, info, kept):
        inst, _ = _host_clusters(reg, info)
        assert st["instances"] == inst
        if chain <= 4096:
            assert st["status"] == 0 and st["usable"], st
        else:
            assert st["status"] & 1 and not st["usable"], st  # a chain beyond CL_MAXWALK: the per-word search takes the plan
    _view_check(reg, "NGG", 20, False, 2 if chain <= 4096 else 1, stats=cap)


# ---- D: row bounds ---------------------------------------------------------------------------------------------------------
# cl_cut (hawk_cldict.hip) classes an instance by where its windows (starts [o_first - 43, o_end), L <= 44) can fall against the
# row's scan range [ss, se) and the string [PAD, hl - 44 - PAD]: outside (any of its comparisons holds: no cluster), interior (all
# of them hold: shareable) or neither (a cluster of its own row); run_inside (all hold) lets the search count the clean run in front
# without the row.  Each comparison: (name, predicate, holds when its value is <= 0 ('le') or >= 0 ('ge')).
_TERMS = (("o_end vs ss-44", "outside", "le"), ("o_first-43 vs se", "outside", "ge"),
          ("o_first-43 vs lo", "interior", "ge"), ("o_first vs 64", "interior", "ge"), ("o_end vs se-44", "interior", "le"),
          ("o_end vs hl-44-PAD+1", "interior", "le"), ("o_end vs hl-128", "interior", "le"),
          ("pa vs lo", "run_inside", "ge"), ("o_first vs se-44", "run_inside", "le"), ("o_first vs hl-44-PAD+1", "run_inside", "le"))
# the comparisons a padded region can make decisive (see _bounds_panel for the others)
_DECIDED = ("o_end vs ss-44", "o_first-43 vs se", "o_first-43 vs lo", "o_end vs se-44", "o_end vs hl-128", "pa vs lo", "o_first vs se-44")


def _bound_values(o_first, o_end, pa, ss, se, hl):
    lo, q = max(ss, HAWK_PAD), hl - 44 - HAWK_PAD + 1
    return {"o_end vs ss-44": o_end - (ss - 44), "o_first-43 vs se": o_first - 43 - se, "o_first-43 vs lo": o_first - 43 - lo,
            "o_first vs 64": o_first - 64, "o_end vs se-44": o_end - (se - 44), "o_end vs hl-44-PAD+1": o_end - q,
            "o_end vs hl-128": o_end + 128 - hl, "pa vs lo": pa - lo, "o_first vs se-44": o_first - (se - 44), "o_first vs hl-44-PAD+1": o_first - q}


def _outcome(holds):
    """(class: 0 outside, 1 shareable, 2 own row; run_inside) from the comparisons that hold"""
    by = {}
    for name, pred, _ in _TERMS:
        by.setdefault(pred, []).append(holds[name])
    return (0 if any(by["outside"]) else 1 if all(by["interior"]) else 2), all(by["run_inside"])


def _alleles(reg):
    """positions, REF and ALT lengths of the region's variants"""
    return tuple(np.array(x, dtype=np.int64) for x in zip(*[(v.pos, len(v.ref), len(v.alt)) for v in reg.variants]))


def _row_geometry(reg, al, plan, r, idx):
    """row positions of a row's records (sorted variant indices), their ends, cluster starts / ends (record ranks), and the row's
    scan range and length as the plan holds them"""
    pos, reflen, altlen = al
    o = pos[idx] - reg.startp + np.concatenate(([0], np.cumsum(altlen[idx] - reflen[idx])[:-1]))
    oe = o + altlen[idx]
    ss, se, hl = int(plan.host_meta.scan_lo[r]), int(plan.host_meta.scan_hi[r]), int(plan.hap_len[r])
    assert hl == len(reg.sequence) + int((altlen[idx] - reflen[idx]).sum())
    starts = np.flatnonzero(np.concatenate(([True], o[1:] - oe[:-1] > 64)))
    ends = np.concatenate((starts[1:], [len(idx)]))
    return o, oe, starts, ends, ss, se, hl


def _host_distinct(reg, plan, info, kept):
    """the distinct clusters the dictionary must count, from the classes: a shareable instance is its variant tuple, one that
    could meet a bound of its row is a cluster of its own, one wholly outside the scan range has none"""
    al = _alleles(reg)
    singles, multis, own = set(), set(), 0
    for r, inf in zip(kept, info):
        idx = np.sort(np.asarray(inf.variant_idx, dtype=np.int64))
        if len(idx) == 0:
            continue
        o, oe, starts, ends, ss, se, hl = _row_geometry(reg, al, plan, r, idx)
        of, ol = o[starts], oe[ends - 1]
        outside = (ol <= ss - 44) | (of - 43 >= se)
        interior = (of - 43 >= max(ss, HAWK_PAD)) & (of >= 64) & (ol <= se - 44) & (ol <= hl - 44 - HAWK_PAD + 1) & (ol + 128 <= hl)
        one = ends - starts == 1
        singles.update(idx[starts[~outside & interior & one]].tolist())
        for k in np.flatnonzero(~outside & interior & ~one):
            multis.add(tuple(idx[starts[k]:ends[k]].tolist()))
        own += int((~outside & ~interior).sum())
    return len(singles) + len(multis) + own


def _bounds_panel(seed, pamlen):
    """Shared SNVs (two copies or more; a private SNV per copy keeps rows apart) at every offset of every comparison a padded region
    can make decisive.  Per d in -4..4 - P copies: around ss - 45, ss + 43, se - 45, se + 43; Q copies: a record ending at ss + d
    and one 70 nt behind it (pa), and an SNV ending at hl - 158 + d; T copies: that SNV and a 30-base deletion behind the scan range,
    65+ nt behind it - the row is 30 bases shorter, o_end + 128 <= hl decides its class, and the same variant is shareable in the
    Q rows and at the bound in the T rows.  Not decisive here: o_first >= 64 and the PAD side of o_first - 43 >= max(ss, PAD) (any
    cluster after a record starts 66+ bases into the row, so both hold whenever o_first - 43 >= ss does); o_end <= hl - 44 - PAD + 1
    (implied by o_end + 128 <= hl); o_first <= hl - 44 - PAD + 1 in run_inside (binds under o_first <= se - 44 only behind a trailing
    deletion of 95+ bases, whose anchor then joins the probe's cluster); the PAD side of pa >= max(ss, PAD) (only behind a leading
    deletion of ~90+ bases across the scan start)."""
    p = Panel(seed, 7_000, 27)
    hl = len(p.seq)
    ss, se = ora.scan_bounds(np.arange(p.reg.startp, p.reg.startp + hl, dtype=np.int64), p.reg.startp, p.reg.stopp, pamlen)
    col = 0
    for d in range(-4, 5):
        P, Q, T = [col, col + 1], [col + 2, col + 3], [col + 4, col + 5]
        col += 6
        for x in (ss - 45 + d, ss + 43 + d, se - 45 + d, se + 43 + d):
            p.snv(x, P)
        p.snv(ss - 1 + d, Q)
        p.snv(ss - 1 + d + 70, Q)
        p.snv(hl - 159 + d, Q + T)
        p.deletion(hl - 88, 30, T)
    for c in range(col):
        p.snv(1_000 + 80 * c, [c])
    return p.region()


def _bound_coverage(reg, plan, info, kept):
    """the offsets -3..+3 at which each comparison DECIDES the outcome of a shared one-SNV instance (flipping it alone would change
    the class or run_inside), from the rows as the plan holds them"""
    al = _alleles(reg)
    carried = np.array([int(v.gt.sum()) for v in reg.variants])
    seen = {}
    for r, inf in zip(kept, info):
        idx = np.sort(np.asarray(inf.variant_idx, dtype=np.int64))
        if len(idx) == 0:
            continue
        o, oe, starts, ends, ss, se, hl = _row_geometry(reg, al, plan, r, idx)
        for a, b in zip(starts, ends):
            v = idx[a]
            if b - a != 1 or al[1][v] != 1 or al[2][v] != 1 or carried[v] < 2:
                continue
            vals = _bound_values(int(o[a]), int(oe[a]), int(oe[a - 1]) if a else 0, ss, se, hl)
            holds = {n: (vals[n] <= 0 if side == "le" else vals[n] >= 0) for n, _, side in _TERMS}
            base = _outcome(holds)
            for n, val in vals.items():
                if -3 <= val <= 3 and _outcome(dict(holds, **{n: not holds[n]})) != base:
                    seen.setdefault(n, set()).add(val)
    return seen


@pytest.mark.parametrize("pam_s,guidelen,right", [("NGG", 20, False), ("NRG", 41, False), ("TTTV", 19, True), ("TTTV", 40, True)])
def test_instances_at_row_bounds(monkeypatch, pam_s, guidelen, right):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _bounds_panel(9401, len(pam_s))

    def coverage(st, plan, info, kept):
        seen = _bound_coverage(reg, plan, info, kept)
        for name in _DECIDED:
            assert seen.get(name) == set(range(-3, 4)), (name, seen.get(name))
        inst, _ = _host_clusters(reg, info)
        distinct = _host_distinct(reg, plan, info, kept)
        # (the classes show in the distinct count too: a probe classed shareable one base too early merges its copies' rows - right
        # at the scan start, where nothing can lie between the bound and the cluster, but not what the classes promise)
        assert st["status"] == 0 and st["instances"] == inst and st["distinct"] == distinct, (st, inst, distinct)
    _view_check(reg, pam_s, guidelen, right, 2, stats=coverage)


# ---- E: seams of the cutting passes ----------------------------------------------------------------------------------------
def _seams_panel(seed):
    """Rows laid out record by record (isolated SNVs 70 nt apart, cluster members 20 nt apart; each layout carried by two copies
    that differ in their last record): cluster starts at record 62, 63, 64, 255, 256, 1023, 1024, 1025, 2047 (wave, slice and chunk
    ends), clusters of 2-4 records that begin at 62, 63, 254, 255, 1022, 1023 and 2046, rows of exactly 1024, 1025 and 2048 records."""
    layouts = [  # (records before the last one, {record index: cluster size})
        (2100, {62: 3, 254: 4, 1022: 2, 2046: 3}),
        (2100, {63: 2, 255: 3, 1023: 4}),
        (2100, {}),
        (2100, {62: 4, 255: 2, 1022: 4, 2046: 2}),
        (1023, {}), (1024, {}), (2047, {1023: 2}),
    ]
    p = Panel(seed, 2101 * 70 + 2_000, len(layouts))
    for li, (n, multi) in enumerate(layouts):
        cols = [2 * li, 2 * li + 1]
        i, k = 300, 0
        while k < n:
            size = min(multi.get(k, 1), n - k)
            for m in range(size):
                p.snv(i, cols)
                i += 20 if m + 1 < size else 70
            k += size
        p.snv(i, cols[:1])
        p.snv(i + 1, cols[1:])
    return p.region()


@pytest.mark.parametrize("pam_s,guidelen,right", [("NGG", 20, False), ("TTTV", 40, True)])
def test_cutting_seams(monkeypatch, pam_s, guidelen, right):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _seams_panel(9501)

    def counts(st, plan, info, kept):
        inst, distinct = _host_clusters(reg, info)
        sizes = sorted(len(inf.variant_idx) for inf in info if len(inf.variant_idx))
        assert {1024, 1025, 2048} <= set(sizes) and max(sizes) > 2048
        assert st["status"] == 0 and st["instances"] == inst and st["distinct"] == len(distinct), (st, inst, len(distinct))
    _view_check(reg, pam_s, guidelen, right, 2, stats=counts)


# ---- F: the head launch and the bitmap in HBM ------------------------------------------------------------------------------
def _wide_panel(seed, n_var, step, af, n_samples=800):
    """n_var SNVs `step` nt apart, every copy carries each with probability af (sparse rows): the rows' chunks span af^-1 x 1024
    variant indices; rows + chunks >= 1536 start the head launch"""
    length = step * n_var + 600
    reg = synth.make_region(seed, "chrW", length + 2_000, 1_000, 1_000 + length - 201)
    rng = np.random.default_rng(seed + 1)
    seq = reg.sequence.upper()
    n_col = 2 * n_samples
    G = np.empty((n_var, n_col), dtype=np.uint8)
    for k0 in range(0, n_var, 8192):
        k1 = min(n_var, k0 + 8192)
        G[k0:k1] = rng.random((k1 - k0, n_col), dtype=np.float32) < af
    reg.samples = [f"S{s:04d}" for s in range(n_samples)]
    out = []
    for k in range(n_var):
        i = 300 + step * k
        r = seq[i]
        out.append(synth.VariantSite(reg.startp + i, r, BASES[(BASES.index(r) + 1 + k % 3) % 4], float(G[k].mean()), G[k].reshape(n_samples, 2)))
    reg.variants = out
    reg.gt_matrix = G
    return reg


def _sub_region(reg, samples):
    """the same region with only `samples` (and the variants they carry): what the oracle is run on"""
    sub = synth.SynthRegion(reg.contig, reg.contig_seq, reg.bed_start, reg.bed_stop)
    sub.samples = [reg.samples[s] for s in samples]
    sub.variants = [synth.VariantSite(v.pos, v.ref, v.alt, v.af, v.gt[samples]) for v in reg.variants if v.gt[samples].any()]
    return sub


def _by_label(rows):
    out = {}
    for r in rows:
        out.setdefault(r[0], []).append(r[1:])
    return out


@pytest.mark.parametrize("n_var,step,af,hbm", [(200_000, 3, 1 / 250, True), (60_000, 10, 1 / 60, False)])
def test_head_launch_and_bitmap_window(monkeypatch, n_var, step, af, hbm):
    # (variants far enough apart in a row that most clusters are one record: the template rows stay within their default budget)
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    reg = _wide_panel(9601 if hbm else 9602, n_var, step, af)
    pam_s, guidelen = "NGG", 20
    bits, bitsrc, _, _ = ora.pam_encode(pam_s)
    mm, pt = synth.cfd_tables()
    ds, info, _ms, kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        # the chunk geometry the launches see: rows in plan order, chunks of 1024 records
        spans = []
        for inf in info:
            idx = np.sort(np.asarray(inf.variant_idx, dtype=np.int64))
            if len(idx) == 0:
                continue
            for c0 in range(0, len(idx), 1024):
                part = idx[c0:c0 + 1024]
                spans.append((int(part[-1]) >> 5) - (int(part[0]) >> 5) + 1)
        bound = sum(len(inf.variant_idx) for inf in info) // 1024 + ds.plan.n_hap
        assert bound >= 16 * 96  # the head launch runs (hawk_launch_cl_fill)
        if hbm:
            assert min(spans[96:]) > 4096  # every chunk of the later launch reads the bitmap from HBM
        else:
            assert max(spans) <= 4096      # ... through its LDS window
        view = ds.plan.view()
        st = ds.plan.cluster_stats()
        inst, _ = _host_clusters(reg, info)
        assert st["status"] == 0 and st["usable"] and st["instances"] == inst
        assert st["distinct"] == _host_distinct(reg, ds.plan, info, kept)
        a = ds.search(bits, bitsrc, 3, guidelen, False, mm, pt)
        c = view.search(bits, bitsrc, 3, guidelen, False, mm, pt)
        assert c.timing["v_path"] == 2
        _same_rows(a, c)
        got = _by_label(_table_rows(c, info, kept, True))
        # a dozen sampled carriers against the oracle, the first rows (described by the head launch) among them
        picks = [0, 1, 2, 3] + [int(s) for s in np.linspace(40, len(reg.samples) - 1, 8)]
        sub = _sub_region(reg, picks)
        want, _, _ = _oracle_rows(sub, pam_s, guidelen, False, mm, pt)
        want = _by_label(want)
        assert want.pop(("REF",)) == got[("REF",)]
        assert len(want) >= 2 * len(picks) - 2
        for lab, rows in want.items():
            mine = [k for k in got if lab[0] in k]
            assert len(mine) == 1 and set(lab) <= set(mine[0]), lab
            assert got[mine[0]] == rows, lab
    finally:
        ds.plan.close()
        ds.close()


# ---- G: the sharing decision at its defaults -------------------------------------------------------------------------------
def _share_panel(seed, n_shared):
    """10 copies that all carry n_shared isolated SNVs, and two private SNVs each: 10 (n_shared + 3) instances over n_shared + 20
    distinct clusters - above 3 per distinct cluster from 5 shared SNVs, below it at 4"""
    p = Panel(seed, 12_000, 5)
    i = 500
    for _ in range(n_shared):
        p.snv(i, range(10))
        i += 300
    for c in range(10):
        for t in range(2):
            p.snv(i, [c])
            i += 300
    return p.region()


@pytest.mark.parametrize("n_shared,above", [(5, True), (4, False)])
def test_sharing_decision_at_its_default(n_shared, above):
    reg = _share_panel(9701, n_shared)

    def ratio(st, plan, info, kept):
        assert st["status"] == (0 if above else 4), st
        assert st["instances"] == 10 * (n_shared + 3) and st["distinct"] == n_shared + 20, st
        assert (st["instances"] > 3 * st["distinct"]) == above and st["instances"] != 3 * st["distinct"]
    _view_check(reg, "NGG", 20, False, 2 if above else 1, stats=ratio)


def test_template_slot_budget(monkeypatch):
    reg = _share_panel(9702, 8)
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    mm, pt = synth.cfd_tables()
    ds, info, _ms, kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        view = ds.plan.view()
        st = ds.plan.cluster_stats()
        assert st["usable"] and st["template_slots"] > 0, st
        want, n_cand, n_hits = _oracle_rows(reg, "NGG", 20, False, mm, pt)
        for slots, path in ((st["template_slots"] - 1, 1), (st["template_slots"], 2)):
            monkeypatch.setenv("HAWK_CLUSTER_MAX_SLOTS", str(slots))
            ds.plan.rebuild_dictionary()
            s2 = ds.plan.cluster_stats()
            assert s2["usable"] == (path == 2) and s2["template_slots"] == st["template_slots"], s2
            c = view.search(bits, bitsrc, 3, 20, False, mm, pt)
            assert c.timing["v_path"] == path
            assert (c.n_candidates, c.n_hits) == (n_cand, n_hits)
            assert _table_rows(c, info, kept, True) == want
    finally:
        ds.plan.close()
        ds.close()


# ---- H: hash collisions in the dictionary ----------------------------------------------------------------------------------
def collision_panel(seed, kind):
    """Clusters that share their first record A.  'alt': {A, B}, {A, B'} with B' another ALT at B's site, and {A, B''} with B'' 1 nt
    from B; 'longer': {A, B}, {A, B, C}; 'same': {A, B} only.  Each cluster is carried by 4 ('alt'), 6 ('longer') or 12 ('same')
    copies, every copy with a private SNV elsewhere."""
    p = Panel(seed, 20_000, 6)
    i = 500
    for _ in range(12):
        p.snv(i, range(12))
        if kind == "alt":
            p.snv(i + 20, [0, 1, 2, 3], shift=1)
            p.snv(i + 20, [4, 5, 6, 7], shift=2)
            p.snv(i + 21, [8, 9, 10, 11])
        elif kind == "longer":
            p.snv(i + 20, range(12))
            p.snv(i + 40, range(6, 12))
        else:
            p.snv(i + 20, range(12))
        i += 1_000
    for c in range(12):
        p.snv(i + 200 * c, [c])
    return p.region()


def test_product_library_ignores_the_weak_hash_switch(monkeypatch):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    monkeypatch.setenv("HAWK_CLUSTER_WEAK_HASH", "1")
    assert os.path.basename(_lib.LIB_PATH) == "libhawk_hip.so"
    st = _view_check(collision_panel(9801, "alt"), "NGG", 20, False, 2)
    assert st["status"] == 0


def test_dictionary_compare_catches_hash_collisions():
    """The compare of k_cl_uid against real collisions: only the hooks library (-DHAWK_TEST_HOOKS) can weaken the dictionary's key,
    so the check runs in a process of its own that loads it (tests/hooks_cluster_check.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    hooks = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhawk_hip_hooks.so")
    assert os.path.exists(hooks), "make -C crispr-hawk_amd/csrc builds libhawk_hip_hooks.so beside the product library"
    env = dict(os.environ, CRISPRHAWK_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, os.path.join(here, "hooks_cluster_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "hooks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
