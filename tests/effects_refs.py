"""Shared by test_effects_host.py, test_gpu_effects.py and test_gpu_effects_seams.py: the g7 report groups rebuilt through the
oracle, the comparison of a delta table against tests/golden/g14_effects.json.gz, the hand-built panels, the plain reference of
the stage (plain_effects) and the seam panels that prove of themselves which seam they sit on (prove / REQUIRED).

THE COMPARISON RULE.  Rows compare exactly - ids, ranks, strings, doubles bit for bit - with one exemption: inside a run of equal
worst deltas the reference's order is undefined (pandas' single-column sort_values is not stable), so such a run is compared as
a SET of rows and our order inside it must be first appearance in the report.  Where the cut at rank 25 splits a run, our ids
of that run must be a subset of the run's ids (stored by the generator), of the right size, and the first of them by report
appearance.  So that the exemption cannot hide a failure, the callers assert: at most one split run per table (there is one cut),
at most one of a score's three NO-CANDIDATE tables split - a departure from the issue, which states this of every table: the
generator asserts it of the reference alone for the no-candidate tables only, because with a candidate forced in the cut moves
into phased16's run of seven positions at -0.9659 (ranks 19-25), which no none-valid candidate avoids, so two of the three
CFDon tables with candidates split a run (phased16 and indel_dense) -,
and every row outside such runs compared exactly."""
import functools
import io
import struct

import numpy as np

from crisprhawk_hip import reports, synth
from crisprhawk_hip.hapset import PosSegments, segments_from_posmap
from crisprhawk_hip.pam import PAM
from oracle import oracle as ora
from util import load_golden, oracle_haplotypes

FIXTURES = ["phased16", "phased4", "indel_dense"]


class _Hap:
    def __init__(self, label, posmap, n):
        self.samples, self.variants, self.id = label["samples"], label["variants"], label["id"]
        self.afs = {k: (float("nan") if v is None else v) for k, v in label["afs"].items()}
        rel, gen = segments_from_posmap(posmap)
        self.segments = PosSegments(rel, gen, n)


def g14():
    return _g14()


@functools.lru_cache(maxsize=None)
def _g14():
    return load_golden("g14_effects.json.gz")


def fixture_pam(fx):
    pam = PAM(fx["pam"], fx["right"], True)
    pam.encode(0)
    return pam


def oracle_inputs(fx):
    """(oracle HapSet, label objects) of a g7 fixture, as tests/test_reports.py builds them"""
    haps = oracle_haplotypes(fx)
    scan = [ora.scan_bounds(h["posmap"], fx["startp"], fx["stopp"], len(fx["pam"])) for h in haps]
    hs = ora.HapSet([h["seq"] for h in haps], [h["posmap"] for h in haps], [h["samples"] == ["REF"] for h in haps], scan)
    labels = [_Hap(lb, h["posmap"], len(h["seq"])) for lb, h in zip(fx["haplotypes"], haps)]
    return hs, labels


@functools.lru_cache(maxsize=None)
def host_report(name):
    """(fixture, ReportGroups, HapLabels, (cols, order, plain)) of g7_report_<name> through the oracle's search and collapse"""
    fx = load_golden(f"g7_report_{name}.json.gz")
    hs, labels = oracle_inputs(fx)
    res = ora.search(hs, fx["pam"], fx["guidelen"], fx["right"])
    g = res.guides
    mm, pt = synth.cfd_tables()
    _, _, _, cfd, _ = ora.reverse_and_cfdon(res, hs.is_ref, fx["guidelen"], len(fx["pam"]), mm, pt)
    isref_row = np.asarray(hs.is_ref)[g["hap"]]
    groups, gc = ora.collapse_rows(g["start"], g["stop"], g["strand"], isref_row, res.windows, fx["guidelen"], len(fx["pam"]), fx["right"])
    perm, off, num, den = [], [0], [], []
    for key, rows in groups.items():
        perm += rows
        off.append(len(perm))
        num.append(gc[key][0]); den.append(gc[key][1])
    inp = reports.ReportInput(g["start"], g["stop"], g["strand"], g["hap"], g["pos"], res.windows, cfd, np.array(perm), np.array(off),
                              np.array(num), np.array(den), fx["guidelen"], len(fx["pam"]), fx["right"])
    G = reports.ReportGroups.from_report_input(inp)
    lab = reports.HapLabels.from_objects(labels)
    columns = reports.group_columns(G, lab, fixture_pam(fx), fx["contig"], fx["target"], with_cfdon=True)
    return fx, G, lab, columns


def group_scores(column, order):
    """the generator's per-report-row column (None = NaN) -> one value per group"""
    vals = np.array([np.nan if v is None else v for v in column], dtype=np.float64)
    out = np.empty(len(vals))
    out[np.asarray(order)] = vals
    return out


def bits(v):
    return None if v is None else struct.pack("<d", float(v)) if isinstance(v, float) else v


def _row(values):
    return tuple(bits(None if (isinstance(v, float) and v != v) else v) for v in values)


def frame_rows(df):
    rows = []
    for rec in df.itertuples(index=False):
        rows.append([None if (isinstance(v, float) and v != v) else (v.item() if hasattr(v, "item") else v) for v in rec])
    return rows


def first_appearance(report_tsv):
    """guide_id -> index of its first row in the report"""
    import pandas as pd
    rep = pd.read_csv(io.StringIO(report_tsv), sep="\t", usecols=["chr", "start", "strand"])
    seen = {}
    for i, gid in enumerate((rep["chr"].astype(str) + "_" + rep["start"].astype(str) + "_" + rep["strand"]).tolist()):
        seen.setdefault(gid, i)
    return seen


def compare_table(df, want, n_cand, report_tsv):
    """the comparison rule above; returns whether the table holds a split run"""
    assert list(df.columns) == want["columns"]
    assert [str(t) for t in df.dtypes] == want["dtypes"]
    got_rows, want_rows = frame_rows(df), want["rows"]
    assert len(got_rows) == len(want_rows)
    first = first_appearance(report_tsv)
    worst = [bits(None if w is None else float(w)) for w in want["worst"]]
    n = len(want_rows)
    i = 0
    exact = 0
    while i < n:
        j = i + 1
        if i >= n_cand:  # (candidates come in the order given: never a run)
            while j < n and worst[j] == worst[i]:
                j += 1
        last = j == n and want["cut"]["split"]
        if j - i == 1 and not last:
            assert _row(got_rows[i]) == _row(want_rows[i]), (i, got_rows[i], want_rows[i])
            exact += 1
        else:
            ids = [r[0] for r in got_rows[i:j]]
            assert [r[1] for r in got_rows[i:j]] == list(range(i + 1, j + 1))  # Rank
            assert ids == sorted(ids, key=lambda g: first[g]), "inside a run of equal worst deltas: first appearance in the report"
            if last:
                run = want["cut"]["run_ids"]
                assert set(ids) <= set(run) and len(set(ids)) == j - i
                assert ids == sorted(run, key=lambda g: first[g])[:j - i], "the cut takes the run's first positions in report order"
                theirs = {r[0]: r for r in want_rows[i:j]}
                for r in got_rows[i:j]:  # a position both chose: the same row but for its rank
                    if r[0] in theirs:
                        assert _row(r[2:]) == _row(theirs[r[0]][2:]) and r[0] == theirs[r[0]][0]
            else:
                assert sorted(_row(r[:1] + r[2:]) for r in got_rows[i:j]) == sorted(_row(r[:1] + r[2:]) for r in want_rows[i:j])
        i = j
    runs_split = 1 if want["cut"]["split"] else 0
    assert runs_split <= 1
    return bool(want["cut"]["split"]), exact


# ---------------------------------------------------------------------------------------------------------------- the seam panel
class Panel:
    """Hand-built group columns (what hapset.GroupTable / reports.ReportGroups expose) + haplotype sample labels"""

    def __init__(self, guidelen=20, pamlen=3, right=False):
        self.guidelen, self.pamlen, self.right = guidelen, pamlen, right
        self.start, self.stop, self.strand, self.cfdon, self.wins, self.members = [], [], [], [], [], []
        self.hap_samples, self.is_ref_hap = ["REF"], [True]
        self.name, self.proved = "panel", []

    def prove(self, label, cond):
        """the panel sits on the seam it was built for (the tests hold REQUIRED against `proved`)"""
        assert bool(cond), f"{self.name}: off its seam: {label}"
        self.proved.append(label)

    def hap(self, label):
        self.hap_samples.append(label)
        self.is_ref_hap.append(False)
        return len(self.hap_samples) - 1

    def group(self, start, strand, score, members, core=None, flank=0, stop=None):
        """core: cased spacer+PAM text in window order (default: upper case for REF members, one lower-case base else)"""
        L = self.guidelen + self.pamlen
        if core is None:
            core = "A" * L if members == [0] else "A" * 5 + "c" + "A" * (L - 6)
        assert len(core) == L
        left = "ACGTACGTAC"[:10 - 1] + "ACGT"[flank % 4]
        self.start.append(start); self.stop.append(start + L if stop is None else stop); self.strand.append(strand)
        self.cfdon.append(score); self.wins.append(left + core + "TTTTTTTTTT"); self.members.append(list(members))
        return len(self.start) - 1

    _LUT = {ch: code for code, ch in enumerate("?ACMGRSVTWYHKDBN?acmgrsvtwyhkdbn") if ch != "?"}

    @classmethod
    def _planes(cls, w):
        """the five bit planes of one window text (bit i of plane p: bit p of the code of character i)"""
        out = [0] * 5
        for i, ch in enumerate(w):
            for p in range(5):
                if (cls._LUT[ch] >> p) & 1:
                    out[p] |= 1 << i
        return out

    def build(self):
        n = len(self.start)
        seen, table = {}, []   # every distinct window text is encoded once; the planes are filled by one gather
        idx = np.empty(n, dtype=np.int64)
        for g, w in enumerate(self.wins):
            k = seen.get(w)
            if k is None:
                k = seen[w] = len(table)
                table.append(self._planes(w))
            idx[g] = k
        win = np.ascontiguousarray(np.array(table, dtype=np.uint64).reshape(-1, 5).T[:, idx]) if n else np.zeros((5, 0), dtype=np.uint64)
        self.n_groups = n
        self.win = win
        self.member_off = np.concatenate(([0], np.cumsum([len(m) for m in self.members]))).astype(np.int64)
        self.member_hap = np.array([h for m in self.members for h in m], dtype=np.uint32)
        self.start, self.stop = np.array(self.start, dtype=np.int64), np.array(self.stop, dtype=np.int64)
        self.strand, self.cfdon = np.array(self.strand, dtype=np.uint8), np.array(self.cfdon, dtype=np.float64)
        return self


def results_equal(a, b):
    """two EffectsResult bit for bit (NaN patterns included)"""
    for k in a.ARRAYS:
        x, y = np.ascontiguousarray(getattr(a, k)), np.ascontiguousarray(getattr(b, k))
        if k == "counts":
            x, y = x[:7], y[:7]
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), (k, x[:20], y[:20])


def rules_panel():
    """duplicates under a flank, a strand-1 group, a position without REF, an alternative without a lower-case base"""
    p = Panel()
    a, b = p.hap("S1:1|0"), p.hap("S1:0|1,S2:1|0,S3:1|1")
    L = 23
    p.group(100, 0, 0.9, [0])
    p.group(100, 0, 0.5, [a], core="A" * 5 + "c" + "A" * 17, flank=1)
    p.group(100, 0, 0.5, [b], core="A" * 5 + "c" + "A" * 17, flank=2)           # the same guide text: a duplicate
    p.group(100, 0, 0.2, [a, b], core="A" * 21 + "g" + "A")                      # PAM only
    p.group(100, 1, 0.7, [0])
    p.group(100, 1, 0.1, [a], core="a" + "A" * 22)                               # strand 1: the window's first 3 bases are the PAM
    p.group(200, 0, 0.3, [a], core="A" * 4 + "t" + "A" * 16 + "c" + "A")         # no REF here; spacer + PAM
    p.group(300, 0, 0.4, [0])
    p.group(300, 0, 0.4, [b], core="C" + "A" * (L - 1))                          # an alt without a lower-case base
    return p.build()


def right_panel():
    pr = Panel(right=True)
    h = pr.hap("S1:1|0")
    pr.group(10, 0, 1.0, [0]); pr.group(10, 0, 0.5, [h], core="a" + "A" * 22); pr.group(10, 0, 0.4, [h], core="A" * 3 + "c" + "A" * 19)
    return pr.build()


def _core(i, L=23):
    """a distinct cased core per i: upper-case C where i has a bit, one lower-case base"""
    c = ["C" if (i >> k) & 1 else "A" for k in range(L)]
    k = i % L
    c[k] = c[k].lower()
    return "".join(c)


def positions_panel(seed=1, block=256):
    """Positions of 1, 2, 63, 64 and 65 groups, one position across each workgroup boundary of the per-group kernels, 2 workgroups
    + 1 group in all; positions without REF, with REF only, with REF last in collapse order; scores with ties and NaN"""
    rng = np.random.default_rng(seed)
    p = Panel()
    haps = [p.hap(f"S{i}:1|0") for i in range(40)]
    sizes = [1, 2, 63, 64, 65]
    while sum(sizes) + 3 <= block - 4:
        sizes.append(3)
    sizes.append(block + 4 - sum(sizes))          # ends 4 groups into the second workgroup
    while sum(sizes) + 3 <= 2 * block - 3:
        sizes.append(3)
    sizes.append(2 * block + 1 - sum(sizes))      # ends 1 group into the third
    assert sum(sizes) == 2 * block + 1 and all(s >= 1 for s in sizes)
    n = 0
    for k, size in enumerate(sizes):
        start, strand = 1000 + 7 * (k // 2), k % 2
        kind = k % 5  # 0, 1, 3: REF first; 2: no REF; 4: REF last in collapse order
        if size == 1:
            kind = 0 if k % 2 == 0 else 2
        ref_at = None if kind == 2 else (size - 1 if kind == 4 else 0)
        for j in range(size):
            n += 1
            score = float(rng.integers(0, 8)) / 8 + (1e-5 if rng.random() < 0.2 else 0.0)
            if rng.random() < 0.05:
                score = float("nan")
            if j == ref_at:
                p.group(start, strand, score, [0])
            else:
                m = [haps[int(x)] for x in rng.choice(40, size=int(rng.integers(1, 4)), replace=False)]
                p.group(start, strand, score, m, core=_core(n))
    return p.build(), sizes


def samples_panel(n_names=65536):
    """member lists of 1, 2, 63, 64, 65 and 4097 rows; sample ids 0, 31, 32, 63, 64 and n_names - 1; a row listing three samples;
    one sample on both of its rows; lists of exactly FX_SHORT_LIST entries and one more"""
    p = Panel()
    p.hap_samples += [f"N{i}:1|0" for i in range(n_names)]   # row 1 + i names sample id i
    p.is_ref_hap += [False] * n_names
    three = p.hap("N5:1|0,N6:0|1,N7:1|1")
    both = [p.hap("N9:1|0"), p.hap("N9:0|1")]
    want = []
    p.group(50, 0, 1.0, [0]); want.append(0)
    n = 0

    def alt(members, expect):
        nonlocal n
        n += 1
        p.group(50, 0, 0.5, members, core=_core(n))
        want.append(expect)
    for size in (1, 2, 63, 64, 65, 4097, 16, 17):
        alt(list(range(100, 100 + size)), size)
    alt([1 + i for i in (0, 31, 32, 63, 64, n_names - 1)], 6)
    alt([1 + i for i in (0, 31, 32, 63, 64, n_names - 1)] * 3 + list(range(2000, 2020)), 26)  # every id three times + 20 more: the wave path dedups
    alt([three], 3)
    alt([three, 1 + 5, 1 + 6], 3)
    alt(both, 1)
    alt(both + [1 + 9], 1)
    return p.build(), want


def tie_panel(n_pos=30, seed=3):
    """every position REF + one alternative with the same delta: the ranking is the report's order"""
    rng = np.random.default_rng(seed)
    p = Panel()
    h = p.hap("S1:1|0")
    for k in range(n_pos):
        p.group(500 + 3 * k, 0, 0.75, [0])
        p.group(500 + 3 * k, 0, 0.25, [h], core=_core(k + 1))
    p.build()
    return p, rng.permutation(p.n_groups)


# ------------------------------------------------------------------------------------------- the plain reference of the stage
# Written from the rules at the top of csrc/hawk_effects.h and DESIGN.md §4 on Python floats, lists, sets and sorted(): nothing
# of the library runs here.  The constants restate the kernels' (hawk_effects.h, hawk_device.h, hawk_effects.hip).
FX_BLOCK, FX_MAX_K, FX_TOPK_MAX_BLOCKS, FX_SHORT_LIST, FX_LONG_WAVES = 256, 64, 1024, 16, 4096
FX_NONE, FX_TYPE_UNKNOWN, SIGNED, ABSOLUTE = 0xFFFFFFFF, 255, 0, 1
_DTYPES = dict(score=np.float64, delta=np.float64, abs_delta=np.float64, n_samples=np.uint32, type=np.uint8, dup=np.uint8, position=np.uint32,
               pos_ref=np.uint32, pos_worst=np.float64, pos_nvalid=np.uint32, pos_first_rank=np.uint32, chosen=np.uint32, alt_off=np.uint64,
               alt_group=np.uint32, counts=np.uint64)


class PlainResult:
    ARRAYS = tuple(_DTYPES)   # the names and order of graphical_reports.EffectsResult.ARRAYS (asserted by the tests)


def label_names(label):
    return [] if label in ("REF", "") else [e.split(":")[0] for e in label.split(",")]


def _okey(order):
    return np.asarray(order, dtype=np.int64).tobytes()


def _plain_static(panel, order):
    """what no score changes: positions, report order inside them, origin, type, duplicates, distinct samples, the counts"""
    cache = panel.__dict__.setdefault("_plain_static", {})
    if _okey(order) in cache:
        return cache[_okey(order)]
    n, L = panel.n_groups, panel.guidelen + panel.pamlen
    start, stop, strand = panel.start.tolist(), panel.stop.tolist(), panel.strand.tolist()
    assert all((start[g - 1], strand[g - 1]) <= (start[g], strand[g]) for g in range(1, n)), "the panels are built in collapse order"
    rank = [0] * n
    for r, g in enumerate(np.asarray(order).tolist()):
        rank[g] = r
    names = [label_names(lb) for lb in panel.hap_samples]
    is_ref = [bool(panel.is_ref_hap[m[0]]) for m in panel.members]
    positions, h = [], 0
    for g in range(1, n + 1):
        if g == n or (start[g], strand[g]) != (start[h], strand[h]):
            positions.append(sorted(range(h, g), key=rank.__getitem__))   # a position: its groups in report order
            h = g
    head, typ, dup, ns, counts = [0] * n, [0] * n, [0] * n, [0] * n, [0] * 8
    memo_type, memo_ns = {}, {}
    for grp in positions:
        h = min(grp)
        counts[5] += 1
        shown = set()
        for g in grp:
            head[g] = h
            core = panel.wins[g][10:10 + L]
            if not is_ref[g]:
                t = memo_type.get((core, strand[g]))
                if t is None:
                    pamfirst = bool(panel.right) != bool(strand[g])   # in window order; which slice is which is all the rule asks
                    sp, pm = (core[panel.pamlen:], core[:panel.pamlen]) if pamfirst else (core[:panel.guidelen], core[panel.guidelen:])
                    lo_sp, lo_pm = any(c.islower() for c in sp), any(c.islower() for c in pm)
                    t = memo_type[(core, strand[g])] = 1 if lo_sp and lo_pm else 2 if lo_sp else 3 if lo_pm else FX_TYPE_UNKNOWN
                typ[g] = t
                mk = tuple(panel.members[g])
                v = memo_ns.get(mk)
                if v is None:
                    listed = [s for m in mk for s in names[m]]
                    v = memo_ns[mk] = (len(set(listed)), len(listed))
                ns[g] = v[0]
                if len(mk) > FX_SHORT_LIST or v[1] > FX_SHORT_LIST:
                    counts[6] += 1
            if (stop[g], core) in shown:
                dup[g] = 1
            else:
                shown.add((stop[g], core))
                counts[4 if typ[g] == FX_TYPE_UNKNOWN else typ[g]] += 1
    st = dict(n=n, start=start, strand=strand, rank=rank, is_ref=is_ref, positions=positions, head=head, type=typ, dup=dup, n_samples=ns, counts=counts)
    cache[_okey(order)] = st
    return st


def _plain_positions(panel, order, family, score):
    """per score: rounded scores, deltas, per position REF / valid alternatives / worst delta, and the full ranking"""
    st = _plain_static(panel, order)
    sc = np.ascontiguousarray(panel.cfdon if score is None else score, dtype=np.float64)
    cache = panel.__dict__.setdefault("_plain_positions", {})
    key = (_okey(order), family, sc.tobytes())
    if key in cache:
        return cache[key]
    n, is_ref, rank = st["n"], st["is_ref"], st["rank"]
    rs = [round(x, 4) for x in sc.tolist()]
    nan = float("nan")
    delta, adelta, pos_ref, worst, nvalid, first, alts = [0.0] * n, [0.0] * n, [FX_NONE] * n, [0.0] * n, [0] * n, [FX_NONE] * n, {}
    ranked = []
    for grp in st["positions"]:
        h = st["head"][grp[0]]
        first[h] = rank[grp[0]]
        ref = next((g for g in grp if is_ref[g]), None)   # the first REF group in report order
        if ref is None:
            continue
        pos_ref[h], r = ref, rs[ref]
        valid = []
        for g in grp:
            d = rs[g] - r
            if d != d:
                d = nan
            delta[g], adelta[g] = d, abs(d)
            if not is_ref[g] and (family == ABSOLUTE or rs[g] < r):
                valid.append(g)
        nvalid[h], alts[h] = len(valid), valid
        if valid:
            worst[h] = min(delta[g] for g in valid) if family == SIGNED else max(adelta[g] for g in valid)
        ranked.append(h)
    w = worst
    ranked = sorted(ranked, key=lambda h: (w[h] != w[h], 0.0 if w[h] != w[h] else w[h] if family == SIGNED else -w[h], first[h]))
    out = dict(score=rs, delta=delta, abs_delta=adelta, pos_ref=pos_ref, pos_worst=worst, pos_nvalid=nvalid, pos_first_rank=first, alts=alts,
               ranked=ranked)
    if len(cache) >= 4:
        cache.clear()
    cache[key] = out
    return out


def plain_effects(panel, order, family, score=None, cands=(), K=25):
    """The stage in plain Python: a PlainResult with the arrays of graphical_reports.EffectsResult.ARRAYS"""
    st, ps = _plain_static(panel, order), _plain_positions(panel, order, family, score)
    assert 1 <= K <= FX_MAX_K and len(cands) <= K
    start, strand = st["start"], st["strand"]
    at = {(start[h], strand[h]): h for h in ps["ranked"]}
    named = {(int(s), int(t)) for s, t in cands}
    chosen = [at.get((int(s), int(t)), FX_NONE) for s, t in cands]
    take = K - len(cands)
    for h in ps["ranked"]:
        if take == 0:
            break
        if (start[h], strand[h]) not in named:
            chosen.append(h)
            take -= 1
    alt_off, alt_group = [0], []
    for h in chosen:
        if h != FX_NONE:
            alt_group += ps["alts"][h]
        alt_off.append(len(alt_group))
    vals = dict(score=ps["score"], delta=ps["delta"], abs_delta=ps["abs_delta"], n_samples=st["n_samples"], type=st["type"], dup=st["dup"],
                position=st["head"], pos_ref=ps["pos_ref"], pos_worst=ps["pos_worst"], pos_nvalid=ps["pos_nvalid"],
                pos_first_rank=ps["pos_first_rank"], chosen=chosen, alt_off=alt_off, alt_group=alt_group, counts=st["counts"])
    res = PlainResult()
    for k, dt in _DTYPES.items():
        setattr(res, k, np.array(vals[k], dtype=dt))
    return res


# ------------------------------------------------------------------------------------------------------- the seam panels
def _ulp_down(x):
    import math
    return math.nextafter(x, -math.inf)


def round4_values():
    """what round(x, 4) is pinned on: the fixtures' distinct unrounded scores, exact binary ties, both neighbours of each, the
    doubles nearest the decimal ties, random values, the specials"""
    import math
    vals = []
    for name in FIXTURES:  # the fixtures' distinct unrounded scores
        _, G, _, _ = host_report(name)
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
    special += [-0.0, -4e-5, math.inf, -math.inf, 2.0 ** 38, _ulp_down(2.0 ** 38), -2.0 ** 38, 5e-324]
    return vals + ties + near + rand + decimal_ties + special


@functools.lru_cache(maxsize=None)
def round_panel():
    """positions of REF + one alternative over consecutive values of round4_values(), each pair both ways round: the device's
    fx_round4 and fx_delta meet the ties, their neighbours, the specials and the sign of zero.  -> (panel, order, score)"""
    v = round4_values()
    if len(v) % 2:
        v.append(0.0)
    inf = float("inf")
    v += [0.0, -4e-5, inf, inf, -inf, inf, -inf, -inf, 2.0 ** 38, _ulp_down(2.0 ** 38)]   # pairs that must meet whatever the list's parity
    p = Panel()
    p.name = "round"
    h = p.hap("S1:1|0")
    score = []
    for i in range(0, len(v), 2):
        for a, b in ((v[i], v[i + 1]), (v[i + 1], v[i])):
            s = 100 + 3 * (len(score) // 2)
            p.group(s, 0, 0.0, [0]); p.group(s, 0, 0.0, [h])
            score += [a, b]
    p.build()
    score = np.array(score, dtype=np.float64)
    rs = [round(x, 4) for x in score.tolist()]
    zero = lambda x: struct.pack("<d", x)
    p.prove("-4e-5 rounds to -0.0 with its sign", zero(round(-4e-5, 4)) == zero(-0.0) and zero(-0.0) in {zero(x) for x in rs})
    d = [rs[i + 1] - rs[i] for i in range(0, len(rs), 2)]
    p.prove("a delta of -0.0", any(zero(x) == zero(-0.0) for x in d))
    p.prove("inf - inf: the quiet NaN", any(x != x for x in d) and any(x == float("inf") for x in d) and any(x == float("-inf") for x in d))
    p.prove("2^38 and the double below it", 2.0 ** 38 in rs and round(_ulp_down(2.0 ** 38), 4) in rs and 5e-324 in score.tolist())
    p.prove("exact ties, both ways", round(0.03125, 4) == 0.0312 and round(0.09375, 4) == 0.0938 and 0.03125 in score.tolist())
    return p, np.arange(p.n_groups), score


MERGE_LAYOUTS = (["best_first", "best_last", "random", "all_tied", "nan_many", "nan_few"]
                 + [f"ranked_{n}" for n in sorted({k + d for k in (1, 25, 63, 64) for d in (-1, 0, 1)})])
MERGE_KS = (1, 25, 63, 64)


def topk_blocks(n_groups):
    return max(1, min(FX_TOPK_MAX_BLOCKS, (n_groups + FX_BLOCK - 1) // FX_BLOCK))


def merge_tiles(n_groups):
    return (topk_blocks(n_groups) * FX_MAX_K + FX_BLOCK - 1) // FX_BLOCK


@functools.lru_cache(maxsize=None)
def merge_panel(layout, n_pos=4000):
    """REF + one alternative per position, 2 * n_pos groups: k_fx_topk_merge reads more than one tile of workgroup results.
    -> (panel, order, heads of the ranked positions)"""
    rng = np.random.default_rng(21)
    p = Panel()
    p.name = f"merge[{layout}]"
    h1, h2 = p.hap("S1:1|0"), p.hap("S2:0|1")
    D = [round(-0.9999 + 2e-4 * i, 4) for i in range(n_pos)]   # distinct worst deltas, the best first
    per_block = FX_BLOCK // 2
    n_blocks = (2 * n_pos + FX_BLOCK - 1) // FX_BLOCK
    with_ref = set(range(n_pos))
    if layout == "best_first":   # ... but for one straggler in the last workgroup, 21st by value: from K = 25 on the merge returns early
        D[n_pos - 1] = round(D[19] + 1e-4, 4)   # on its middle tiles and then joins ONE survivor with a full L
    elif layout == "best_last":
        D = D[::-1]
    elif layout == "random":
        D = [D[i] for i in rng.permutation(n_pos)]
    elif layout == "all_tied":
        D = [-0.5] * n_pos
    elif layout.startswith("ranked_"):
        D = [D[i] for i in rng.permutation(n_pos)]
        with_ref = {((5 * j) % n_blocks) * per_block + 3 + j // n_blocks for j in range(int(layout.split("_")[1]))}
    elif layout.startswith("nan"):
        D = [D[i] for i in rng.permutation(n_pos)]
        keep = set(rng.choice(n_pos, size=100 if layout == "nan_many" else 10, replace=False).tolist())
        D = [d if i in keep else float("nan") for i, d in enumerate(D)]
    for i in range(n_pos):
        s = 1000 + 3 * i
        if i in with_ref:
            p.group(s, 0, 1.0, [0])
        else:
            p.group(s, 0, 0.9, [h2], core=_core(2 * n_pos + i + 1))
        p.group(s, 0, round(1.0 + D[i], 4), [h1], core=_core(i + 1))
    p.build()
    order = np.arange(p.n_groups)[::-1].copy() if layout == "all_tied" else np.arange(p.n_groups)
    heads = [2 * i for i in sorted(with_ref)]
    p.prove("the merge reads more than one tile", merge_tiles(p.n_groups) > 1 and topk_blocks(p.n_groups) == n_blocks)
    first_tile, last_tile = FX_BLOCK // FX_MAX_K * FX_BLOCK, (n_blocks - FX_BLOCK // FX_MAX_K) * FX_BLOCK   # group bounds of the merge's end tiles
    for fam in (SIGNED, ABSOLUTE):
        for K in MERGE_KS:
            c = plain_effects(p, order, fam, None, (), K).chosen.tolist()
            if layout == "best_first" and K == 1:
                p.prove("later tiles add nothing", c[0] < first_tile)
            elif layout == "best_first":
                p.prove("one straggler of the last tile joins a full L", len(c) == K and sorted(c)[-1] == 2 * (n_pos - 1) and sorted(c)[-2] < first_tile)
            if layout in ("best_last", "all_tied"):
                p.prove("the winners sit in the last tile", len(c) == K and min(c) >= last_tile)
            if layout == "random":
                p.prove("winners in several tiles", K == 1 or len({h // first_tile for h in c}) > 1)
    if layout.startswith("ranked_"):
        n = int(layout.split("_")[1])
        blocks = [h // FX_BLOCK for h in heads]
        p.prove(f"exactly {n} ranked positions", len(heads) == n and len(plain_effects(p, order, SIGNED, None, (), 64).chosen) == min(n, 64))
        p.prove("spread over the workgroups", len(set(blocks)) == min(n, n_blocks) and (n < 2 or len({b // (FX_BLOCK // FX_MAX_K) for b in blocks}) > 1))
    if layout.startswith("nan"):
        pw = plain_effects(p, order, ABSOLUTE, None, (), 64)
        nn = sum(1 for h in heads if pw.pos_worst[h] == pw.pos_worst[h])
        if layout == "nan_many":
            p.prove("more than K positions without NaN", nn > 64 and not np.isnan(pw.pos_worst[pw.chosen]).any())
        else:
            w = pw.pos_worst[pw.chosen]
            fr = pw.pos_first_rank[pw.chosen][nn:].tolist()
            p.prove("fewer than K positions without NaN: NaN last, then by rank", nn < 25 and not np.isnan(w[:nn]).any() and np.isnan(w[nn:]).all()
                    and fr == sorted(fr) and len(w) == 64)
    return p, order, heads


def merge_candidates(panel, heads, K):
    """the candidate lists of one K: none, three (one in the last workgroup), one naming no position, n_cand == K, n_cand == K - 1"""
    pos = lambda h: (int(panel.start[h]), int(panel.strand[h]))
    out = [()]
    if K >= 3 and len(heads) >= 3:
        out.append((pos(heads[1]), pos(heads[-1]), pos(heads[len(heads) // 2])))
    out.append(((1, 0),))
    if len(heads) >= 2 and K >= 3:
        out.append((pos(heads[0]), (1, 0), pos(heads[-1])))
    for n in (K, K - 1):
        if 1 <= n <= len(heads):
            step = len(heads) // n
            out.append(tuple(pos(h) for h in heads[::step][:n][::-1]))
    return out


STRIDE_G = FX_TOPK_MAX_BLOCKS * FX_BLOCK + FX_BLOCK + 1
STRIDE_LAYOUTS = ("tail", "head")


@functools.lru_cache(maxsize=None)
def stride_panel(layout):
    """G = 1024 * 256 + 256 + 1 groups: k_fx_topk_part's workgroups 0 and 1 take a second tile, workgroup 1's holds one group
    (a REF-only position).  `tail`: report reversed; the best |delta| lie at groups >= 262144, the signed family's few negative
    deltas are split between the first and the second tile of workgroup 0, and its ties at 0.0 are won by the lowest ranks - the
    last groups.  `head`: collapse order, everything that wins lies in workgroup 0's first tile.  -> (panel, order)"""
    rng = np.random.default_rng(33)
    G = STRIDE_G
    n_pos = G // 2
    tail0 = FX_TOPK_MAX_BLOCKS * FX_BLOCK // 2           # the first position of the second tiles
    per = FX_BLOCK // 2
    d = (rng.integers(1, 3000, n_pos) / 1e4).tolist()   # everywhere else: small positive deltas (no valid alternative when signed)
    pick = lambda lo, hi, k: [x / 1e4 for x in rng.choice(np.arange(lo, hi), size=k, replace=False).tolist()]
    if layout == "tail":
        where = rng.permutation(per)
        for j, x in enumerate([-x for x in pick(9000, 9900, 20)] + pick(8000, 8900, 30)):
            d[tail0 + int(where[j])] = x
        for j, x in enumerate([-x for x in pick(7000, 8000, 10)] + pick(6000, 7000, 20)):
            d[int(where[j])] = x
    else:
        where = rng.permutation(per)
        for j, x in enumerate([-x for x in pick(9000, 9900, 20)] + pick(5000, 8900, per - 20)):
            d[int(where[j])] = x
    p = Panel()
    p.name = f"stride[{layout}]"
    h = p.hap("S1:1|0")
    alt = "A" * 5 + "c" + "A" * 17
    for i in range(n_pos):
        s = 1000 + 3 * i
        p.group(s, 0, 1.0, [0]); p.group(s, 0, round(1.0 + d[i], 4), [h], core=alt)
    p.group(1000 + 3 * n_pos, 0, 1.0, [0])
    p.build()
    order = np.arange(G)[::-1].copy() if layout == "tail" else np.arange(G)
    p.prove("two workgroups take a second tile, the second one group", p.n_groups == G and topk_blocks(G) == FX_TOPK_MAX_BLOCKS
            and G - FX_TOPK_MAX_BLOCKS * FX_BLOCK == FX_BLOCK + 1)
    second = FX_TOPK_MAX_BLOCKS * FX_BLOCK
    for fam in (SIGNED, ABSOLUTE):
        for K in (25, 64):
            c = plain_effects(p, order, fam, None, (), K).chosen.tolist()
            assert len(c) == K
            if layout == "head":
                p.prove("all in the first tile", max(c) < FX_BLOCK)
            elif fam == ABSOLUTE and K == 25:
                p.prove("the K best lie in the second tile", min(c) >= second)
            else:
                p.prove("the kept and the new are joined", min(c) < FX_BLOCK and max(c) >= second and all(x < FX_BLOCK or x >= second for x in c))
            if layout == "tail" and fam == SIGNED and K == 64:
                p.prove("the lone group of workgroup 1's second tile is chosen", G - 1 in c)
    if layout == "head":   # no entry of the second tile comes before the K-th of workgroup 0's first tile
        for fam in (SIGNED, ABSOLUTE):
            ps = _plain_positions(p, order, fam, None)
            place = {x: i for i, x in enumerate(ps["ranked"])}
            kth = sorted(place[x] for x in range(0, FX_BLOCK, 2))[FX_MAX_K - 1]   # K = 64: the weakest threshold
            p.prove("the second tile's filter rejects everything", all(place[x] > kth for x in range(second, G) if x in place))
    return p, order


@functools.lru_cache(maxsize=None)
def queue_panel(n_long=FX_LONG_WAVES + 64 + 40):
    """More long groups than k_fx_samples_long has waves, every one long by its ENTRIES (one or two member rows whose labels list
    17 or more samples), 40 sample ids (2 bitmap words: 62 lanes have none), sets of several sizes none of which contains another,
    consecutive groups' sets disjoint.  -> (panel, order)"""
    rng = np.random.default_rng(44)
    p = Panel()
    p.name = "queue"
    label = lambda ids, gt="1|0": ",".join(f"N{i}:{gt}" for i in ids)
    p.hap(label(range(40)))   # (names every id once, in order; no group's member)
    short = p.hap(label([3, 24, 39]))
    shapes = [(3, 9), (5, 6), (7, 4), (8, 2)]   # ids taken from each half of a side: more of one means fewer of the other - no set holds another
    sets = []
    n = 0
    for k in range(n_long // 2 + 1):
        s = 1000 + 3 * k
        p.group(s, 0, 1.0, [0])
        for side in (0, 1):   # ids 0..19 / 20..39: consecutive long groups share no sample
            if len(sets) == n_long:
                break
            a, b = shapes[int(rng.integers(0, 4))]
            ids = sorted((20 * side + rng.choice(10, size=a, replace=False)).tolist() + (20 * side + 10 + rng.choice(10, size=b, replace=False)).tolist())
            sets.append(ids)
            n += 1
            if n % 3 == 0:     # one row: the set, then its head again until 17 entries are listed
                members = [p.hap(label(ids + ids[:17 - len(ids)]))]
            else:              # two rows: both haplotypes of every sample carry the allele (8 + 9 entries and more)
                members = [p.hap(label(ids)), p.hap(label(ids[:max(17 - len(ids), 5) + n % 4], "0|1"))]
            p.group(s, 0, 0.5, members, core=_core(n))
        p.group(s, 0, 0.4, [short], core=_core(n + n_long))
    p.build()
    st = _plain_static(p, np.arange(p.n_groups))
    _, _, n_ids = _sample_ids(p)
    p.prove("40 sample ids: two bitmap words", n_ids == 40)
    p.prove("more long groups than waves + 64", st["counts"][6] == n_long and n_long >= FX_LONG_WAVES + 64 + 1)
    long_by_entries = [g for g in range(p.n_groups) if not st["is_ref"][g] and len(p.members[g]) <= 2
                       and sum(len(label_names(p.hap_samples[m])) for m in p.members[g]) > FX_SHORT_LIST]
    p.prove("long by entries, one or two member rows", len(long_by_entries) == n_long and {len(p.members[g]) for g in long_by_entries} == {1, 2})
    p.prove("short groups and REF groups", sum(st["is_ref"]) > 0 and st["n_samples"].count(3) > 0)
    masks = np.array([sum(1 << i for i in ids) for ids in sets], dtype=np.uint64)
    nested = 0
    for i in range(0, len(masks), 512):
        sub = (masks[i:i + 512, None] & ~masks[None, :]) == 0        # set i inside set j
        nested += int(sub.sum()) - int((masks[i:i + 512, None] == masks[None, :]).sum())
    p.prove("no set holds another, the sizes differ", nested == 0 and len({len(s) for s in sets}) >= 3)
    p.prove("consecutive sets are disjoint", all(not (set(a) & set(b)) for a, b in zip(sets, sets[1:])))
    return p, np.arange(p.n_groups)


def _sample_ids(panel):
    ids = {}
    for lb in panel.hap_samples:
        for nm in label_names(lb):
            ids.setdefault(nm, len(ids))
    return ids, [[ids[nm] for nm in label_names(lb)] for lb in panel.hap_samples], len(ids)


EDGE_IDS = (1, 31, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def edge_panel(n_ids):
    """the short / long classification at its edge, with `n_ids` sample ids and the highest id present in a long group.
    -> (panel, order, per alternative (n_samples, is_long))"""
    p = Panel()
    p.name = f"edge[{n_ids}]"
    label = lambda ids: ",".join(f"N{i % n_ids}:1|0" for i in ids)
    down = lambda k, at=0: [n_ids - 1 - ((at + t) % n_ids) for t in range(k)]   # k entries from the highest id down
    p.hap(label(range(n_ids)))   # row 1: names every id once, in order
    want = []
    p.group(50, 0, 1.0, [0])

    def alt(members, ns, is_long):
        want.append((ns, is_long))
        p.group(50, 0, 0.5, members, core=_core(len(want)))
    d = lambda k: min(k, n_ids)
    alt([p.hap(label(down(16)))], d(16), False)                                   # 1 row x 16 entries
    alt([p.hap(label(down(17)))], d(17), True)                                    # 1 row x 17 entries
    alt([p.hap(label(down(8))), p.hap(label(down(8, 8)))], d(16), False)          # 2 rows x 8 entries
    alt([p.hap(label(down(8))), p.hap(label(down(9, 8)))], d(17), True)           # 8 + 9 entries
    alt([p.hap(label([n_ids - 1 - (t % 8) % n_ids])) for t in range(16)], d(8), False)   # 16 rows, 8 ids twice: pairwise across rows
    alt([p.hap(label([n_ids - 1])) for _ in range(17)], 1, True)                  # 17 rows, one sample: long by its member count
    alt([1, 1], n_ids, 2 * n_ids > FX_SHORT_LIST)                                 # every id on two rows
    p.build()
    st = _plain_static(p, np.arange(p.n_groups))
    _, _, n = _sample_ids(p)
    p.prove(f"{n_ids} sample ids, the highest in a long group", n == n_ids and f"N{n_ids - 1}:" in p.hap_samples[p.members[2][0]] and want[1][1])
    p.prove("the classification edge", st["n_samples"][1:] == [w[0] for w in want] and st["counts"][6] == sum(1 for w in want if w[1]))
    return p, np.arange(p.n_groups), want


ALTS_ORDERS = ("collapse", "reverse", "random")
ALTS_SIZES = (63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def alts_panel(order_kind):
    """positions of 63, 64, 65 and 130 groups with two or three REF groups none of which is first in collapse order, valid,
    invalid (score >= ref, NaN) and duplicate alternatives interleaved, and 70 small positions, some without a valid
    alternative.  -> (panel, order, score, candidates): the candidates name the four large positions, no position at all (in
    the middle) and two positions without a valid alternative"""
    rng = np.random.default_rng(55)
    p = Panel()
    p.name = f"alts[{order_kind}]"
    haps = [p.hap(f"S{i}:1|0") for i in range(12)]
    score, cands, n = [], [], 0
    for k, size in enumerate(ALTS_SIZES):
        s = 1000 + 5 * k
        refs_at = sorted(rng.choice(np.arange(1, size - 1), size=2 + k % 2, replace=False).tolist())
        for j in range(size):
            if j in refs_at:
                p.group(s, 1, 0.0, [0], flank=j)          # the same REF text under another flank
                score.append(0.5 + 0.01 * refs_at.index(j))
                continue
            n += 1
            kind = 3 if j == size - 1 else int(rng.integers(0, 5))   # (the last group of every position is a valid alternative)
            core = _core(n) if kind else _core(n - 1 if j - 1 not in refs_at and j > 0 else n)   # kind 0: the text of the group before
            p.group(s, 1, 0.0, [haps[n % 12]], core=core, flank=j)
            score.append(float("nan") if kind == 1 else 0.5 + 0.01 * int(rng.integers(0, 5)) if kind == 2 else round(float(rng.random()) * 0.45, 4))
        cands.append((s, 1))
    small = []
    for k in range(70):
        s = 2000 + 5 * k
        p.group(s, 0, 0.0, [0]); score.append(0.5)
        p.group(s, 0, 0.0, [haps[k % 12]], core=_core(1000 + k))
        score.append(0.7 if k % 7 == 0 else round(0.4 - 0.001 * k, 4))   # every seventh: no valid alternative in the signed family
        small.append((s, 0))
    cands = cands[:2] + [(1, 0)] + cands[2:] + [small[0], small[7]]
    p.build()
    n = p.n_groups
    order = {"collapse": np.arange(n), "reverse": np.arange(n)[::-1].copy(), "random": np.random.default_rng(56).permutation(n)}[order_kind]
    score = np.array(score, dtype=np.float64)
    st = _plain_static(p, order)
    r = plain_effects(p, order, SIGNED, score, cands, 64)
    sizes = sorted(len(g) for g in st["positions"])
    p.prove("positions of 63, 64, 65 and 130 groups, all chosen", sizes[-4:] == list(ALTS_SIZES) and all(int(h) != FX_NONE and r.position[h] == h for h in r.chosen[[0, 1, 3, 4]]))
    big = [g for g in st["positions"] if len(g) >= 63]
    p.prove("two or three REF groups, none first in collapse order", all(2 <= sum(st["is_ref"][x] for x in g) <= 3 and not st["is_ref"][min(g)] for g in big))
    p.prove("valid, invalid and duplicate alternatives interleaved", all(0 < r.pos_nvalid[min(g)] < len(g) - 3 for g in big) and sum(1 for g in range(p.n_groups) if st["dup"][g] and not st["is_ref"][g]) >= 8
            and all(np.isnan(score[g]).any() for g in big))
    p.prove("valid alternatives past the 64th group of a position", int(max(r.alt_group[r.alt_off[3]:r.alt_off[4]])) == int(r.chosen[3]) + 64 and int(max(r.alt_group[r.alt_off[4]:r.alt_off[5]])) == int(r.chosen[4]) + 129)
    p.prove("64 chosen, FX_NONE in the middle, positions without a valid alternative", len(r.chosen) == 64 and r.chosen[2] == FX_NONE
            and r.pos_nvalid[r.chosen[5]] == 0 and r.pos_nvalid[r.chosen[6]] == 0 and r.alt_off[-1] == len(r.alt_group) > 130)
    return p, order, score, cands


SHAPES = ((41, 3, False), (41, 3, True), (1, 1, False), (1, 1, True))


@functools.lru_cache(maxsize=None)
def shape_panel(guidelen, pamlen, right, n_pos=300):
    """The widest core (guidelen + pamlen = 44: the core mask reaches bit 53, the window bit 63) and the narrowest (1 + 1), both
    strands: one lower-case base at the first and the last base of the spacer and of the PAM, both, none; more than 256
    non-duplicate groups of every type over several workgroups; one guide shown three times across a workgroup boundary"""
    p = Panel(guidelen, pamlen, right)
    p.name = f"shape[{guidelen}+{pamlen}{' right' if right else ''}]"
    L = guidelen + pamlen
    h = p.hap("S1:1|0")
    low = lambda at: "".join(c.lower() if i in at else c for i, c in enumerate("A" * L))
    for k in range(n_pos):
        s, strand = 1000 + 50 * (k // 2), k % 2
        first = pamlen if bool(right) != bool(strand) else guidelen
        p.group(s, strand, 1.0, [0], core="A" * L)
        for at in sorted({0, first - 1, first, L - 1}):
            p.group(s, strand, 0.5, [h], core=low({at}))
        p.group(s, strand, 0.5, [h], core=low({0, L - 1}))
        p.group(s, strand, 0.5, [h], core="C" + "A" * (L - 1))
        while FX_BLOCK - 8 <= len(p.start) < FX_BLOCK + 2:    # the same guide again on both sides of group 256
            p.group(s, strand, 0.5, [h], core=low({0, L - 1}), flank=len(p.start))
    p.build()
    st = _plain_static(p, np.arange(p.n_groups))
    p.prove("the core mask reaches bit 53" if L == 44 else "the narrowest core", L + 20 <= 64 and (L == 44 or L == 2))
    p.prove("more than 256 groups of every type", all(c > FX_BLOCK for c in st["counts"][:5]) and p.n_groups > 4 * FX_BLOCK)
    dups = [g for g in range(p.n_groups) if st["dup"][g]]
    p.prove("one guide three times across a workgroup boundary", len(dups) >= 3 and min(dups) < FX_BLOCK <= max(dups) and
            st["head"][min(dups)] == st["head"][max(dups)])
    p.prove("both strands", set(st["strand"]) == {0, 1})
    return p, np.arange(p.n_groups)


REQUIRED = {
    "round": ["-0.0 with its sign", "a delta of -0.0", "quiet NaN", "2^38", "exact ties"],
    "merge": ["more than one tile"],
    "merge[best_first]": ["later tiles add nothing", "straggler"], "merge[best_last]": ["last tile"], "merge[all_tied]": ["last tile"],
    "merge[random]": ["several tiles"], "merge[nan_many]": ["more than K"], "merge[nan_few]": ["fewer than K"],
    "merge[ranked]": ["ranked positions", "spread over the workgroups"],
    "stride": ["take a second tile"], "stride[tail]": ["the K best lie in the second tile", "joined", "lone group"],
    "stride[head]": ["all in the first tile", "rejects everything"],
    "queue": ["two bitmap words", "more long groups than waves", "long by entries", "short groups and REF", "no set holds another", "disjoint"],
    "edge": ["the highest in a long group", "classification edge"],
    "alts": ["63, 64, 65 and 130", "none first in collapse order", "interleaved", "past the 64th group", "FX_NONE in the middle"],
    "shape": ["core", "more than 256", "three times across a workgroup boundary", "both strands"],
}


def seam_case(name):
    """-> (panel, order, the rank calls [(family, score, candidates, K), ...] one handle serves in this order, n_long or None)"""
    kind, _, arg = name.partition(":")
    if kind == "round":
        p, order, score = round_panel()
        return p, order, [(ABSOLUTE, score, (), 25), (SIGNED, score, (), 64)], None
    if kind == "merge":
        p, order, heads = merge_panel(arg)
        calls = []
        for K in MERGE_KS:
            for i, cands in enumerate(merge_candidates(p, heads, K)):
                fams = (SIGNED, ABSOLUTE) if not cands else (SIGNED,) if (i + K) % 2 else (ABSOLUTE,)
                calls += [(f, None if f == SIGNED else p.cfdon.copy(), cands, K) for f in fams]
        return p, order, calls, None
    if kind == "stride":
        p, order = stride_panel(arg)
        return p, order, [(SIGNED, None, (), 25), (ABSOLUTE, None, (), 64), (SIGNED, None, (), 64), (ABSOLUTE, None, (), 25)], None
    if kind == "queue":
        p, order = queue_panel()
        return p, order, [(SIGNED, None, (), 25)], _plain_static(p, order)["counts"][6]
    if kind == "edge":
        p, order, _ = edge_panel(int(arg))
        return p, order, [(SIGNED, None, (), 25)], _plain_static(p, order)["counts"][6]
    if kind == "alts":
        p, order, score, cands = alts_panel(arg)
        return p, order, [(SIGNED, score, cands, 64), (ABSOLUTE, score, cands, 64), (SIGNED, score, cands[:2], 25), (ABSOLUTE, score, (), 1),
                          (ABSOLUTE, score, cands[::-1], 7)], None
    if kind == "shape":
        g, pl, right = arg.split("+")
        p, order = shape_panel(int(g), int(pl), right == "right")
        return p, order, [(SIGNED, None, (), 25), (ABSOLUTE, None, (), 64)], None
    raise KeyError(name)


SEAM_CASES = (["round"] + [f"merge:{x}" for x in MERGE_LAYOUTS] + [f"stride:{x}" for x in STRIDE_LAYOUTS] + ["queue"]
              + [f"edge:{n}" for n in EDGE_IDS] + [f"alts:{x}" for x in ALTS_ORDERS]
              + [f"shape:{g}+{pl}+{'right' if r else 'left'}" for g, pl, r in SHAPES])


def check_required(panel):
    """every fragment REQUIRED names for the panel's family (`name`) and for the panel itself (`name[layout]`) was proved"""
    base = panel.name.split("[")[0]
    keys = [base, panel.name] + ([f"{base}[ranked]"] if "[ranked_" in panel.name else [])
    for k in keys:
        for frag in REQUIRED.get(k, []):
            assert any(frag in label for label in panel.proved), (panel.name, frag)
