"""Reference and case builders for tests/test_gpu_collapse.py, all on the CPU: a dictionary grouping of a guide table's own rows
(the report's groupby, reports.py:958-1008, with the model scorers' flanks in the key where asked), the key-width arithmetic of
the collapse driver (hawk_api_collapse.hip) restated, and hand-built haplotype sets - short sequences with a free position map -
placed on the seams of the collapse: one key field at a time, a flank base in and just outside the compared slice, position-map
spans one below and exactly at the steps of the sort key, thousands of different rows under one (start, strand).  Every builder
PROVES its seam from the oracle's search of the same set; a case that has drifted off its seam fails in its builder, and
tests/test_collapse_refs.py runs every builder without a GPU."""
import numpy as np

from crisprhawk_hip.hapset import DeviceHapSet, HostHaplotype, PosSegments, segments_from_posmap
from oracle import oracle as ora

PAD = 10  # GUIDESEQPAD / HAWK_PAD: bases stored on either side of spacer + PAM
MAX_FLANK = PAD
MAX_CORE = 44  # guidelen + pamlen the 64-bit window slices hold with both pads


# ---- the reference ---------------------------------------------------------------------------------------------------------
def key_slice(w: str, strand: int, up: int, down: int) -> str:
    """What two rows must share to merge: spacer + PAM widened by `up` bases on the guide's 5' side and `down` on its 3' side.
    Rows are stored on the + strand, so a strand-1 guide's 5' side is the window's right end."""
    n = len(w)
    return w[PAD - up:n - PAD + down] if strand == 0 else w[PAD - down:n - PAD + up]


def group_rows(start, stop, strand, is_ref_row, windows, guidelen, pamlen, right, flank=(0, 0)):
    """({key: [rows ascending]}, {key: (gc_num, gc_den)}); key = (start, stop, strand, origin, cased slice); GC of the spacer as in
    oracle.collapse_rows (C, G, S over A, C, G, T, S, W, U; either case)"""
    up, down = flank
    groups, gc = {}, {}
    for i, w in enumerate(windows):
        s = int(strand[i])
        key = (int(start[i]), int(stop[i]), s, bool(is_ref_row[i]), key_slice(w, s, up, down))
        groups.setdefault(key, []).append(i)
        if key not in gc:
            core = w[PAD:len(w) - PAD]
            pamfirst = bool(right) != bool(s)
            spacer = core[pamlen:] if pamfirst else core[:guidelen]
            num = sum(spacer.count(c) for c in "CGScgs")
            gc[key] = (num, num + sum(spacer.count(c) for c in "ATWUatwu"))
    return groups, gc


def reference_arrays(groups, gc, perm, off):
    """The arrays a collapse must return for this grouping.  Groups come in key order - start, then strand - and within one
    (start, strand) in the order of a hash the reference does not know: there the device's own order of the groups' FIRST members
    is taken, which every group must open with.  -> (perm, off, gc_num, gc_den), or an AssertionError naming what is off."""
    perm, off = np.asarray(perm, dtype=np.int64), np.asarray(off, dtype=np.int64)
    assert len(off) == len(groups) + 1, ("number of groups", len(off) - 1, len(groups))
    assert off[0] == 0 and (np.diff(off) > 0).all() and off[-1] == len(perm)
    by_first = {rows[0]: k for k, rows in groups.items()}
    heads = perm[off[:-1]].tolist()
    keys = []
    for h in heads:
        assert h in by_first, ("a group opens with a row that is no group's first member", h)
        keys.append(by_first[h])
    assert len(set(keys)) == len(keys)
    order = [(k[0], k[2]) for k in keys]
    assert order == sorted(order), "groups are not in (start, strand) order"
    want_perm = np.concatenate([np.asarray(groups[k], dtype=np.int64) for k in keys]) if keys else np.zeros(0, np.int64)
    want_off = np.concatenate(([0], np.cumsum([len(groups[k]) for k in keys]))).astype(np.int64)
    return (want_perm, want_off, np.array([gc[k][0] for k in keys], dtype=np.uint8), np.array([gc[k][1] for k in keys], dtype=np.uint8))


# ---- the sort key's widths (the collapse driver in hawk_api_collapse.hip, restated) ----------------------------------------
SPAN_MAX = 0xffffffff


def key_bits(span: int) -> dict:
    """span = max_gen - min_gen of the set's position maps (max_gen is one behind the last mapped position)"""
    if span > SPAN_MAX:
        return dict(accepted=False)
    end_bit = 32
    while end_bit < 64 and (span >> (end_bit - 32)) != 0:
        end_bit += 1
    pos_bits = end_bit - 31
    hash_bits = min(31, (pos_bits + 24 + 7) // 8 * 8 - pos_bits)
    begin_bit = 31 - hash_bits
    return dict(accepted=True, end_bit=end_bit, pos_bits=pos_bits, hash_bits=hash_bits, begin_bit=begin_bit,
                passes=(end_bit - begin_bit + 7) // 8, hash_table=span < SPAN_MAX)


# ---- direct sets ------------------------------------------------------------------------------------------------------------
_COMP = str.maketrans("ACGTSWNRYKMacgtswnrykm", "TGCASWNYRMKtgcaswnyrmk")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


class Direct:
    """A hand-built haplotype set + one search of it.  `rows()` is the oracle's search: (guides, windows)."""

    def __init__(self, name, pam, guidelen, right, flanks=((0, 0),)):
        self.name, self.pam, self.guidelen, self.right, self.flanks = name, pam, guidelen, right, tuple(flanks)
        self.seqs, self.posmaps, self.is_ref, self.scan = [], [], [], []
        self.proofs = []
        self._rows = None

    @property
    def pamlen(self):
        return len(self.pam)

    @property
    def L(self):
        return self.guidelen + len(self.pam)

    def add(self, seq, posmap=None, is_ref=False, scan=None):
        pm = np.arange(1, len(seq) + 1, dtype=np.int64) if posmap is None else np.asarray(posmap, dtype=np.int64)
        assert len(pm) == len(seq)
        self.seqs.append(seq)
        self.posmaps.append(pm)
        self.is_ref.append(bool(is_ref))
        self.scan.append((0, len(seq) - len(self.pam)) if scan is None else tuple(scan))
        self._rows = None
        return len(self.seqs) - 1

    def prove(self, what, ok):
        assert ok, f"{self.name}: off its seam - {what}"
        self.proofs.append(what)

    def hapset(self):
        return ora.HapSet(self.seqs, self.posmaps, self.is_ref, self.scan)

    def span(self):
        """max_gen - min_gen as meta_build computes them: every segment's start, and one behind its last position"""
        return int(max(int(pm.max()) + 1 for pm in self.posmaps) - min(int(pm.min()) for pm in self.posmaps))

    def rows(self):
        if self._rows is None:
            res = ora.search(self.hapset(), self.pam, self.guidelen, self.right)
            self._rows = (res.guides, res.windows)
        return self._rows

    def reference(self, flank=(0, 0)):
        g, wins = self.rows()
        isref_row = np.asarray(self.is_ref)[g["hap"]]
        return group_rows(g["start"], g["stop"], g["strand"], isref_row, wins, self.guidelen, self.pamlen, self.right, flank)

    def rows_at(self, start, strand):
        g, wins = self.rows()
        return [(int(g["hap"][i]), int(g["stop"][i]), wins[i]) for i in np.flatnonzero((g["start"] == start) & (g["strand"] == strand))]

    def device_set(self):
        haps = []
        for seq, pm, r, sc in zip(self.seqs, self.posmaps, self.is_ref, self.scan):
            rel, gen = segments_from_posmap(pm)
            haps.append(HostHaplotype(seq, PosSegments(rel, gen, len(seq)), r, sc))
        return DeviceHapSet(haps)


def _filler(rng, n, pam):
    """bases that open no PAM hit on either strand: A/T for G-rich PAMs, C/G (never doubled) for T-rich ones"""
    if "T" in pam.upper():
        first = int(rng.integers(2))
        return "".join("CG"[(first + i) % 2] for i in range(n))
    return "".join(rng.choice(list("AT"), size=n))


def _spacer(rng, n):
    """random ACGT with no GG, CC, TTT or AAA (no PAM of the cases below inside a spacer)"""
    out = []
    while len(out) < n:
        c = "ACGT"[int(rng.integers(4))]
        t = "".join(out[-2:]) + c
        if t.endswith(("GG", "CC", "TTT", "AAA")):
            continue
        out.append(c)
    return "".join(out)


def _pam_instance(pam):
    return pam.upper().replace("N", "T").replace("V", "A").replace("R", "A")


def _block(rng, pam, guidelen, right, strand, spacer=None):
    """the + strand text of one guide: spacer + PAM (PAM + spacer when `right`), reverse-complemented for strand 1 -> (text,
    offset of the spacer's first + strand base)"""
    sp = _spacer(rng, guidelen) if spacer is None else spacer
    p = _pam_instance(pam)
    txt = p + sp if right else sp + p
    sp_off = len(p) if right else 0
    if strand:
        txt = revcomp(txt)
        sp_off = len(txt) - sp_off - guidelen
    return txt, sp_off


def _snv(seq, i, to=None):
    """lower-case substitution at i (another base than the one there, or `to`)"""
    c = seq[i].upper()
    alt = to if to is not None else "ACGT"[("ACGT".index(c) + 1) % 4].lower()
    assert alt.upper() != c or to is not None
    return seq[:i] + alt + seq[i + 1:]


def _layout(rng, pam, guidelen, right, strands, gap=40, spacers=None):
    """filler + one block per entry of `strands` + filler -> (REF text, [core offset], [spacer offset])"""
    txt = _filler(rng, gap, pam)
    cores, sps = [], []
    for k, s in enumerate(strands):
        b, so = _block(rng, pam, guidelen, right, s, None if spacers is None else spacers[k])
        cores.append(len(txt))
        sps.append(len(txt) + so)
        txt += b + _filler(rng, gap, pam)
    return txt, cores, sps


# ---- A: key fields one at a time -------------------------------------------------------------------------------------------
def case_stop_only(strand=0):
    c = Direct(f"stop-only-s{strand}", "NGG", 20, False)
    rng = np.random.default_rng(41 + strand)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [strand])
    c.add(ref, is_ref=True)
    alt = _snv(ref, sps[0] + 5)
    c.add(alt)
    pm = np.arange(1, len(alt) + 1, dtype=np.int64)
    pm[cores[0] + 12:] += 7  # a deletion's jump inside the guide, behind its first base
    c.add(alt, pm)
    rows = c.rows_at(cores[0] + 1, strand)
    nonref = [r for r in rows if r[0] != 0]
    c.prove("two non-REF rows of one start and strand with one window", len(nonref) == 2 and nonref[0][2] == nonref[1][2])
    c.prove("that differ in stop alone", nonref[0][1] != nonref[1][1])
    groups, _ = c.reference()
    c.prove("the reference keeps them apart", sum(1 for k in groups if k[0] == cores[0] + 1 and k[2] == strand and not k[3]) == 2)
    return c


def case_origin():
    """REF and non-REF rows with equal windows cannot both leave the search: a non-REF row is kept only when its core differs from
    REF's at the same (start, strand), case aside (remove_redundant_guides).  The builder proves exactly that - the origin bit of
    the key never decides between two rows of one table - and the case pins the table the device keeps."""
    c = Direct("origin", "NGG", 20, False)
    rng = np.random.default_rng(43)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0, 1])
    ref = ref[:sps[0] + 4] + ref[sps[0] + 4].lower() + ref[sps[0] + 5:]  # a REF with a lower-case base of its own
    c.add(ref, is_ref=True)
    c.add(ref)            # the same text as a non-REF copy
    c.add(_snv(ref, sps[1] + 3))
    rows = c.rows_at(cores[0] + 1, 0)
    c.prove("the non-REF twin of a REF row does not survive the search", [r[0] for r in rows] == [0])
    c.prove("a non-REF row that differs does", sorted(r[0] for r in c.rows_at(cores[1] + 1, 1)) == [0, 2])
    return c


def case_case_only(where):
    """two non-REF rows whose windows differ in the case of ONE base (the V plane): the spacer's first base or the PAM's last"""
    c = Direct(f"case-only-{where}", "NGG", 20, False)
    rng = np.random.default_rng(47)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0])
    c.add(ref, is_ref=True)
    a = _snv(ref, sps[0] + 9)
    i = sps[0] if where == "spacer0" else cores[0] + c.L - 1
    b = a[:i] + a[i].lower() + a[i + 1:]
    c.add(a)
    c.add(b)
    rows = [r for r in c.rows_at(cores[0] + 1, 0) if r[0] != 0]
    c.prove("two non-REF rows of one start, stop and strand", len(rows) == 2 and rows[0][1] == rows[1][1])
    w0, w1 = rows[0][2], rows[1][2]
    diff = [k for k in range(len(w0)) if w0[k] != w1[k]]
    c.prove("whose windows differ at one base, in its case only", len(diff) == 1 and w0.upper() == w1.upper())
    c.prove("inside the core", diff[0] == (PAD if where == "spacer0" else PAD + c.L - 1))
    return c


def case_iupac():
    """two non-REF rows that differ in one base: the IUPAC code r against its member a"""
    c = Direct("iupac", "NGG", 20, False)
    rng = np.random.default_rng(53)
    sp = _spacer(rng, 20)
    sp = sp[:7] + "C" + sp[8:]
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0, 1], spacers=[sp, sp])
    c.add(ref, is_ref=True)
    for k, s in enumerate((0, 1)):
        i = sps[k] + (7 if s == 0 else 12)
        c.add(_snv(ref, i, "r"))
        c.add(_snv(ref, i, "a"))
    for k, s in enumerate((0, 1)):
        rows = [r for r in c.rows_at(cores[k] + 1, s) if r[0] != 0]
        c.prove("two non-REF rows under one start", len(rows) == 2)
        diff = [(x, y) for x, y in zip(rows[0][2], rows[1][2]) if x != y]
        c.prove("differing in one base, r against a", len(diff) == 1 and set(diff[0]) == {"r", "a"})
    return c


def case_many_identical(copies=300):
    c = Direct(f"identical-{copies}", "NGG", 20, False)
    rng = np.random.default_rng(59)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0, 1, 0])
    c.add(ref, is_ref=True)
    alt = _snv(_snv(_snv(ref, sps[0] + 2), sps[1] + 17), sps[2] + 11)
    for _ in range(copies):
        c.add(alt)
    groups, _ = c.reference()
    big = [k for k, v in groups.items() if len(v) == copies]
    c.prove("one group of all the copies per non-REF key", len(big) >= 3 and all((len(v) == copies) != k[3] for k, v in groups.items()))
    return c


def case_counts(n_groups, copies):
    """exactly n_groups groups of `copies` rows each, trimmed through the scan bounds of an all-N stretch (every position a PAM
    hit on both strands): copies = 1 REF's own rows, copies = 2 two equal lower-case non-REF copies over a REF without hits"""
    c = Direct(f"counts-{n_groups}x{copies}", "NGG", 20, False)
    rng = np.random.default_rng(61)
    target = n_groups * copies
    fl = _filler(rng, 40, c.pam)

    def count(n, stop):
        # the stretch ends the row: its last positions hold + strand rows only (the - strand window would leave the row), so the
        # number of rows moves in steps of `copies` there
        c.seqs, c.posmaps, c.is_ref, c.scan, c._rows = [], [], [], [], None
        sc = (30, stop)
        if copies == 1:
            c.add(fl + "N" * n, is_ref=True, scan=sc)
        else:
            c.add(fl + _filler(rng, n, c.pam), is_ref=True, scan=sc)
            for _ in range(copies):
                c.add(fl + "n" * n, scan=sc)
        return len(c.rows()[0])
    n = 4
    while count(n, 40 + n - 3) < target:
        n += 1
    got = -1
    for stop in range(40 + n - 3, 30, -1):
        got = count(n, stop)
        if got <= target:
            break
    groups, _ = c.reference()
    c.prove(f"{n_groups * copies} rows", got == n_groups * copies)
    c.prove(f"{n_groups} groups of {copies}", len(groups) == n_groups and all(len(v) == copies for v in groups.values()))
    return c


def case_isolated_pams(k):
    """exactly k groups of one row: a REF-only A/T background with k isolated AGG, 30 nt apart - k forward rows, no reverse hit.
    (1, 255, 256 and 257 groups, of one row and of two, are case_counts' above; this adds the count between 1 and 255 at which the
    bits of the (group number, row) sort step from 1 to 2.)"""
    c = Direct(f"isolated-{k}", "NGG", 20, False)
    rng = np.random.default_rng(67)
    c.add(_filler(rng, 40, c.pam) + "".join("AGG" + _filler(rng, 27, c.pam) for _ in range(k)) + _filler(rng, 40, c.pam), is_ref=True)
    g, _ = c.rows()
    groups, _ = c.reference()
    c.prove(f"{k} forward rows of REF", len(g) == k and (g["strand"] == 0).all())
    c.prove(f"{k} groups of one row", len(groups) == k and all(len(v) == 1 for v in groups.values()))
    return c


GC_SHAPES = [(1, "NGG", False), (1, "TTTV", True), (20, "NGG", False), (20, "TTTV", True), (41, "NGG", False), (40, "TTTV", True),
             (43, "G", False), (43, "G", True)]


def case_gc(guidelen, pam, right):
    """REF-only: spacers of S, of W, of N and of mixed case on both strands; guidelen + pamlen up to the 44-base core"""
    c = Direct(f"gc-{guidelen}-{pam}-{'R' if right else 'L'}", pam, guidelen, right)
    rng = np.random.default_rng(67 + guidelen)
    mixed = "".join(ch.lower() if k % 3 == 0 else ch for k, ch in enumerate(_spacer(rng, guidelen)))
    spacers = ["S" * guidelen, "W" * guidelen, "N" * guidelen, mixed]
    strands = [0, 0, 0, 0, 1, 1, 1, 1]
    ref, cores, sps = _layout(rng, pam, guidelen, right, strands, gap=30, spacers=spacers + spacers)
    c.add(ref, is_ref=True)
    groups, gc = c.reference()
    want_mixed = (sum(mixed.upper().count(x) for x in "CG"), guidelen)
    for k, s in enumerate(strands):
        hit = [key for key in groups if key[0] == cores[k] + 1 and key[2] == s]
        c.prove(f"the planted guide {k} is a row", len(hit) == 1)
        want = [(guidelen, guidelen), (0, guidelen), (0, 0), want_mixed][k % 4]
        c.prove(f"guide {k}: the reference's GC counts are the spacer's {want}", gc[hit[0]] == want)
    c.prove("the core reaches the 44-base limit" if guidelen + len(pam) == MAX_CORE else "core below the limit", c.L <= MAX_CORE)
    return c


# ---- B: flanks ---------------------------------------------------------------------------------------------------------------
FLANKS = ((0, 0), (4, 3), (10, 0), (0, 10), (10, 10))


def case_flank(strand, right, guidelen=20, places=(("5", 4), ("5", 5), ("3", 3), ("3", 4))):
    """Per entry of `places` one guide: four non-REF copies share a core SNV, two of them carry a second SNV d bases outside the
    core on the guide's 5' or 3' side.  The second SNV splits the group iff the flank on that side reaches it."""
    pam = "TTTV" if right else "NGG"
    name = f"flank-s{strand}-{'R' if right else 'L'}-{guidelen}-" + "".join(f"{s}{d}" for s, d in places)
    c = Direct(name, pam, guidelen, right, FLANKS)
    rng = np.random.default_rng(71 + 2 * strand + int(right) + guidelen)
    ref, cores, sps = _layout(rng, pam, guidelen, right, [strand] * len(places), gap=48)
    c.add(ref, is_ref=True)
    one = ref
    two = ref
    second = []
    for k, (side, d) in enumerate(places):
        left = (side == "5") == (strand == 0)  # the guide's 5' side is the window's left end on strand 0, its right end on strand 1
        i = cores[k] - d if left else cores[k] + c.L - 1 + d
        one = _snv(one, sps[k] + guidelen // 2)
        two = _snv(_snv(two, sps[k] + guidelen // 2), i)
        second.append(PAD - d if left else PAD + c.L - 1 + d)
    for seq in (one, two, one, two):
        c.add(seq)
    g, wins = c.rows()
    for k, (side, d) in enumerate(places):
        rows = [r for r in c.rows_at(cores[k] + 1, strand) if r[0] != 0]
        c.prove(f"guide {k}: four non-REF rows with one core", len(rows) == 4 and len({r[2][PAD:-PAD] for r in rows}) == 1)
        w1, w2 = [r[2] for r in rows if r[0] == 1][0], [r[2] for r in rows if r[0] == 2][0]
        diff = [x for x in range(len(w1)) if w1[x] != w2[x]]
        c.prove(f"guide {k}: the copies differ at window base {second[k]} alone", diff == [second[k]])
        for up, down in c.flanks:
            groups, _ = c.reference((up, down))
            n = sum(1 for key in groups if key[0] == cores[k] + 1 and key[2] == strand and not key[3])
            reach = up if side == "5" else down
            c.prove(f"guide {k}, flank {(up, down)}: {'split' if d <= reach else 'one group'}", n == (2 if d <= reach else 1))
    return c


def flank_cases():
    out = [case_flank(s, r) for s in (0, 1) for r in (False, True)]
    # the widest key: 44 + 10 + 10 = 64 bits of every plane (the mask branch `width >= 64`)
    out += [case_flank(s, r, 40 if r else 41, (("5", 10), ("3", 10), ("5", 4), ("3", 4))) for s in (0, 1) for r in (False, True)]
    return out


# ---- C: key width ------------------------------------------------------------------------------------------------------------
SPANS = [(1 << 15) - 1, 1 << 15, (1 << 16) - 1, 1 << 16, (1 << 23) - 1, 1 << 23, (1 << 31) - 1, 1 << 31, 0xfffffffe, 0xffffffff]
SPAN_BITS = {  # span -> (end_bit, begin_bit, passes), worked out by hand from collapse_rows
    (1 << 15) - 1: (47, 7, 5), 1 << 15: (48, 0, 6), (1 << 16) - 1: (48, 0, 6), 1 << 16: (49, 1, 6), (1 << 23) - 1: (55, 7, 6),
    1 << 23: (56, 0, 7), (1 << 31) - 1: (63, 7, 7), 1 << 31: (64, 0, 8), 0xfffffffe: (64, 0, 8), 0xffffffff: (64, 0, 8),
}


def case_span(span):
    """A non-REF copy whose position map jumps between two guides, so that max_gen - min_gen of the set is `span` and rows sit on
    both sides of the jump: the high start bits decide the order of the groups."""
    c = Direct(f"span-{span:#x}", "NGG", 20, False)
    rng = np.random.default_rng(79)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0, 1, 0, 1])
    n = len(ref)
    c.add(ref, is_ref=True)
    alt = ref
    for k in range(4):
        alt = _snv(alt, sps[k] + 6)
    pm = np.arange(1, n + 1, dtype=np.int64)
    pm[cores[2] - 15:] += span - n  # behind the second guide's window, before the third's
    c.add(alt, pm)
    c.add(alt, pm)
    c.prove(f"max_gen - min_gen = {span:#x}", c.span() == span)
    kb = key_bits(span)
    if span in SPAN_BITS:
        c.prove(f"(end_bit, begin_bit, passes) = {SPAN_BITS[span]}", kb["accepted"] and (kb["end_bit"], kb["begin_bit"], kb["passes"]) == SPAN_BITS[span])
        c.prove("the hash table is offered below 0xffffffff only", kb["hash_table"] == (span < 0xffffffff))
        g, _ = c.rows()
        far = g["start"] - 1 >= span - n
        c.prove("rows on both sides of the jump", far.any() and (~far).any() and int(g["start"].max()) - 1 < span)
        c.prove("the far rows' starts use key bits the near rows leave zero",
                int(g["start"][far].min() - 1).bit_length() > int(g["start"][~far].max() - 1).bit_length() and
                int(g["start"][far].min() - 1).bit_length() >= kb["end_bit"] - 33)
    else:
        c.prove("beyond the largest span the key holds", not kb["accepted"])
    return c


# ---- D: many distinct rows under one (start, strand) ------------------------------------------------------------------------
def case_many_distinct(k=8192, starts=4):
    """k non-REF copies, each with a 20-mer of its own in front of `starts` shared PAM positions, in a set whose span leaves 24
    hash bits in the sort key: about k^2 / 2^25 pairs of different rows per start collide there under any seed."""
    c = Direct(f"distinct-{k}x{starts}", "NGG", 20, False)
    rng = np.random.default_rng(83)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0] * starts, gap=14)
    n = len(ref)
    span = (1 << 30) + 5
    pm = np.arange(1, n + 1, dtype=np.int64)
    pm[cores[starts // 2] - 12:] += span - n
    c.add(ref, is_ref=True)
    body = np.frombuffer(ref.encode(), dtype=np.uint8)
    low = np.frombuffer(b"acgt", dtype=np.uint8)
    for _ in range(k):
        b = body.copy()
        for s in sps:
            x = rng.integers(4, size=20)
            for j in range(1, 20):  # no gg / cc: the shared PAMs stay the only hits
                while x[j] == x[j - 1] and x[j] in (1, 2):
                    x[j] = rng.integers(4)
            b[s:s + 20] = low[x]
        c.add(b.tobytes().decode(), pm)
    kb = key_bits(c.span())
    c.prove("span >= 2^23 with 24 hash bits left in the sort key", c.span() >= 1 << 23 and kb["hash_bits"] == 24)
    g, wins = c.rows()
    per_start = {}
    for i in np.flatnonzero(np.asarray(c.is_ref)[g["hap"]] == 0):
        per_start.setdefault((int(g["start"][i]), int(g["strand"][i])), set()).add(wins[i][PAD:-PAD])
    full = [v for v in per_start.values() if len(v) >= k - 8]
    c.prove(f"{starts} starts with ~{k} different rows each", len(full) == starts and len(per_start) == starts)
    expect = k * k / 2.0 ** (kb["hash_bits"] + 1)
    c.prove("expected colliding pairs per start and seed >= 1", expect >= 1.0)
    c.expected_pairs = expect
    return c


# ---- F: the memory of the hash table's size ---------------------------------------------------------------------------------
def case_table_memory():
    """One set, three scan windows: (few) 64 equal non-REF copies over three guides, (all) REF's all-N stretch where every row is
    its own group, (few) again.  -> (case with the 'few' bounds, the 'all' bounds per haplotype)"""
    c = Direct("table-memory", "NGG", 20, False)
    rng = np.random.default_rng(89)
    ref, cores, sps = _layout(rng, c.pam, 20, False, [0, 1, 0])
    nrun = 3000
    head = len(ref)
    ref = ref + "N" * nrun + _filler(rng, 40, c.pam)
    alt = _snv(_snv(_snv(ref, sps[0] + 2), sps[1] + 17), sps[2] + 11)
    few, every = (0, head - 20), (head + 30, head + nrun - 30)
    c.add(ref, is_ref=True, scan=few)
    for _ in range(64):
        c.add(alt, scan=few)
    groups, _ = c.reference()
    c.prove("few: 6 groups over 195 rows", len(groups) == 6 and len(c.rows()[0]) == 3 + 3 * 64)
    d = Direct("table-memory-all", "NGG", 20, False)
    d.add(ref, is_ref=True, scan=every)
    for _ in range(64):
        d.add(alt, scan=every)
    ga, _ = d.reference()
    d.prove("all: every row its own group, more than a 1024-slot table holds", len(ga) == len(d.rows()[0]) > 4096)
    return c, d


CASES_A = ([lambda s=s: case_stop_only(s) for s in (0, 1)] + [case_origin, lambda: case_case_only("spacer0"), lambda: case_case_only("pam-last"),
           case_iupac, case_many_identical] + [lambda n=n, m=m: case_counts(n, m) for m in (1, 2) for n in (255, 256, 257)] +
           [lambda: case_counts(1, 1)] + [lambda a=a: case_gc(*a) for a in GC_SHAPES] + [lambda: case_isolated_pams(2)])


# ---- E: panels for the template path (built on test_gpu_clusters.Panel: sites are 0-based indices into the region string) ------
def _free(taken, i, gap=200):
    return all(abs(i - t) >= gap for t in taken)


def quiet_sites(seq, lo, hi):
    """indices whose 27-base neighbourhood holds no GG / CC on REF and none after the SNV (shift 1..3 tried): no NGG guide of
    either strand can cover them -> [(index, shift)]"""
    out = []
    for i in range(lo, hi):
        w = seq[i - 27:i + 28]
        if "GG" in w or "CC" in w:
            continue
        for sh in (1, 2, 3):
            alt = "ACGT"[("ACGT".index(seq[i]) + sh) % 4]
            t = seq[i - 1] + alt + seq[i + 1]
            if "GG" not in t and "CC" not in t:
                out.append((i, sh))
                break
    return out


def loud_sites(seq, lo, hi):
    """indices ten bases inside the spacer of a + strand NGG guide"""
    return [i for i in range(lo, hi) if seq[i + 11:i + 13] == "GG"]


def panel_zero_rows(p):
    """variants in position order: zero-row, full, full, zero-row, zero-row, full, full, zero-row -> [(index, kind)]"""
    seq, n = p.seq, len(p.seq)
    quiet, loud = quiet_sites(seq, 1300, n - 1300), loud_sites(seq, 1300, n - 1300)
    out, cur = [], 1300
    for kind in "ZFFZZFFZ":
        if kind == "Z":
            i, sh = next((i, sh) for i, sh in quiet if i >= cur)
        else:
            i, sh = next(i for i in loud if i >= cur and not any(abs(i - q) < 120 for q, _ in quiet)), 1
        p.snv(i, (0, 1, 2) if len(out) % 2 else (0, 1), shift=sh)
        out.append((i, kind))
        cur = i + 200
    return out


def panel_isolated(p, per_col, first=600, step=150):
    """isolated SNVs: per_col[c] of them on column c alone, laid out column after column -> number of sites"""
    i = first
    for c, k in enumerate(per_col):
        for _ in range(k):
            p.snv(i, (c,))
            i += step
    assert i < len(p.seq) - 600
    return sum(per_col)


def panel_distinct(p, n, first=600, step=150):
    """n isolated SNVs carried by column 0, column 1 or both in turn: n distinct clusters"""
    for k in range(n):
        p.snv(first + k * step, ((0,), (1,), (0, 1))[k % 3])
    assert first + n * step < len(p.seq) - 600


def panel_reservation(p, n_sites):
    """per column one insertion that doubles its anchor base 20 bases in front of a + strand NGG: the window that starts on the
    inserted base reads like REF's at the same start, is kept by the search's first pass (it is lower case) and dropped as a
    repeat of REF - a template reservation longer than its live rows"""
    seq, taken = p.seq, []
    for i in range(1300, len(seq) - 1300):
        if seq[i + 21:i + 23] == "GG" and _free(taken, i):
            p._add(i, seq[i], seq[i] + seq[i], (len(taken),))
            taken.append(i)
            if len(taken) == n_sites:
                return taken
    raise AssertionError("not enough sites")


def panel_flanks(p, pam, guidelen, right, places):
    """per strand and entry of `places` one guide of the region with a core SNV on columns 0-3 and a second SNV d bases outside the
    core on columns 1 and 3 -> [(core index, strand, side, d)]"""
    seq, L, pl = p.seq, guidelen + len(pam), len(pam)
    taken, out = [], []
    for strand in (0, 1):
        for side, d in places:
            for q in range(1300, len(seq) - 1300):
                if pam == "NGG":
                    hit = seq[q + 1:q + 3] == "GG" if strand == 0 else seq[q:q + 2] == "CC"
                    c0 = q - guidelen if strand == 0 else q
                else:  # TTTV, PAM first
                    hit = (seq[q:q + 3] == "TTT" and seq[q + 3] in "ACG") if strand == 0 else (seq[q + 1:q + 4] == "AAA" and seq[q] in "CGT")
                    c0 = q if strand == 0 else q - guidelen
                if not hit or not _free(taken, c0, 260):
                    continue
                pamfirst = right != bool(strand)
                s1 = c0 + (pl if pamfirst else 0) + guidelen // 2
                left = (side == "5") == (strand == 0)
                s2 = c0 - d if left else c0 + L - 1 + d
                p.snv(s1, (0, 1, 2, 3), shift=2)
                p.snv(s2, (1, 3), shift=2)
                taken.append(c0)
                out.append((c0, strand, side, d))
                break
            else:
                raise AssertionError("no site")
    for c in range(4):  # a private SNV far behind the guides keeps the four copies four rows of the set
        p.snv(max(taken) + 900 + 300 * c, (c,))
    return out
