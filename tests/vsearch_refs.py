"""Case builders for tests/test_gpu_vsearch_seams.py, all on the CPU: hand-placed variants and planted guides on the seams of
the per-dirty-word view search (hawk_vsearch.hip: k_vsearch, k_ref_hits_prefix; hawk_vc.h: vc_string_fast, vc_count_run), the
expected table from the string-level oracle, and a restatement - tile_plan - of what one workgroup of k_vsearch derives for a
(row, tile): where staging starts, how many records are within reach, which words are dirty, which builder serves a word, the
survivors and valid rows of every chunk and strand, the clean runs with their shifts, the staged segments.  Every case PROVES
from that restatement, the oracle's strings and ora.scan / ora.search that it sits on the seam it is named after; a case that
drifts off its seam fails in its builder.  tests/test_vsearch_refs.py runs every builder without a GPU (all builders together:
about 2 s on one CPU core).

A region is a filler that cannot hold the PAM (A/T for NGG, C/G for TTTV) with the PAM's letters planted at chosen window
starts, as in tests/search_refs.py, so hits and survivors are exact; the rows are chromosome copies through oracle.hap_build,
as in tests/expansion_refs.py, whose Case and Row this module subclasses and reuses.  Variants stay inside the filler's
alphabet unless a builder plants a PAM letter into an allele on purpose.

tile_plan checks itself against the strings: the window starts the staged records dirty must be exactly those whose window
holds a lower-case base, every clean run's REF hits under the run's shift must be the row's own hits there, and the totals over
all rows must be the oracle's n_hits and n_candidates.

Seams that cannot be reached, and why (in REQUIRED's place):
  * `rem >= 32` in the V plane's sliding OR needs L >= 64; HAWK_MAX_CORE (include/hawk.h) limits L to 44.
  * the closing entry hp[S] of k_ref_hits_prefix is written but never read: a clean run ends at most at the row's length rounded
    up to a word plus its shift, which is at most REF's length rounded up, and the stride S keeps two spare words behind that.
    For the same reason no counted hit lies in REF's last word: every scan stops 100 bases in front of the row's end.  The stride
    cases (1024, 1028, 2048 words) pin what can be reached - the hits nearest to the scan stop, counted through a run that ends with
    the row, under a shift, and at 2048 words through the table's second round - and not the closing entry itself.
  * `hi` of a dirty range is never clipped to 32 nwt - 1: an allele lies inside the row.  The case with an insertion as the row's
    last bases proves that the range then ends in the row's last, partial word.
What the restatement also shows about the constants: a tile's strings need the records of ten positions in front of it, so ten
records back would do where VC_BACK is eleven, and they read at most up to p_hi + L + PAD - 2 <= p_hi + 52 where VC_REACH is 64;
`alt_len > 32` against `>= 32` only moves a word from one builder to the other.  Moving those in the kernel changes no table; moving
the dirty range's edge, the 96-bit cut or the guard of the XCD remap does, in the cases named after them."""
from collections import OrderedDict

import numpy as np

import expansion_refs as xr
from oracle import oracle as ora

# the geometry of hawk_vsearch.hip / hawk_vc.h / hawk_device.h
TILE = xr.TILE      # hawk_hx.h:7    HX_TW * 32 window starts per workgroup
HX_TW = xr.HX_TW    # hawk_hx.h:7    words per tile, bits of the dirty map
VC_BLOCK = 128      # hawk_vsearch.hip:22
VC_MAXV = 128       # hawk_vsearch.hip:23  records staged per tile
VC_SLOTS = 128      # hawk_vsearch.hip:24  dirty words per chunk
PAD = 10            # hawk_device.h:10     HAWK_PAD
VC_BACK = PAD + 1   # hawk_vsearch.hip:25  records staging starts in front of the tile-index record
VC_REACH = 64       # hawk_vsearch.hip:26  a record is "within reach" when o < p_hi + VC_REACH
NSEG = 64           # hawk_device.h        position-map segments staged per tile
TAIL = 64           # hawk_vsearch.hip:93  tile_end = p_lo + TILE + 64
FAST_ALLELE = 32    # hawk_vc.h:128,155    vc_string_fast declines an allele longer than a word
FAST_SPAN = 96      # hawk_vc.h:149        ... and stops at the first record with o - p0 >= 96
WINDOW_EDGE = 1     # hawk_vsearch.hip:120 a record dirties the window starts from o - L + 1 on
REF_ROUND = 1024    # hawk_vsearch.hip:390 entries k_ref_hits_prefix scans per round
stride_words = xr.stride_words

_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "V": "B", "B": "V"}


def tiles_per_row(max_len: int) -> int:
    return (stride_words(max_len) // 4 + 255) // 256


def S(r0):
    """a SNV inside the filler's alphabet on REF position r0 (relative to the padded region)"""
    return ("snv", r0)


def SNV_TO(r0, alt):
    return ("snv", r0, alt)


def D(r0, d):
    return ("del", r0, d)


def I(r0, text):
    """an insertion behind the anchor r0 of the bases `text`"""
    return ("ins", r0, text)


def emit_tile(block: int, grid: int, guard: bool = True) -> int:
    """the view tile (relative to tile0) block `block` of the emit pass takes under the XCD remap: every XCD a contiguous run of
    `per` tiles, the grid's last grid % 8 blocks their own"""
    per = grid >> 3
    if not guard or block < per * 8:
        return (block & 7) * per + (block >> 3)
    return block


def prefix_rounds(S_words: int, closing: bool = True):
    """the rounds of k_ref_hits_prefix over a table of S_words + 1 entries: [(first entry, entries written)]"""
    out, b0 = [], 0
    while b0 <= S_words if closing else b0 < S_words:
        out.append((b0, min(REF_ROUND, S_words + 1 - b0)))
        b0 += REF_ROUND
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# what one workgroup of k_vsearch derives
# ---------------------------------------------------------------------------------------------------------------------------
def string_fast(o, al, shift, start, n, every, p0c):
    """vc_string_fast's verdict for the string from row position p0c: True when it serves the word, False when the expansion's
    general builder does.  o / al / shift: the row's records (shift = rs - (o + alt_len)); start, n: the staged ones within reach."""
    if not every:
        return False
    so, sa, ss = o[start:start + n], al[start:start + n], shift[start:start + n]
    k = int(np.searchsorted(so, p0c, side="right")) - 1
    base = 0
    if k >= 0:
        base = int(ss[k])
        if sa[k] > FAST_ALLELE and p0c < so[k] + sa[k]:
            return False
    for j in range(k + 1, n):
        if so[j] - p0c >= FAST_SPAN:
            break
        if sa[j] == 1 and ss[j] == base:
            continue
        if sa[j] > FAST_ALLELE:
            return False
        base = int(ss[j])
    return True


def tile_plan(row, tile, L, pam, *, guidelen, right, scan, row_q, ref_q, valid_q, low, ref_len):
    """k_vsearch for tile `tile` of `row`, restated.  scan: the row's (scan_start, scan_stop); row_q[s]: window starts of the row's
    own PAM hits on strand s (ora.scan over its scan range); ref_q[s]: window starts of REF's hits, not cut to any range;
    valid_q[s]: window starts of the oracle's rows of this row; low: prefix counts of the row's lower-case bases."""
    o, al, rs, K = row.o, row.alt_len, row.rs, len(row.o)
    shift = rs - (o + al)
    n_len = row.len
    p_lo, p_hi = tile * TILE, (tile + 1) * TILE
    ss, se = scan
    out = dict(live=p_lo < n_len and se > ss, p_lo=p_lo, p_hi=p_hi)
    if not out["live"]:
        out.update(n_tasks=0, n_chunks=0, chunks=[], hits=0, cand=0, valid=0, words=[], runs=[], nseg=0, ovf=False)
        return out
    nwt = min((n_len - p_lo + 31) // 32, HX_TW)
    idx = xr.tile_index(row, tile, ref_len)["first"]  # the tile-index record: the last one starting at or before the tile
    before = idx                                       # records of the row before it
    back = min(VC_BACK, before)
    start = idx - back
    avail = K - start
    staged = min(avail, VC_MAXV)
    n = int((o[start:start + staged] < p_hi + VC_REACH).sum())
    every = n < VC_MAXV or avail <= VC_MAXV
    # ---- the dirty map
    jn = n if every else avail
    dirty_q = np.zeros(32 * HX_TW, dtype=bool)
    dirty_w = np.zeros(HX_TW, dtype=bool)
    clipped_lo = clipped_hi = False
    widest = 0
    for j in range(start, start + jn):
        if o[j] >= p_hi + L:
            break
        lo, hi = int(o[j]) - L + WINDOW_EDGE - p_lo, int(o[j] + al[j]) - 1 - p_lo
        if hi >= 0 and lo < 0:
            clipped_lo = True
        if hi > 32 * nwt - 1 and lo <= 32 * nwt - 1:
            clipped_hi = True
        lo, hi = max(lo, 0), min(hi, 32 * nwt - 1)
        if hi < lo:
            continue
        dirty_q[lo:hi + 1] = True
        dirty_w[lo >> 5:(hi >> 5) + 1] = True
        widest = max(widest, (hi >> 5) - (lo >> 5) + 1)
    # the staged records dirty exactly the window starts whose window holds an alt base
    qs = np.arange(p_lo, min(p_hi, n_len))
    touched = low[np.minimum(qs + L, n_len)] - low[qs] > 0
    assert np.array_equal(dirty_q[:len(qs)], touched), "the dirty window starts are not those the row's case shows"
    words = np.flatnonzero(dirty_w)
    n_tasks = len(words)
    n_chunks = (n_tasks + VC_SLOTS - 1) // VC_SLOTS
    # ---- ranges on the window start
    po = (0 if right else guidelen, guidelen if right else 0)
    slo, shi = [ss - po[0], ss - po[1]], [se - po[0], se - po[1]]
    qmin, qmax = PAD, n_len - L - PAD + 1
    rlo, rhi = [max(slo[s], qmin) for s in (0, 1)], [min(shi[s], qmax) for s in (0, 1)]
    # ---- dirty words: hits, candidates, survivors, valid rows per chunk and strand
    hits = cand = 0
    per_word = {}
    surv_all = [None, None]
    for s in (0, 1):
        q = row_q[s]
        q = q[(q >= p_lo) & (q < p_hi)]
        assert ((q >= slo[s]) & (q < shi[s])).all()
        inw = dirty_w[(q - p_lo) >> 5]
        hits += int(inw.sum())
        c = q[inw & (q >= rlo[s]) & (q < rhi[s])]
        cand += len(c)
        sv = c[low[c + L] - low[c] > 0]
        surv_all[s] = sv
        every_surv = q[(q >= rlo[s]) & (q < rhi[s])]
        every_surv = every_surv[low[every_surv + L] - low[every_surv] > 0]
        assert len(every_surv) == len(sv), "a survivor outside the dirty words"
        v = valid_q[s]
        v = v[(v >= p_lo) & (v < p_hi)]
        assert np.isin(v, sv).all(), "an oracle row that is no survivor of a dirty word"
        for w in words.tolist():
            a, b = p_lo + 32 * w, p_lo + 32 * w + 32
            per_word.setdefault(w, [0, 0, 0, 0])
            per_word[w][s] = int(((sv >= a) & (sv < b)).sum())
            per_word[w][2 + s] = int(((v >= a) & (v < b)).sum())
    chunks = []
    for ci in range(n_chunks):
        ws = words[ci * VC_SLOTS:(ci + 1) * VC_SLOTS].tolist()
        TF, TR = sum(per_word[w][0] for w in ws), sum(per_word[w][1] for w in ws)
        chunks.append(dict(words=ws, TF=TF, TR=TR, T=TF + TR, valid0=sum(per_word[w][2] for w in ws), valid1=sum(per_word[w][3] for w in ws),
                           slot_max=(max(per_word[w][0] for w in ws), max(per_word[w][1] for w in ws))))
    # ---- which builder serves a word
    fast = {}
    for w in words.tolist():
        p0c = max(p_lo + 32 * w - PAD, 0)
        fast[w] = string_fast(o, al, shift, start, n, every, p0c)
    # ---- clean runs: REF's hits under the run's shift
    def shift_at(pa):
        k = int(np.searchsorted(o, pa, side="right")) - 1
        return 0 if k < 0 else int(shift[k])

    def nd(w):
        later = words[words > w]
        return int(later[0]) if len(later) else HX_TW
    runs = []
    lomax, himin = max(rlo), min(rhi)
    for w in [-1] + words.tolist():
        pa, pb = p_lo + 32 * (w + 1), p_lo + 32 * min(nd(w), nwt)
        if pb <= pa:
            continue
        sh = shift_at(pa)
        assert shift_at(pb - 1) == sh, "a record starts inside a clean run"
        rh = rc = own = 0
        for s in (0, 1):
            a, b = max(pa, slo[s]), min(pb, shi[s])
            a2, b2 = max(pa, rlo[s]), min(pb, rhi[s])
            if a < b:
                rh += int(np.searchsorted(ref_q[s], b + sh) - np.searchsorted(ref_q[s], a + sh))
            if a2 < b2:
                rc += int(np.searchsorted(ref_q[s], b2 + sh) - np.searchsorted(ref_q[s], a2 + sh))
            own += int(((row_q[s] >= pa) & (row_q[s] < pb)).sum())
        assert rh == own, "REF's hits under the run's shift are not the row's own hits in the run"
        hits += rh
        cand += rc
        runs.append(dict(pa=pa, pb=pb, shift=sh, hits=rh, cand=rc, branch="two" if pa >= lomax and pb <= himin else "partial",
                         ref_word_hi=(pb + sh) >> 5))
    # ---- the position-map slice
    rel, _ = row.device_segments()
    rel = rel.astype(np.int64)
    k0 = int(np.searchsorted(rel, p_lo, side="right")) - 1
    nseg = 1 + int((rel[k0 + 1:] < p_lo + TILE + TAIL).sum())
    # the smallest number of records staging must go back for the builders' search to hold: the first staged record is the
    # row's first or starts at or before the first string of the tile
    p_first = max(p_lo - PAD, 0)
    need_back = 0
    while idx - need_back > 0 and o[idx - need_back] > p_first:
        need_back += 1
    assert need_back <= back, "staging does not reach back far enough"
    out.update(nwt=nwt, before=before, back=back, need_back=need_back, start=start, avail=avail, n=n, all=every, words=words.tolist(),
               n_tasks=n_tasks, n_chunks=n_chunks, chunks=chunks, fast=fast, runs=runs, hits=hits, cand=cand,
               valid=sum(c["valid0"] + c["valid1"] for c in chunks), valid0=sum(c["valid0"] for c in chunks),
               nseg=nseg, ovf=nseg > NSEG, seg_starts=rel[k0:k0 + nseg], clipped_lo=clipped_lo, clipped_hi=clipped_hi, widest=widest,
               surv=surv_all, bitmap_words=sorted({w >> 5 for w in words.tolist()}))
    return out


class Case(xr.Case):
    """expansion_refs.Case over a filler region with planted PAMs.  Variants are kept as specs - ("snv", r0[, alt]), ("del", r0, d),
    ("ins", r0, text) - and turned into (pos, ref, alt) from the region's letters when they are read, so a builder may place its
    variants first, read the row's geometry, and then plant PAM letters at row positions."""

    def __init__(self, name: str, length: int, seed: int, pam: str = "NGG", guidelen: int = 20, right: bool = False, filler: str = None):
        self._letters = None
        self._specs = []
        xr.Case.__init__(self, name, length, seed, pamlen=len(pam))
        self.pam, self.guidelen, self.right, self.L = pam, guidelen, bool(right), guidelen + len(pam)
        self.filler = filler or ("AT" if pam == "NGG" else "CG" if pam == "TTTV" else "ACGT")
        self._letters = list(np.array(list(self.filler))[self.rng.integers(0, len(self.filler), length + 300)])
        self._touch()

    def _touch(self):
        self._contig = self._refs = self._copies = self._ora = None
        self._rows, self._low, self._plans = {}, {}, {}

    # the parent's attributes, derived from the letters and the specs
    @property
    def contig_seq(self):
        if self._letters is None:
            return self._contig0
        if self._contig is None:
            self._contig = "".join(self._letters)
        return self._contig

    @contig_seq.setter
    def contig_seq(self, v):
        self._contig0 = v

    @property
    def ref(self):
        if self._letters is None:
            return self._contig0[self.startp - 1:self.stopp]
        if self._refs is None:
            self._refs = self.contig_seq[self.startp - 1:self.stopp]
        return self._refs

    @ref.setter
    def ref(self, v):
        pass

    @property
    def copies(self):
        if self._copies is None:
            key = lambda v: (v[0], v[1], v[2])
            self._copies = [tuple(sorted((self._variant(sp) for sp in cp), key=key) for cp in pair) for pair in self._specs]
        return self._copies

    @copies.setter
    def copies(self, v):
        pass

    def _variant(self, sp):
        if sp[0] == "snv":
            b = self.ref[sp[1]]
            if len(sp) > 2:
                return (self.startp + sp[1], b, sp[2])
            assert b in self.filler, f"{self.name}: a SNV on a planted PAM letter at {sp[1]}"
            return (self.startp + sp[1], b, self.filler[1 - self.filler.index(b)] if len(self.filler) == 2 else "ACGT"[("ACGT".index(b) + 1) % 4])
        if sp[0] == "del":
            return self.dele(sp[1], sp[2])
        return self.ins(sp[1], text=sp[2])

    def add(self, v0, v1=()) -> int:
        self._specs.append((list(v0), list(v1)))
        self._touch()
        return len(self._specs) - 1

    def text(self, k: int) -> str:
        return "".join(np.array(list(self.filler))[self.rng.integers(0, len(self.filler), k)])

    # ---- planting ---------------------------------------------------------------------------------------------------------
    def pam_at(self, strand: int) -> int:
        """offset of the PAM inside spacer+PAM on the + strand"""
        return 0 if (self.right != bool(strand)) else self.guidelen

    def letters(self, strand: int) -> str:
        return self.pam if strand == 0 else "".join(_COMP[ch] for ch in reversed(self.pam))

    def set_ref(self, r0: int, ch: str) -> None:
        self._letters[self.startp - 1 + r0] = ch
        self._touch()

    def plant_row(self, si: int, q: int, strand: int, c: int = 0) -> None:
        """write the PAM's letters for a guide whose window starts at row position q of copy (si, c); a letter that falls on an
        alt base must already be there (the builder chose the allele)"""
        row = self.row(si, c)
        todo = []
        for t, ch in enumerate(self.letters(strand)):
            if ch not in "ACGT":
                continue
            i = q + self.pam_at(strand) + t
            if row.seq[i].islower():
                assert row.seq[i].upper() == ch, f"{self.name}: PAM letter {ch} on an alt base {row.seq[i]} at row position {i}"
            else:
                todo.append((int(row.pm[i]) - self.startp, ch))
        for r0, ch in todo:
            self._letters[self.startp - 1 + r0] = ch
        self._touch()

    def snv_row(self, si: int, p: int, c: int = 0) -> None:
        """one more SNV of copy (si, c), on the unmodified base at row position p (a SNV moves nothing)"""
        row = self.row(si, c)
        assert row.seq[p].isupper(), f"{self.name}: row position {p} is an alt base already"
        self._specs[si][c].append(S(int(row.pm[p]) - self.startp))
        self._touch()

    def spacer(self, q: int, k: int = 5) -> int:
        """a position inside the spacer of both strands' guides at window start q"""
        return q + self.pamlen + k if self.guidelen >= self.pamlen + k + 1 else q + self.guidelen // 2

    def guide(self, si: int, q: int, strands=(0, 1), mark: bool = True, k: int = 5, c: int = 0) -> None:
        """a guide at row window start q of copy (si, c) on each of `strands`; mark: with a SNV of its own in the spacer, so that
        it is a valid row with a REF partner"""
        if mark:
            self.snv_row(si, self.spacer(q, k), c)
        for s in strands:
            self.plant_row(si, q, s, c)

    # ---- the oracle -------------------------------------------------------------------------------------------------------
    def qstart(self, pos, strand):
        pos, strand = np.asarray(pos, dtype=np.int64), np.asarray(strand, dtype=np.int64)
        return np.where(strand.astype(bool) != self.right, pos, pos - self.guidelen)

    def oracle(self):
        """(haplotypes, scan bounds, is_ref, ora.search result) of the case"""
        if self._ora is None:
            haps = self.expected_haplotypes()
            scan = [ora.scan_bounds(h["posmap"], self.startp, self.stopp, self.pamlen) for h in haps]
            is_ref = [h["samples"] == ["REF"] for h in haps]
            hs = ora.HapSet([h["seq"] for h in haps], [h["posmap"] for h in haps], is_ref, scan)
            self._ora = (haps, scan, is_ref, ora.search(hs, self.pam, self.guidelen, self.right))
        return self._ora

    @property
    def want(self):
        return self.oracle()[3]

    def hap_index(self, si: int, c: int = 0) -> int:
        seq = self.row(si, c).seq
        return next(j for j, h in enumerate(self.oracle()[0]) if h["seq"] == seq)

    def device_rows(self):
        """per device row 1 + k: (sample, copy, oracle haplotype, kept) - kept: the first row with its string, which alone is searched"""
        out, seen = [], {self.ref}
        for si, c in self.live_columns():
            seq = self.row(si, c).seq
            out.append((si, c, self.hap_index(si, c), seq not in seen))
            seen.add(seq)
        return out

    @property
    def bph(self) -> int:
        return tiles_per_row(max([len(self.ref)] + [self.row(si, c).len for si, c in self.live_columns()]))

    def rows_of(self, si: int, c: int = 0):
        """(window start, strand) of the oracle's rows of copy (si, c)"""
        g = self.want.guides
        m = g["hap"] == self.hap_index(si, c)
        return self.qstart(g["pos"][m], g["strand"][m]), g["strand"][m].astype(np.int64)

    def has_row(self, si: int, q: int, strand: int, c: int = 0) -> bool:
        qq, st = self.rows_of(si, c)
        return bool(((qq == q) & (st == strand)).any())

    def _scan_q(self, seq: str, ss: int, se: int):
        bits, bitsrc, _, _ = ora.pam_encode(self.pam)
        f, r = ora.scan(ora.encode(seq), ss, se, bits, bitsrc, self.pamlen)
        return [np.sort(self.qstart(f, np.zeros(len(f)))), np.sort(self.qstart(r, np.ones(len(r))))]

    def low(self, si: int, c: int = 0):
        if (si, c) not in self._low:
            seq = self.row(si, c).seq
            self._low[(si, c)] = np.concatenate(([0], np.cumsum(np.frombuffer(seq.encode(), dtype=np.uint8) >= ord("a"))))
        return self._low[(si, c)]

    def plan(self, si: int, tile: int, c: int = 0) -> dict:
        key = (si, tile, c)
        if key not in self._plans:
            row = self.row(si, c)
            scan = self.oracle()[1][self.hap_index(si, c)]
            if "refq" not in self._plans:
                self._plans["refq"] = self._scan_q(self.ref, 0, len(self.ref) - self.pamlen + 1)
            if ("rowq", si, c) not in self._plans:
                self._plans[("rowq", si, c)] = self._scan_q(row.seq, *scan)
            qq, st = self.rows_of(si, c)
            self._plans[key] = tile_plan(row, tile, self.L, self.pam, guidelen=self.guidelen, right=self.right, scan=scan,
                                         row_q=self._plans[("rowq", si, c)], ref_q=self._plans["refq"],
                                         valid_q=[np.sort(qq[st == 0]), np.sort(qq[st == 1])], low=self.low(si, c), ref_len=len(self.ref))
        return self._plans[key]

    def is_hit(self, si: int, q: int, strand: int, c: int = 0) -> bool:
        """the row has a PAM hit with window start q inside its scan range"""
        self.plan(si, q // TILE, c)
        return bool((self._plans[("rowq", si, c)][strand] == q).any())

    def is_survivor(self, si: int, q: int, strand: int, c: int = 0) -> bool:
        return bool((self.plan(si, q // TILE, c)["surv"][strand] == q).any())

    def tally(self) -> dict:
        """per (device row, tile): the rows the tile keeps (0 for a collapsed row); asserts that the restated totals over every row
        and REF's own are the oracle's n_hits and n_candidates"""
        _, scan, is_ref, want = self.oracle()
        rq = self._scan_q(self.ref, *scan[0])
        n = len(self.ref)
        hits = sum(len(q) for q in rq)
        cand = sum(int(((q - PAD >= 0) & (q + self.L + PAD <= n)).sum()) for q in rq)
        out, bph = {}, self.bph
        for r, (si, c, _, kept) in enumerate(self.device_rows(), 1):
            for t in range(bph):
                if not kept:
                    out[(r, t)] = 0
                    continue
                p = self.plan(si, t, c)
                hits, cand = hits + p["hits"], cand + p["cand"]
                out[(r, t)] = p["valid"]
        assert (hits, cand) == (want.n_hits, want.n_candidates), ((hits, cand), (want.n_hits, want.n_candidates))
        g = want.guides
        assert sum(out.values()) + int(np.asarray(is_ref)[g["hap"]].sum()) == len(g)
        return out

    def expected_flags(self) -> np.ndarray:
        """per oracle row: REF has a guide at this (start, strand)"""
        _, _, is_ref, want = self.oracle()
        g = want.guides
        m = np.asarray(is_ref)[g["hap"]]
        keys = set(zip(g["start"][m].tolist(), g["strand"][m].tolist()))
        return np.array([(a, b) in keys for a, b in zip(g["start"].tolist(), g["strand"].tolist())], dtype=np.uint8)

    def summary(self) -> str:
        cells = []
        for r, (si, c, _, kept) in enumerate(self.device_rows(), 1):
            for t in range(self.bph):
                p = self.plan(si, t, c)
                if kept and p["live"] and p["n_tasks"]:
                    cells.append(f"row {r} tile {t}: {p['n']} staged, {p['n_tasks']} words, T {[ch['T'] for ch in p['chunks']]}, {p['valid']} rows")
        return f"{self.name}: " + "; ".join(cells[:3])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a window that touches a variant by one base
# ---------------------------------------------------------------------------------------------------------------------------
def touch_case(name: str, pam: str, guidelen: int, right: bool, seed: int) -> Case:
    """per kind of variant (SNV, 5 inserted bases, 5 deleted bases), edge and strand one sample with one variant and one guide:
    window starts o - L (no survivor), o - L + 1 (survivor, on bit 31 of a word the variant dirties by that start alone),
    o + alt_len - 1 (survivor, on bit 0 of such a word) and o + alt_len (no survivor).  Where the PAM itself lies on the touching base the allele carries
    the PAM's letter: REF then has no guide there."""
    c = Case(name, 5200, seed, pam, guidelen, right)
    L = c.L
    slot = 0
    steps = 0
    r = 1
    while 2 * r <= L and r < 32:
        r, steps = 2 * r, steps + 1
    c.prove(f"L = {L}: the V plane's sliding OR takes {steps} doubling steps and a rest of {L - r}", 4 <= L <= 44 and L - r < 32)
    for kind in ("snv", "ins", "del"):
        al = 6 if kind == "ins" else 1
        for edge in ("o-L", "o-L+1", "o+alt_len-1", "o+alt_len"):
            for s in (0, 1):
                base = 160 + 96 * slot  # a multiple of 32: room for one scenario
                slot += 1
                if edge in ("o-L", "o-L+1"):
                    q = base + 31 if edge == "o-L+1" else base + 30  # the surviving start is the last of its word
                    o = base + 31 + L - 1
                else:
                    o = base + 64 - (al - 1)
                    q = base + 64 if edge == "o+alt_len-1" else base + 65  # the surviving start is the first of its word
                # which of the guide's PAM letters fall on the allele's bases [o, o + al)
                need = {q + c.pam_at(s) + t: ch for t, ch in enumerate(c.letters(s)) if ch in "ACGT"}
                on = {p: ch for p, ch in need.items() if o <= p < o + al}
                if kind == "snv":
                    spec = SNV_TO(o, on[o]) if o in on else S(o)
                elif kind == "del":
                    if o in on:
                        c.set_ref(o, on[o])
                    spec = D(o, 5)
                else:
                    if o in on:
                        c.set_ref(o, on[o])
                    txt = list(c.text(5))
                    for p, ch in on.items():
                        if p > o:
                            txt[p - o - 1] = ch
                    spec = I(o, "".join(txt))
                si = c.add([spec])
                row = c.row(si)
                assert int(row.o[0]) == o and int(row.alt_len[0]) == al
                c.plant_row(si, q, s)
                hit, surv = c.is_hit(si, q, s), c.is_survivor(si, q, s)
                if edge in ("o-L", "o+alt_len"):
                    c.prove(f"{kind} strand {s}: window start {edge} is a candidate and no survivor", hit and not surv and q == (o - L if edge == "o-L" else o + al)
                            and not c.has_row(si, q, s))
                else:
                    c.prove(f"{kind} strand {s}: window start {edge} is a survivor" + (" and a row" if c.has_row(si, q, s) else " (redundant with REF's guide)"),
                            hit and surv and q == (o - L + 1 if edge == "o-L+1" else o + al - 1))
                    p = c.plan(si, 0)
                    w = q // 32
                    c.prove(f"{kind} strand {s}: the survivor at {edge} is alone in a dirty word at bit {q % 32}",
                            q % 32 == (31 if edge == "o-L+1" else 0) and w in p["words"]
                            and ((w + 1 in p["words"] and w - 1 not in p["words"]) if edge == "o-L+1" else (w - 1 in p["words"] and w + 1 not in p["words"])))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 2. staging: VC_BACK, VC_MAXV, VC_REACH, the next tile's records
# ---------------------------------------------------------------------------------------------------------------------------
TWO_TILES = TILE + 1800


def back_case(name: str, n_snv: int, extra: int, seed: int) -> Case:
    """tile 1 of a row: SNVs on the n_snv row positions in front of p_lo behind a deletion further back (and `extra` SNVs between);
    guides at q = p_lo (its left pad is those bases) and at q = p_lo - 1 (tile 0's last window start)"""
    c = Case(name, TWO_TILES, seed)
    d = 7
    before = 1 + extra + n_snv - 1  # records in front of the tile-index record, the SNV at p_lo - 1
    specs = [D(TILE - 900, d)] + [S(TILE - 800 + 37 * i) for i in range(extra)]
    specs += [S(TILE + d - n_snv + i) for i in range(n_snv)]
    si = c.add(specs)
    c.snv_row(si, TILE + 5)
    row = c.row(si)
    c.prove(f"{n_snv} SNVs on row positions p_lo-{n_snv} .. p_lo-1", row.seq[TILE - n_snv:TILE].islower() and row.seq[TILE - n_snv - 1].isupper() and row.seq[TILE].isupper())
    for s in (0, 1):
        c.plant_row(si, TILE, s)
    c.plant_row(si, TILE - 1, 0)
    p = c.plan(si, 1)
    c.prove(f"{before} records precede tile 1's index record: staging goes back {min(before, VC_BACK)} (the strings need {p['need_back']})",
            p["before"] == before and p["back"] == min(before, VC_BACK) and p["need_back"] == (9 if n_snv == 10 else before) and (before < VC_BACK) == (p["start"] == 0))
    k = int(np.searchsorted(row.o, TILE, side="right")) - 1
    c.prove("the shift in force in front of tile 1 is not 0", int(row.rs[k] - row.end(k)) == d)
    c.prove("a guide at q = p_lo on both strands, kept", c.has_row(si, TILE, 0) and c.has_row(si, TILE, 1) and 0 in p["words"])
    c.prove("a guide at q = p_lo - 1 belongs to tile 0, kept", c.has_row(si, TILE - 1, 0) and (HX_TW - 1) in c.plan(si, 0)["words"])
    c.prove("word 0 of tile 1 takes the fast builder", p["fast"][0] and p["all"])
    return c


def staged_case(name: str, kind: str, seed: int) -> Case:
    """tile 0 of a row whose records start at its first base: 127 / 128 records in all, 128 within reach with more far behind, or
    129 within reach - the 129th an indel under a planted guide"""
    c = Case(name, 3 * 1024 + 600 if kind != "128_more" else TWO_TILES + 400, seed)
    at = [150 + 20 * i for i in range(127)]
    specs = [S(p) for p in at]
    if kind in ("128_all", "128_more", "129"):
        specs.append(S(150 + 20 * 127))
    if kind == "128_more":
        specs.append(S(TILE + 200))
    if kind == "129":
        specs.append(D(150 + 20 * 128, 6))
        specs.append(S(150 + 20 * 128 + 300))
    si = c.add(specs)
    row = c.row(si)
    qs = [at[3] - 8, at[126] - 8]
    if kind == "129":
        qs.append(int(row.o[128]) - 10)
        qs.append(int(row.o[128]) + 64)  # a clean stretch behind the unstaged deletion: counted under its shift
    for i, q in enumerate(qs):
        c.plant_row(si, q, i % 2)
    p = c.plan(si, 0)
    if kind == "127":
        c.prove("127 records: all staged", p["avail"] == 127 and p["n"] == 127 and p["all"])
    elif kind == "128_all":
        c.prove("avail == 128 records: all staged, n == VC_MAXV", p["avail"] == 128 and p["n"] == 128 and p["all"])
    elif kind == "128_more":
        c.prove("n == 128 staged within reach, avail > 128, nothing further within reach: the unstaged path", p["avail"] == 129 and p["n"] == 128 and not p["all"]
                and int(row.o[128]) >= TILE + VC_REACH)
    else:
        c.prove("129 records within reach: the 129th an indel read from global memory", p["avail"] == 130 and p["n"] == 128 and not p["all"]
                and int(row.chain[128]) != 0 and int(row.o[128]) < TILE)
        q = qs[2]
        c.prove("a kept guide's window covers the unstaged indel", q <= int(row.o[128]) < q + c.L and c.has_row(si, q, 0) and not p["fast"][q // 32])
        run = [r for r in p["runs"] if r["pa"] <= qs[3] < r["pb"]]
        c.prove("the clean run behind the unstaged indel is counted under its shift", len(run) == 1 and run[0]["shift"] == 6 and run[0]["hits"] >= 1
                and c.is_hit(si, qs[3], 1))
    c.prove("kept guides over the first and the last staged records", c.has_row(si, qs[0], 0) and c.has_row(si, qs[1], 1))
    return c


def reach_case(name: str, seed: int) -> Case:
    """records at o = p_hi + 63 (within reach) and p_hi + 64 (not), and the next tile's record that dirties this tile's last window
    start (o = p_hi + L - 2) against the one that does not (o = p_hi + L - 1)"""
    c = Case(name, TWO_TILES, seed)
    L = c.L
    for d in (63, 64):
        si = c.add([S(TILE - 300), S(TILE + d)])
        c.guide(si, TILE - 305, (0, 1), mark=False)
        p = c.plan(si, 0)
        c.prove(f"a record at o = p_hi + {d} is {'within' if d < VC_REACH else 'out of'} reach", p["n"] == (2 if d < VC_REACH else 1) and p["avail"] == 2 and p["all"])
        c.prove("a clean run from the tile's last dirty word to the tile's end", p["runs"][-1]["pb"] == TILE and p["runs"][-1]["pa"] > 32 * p["words"][-1] and p["nwt"] == HX_TW)
    for d, what in ((L - 2, "dirties"), (L - 1, "does not dirty")):
        si = c.add([S(TILE - 300), S(TILE + d)])
        c.plant_row(si, TILE - 1, 1)
        c.plant_row(si, TILE - 305, 0)
        p = c.plan(si, 0)
        last = (HX_TW - 1) in p["words"]
        c.prove(f"next_tile_touch: a record at o = p_hi + L - {L - d} {what} the tile's last window start",
                last == (d == L - 2) and c.is_hit(si, TILE - 1, 1) and c.has_row(si, TILE - 1, 1) == (d == L - 2))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the dirty map
# ---------------------------------------------------------------------------------------------------------------------------
def dirty_map_case(name: str, seed: int) -> Case:
    c = Case(name, TWO_TILES, seed)
    # a range across words 31 | 32 of the map: row positions around 1024 k
    for k in (1, 2):
        si = c.add([S(1024 * k + 4)])
        c.guide(si, 1024 * k - 10, (0,), mark=False)
        c.guide(si, 1024 * k + 2, (1,), mark=False)
        p = c.plan(si, 0)
        c.prove(f"a dirty range across map words {k - 1} | {k}", {32 * k - 1, 32 * k} <= set(p["words"]) and p["bitmap_words"] == [k - 1, k]
                and c.has_row(si, 1024 * k - 10, 0) and c.has_row(si, 1024 * k + 2, 1))
    # a 1200-base insertion: 38 words, a full inner mask word (32 words of the map are 1024 bases: 400 would not fill one)
    txt = list(c.text(1200))
    inside = ((3100, 0), (3100 + 512, 1), (3100 + 1000, 0))
    for q, s in inside:  # the PAMs of the guides inside the allele are part of the inserted text
        for t, ch in enumerate(c.letters(s)):
            if ch in "ACGT":
                txt[q + c.pam_at(s) + t - 3001] = ch
    si = c.add([I(3000, "".join(txt))])
    row = c.row(si)
    for q, s in ((3000 - 5, 1),) + inside + ((row.end(0) - 3, 0),):
        c.plant_row(si, q, s)
    p = c.plan(si, 0)
    c.prove("a 1200-base insertion dirties more than 32 words: a full inner mask word", p["widest"] > 32 and len(p["bitmap_words"]) >= 3
            and all(not f for w, f in p["fast"].items() if 32 * w >= 3010 and 32 * w + 32 < row.end(0)))
    c.prove("kept guides inside the long allele, in each of its map words", all(c.has_row(si, q, s) for q, s in inside))
    # the 400-base insertion of the random panels: 13 words, here across map words 1 | 2
    txt = list(c.text(400))
    for t, ch in enumerate(c.letters(1)):
        if ch in "ACGT":
            txt[2040 + c.pam_at(1) + t - 1901] = ch
    si = c.add([I(1900, "".join(txt))])
    c.plant_row(si, 2040, 1)
    p = c.plan(si, 0)
    c.prove("a 400-base insertion across map words 1 | 2 with a kept guide inside it", p["bitmap_words"] == [1, 2] and 12 <= p["widest"] <= 14 and c.has_row(si, 2040, 1)
            and not any(p["fast"][w] for w in p["words"] if 1912 <= 32 * w and 32 * w + 32 <= c.row(si).end(0)))
    # the same as the row's last bases
    n = len(c.ref)
    si = c.add([S(TILE - 200), I(n - 2, c.text(400))])
    row = c.row(si)
    p = c.plan(si, 1)
    c.prove("an insertion as the row's last bases: its range ends in the row's last word (an allele lies inside the row, so hi never passes 32 nwt - 1)",
            not p["clipped_hi"] and row.end(1) == row.len - 1 and p["nwt"] < HX_TW and p["words"][-1] == p["nwt"] - 1 and row.len % 32 != 0)
    # a record in front of tile 1 whose range is clipped at 0
    si = c.add([I(TILE - 3, c.text(10))])
    c.guide(si, TILE + 2, (0,), mark=False)
    p = c.plan(si, 1)
    c.prove("a record in front of the tile whose dirty range is clipped at 0", p["clipped_lo"] and p["words"] == [0] and c.has_row(si, TILE + 2, 0)
            and int(c.row(si).o[0]) < TILE < c.row(si).end(0))
    return c


def tasks_case(name: str, n_tasks: int, seed: int) -> Case:
    """an alt row with exactly n_tasks dirty words in tile 0; from two chunks on the first and the last chunk hold kept guides on both
    strands.  n_tasks == 0: the row's only variant lies in tile 1, tile 0 is one clean run."""
    c = Case(name, TWO_TILES if n_tasks in (0, 1024) else 32 * (n_tasks + 12) + 400, seed)
    L = c.L
    if n_tasks == 0:
        si = c.add([S(TILE + 500)])
        c.guide(si, 2000, (0, 1), mark=False)
        p = c.plan(si, 0)
        c.prove("tasks_0: no dirty word, the whole tile is one clean run", p["n_tasks"] == 0 and len(p["runs"]) == 1 and p["runs"][0]["pa"] == 0
                and p["runs"][0]["pb"] == TILE and p["runs"][0]["hits"] == 2)
        return c
    if n_tasks == 1024:
        at = [32 * w + 28 for w in range(HX_TW)]  # every word of the tile
    else:
        first = 6
        at = [32 * (first + w) + 28 for w in range(n_tasks)]  # a SNV at bit 28 dirties starts 6 .. 28 of its word only
    si = c.add([S(p) for p in at])
    # guides on both strands in the first and the last chunk: the window start 12 bits into a dirty word
    w_all = sorted({(p - L + 1) // 32 for p in at} | {p // 32 for p in at})
    w_all = [w for w in w_all if w < HX_TW]
    picks = [w_all[min(3, len(w_all) - 1)], w_all[-1]]
    if n_tasks > 2 * VC_SLOTS:
        picks.append(w_all[VC_SLOTS + 5])
    for w in dict.fromkeys(picks):
        for s in (0, 1):
            c.plant_row(si, 32 * w + 10 + s, s)
    p = c.plan(si, 0)
    c.prove(f"tasks_{n_tasks}: {n_tasks} dirty words in {-(-n_tasks // VC_SLOTS)} chunk(s)", p["n_tasks"] == n_tasks and p["n_chunks"] == -(-n_tasks // VC_SLOTS))
    if p["n_chunks"] >= 2:
        a, b = p["chunks"][0], p["chunks"][-1]
        c.prove("the first and the last chunk hold valid rows on both strands: strand 0 of the last chunk lands in front of strand 1 of the first",
                min(a["valid0"], a["valid1"], b["valid0"], b["valid1"]) >= 1)
        c.prove(f"the last chunk holds {len(b['words'])} word(s)", len(b["words"]) == n_tasks - VC_SLOTS * (p["n_chunks"] - 1))
    else:
        c.prove("valid rows on both strands", p["chunks"][0]["valid0"] >= 1 and p["chunks"][0]["valid1"] >= 1)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 4. survivors of a chunk
# ---------------------------------------------------------------------------------------------------------------------------
def survivors_case(name: str, TF: int, TR: int, seed: int) -> Case:
    """one chunk of dirty words with exactly TF + TR survivors: SNVs 32 apart, guides planted next to them"""
    per = 4  # survivors of a strand per word
    words = max(-(-TF // per), -(-TR // per), 1) + 1
    assert words <= VC_SLOTS
    c = Case(name, 32 * (words + 12) + 400, seed, pam="NGG", guidelen=5)  # L = 8: many starts per word touch one SNV
    first = 6
    si = c.add([S(32 * (first + w) + 20) for w in range(words)])
    # the SNV at bit 20 of a word dirties the starts 13 .. 20 of that word.  + strand: GG at q + 6, q + 7; - strand: CC at q, q + 1.
    # + starts 15 .. 18 put G on bits 21 .. 25, - starts 13 .. 16 put C on bits 13 .. 17: no letter on the SNV
    f = r = 0
    for w in range(words):
        b = 32 * (first + w)
        for k in range(per):
            if f < TF:
                c.plant_row(si, b + 15 + k, 0)
                f += 1
        for k in range(per):
            if r < TR:
                c.plant_row(si, b + 13 + k, 1)
                r += 1
    p = c.plan(si, 0)
    ch = p["chunks"][0]
    c.prove(f"one chunk with TF = {TF}, TR = {TR}, T = {TF + TR}: {-(-(TF + TR) // (2 * VC_BLOCK))} trip(s) of two survivors per thread",
            p["n_chunks"] == 1 and (ch["TF"], ch["TR"]) == (TF, TR))
    c.prove(f"valid rows on {'both strands' if TF and TR else 'one strand only'}", (ch["valid0"] > 0) == (TF > 0) and (ch["valid1"] > 0) == (TR > 0))
    return c


def chunk_max_case(name: str, seed: int) -> Case:
    """128 dirty words with a SNV every 16 nt under a PAM every base matches: every slot holds 32 survivors on each strand, both
    packed 16-bit fields of the chunk scan pass 255"""
    c = Case(name, 32 * 150 + 400, seed, pam="NN", guidelen=20, filler="AT")
    si = c.add([S(32 * 8 + 21 + 16 * i) for i in range(255)])
    p = c.plan(si, 0)
    ch = p["chunks"][0]
    c.prove("chunk_max: a slot holds 32 survivors on each strand, both packed 16-bit fields exceed 255", ch["slot_max"] == (32, 32) and ch["TF"] > 255 and ch["TR"] > 255
            and len(ch["words"]) == VC_SLOTS and p["n_chunks"] == 1)
    c.prove(f"T = {ch['T']} survivors in {-(-ch['T'] // (2 * VC_BLOCK))} trips, {ch['valid0'] + ch['valid1']} valid rows", ch["T"] > 4 * VC_BLOCK and ch["valid0"] > 255 and ch["valid1"] > 255)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the string builder
# ---------------------------------------------------------------------------------------------------------------------------
def strings_case(name: str, seed: int) -> Case:
    c = Case(name, 6000, seed)
    L = c.L
    slot = [0]

    def base():
        slot[0] += 1
        return 32 * (4 + 9 * slot[0])  # a word start; nine words per scenario
    # an allele of 32 / 33 bases as the record in force at p0, and as a record starting inside the string
    for k in (32, 33):
        b = base()
        si = c.add([I(b - 40, c.text(k - 1)), S(b + 45)])
        row = c.row(si)
        w = (int(row.o[0]) + PAD + 31) // 32  # the word whose string starts inside the allele: o < 32 w - PAD < o + k
        q = 32 * w + 3
        c.guide(si, q, (0, 1), mark=True, k=7)
        p = c.plan(si, 0)
        c.prove(f"an allele of {k} bases in force at p0: {'fast' if k <= FAST_ALLELE else 'general'} builder",
                int(row.o[0]) < 32 * w - PAD < row.end(0) and p["fast"][w] == (k <= FAST_ALLELE) and c.has_row(si, q, 0) and c.has_row(si, q, 1))
        b = base()
        si = c.add([I(b + 40, c.text(k - 1))])
        row = c.row(si)
        w = b // 32
        q = b + 25
        c.plant_row(si, q, 1)
        p = c.plan(si, 0)
        c.prove(f"an allele of {k} bases starting inside the string: {'fast' if k <= FAST_ALLELE else 'general'} builder",
                32 * w - PAD < int(row.o[0]) < 32 * w - PAD + FAST_SPAN and w in p["words"] and p["fast"][w] == (k <= FAST_ALLELE) and c.has_row(si, q, 1))
    # a record at o - p0 = 95 / 96: an allele of 33 bases there sends the word to the general builder only at 95
    for d in (95, 96):
        b = base()
        si = c.add([S(b + 30), I(b - PAD + d, c.text(32))])
        c.guide(si, b + 25, (0, 1), mark=False)
        p = c.plan(si, 0)
        w = b // 32
        c.prove(f"a long allele at o - p0 = {d}: {'general' if d < FAST_SPAN else 'fast'} builder", w in p["words"] and p["fast"][w] == (d >= FAST_SPAN)
                and c.has_row(si, b + 25, 0))
        # ... and a SNV there: bit 64 of the string is inside the padded window of the guide at bit 25
        b = base()
        si = c.add([S(b + 30), S(b - PAD + d)])
        c.guide(si, b + 25, (0, 1), mark=False)
        c.prove(f"a SNV at o - p0 = {d} behind a guide whose padded window covers bit 64 of the string", b + 25 - PAD + L + 2 * PAD > b - PAD + 64
                and c.has_row(si, b + 25, 0) and c.has_row(si, b + 25, 1))
    # an allele running across bit 96
    b = base()
    si = c.add([S(b + 30), I(b - PAD + 85, c.text(20))])
    c.guide(si, b + 25, (0, 1), mark=False)
    p = c.plan(si, 0)
    c.prove("an allele running across bit 96 of a string", c.row(si).end(1) > b - PAD + 96 > int(c.row(si).o[1]) and p["fast"][b // 32] and c.has_row(si, b + 25, 1))
    # a deletion followed by a SNV inside one string; two indels inside one string
    for what in ("a deletion followed by a SNV", "two indels"):
        b = base()
        if what.startswith("a deletion"):
            si = c.add([D(b + 8, 6), S(b + 8 + 6 + 9)])
        else:
            si = c.add([D(b + 8, 6), I(b + 8 + 6 + 9, c.text(4))])
        row = c.row(si)
        q = b + 2
        for s in (0, 1):
            c.plant_row(si, q, s)
        p = c.plan(si, 0)
        c.prove(f"{what} inside one string: second REF fetch" + (", then the SNV sweep" if what.startswith("a deletion") else " twice"),
                b - PAD < int(row.o[0]) < int(row.o[1]) < b - PAD + FAST_SPAN and p["fast"][b // 32] and c.has_row(si, q, 0) and c.has_row(si, q, 1)
                and q <= int(row.o[0]) and int(row.o[1]) < q + L)
    return c


def row_ends_case(name: str, seed: int) -> Case:
    """the row's first word (variants on row positions 0 .. 9 behind a deletion that moves the scan start to 10, a guide at q = 10)
    and the row ending inside a string (a variant in the last ten bases, the last valid window start)"""
    c = Case(name, 3000, seed)
    L = c.L
    n = len(c.ref)
    # deleting REF positions 1 .. 90 puts REF position 100 on row position 10
    si = c.add([D(0, 90)] + [S(91 + i) for i in range(9)])
    row = c.row(si)
    c.snv_row(si, 10 + 4)
    c.plant_row(si, 10, 1)
    scan = c.oracle()[1]
    sc = scan[c.hap_index(si)]
    p = c.plan(si, 0)
    c.prove("variants on row positions 0 .. 9, the scan starts at 10", row.seq[:10].islower() and sc[0] == 10)
    c.prove("the row's first word: a kept guide at q = 10, its string has nothing in front of position 0", c.has_row(si, 10, 1) and 0 in p["words"] and p["fast"][0])
    # the row's end: deleting 92 of the last 100 bases leaves the scan stop behind the last legal window start
    # (the oracle, like the reference, cannot place a second variant behind such a deletion: the anchor is the variant of the row's end)
    si = c.add([D(n - 100, 92)])
    row = c.row(si)
    sc = c.oracle()[1][c.hap_index(si)]
    qlast = row.len - L - PAD
    c.prove("a variant in the row's last ten bases", row.len - 10 <= int(row.o[-1]) < row.len and sc[1] > qlast + c.guidelen)
    c.snv_row(si, qlast + 6)
    c.plant_row(si, qlast, 0)
    c.plant_row(si, qlast + 1, 0)
    p = c.plan(si, 0)
    c.prove("the last valid window start is kept, the next one is a hit and no candidate", c.has_row(si, qlast, 0) and c.is_hit(si, qlast + 1, 0)
            and not c.has_row(si, qlast + 1, 0) and p["words"][-1] == p["nwt"] - 1 and row.len % 32 != 0)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the position map
# ---------------------------------------------------------------------------------------------------------------------------
def segments_case(name: str, nseg: int, seed: int) -> Case:
    """tile 0 of a row in which exactly nseg segments start before tile_end (Row.device_segments: with the extra segment the device
    opens behind every insertion); guides whose q and q + L lie on either side of a segment start"""
    c = Case(name, TWO_TILES, seed)
    L = c.L
    # a deletion opens one segment, an insertion of k bases k + 1
    specs = [D(400 + 90 * i, 3) for i in range(nseg - 1 - 4)] + [I(400 + 90 * (nseg - 5), c.text(3))]
    specs.append(S(TILE + 900))
    si = c.add(specs)
    row = c.row(si)
    rel = row.device_segments()[0].astype(np.int64)
    picks = [int(rel[1]), int(rel[len(rel) // 2]), int(rel[nseg - 5])]
    for j, s0 in enumerate(picks):
        c.plant_row(si, s0 - 12, j % 2)  # q < segment start <= q + L
    p = c.plan(si, 0)
    c.prove(f"segments_{nseg}: {nseg} segments start before tile_end -> {'posmap_global' if nseg > NSEG else 'staged'}", p["nseg"] == nseg and p["ovf"] == (nseg > NSEG)
            and len(rel) == nseg)
    c.prove("kept guides whose q and q + L lie on either side of a segment start", all(c.has_row(si, s0 - 12, j % 2) and s0 - 12 < s0 <= s0 - 12 + L for j, s0 in enumerate(picks)))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 7. clean runs and totals
# ---------------------------------------------------------------------------------------------------------------------------
def runs_case(name: str, seed: int) -> Case:
    c = Case(name, TILE - 2000, seed)
    n = len(c.ref)
    for kind in ("del", "ins"):
        si = c.add([S(50), (D(3000, 9) if kind == "del" else I(3000, c.text(9))), S(9000), S(n - 60)])
        for q, s in ((500, 0), (520, 1), (6000, 0), (6100, 1), (12_000, 0), (12_100, 1), (n - 150, 0), (n - 180, 1)):
            c.plant_row(si, q, s)
        p = c.plan(si, 0)
        runs = p["runs"]
        sc = c.oracle()[1][c.hap_index(si)]
        c.prove(f"{kind}: a clean run that contains scan_start and one that contains scan_stop take the partial-range branch",
                any(r["pa"] < sc[0] < r["pb"] and r["branch"] == "partial" for r in runs) and any(r["pa"] < sc[1] - c.guidelen < r["pb"] and r["branch"] == "partial" for r in runs))
        inner = [r for r in runs if r["branch"] == "two" and r["hits"] >= 2]
        c.prove(f"{kind}: a run wholly inside both strands' ranges behind the indel, shift {'+9' if kind == 'del' else '-9'}: the two-entry branch",
                any(r["shift"] == (9 if kind == "del" else -9) for r in inner))
        c.prove(f"{kind}: the last run ends with the row inside the tile", runs[-1]["pb"] == 32 * p["nwt"] and p["nwt"] < HX_TW and p["words"][-1] < p["nwt"] - 1)
    return c


def stride_case(name: str, S_words: int, seed: int) -> Case:
    """REF of a length whose stride is S_words: k_ref_hits_prefix closes its table alone in a round (1024, 2048) or inside one
    (1028).  The scan stops 100 bases in front of a row's end, so no counted hit lies in REF's last word; the hits nearest to it are
    counted through an alt row's last clean run, under a shift, up to the scan stop."""
    n = 32 * (S_words - 3) - 7
    c = Case(name, n, seed)
    rounds = prefix_rounds(S_words)
    c.prove(f"REF of {n} bases: a stride of {S_words} words, the closing entry {'alone in its round' if S_words % 1024 == 0 else 'inside a round'}",
            stride_words(n) == S_words and sum(k for _, k in rounds) == S_words + 1 and (rounds[-1][1] == 1) == (S_words % 1024 == 0))
    si = c.add([S(700), D(n - 400, 80)])
    row = c.row(si)
    sc = c.oracle()[1][c.hap_index(si)]
    q = sc[1] - 5
    c.plant_row(si, q, 1)
    c.plant_row(si, q - 40, 0)
    c.guide(si, 3000, (0, 1))
    t = (row.len - 1) // TILE
    p = c.plan(si, t)
    run = p["runs"][-1]
    c.prove("the row's last clean run ends with the row, holds the last hits in front of the scan stop and is counted under the deletion's shift",
            run["pb"] == t * TILE + 32 * p["nwt"] and run["hits"] == 2 and run["shift"] == 80 and run["branch"] == "partial" and c.is_hit(si, q, 1))
    c.prove(f"the last entry a run can read is {(sc[1] + 80) >> 5} of {S_words}: the closing one is never read", (sc[1] + 80) >> 5 < S_words - 1)
    if S_words > 1028:
        c.prove("entries of the table's second round are read: the carry between rounds", (q + 80) >> 5 > 1024)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 8. launch: the XCD remap of the emit grid, empty tiles, collapsed rows
# ---------------------------------------------------------------------------------------------------------------------------
def launch_case(name: str, n_tiles: int, seed: int) -> Case:
    """n_tiles alt rows of one tile each; view tile i keeps i % 3 rows"""
    c = Case(name, 2400, seed)
    for i in range(n_tiles):
        si = c.add([S(2150 + 3 * i)])  # a private variant: every row is a row of its own
        for k in range(i % 3):
            c.guide(si, 200 + 40 * i + 800 * k, (k,), mark=True)
    t = c.tally()
    c.prove(f"{n_tiles} view tiles: per = {n_tiles >> 3}, {n_tiles - 8 * (n_tiles >> 3)} in the tail of the remap", c.bph == 1 and len(t) == n_tiles)
    c.prove("view tile i keeps i % 3 rows", all(t[(1 + i, 0)] == i % 3 for i in range(n_tiles)))
    took = sorted(emit_tile(b, n_tiles) for b in range(n_tiles))
    loose = sorted(emit_tile(b, n_tiles, guard=False) for b in range(n_tiles))
    tail = n_tiles % 8 and n_tiles > 1
    c.prove("the remap with its guard deals every tile once" + ("; without it a tile with rows is left out" if tail else "; the grid has no tail to guard"),
            took == list(range(n_tiles)) and ((loose != took and any(t[(1 + i, 0)] for i in set(took) - set(loose))) if tail else loose == took))
    if n_tiles >= 5:
        c.prove("a tile of zero rows between tiles with rows", t[(3, 0)] > 0 and t[(4, 0)] == 0 and t[(5, 0)] > 0)
    return c


def collapsed_case(name: str, seed: int) -> Case:
    """two samples carrying the same copy: the second row collapses onto the first and is skipped"""
    c = Case(name, 3000, seed)
    a = c.add([S(1000), D(1500, 4)])
    c.guide(a, 990, (0, 1), mark=False)
    c.add([S(1000), D(1500, 4)])
    d = c.add([S(2000)])
    c.guide(d, 1990, (0,), mark=False)
    rows = c.device_rows()
    c.prove("two samples carry the same copy: the collapsed row is skipped", [r[3] for r in rows] == [True, False, True] and rows[0][2] == rows[1][2]
            and len(c.oracle()[0]) == 3)
    t = c.tally()
    c.prove("the rows on either side of it keep rows", t[(1, 0)] >= 2 and t[(2, 0)] == 0 and t[(3, 0)] >= 1)
    return c


def default_route_case(name: str, seed: int) -> Case:
    """a two-sample panel: fewer than HAWK_CLUSTER_MIN_SHARE instances per distinct cluster, the dictionary is declined"""
    c = Case(name, 3000, seed)
    a = c.add([S(800), D(1200, 5)], [S(2100)])
    c.guide(a, 790, (0, 1), mark=False)
    c.guide(a, 2090, (1,), mark=False, c=1)
    b = c.add([I(1700, c.text(4))])
    c.guide(b, 1690, (0,), mark=False)
    t = c.tally()
    c.prove("a two-sample panel of three distinct copies, each with rows", len(c.device_rows()) == 3 and all(t[(r, 0)] >= 1 for r in (1, 2, 3)))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
CASES = OrderedDict()
REQUIRED = {}


def _reg(name, fn, required):
    CASES[name] = fn
    REQUIRED[name] = required


TOUCH_REQ = [f"{k} strand {s}: window start {e}" for k in ("snv", "ins", "del") for s in (0, 1) for e in ("o-L is", "o-L+1 is a survivor", "o+alt_len-1 is a survivor", "o+alt_len is")]
TOUCH_REQ += ["snv strand 0: window start o-L+1 is a survivor and a row", "snv strand 1: window start o+alt_len-1 is a survivor and a row", "alone in a dirty word at bit 31",
              "alone in a dirty word at bit 0"]
for _i, (_pam, _g, _right) in enumerate((("NGG", 1, False), ("NGG", 20, False), ("TTTV", 23, True), ("NGG", 29, False), ("NGG", 30, False), ("NGG", 41, False))):
    _name = f"touch_L{_g + len(_pam)}"
    _reg(_name, (lambda nm, p, g, r, sd: lambda: touch_case(nm, p, g, r, sd))(_name, _pam, _g, _right, 9900 + _i), [f"L = {_g + len(_pam)}"] + TOUCH_REQ)
_reg("back_full", lambda: back_case("back_full", 10, 2, 9911), ["12 records precede", "goes back 11", "shift in force", "q = p_lo on both strands", "q = p_lo - 1"])
_reg("back_short", lambda: back_case("back_short", 5, 0, 9912), ["5 records precede", "goes back 5", "q = p_lo on both strands"])
for _k, _req in (("127", "127 records"), ("128_all", "avail == 128"), ("128_more", "avail > 128"), ("129", "129th an indel")):
    _reg(f"staged_{_k}", (lambda k: lambda: staged_case(f"staged_{k}", k, 9920 + len(k)))(_k),
         [_req, "first and the last staged"] + (["covers the unstaged indel", "counted under its shift"] if _k == "129" else []))
_reg("reach", lambda: reach_case("reach", 9930), ["p_hi + 63 is within", "p_hi + 64 is out of", "L - 2 dirties", "L - 1 does not dirty", "to the tile's end"])
_reg("dirty_map", lambda: dirty_map_case("dirty_map", 9931), ["map words 0 | 1", "map words 1 | 2", "full inner mask word", "inside the long allele", "400-base insertion across map words", "ends in the row's last word", "clipped at 0"])
for _n in (0, 1, 127, 128, 129, 256, 257, 1024):
    _reg(f"tasks_{_n}", (lambda n: lambda: tasks_case(f"tasks_{n}", n, 9940 + n % 97))(_n),
         [f"tasks_{_n}: {_n} dirty words in {-(-_n // 128)} chunk(s)" if _n else "tasks_0: no dirty word"] + (["strand 0 of the last chunk lands in front"] if _n > 128 else []))
for _tf, _tr in ((255, 0), (200, 56), (200, 57), (256, 256), (256, 257), (63, 9), (64, 9), (65, 9), (0, 9), (9, 0)):
    _name = f"surv_{_tf}_{_tr}"
    _reg(_name, (lambda nm, f, r: lambda: survivors_case(nm, f, r, 9950 + f + 3 * r))(_name, _tf, _tr), [f"TF = {_tf}, TR = {_tr}", "valid rows on"])
_reg("chunk_max", lambda: chunk_max_case("chunk_max", 9960), ["a slot holds 32", "trips"])
_reg("strings", lambda: strings_case("strings", 9961),
     ["32 bases in force at p0: fast", "33 bases in force at p0: general", "32 bases starting inside the string: fast", "33 bases starting inside the string: general",
      "o - p0 = 95: general", "o - p0 = 96: fast", "SNV at o - p0 = 95", "SNV at o - p0 = 96", "across bit 96", "a deletion followed by a SNV", "two indels"])
_reg("row_ends", lambda: row_ends_case("row_ends", 9962), ["scan starts at 10", "row's first word", "last ten bases", "last valid window start"])
for _n in (64, 65):
    _reg(f"segments_{_n}", (lambda n: lambda: segments_case(f"segments_{n}", n, 9970 + n))(_n), [f"{_n} segments start before tile_end -> {'staged' if _n <= 64 else 'posmap_global'}", "either side of a segment start"])
_reg("runs", lambda: runs_case("runs", 9980), ["del: a clean run that contains scan_start", "ins: a clean run that contains scan_start", "shift +9", "shift -9", "ends with the row"])
for _s in (1024, 1028, 2048):
    _reg(f"stride_{_s}", (lambda s: lambda: stride_case(f"stride_{s}", s, 9990 + s % 7))(_s), [f"stride of {_s} words", "ends with the row", "closing one is never read"] + (["carry between rounds"] if _s == 2048 else []))
for _n in (1, 7, 8, 9, 15, 16, 17):
    _reg(f"launch_{_n}", (lambda n: lambda: launch_case(f"launch_{n}", n, 10_000 + n))(_n), [f"{_n} view tiles", "i % 3 rows", "deals every tile once"])
_reg("collapsed", lambda: collapsed_case("collapsed", 10_020), ["collapsed row is skipped", "either side"])
_reg("default_route", lambda: default_route_case("default_route", 10_021), ["two-sample panel"])
