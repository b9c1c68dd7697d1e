"""Case builders and references for tests/test_gpu_expansion.py, all on the CPU: hand-placed variants on the seams of the
device haplotype expansion (hawk_expand.hip, hawk_hx.h, hawk_meta.hip), the expected rows from the string-level oracle
(oracle.hap_build per chromosome copy), and a restatement of the per-tile arithmetic of k_hx_index so that every case can
PROVE - from the oracle's strings and position maps alone - that it sits on the seam it is named after.  A case whose
variants drift off their seam fails in its builder; tests/test_expansion_refs.py runs every builder without a GPU."""
from collections import OrderedDict

import numpy as np

from crisprhawk_hip import synth
from crisprhawk_hip.hapset import segments_from_posmap
from oracle import oracle as ora

# the geometry of hawk_hx.h
HX_TW = 1024                # output words per tile
TILE = HX_TW * 32           # 32768 output positions
HX_MAXV = 96                # records staged per tile
HX_RW = HX_TW + 64          # REF words staged per plane
QUAD = 128                  # output positions one thread builds (four words)
SEG_ROUND = 256             # indels k_seg_fill / k_seg_count take per round
SCAN_ROUND = 4096           # counts k_scan_u32 takes per round
IUPAC15 = "ACMGRSVTWYHKDBN"  # nibble values 1 .. 15 in order


def stride_words(max_len: int) -> int:
    """words per row of a set whose longest row has max_len bases (two spare words, whole 16-byte quads)"""
    return ((max_len + 31) // 32 + 2 + 3) // 4 * 4


def planes_from_string(seq: str, S: int) -> np.ndarray:
    """[5, S] uint32: the four base planes from the oracle's encoder, the V plane from the string's case; bit i of word w is
    position 32 w + i, words behind the row are zero."""
    n = len(seq)
    nib = ora.encode(seq)
    low = np.frombuffer(seq.encode("ascii"), dtype=np.uint8)
    low = (low >= ord("a")) & (low <= ord("z"))  # str.islower, letter by letter
    bits = np.zeros((5, S * 32), dtype=np.uint8)
    for p in range(4):
        bits[p, :n] = (nib >> p) & 1
    bits[4, :n] = low
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(5, S)


def canonical_segments(rel, gen):
    """(rel, gen) without the breaks that change nothing: a segment that continues its predecessor at unit slope.  The device
    opens one behind every insertion (where REF resumes at anchor + 1, which the last inserted base - mapped to the anchor -
    already leads to); segments_from_posmap cannot see such a break."""
    rel, gen = np.asarray(rel, dtype=np.int64), np.asarray(gen, dtype=np.int64)
    keep = np.ones(len(rel), dtype=bool)
    keep[1:] = (gen[1:] - gen[:-1]) != (rel[1:] - rel[:-1])
    return rel[keep].astype(np.uint32), gen[keep]


class Row:
    """One chromosome copy through the oracle: cased string, position map, and per carried variant where it starts in the
    row (`o`), where REF resumes behind it (`rs`) and how long its alt allele is - the fields of a device record, here read
    off the oracle's position map and checked against the prefix sum of the length changes."""

    def __init__(self, ref: str, startp: int, variants):
        self.variants = list(variants)
        self.seq, self.pm = ora.hap_build(ref, startp, self.variants)
        self.len = len(self.seq)
        pos = np.array([v[0] for v in self.variants], dtype=np.int64)
        reflen = np.array([len(v[1]) for v in self.variants], dtype=np.int64)
        self.alt_len = np.array([len(v[2]) for v in self.variants], dtype=np.int64)
        self.chain = self.alt_len - reflen
        self.r0 = pos - startp
        self.span = np.where(self.chain < 0, 1 - self.chain, 1)
        self.rs = self.r0 + self.span
        # the first row position that maps to the variant's anchor: where its alt allele starts
        self.o = np.searchsorted(self.pm, pos, side="left").astype(np.int64)
        assert np.array_equal(self.pm[self.o], pos), "a carried variant's anchor is missing from the oracle's position map"
        assert np.array_equal(self.o, self.r0 + np.concatenate(([0], np.cumsum(self.chain)[:-1]))), "output starts drifted"
        for o, n in zip(self.o.tolist(), self.alt_len.tolist()):
            assert self.seq[o:o + n].islower(), "an alt allele is not where the position map says"
        assert self.len == len(ref) + int(self.chain.sum())

    def end(self, i: int) -> int:
        """first row position behind variant i's alt allele"""
        return int(self.o[i] + self.alt_len[i])

    def device_segments(self):
        """The segment list the device writes for this row, from the oracle's position map: every break of the map, and behind
        every insertion the position where REF resumes if the row still has it (k_seg_fill opens n + 1 segments for n inserted
        bases; the last of them continues the map at unit slope, so it is no break of the map itself)."""
        rel, _ = segments_from_posmap(self.pm)
        resume = [self.end(i) for i in np.flatnonzero(self.chain > 0).tolist() if self.end(i) < self.len]
        rel = np.union1d(rel.astype(np.int64), np.asarray(resume, dtype=np.int64))
        return rel.astype(np.uint32), self.pm[rel].copy()


def tile_index(row: Row, wb: int, ref_len: int) -> dict:
    """k_hx_index for tile wb of a row, restated: which records the tile needs, whether they fit the staged ones (HX_ALL),
    whether a record starts at or before the tile (HX_HEAD), the staged REF window [ws, we) and whether it fits (HX_FITS)."""
    o, K = row.o, len(row.o)
    p_lo, p_hi = wb * TILE, (wb + 1) * TILE
    a = int(np.searchsorted(o, p_lo, side="right"))  # first index with o > p_lo
    c = int(np.searchsorted(o, p_hi, side="left"))   # first index with o >= p_hi
    first = max(a - 1, 0)
    want = c - first
    n = min(max(want, 0), HX_MAXV)

    def refpos(k, p):
        if k < 0:
            return p
        e = row.end(k)
        return int(row.rs[k]) + max(p - e, 0)
    plast = min(p_hi, row.len) - 1
    ws, we, fits = 0, None, True
    if plast >= p_lo:
        ws = (refpos(a - 1, p_lo) >> 5) & ~3
        we = (refpos(c - 1, plast) >> 5) + 2
        fits = we - ws <= HX_RW
    every = n == want or want < 0
    ref_S = stride_words(ref_len)
    return dict(a=a, c=c, first=first, want=want, n=n, head=a - 1 >= 0, all=every, fits=fits, ws=ws, we=we,
                fast=fits and every, K=K, live=plast >= p_lo, raw_ws=(refpos(a - 1, p_lo) >> 5) if plast >= p_lo else None,
                window_clamped=plast >= p_lo and ws + HX_RW > ref_S)


class Case:
    """A region, its samples and what each chromosome copy carries.  `prove(label, cond)` records a seam condition that held;
    a false one fails the builder."""

    def __init__(self, name: str, length: int, seed: int, patches=None, pamlen: int = 3):
        self.name, self.pamlen = name, pamlen
        rng = np.random.default_rng(seed)
        self.rng = rng
        bed_start = 201
        contig = list(synth.random_sequence(rng, length + 300))
        for at, text in (patches or {}).items():  # relative to the padded region
            contig[100 + at:100 + at + len(text)] = text
        self.contig_seq = "".join(contig)
        self.bed_start, self.bed_stop = bed_start, length
        self.startp, self.stopp = bed_start - 100, length + 100
        self.ref = self.contig_seq[self.startp - 1:self.stopp]
        assert len(self.ref) == length
        self.copies = []   # per sample (variants of copy 0, variants of copy 1)
        self.proved = []
        self.expect_error = None  # "overlap" / "clamp": the API refuses the plan with that status
        self._rows = {}

    # ---- variants by position relative to the padded region -------------------------------------------------------------
    def snv(self, r0: int, alt: str = None):
        b = self.ref[r0]
        return (self.startp + r0, b, alt if alt is not None else "ACGT"[("ACGT".index(b) + 1) % 4])

    def dele(self, r0: int, d: int):
        assert d >= 1 and r0 + d < len(self.ref)
        return (self.startp + r0, self.ref[r0:r0 + d + 1], self.ref[r0])

    def ins(self, r0: int, k: int = None, text: str = None):
        """an insertion whose alt allele (anchor included) has k bases"""
        if text is None:
            text = "".join("ACGT"[b] for b in self.rng.integers(0, 4, k - 1))
        return (self.startp + r0, self.ref[r0], self.ref[r0] + text)

    def add(self, v0, v1=()) -> int:
        """a sample whose copy 0 carries v0 and whose copy 1 carries v1; returns the sample's index"""
        key = lambda v: (v[0], v[1], v[2])
        self.copies.append((sorted(v0, key=key), sorted(v1, key=key)))
        return len(self.copies) - 1

    def prove(self, label: str, cond) -> None:
        assert bool(cond), f"{self.name}: off its seam: {label}"
        self.proved.append(label)

    # ---- what the oracle makes of it ------------------------------------------------------------------------------------
    @property
    def samples(self):
        return [f"S{i:04d}" for i in range(len(self.copies))]

    def row(self, si: int, c: int = 0) -> Row:
        if (si, c) not in self._rows:
            self._rows[(si, c)] = Row(self.ref, self.startp, self.copies[si][c])
        return self._rows[(si, c)]

    def tile(self, si: int, wb: int, c: int = 0) -> dict:
        return tile_index(self.row(si, c), wb, len(self.ref))

    def live_columns(self):
        """[(sample, copy)] of the chromosome copies that carry something, in column order: device row 1 + k"""
        return [(si, c) for si in range(len(self.copies)) for c in (0, 1) if self.copies[si][c]]

    def expected_haplotypes(self):
        """tests/util.py oracle_haplotypes from the per-copy lists: REF, then per sample copy 0 / copy 1 (one entry when both
        hold the same cased string), collapsed by identical string keeping the first member's position map"""
        entries = [(self.ref, np.arange(self.startp, self.startp + len(self.ref), dtype=np.int64), "REF")]
        ref_row = None
        for si, (v0, v1) in enumerate(self.copies):
            if not v0 and not v1:
                continue
            s = self.samples[si]
            rows = []
            for c, v in ((0, v0), (1, v1)):
                if v:
                    rows.append(self.row(si, c))
                else:
                    ref_row = ref_row or Row(self.ref, self.startp, [])
                    rows.append(ref_row)
            if rows[0].seq == rows[1].seq:
                entries.append((rows[0].seq, rows[0].pm, f"{s}:1|1"))
            else:
                entries.append((rows[0].seq, rows[0].pm, f"{s}:1|0"))
                entries.append((rows[1].seq, rows[1].pm, f"{s}:0|1"))
        groups = OrderedDict()
        for seq, pm, smp in entries:
            groups.setdefault(seq, []).append((pm, smp))
        return [dict(seq=seq, posmap=m[0][0], samples=["REF"] if seq.isupper() else sorted({x[1] for x in m}))
                for seq, m in groups.items()]

    def sites(self):
        """the distinct (pos, ref, alt) of all copies in position order, and G[site, sample, copy]"""
        all_v = sorted({v for v0, v1 in self.copies for v in list(v0) + list(v1)})
        index = {v: i for i, v in enumerate(all_v)}
        G = np.zeros((len(all_v), len(self.copies), 2), dtype=np.uint8)
        for si, cp in enumerate(self.copies):
            for c in (0, 1):
                for v in cp[c]:
                    G[index[v], si, c] = 1
        return all_v, G

    def region(self) -> synth.SynthRegion:
        reg = synth.SynthRegion("chrE", self.contig_seq, self.bed_start, self.bed_stop)
        assert (reg.startp, reg.stopp, reg.sequence) == (self.startp, self.stopp, self.ref)
        reg.samples = self.samples
        all_v, G = self.sites()
        reg.variants = [synth.VariantSite(p, r, a, 0.5, G[i]) for i, (p, r, a) in enumerate(all_v)]
        reg.gt_matrix = np.ascontiguousarray(G.reshape(len(all_v), -1))
        return reg

    def fixture(self) -> dict:
        """the raw inputs in the form tests/util.py oracle_haplotypes reads"""
        all_v, G = self.sites()
        return dict(region_seq=self.ref, startp=self.startp, samples=self.samples,
                    variants=[[p, r, a, 0.5, ["".join(str(int(x)) for x in row) for row in G[i]]] for i, (p, r, a) in enumerate(all_v)])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. tile seams: the binary searches of k_hx_index and HX_HEAD
# ---------------------------------------------------------------------------------------------------------------------------
def case_tile_seams() -> Case:
    c = Case("tile_seams", 3 * TILE - 1000, 8101)
    for seam in (TILE, 2 * TILE):
        wb = seam // TILE
        for d in (-1, 0, 1):
            for kind in ("snv", "del", "ins"):
                at = seam + d
                v = c.snv(at) if kind == "snv" else c.dele(at, 5) if kind == "del" else c.ins(at, 6)
                si = c.add([v])
                row, t, prev = c.row(si), c.tile(si, wb), c.tile(si, wb - 1)
                c.prove(f"{kind} starts at p_hi{d:+d} of tile {wb - 1}", int(row.o[0]) == at and row.seq[at].islower()
                        and not row.seq[at - 1].islower())
                if d <= 0:  # at or before the tile: the tile's head record
                    c.prove(f"{kind} at p_lo{d:+d} is the head of tile {wb}", t["head"] and t["first"] == 0 and t["n"] == 1)
                else:
                    c.prove(f"{kind} at p_lo+1: tile {wb} has no head", not t["head"] and t["a"] == 0 and t["n"] == 1)
                if d < 0:
                    c.prove(f"{kind} at p_hi-1 is inside tile {wb - 1}", prev["c"] == 1 and prev["n"] == 1)
                    c.prove(f"the only record of the row lies in an earlier tile than {wb}", t["c"] == t["a"] == 1)
                else:
                    c.prove(f"{kind} at p_hi{d:+d} is not needed by tile {wb - 1}", prev["c"] == 0 and prev["n"] == 0 and not prev["head"])
                if kind == "del" and d == -1:
                    c.prove("a deletion anchored on the last position of a tile", int(row.o[0]) == seam - 1 and row.pm[seam] - row.pm[seam - 1] == 6)
        # an insertion of the previous tile reaching across the seam
        for reach, alt_len, label in ((1, 32, "plane bits"), (31, 32, "plane bits"), (1, 11, "plane bits"), (1, 41, "text"), (31, 41, "text"),
                                      (32, 42, "text"), (33, 43, "text"), (200, 210, "text"), (2 * QUAD + 3, 3 * QUAD, "text")):
            at = seam + reach - alt_len
            si = c.add([c.ins(at, alt_len)])
            row, t = c.row(si), c.tile(si, wb)
            c.prove(f"insertion allele ({label}) reaches {reach} bases across seam {seam}",
                    int(row.o[0]) < seam and row.end(0) == seam + reach and row.seq[seam + reach - 1].islower()
                    and not row.seq[seam + reach].islower() and (alt_len <= 32) == (label == "plane bits") and t["head"])
            if reach >= QUAD:
                c.prove("a thread's four words lie inside one allele", int(row.o[0]) <= seam and row.end(0) >= seam + QUAD)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 2. word and quad seams inside a tile (hx_words_t)
# ---------------------------------------------------------------------------------------------------------------------------
def case_word_seams() -> Case:
    c = Case("word_seams", 9000, 8102)
    quad = 40  # words 40 .. 43 are one thread's
    for w, wl in ((quad, "first"), (quad + 3, "last")):
        for bit in (0, 31):
            for kind in ("snv", "del", "ins"):
                at = 32 * w + bit
                si = c.add([c.snv(at) if kind == "snv" else c.dele(at, 3) if kind == "del" else c.ins(at, 4)])
                o = int(c.row(si).o[0])
                c.prove(f"{kind} at bit {bit} of the {wl} word of a quad", o % 32 == bit and (o // 32) % 4 == (0 if wl == "first" else 3))
    # several variants starting inside one word
    base = 32 * 81
    for n in (2, 3, 32):
        at = [base + 5, base + 20] if n == 2 else [base + 1, base + 2, base + 30] if n == 3 else list(range(base, base + 32))
        si = c.add([c.snv(p) for p in at])
        o = c.row(si).o
        c.prove(f"{n} SNVs start inside one word", len(o) == n and len(set((o // 32).tolist())) == 1)
    # an indel, then a SNV in the same word: the word is copied again behind the indel and not behind the SNV
    for kind in ("del", "ins"):
        first = c.dele(base + 3, 7) if kind == "del" else c.ins(base + 3, 5)
        si = c.add([first, c.snv(base + 3 + 8 + (0 if kind == "ins" else 8))])
        row = c.row(si)
        c.prove(f"{kind} then SNV in one word: re-copy taken, then skipped",
                row.o[0] // 32 == row.o[1] // 32 and row.o[0] % 32 > 0 and row.end(0) % 32 != 0 and row.end(0) // 32 == row.o[0] // 32
                and row.chain[0] != 0 and row.chain[1] == 0)
    for start_bit in (5, 0):  # starting inside the word, and exactly at it
        si = c.add([c.ins(base + start_bit, 32 - start_bit), c.snv(base + 40)])
        row = c.row(si)
        c.prove(f"insertion from bit {start_bit} ends exactly at a word end", int(row.o[0]) % 32 == start_bit and row.end(0) % 32 == 0
                and row.end(0) // 32 == row.o[0] // 32 + 1)
    for bit in (4, 30, 31):  # the SNV in the same word, in its last bit, and in the first bit of the next
        si = c.add([c.dele(base + bit, 9), c.snv(base + bit + 10)])
        row = c.row(si)
        c.prove(f"deletion at bit {bit} immediately followed by a SNV", int(row.o[1]) == int(row.o[0]) + 1 and int(row.o[0]) % 32 == bit
                and row.seq[int(row.o[0]):int(row.o[0]) + 2].islower())
    # a deletion and an insertion whose copy behind them starts a word: the variant starts exactly at the word (next_o <= wp0)
    si = c.add([c.dele(base, 40), c.ins(base + 64 + 40, 3), c.snv(base + 96 + 40 - 2)])
    row = c.row(si)
    c.prove("records starting exactly at a word start", all(int(x) % 32 == 0 for x in row.o))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 3. allele lengths: plane bits up to 32 bases, the allele text beyond
# ---------------------------------------------------------------------------------------------------------------------------
def case_allele_lengths() -> Case:
    c = Case("allele_lengths", TILE + 3000, 8103)
    for n in (31, 32, 33, 64, 65):
        for bit in (0, 7, 31):
            at = 32 * 50 + bit
            si = c.add([c.ins(at, n), c.snv(at + 70)])
            row = c.row(si)
            c.prove(f"insertion of alt_len {n} from bit {bit} ({'plane bits' if n <= 32 else 'text'})",
                    int(row.alt_len[0]) == n and int(row.o[0]) % 32 == bit and row.seq[at:at + n].islower() and not row.seq[at + n].islower())
    si = c.add([c.ins(TILE - 150, 400)])
    row = c.row(si)
    c.prove("an allele of 400 bases across word, quad and tile seams",
            int(row.o[0]) < TILE < row.end(0) and (row.end(0) - 1) // QUAD - int(row.o[0]) // QUAD >= 3 and int(row.o[0]) % 32 != 0)
    for reps, path in ((1, "plane bits"), (3, "text")):
        for bit in (0, 13):
            at = 32 * 120 + bit
            si = c.add([c.ins(at, text=IUPAC15 * reps)])
            row = c.row(si)
            got = set(ora.encode(row.seq[at + 1:row.end(0)]).tolist())
            c.prove(f"all 15 IUPAC codes in an allele on the {path} path from bit {bit}",
                    got == set(range(1, 16)) and (int(row.alt_len[0]) <= 32) == (path == "plane bits"))
    last = len(c.ref) - 1
    for n in (3, 40):
        si = c.add([c.ins(last - 2, n)])
        row = c.row(si)
        c.prove(f"an allele of {n} bases begins in the last word of the row", int(row.o[0]) // 32 == (row.len - 1) // 32 or n > 32 and
                int(row.o[0]) // 32 == (len(c.ref) - 1) // 32)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 4. staged-record capacity: HX_MAXV, HX_ALL
# ---------------------------------------------------------------------------------------------------------------------------
CAP_LEN = 2 * TILE + 5056  # 2206 words: a multiple of 32 bases and two words short of a whole quad


def case_record_capacity() -> Case:
    c = Case("record_capacity", CAP_LEN, 8104)
    nw = (CAP_LEN + 31) // 32
    c.prove("REF ends on a word end, two words into a quad", CAP_LEN % 32 == 0 and nw % 4 == 2 and stride_words(CAP_LEN) - 3 == nw - 1)
    inside = lambda k: [TILE + 300 + 310 * i for i in range(k)]  # k starts inside tile 1, none at its first position
    for want in (95, 96, 97, 98):
        for head in (True, False):
            at = ([TILE - 777] if head else []) + inside(want - (1 if head else 0))
            si = c.add([c.snv(p) for p in at])
            t = c.tile(si, 1)
            c.prove(f"tile 1 needs exactly {want} records, {'with' if head else 'without'} a head",
                    t["want"] == want and t["head"] == head and t["all"] == (want <= HX_MAXV) and t["fits"] and t["n"] == min(want, HX_MAXV))
            c.prove("the neighbouring tiles of the row stay on the fast path", c.tile(si, 0)["fast"] and c.tile(si, 2)["fast"])
    # records beyond the staged ones that move the mapping: a deletion and an insertion as records 96.. of the tile
    for tail in (("del",), ("ins",), ("del", "ins", "snv")):
        at = inside(96)
        vs = [c.snv(p) for p in at]
        p = at[-1] + 200
        for kind in tail:
            vs.append(c.dele(p, 11) if kind == "del" else c.ins(p, 40) if kind == "ins" else c.snv(p))
            p += 300
        si = c.add(vs)
        t, row = c.tile(si, 1), c.row(si)
        c.prove(f"records past the {HX_MAXV} staged ones include {'+'.join(tail)}", t["want"] == 96 + len(tail) and not t["all"]
                and (row.chain[96:] != 0).any() and row.end(len(vs) - 1) + 500 < 2 * TILE)
    # the last tile on the slow path: its quads reach past the row's words, its REF reads past REF's
    for extra in ((), ("del_to_end",)):
        at = [2 * TILE + 100 + 45 * i for i in range(98)]
        vs = [c.snv(p) for p in at]
        if extra:
            vs.append(c.dele(CAP_LEN - 1 - 37, 37))
        si = c.add(vs)
        t, row = c.tile(si, 2), c.row(si)
        c.prove("more than 96 records in the last tile of a row" + (" that ends on a deletion's anchor" if extra else ""),
                not t["all"] and t["window_clamped"] and (row.len == CAP_LEN if not extra else int(row.o[-1]) + 1 == row.len))
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 5. staged REF window: HX_RW, HX_FITS, ws rounded down to a quad
# ---------------------------------------------------------------------------------------------------------------------------
def _window_words(case: Case, variants, wb: int):
    row = Row(case.ref, case.startp, variants)
    t = tile_index(row, wb, len(case.ref))
    return t["we"] - t["ws"], t


def case_ref_window() -> Case:
    c = Case("ref_window", CAP_LEN, 8105)
    # tile 0: ws = 0, we = ((32767 + D) >> 5) + 2 for D bases deleted inside the tile
    for D, words in ((1984, HX_RW - 1), (1985, HX_RW), (2016, HX_RW), (2017, HX_RW + 1)):
        c.prove(f"{D} deleted bases give a window of {words} words by the arithmetic of k_hx_index", ((TILE - 1 + D) >> 5) + 2 == words)
        si = c.add([c.dele(1000, D), c.snv(1000 + D + 500)])
        t = c.tile(si, 0)
        c.prove(f"tile 0 reads a window of HX_RW{words - HX_RW:+d} words", t["we"] - t["ws"] == words and t["fits"] == (words <= HX_RW) and t["all"])
    # tile 1 behind U deleted bases: the window starts at every residue of a quad
    for U in (32, 64, 96, 128):
        up = [c.dele(500, U)]
        # the largest deletion inside tile 1 whose window still fits, from the same arithmetic
        D = max(d for d in range(1800, 2200) if _window_words(c, up + [c.dele(TILE + 900, d)], 1)[0] == HX_RW)
        for dd, words in ((D, HX_RW), (D + 1, HX_RW + 1), (D - 32, HX_RW - 1)):
            si = c.add(up + [c.dele(TILE + 900, dd), c.snv(TILE + 900 + dd + 777)])
            t = c.tile(si, 1)
            c.prove(f"tile 1 window starts at residue {(1024 + U // 32) % 4} of a quad and has HX_RW{words - HX_RW:+d} words",
                    t["raw_ws"] % 4 == (U // 32) % 4 and t["ws"] == t["raw_ws"] & ~3 and t["we"] - t["ws"] == words
                    and t["fits"] == (words <= HX_RW) and t["head"])
    si = c.add([c.snv(2 * TILE + 50)])
    t = c.tile(si, 2)
    c.prove("the staged window of the region's last tile is clamped at the end of REF", t["fits"] and t["window_clamped"]
            and t["ws"] + HX_RW > stride_words(CAP_LEN))
    si = c.add([c.dele(TILE + 900, 2100)] + [c.snv(TILE + 4000 + 200 * i) for i in range(100)])
    t = c.tile(si, 1)
    c.prove("a window that does not fit together with more than 96 records", not t["fits"] and not t["all"] and t["want"] == 101)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 6. row ends and the stride
# ---------------------------------------------------------------------------------------------------------------------------
def case_row_ends() -> Case:
    L = 2 * TILE + 64
    c = Case("row_ends", L, 8106)
    for want in (2 * TILE - 1, 2 * TILE, 2 * TILE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 129, 2 * TILE - 127, 40 * QUAD - 1, 40 * QUAD + 1):
        si = c.add([c.snv(100), c.dele(300, L - want)])
        row = c.row(si)
        c.prove(f"a row of {want} bases ({want % 32} past a word, {want % QUAD} past a quad, {want % TILE} past a tile)", row.len == want)
    c.prove("row lengths 32k-1, 32k, 32k+1, 128k-1, 128k+1, 32768 and 65536",
            {c.row(si).len % 32 for si in range(len(c.copies))} >= {31, 0, 1} and {TILE, 2 * TILE} <= {c.row(si).len for si in range(len(c.copies))})
    si = c.add([c.ins(5000, 201)])
    longest = max(c.row(s).len for s in range(len(c.copies)))
    c.prove("one row longer than REF sets the stride alone", c.row(si).len == L + 200 == longest and stride_words(longest) > stride_words(L)
            and sum(c.row(s).len > L for s in range(len(c.copies))) == 1)
    c.prove("rows shorter than REF leave trailing words and a trailing tile empty",
            any((c.row(s).len + 31) // 32 <= HX_TW for s in range(len(c.copies))))
    for kind in ("snv", "del", "ins"):
        si = c.add([c.snv(0) if kind == "snv" else c.dele(0, 4) if kind == "del" else c.ins(0, 5)])
        c.prove(f"{kind} at relative position 0", int(c.row(si).o[0]) == 0 and c.row(si).seq[0].islower())
    si = c.add([c.snv(L - 1)])
    c.prove("SNV on the last base of the region", int(c.row(si).o[0]) == c.row(si).len - 1 and c.row(si).seq[-1].islower())
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# 7. metadata kernels
# ---------------------------------------------------------------------------------------------------------------------------
def case_segments() -> Case:
    """k_seg_count / k_seg_fill: rounds of 256 indels, segments cut by the row end; k_rev_lookup at the scan bounds' positions"""
    L = 12_000
    c = Case("segments", L, 8107)
    lo, hi = 100, L - 101  # relative positions of startp + 100 and stopp - 100
    for n in (SEG_ROUND, SEG_ROUND + 1, 2 * SEG_ROUND + 44):
        vs = [c.dele(400 + 20 * i, 1 + i % 3) if i % 2 else c.ins(400 + 20 * i, 2 + i % 4) for i in range(n)]
        si = c.add(vs)
        row = c.row(si)
        rel, _ = segments_from_posmap(row.pm)
        c.prove(f"a row with {n} carried indels ({-(-n // SEG_ROUND)} rounds of {SEG_ROUND})", int((row.chain != 0).sum()) == n and len(rel) > n)
    si = c.add([c.ins(L - 1, 6)])
    row = c.row(si)
    rel, _ = segments_from_posmap(row.pm)
    c.prove("an insertion on the last base: the segment behind it is cut off by the row end",
            int(row.o[0]) + 1 + 5 == row.len and len(rel) == 1 + 5)
    si = c.add([c.dele(L - 1 - 9, 9)])
    row = c.row(si)
    c.prove("a deletion whose anchor is the row's last base opens no segment", int(row.o[0]) + 1 == row.len
            and len(segments_from_posmap(row.pm)[0]) == 1)
    # reverse look-ups of genomic positions startp + 100 and stopp - 100 (relative lo, hi) at every kind of edge
    g_lo, g_hi = c.startp + lo, c.startp + hi
    many = [c.dele(3000 + 30 * i, 2) for i in range(70)]  # > 64 segments: the match is found by one lane, the others hold -1

    def rev_case(label, vs, want_lo=None, want_hi=None, check=None):
        si = c.add(vs)
        row = c.row(si)
        a, b = ora.posmap_rev(row.pm, g_lo), ora.posmap_rev(row.pm, g_hi)
        ok = (want_lo is None or a == want_lo) and (want_hi is None or b == want_hi) and (check is None or check(row, a, b))
        c.prove(f"reverse look-up: {label}", ok)
    rev_case("an insertion anchor: the last inserted base wins", [c.ins(lo, 5)] + many, want_lo=lo + 4)
    rev_case("an insertion anchor behind 70 deletions", many + [c.ins(hi, 7)], want_hi=hi - 140 + 6)
    rev_case("a deleted position", many + [c.dele(hi - 1, 4)], want_hi=-1)
    rev_case("a deleted position right behind an insertion anchor", [c.ins(hi - 9, 4), c.dele(hi - 3, 6)], want_hi=-1)
    # (a deleted position at the START of the scan range is no valid input: the reference looks it up without a walk and raises)
    gone = Row(c.ref, c.startp, [c.dele(lo - 3, 5)])
    try:
        ora.scan_bounds(gone.pm, c.startp, c.stopp, c.pamlen)
        refused = False
    except ora.OracleError as e:
        refused = e.code == -3
    c.prove("the oracle refuses a row whose scan start is deleted", refused and ora.posmap_rev(gone.pm, g_lo) == -1)
    rev_case("the first position of a segment", [c.dele(lo - 6, 5)] + many, want_lo=lo - 5,
             check=lambda row, a, b: a in segments_from_posmap(row.pm)[0].tolist())
    rev_case("the last position of a segment", [c.dele(lo, 5)] + many, want_lo=lo,
             check=lambda row, a, b: a + 1 in segments_from_posmap(row.pm)[0].tolist())
    rev_case("the last position of a segment behind more than 64 segments", many + [c.dele(hi, 5)], want_hi=hi - 140,
             check=lambda row, a, b: len(segments_from_posmap(row.pm)[0]) > 64 and b + 1 == segments_from_posmap(row.pm)[0][-1])
    rev_case("the first position of the last of more than 64 segments", many + [c.dele(hi - 4, 3)], want_hi=hi - 140 - 3,
             check=lambda row, a, b: b == segments_from_posmap(row.pm)[0][-1])
    rev_case("both positions in the identity segment of a row of SNVs", [c.snv(lo), c.snv(hi)], want_lo=lo, want_hi=hi)
    rev_case("an insertion one base before the position", [c.ins(lo - 1, 9)], want_lo=lo + 8)
    return c


def _many_rows(name: str, n_samples: int, seed: int) -> Case:
    """n_samples + 1 rows over a small region: one private SNV per sample, every seventh sample a deletion and every
    eleventh an insertion besides, so the segment counts k_scan_u32 sums differ from row to row"""
    L = n_samples + 400
    c = Case(name, L, seed)
    for i in range(n_samples):
        vs = [c.snv(120 + i)]
        if i % 7 == 3:
            vs.append(c.dele(L - 150, 3))
        if i % 11 == 5:
            vs.append(c.ins(L - 130, 3))
        c.add(vs)
    n_rows = 1 + len(c.live_columns())
    c.prove(f"a plan of {n_rows} rows ({n_rows - SCAN_ROUND:+d} against one round of the scan)", n_rows == n_samples + 1)
    counts = {len(segments_from_posmap(c.row(si).pm)[0]) for si in range(0, n_samples, 13)}
    c.prove("segment counts differ between rows", len(counts) >= 3)
    return c


def case_rows_4096() -> Case:
    return _many_rows("rows_4096", SCAN_ROUND - 1, 8108)


def case_rows_4097() -> Case:
    return _many_rows("rows_4097", SCAN_ROUND, 8109)


def case_rows_4500() -> Case:
    return _many_rows("rows_4500", 4499, 8110)


def _list_check(name: str, seed: int, gap: int, clamp_over: int) -> Case:
    """`gap`: bases between the end of a deletion and the next variant (-1: it covers the variant's base);
    `clamp_over`: by how much a deletion behind an upstream insertion reaches past the region's original length"""
    L = 6000
    c = Case(name, L, seed)
    d = 12
    vs = [c.dele(1000, d), c.snv(1000 + d + 1 + gap)]
    r0, span = 1000, d + 1
    c.prove(f"the next variant starts {gap:+d} bases from the end of the deletion", vs[1][0] - c.startp - (r0 + span) == gap)
    k = 25  # inserted bases upstream
    span2 = L - (4000 + k) + clamp_over  # o + span == L + clamp_over with o = 4000 + k
    vs2 = [c.ins(2000, k + 1), c.dele(4000, span2 - 1)] if 4000 + span2 <= L else None
    c.prove(f"an indel behind {k} inserted bases ends {clamp_over:+d} past the original length", vs2 is not None
            and (4000 + k) + span2 - L == clamp_over)
    if gap < 0:
        c.expect_error = "overlap"
        c.add(vs)
        c.add([c.snv(50)])
    elif clamp_over > 0:
        c.expect_error = "clamp"
        try:
            ora.hap_build(c.ref, c.startp, sorted(vs2))
            refused = False
        except ora.OracleError as e:
            refused = e.code == -6
        c.prove("the oracle refuses the indel with the reference's clamp error", refused)
        c.add(vs2)
        c.add(vs)
    else:
        si = c.add(vs)
        row = c.row(si)
        c.prove("deletion and next variant are adjacent and both applied", int(row.o[1]) == int(row.o[0]) + 1 + gap)
        sj = c.add(vs2)
        row = c.row(sj)
        c.prove("the indel ends exactly on the original length", int(row.o[1]) + int(row.span[1]) == L)
    return c


def case_list_ok() -> Case:
    return _list_check("list_ok", 8111, 0, 0)


def case_list_overlap() -> Case:
    return _list_check("list_overlap", 8111, -1, 0)


def case_list_clamp() -> Case:
    return _list_check("list_clamp", 8111, 0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. content hash and row identity
# ---------------------------------------------------------------------------------------------------------------------------
def _identity(name: str, wide: bool) -> Case:
    L = 3 * QUAD * 10 + 17   # the last word holds 17 bases
    c = Case(name, L, 8112, patches={600: "CCCC"})
    # different variant sets, one cased string: in CCCC, (delete base 1 anchored on base 0, mark base 2) and
    # (mark base 0, delete base 2 anchored on base 1) both read "ccC"
    a = c.add([c.dele(600, 1), c.snv(602, "C")])
    b = c.add([c.snv(600, "C"), c.dele(601, 1)])
    c.prove("two different variant sets give one cased string", c.row(a).seq == c.row(b).seq and c.copies[a][0] != c.copies[b][0]
            and not np.array_equal(c.row(a).pm, c.row(b).pm))
    # one V bit apart
    m = c.add([c.snv(900, c.ref[900])])
    c.prove("a SNV whose alt is the REF base differs from REF in one V bit only", c.row(m).seq.upper() == c.ref
            and sum(x != y for x, y in zip(c.row(m).seq, c.ref)) == 1)
    d1 = c.add([c.dele(1500, 2)])
    d2 = c.add([c.dele(1500, 2), c.snv(1503, c.ref[1503])])
    c.prove("rows that differ in one V bit behind a deletion", c.row(d1).seq.upper() == c.row(d2).seq.upper()
            and sum(x != y for x, y in zip(c.row(d1).seq, c.row(d2).seq)) == 1)
    e = c.add([c.snv(L - 1)])
    c.prove("a row that differs from REF in the last base of the last word only",
            c.row(e).seq[:-1] == c.ref[:-1] and c.row(e).seq[-1] != c.ref[-1] and (L - 1) // 32 == (L + 31) // 32 - 1)
    if wide:
        w = c.add([c.ins(2000, 1 + 2 * QUAD)])
        c.prove("one long row widens the stride of the plan", stride_words(c.row(w).len) > stride_words(L))
    else:
        c.prove("no row is longer than REF", max(c.row(s).len for s in range(len(c.copies))) <= L)
    kept = c.expected_haplotypes()
    c.prove("the equal strings collapse, the one-bit neighbours do not", len(kept) == 1 + len(c.copies) - 1)
    return c


def case_identity() -> Case:
    return _identity("identity", False)


def case_identity_wide() -> Case:
    return _identity("identity_wide", True)


CASES = OrderedDict((f.__name__[5:], f) for f in (
    case_tile_seams, case_word_seams, case_allele_lengths, case_record_capacity, case_ref_window, case_row_ends, case_segments,
    case_rows_4096, case_rows_4097, case_rows_4500, case_list_ok, case_list_overlap, case_list_clamp, case_identity, case_identity_wide))
# what every case must have proved before anything is compared: a fragment of a label per seam it is listed for
REQUIRED = {
    "tile_seams": ["snv starts at p_hi-1", "del starts at p_hi+0", "ins starts at p_hi+1", "tile 2 has no head", "earlier tile than 1",
                   "reaches 1 bases", "reaches 31 bases", "reaches 32 bases", "reaches 33 bases", "reaches 200 bases", "four words lie inside",
                   "anchored on the last position"],
    "word_seams": ["bit 0 of the first word", "bit 31 of the last word", "2 SNVs", "3 SNVs", "32 SNVs", "del then SNV", "ins then SNV",
                   "ends exactly at a word end", "immediately followed by a SNV", "exactly at a word start"],
    "allele_lengths": ["alt_len 31", "alt_len 32", "alt_len 33", "alt_len 64", "alt_len 65", "400 bases", "plane bits path", "text path",
                       "last word of the row"],
    "record_capacity": ["exactly 95 records, with", "exactly 96 records, without", "exactly 97 records, with", "exactly 98 records, without",
                        "include del", "include ins", "fast path", "last tile of a row"],
    "ref_window": ["HX_RW-1 words", "HX_RW+0 words", "HX_RW+1 words", "residue 0", "residue 1", "residue 2", "residue 3", "clamped at the end",
                   "together with more than 96"],
    "row_ends": ["32768 and 65536", "sets the stride alone", "trailing tile empty", "snv at relative position 0", "del at relative position 0",
                 "ins at relative position 0", "last base of the region"],
    "segments": ["256 carried indels", "257 carried indels", "556 carried indels", "cut off by the row end", "opens no segment",
                 "last inserted base wins", "a deleted position", "first position of a segment", "last position of a segment", "more than 64"],
    "rows_4096": ["4096 rows"], "rows_4097": ["4097 rows"], "rows_4500": ["4500 rows"],
    "list_ok": ["+0 bases from the end", "+0 past the original"], "list_overlap": ["-1 bases from the end"], "list_clamp": ["+1 past the original", "refuses"],
    "identity": ["one cased string", "one V bit only", "V bit behind a deletion", "last base of the last word", "collapse"],
    "identity_wide": ["one cased string", "widens the stride"],
}
