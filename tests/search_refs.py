"""Case builders for tests/test_gpu_search_seams.py, all on the CPU: hand-built haplotype strings on the seams of the plane
search (hawk_search.hip: k_search_count, k_emit_list, k_search_emit, k_ref_bits and the offset scan hawk_launch_mscan), and a
restatement of the per-tile arithmetic of those kernels - survivors, valid rows, TF, staged segments, tile counts - so that every
case can PROVE, from ora.search / ora.scan output and the position maps alone, that it sits on the seam it is named after.  A
case that drifts off its seam fails in its builder; tests/test_search_refs.py runs every builder without a GPU.

Strings are a filler that cannot match the PAM (A/T for NGG, C/G for TTTV) with the PAM planted, so the counts are exact:
a window start q (the first base of spacer+PAM on the + strand) is a guide only where a builder wrote the PAM's letters.  An alt
row is REF with lower-case bases: a lower-case copy of REF's own letter makes a window a survivor that is redundant with REF's
guide, a real SNV makes a valid row with a REF partner, a SNV that completes a PAM REF lacks makes a valid row without one."""
from collections import OrderedDict

import numpy as np

from oracle import oracle as ora

# the geometry of hawk_search.hip / hawk_rows.h
TILE = 32768        # window starts per tile (HAWK_BLOCK * 128)
LIST_CAP = 512      # valid survivors the count pass hands to k_emit_list
CAP = 512           # survivors per round (count rounds, REF rounds of k_search_emit)
BLOCK = 256         # HAWK_BLOCK: survivors one pass of phase C takes
NSEG = 64           # position-map segments staged per tile
TAIL = 64           # tile_end = tile + TILE + TAIL
MS_TILE = 1024      # counts per workgroup of k_mscan1 / k_mscan23 / k_mscan3
MSW_TILE = 4096     # ... of the wide pair k_mscan1w / k_mscan23w (16 per thread)
PAD = 10            # GUIDESEQPAD
STARTP = 100_001    # genomic position of REF's first base


def stride_words(max_len: int) -> int:
    return ((max_len + 31) // 32 + 2 + 3) // 4 * 4


def tiles_per_row(max_len: int) -> int:
    """bph: tiles per row of a set whose longest row has max_len bases"""
    return (stride_words(max_len) // 4 + BLOCK - 1) // BLOCK


def segment_starts(pm) -> np.ndarray:
    """where a position map leaves unit slope: crisprhawk_hip.hapset.segments_from_posmap restated (this module never imports
    the product)"""
    pm = np.asarray(pm, dtype=np.int64)
    return np.concatenate(([0], np.flatnonzero(np.diff(pm) != 1) + 1)).astype(np.int64)


def scan_route(n: int, shards: bool = True, aligned: bool = True) -> dict:
    """hawk_mscan_route restated, with the figures the kernels of the route derive from n: route (ONE / M1_M23 / WIDE / M1_M2_M3),
    tile (counts per workgroup), partials (workgroups), chunks (trips of k_mscan2's loop over 1024 partials), last_chunk (partials
    in its last trip), trips (of the prefix loop of k_mscan23 / k_mscan23w in the last workgroup), tail (counts in the last
    workgroup).  aligned: counts and offsets both on a 16-byte boundary."""
    assert n >= 1
    if n <= 2048 and shards:
        return dict(route="ONE", tile=0, partials=0, chunks=0, last_chunk=0, trips=0, tail=n, ipt=max(1, (n + 1023) // 1024))
    nb, nbw = (n + MS_TILE - 1) // MS_TILE, (n + MSW_TILE - 1) // MSW_TILE
    if nb > 4096 and nbw <= 4096 and shards and aligned:
        return dict(route="WIDE", tile=MSW_TILE, partials=nbw, chunks=0, last_chunk=0, trips=(nbw - 1 + BLOCK - 1) // BLOCK,
                    tail=n - (nbw - 1) * MSW_TILE)
    if nb <= 4096 and shards:
        return dict(route="M1_M23", tile=MS_TILE, partials=nb, chunks=0, last_chunk=0, trips=(nb - 1 + BLOCK - 1) // BLOCK,
                    tail=n - (nb - 1) * MS_TILE)
    chunks = (nb + 1023) // 1024
    return dict(route="M1_M2_M3", tile=MS_TILE, partials=nb, chunks=chunks, last_chunk=nb - (chunks - 1) * 1024, trips=0,
                tail=n - (nb - 1) * MS_TILE)


def scan_kernel(n: int, shards: bool = True, aligned: bool = True) -> str:
    """hawk_launch_mscan's choice for n counts, in words"""
    r = scan_route(n, shards, aligned)
    if r["route"] == "ONE":
        return f"k_mscan_one ipt={r['ipt']}"
    name = {"M1_M23": "k_mscan1+k_mscan23", "WIDE": "k_mscan1w+k_mscan23w", "M1_M2_M3": "k_mscan1/2/3"}[r["route"]]
    return f"{name} {r['partials']} partials"


def emit_path(valid: int, is_ref: bool, survivors: int) -> str:
    if valid == 0:
        return "none"
    if valid <= LIST_CAP:
        return "list"
    return f"{-(-survivors // CAP)} rounds" if is_ref else "recompute"


_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "V": "B", "B": "V"}


class Case:
    """(seqs, posmaps, is_ref, scan, pam, guidelen, right) and what was proved about it"""

    def __init__(self, name: str, pam: str, guidelen: int, right: bool, seed: int):
        self.name, self.pam, self.guidelen, self.right = name, pam, guidelen, bool(right)
        self.pamlen, self.L = len(pam), guidelen + len(pam)
        self.filler = "AT" if pam == "NGG" else "CG" if pam == "TTTV" else "ACGT"
        self.rng = np.random.default_rng(seed)
        self.seqs, self.posmaps, self.is_ref, self.scan, self.proved = [], [], [], [], []
        self._want = self._tally = None
        self.row_cap = None  # rows the oracle is given room for (default: two per base of the set)

    # ---- strings ----------------------------------------------------------------------------------------------------------
    def fill(self, n: int) -> list:
        return list(np.array(list(self.filler))[self.rng.integers(0, len(self.filler), n)])

    def pam_at(self, strand: int) -> int:
        """offset of the PAM inside spacer+PAM on the + strand"""
        return 0 if (self.right != bool(strand)) else self.guidelen

    def plant(self, s: list, q: int, strand: int, skip=()) -> None:
        """write the PAM's letters for a guide whose window starts at q on `strand` (N, V, B are left to the filler)"""
        letters = self.pam if strand == 0 else "".join(_COMP[c] for c in reversed(self.pam))
        for t, c in enumerate(letters):
            if c in "ACGT" and t not in skip:
                i = q + self.pam_at(strand) + t
                s[i] = c.lower() if s[i].islower() else c

    def swap(self, c: str) -> str:
        """a real SNV inside the filler's alphabet, lower case"""
        a, b = self.filler[0], self.filler[1]
        assert c.upper() in (a, b), "a SNV would overwrite a planted PAM letter"
        return (b if c.upper() == a else a).lower()

    def spacer_pos(self, q: int, k: int = 5) -> int:
        """a position that lies in the spacer of both strands' guides at window start q"""
        return q + self.pamlen + k if self.guidelen >= self.pamlen + k + 1 else q + self.guidelen // 2

    def add(self, seq, pm=None, is_ref=False, scan=None) -> int:
        seq = "".join(seq)
        self.seqs.append(seq)
        self.posmaps.append(np.arange(STARTP, STARTP + len(seq), dtype=np.int64) if pm is None else np.asarray(pm, dtype=np.int64))
        self.is_ref.append(bool(is_ref))
        self.scan.append(scan if scan is not None else (0, len(seq) - self.pamlen + 1))
        self._want = self._tally = None
        return len(self.seqs) - 1

    def prove(self, label: str, cond) -> None:
        assert bool(cond), f"{self.name}: off its seam: {label}"
        self.proved.append(label)

    # ---- what the oracle makes of it --------------------------------------------------------------------------------------
    def hapset(self) -> ora.HapSet:
        return ora.HapSet(self.seqs, self.posmaps, self.is_ref, self.scan)

    @property
    def want(self) -> ora.SearchResult:
        if self._want is None:
            self._want = ora.search(self.hapset(), self.pam, self.guidelen, self.right, cap=self.row_cap)
        return self._want

    def qstart(self, pos, strand):
        """window start of a PAM hit at `pos`"""
        pos, strand = np.asarray(pos, dtype=np.int64), np.asarray(strand, dtype=np.int64)
        pamfirst = strand.astype(bool) != self.right
        return np.where(pamfirst, pos, pos - self.guidelen)

    @property
    def bph(self) -> int:
        return tiles_per_row(max(len(s) for s in self.seqs))

    def tally(self) -> dict:
        """per (row, tile): survivors, TF, TR (k_search_count's workgroup totals), valid (counts[tile]) and nseg (the segments
        the tile may stage: its first one and those starting before tile_end) - from ora.scan, the strings' case, ora.search and the
        position maps; and the totals n_hits / n_candidates the shard sums must reach"""
        if self._tally is not None:
            return self._tally
        bits, bitsrc, _, _ = ora.pam_encode(self.pam)
        bph = self.bph
        out, hits, cand = {}, 0, 0
        for h, (seq, pm, isref, (ss, se)) in enumerate(zip(self.seqs, self.posmaps, self.is_ref, self.scan)):
            n = len(seq)
            per = np.zeros((bph, 2), dtype=np.int64)
            low = np.concatenate(([0], np.cumsum(np.frombuffer(seq.encode(), dtype=np.uint8) >= ord("a"))))
            for s, pos in enumerate(ora.scan(ora.encode(seq), ss, se, bits, bitsrc, self.pamlen)):
                q = self.qstart(pos, np.full(len(pos), s))
                hits += len(q)
                q = q[(q - PAD >= 0) & (q + self.L + PAD <= n)]
                cand += len(q)
                if not isref:
                    q = q[low[q + self.L] - low[q] > 0]
                per[:, s] = np.bincount(q // TILE, minlength=bph)[:bph]
                assert len(q) == 0 or q.max() // TILE < bph
            segs = segment_starts(pm)
            for t in range(bph):
                nseg = 1 + int(((segs > t * TILE) & (segs < (t + 1) * TILE + TAIL)).sum()) if t else int((segs < TILE + TAIL).sum())
                out[(h, t)] = dict(survivors=int(per[t].sum()), TF=int(per[t, 0]), TR=int(per[t, 1]), valid=0, nseg=nseg,
                                   segs_row=len(segs))
        g = self.want.guides
        q = self.qstart(g["pos"], g["strand"])
        if len(g):
            keys, cnt = np.unique(g["hap"].astype(np.int64) * bph + q // TILE, return_counts=True)
            for k, c in zip(keys.tolist(), cnt.tolist()):
                out[(k // bph, k % bph)]["valid"] = c
        assert (hits, cand) == (self.want.n_hits, self.want.n_candidates), "the tally restates the oracle's scan and range test"
        for (h, t), v in out.items():
            assert v["valid"] <= v["survivors"] and (not self.is_ref[h] or v["valid"] == v["survivors"])
            v["path"] = emit_path(v["valid"], self.is_ref[h], v["survivors"])
        self._tally = out
        return out

    def rows_of(self, h: int):
        """(window start, strand, start) of the oracle's rows of row h"""
        g = self.want.guides
        m = g["hap"] == h
        return self.qstart(g["pos"][m], g["strand"][m]), g["strand"][m], g["start"][m]

    def ref_keys(self) -> set:
        g = self.want.guides
        m = np.asarray(self.is_ref)[g["hap"]]
        return set(zip(g["start"][m].tolist(), g["strand"][m].tolist()))

    def expected_flags(self) -> np.ndarray:
        """per oracle row: REF has a guide at this (start, strand)"""
        keys = self.ref_keys()
        g = self.want.guides
        return np.array([(a, b) in keys for a, b in zip(g["start"].tolist(), g["strand"].tolist())], dtype=np.uint8)

    def in_domain(self) -> bool:
        return all(0 <= a <= b <= len(s) - self.pamlen + 1 for s, (a, b) in zip(self.seqs, self.scan))

    def summary(self) -> str:
        """one line per interesting tile for the coverage table"""
        t = self.tally()
        big = sorted(t.items(), key=lambda kv: (-kv[1]["survivors"], kv[0]))[:2]
        tiles = len(self.seqs) * self.bph
        cells = "; ".join(f"row {h} tile {b}: {v['survivors']} surv / {v['valid']} valid / TF {v['TF']} / {v['nseg']} seg -> {v['path']}"
                          for (h, b), v in big)
        return f"{self.name}: {tiles} tiles ({scan_kernel(tiles)}); {cells}"


# ---------------------------------------------------------------------------------------------------------------------------
# planted sites: (window start, strand, kind)
#   ref   REF has the guide, the alt row's window is upper case (a candidate, no survivor)
#   snv   REF has the guide, the alt row a real SNV in the spacer: valid, REF partner, CFDon finite
#   same  REF has the guide, the alt row a lower-case copy of REF's letter: a survivor redundant with REF's guide
#   new   REF lacks the PAM's last letter, the alt row's SNV completes it: valid, no partner, CFDon NaN
# ---------------------------------------------------------------------------------------------------------------------------
def planted_pair(c: Case, n: int, sites, ref_scan=None, alt=True):
    ref = c.fill(n)
    for q, s, kind in sites:
        last = [t for t, ch in enumerate(c.pam if s == 0 else c.pam[::-1]) if ch in "ACGT"][-1]
        c.plant(ref, q, s, skip=(last,) if kind == "new" else ())
    c.add(ref, is_ref=True, scan=ref_scan)
    if not alt:
        return
    row = list(ref)
    for i, (q, s, kind) in enumerate(sites):
        p = c.spacer_pos(q, 3 + i % 7)
        if kind == "snv":
            row[p] = c.swap(row[p])
        elif kind == "same":
            row[p] = row[p].lower()
        elif kind == "new":
            c.plant(row, q, s)
            last = [t for t, ch in enumerate(c.pam if s == 0 else c.pam[::-1]) if ch in "ACGT"][-1]
            row[q + c.pam_at(s) + last] = row[q + c.pam_at(s) + last].lower()
    c.add(row, scan=ref_scan)


def _spread(nF: int, nR: int, q0: int, step: int):
    """nF + nR window starts `step` apart, the strands interleaved along the row while both last"""
    out, f, r, i = [], 0, 0, 0
    while f < nF or r < nR:
        s = 1 if (r < nR and (f >= nF or i % 2)) else 0
        out.append((q0 + step * i, s))
        f, r, i = f + (s == 0), r + (s == 1), i + 1
    return out


def _prove_tile(c: Case, h: int, t: int, survivors: int, valid: int, TF=None, what="row"):
    v = c.tally()[(h, t)]
    label = f"{what} {h} tile {t}: {survivors} survivors, {valid} valid"
    if TF is not None:
        label += f", TF {TF}"
    c.prove(label + f" -> {v['path']}", (v["survivors"], v["valid"]) == (survivors, valid) and (TF is None or v["TF"] == TF))
    return v


def _prove_flags(c: Case, h: int):
    """row h has valid rows with a REF partner and valid rows without one"""
    _, strand, start = c.rows_of(h)
    keys = c.ref_keys()
    has = np.array([(a, b) in keys for a, b in zip(start.tolist(), strand.tolist())])
    c.prove(f"row {h}: valid rows with a REF partner ({int(has.sum())}) and without one ({int((~has).sum())})", has.any() and (~has).any())


# ---- 1. list against recompute on a non-REF tile ---------------------------------------------------------------------------
def list_case(name: str, nF: int, nR: int = 0, same: int = 0) -> Case:
    c = Case(name, "NGG", 20, False, 9100 + nF + 7 * nR + same)
    step = 25  # > L = 23: no window holds another site's variant
    valid = nF + nR
    total = valid + same
    pos = _spread(nF + (same if nR == 0 else 0), nR + (same if nR else 0), 64, step)
    assert len(pos) == total and (not pos or pos[-1][0] + 60 < TILE)
    # the redundant survivors are dealt evenly over the tile; of the valid ones every third lacks a REF partner
    is_same = np.zeros(total, dtype=bool)
    if same:
        is_same[np.linspace(0, total - 1, same).round().astype(int)] = True
        assert is_same.sum() == same
    sites, k = [], 0
    for (q, s), sm in zip(pos, is_same):
        if sm:
            sites.append((q, s, "same"))
        else:
            sites.append((q, s, "new" if k % 3 == 1 else "snv"))
            k += 1
    sites += [(TILE - 2000 + 40 * j, j % 2, "ref") for j in range(20)]  # REF guides the alt row does not touch: candidates only
    planted_pair(c, 40_000, sites)
    TF = sum(1 for q, s, kind in sites if s == 0 and kind != "ref")
    v = _prove_tile(c, 1, 0, total, valid, TF)
    c.prove(f"alt tile takes the {'list' if valid <= LIST_CAP else 'recompute'} path" if valid else "alt tile is empty",
            v["path"] == ("none" if valid == 0 else "list" if valid <= LIST_CAP else "recompute"))
    if nR:
        c.prove(f"the strand boundary TF = {TF} lies inside a round of {total} survivors", 0 < TF < total and TF % CAP != 0)
    if same:
        first = int(np.count_nonzero(~is_same[:CAP])) if nR == 0 else None
        c.prove(f"{same} survivors are redundant with REF's guide, dealt over {-(-total // CAP)} count rounds",
                total - valid == same and total > CAP and (first is None or 0 < first < valid))
    if valid >= 2:
        _prove_flags(c, 1)
    c.prove("the alt row's second tile is empty", c.bph == 2 and c.tally()[(1, 1)]["survivors"] == 0)
    return c


# ---- 2. REF rounds ---------------------------------------------------------------------------------------------------------
def ref_rounds_case(name: str, nF: int, nR: int = 0, second_tile: int = 0) -> Case:
    c = Case(name, "NGG", 20, False, 9200 + nF + 3 * nR + second_tile)
    total = nF + nR
    pos = _spread(nF, nR, 64, 25)
    marks = {0, total - 1, min(CAP - 1, total - 1), min(CAP, total - 1), total // 2}
    sites = [(q, s, "snv" if i in marks else "ref") for i, (q, s) in enumerate(pos)]
    sites.append((TILE - 300, 0, "new"))  # alt only: a valid row without a partner
    n = 40_000
    if second_tile:
        n = 70_000
        sites += [(TILE + 64 + 25 * i, i % 2, "snv" if i % 97 == 0 else "ref") for i in range(second_tile)]
    planted_pair(c, n, sites)
    v = _prove_tile(c, 0, 0, total, total, nF, what="REF row")
    c.prove(f"REF tile 0 takes {-(-total // CAP)} rounds" if total > CAP else "REF tile 0 fits the list", v["path"] == emit_path(total, True, total))
    if nR:
        c.prove(f"TF = {nF} = {nF // CAP} rounds + {nF % CAP}: the strand boundary at {nF % CAP} of a round", v["TF"] == nF and v["TR"] == nR)
    if second_tile:
        w = _prove_tile(c, 0, 1, second_tile, second_tile, what="REF row")
        c.prove("one REF tile on the list, one in rounds", {v["path"] == "list", w["path"] == "list"} == {True, False})
    _prove_flags(c, 1)
    return c


# ---- 3. counter maximum ----------------------------------------------------------------------------------------------------
def counter_max_case(name: str, alt: bool) -> Case:
    c = Case(name, "N", 20, False, 9300)
    n = 3 * TILE - 300
    ref = c.fill(n)
    scan = (TILE, 2 * TILE + 20)  # + strand: PAM at q + 20, - strand: PAM at q
    c.add(ref, is_ref=True, scan=scan)
    if alt:
        row = list(ref)
        for p in range(TILE - 24, 2 * TILE + 48, 12):
            row[p] = "ACGT"[("ACGT".index(row[p]) + 1 + p % 3) % 4].lower()
        c.add(row, scan=scan)
    t = c.tally()
    c.prove("three tiles per row", c.bph == 3)
    v = t[(0, 1)]
    c.prove("REF tile 1: TF == TR == 32768, 65536 rows in 128 rounds", v["TF"] == v["TR"] == TILE and v["valid"] == 2 * TILE
            and -(-v["survivors"] // CAP) == 128 and v["path"] == "128 rounds")
    c.prove("the neighbouring REF tiles hold the 20 rows of one strand each", t[(0, 0)]["TF"] == 20 and t[(0, 0)]["TR"] == 0
            and t[(0, 2)]["TR"] == 20 and t[(0, 2)]["TF"] == 0)
    if alt:
        w = t[(1, 1)]
        c.prove("alt tile 1: 65536 survivors, 65536 valid -> recompute", w["TF"] == w["TR"] == TILE and w["valid"] == 2 * TILE
                and w["path"] == "recompute")
    return c


# ---- 4. staged segments ----------------------------------------------------------------------------------------------------
def _indel_row(c: Case, ref: list, variants, snv_at=(), same_at=()):
    """the alt row of REF through ora.hap_build: (pos, ref, alt) variants in REF coordinates, SNVs given by REF position"""
    refs = "".join(ref)
    vs = list(variants)
    vs += [(STARTP + p, refs[p], c.swap(refs[p]).upper()) for p in snv_at]
    vs += [(STARTP + p, refs[p], refs[p]) for p in same_at]
    return ora.hap_build(refs, STARTP, sorted(vs))


def segments_case(name: str, kind: str, nseg: int, valid: int, tail: bool = False) -> Case:
    """an alt row whose tile 0 stages `nseg` segments (first one included), built from deletions (`del`) or one insertion
    (`ins`); `tail`: segment number nseg starts inside the 64 positions behind the tile"""
    c = Case(name, "NGG", 20, False, 9400 + nseg)
    L = c.L
    n = 46_000
    ref = c.fill(n)
    d = 3
    offs = (0, 1, L, L + 1)
    if kind == "del":
        in_tile = nseg - 1 - (1 if tail else 0)
        at = [300 + 70 * i for i in range(in_tile)]   # REF positions of the anchors
        if tail:
            at.append(TILE + 19 + d * in_tile)       # its successor starts at row position TILE + 20
        at.append(41_000)                            # one more segment far behind tile_end
        dele = lambda: [(STARTP + r, "".join(ref[r:r + d + 1]), ref[r]) for r in at]
        free0 = 300 + 70 * in_tile + 200
    else:
        k = nseg - 1
        a = 5000
        text = c.fill(k)
        for i in (25, 26, 59, 60, k - 3, k - 2):       # GG inside the inserted bases
            text[i] = "G"
        ins = lambda: [(STARTP + a, ref[a], ref[a] + "".join(text)), (STARTP + 41_000, "".join(ref[41_000:41_000 + d + 1]), ref[41_000])]
        free0 = a + 400
    variants = dele if kind == "del" else ins
    seq, pm = _indel_row(c, ref, variants())
    segs = segment_starts(pm)
    # windows whose start or stop look-up sits on a segment start: s == q, q + 1, q + L, q + L + 1.  The PAM is written into REF
    # where the alt row's position maps to; the row is then built again from the changed REF.
    inserted = np.concatenate(([False], np.diff(pm) == 0))
    snv = []
    rot = (2 - (nseg - 2)) % 4  # the last segment before tile_end gets the window whose stop look-up starts it (s == q + L)
    plan = [(s, offs[(i + rot) % 4]) for i, s in enumerate(segs[1:].tolist())
            if s < TILE + TAIL + 100 and (kind == "del" or i % 9 in (0, 4) or i >= len(segs) - 4)]
    if kind == "ins":  # the row's FIRST break exactly at the stop look-up and one past it: no other break inside those windows
        plan += [(int(segs[1]), L), (int(segs[1]), L + 1)]
    for s, off in plan:
        q = s - off
        for x in (q + 21, q + 22):
            if not inserted[x]:
                ref[int(pm[x] - STARTP)] = "G"
    for s, off in plan:  # a window that ends in front of the break is REF's own without a SNV of its own: one in every spacer
        q = s - off
        if not inserted[q:q + L].any():
            x = next(x for x in range(q + 3, q + 12) if seq[x].isupper() and ref[int(pm[x] - STARTP)] in c.filler)
            snv.append(int(pm[x] - STARTP))
    snv = sorted(set(snv))
    seq, pm = _indel_row(c, ref, variants(), snv_at=snv)
    c.add(ref, is_ref=True)
    h = c.add(seq, pm)
    v0 = c.tally()[(h, 0)]["valid"]
    assert v0 <= valid, (v0, valid)
    # pad the tile to its valid count with plain SNV guides in the stretch no segment starts in
    pads = [free0 + 25 * j for j in range(valid - v0)]
    assert not pads or pads[-1] + 60 < TILE - 300
    shift = int(pm[free0] - STARTP) - free0  # row position -> REF position in that stretch
    for q in pads:
        ref[q + shift + 21] = ref[q + shift + 22] = "G"
    snv += [q + shift + 5 for q in pads]
    c.seqs, c.posmaps, c.is_ref, c.scan = [], [], [], []
    seq, pm = _indel_row(c, ref, variants(), snv_at=snv)
    c.add(ref, is_ref=True)
    h = c.add(seq, pm)
    segs = segment_starts(pm)
    t = c.tally()[(h, 0)]
    before = int((segs < TILE + TAIL).sum())
    c.prove(f"alt tile 0: {nseg} segments start before tile_end ({'staged' if nseg <= NSEG else 'global look-up'}), {len(segs)} in the row",
            before == nseg == t["nseg"] and len(segs) > nseg)
    if tail:
        c.prove(f"segment {nseg} starts inside the {TAIL} positions behind the tile", TILE <= segs[nseg - 1] < TILE + TAIL and segs[nseg - 2] < TILE)
    if kind == "ins":
        run = segs[1:nseg]
        c.prove("every inserted base is a segment of its own", np.array_equal(np.diff(run), np.ones(len(run) - 1)) and seq[int(run[0]):int(run[-1]) + 1].islower())
    _prove_tile(c, h, 0, t["survivors"], valid)
    c.prove(f"alt tile 0 takes the {'list' if valid <= LIST_CAP else 'recompute'} path", t["path"] == ("list" if valid <= LIST_CAP else "recompute"))
    q, strand, start = c.rows_of(h)
    # the NEXT segment start behind a kept window's own start: posmap_staged_span searches a second time iff it is <= q + L
    nxt = segs[np.minimum(np.searchsorted(segs, q, side="right"), len(segs) - 1)] - q
    inside = q < TILE
    c.prove("a kept window with a segment starting exactly at q", (np.isin(q, segs[1:]) & inside).any())
    c.prove("a kept window with a segment starting exactly at q+1", ((nxt == 1) & inside).any())
    c.prove("a kept window with a segment starting exactly at q+L and none before it: the last stop that needs a second look-up", ((nxt == L) & inside).any())
    c.prove("a kept window with a segment starting exactly at q+L+1 and none before it: the first stop that needs none", ((nxt == L + 1) & inside).any())
    last = int(segs[nseg - 1])
    c.prove(f"a kept window's start or stop look-up lands in segment {nseg}, the last before tile_end",
            any(last <= x < last + (1 if kind == "ins" else 40) or last <= x + L < last + (1 if kind == "ins" else 40) for x in q.tolist() if x < TILE))
    return c


# ---- 5. word, thread, wave and tile geometry -------------------------------------------------------------------------------
REL_STARTS = (0, 31, 32, 127, 128, 8191, 8192, 32745, 32767, 32768)


# TTTV's last letter excludes T: two neighbouring starts of one strand cannot both be guides there
CPF1_STARTS = ((0, 31, 127, 8191, 32745, 32767), (0, 32, 128, 8192, 32768))


def geometry_case(name: str, pam: str, guidelen: int, right: bool, rels=(REL_STARTS, REL_STARTS)) -> Case:
    c = Case(name, pam, guidelen, right, 9500 + guidelen + 50 * right)
    sites = [(TILE + rel, s, "ref") for s in (0, 1) for rel in rels[s]]
    n = 2 * TILE + 3000
    ref = c.fill(n)
    for q, s, _ in sites:
        c.plant(ref, q, s)
    c.add(ref, is_ref=True)
    row = list(ref)
    for rel in sorted(set(rels[0] + rels[1])):
        p = c.spacer_pos(TILE + rel, 2)
        row[p] = c.swap(row[p])
    c.add(row)
    c.prove(f"L = {c.L}, W = {c.L + 2 * PAD}", 13 <= c.L <= 44 and c.bph == 3)
    for h in (0, 1):
        q, strand, _ = c.rows_of(h)
        for s in (0, 1):
            got = set((q[strand == s] - TILE).tolist())
            c.prove(f"row {h} strand {s}: window starts at tile-relative {', '.join(map(str, rels[s]))}", got >= set(rels[s]))
    t = c.tally()
    c.prove("start 32768 is the first of the next tile, 32767 the last of this one", t[(0, 2)]["valid"] >= 1 and t[(1, 2)]["valid"] >= 1)
    _, strand, start = c.rows_of(1)
    keys = c.ref_keys()
    c.prove("alt rows with a REF partner", any((a, b) in keys for a, b in zip(start.tolist(), strand.tolist())))
    return c


def ends_case(name: str, n: int, right: bool) -> Case:
    """the first and last legal window start of a row of n bases, and one past each; the scan range is the whole row"""
    c = Case(name, "NGG", 20, right, 9600 + n % 1000 + right)
    L = c.L
    qlast = n - L - PAD
    sites = [(q, s, "snv") for s in (0, 1) for q in (PAD - 1, PAD, qlast, qlast + 1)]  # neighbours merge into runs of three letters
    sites += [((2000 if n > 3000 else 200) + 50 * i, i % 2, "snv") for i in range(4)]
    ref = c.fill(n)
    for q, s, _ in sites:
        c.plant(ref, q, s)
    c.add(ref, is_ref=True)
    row = list(ref)
    for q, s, _ in sites:
        p = c.spacer_pos(q)
        if row[p].isupper():
            row[p] = c.swap(row[p])
    c.add(row)
    c.prove(f"hap_len {n} = {n % 32} (mod 32), stride {stride_words(n)} words, {c.bph} tile(s) per row", c.in_domain())
    for h in (0, 1):
        q, strand, _ = c.rows_of(h)
        for s in (0, 1):
            got = set(q[strand == s].tolist())
            c.prove(f"row {h} strand {s}: window start {PAD} and hap_len - L - 10 kept, {PAD - 1} and hap_len - L - 9 dropped",
                    {PAD, qlast} <= got and not ({PAD - 1, qlast + 1} & got))
    c.prove("n_hits > n_candidates: window starts below 10 and past the last legal one are hits", c.want.n_hits == c.want.n_candidates + 8)
    return c


def scan_edges_case(name: str, right: bool, strand: int) -> Case:
    """(both strands' PAMs cannot sit at the same four positions: one case per strand)"""
    c = Case(name, "NGG", 20, right, 9700 + right)
    n = 6000
    ss, se = 500, 5200
    ref = c.fill(n)
    want = {0: [], 1: []}
    for s in (strand,):
        for ppos in (ss - 1, ss, se - 1, se):  # PAM hit positions
            q = ppos - c.pam_at(s)
            c.plant(ref, q, s)
            want[s].append(q)
    c.add(ref, is_ref=True, scan=(ss, se))
    row = list(ref)
    for s in (0, 1):
        for q in want[s]:
            p = c.spacer_pos(q)
            if row[p].isupper():
                row[p] = c.swap(row[p])
    c.add(row, scan=(ss, se))
    bits, bitsrc, _, _ = ora.pam_encode(c.pam)
    every = ora.scan(ora.encode(c.seqs[0]), 0, n - 2, bits, bitsrc, 3)
    for h in (0, 1):
        q, st, _ = c.rows_of(h)
        for s in (strand,):
            got = set((q[st == s] + c.pam_at(s)).tolist())
            c.prove(f"row {h} strand {s}: PAM at scan_start and scan_stop - 1 kept, at scan_start - 1 and scan_stop dropped",
                    got == {ss, se - 1} and {ss - 1, ss, se - 1, se} <= set(every[s].tolist()))
    return c


# ---- 6. tile counts --------------------------------------------------------------------------------------------------------
def tiles_case(name: str, n_hap: int, big_row: int = -1) -> Case:
    """n_hap rows of one tile each, REF first; alt row i keeps i % 3 rows.  `big_row`: that row keeps 513 (and every row is long
    enough to hold them)"""
    c = Case(name, "NGG", 20, False, 9800 + n_hap)
    c.row_cap = 4 * n_hap + 2000
    n = 120 if big_row < 0 else 13_500
    ref = c.fill(n)
    base = [12, 60]
    many = [130 + 25 * j for j in range(513)] if big_row >= 0 else []
    for q in base + many:
        c.plant(ref, q, 0)
    refs = "".join(ref)
    c.add(refs, is_ref=True)
    for i in range(1, n_hap):
        row = refs
        for k, q in enumerate(many if i == big_row else base[: i % 3]):
            p = q + 2 + (i + k) % 17
            row = row[:p] + c.swap(row[p]) + row[p + 1:]
        c.add(row)
    t = c.tally()
    c.prove(f"{n_hap} tiles of one row each -> {scan_kernel(n_hap)}", c.bph == 1 and len(c.seqs) == n_hap)
    ok = all(t[(i, 0)]["valid"] == (513 if i == big_row else i % 3) for i in range(1, n_hap))
    c.prove("alt row i keeps i % 3 rows" + (f", row {big_row} keeps 513 -> recompute" if big_row >= 0 else ""), ok and t[(0, 0)]["valid"] == len(base + many))
    if big_row >= 0:
        c.prove("the recompute tile and REF's rounds lie behind the first 1024 counts: their offsets come from k_mscan23's second workgroup",
                big_row >= MS_TILE and t[(big_row, 0)]["path"] == "recompute" and t[(0, 0)]["path"] == "2 rounds")
    return c


def pam_scan_partials(n_hap: int, bph: int = 1) -> str:
    """hawk_pam_scan scans [strand][row][tile] counts without shard sums"""
    return scan_kernel(2 * n_hap * bph, shards=False)


# ---------------------------------------------------------------------------------------------------------------------------
CASES = OrderedDict()
REQUIRED = {}


def _reg(name, fn, required):
    CASES[name] = fn
    REQUIRED[name] = required


for _n in (0, 1, 255, 256, 257, 511, 512, 513, 1024, 1025):
    _reg(f"list_{_n}", (lambda n: lambda: list_case(f"list_{n}", n))(_n),
         [f"row 1 tile 0: {_n} survivors, {_n} valid, TF {_n}", "path" if _n else "empty"] + (["with a REF partner"] if _n >= 2 else []))
for _f, _r in ((300, 212), (300, 213)):
    _reg(f"list_{_f}_{_r}", (lambda f, r: lambda: list_case(f"list_{f}_{r}", f, r))(_f, _r),
         [f"{_f + _r} survivors, {_f + _r} valid, TF {_f}", "strand boundary", "with a REF partner"])
_reg("list_600_512", lambda: list_case("list_600_512", 512, 0, 88), ["row 1 tile 0: 600 survivors, 512 valid", "list path", "88 survivors are redundant", "2 count rounds"])
_reg("list_1100_513", lambda: list_case("list_1100_513", 513, 0, 587), ["row 1 tile 0: 1100 survivors, 513 valid", "recompute path", "587 survivors are redundant"])
for _n in (512, 513, 1024, 1025):
    _reg(f"ref_{_n}", (lambda n: lambda: ref_rounds_case(f"ref_{n}", n))(_n), [f"REF row 0 tile 0: {_n} survivors, {_n} valid", "with a REF partner"])
for _f in (511, 512, 513, 768, 769):
    _reg(f"ref_tf_{_f}", (lambda f: lambda: ref_rounds_case(f"ref_tf_{f}", f, 300))(_f), [f"TF {_f}", f"boundary at {_f % CAP} of a round", "rounds"])
_reg("ref_two_tiles", lambda: ref_rounds_case("ref_two_tiles", 100, 0, 700), ["one REF tile on the list, one in rounds"])
_reg("counter_max_ref", lambda: counter_max_case("counter_max_ref", False), ["TF == TR == 32768", "128 rounds"])
_reg("counter_max_alt", lambda: counter_max_case("counter_max_alt", True), ["TF == TR == 32768", "alt tile 1: 65536 survivors"])
SEG_REQUIRED = ["exactly at q", "exactly at q+1", "exactly at q+L", "exactly at q+L+1", "the last before tile_end"]
for _kind in ("del", "ins"):
    for _s in (63, 64, 65, 66):
        for _v in (100, 600):
            _name = f"seg_{_kind}_{_s}_{_v}"
            _reg(_name, (lambda nm, k, s, v: lambda: segments_case(nm, k, s, v))(_name, _kind, _s, _v),
                 [f"{_s} segments start before tile_end", f"{_v} valid", "list path" if _v <= LIST_CAP else "recompute path"] + SEG_REQUIRED
                 + (["segment of its own"] if _kind == "ins" else []))
for _v in (100, 600):
    _reg(f"seg_tail_{_v}", (lambda v: lambda: segments_case(f"seg_tail_{v}", "del", 65, v, tail=True))(_v),
         ["65 segments start before tile_end", "behind the tile", f"{_v} valid"] + SEG_REQUIRED)
for _L, _g in ((44, 41), (13, 10)):
    for _right in (False, True):
        _name = f"geom_L{_L}_{'right' if _right else 'left'}"
        _reg(_name, (lambda nm, g, r: lambda: geometry_case(nm, "NGG", g, r))(_name, _g, _right),
             [f"L = {_L}, W = {_L + 20}", "row 0 strand 0", "row 0 strand 1", "row 1 strand 0", "row 1 strand 1", "first of the next tile"])
for _L, _g in ((32, 29), (33, 30)):  # start 0's + strand PAM and start 31's - strand PAM would share letters: one strand per case
    for _right in (False, True):
        for _s in (0, 1):
            _name = f"geom_L{_L}_{'right' if _right else 'left'}_s{_s}"
            _rels = (REL_STARTS, ()) if _s == 0 else ((), REL_STARTS)
            _reg(_name, (lambda nm, g, r, rl: lambda: geometry_case(nm, "NGG", g, r, rl))(_name, _g, _right, _rels),
                 [f"L = {_L}, W = {_L + 20}", f"row 0 strand {_s}", f"row 1 strand {_s}", "first of the next tile"])
_reg("geom_cpf1", lambda: geometry_case("geom_cpf1", "TTTV", 23, True, CPF1_STARTS), ["L = 27", "row 1 strand 0", "row 1 strand 1"])
for _n, _what in ((2048, "0 (mod 32)"), (2049, "1 (mod 32)"), (2079, "31 (mod 32)"), (32704, "1 tile(s)"), (32705, "2 tile(s)")):
    for _right in (False, True):
        _name = f"ends_{_n}_{'right' if _right else 'left'}"
        _reg(_name, (lambda nm, n, r: lambda: ends_case(nm, n, r))(_name, _n, _right), [_what, "row 1 strand 1", "n_hits > n_candidates"])
for _right in (False, True):
    for _s in (0, 1):
        _name = f"scan_edges_{'right' if _right else 'left'}_s{_s}"
        _reg(_name, (lambda nm, r, s: lambda: scan_edges_case(nm, r, s))(_name, _right, _s), [f"row 0 strand {_s}", f"row 1 strand {_s}"])
TILE_COUNTS = (1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 513, 1024, 1025, 2047, 2048, 2049, 3073)
for _n in TILE_COUNTS:
    _reg(f"tiles_{_n}", (lambda n: lambda: tiles_case(f"tiles_{n}", n))(_n), [f"{_n} tiles of one row each", "i % 3 rows"])
_reg("tiles_2049_big", lambda: tiles_case("tiles_2049_big", 2049, 1500), ["2049 tiles", "row 1500 keeps 513 -> recompute", "k_mscan23's second workgroup"])
PAM_SCAN_SETS = ("tiles_513", "tiles_1025", "tiles_2049")
