"""Shared by tests/test_resolve_host.py and tests/test_gpu_resolve_unphased.py: table rows derived from haplotype strings the
way the reference's retrieve_guides derives them (search_guides.py:463-471), the expected guide list by the Python restatement
(resolve_guide + remove_redundant_guides), the host twin (hawk_host_resolve_unphased) on such rows, and the seam panel.

A panel scene is a REF haplotype over a background alphabet that cannot hold the PAM on either strand, guides planted at chosen
positions, and non-REF haplotypes that are copies of REF (or short windows with coordinates of their own) with lower-case IUPAC
letters and their allele entries at chosen positions - so every row of a scene is there on purpose."""
from types import SimpleNamespace

import numpy as np

from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.crisprhawk_error import CrisprHawkCfdScoreError
from crisprhawk_hip.guide import GUIDESEQPAD
from crisprhawk_hip.haplotype import Haplotype
from crisprhawk_hip.hapset import ResolvedColumns, resolve_columns_host
from crisprhawk_hip.pam import IUPAC_BITS, PAM
from crisprhawk_hip.region import Region
from crisprhawk_hip.search_guides import (compute_scan_start_stop, extract_guide_sequence, flatten_variant_alleles,
                                          is_pamhit_in_range, is_pamhit_valid, remove_redundant_guides, resolve_guide)
from crisprhawk_hip.sequence import Sequence

G4_FIXTURES = ["g4_unphased", "g4_unphased_cpf1", "g4_unphased_dense"]
_CODE = {c: i for i, c in enumerate("?ACMGRSVTWYHKDBN")}
_CODE.update({c.lower(): i | 16 for c, i in list(_CODE.items()) if c != "?"})


def encode_windows(seqs):
    """cased strings -> [5, n] window slices (bit 0 = leftmost base), the inverse of hapset.decode_windows"""
    out = np.zeros((5, len(seqs)), np.uint64)
    for k, s in enumerate(seqs):
        for i, ch in enumerate(s):
            code = _CODE[ch]
            for p in range(5):
                if (code >> p) & 1:
                    out[p, k] |= np.uint64(1) << np.uint64(i)
    return out


def py_pam_hits(seq: str, pam: PAM, start: int, stop: int):
    """scan_haplotype (search_guides.py:87-99) on the string: a nibble-wise set intersection per strand"""
    nib = [IUPAC_BITS[c.upper()] for c in seq]
    out = []
    for pat in (pam.pam, pam.pamrc):
        pb = [IUPAC_BITS[c] for c in pat]
        out.append([p for p in range(start, stop) if all(pb[i] & nib[p + i] for i in range(len(pb)))])
    return out[0], out[1]


def haplotypes_from_fixture(fx):
    """the fixture's haplotypes as objects (as tests/test_gpu_api.py builds them) -> (region, haps, pam)"""
    from util import posmap_from_breaks
    region = Region(Sequence(fx["region_seq"], True), Coordinate(fx["contig"], fx["bed_start"], fx["bed_stop"], 100))
    haps = []
    for i, gh in enumerate(fx["haplotypes"]):
        sp, ep, s0, e0 = gh["coord"]
        h = Haplotype(Sequence(gh["seq"], True, allow_lower_case=True), Coordinate(gh["contig"], sp, ep, sp - s0), False, 0, True)
        h.samples, h.variants = gh["samples"], gh["variants"]
        h.set_posmap({k: int(v) for k, v in enumerate(posmap_from_breaks(gh["posmap_breaks"], gh["posmap_len"]))})
        h.set_variant_alleles({int(k): [tuple(t) for t in v] for k, v in gh["variant_alleles"].items()})
        h.id = f"hap_{i:08d}"
        haps.append(h)
    pam = PAM(fx["pam"], fx["right"], True)
    pam.encode(0)
    return region, haps, pam


def derive_rows(haps, hits, pamlen: int, guidelen: int, right: bool):
    """The table rows of a haplotype list and its PAM hits, in emission order (haplotype, strand, position): in-range hits whose
    core is not all upper case on a non-REF haplotype (retrieve_guides, search_guides.py:463-471).  flags bit 0: REF has a row
    at the same (start, strand).  Columns as numpy arrays + the windows as strings."""
    rows = []
    for hi, h in enumerate(haps):
        for strand in (0, 1):
            r = (not right) if strand == 1 else right
            for pos in hits[hi][strand]:
                if not is_pamhit_in_range(pos, guidelen, pamlen, len(h), r):
                    continue
                seq = extract_guide_sequence(h, pos, pamlen, guidelen, r)
                if h.samples != "REF" and seq[GUIDESEQPAD:-GUIDESEQPAD].isupper():
                    continue
                pivot = pos if r else pos - guidelen
                start, stop = (int(x) for x in h.segments.lookup(np.array([pivot, pivot + guidelen + pamlen])))
                rows.append((hi, pos, strand, start, stop, seq))
    refkeys = {(r[3], r[2]) for r in rows if haps[r[0]].samples == "REF"}
    t = SimpleNamespace()
    t.n_rows = len(rows)
    t.hap = np.array([r[0] for r in rows], np.uint32); t.pos = np.array([r[1] for r in rows], np.uint32)
    t.strand = np.array([r[2] for r in rows], np.uint8); t.start = np.array([r[3] for r in rows], np.int64)
    t.stop = np.array([r[4] for r in rows], np.int64)
    t.flags = np.array([1 if (r[3], r[2]) in refkeys else 0 for r in rows], np.uint8)
    t.seqs = [r[5] for r in rows]
    t.win = encode_windows(t.seqs)
    t.emission_order = lambda: np.lexsort((t.pos, t.strand, t.hap))
    return t


def expected_guides(haps, t, pam: PAM, guidelen: int, right: bool):
    """The Python restatement on the rows: resolve_guide per valid row in emission order, remove_redundant_guides on the lot ->
    [[start, stop, strand, sequence, hap, right, samples]] in the reference's list order."""
    guides = []
    for i in t.emission_order():
        h = haps[int(t.hap[i])]
        strand, pos = int(t.strand[i]), int(t.pos[i])
        r = (not right) if strand == 1 else right
        if not is_pamhit_valid(pos, len(h), guidelen, len(pam), r):
            continue
        for seq in resolve_guide(t.seqs[i], pam, strand, r, pos, guidelen, h, True):
            guides.append(SimpleNamespace(start=int(t.start[i]), stop=int(t.stop[i]), strand=strand, sequence=seq, samples=h.samples,
                                          hap=int(t.hap[i]), right=r))
    return [[g.start, g.stop, g.strand, g.sequence, g.hap, g.right, g.samples] for g in remove_redundant_guides(guides, True)]


def twin(haps, t, pam: PAM, guidelen: int, right: bool, batch_bytes=None) -> ResolvedColumns:
    """hawk_host_resolve_unphased on the rows"""
    res = ResolvedColumns()
    res.n_resolved = np.zeros(t.n_rows, np.uint32); res.n_kept = np.zeros(t.n_rows, np.uint32)
    hap_len = np.array([len(h) for h in haps], np.uint32)
    is_ref = np.array([h.samples == "REF" for h in haps], np.uint8)
    res.src_row, res.win = resolve_columns_host(t.hap, t.pos, t.strand, t.start, t.flags, t.win, hap_len, is_ref, flatten_variant_alleles(haps),
                                                pam.bits, pam.bitsrc, guidelen, len(pam), right, res.n_resolved, res.n_kept, batch_bytes)
    res.window_len, res.engine, res.timing = guidelen + len(pam) + 2 * GUIDESEQPAD, "host", {}
    return res


def guides_of(res: ResolvedColumns, haps, t, right: bool):
    """the resolved columns as the list expected_guides returns, in ResolvedColumns.reference_order"""
    seqs = res.windows()
    out = []
    for k in res.reference_order(t):
        i = int(res.src_row[k])
        strand = int(t.strand[i])
        out.append([int(t.start[i]), int(t.stop[i]), strand, seqs[k], int(t.hap[i]), (not right) if strand == 1 else right,
                    haps[int(t.hap[i])].samples])
    return out


# ---------------------------------------------------------------------------- the seam panel
class Scene:
    """REF over `bg` (an alphabet without the PAM on either strand), planted guides, non-REF haplotypes with IUPAC letters"""

    def __init__(self, name: str, pam: str, guidelen: int, right: bool, n: int = 420, seed: int = 1):
        self.name, self.pam_s, self.guidelen, self.right, self.n = name, pam, guidelen, bool(right), n
        bg = "AT" if pam in ("NGG",) else "CG"
        rng = np.random.default_rng(7000 + seed)
        self.ref = [bg[int(x)] for x in rng.integers(0, 2, n)]
        self.g0 = 5000            # genomic position of REF's base 0 (the padded region start)
        self.haps = []            # (kind, start, stop, {pos: letter}, {pos: entries}, samples)
        self.ref_last = False
        self.ref_alleles = {}     # pos -> entries of REF itself (the REF_AMBIG decline)
        self.claims = {}

    def plant(self, pos: int, text: str) -> int:
        self.ref[pos:pos + len(text)] = list(text)
        return pos

    def copy(self, samples: str, edits: dict) -> None:
        """a full-length copy of REF; edits: pos -> (letter, entries or None)"""
        self.haps.append((0, self.n, edits, samples))

    def window(self, samples: str, a: int, b: int, edits: dict) -> None:
        """REF[a:b] as a haplotype with coordinates of its own (what the reference builds around an indel)"""
        self.haps.append((a, b, edits, samples))

    def build(self):
        """-> (region, haplotypes, pam)"""
        ref = "".join(self.ref)
        region = Region(Sequence(ref, True), Coordinate("chrP", self.g0 + 100, self.g0 + self.n - 100, 100))
        hs = [Haplotype(Sequence(ref, True), region.coordinates, False, 0, True)]
        hs[0].set_variant_alleles({p: [(r, al, self.g0 + p) for r, al in e] for p, e in self.ref_alleles.items()})
        for a, b, edits, samples in self.haps:
            s = list(ref[a:b])
            va = {}
            for p, (letter, entries) in edits.items():
                s[p - a] = letter
                if entries is not None:
                    va[p - a] = [(r, al, self.g0 + p) for r, al in entries]
            coord = region.coordinates if (a, b) == (0, self.n) else Coordinate("chrP", self.g0 + a, self.g0 + b - 1, 0)
            h = Haplotype(Sequence("".join(s), True, allow_lower_case=True), coord, False, 0, True)
            h.samples, h.variants = samples, "NA"
            h.set_variant_alleles(va)
            hs.append(h)
        if self.ref_last:
            hs = hs[1:] + hs[:1]
        for i, h in enumerate(hs):
            h.id = f"hap_{i:08d}"
        pam = PAM(self.pam_s, self.right, True)
        pam.encode(0)
        return region, hs, pam

    def rows(self):
        region, haps, pam = self.build()
        hits = []
        for h in haps:
            a, b = compute_scan_start_stop(h, region.start, region.stop, len(pam))
            hits.append(py_pam_hits(h.sequence.sequence, pam, a, b))
        return region, haps, pam, derive_rows(haps, hits, len(pam), self.guidelen, self.right)


AG = [("A", "G")]


def _ngg_pair(s: Scene, p0: int, p1: int):
    """a strand-0 guide with its AGG at p0 and a strand-1 guide with its CCA at p1"""
    s.plant(p0, "AGG")
    s.plant(p1, "CCA")


def panel():
    """name -> Scene.  What each scene is there for is in its `claims`, checked by test_resolve_host.test_panel_claims."""
    out = {}

    def add(s):
        out[s.name] = s
        return s

    # options: k = 2 at a 3-letter code (6 options, each base twice), a 4-letter code, a multi-base ref (all lower case)
    s = add(Scene("options", "NGG", 20, False, seed=1))
    s.plant(200, "AGG")
    s.ref[190] = "A"; s.ref[185] = "A"; s.ref[180] = "A"
    s.copy("S1", {190: ("d", [("A", "G"), ("A", "T")])})
    s.copy("S2", {185: ("n", [("A", "C")])})
    s.copy("S3", {180: ("r", [("AT", "A")])})
    s.claims = dict(n_resolved=[1, 6, 4, 2], n_kept=[1, 4, 3, 1])
    # an ambiguous position in the left pad, the spacer, the first and the last PAM base and the right pad of one window; the
    # last PAM base keeps only its G; combinations that equal REF, differ in the flanks only (dropped) or in the core (kept)
    s = add(Scene("positions", "NGG", 20, False, seed=2))
    s.plant(200, "AGG")
    for p in (173, 195, 208):
        s.ref[p] = "A"
    s.copy("S1", {173: ("w", [("A", "T")]), 195: ("r", AG), 200: ("r", AG), 202: ("r", [("G", "A")]), 208: ("w", [("A", "T")])})
    s.claims = dict(n_resolved=[1, 16, 16], n_kept=[1, 16, 12])  # (the r under the N makes a second PAM one base to the left: no REF partner there)
    # both strands of a left-sided PAM: strand 1 has `right` True as stored; a PAM position where only some options survive
    s = add(Scene("strands_left", "NGG", 20, False, seed=3))
    _ngg_pair(s, 160, 260)
    s.ref[150] = "A"; s.ref[270] = "A"
    s.copy("S1", {150: ("r", AG), 161: ("k", [("G", "T")]), 270: ("r", AG), 261: ("m", [("C", "A")])})
    s.claims = dict(n_resolved=[1, 1, 2, 2], n_kept=[1, 1, 1, 1])
    # the same for a right-sided PAM (Cpf1): strand 0 has `right` True, strand 1 False; the V of TTTV and the B of BAAA thin an n
    s = add(Scene("strands_right", "TTTV", 23, True, seed=4))
    s.plant(150, "TTTC")
    s.plant(280, "GAAA")
    s.copy("S1", {153: ("n", [("C", "A")]), 160: ("s", [("C", "G")]), 280: ("n", [("G", "T")]), 270: ("s", [("C", "G")])})
    s.claims = dict(n_resolved=[1, 1, 6, 2, 2, 6], n_kept=[1, 1, 5, 2, 2, 5])  # (each n, read as T / A, makes a second PAM beside the planted one)
    # W = 64: every bit of a window slice in use; W = 33: the first window longer than a word; and the smallest guide there is,
    # one base (W = pamlen + 21: a core that is nearly all PAM), ambiguous letters in its spacer and both pads on both strands
    s = add(Scene("widest", "NGG", 41, False, n=460, seed=5))
    _ngg_pair(s, 200, 300)
    s.ref[149] = "A"; s.ref[212] = "A"; s.ref[290] = "A"; s.ref[353] = "A"
    s.copy("S1", {149: ("w", [("A", "T")]), 170: ("s" if s.ref[170] in "CG" else "w", [(s.ref[170], "T" if s.ref[170] == "A" else "A")]),
                  212: ("w", [("A", "T")]), 290: ("w", [("A", "T")]), 353: ("w", [("A", "T")]), 320: ("w", [(s.ref[320], "T" if s.ref[320] == "A" else "A")])})
    s.claims = dict(n_resolved=[1, 1, 8, 8], n_kept=[1, 1, 4, 4])
    s = add(Scene("w33", "NGG", 10, False, seed=6))
    _ngg_pair(s, 200, 300)
    s.copy("S1", {195: ("w", [(s.ref[195], "T" if s.ref[195] == "A" else "A")]), 305: ("w", [(s.ref[305], "T" if s.ref[305] == "A" else "A")])})
    s.claims = dict(n_resolved=[1, 1, 2, 2], n_kept=[1, 1, 1, 1])
    s = add(Scene("shortest", "NGG", 1, False, seed=10))
    _ngg_pair(s, 200, 300)
    w = lambda p: ("w", [(s.ref[p], "T" if s.ref[p] == "A" else "A")])
    s.copy("S1", {p: w(p) for p in (190, 199, 210, 292, 303, 312)})
    s.claims = dict(n_resolved=[1, 1, 8, 8], n_kept=[1, 1, 4, 4])
    # a window that ends exactly with its haplotype: in the table, not valid, no guides; the same guide one base earlier is valid
    s = add(Scene("hap_end", "NGG", 20, False, seed=7))
    s.plant(200, "CCA")   # strand 1, stored right: window [190, 233)
    s.ref[215] = "A"
    s.window("S1", 150, 233, {215: ("r", AG)})   # rbound == len
    s.window("S2", 150, 234, {215: ("r", AG)})   # one base more
    s.claims = dict(n_resolved=[1, 0, 2], n_kept=[1, 0, 1])
    # a key without a REF partner: a PAM only the variant makes - everything is kept
    s = add(Scene("no_partner", "NGG", 20, False, seed=8))
    s.plant(200, "AGA")
    s.ref[190] = "A"
    s.copy("S1", {202: ("r", [("A", "G")]), 190: ("w", [("A", "T")])})
    s.claims = dict(n_resolved=[2], n_kept=[2])
    # REF last in the list: first-seen order of the keys changes, the redundancy rule does not
    s = add(Scene("ref_last", "NGG", 20, False, seed=9))
    _ngg_pair(s, 160, 260)
    s.ref[150] = "A"; s.ref[270] = "A"
    s.copy("S1", {150: ("r", AG), 270: ("r", AG)})
    s.copy("S2", {150: ("m", [("A", "C")])})
    s.ref_last = True
    s.claims = dict(n_resolved=[2, 2, 2, 1, 1], n_kept=[1, 1, 1, 1, 1])
    return out


def decline_scenes():
    """name -> (Scene, reason, exception of the host route)"""
    out = {}
    s = Scene("no_entry", "NGG", 20, False, seed=20)   # an N of the genome inside a window
    s.plant(200, "AGG")
    s.copy("S1", {190: ("g", None), 185: ("N", None)})
    out[s.name] = (s, 1, KeyError)
    s = Scene("multi_ref", "NGG", 20, False, seed=21)
    s.plant(200, "AGG")
    s.copy("REF", {})
    out[s.name] = (s, 2, CrisprHawkCfdScoreError)
    s = Scene("ref_ambig", "NGG", 20, False, seed=22)   # REF itself resolves to two guides at one key: "Duplicate REF guide"
    s.plant(200, "AGG")
    s.ref[190] = "W"
    s.ref_alleles = {190: [("A", "T")]}
    out[s.name] = (s, 3, CrisprHawkCfdScoreError)
    return out


def wide_row_scene(n_amb: int, name: str = "wide_row", seed: int = 30, partner: bool = True) -> Scene:
    """one non-REF row with n_amb two-way positions, in its spacer first (20) and then in its left pad: 2^n_amb combinations.
    With a REF partner the one that is REF's core goes (times the pad's share); without - the PAM's last G is the variant's - all stay."""
    s = Scene(name, "NGG", 20, False, seed=seed)
    s.plant(200, "AGG" if partner else "AGA")
    edits = {} if partner else {202: ("r", [("A", "G")])}
    for p in (list(range(180, 200)) + list(range(171, 180)))[:n_amb]:
        edits[p] = ("w", [(s.ref[p], "T" if s.ref[p] == "A" else "A")])
    s.copy("S1", edits)
    return s


def many_rows_scene(n_guides: int, name: str, seed: int = 40, n_amb: int = 1) -> Scene:
    """REF with n_guides strand-0 guides 50 nt apart and one copy with n_amb two-way spacer positions per guide: n_guides REF
    rows and n_guides rows of 2^n_amb combinations"""
    s = Scene(name, "NGG", 20, False, n=300 + 50 * n_guides, seed=seed)
    edits = {}
    for k in range(n_guides):
        p = 150 + 50 * k
        s.plant(p, "AGG")
        for j in range(n_amb):
            q = p - 1 - j
            edits[q] = ("w", [(s.ref[q], "T" if s.ref[q] == "A" else "A")])
    s.copy("S1", edits)
    return s
