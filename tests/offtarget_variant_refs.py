"""References and scenes for the off-target scan over a variant-enriched genome (hawk_offtarget_variant_scan and its host twin).

`brute` applies the semantics of include/hawk.h literally, in plain Python over strings: per position a REF letter and a set of
letters, every window of every contig cut out letter by letter, turned into guide orientation and resolved against every
guide.  It knows no rows, no masks and no 2-bit codes.  `Scene` places its cases by construction - each site is written into a
random contig at a chosen position and strand, with REF edits and ALT alleles given at window positions in guide orientation -
and records what it placed, so that a test can first hold the brute force to the scene (the case is really there) and then the
library to the brute force."""
import functools
import random

import numpy as np

from crisprhawk_hip.pam import PAM

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "N": "ACGT", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
PIECE = 1024


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def make_pam(text, right):
    pam = PAM(text, right, True)
    pam.encode(0)
    return pam


def allele_sets(contigs, records):
    """({contig: [set of letters per position]}, stats) by the drop rules of the issue: a record is dropped and counted, never
    raised"""
    sets = {name: [{c} if c in "ACGT" else set() for c in seq.upper()] for name, seq in contigs.items()}
    dropped = dict(not_snv=0, unknown_contig=0, out_of_contig=0, ref_n=0, ref_mismatch=0, alt_is_ref=0, no_row=0, other_shard=0)
    applied = 0
    for contig, pos, ref, alts in records:
        for alt in alts.split(","):
            ref, alt = ref.upper(), alt.upper()
            if len(ref) != 1 or len(alt) != 1 or ref not in "ACGT" or alt not in "ACGT":
                dropped["not_snv"] += 1
            elif contig not in contigs:
                dropped["unknown_contig"] += 1
            elif not 0 <= pos < len(contigs[contig]):
                dropped["out_of_contig"] += 1
            elif alt == ref:
                dropped["alt_is_ref"] += 1
            elif contigs[contig][pos].upper() not in "ACGT":
                dropped["ref_n"] += 1
            elif contigs[contig][pos].upper() != ref:
                dropped["ref_mismatch"] += 1
            else:
                sets[contig][pos].add(alt)
                applied += 1
    return sets, dict(applied=applied, dropped=dropped)


def brute(contigs, records, guides, pam_text, right, max_mm):
    """sorted [(guide, contig, pos, strand, mm, resolved window, alt mask)] of the variant rows"""
    sets, _stats = allele_sets(contigs, records)
    G, P = len(guides[0]), len(pam_text)
    L = G + P
    sp0, pam0 = (P, 0) if right else (0, G)
    out = []
    for name, seq in contigs.items():
        seq = seq.upper()
        for s in range(len(seq) - L + 1):
            if all(len(a) <= 1 for a in sets[name][s:s + L]):
                continue  # no ALT allele in the window: whatever it yields has alt == 0
            for strand in (0, 1):
                ref = [c if c in "ACGT" else "N" for c in seq[s:s + L]]
                al = [set(a) for a in sets[name][s:s + L]]
                if strand:
                    ref = [COMP[c] for c in reversed(ref)]
                    al = [{COMP[c] for c in a} for a in reversed(al)]
                res, alt, ok = list(ref), 0, True
                for k in range(P):
                    i = pam0 + k
                    if pam_text[k] == "N":
                        continue
                    both = sorted(al[i] & set(IUPAC[pam_text[k]]))
                    if not both:
                        ok = False
                        break
                    if ref[i] in IUPAC[pam_text[k]] and ref[i] != "N":
                        continue
                    res[i] = both[0]
                    alt |= 1 << i
                if not ok:
                    continue
                for gi, g in enumerate(guides):
                    r, a, mm = list(res), alt, 0
                    for j in range(G):
                        i = sp0 + j
                        if g[j] in al[i]:
                            r[i] = g[j]
                            if g[j] != ref[i]:
                                a |= 1 << i
                        else:
                            mm += 1
                            if mm > max_mm:
                                break
                    if mm <= max_mm and a:
                        out.append((gi, name, s, strand, mm, "".join(r), a))
    return sorted(out)


def sites(contigs, records, pam_text, G, right):
    """{(contig, start, strand)} of the windows that lie wholly in their contig, hold an ALT allele at one position at least and
    bear the PAM: in guide orientation every PAM position is 'N' or has an allele set that meets the PAM letter's IUPAC set (a
    position with an ambiguous REF base holds the empty set).  What hawk_offtarget_variant_scan counts in timing.n_sites."""
    sets, _stats = allele_sets(contigs, records)
    P = len(pam_text)
    L = G + P
    pam0 = 0 if right else G
    pam_sets = [None if c == "N" else set(IUPAC[c]) for c in pam_text]
    out = set()
    for name in contigs:
        col = sets[name]
        for s in range(len(col) - L + 1):
            win = col[s:s + L]
            if all(len(a) <= 1 for a in win):
                continue
            for strand in (0, 1):
                w = [{COMP[c] for c in a} for a in reversed(win)] if strand else win
                if all(p is None or (w[pam0 + k] & p) for k, p in enumerate(pam_sets)):
                    out.add((name, s, strand))
    return out


def rows_as_tuples(h, rows, L):
    """the columns of variant_arrays / host_variant_scan as brute's tuples; `rows` = [(contig, offset, ...)] of the index"""
    if not len(h["guide"]):
        return []
    k = np.arange(L, dtype=np.uint64)
    letters = np.frombuffer(b"ACGT", np.uint8)[((h["code"].astype(np.uint64)[:, None] >> (2 * k)) & np.uint64(3)).astype(np.intp)]
    letters[((h["nmask"].astype(np.uint64)[:, None] >> k) & np.uint64(1)).astype(bool)] = ord("N")
    wins = [w.decode() for w in np.ascontiguousarray(letters).view(f"S{L}").ravel().tolist()]
    where = [(rows[r][0], rows[r][1] + q) for r, q in zip(h["row"].tolist(), h["q"].tolist())]
    return sorted((g, name, pos, s, mm, w, a) for g, (name, pos), s, mm, w, a in
                  zip(h["guide"].tolist(), where, h["strand"].tolist(), h["mm"].tolist(), wins, h["alt"].tolist()))


def raw_tuples(h):
    return sorted(zip(*(h[k].tolist() for k in ("guide", "row", "q", "strand", "mm", "code", "nmask", "alt"))))


class Scene:
    """Contigs of random bases with sites written into them.  place(): the window `guide + PAM` (PAM in front when `right`) in
    guide orientation, with `edits` {window position: REF letter} applied, lands at `pos` on `strand`; `alts` {window position:
    letters} become records (contig, genome position, REF, ALT) on the + strand."""

    def __init__(self, pam_text, G, right, seed, lengths=(3000, 2500), n_guides=8, alphabet="ACGT"):
        """`alphabet`: the letters the contigs are drawn from - a background without G and C bears no NGG on either strand, so
        that every PAM-bearing window of the scene is one that was placed"""
        self.rng = random.Random(seed)
        self.pam_text, self.G, self.right = pam_text, G, right
        self.P = len(pam_text)
        self.L = G + self.P
        self.pam_site = "".join(IUPAC[c][-1] if c != "N" else "T" for c in pam_text)  # NGG -> TGG, TTTV -> TTTG
        self.contigs = {f"chr{k + 1}": [self.rng.choice(alphabet) for _ in range(n)] for k, n in enumerate(lengths)}
        self.guides = ["".join(self.rng.choice("ACGT") for _ in range(G)) for _ in range(n_guides)]
        self.records = []
        self.placed = {}  # label -> (guide, contig, pos, strand)
        self.spans = []   # (contig, pos, pos + L) of everything placed
        self.want = {}    # label -> (mm, resolved window, alt mask): the row the placed case must have (seam scenes)
        self.min_mm = {}  # label -> the smallest max_mm at which that row exists (default 0); below it the pair has no row
        self.absent = []  # (contig, pos): windows that bear a perfect PAM and guide and must be no site on either strand
        self._memo = {}

    def window(self, gi):
        return (self.pam_site + self.guides[gi]) if self.right else (self.guides[gi] + self.pam_site)

    def sp(self, j):
        """window position of spacer base j"""
        return (self.P if self.right else 0) + j

    def pm(self, k):
        """window position of PAM base k"""
        return (0 if self.right else self.G) + k

    def other(self, c, avoid=""):
        return self.rng.choice([x for x in "ACGT" if x != c and x not in avoid])

    def place(self, label, contig, pos, strand, gi, edits=None, alts=None, ref_as=None):
        win = list(self.window(gi))
        for i, c in (edits or {}).items():
            win[i] = c
        plus = win if not strand else [COMP[c] for c in reversed(win)]
        self.contigs[contig][pos:pos + self.L] = plus
        for i, letters in (alts or {}).items():
            gpos = pos + (self.L - 1 - i if strand else i)
            refc = self.contigs[contig][gpos]
            stated = (ref_as or {}).get(i, refc)
            self.records.append((contig, gpos, stated, ",".join(COMP[a] if strand else a for a in letters)))  # multi-allelic: one record
        self.placed[label] = (gi, contig, pos, strand)
        self.spans.append((contig, pos, pos + self.L))

    def brute(self, max_mm, guides=None):
        """brute() of the finished scene, computed once per (max_mm, guides) and shared: the scene must not change afterwards"""
        key = ("brute", max_mm, None if guides is None else tuple(guides))
        if key not in self._memo:
            self._memo[key] = brute(self.text(), self.records, self.guides if guides is None else guides, self.pam_text, self.right, max_mm)
        return self._memo[key]

    def sites(self):
        if "sites" not in self._memo:
            self._memo["sites"] = sites(self.text(), self.records, self.pam_text, self.G, self.right)
        return self._memo["sites"]

    def text(self):
        return {name: "".join(seq) for name, seq in self.contigs.items()}


def standard_scene(pam_text, G, right, max_mm, seed=5, with_n=True):
    """The cases of the issue, each on both strands, sites 2 L apart so that no window sees two of them.  `with_n` False leaves the
    two N bases out (a table with CFD scores refuses a row with an N under a lookup)."""
    sc = Scene(pam_text, G, right, seed)
    L, P = sc.L, sc.P
    pam_k = next(k for k, c in enumerate(pam_text) if c != "N")       # a PAM position that constrains
    pam_n = next((k for k, c in enumerate(pam_text) if len(IUPAC[c]) > 1), None)  # one that admits several bases
    slot = iter(range(2 * L, 2400, 2 * L + 7))
    for strand in (0, 1):
        tag = "+-"[strand]
        c1, c2 = "chr1", "chr2"
        # an alt that creates the PAM: REF breaks a constraining PAM base, the ALT restores it
        good = sc.pam_site[pam_k]
        bad = sc.other(good, IUPAC[pam_text[pam_k]])
        sc.place("pam_created" + tag, c1, next(slot), strand, 0, {sc.pm(pam_k): bad}, {sc.pm(pam_k): good})
        # an alt under a PAM position that admits it and REF: REF stays, no row - unless another position takes an alt
        if pam_n is not None:
            refc = sc.pam_site[pam_n]
            altc = next(x for x in IUPAC[pam_text[pam_n]] if x != refc)
            sc.place("pam_n_only" + tag, c1, next(slot), strand, 1, None, {sc.pm(pam_n): altc})
            g = sc.guides[1]
            sc.place("pam_n_and_spacer" + tag, c1, next(slot), strand, 1, {sc.sp(4): sc.other(g[4])}, {sc.pm(pam_n): altc, sc.sp(4): g[4]})
        # an alt that turns max_mm + 1 mismatches into max_mm
        g = sc.guides[2]
        spots = list(range(3, 3 + 2 * (max_mm + 1), 2))
        sc.place("mm_rescued" + tag, c1, next(slot), strand, 2, {sc.sp(j): sc.other(g[j]) for j in spots}, {sc.sp(spots[0]): g[spots[0]]})
        # an alt that matches no guide base (the window itself is a perfect REF site: the plain scan's row, no variant row)
        g = sc.guides[3]
        sc.place("alt_unused" + tag, c1, next(slot), strand, 3, None, {sc.sp(7): sc.other(g[7])})
        # two and three variants in one window, each needed
        g = sc.guides[4]
        sc.place("two_in_window" + tag, c2, next(slot), strand, 4, {sc.sp(2): sc.other(g[2]), sc.sp(11): sc.other(g[11])},
                 {sc.sp(2): g[2], sc.sp(11): g[11]})
        sc.place("three_in_window" + tag, c2, next(slot), strand, 4, {sc.sp(1): sc.other(g[1]), sc.sp(9): sc.other(g[9]), sc.sp(15): sc.other(g[15])},
                 {sc.sp(1): g[1], sc.sp(9): g[9], sc.sp(15): g[15]})
        # two ALTs at one position: one is the guide's
        g = sc.guides[5]
        r = sc.other(g[6])
        sc.place("two_alts" + tag, c2, next(slot), strand, 5, {sc.sp(6): r}, {sc.sp(6): sc.other(g[6], r) + g[6]})
        # variants at window positions 0 and L - 1
        g = sc.guides[6]
        w = sc.window(6)
        e0 = sc.other(w[0], IUPAC.get(pam_text[0], "") if right else "")
        e1 = sc.other(w[L - 1], "" if right else IUPAC[pam_text[P - 1]])
        sc.place("window_ends" + tag, c2, next(slot), strand, 6, {0: e0, L - 1: e1}, {0: w[0], L - 1: w[L - 1]})
        # a variant beside an N (the N is a mismatch: a row only from max_mm 1 on)
        g = sc.guides[7]
        if with_n:
            sc.place("beside_n" + tag, c2, next(slot), strand, 7, {sc.sp(12): "N", sc.sp(13): sc.other(g[13])}, {sc.sp(13): g[13]})
        # dropped and counted: on a REF N, with a wrong REF, with alt == ref
        g = sc.guides[0]
        wrong = sc.other(g[8])
        plus = lambda c: COMP[c] if strand else c
        third = lambda a, b: next(x for x in "ACGT" if x not in (plus(a), plus(b)))  # a stated REF that is neither the ALT nor the index's base
        sc.place("dropped" + tag, c1, next(slot), strand, 0, {sc.sp(5): "N", sc.sp(8): wrong} if with_n else {sc.sp(8): wrong},
                 {sc.sp(5): g[5], sc.sp(8): g[8], sc.sp(10): g[10]} if with_n else {sc.sp(8): g[8], sc.sp(10): g[10]},
                 ref_as={sc.sp(5): third(g[5], g[5]), sc.sp(8): third(g[8], wrong)})
    # windows at contig starts and ends, each needing its alt
    for label, contig, pos, strand, gi in (("start1", "chr1", 0, 0, 1), ("end1", "chr1", len(sc.contigs["chr1"]) - L, 1, 2),
                                           ("start2", "chr2", 0, 1, 3), ("end2", "chr2", len(sc.contigs["chr2"]) - L, 0, 4)):
        g = sc.guides[gi]
        sc.place(label, contig, pos, strand, gi, {sc.sp(0): sc.other(g[0]), sc.sp(G - 1): sc.other(g[G - 1])}, {sc.sp(0): g[0], sc.sp(G - 1): g[G - 1]})
    # alt == ref stated outright, a record that is no SNV, an unknown contig, a position outside its contig
    c = sc.contigs["chr1"][1500]
    sc.records += [("chr1", 1500, c, c), ("chr1", 1501, "AT", "A"), ("chr1", 1502, sc.contigs["chr1"][1502], "<DEL>"), ("chrUn", 5, "A", "C"),
                   ("chr2", 10 ** 6, "A", "C")]
    # a contig shorter than a window, with a variant on it
    sc.contigs["tiny"] = list(("ACGT" * 8)[:L - 3])
    sc.records.append(("tiny", 3, sc.contigs["tiny"][3], sc.other(sc.contigs["tiny"][3])))
    return sc


def expect_rows(sc, max_mm):
    """{label: whether the brute force must list a variant row for the placed (guide, contig, pos, strand)}"""
    want = {}
    for label in sc.placed:
        base = label.rstrip("+-")
        if base in ("pam_n_only", "alt_unused", "dropped"):
            want[label] = False
        elif base == "beside_n":
            want[label] = max_mm >= 1
        else:
            want[label] = True
    return want


# ---- scenes at the seams of the device kernels (test_gpu_offtarget_variant_seams.py; test_offtarget_variants_host.py holds them to
# the brute force without a device).  Each builder is cached: a scene and its references are computed once per process and shared,
# and nobody changes a scene after it was built. -------------------------------------------------------------------------------------
WINDOW_SYSTEMS = (("TTTV", 28, True), ("NGG", 29, False), ("NGG", 28, False), ("NG", 6, False), ("NNGRRT", 21, False))  # L = 32, 32, 31, 8, 27
SEAM_SYSTEMS = (("NGG", 20, False, "AT"), ("TTTV", 23, True, "CG"))  # with a background alphabet that bears no PAM on either strand
SEAMS = (32, 128, 8192, 32768)  # in-row bit positions where a bitmap word, a lane's four words, a wave and a workgroup end
BIG_PIECE = 1 << 16
TILE = 32768            # window starts per workgroup of k_scan_raw / k_ov_filter / k_ov_sites


def needed(sc, gi, i):
    """({i: a REF letter that spoils window position i of guide gi's site}, {i: the ALT letter that mends it}): a spacer position
    gets a base that is not the guide's, a PAM position one outside the PAM letter's set"""
    w = sc.window(gi)
    k = i - sc.pm(0)
    return {i: sc.other(w[i], IUPAC[sc.pam_text[k]] if 0 <= k < sc.P else "")}, {i: w[i]}


def place_needed(sc, label, contig, pos, strand, gi, positions):
    """guide gi's site at (contig, pos, strand) with REF spoiled at the window `positions` and the mending ALT at each: its row
    reads mm 0, the site's window and exactly these alt bits"""
    edits, alts = {}, {}
    for i in positions:
        e, a = needed(sc, gi, i)
        edits.update(e)
        alts.update(a)
    sc.place(label, contig, pos, strand, gi, edits, alts)
    sc.want[label] = (0, sc.window(gi), sum(1 << i for i in positions))


def sprinkle(sc, every):
    """random SNVs, one per `every` bases, none within L of a placed window (the claims of the placed cases stay what they are)"""
    for name, seq in sc.contigs.items():
        blocked = [(a - sc.L, b + sc.L) for c, a, b in sc.spans if c == name]
        for pos in range(len(seq)):
            if sc.rng.randrange(every) == 0 and not any(a <= pos < b for a, b in blocked):
                alts = sc.rng.sample([x for x in "ACGT" if x != seq[pos]], sc.rng.choice((1, 1, 2)))
                sc.records.append((name, pos, seq[pos], ",".join(alts)))


def check_claims(sc, rows, max_mm, n_guides=None):
    """`rows` (brute's tuples) and sites() hold what the scene placed; `n_guides`: only the scene's first guides were searched"""
    have = {(g, c, p, s): (mm, w, a) for g, c, p, s, mm, w, a in rows}
    for label, want in sc.want.items():
        if n_guides is not None and sc.placed[label][0] >= n_guides:
            continue
        if max_mm >= sc.min_mm.get(label, 0):
            assert have.get(sc.placed[label]) == want, label
        else:
            assert sc.placed[label] not in have, label
    where = {(c, p) for _g, c, p, _s, _mm, _w, _a in rows}
    for contig, pos in sc.absent:
        assert (contig, pos, 0) not in sc.sites() and (contig, pos, 1) not in sc.sites() and (contig, pos) not in where, (contig, pos)


def owned(keys, rows, row_lo=0, row_hi=None):
    """[(row, start in the row, strand)] of the (contig, start, strand) `keys` whose window start a row of [row_lo, row_hi) owns;
    `rows` = [(contig, offset, ..., owned starts)] as GenomeIndex.rows or row_geometry list them"""
    by = {}
    for k, r in enumerate(rows):
        by.setdefault(r[0], []).append((r[1], r[-1], k))
    out = []
    for contig, start, strand in keys:
        for off, own, k in by.get(contig, ()):
            if off <= start < off + own and row_lo <= k < (len(rows) if row_hi is None else row_hi):
                out.append((k, start - off, strand))
    return out


@functools.lru_cache(maxsize=None)
def window_scene(pam_text, G, right):
    """Window lengths the NGG / 20 and TTTV / 23 scenes never reach.  On each strand (chr1: +, chr2: -) a site that needs an ALT
    at window position 0, at L - 1, at the first and at the last spacer base, a site whose PAM an ALT creates, for L = 32 one with
    ALTs at 0 and 31 together, and one at the contig's first and last window; random SNVs between them."""
    sc = Scene(pam_text, G, right, 7, lengths=(1400, 1200))
    L = sc.L
    pam_k = next(k for k, c in enumerate(pam_text) if c != "N")
    spots = []
    for i in (0, L - 1, sc.sp(0), sc.sp(G - 1), sc.pm(pam_k)):
        if (i,) not in spots:
            spots.append((i,))
    if L == 32:
        spots.append((0, 31))
    for strand, contig in enumerate(("chr1", "chr2")):
        n = len(sc.contigs[contig])
        for k, at in enumerate(spots):
            place_needed(sc, "w" + "_".join(map(str, at)) + "+-"[strand], contig, 2 * L + k * (2 * L + 7), strand, k % 8, at)
        place_needed(sc, "first" + "+-"[strand], contig, 0, strand, 6, (sc.sp(G - 1),))
        place_needed(sc, "last" + "+-"[strand], contig, n - L, strand, 7, (sc.sp(0),))
    sprinkle(sc, 9)
    return sc


@functools.lru_cache(maxsize=None)
def seam_scene(pam_text, G, right, alphabet):
    """Eight contigs of 40000 bases, one row each under BIG_PIECE, two workgroups per row.  One contig per (kind, strand), one
    window per kind at every boundary B of SEAMS:
      far     start B - 1, its needed ALT at the window's last genome base (a PAM base on one strand, a spacer base on the other)
      across  start B - L + 1, its needed ALT at genome position B
      after   a perfect PAM and guide at start B - L, an ALT at B, one past its end: no site
      before  the same at start B + 1, the ALT at B, one before its start: no site
    The background bears no PAM, so the sites of a (strand, row, workgroup) cell are those placed there: behind the seam windows
    every cell gets a number of filler sites of its own, each a site whose row needs its ALT."""
    sc = Scene(pam_text, G, right, 13, lengths=(40000,) * 8, alphabet=alphabet)
    L = sc.L
    for gi in range(8):  # the guides are of the background's letters: no PAM inside them either
        sc.guides[gi] = "".join(sc.rng.choice(alphabet) for _ in range(G))
    for kind, name in enumerate(("far", "across", "after", "before")):
        for strand in (0, 1):
            contig = f"chr{2 * kind + strand + 1}"
            last = 0 if strand else L - 1  # the window position that lies on the window's last genome base
            for gi, B in enumerate(SEAMS):
                label = f"{name}{B}{'+-'[strand]}"
                if name == "far":
                    place_needed(sc, label, contig, B - 1, strand, gi, (last,))
                elif name == "across":
                    place_needed(sc, label, contig, B - L + 1, strand, gi, (last,))
                else:
                    start = B - L if name == "after" else B + 1
                    sc.place(label, contig, start, strand, gi)
                    refc = sc.contigs[contig][B]
                    sc.records.append((contig, B, refc, sc.other(refc)))
                    sc.absent.append((contig, start))
    for row in range(8):
        for wg in range(2):
            slot = (9000, TILE + 700)[wg]
            for strand in (0, 1):
                for j in range(1 + 6 * (2 * row + wg) + 3 * strand):
                    gi = 4 + (j + row) % 4
                    place_needed(sc, f"fill{row}.{wg}{'+-'[strand]}{j}", f"chr{row + 1}", slot, strand, gi, (sc.sp((3 * j + row) % G),))
                    slot += L + 6
    return sc


@functools.lru_cache(maxsize=None)
def row_end_scene(pam_text, G, right, n, strand):
    """One contig of n bases in one row; the last window, at n - L on `strand`, needs an ALT at the contig's last base"""
    sc = Scene(pam_text, G, right, 29 + strand, lengths=(n,))
    place_needed(sc, "end", "chr1", n - sc.L, strand, 0, (0 if strand else sc.L - 1,))
    place_needed(sc, "before", "chr1", n - 3 * sc.L, 1 - strand, 1, (sc.sp(2),))
    sprinkle(sc, 11)
    return sc


DENSE_N, DENSE_RUN = 3004, 200


@functools.lru_cache(maxsize=None)
def dense_scene():
    """NGG / 20, one row: the contig's last 200 positions (in-row offset 2804 = 20 mod 32) carry all three ALTs each, as single
    multi-allelic records - every window inside the run bears the PAM and matches every guide on both strands - and some 400
    further SNVs lie before it, every tenth with a wrong REF.  1100 guides: random ones, three cut from windows that read an ALT."""
    sc = Scene("NGG", 20, False, 43, lengths=(DENSE_N,), n_guides=1100)
    seq = sc.contigs["chr1"]
    for pos in range(DENSE_N - DENSE_RUN, DENSE_N):
        sc.records.append(("chr1", pos, seq[pos], ",".join(x for x in "ACGT" if x != seq[pos])))
    sc.spans.append(("chr1", DENSE_N - DENSE_RUN, DENSE_N))
    for k, slot in enumerate((3, 1030, 1099)):
        place_needed(sc, f"g{slot}", "chr1", 100 + 300 * k, k & 1, slot, (sc.sp(5 + k),))
    lone = []
    for pos in range(30, DENSE_N - DENSE_RUN - 2 * sc.L):
        if sc.rng.randrange(6) == 0 and not any(a - sc.L <= pos < b + sc.L for _c, a, b in sc.spans):
            ref = seq[pos] if sc.rng.randrange(10) else sc.other(seq[pos])
            lone.append(("chr1", pos, ref, ",".join(sc.rng.sample([x for x in "ACGT" if x != ref], sc.rng.choice((1, 2))))))
    sc.records = lone[:len(lone) // 2] + sc.records + lone[len(lone) // 2:]  # the run's entries lie inside the call's list
    return sc


def dense_claims(sc, rows):
    """What the dense scene must give k_ov_match, from the references alone: more than one workgroup of sites, the last partly
    filled, and in it - the sites are listed + strand first, ascending - a site with rows for a guide of the second LDS chunk"""
    st = sc.sites()
    assert len(st) > 256 and len(st) % 256 != 0
    last = max(p for _c, p, s in st if s == 1)
    assert last == DENSE_N - sc.L and any(g >= 1024 and p == last and s == 1 for g, _c, p, s, _mm, _w, _a in rows)


@functools.lru_cache(maxsize=None)
def pam_lowest_scene():
    """TTTV in front: REF T under the V and two ALTs whose alleles IN GUIDE ORIENTATION are {A, G} resp. {C, G}, on each strand.
    The window reads the lowest of them in guide orientation - A resp. C; taken on the + strand, a - strand site (its records
    state the complements, {T, C} resp. {G, C}) would read G."""
    sc = Scene("TTTV", 23, True, 17, lengths=(900,))
    slot = 40
    for k, (letters, low) in enumerate((("AG", "A"), ("CG", "C"))):
        for strand in (0, 1):
            label = f"{letters}{'+-'[strand]}"
            sc.place(label, "chr1", slot, strand, k, {sc.pm(3): "T"}, {sc.pm(3): letters})
            w = sc.window(k)
            sc.want[label] = (0, w[:3] + low + w[4:], 1 << 3)
            slot += 2 * sc.L + 5
    return sc


@functools.lru_cache(maxsize=None)
def pam_n_scene():
    """NGG: an N in the genome under the PAM's N with a needed spacer ALT beside it - a row at max_mm 0, the N stays in the
    window - and the same site with the N at a spacer base: a mismatch, a row from max_mm 1 on"""
    sc = Scene("NGG", 20, False, 19, lengths=(700,))
    slot = 40
    for strand in (0, 1):
        tag = "+-"[strand]
        g = sc.guides[0]
        sc.place("under_pam_n" + tag, "chr1", slot, strand, 0, {sc.pm(0): "N", sc.sp(19): sc.other(g[19])}, {sc.sp(19): g[19]})
        w = sc.window(0)
        sc.want["under_pam_n" + tag] = (0, w[:20] + "N" + w[21:], 1 << 19)
        g = sc.guides[1]
        sc.place("spacer_n" + tag, "chr1", slot + 60, strand, 1, {sc.sp(12): "N", sc.sp(13): sc.other(g[13])}, {sc.sp(13): g[13]})
        w = sc.window(1)
        sc.want["spacer_n" + tag] = (1, w[:12] + "N" + w[13:], 1 << 13)
        sc.min_mm["spacer_n" + tag] = 1
        slot += 130
    return sc


@functools.lru_cache(maxsize=None)
def shard_scene():
    """standard_scene (NGG / 20, max_mm 2) and a site at chr1:2040 whose needed ALT at 2050 lies in the overlap of the rows that
    start at 1024 and 2048: of three shards over the six rows the first owns the window, the second holds the variant too"""
    sc = standard_scene("NGG", 20, False, 2)
    place_needed(sc, "shard_overlap", "chr1", 2040, 0, 0, (sc.sp(10),))
    return sc


def split_calls(records):
    """the records, multi-allelic ones split per ALT, dealt into three lists; the ALTs of one record land in different lists"""
    calls = [[], [], []]
    for k, (contig, pos, ref, alts) in enumerate(records):
        for j, alt in enumerate(alts.split(",")):
            calls[(k + j) % 3].append((contig, pos, ref, alt))
    return calls
