"""References and scenes for the off-target scan over a variant-enriched genome (hawk_offtarget_variant_scan and its host twin).

`brute` applies the semantics of include/hawk.h literally, in plain Python over strings: per position a REF letter and a set of
letters, every window of every contig cut out letter by letter, turned into guide orientation and resolved against every
guide.  It knows no rows, no masks and no 2-bit codes.  `Scene` places its cases by construction - each site is written into a
random contig at a chosen position and strand, with REF edits and ALT alleles given at window positions in guide orientation -
and records what it placed, so that a test can first hold the brute force to the scene (the case is really there) and then the
library to the brute force."""
import random

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


def rows_as_tuples(h, rows, L):
    """the columns of variant_arrays / host_variant_scan as brute's tuples; `rows` = [(contig, offset, ...)] of the index"""
    out = []
    for i in range(len(h["guide"])):
        name, off = rows[int(h["row"][i])][0], rows[int(h["row"][i])][1]
        code, nm = int(h["code"][i]), int(h["nmask"][i])
        win = "".join("N" if (nm >> k) & 1 else "ACGT"[(code >> (2 * k)) & 3] for k in range(L))
        out.append((int(h["guide"][i]), name, off + int(h["q"][i]), int(h["strand"][i]), int(h["mm"][i]), win, int(h["alt"][i])))
    return sorted(out)


def raw_tuples(h):
    return sorted(zip(*(h[k].tolist() for k in ("guide", "row", "q", "strand", "mm", "code", "nmask", "alt"))))


class Scene:
    """Contigs of random bases with sites written into them.  place(): the window `guide + PAM` (PAM in front when `right`) in
    guide orientation, with `edits` {window position: REF letter} applied, lands at `pos` on `strand`; `alts` {window position:
    letters} become records (contig, genome position, REF, ALT) on the + strand."""

    def __init__(self, pam_text, G, right, seed, lengths=(3000, 2500), n_guides=8):
        self.rng = random.Random(seed)
        self.pam_text, self.G, self.right = pam_text, G, right
        self.P = len(pam_text)
        self.L = G + self.P
        self.pam_site = "".join(IUPAC[c][-1] if c != "N" else "T" for c in pam_text)  # NGG -> TGG, TTTV -> TTTG
        self.contigs = {f"chr{k + 1}": [self.rng.choice("ACGT") for _ in range(n)] for k, n in enumerate(lengths)}
        self.guides = ["".join(self.rng.choice("ACGT") for _ in range(G)) for _ in range(n_guides)]
        self.records = []
        self.placed = {}  # label -> (guide, contig, pos, strand)

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
