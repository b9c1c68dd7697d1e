"""K7 off-target scan vs the oracle's brute force (parity UNPINNED to the reference: it delegates
this to the external CRISPRitz binary; see oracle/hawk_oracle.c).  Bit-exact row sets."""
import numpy as np
import pytest

from crisprhawk_hip import synth
from crisprhawk_hip.genome import GenomeIndex
from crisprhawk_hip.pam import PAM
from oracle import oracle as ora

pytestmark = pytest.mark.gpu


def _plant(rng, genome: list, guide: str, pam_seq: str, right: bool, n: int, max_mm: int):
    """write mutated copies of guide+PAM (both strands) into the genome so there is something to find"""
    L = len(guide) + len(pam_seq)
    for _ in range(n):
        g = list(guide)
        for p in rng.integers(0, len(g), size=int(rng.integers(0, max_mm + 2))):
            g[p] = "ACGT"[rng.integers(0, 4)]
        w = (pam_seq + "".join(g)) if right else ("".join(g) + pam_seq)
        if rng.random() < 0.5:
            w = ora.revcomp(w)
        pos = int(rng.integers(0, len(genome) - L))
        genome[pos:pos + L] = list(w)


@pytest.mark.parametrize("n_guides", [6, 200, 2300, -2300])  # 6: all pairs; 200 / 2300: pair seeds (max_mm + 2 blocks, candidates dealt
#   evenly over a wave); -2300: 2300 guides at max_mm = 7, the single-block seeds (pair seeds would need 9 blocks)
@pytest.mark.parametrize("pam_s,guidelen,right,max_mm,piece", [("NGG", 20, False, 4, 1 << 22), ("TTTV", 23, True, 3, 4096),
                                                              ("TTTV", 23, True, 4, 1 << 22),  # C5 as BASELINE.json states it
                                                              ("NNGRRT", 21, False, 2, 10000), ("NGG", 20, False, 0, 1 << 22),
                                                              ("NGG", 17, False, 6, 1 << 22)])
def test_offtarget_scan_matches_bruteforce(pam_s, guidelen, right, max_mm, piece, n_guides):
    if n_guides < 0:
        n_guides, max_mm = -n_guides, 7
    rng = np.random.default_rng(77)
    contigs = {}
    guides = [synth.random_sequence(rng, guidelen) for _ in range(n_guides)]
    # families of near-identical guides: pairs that agree in several seed blocks must still be reported once
    for k in range(6, n_guides, 9):
        g = list(guides[k % 6])
        g[int(rng.integers(0, guidelen))] = "ACGT"[int(rng.integers(0, 4))]
        guides[k] = "".join(g)
    concrete = {"NGG": "TGG", "TTTV": "TTTA", "NNGRRT": "ACGAGT"}[pam_s]
    for name, n in (("c1", 60_000), ("c2", 25_001), ("c3", 300)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
        for gd in guides[:6]:
            _plant(rng, g, gd, concrete, right, 12 if n > 1000 else 1, max_mm)
        if n > 5000:  # an N run: must not produce hits nor blow up
            g[3000:3400] = "N" * 400
        contigs[name] = "".join(g)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, guidelen, len(pam_s), piece=piece)
    got = idx.scan(guides, pam, right, max_mm, cap=64)  # small cap: exercises the capacity retry
    want = []
    for name, seq in contigs.items():
        for r in ora.offtargets(seq, guides, pam_s, right, max_mm):
            want.append((int(r["guide"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"])))
    ci = {n: i for i, n in enumerate(contigs)}
    want.sort(key=lambda t: (t[0], ci[t[1]], t[2], t[3] == "-"))
    assert len(want) > (20 if max_mm else 3)
    assert len(set(want)) == len(want)
    assert [(h.guide, h.contig, h.position, h.strand, h.mm) for h in got] == want
    # the reported window is the genome window in guide orientation
    L = guidelen + len(pam_s)
    for h in got[:200]:
        w = contigs[h.contig][h.position:h.position + L].upper()
        w = ora.revcomp(w) if h.strand == "-" else w
        assert h.window == "".join(c if c in "ACGT" else "N" for c in w)


def test_offtargets_search_pipeline(tmp_path):
    """search() -> offtargets_search(): per-guide counts and global CFD 100/(100+sum) as in the
    reference's annotate_guides_offtargets (offtargets.py:597-627)."""
    from types import SimpleNamespace
    from crisprhawk_hip import scoring
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.haplotype import Haplotype
    from crisprhawk_hip.region import Region
    from crisprhawk_hip.search_guides import search
    from crisprhawk_hip.annotation import reverse_guides
    from crisprhawk_hip.search_offtargets import offtargets_search
    from crisprhawk_hip.sequence import Sequence

    reg = synth.make_region(901, "chrG", 30_000, 10_000, 10_400)
    region = Region(Sequence(reg.sequence, True), Coordinate("chrG", 10_000, 10_400, 100))
    hap = Haplotype(Sequence(reg.sequence, True), region.coordinates, False, 0, True)
    hap.id = "hap_ref"
    pam = PAM("NGG", False, True)
    pam.encode(0)
    guides = reverse_guides(search(pam, region, [hap], None, 20, False, False, False, 0, True), 0)
    assert len(guides) > 10
    mm, pt = synth.cfd_tables()
    scoring.set_cfd_tables(mm, pt)
    args = SimpleNamespace(verbosity=0, debug=True, crispritz_index={"chrG": reg.contig_seq}, mm=3, bdna=0, brna=0,
                           guidelen=20, right=False, outdir=str(tmp_path))
    out = offtargets_search({region: guides}, pam, args)[region]
    for g in out[:25]:
        rows = ora.offtargets(reg.contig_seq, [g.guide.upper()], "NGG", False, 3)
        assert int(g.offtargets) == len(rows) >= 1  # the on-target site itself is always there
        tot = 0.0
        for r in rows:
            w = reg.contig_seq[int(r["pos"]):int(r["pos"]) + 23]
            w = ora.revcomp(w) if r["strand"] else w
            tot += round(ora.cfd(g.guide.upper(), w[:20], w[-2:], mm, pt), 4)
        assert g.cfd == str(round(100 / (100 + tot), 4))
    tsv = (tmp_path / "offtargets_chrG_10000_10400.tsv").read_text().splitlines()
    assert tsv[0].split("\t") == ["chrom", "position", "strand", "grna", "spacer", "pam", "mm", "bulge_size", "bulg_type", "cfd", "elevation"]
    assert len(tsv) - 1 >= len(out)


def _verify_hits_on_host(contig_arrays, idx, hits, guides, pam_s, guidelen, right, max_mm):
    """Every reported hit re-derived from the genome bytes: PAM positions inside the PAM's IUPAC sets, mismatch count
    as reported and <= max_mm, window code as reported."""
    from crisprhawk_hip.genome import decode_window
    from crisprhawk_hip.pam import IUPAC_BITS
    L = guidelen + len(pam_s)
    nib = {"A": 1, "C": 2, "G": 4, "T": 8}
    comp = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    n = len(hits["guide"])
    sel = np.arange(n) if n <= 20000 else np.random.default_rng(0).choice(n, 20000, replace=False)
    for i in sel.tolist():
        name, off, _own = idx.rows[int(hits["row"][i])]
        p0 = off + int(hits["q"][i])
        w = contig_arrays[name][p0:p0 + L]
        if hits["strand"][i]:
            w = comp[w[::-1]]
        w = w.tobytes().decode()
        assert decode_window(int(hits["code"][i]), int(hits["nmask"][i]), L) == w
        sp, pm = (w[len(pam_s):], w[:len(pam_s)]) if right else (w[:guidelen], w[guidelen:])
        assert all(nib[c] & IUPAC_BITS[q] for c, q in zip(pm, pam_s))
        mm = sum(a != b for a, b in zip(sp, guides[int(hits["guide"][i])]))
        assert mm == int(hits["mm"][i]) <= max_mm


C5_CONTIG_NT, C5_GUIDES = 129_166_667, 10_000  # 24 contigs: 3.1 x 10^9 nt


def test_c5_full_size_properties():
    """C5 at BASELINE.json's full size - a 3.1 x 10^9-nt genome in 24 contigs, 10^4 guides, TTTV / 23, <= 4 mismatches - which no
    brute force reaches: the pair-seed
    match kernel must report the hit set of the all-pairs kernel, every guide must find its planted on-target, and every hit must
    re-verify against the genome bytes on the host."""
    import subprocess, sys, os, json
    code = r"""
import json, sys, hashlib
import numpy as np
C5_CONTIG_NT, C5_GUIDES = %d, %d
sys.path[:0] = [%r, %r]
from crisprhawk_hip.genome import GenomeIndex
from crisprhawk_hip.pam import PAM
rng = np.random.default_rng(1006)
acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
contigs = {f"chr{i+1}": acgt[rng.integers(0, 4, size=C5_CONTIG_NT, dtype=np.uint8)] for i in range(24)}
grng = np.random.default_rng(1005)
names = list(contigs)
guides = []
while len(guides) < C5_GUIDES:
    c = contigs[names[int(grng.integers(0, 24))]]
    p = int(grng.integers(0, len(c) - 64))
    guides.append(c[p:p + 23].tobytes().decode())
pam = PAM("TTTV", True, True); pam.encode(0)
idx = GenomeIndex(contigs, 23, 4)
hits, tm = idx.scan_arrays(guides, pam, True, 4)
order = np.lexsort((hits["strand"], hits["q"], hits["row"], hits["guide"]))
h = hashlib.sha256()
for k in ("guide", "row", "q", "strand", "mm", "code", "nmask"):
    h.update(np.ascontiguousarray(hits[k][order]).tobytes())
print("RESULT", json.dumps({"n": int(len(order)), "digest": h.hexdigest(), "n_sites": int(tm["n_sites"]), "match_ms": tm["match_ms"]}))
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = code % (C5_CONTIG_NT, C5_GUIDES, os.path.join(root, "crispr-hawk_amd"), root)
    res = {}
    for label, env in (("pair_seeds", {}), ("all_pairs", {"HAWK_OT_ALLPAIRS": "1"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=1100)
        assert r.returncode == 0, r.stderr[-2000:]
        res[label] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0][7:])
    assert res["pair_seeds"]["digest"] == res["all_pairs"]["digest"]
    print("match_ms", {k: round(v["match_ms"], 2) for k, v in res.items()})
    assert res["pair_seeds"]["n"] >= 100  # ~1 guide in 85 sits behind a TTTV and is its own on-target; the rest are chance near-matches
    # in-process: host re-verification of the default kernel's hits
    rng = np.random.default_rng(1006)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = {f"chr{i+1}": acgt[rng.integers(0, 4, size=C5_CONTIG_NT, dtype=np.uint8)] for i in range(24)}
    grng = np.random.default_rng(1005)
    names = list(contigs)
    guides, origin = [], []
    while len(guides) < C5_GUIDES:
        ci = int(grng.integers(0, 24))
        c = contigs[names[ci]]
        p = int(grng.integers(0, len(c) - 64))
        guides.append(c[p:p + 23].tobytes().decode())
        origin.append((names[ci], p))
    pam = PAM("TTTV", True, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, 23, 4)
    hits, _tm = idx.scan_arrays(guides, pam, True, 4)
    assert len(hits["guide"]) == res["pair_seeds"]["n"]
    _verify_hits_on_host(contigs, idx, hits, guides, "TTTV", 23, True, 4)
    # a guide cut out right behind a TTTV is its own 0-mismatch on-target at PAM start = origin - 4
    found = {(int(g), idx.rows[int(r)][0], idx.rows[int(r)][1] + int(q)) for g, r, q, s, m in
             zip(hits["guide"], hits["row"], hits["q"], hits["strand"], hits["mm"]) if m == 0 and s == 0}
    planted = 0
    for gi, (name, p) in enumerate(origin):
        if p >= 4:
            pm = contigs[name][p - 4:p].tobytes().decode()
            if pm[:3] == "TTT" and pm[3] in "ACG":
                planted += 1
                assert (gi, name, p - 4) in found
    assert planted >= 10


def test_sharded_genome_index_partitions_the_hits():
    """SURVEY §8(e) for C5: the genome's rows block-partitioned over ranks, guides replicated; the union of the
    shards' hits (global row numbers) is the unsharded scan's hit set."""
    rng = np.random.default_rng(78)
    contigs = {f"c{i}": synth.random_sequence(rng, 90_000 + 7000 * i) for i in range(5)}
    guides = [contigs["c1"][p:p + 20] for p in range(100, 70_000, 700)]
    pam = PAM("NGG", False, True)
    pam.encode(0)
    whole, _ = GenomeIndex(contigs, 20, 3, piece=20_000).scan_arrays(guides, pam, False, 3)
    parts = []
    for r in range(3):
        idx = GenomeIndex(contigs, 20, 3, piece=20_000, shard=(r, 3))
        assert (idx.row_hi - idx.row_lo) in (idx.n_rows_total // 3, idx.n_rows_total // 3 + 1)
        parts.append(idx.scan_arrays(guides, pam, False, 3)[0])
    key = lambda h: sorted(zip(h["guide"].tolist(), h["row"].tolist(), h["q"].tolist(), h["strand"].tolist(), h["mm"].tolist()))
    merged = {k: np.concatenate([p[k] for p in parts]) for k in whole}
    assert key(merged) == key(whole) and len(whole["guide"]) >= 5  # ~1 spacer in 16 is followed by NGG and is its own on-target


@pytest.mark.parametrize("pam_s,guidelen,right,max_mm", [("NGG", 20, False, 2), ("TTTV", 23, True, 1)])
@pytest.mark.parametrize("bdna,brna", [(1, 0), (0, 1), (1, 1), (2, 2)])
def test_bulged_offtargets_match_bruteforce(pam_s, guidelen, right, max_mm, bdna, brna):
    """-bDNA / -bRNA (offtargets.py:264-268): sites that pair with a guide once up to 2 bases are bulged out of the DNA or of the
    RNA.  The device path searches them as mismatch-only scans of derived guides (GenomeIndex.scan_bulges) and must report the
    rows of the oracle's brute force over every placement (ora.offtargets_bulges; both sides unpinned to CRISPRitz, which is
    absent): one row per (guide, site, type, size), fewest mismatches, ties to the smallest bulge positions."""
    rng = np.random.default_rng(99 + bdna * 7 + brna)
    n_guides = 5
    guides = [synth.random_sequence(rng, guidelen) for _ in range(n_guides)]
    guides[1] = guides[1][:6] + "AAAA" + guides[1][10:]  # a run of equal bases: several placements spell the same derived guide
    concrete = {"NGG": "TGG", "TTTV": "TTTA"}[pam_s]
    contigs = {}
    for name, n in (("c1", 30_000), ("c2", 9_001)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.0005))
        for gd in guides:
            for _ in range(10):  # planted sites: the guide with mismatches, bases inserted (DNA bulge) or deleted (RNA bulge)
                sp = list(gd)
                for p in rng.integers(0, guidelen, size=int(rng.integers(0, max_mm + 1))):
                    sp[p] = "ACGT"[rng.integers(0, 4)]
                kind = int(rng.integers(0, 3))
                k = int(rng.integers(1, 3))
                if kind == 1:
                    for _ in range(k):
                        sp.insert(int(rng.integers(1, len(sp) - 1)), "ACGT"[rng.integers(0, 4)])
                elif kind == 2:
                    for _ in range(k):
                        del sp[int(rng.integers(1, len(sp) - 1))]
                w = (concrete + "".join(sp)) if right else ("".join(sp) + concrete)
                if rng.random() < 0.5:
                    w = ora.revcomp(w)
                pos = int(rng.integers(0, n - len(w)))
                g[pos:pos + len(w)] = list(w)
        contigs[name] = "".join(g)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, guidelen, len(pam_s), piece=4096, max_bulge=bdna)
    got = idx.scan_bulges(guides, pam, right, max_mm, bdna, brna)
    want = []
    for name, seq in contigs.items():
        for r in ora.offtargets_bulges(seq, guides, pam_s, right, max_mm, bdna, brna):
            want.append((int(r["guide"]), "DNA" if r["btype"] == 1 else "RNA", int(r["bsize"]), name, int(r["pos"]), "-" if r["strand"] else "+",
                         int(r["mm"]), int(r["gaps"])))
    ci = {n: i for i, n in enumerate(contigs)}
    want.sort(key=lambda t: (t[0], t[1], t[2], ci[t[3]], t[4], t[5] == "-"))
    assert len(want) > 30 and {t[1] for t in want} == ({"DNA"} if not brna else {"RNA"} if not bdna else {"DNA", "RNA"})
    assert [(h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps) for h in got] == want
    # the strings of a row: the guide and the site re-derived from the genome, '-' at the bulges, mismatches in lower case
    _verify_bulge_rows_on_host(contigs, got[:300], guides, pam_s, guidelen, right, max_mm)
    # un-bulged scans before and after see the same rows: the window metadata is put back
    assert [(x.guide, x.contig, x.position, x.strand, x.mm) for x in idx.scan(guides, pam, right, max_mm)] == \
        sorted(((int(r["guide"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"])) for name, seq in contigs.items()
                for r in ora.offtargets(seq, guides, pam_s, right, max_mm)), key=lambda t: (t[0], ci[t[1]], t[2], t[3] == "-"))


def _verify_bulge_rows_on_host(contigs, rows, guides, pam_s, guidelen, right, max_mm):
    """Every BulgeHit re-derived from the genome bytes: the crRNA is the guide and the DNA is the site's spacer, with '-' at the
    bulges (as the gaps bitmask says) and mismatches in lower case; the mismatch count as reported and <= max_mm; the site's PAM
    inside the PAM's IUPAC sets."""
    from crisprhawk_hip.pam import IUPAC_BITS
    nib = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 0}
    P = len(pam_s)
    for h in rows:
        Gs = guidelen + h.bulge_size if h.bulge_type == "DNA" else guidelen - h.bulge_size
        w = contigs[h.contig][h.position:h.position + Gs + P].upper()
        assert len(w) == Gs + P
        w = ora.revcomp(w) if h.strand == "-" else w
        w = "".join(c if c in "ACGT" else "N" for c in w)
        site, pm = (w[P:], w[:P]) if right else (w[:Gs], w[Gs:])
        assert h.pam == pm and all(IUPAC_BITS[q] == 15 or nib[c] & IUPAC_BITS[q] for c, q in zip(pm, pam_s))
        assert h.crrna.replace("-", "") == guides[h.guide] and h.dna.replace("-", "").upper() == site
        assert len(h.crrna) == len(h.dna) and h.crrna.count("-") == (h.bulge_size if h.bulge_type == "DNA" else 0)
        assert h.dna.count("-") == (h.bulge_size if h.bulge_type == "RNA" else 0)
        dashes = [i for i, (a, b) in enumerate(zip(h.crrna, h.dna)) if a == "-" or b == "-"]
        assert h.gaps == sum(1 << i for i in dashes)  # DNA: site positions, RNA: guide positions (one column per base of each)
        assert 0 not in dashes and len(h.crrna) - 1 not in dashes  # interior bulges only
        assert sum(1 for a, b in zip(h.crrna, h.dna) if b.islower()) == h.mm <= max_mm
        assert all(b.upper() != a or b.upper() == "N" for a, b in zip(h.crrna, h.dna) if b.islower())
        assert all(b == a for a, b in zip(h.crrna, h.dna) if a != "-" and b != "-" and not b.islower())


def test_offtarget_stage_with_bulges_writes_their_rows(tmp_path):
    """estimate_offtargets_spacers with bdna / brna > 0: the off-targets TSV holds DNA / RNA rows next to the X rows, every row
    in the field set the reference's consumer reads (offtarget.py:77-101), counts per spacer include them."""
    from crisprhawk_hip import scoring
    from crisprhawk_hip.coordinate import Coordinate
    from crisprhawk_hip.offtargets import estimate_offtargets_spacers
    rng = np.random.default_rng(5)
    guide = synth.random_sequence(rng, 20)
    g = list(synth.random_sequence(rng, 20_000))
    sites = {"X": guide + "TGG", "DNA": guide[:9] + "C" + guide[9:] + "AGG", "RNA": guide[:12] + guide[13:] + "CGG"}
    for k, (kind, w) in enumerate(sites.items()):
        g[2000 * (k + 1):2000 * (k + 1) + len(w)] = list(w)
    pam = PAM("NGG", False, True)
    pam.encode(0)
    scoring.set_cfd_tables(*synth.cfd_tables())
    out = estimate_offtargets_spacers([guide], pam, {"chrT": "".join(g)}, Coordinate("chrT", 100, 900, 100), 1, 1, 1, 20, False, str(tmp_path), 0, True)
    (tsv,) = list(tmp_path.glob("offtargets_chrT_*.tsv"))
    rows = [ln.split("\t") for ln in tsv.read_text().splitlines()[1:]]
    kinds = {r[8] for r in rows}
    assert kinds == {"X", "DNA", "RNA"}
    assert out[guide][0] == len(rows) >= 3
    for r in rows:
        if r[8] == "DNA":
            assert "-" in r[3] and int(r[7]) == 1
        if r[8] == "RNA":
            assert "-" in r[4] and int(r[7]) == 1


# ---- the row geometry at its edges, every match kernel, against the brute force -------------------------------------------------
_CONCRETE = {"NGG": "TGG", "TTTV": "TTTA"}
_KINDS = (("X", 0), ("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))


def _mutate(rng, guide: str, kind: str, b: int, n_mm: int, ins: str = "") -> str:
    """the site spacer of a planted site: the guide with n_mm substitutions, then b interior bases inserted (DNA bulge; `ins`
    names them, else random) or deleted (RNA bulge)"""
    sp = list(guide)
    for p in rng.choice(len(sp), n_mm, replace=False).tolist():
        sp[p] = "ACGT"["ACGT".index(sp[p]) ^ int(rng.integers(1, 4))]
    for k in range(b):
        if kind == "DNA":
            sp.insert(int(rng.integers(1, len(sp))), ins[k] if ins else "ACGT"[int(rng.integers(0, 4))])
        elif kind == "RNA":
            del sp[int(rng.integers(1, len(sp) - 1))]
    return "".join(sp)


def _place(g: list, start: int, spacer: str, pam: str, right: bool, minus: bool):
    w = (pam + spacer) if right else (spacer + pam)
    w = ora.revcomp(w) if minus else w
    g[start:start + len(w)] = list(w)
    return len(w)


def _edge_genome(pam_s: str, G: int, right: bool, piece: int, seed: int = 4242):
    """Contigs at the edges of the row geometry - lengths L-2, L-1, L, piece+L-2, piece+L-1, k*piece, k*piece+1 - with sites of
    every kind (mismatch-only, DNA / RNA bulges of 1 and 2) planted at start 0, at the contig's last start n - Lw, and at every
    start from seam - Lw through the seam of many row seams (one per seam), on both strands; N / IUPAC bases as first and last
    bases, in a PAM and as a DNA-bulged base.  Returns (contigs, guides: 70 guides in seed-sharing families, planted: the sites
    as (guide, contig, start, strand, kind, bulge))."""
    rng = np.random.default_rng(seed + piece + G)
    P, pam = len(pam_s), _CONCRETE[pam_s]
    L = G + P
    guides = [synth.random_sequence(rng, G) for _ in range(70)]
    for k in range(6, 70, 5):  # families: pairs that share seed blocks
        g = list(guides[k % 6])
        g[int(rng.integers(0, G))] = "ACGT"[int(rng.integers(0, 4))]
        guides[k] = "".join(g)
    contigs, planted = {}, []

    def plant(g, name, start, gi, kind, b, minus, n_mm=None, ins=""):
        sp = _mutate(rng, guides[gi], kind, b, int(rng.integers(0, 3)) if n_mm is None else n_mm, ins)
        _place(g, start, sp, pam, right, minus)
        planted.append((gi, name, start, "-" if minus else "+", kind, b))

    # whole contigs that are one window each: L-2 (an RNA bulge of 2), L-1 (of 1), L (mismatch-only)
    for n, (kind, b) in ((L - 2, ("RNA", 2)), (L - 1, ("RNA", 1)), (L, ("X", 0))):
        for minus in (False, True):
            g = list(synth.random_sequence(rng, n))
            plant(g, f"w{n}{'m' if minus else 'p'}", 0, 0, kind, b, minus, n_mm=0)
            contigs[f"w{n}{'m' if minus else 'p'}"] = "".join(g)
    # contigs that end at or just past a seam: sites at start 0 and at the last start
    for ci, n in enumerate((piece + L - 2, piece + L - 1, piece, piece + 1, 2 * piece, 2 * piece + 1, 3 * piece + L - 1)):
        for minus in (False, True):
            name = f"e{n}{'m' if minus else 'p'}"
            g = list(synth.random_sequence(rng, n))
            for ki, where in ((ci % 5, 0), ((ci + 2) % 5, None)):  # one kind at start 0, another at its last start
                kind, b = _KINDS[ki]
                Lw = L + (b if kind == "DNA" else -b)
                plant(g, name, n - Lw if where is None else 0, (ki + 1) % 6, kind, b, minus)
            contigs[name] = "".join(g)
    # seams: every kind at every start seam - Lw .. seam, strands alternating, one site per seam of 16-piece contigs
    todo = [(kind, b, d, (d + ki) % 2 == 1) for ki, (kind, b) in enumerate(_KINDS) for d in range(0, L + (b if kind == "DNA" else -b) + 1)]
    per = 15
    for c0 in range(0, len(todo), per):
        name = f"s{c0 // per}"
        g = list(synth.random_sequence(rng, 16 * piece + L - 1))
        for j, (kind, b, d, minus) in enumerate(todo[c0:c0 + per]):
            plant(g, name, (j + 1) * piece - d, j % 4, kind, b, minus)
        contigs[name] = "".join(g)
    # N / IUPAC: first and last bases, a PAM base, a DNA-bulged base
    name = "amb"
    g = list(synth.random_sequence(rng, 3 * piece))
    plant(g, name, 0, 1, "X", 0, False, n_mm=0)
    plant(g, name, len(g) - L, 2, "X", 0, True, n_mm=0)
    g[0], g[-1] = "N", "R"
    ppos = 0 if right else G  # the PAM's first base (+ strand)
    plant(g, name, piece - 7, 3, "X", 0, False, n_mm=0)
    g[piece - 7 + ppos + P - 1] = "N"
    plant(g, name, 2 * piece - 9, 4, "X", 0, False, n_mm=0)
    g[2 * piece - 9 + ppos + P - 1] = "S"
    plant(g, name, piece + 100, 0, "DNA", 1, False, n_mm=0, ins="N")
    plant(g, name, piece + 300, 1, "DNA", 2, True, n_mm=0, ins="YA")
    contigs[name] = "".join(g)
    return contigs, guides, planted


_EDGE_CACHE = {}


def _edge_case(pam_s: str, G: int, right: bool, piece: int, max_mm: int = 2):
    """(contigs, guides, planted, want mismatch-only rows, want bulge rows) of an edge genome - the brute force once per case"""
    key = (pam_s, G, right, piece, max_mm)
    if key not in _EDGE_CACHE:
        contigs, guides, planted = _edge_genome(pam_s, G, right, piece)
        ci = {n: i for i, n in enumerate(contigs)}
        want_mm, want_b = [], []
        for name, seq in contigs.items():
            want_mm += [(int(r["guide"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"]))
                        for r in ora.offtargets(seq, guides, pam_s, right, max_mm)]
            want_b += [(int(r["guide"]), "DNA" if r["btype"] == 1 else "RNA", int(r["bsize"]), name, int(r["pos"]), "-" if r["strand"] else "+",
                        int(r["mm"]), int(r["gaps"])) for r in ora.offtargets_bulges(seq, guides[:6], pam_s, right, max_mm, 2, 2)]
        want_mm.sort(key=lambda t: (t[0], ci[t[1]], t[2], t[3] == "-"))
        want_b.sort(key=lambda t: (t[0], t[1], t[2], ci[t[3]], t[4], t[5] == "-"))
        _EDGE_CACHE[key] = (contigs, guides, planted, want_mm, want_b)
    return _EDGE_CACHE[key]


def _edge_scan(pam_s: str, G: int, right: bool, piece: int, max_mm: int = 2, max_derived: int = 1 << 20):
    """the device's rows of an edge genome: mismatch-only for all 70 guides, DNA / RNA bulges of up to 2 for the first 6"""
    contigs, guides, _planted = _edge_genome(pam_s, G, right, piece)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, G, len(pam_s), piece=piece, max_bulge=2)
    got_mm = [(h.guide, h.contig, h.position, h.strand, h.mm) for h in idx.scan(guides, pam, right, max_mm)]
    got_b = [(h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps)
             for h in idx.scan_bulges(guides[:6], pam, right, max_mm, 2, 2, max_derived=max_derived)]
    return got_mm, got_b


@pytest.mark.parametrize("kernel", ["pair_seeds", "single_block", "all_pairs"])
@pytest.mark.parametrize("pam_s,G,right,piece", [("NGG", 20, False, 512), ("TTTV", 23, True, 1000)])
def test_offtarget_edges_match_bruteforce(pam_s, G, right, piece, kernel, monkeypatch):
    """Sites at the edges of the row geometry (a contig's first and last window start, every start around a row seam, contigs
    no longer than one window, N / IUPAC bases at the ends, in a PAM and in a bulge), mismatch-only and with DNA / RNA bulges of
    1 and 2, on both strands, through each of the three match kernels (single-block seeds: max_mm = 7): exactly the brute force's
    rows."""
    max_mm = 7 if kernel == "single_block" else 2
    if kernel == "all_pairs":
        monkeypatch.setenv("HAWK_OT_ALLPAIRS", "1")
    contigs, guides, planted, want_mm, want_b = _edge_case(pam_s, G, right, piece, max_mm)
    got_mm, got_b = _edge_scan(pam_s, G, right, piece, max_mm)
    # the brute force sees what was planted (the ambiguous-base plants excepted): the sweep reaches every edge it claims to
    sites_mm = {(t[0], t[1], t[2], t[3]) for t in want_mm}
    sites_b = {(t[0], t[1], t[2], t[3], t[4], t[5]) for t in want_b}
    for gi, name, start, strand, kind, b in planted:
        if name == "amb":
            continue
        assert ((gi, name, start, strand) in sites_mm) if kind == "X" else ((gi, kind, b, name, start, strand) in sites_b), (gi, name, start, kind, b)
    assert got_mm == want_mm
    assert got_b == want_b


def test_bulged_site_in_a_contig_tail_is_reported():
    """Regression: an RNA-bulged site whose window starts at `piece` of a contig of piece + L - 1 bases, and one that is a whole
    contig of L - 1 bases, lie in no row of full windows; both must be reported."""
    rng = np.random.default_rng(31)
    G, P, piece = 20, 3, 4096
    L = G + P
    guide = synth.random_sequence(rng, G)
    site = guide[:9] + guide[10:]  # an RNA bulge of 1 at guide position 9
    tail = synth.random_sequence(rng, piece + L - 1 - (L - 1)) + site + "AGG"
    short = site + "TGG"
    contigs = {"tail": tail, "short": short}
    pam = PAM("NGG", False, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, G, P, piece=piece)
    got = [(h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps) for h in idx.scan_bulges([guide], pam, False, 0, 0, 2)]
    assert {(t[3], t[4]) for t in got if t[1:3] == ("RNA", 1) and t[5:7] == ("+", 0)} >= {("tail", piece), ("short", 0)}
    want = sorted(((0, "RNA", int(r["bsize"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"]), int(r["gaps"]))
                   for name, seq in contigs.items() for r in ora.offtargets_bulges(seq, [guide], "NGG", False, 0, 0, 2)),
                  key=lambda t: (t[0], t[1], t[2], ["tail", "short"].index(t[3]), t[4], t[5] == "-"))
    assert got == want


@pytest.mark.parametrize("n_guides", [63, 64, 1024, 1025])
@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("pam_s,G,right,max_mm", [("NGG", 20, False, 3), ("TTTV", 23, True, 4)])
def test_offtarget_guide_count_boundaries(pam_s, G, right, max_mm, n_guides, pairs):
    """Mismatch-only scans at the guide count where the match kernel changes, 63 / 64 (all pairs below 64 guides, seeds from 64),
    and at 1024 / 1025, with pair seeds and with single-block seeds (max_mm = 7), guides in families that share seed blocks:
    exactly the brute force's rows."""
    if not pairs:
        max_mm = 7
    rng = np.random.default_rng(n_guides + G)
    guides = [synth.random_sequence(rng, G) for _ in range(n_guides)]
    for k in range(6, n_guides, 7):
        g = list(guides[k % 6])
        for p in rng.choice(G, int(rng.integers(1, max_mm + 2)), replace=False).tolist():
            g[p] = "ACGT"[int(rng.integers(0, 4))]
        guides[k] = "".join(g)
    contigs = {}
    for name, n in (("c1", 20_000), ("c2", 4096 + G + len(pam_s) - 1)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
        for gd in guides[:6] + guides[-3:]:
            _plant(rng, g, gd, _CONCRETE[pam_s], right, 4, max_mm)
        contigs[name] = "".join(g)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    got = GenomeIndex(contigs, G, len(pam_s), piece=4096).scan(guides, pam, right, max_mm)
    ci = {n: i for i, n in enumerate(contigs)}
    want = sorted(((int(r["guide"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"])) for name, seq in contigs.items()
                   for r in ora.offtargets(seq, guides, pam_s, right, max_mm)), key=lambda t: (t[0], ci[t[1]], t[2], t[3] == "-"))
    assert len(want) > 40 and any(t[0] == n_guides - 1 for t in want)  # the last guide has rows
    assert [(h.guide, h.contig, h.position, h.strand, h.mm) for h in got] == want


@pytest.mark.parametrize("pam_s,G,right,bdna,brna", [("NGG", 29, False, 0, 0), ("TTTV", 28, True, 0, 0), ("NGG", 27, False, 2, 2)])
def test_offtarget_32_base_windows(pam_s, G, right, bdna, brna):
    """Windows at the 32-base limit of the window code (29 + NGG, 28 + TTTV; 27 + NGG with a DNA bulge of 2): exactly the brute
    force's rows.  One base more is refused before any device work."""
    rng = np.random.default_rng(G + bdna)
    max_mm = 3 if not bdna else 2
    guides = [synth.random_sequence(rng, G) for _ in range(70 if not bdna else 3)]
    contigs = {}
    for name, n in (("c1", 12_000), ("c2", 1024 + G + len(pam_s) + bdna - 1)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
        for gi in range(3):
            for _ in range(6):
                kind, b = _KINDS[int(rng.integers(0, 5 if bdna else 1))]
                sp = _mutate(rng, guides[gi], kind, b, int(rng.integers(0, max_mm + 1)))
                _place(g, int(rng.integers(0, n - len(sp) - len(pam_s))), sp, _CONCRETE[pam_s], right, bool(rng.random() < 0.5))
        contigs[name] = "".join(g)
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, G, len(pam_s), piece=1024, max_bulge=bdna)
    ci = {n: i for i, n in enumerate(contigs)}
    got = [(h.guide, h.contig, h.position, h.strand, h.mm) for h in idx.scan(guides, pam, right, max_mm)]
    want = sorted(((int(r["guide"]), name, int(r["pos"]), "-" if r["strand"] else "+", int(r["mm"])) for name, seq in contigs.items()
                   for r in ora.offtargets(seq, guides, pam_s, right, max_mm)), key=lambda t: (t[0], ci[t[1]], t[2], t[3] == "-"))
    assert len(want) >= 3 and got == want
    assert all(len(h.window) == G + len(pam_s) for h in idx.scan(guides[:3], pam, right, max_mm))
    if bdna or brna:
        rows = idx.scan_bulges(guides, pam, right, max_mm, bdna, brna)
        got_b = [(h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps) for h in rows]
        want_b = sorted(((int(r["guide"]), "DNA" if r["btype"] == 1 else "RNA", int(r["bsize"]), name, int(r["pos"]), "-" if r["strand"] else "+",
                          int(r["mm"]), int(r["gaps"])) for name, seq in contigs.items()
                         for r in ora.offtargets_bulges(seq, guides, pam_s, right, max_mm, bdna, brna)),
                        key=lambda t: (t[0], t[1], t[2], ci[t[3]], t[4], t[5] == "-"))
        assert ("DNA", 2) in {(t[1], t[2]) for t in want_b} and got_b == want_b
        _verify_bulge_rows_on_host(contigs, rows, guides, pam_s, G, right, max_mm)
    with pytest.raises(ValueError, match="32 bases"):
        GenomeIndex(contigs, G + 1, len(pam_s), max_bulge=bdna)


def test_bulged_offtargets_at_scale():
    """1 500 guides with DNA and RNA bulges of up to 2 on 120 kb (4.6 million derived guides for the DNA bulges of 2): the rows of
    a random sample of guides equal the brute force's on those guides alone (rows never depend on other guides); the whole row
    list is the same with the derived guides scanned 4 096 at a time and at the default cap; every row re-derives on the host."""
    import random
    rng = np.random.default_rng(2024)
    G, P, max_mm = 20, 3, 2
    guides = [synth.random_sequence(rng, G) for _ in range(1500)]
    contigs = {}
    for name, n in (("c1", 70_000), ("c2", 50_000 + G + P - 1)):
        g = list(synth.random_sequence(rng, n, iupac_frac=0.0005))
        for gi in rng.choice(len(guides), 150, replace=False).tolist():
            kind, b = _KINDS[int(rng.integers(0, 5))]
            sp = _mutate(rng, guides[gi], kind, b, int(rng.integers(0, max_mm + 1)))
            _place(g, int(rng.integers(0, n - len(sp) - P)), sp, "AGG", False, bool(rng.random() < 0.5))
        contigs[name] = "".join(g)
    pam = PAM("NGG", False, True)
    pam.encode(0)
    idx = GenomeIndex(contigs, G, P, piece=1 << 15, max_bulge=2)
    key = lambda h: (h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps, h.crrna, h.dna, h.pam)
    full = [key(h) for h in idx.scan_bulges(guides, pam, False, max_mm, 2, 2)]
    small = idx.scan_bulges(guides, pam, False, max_mm, 2, 2, max_derived=4096)
    assert [key(h) for h in small] == full
    assert len(full) > 300 and {(t[1], t[2]) for t in full} == {("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2)}
    _verify_bulge_rows_on_host(contigs, small, guides, "NGG", G, False, max_mm)
    # a sample of guides (some with planted sites, some without) against the brute force on those guides alone
    with_rows = sorted({t[0] for t in full})
    sample = sorted(random.Random(7).sample(with_rows, 12) + random.Random(8).sample(range(len(guides)), 8))
    sample = list(dict.fromkeys(sample))
    ci = {n: i for i, n in enumerate(contigs)}
    want = sorted(((sample[int(r["guide"])], "DNA" if r["btype"] == 1 else "RNA", int(r["bsize"]), name, int(r["pos"]),
                    "-" if r["strand"] else "+", int(r["mm"]), int(r["gaps"])) for name, seq in contigs.items()
                   for r in ora.offtargets_bulges(seq, [guides[i] for i in sample], "NGG", False, max_mm, 2, 2)),
                  key=lambda t: (t[0], t[1], t[2], ci[t[3]], t[4], t[5] == "-"))
    chosen = set(sample)
    assert [t[:8] for t in full if t[0] in chosen] == want and len(want) >= 12


# ---- hawk_offtarget_scan at its capacity seam, once per match kernel ------------------------------------------------------------
def _raw_scan(idx, guides, pam, right, max_mm, cap, columns=True):
    """hawk_offtarget_scan as the ABI has it: (status, *n_out, the rows written as sorted tuples); `columns` false: every optional
    output column is null"""
    import ctypes as C

    from crisprhawk_hip import _lib
    from crisprhawk_hip.genome import encode_guides
    from crisprhawk_hip.hapset import _p
    g2 = encode_guides(guides)
    par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), idx.guidelen, int(bool(right)), max_mm)
    o = {k: np.zeros(max(cap, 1), t) for k, t in GenomeIndex.OT_COLUMNS[:7]}  # guide row q strand mm code nmask
    n = C.c_uint64(0)
    rc = idx.ds._L.hawk_offtarget_scan(idx.ds._h, C.byref(par), _p(g2), len(g2), *[_p(a) if columns else None for a in o.values()],
                                       C.c_uint64(cap), C.byref(n), None)
    k = min(int(n.value), cap) if rc == _lib.HAWK_OK else 0
    return rc, int(n.value), sorted(zip(*[a[:k].tolist() for a in o.values()]))


_CAP_CACHE = {}


def _cap_case():
    """5 001 random bases in two contigs cut into rows of 2 048, near-copies of the first guides planted; 64 guides of 20 bases"""
    if not _CAP_CACHE:
        rng = np.random.default_rng(5309)
        guides = [synth.random_sequence(rng, 20) for _ in range(64)]
        contigs = {}
        for name, n in (("c1", 3500), ("c2", 1501)):
            g = list(synth.random_sequence(rng, n, iupac_frac=0.001))
            for gd in guides[:4]:
                _plant(rng, g, gd, "TGG", False, 3, 3)
            contigs[name] = "".join(g)
        _CAP_CACHE["case"] = (guides, contigs, GenomeIndex(contigs, 20, 3, piece=2048))
    return _CAP_CACHE["case"]


@pytest.mark.parametrize("kernel,n_guides,max_mm", [("all_pairs", 8, 3), ("pair_seeds", 64, 3), ("single_block", 64, 7)])
def test_scan_capacity_contract(kernel, n_guides, max_mm, monkeypatch):
    """hawk_offtarget_scan raw, one call per match kernel (8 guides: all pairs; 64 guides at max_mm 3: pair seeds; at max_mm 7 the
    max_mm + 2 blocks of pair seeds exceed OT_MAX_BLOCKS: single-block seeds).  The rows of a run with ample room are the
    oracle's; cap one below the need and cap = 0: HAWK_E_CAPACITY with the exact need; cap = need: the same rows; every optional
    column null: OK with the same count."""
    from crisprhawk_hip import _lib
    from crisprhawk_hip.genome import decode_window
    monkeypatch.delenv("HAWK_OT_ALLPAIRS", raising=False)
    guides, contigs, idx = _cap_case()
    guides = guides[:n_guides]
    pam = PAM("NGG", False, True)
    pam.encode(0)
    want = sorted((int(r["guide"]), name, int(r["pos"]), int(r["strand"]), int(r["mm"]))
                  for name, seq in contigs.items() for r in ora.offtargets(seq, guides, "NGG", False, max_mm))
    need = len(want)
    assert need >= 2 and len(set(want)) == need
    rc, n, ample = _raw_scan(idx, guides, pam, False, max_mm, 4096)
    assert rc == _lib.HAWK_OK and n == need == len(ample)
    assert sorted((g, idx.rows[row][0], idx.rows[row][1] + q, strand, mm) for g, row, q, strand, mm, _code, _nmask in ample) == want
    for g, row, q, strand, _mm, code, nmask in ample:  # the window as the genome has it, in guide orientation
        name, off, _own = idx.rows[row]
        w = contigs[name][off + q:off + q + 23].upper()
        w = ora.revcomp(w) if strand else w
        assert decode_window(code, nmask, 23) == "".join(c if c in "ACGT" else "N" for c in w)
    for cap in (need - 1, 0):
        rc, n, none = _raw_scan(idx, guides, pam, False, max_mm, cap)
        assert (rc, n, none) == (_lib.HAWK_E_CAPACITY, need, [])
    rc, n, rows = _raw_scan(idx, guides, pam, False, max_mm, need)
    assert rc == _lib.HAWK_OK and n == need and set(rows) == set(ample) and len(rows) == need
    rc, n, _rows = _raw_scan(idx, guides, pam, False, max_mm, need, columns=False)
    assert rc == _lib.HAWK_OK and n == need
