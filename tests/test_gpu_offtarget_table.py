"""The off-targets table written on the device (hawk_offtarget_text: k_ot_text_len, the 64-bit scan, k_ot_text_fill;
GenomeIndex.offtarget_arrays / rows_text; offtargets.estimate_offtargets_spacers(engine="device")) against the package's host
chain (tests/ottable_refs.py) with `==` on blob, offsets and CFD units, and against the `objects` engine on whole files."""
import itertools
import os

import numpy as np
import pytest

import ottable_refs as R
from crisprhawk_hip import _lib, scoring, synth
from crisprhawk_hip.coordinate import Coordinate
from crisprhawk_hip.crisprhawk_error import CrisprHawkCfdScoreError
from crisprhawk_hip.genome import GenomeIndex
from crisprhawk_hip.offtargets import OTREPCNAMES, estimate_offtargets_spacers
from crisprhawk_hip.pam import PAM
from oracle import oracle as ora
from util import load_golden

pytestmark = pytest.mark.gpu

OTT_SLOT = 8192  # csrc/hawk_ottext.hip: bytes of LDS a wave stages its 64 rows in; a longer range goes straight to global memory
GUIDE = "ACGTTGCAAGCTTAGGCTCA"


def _check(cols, guides, G, pam_text, right, row_contig, row_off, names, want, order=None, tables=None):
    """device result == the reference rows `want` = (rows, units, n_unscorable) of the records in INPUT order"""
    rows, units, n_uns = want
    rc, blob, off, cfd, got_uns, nbytes = R.device_text(cols, guides, G, pam_text, right, row_contig, row_off, names, order, tables)
    assert rc == _lib.HAWK_OK
    idx = np.arange(len(rows)) if order is None else np.asarray(order, dtype=np.int64)
    text = [rows[int(i)] for i in idx]
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in text], dtype=np.int64)]).tolist()
    assert bytes(blob) == "".join(text).encode("ascii")
    assert np.array_equal(cfd, units[idx]) and nbytes == int(off[-1])
    assert got_uns == (n_uns if order is None else sum(1 for i in idx if _unscorable(rows[int(i)], units[int(i)], tables)))
    return off


def _unscorable(row, unit, tables):
    return tables is not None and unit < 0


# ---- row counts and orders ------------------------------------------------------------------------------------------------
_POOL = {}


def _pool():
    """4097 random records of every kind over six rows of four contigs (one name of 300 bytes), with tables: made once"""
    if not _POOL:
        rng = np.random.default_rng(77)
        guides = [synth.random_sequence(rng, 20) for _ in range(9)]
        names = ["c", "chr2", "chromosome_seventeen", "y" * 300]
        row_contig = np.array([0, 1, 1, 2, 2, 0, 3], dtype=np.uint32)
        row_off = np.array([0, 0, 1 << 22, 999_999_999, 5, (1 << 32) + 12345, 9], dtype=np.uint64)
        w = np.array([0.18, 0.18, 0.18, 0.18, 0.18, 0.09, 0.01])  # the 300-byte name is rare: most waves are staged in LDS
        recs = R.random_records(rng, 4097, guides, 3, False, len(row_contig))
        for r, row in zip(recs, rng.choice(len(row_contig), size=len(recs), p=w).tolist()):
            r["row"] = row
        cols = R.columns(recs)
        tables = synth.cfd_tables()
        want = R.expected(cols, guides, "NGG", False, [names[int(c)] for c in row_contig], row_off, tables)
        _POOL.update(guides=guides, names=names, row_contig=row_contig, row_off=row_off, cols=cols, tables=tables, want=want)
    return _POOL


@pytest.mark.parametrize("order_kind", ["none", "reversed", "random"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_row_counts_and_orders(n, order_kind):
    p = _pool()
    cols = {k: v[:n] for k, v in p["cols"].items()}
    rows, units, _ = p["want"]
    want = (rows[:n], units[:n], int(sum(1 for u in units[:n] if u < 0)))
    order = None if order_kind == "none" else np.arange(n)[::-1].copy() if order_kind == "reversed" else np.random.default_rng(n).permutation(n)
    _check(cols, p["guides"], 20, "NGG", False, p["row_contig"], p["row_off"], p["names"], want, order, p["tables"])


def test_order_may_repeat_rows():
    p = _pool()
    n = 200
    cols = {k: v[:n] for k, v in p["cols"].items()}
    rows, units, _ = p["want"]
    order = np.random.default_rng(3).integers(0, n, size=n)
    _check(cols, p["guides"], 20, "NGG", False, p["row_contig"], p["row_off"], p["names"], (rows[:n], units[:n], 0), order, p["tables"])


# ---- row shapes -----------------------------------------------------------------------------------------------------------
def test_row_shapes_names_positions_and_alignment_phases():
    """Contig names of 1..17 bytes and one of 300, positions at every change of the decimal width up to 10^9 and one past 2^32
    (through the row's offset).  The records come in three runs: name-fastest (the long name is one row in 18: its waves are
    staged, short-named neighbours around it), then a run in which every fourth row has the long name (such a wave's range
    exceeds the LDS slot: its rows go straight to global memory between staged waves), then short names only.  From the offsets: both paths occur,
    and every one of the 16 alignment phases of the destination occurs at the first byte of some wave (the blob starts on a
    256-byte boundary: it is a block of the caching allocator)."""
    rng = np.random.default_rng(12)
    names = ["abcdefghijklmnopq"[:k] for k in range(1, 18)] + ["L" * 300]
    positions = [0] + [v for e in range(1, 10) for v in (10 ** e - 1, 10 ** e)]
    row_contig = np.array(list(range(18)) + [3], dtype=np.uint32)
    row_off = np.array([0] * 18 + [(1 << 32) + 1], dtype=np.uint64)
    guides = [GUIDE, synth.random_sequence(rng, 20)]
    recs = []

    def add(row, q):
        one = R.random_records(rng, 1, guides, 3, False, 1, p_n=0.0)[0]
        recs.append(dict(one, row=row, q=q))
    for q in positions + [5]:
        for row in range(19):
            add(row, q)
    for k in range(1024):
        add(17 if k % 4 == 0 else int(rng.integers(0, 17)), positions[k % len(positions)])
    for k in range(3072):  # more first bytes of waves: 16 phases want a few dozen draws
        add(int(rng.integers(0, 17)), positions[k % len(positions)] + k % 7)
    cols = R.columns(recs)
    tables = synth.cfd_tables()
    want = R.expected(cols, guides, "NGG", False, [names[int(c)] for c in row_contig], row_off, tables)
    assert any(r.split("\t")[1] == str((1 << 32) + 1 + 5) for r in want[0])
    assert {r.split("\t")[1] for r in want[0]} >= {str(v) for v in positions}
    off = _check(cols, guides, 20, "NGG", False, row_contig, row_off, names, want, None, tables)
    n = len(recs)
    firsts = list(range(0, n, 64))
    phases = {int(off[i]) % 16 for i in firsts}
    assert phases == set(range(16))
    direct = [int(off[min(i + 64, n)] - off[i]) + int(off[i]) % 16 > OTT_SLOT for i in firsts]
    has_long = [bool((cols["row"][i:i + 64] == 17).any()) for i in firsts]
    assert any(d for d in direct) and any(h and not d for d, h in zip(direct, has_long))
    # a wave straight to global memory between two staged ones
    assert any((not direct[k - 1]) and direct[k] for k in range(1, len(direct))) and any(direct[k - 1] and not direct[k] for k in range(1, len(direct)))


# ---- bulge placements -----------------------------------------------------------------------------------------------------
def _placements(guide, kind, size, pam_site, right, rng):
    G = len(guide)
    Gs = R.site_len(G, kind, size)
    span = Gs if kind == 1 else G
    recs = []
    for pos in itertools.combinations(range(1, span - 1), size):
        gaps = sum(1 << p for p in pos)
        site, gi = [], 0
        if kind == 1:
            for si in range(Gs):
                if (gaps >> si) & 1:
                    site.append("ACGT"[int(rng.integers(0, 4))])
                else:
                    site.append(guide[gi]); gi += 1
        else:
            site = [c for i, c in enumerate(guide) if not (gaps >> i) & 1]
        for k in rng.integers(0, Gs, size=int(rng.integers(0, 3))).tolist():  # up to two substitutions anywhere
            site[k] = "ACGT"[int(rng.integers(0, 4))]
        for strand in (0, 1):
            recs.append(R.make_record(0, guide, "".join(site), pam_site, right, kind, gaps, 0, 1000 + len(recs), strand))
    return recs


@pytest.mark.parametrize("pam_text,pam_site,G,right,kinds", [
    ("NGG", "TGG", 20, False, [(1, 1), (1, 2), (2, 1), (2, 2)]),
    ("NGG", "AGG", 27, False, [(1, 2)]),            # a window of 32 bases
    ("TTTV", "TTTA", 26, True, [(1, 2), (2, 2)]),   # ... with the PAM in front
    ("TTTV", "TTTC", 23, True, [(1, 1), (2, 1)])])
def test_every_bulge_placement(pam_text, pam_site, G, right, kinds):
    """every gap position 1 .. span - 2 (size 1) and every pair (size 2), DNA and RNA, both strands"""
    rng = np.random.default_rng(G)
    guide = synth.random_sequence(rng, G)
    recs = []
    for kind, size in kinds:
        part = _placements(guide, kind, size, pam_site, right, rng)
        span = R.site_len(G, kind, size) if kind == 1 else G
        assert len(part) == 2 * len(list(itertools.combinations(range(span - 2), size)))
        recs += part
    cols = R.columns(recs)
    tables = None if right else synth.cfd_tables()
    rows_of, offs = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    want = R.expected(cols, [guide], pam_text, right, ["chr7"], offs, tables)
    _check(cols, [guide], G, pam_text, right, rows_of, offs, ["chr7"], want, None, tables)
    for row in want[0][:: max(1, len(want[0]) // 50)]:
        f = row.split("\t")
        if right:  # the PAM stands in front, the cfd column is NA
            assert f[3].startswith(pam_text) and f[4].startswith(pam_site) and f[9] == "NA"
        else:
            assert f[3].endswith(pam_text) and f[4].endswith(pam_site) and f[9] != "NA"


# ---- CFD ------------------------------------------------------------------------------------------------------------------
def _one(cols_recs, guides, G, tables, pam_text="NGG"):
    cols = R.columns(cols_recs)
    rows_of, offs = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    want = R.expected(cols, guides, pam_text, False, ["chr1"], offs, tables)
    _check(cols, guides, G, pam_text, False, rows_of, offs, ["chr1"], want, None, tables)
    return want


def test_cfd_table_index_is_the_alignment_column():
    """a DNA bulge at column 5, a mismatch at column 12 (guide base 11): the table is read at [12], not at [11]"""
    mm = np.ones((20, 4, 4))
    a = "ACGT".index(GUIDE[11])
    b = (a + 1) % 4
    mm[12, a, b] = 0.25
    mm[11, a, b] = 0.5
    site = list(GUIDE[:5] + "G" + GUIDE[5:])
    site[12] = "ACGT"[b]
    rec = R.make_record(0, GUIDE, "".join(site), "AGG", False, kind=1, gaps=1 << 5)
    rows, units, n_uns = _one([rec], [GUIDE], 20, (mm, np.ones(16)))
    assert units.tolist() == [2500] and rows[0].split("\t")[9] == "0.25" and n_uns == 0


def test_cfd_reads_twenty_columns():
    """G = 23: a mismatch at guide index 19 is scored, one at 20 is ignored; 20 mismatches in one row multiply up"""
    rng = np.random.default_rng(2)
    g23 = synth.random_sequence(rng, 23)
    mm = np.full((20, 4, 4), 0.5)
    pt = np.ones(16)

    def sub(g, k):
        return g[:k] + "ACGT"[("ACGT".index(g[k]) + 1) % 4] + g[k + 1:]
    recs = [R.make_record(0, g23, sub(g23, 19), "AGG", False), R.make_record(0, g23, sub(g23, 20), "AGG", False, q=1)]
    rows, units, _ = _one(recs, [g23], 23, (mm, pt))
    assert units.tolist() == [5000, 10000] and [r.split("\t")[9] for r in rows] == ["0.5", "1.0"]
    site = "".join("ACGT"[("ACGT".index(c) + 1 + k % 3) % 4] for k, c in enumerate(GUIDE))
    mm, pt = synth.cfd_tables()
    rows, units, n_uns = _one([R.make_record(0, GUIDE, site, "AGG", False)], [GUIDE], 20, (mm, pt))
    assert rows[0].split("\t")[6] == "20" and n_uns == 0 and units[0] >= 0


def test_cfd_exact_ties_and_powers_of_ten():
    """the exact ties of test_rounding_ties_reach_the_kernel (0.03125 = 312.5 units, 0.09375 = 937.5 units, one ulp either side)
    and rows worth 0, 1, 10, 100, 1000 and 10000 units: one mismatch per row, at column j, whose table entry is the value"""
    vals = [0.03125, 0.09375, np.nextafter(0.03125, 1.0), np.nextafter(0.03125, 0.0), np.nextafter(0.09375, 1.0), np.nextafter(0.09375, 0.0),
            0.0, 1e-4, 1e-3, 1e-2, 1e-1, 1.0]
    mm = np.ones((20, 4, 4))
    recs = []
    for j, v in enumerate(vals):
        mm[j, :, :] = v
        site = GUIDE[:j] + "ACGT"[("ACGT".index(GUIDE[j]) + 1 + j % 3) % 4] + GUIDE[j + 1:]
        recs.append(R.make_record(0, GUIDE, site, "AGG", False, q=j, strand=j % 2))
    rows, units, n_uns = _one(recs, [GUIDE], 20, (mm, np.ones(16)))
    assert units.tolist() == [312, 938, 313, 312, 938, 937, 0, 1, 10, 100, 1000, 10000] and n_uns == 0
    assert [r.split("\t")[9] for r in rows] == ["0.0312", "0.0938", "0.0313", "0.0312", "0.0938", "0.0937", "0.0", "0.0001", "0.001", "0.01", "0.1", "1.0"]


def test_ambiguous_bases_under_a_lookup():
    """N in an aligned spacer column and in each of the PAM's last two bases: the row prints n / N, its cfd is NA and it is
    counted; an N beyond column 20 or in the PAM's first base is not under a lookup; without tables nothing is counted"""
    g23 = synth.random_sequence(np.random.default_rng(8), 23)
    tables = synth.cfd_tables()
    recs = [R.make_record(0, GUIDE, GUIDE[:7] + "N" + GUIDE[8:], "AGG", False), R.make_record(0, GUIDE, GUIDE, "ANG", False, q=1),
            R.make_record(0, GUIDE, GUIDE, "AGN", False, q=2), R.make_record(0, GUIDE, GUIDE, "NGG", False, q=3)]
    rows, units, n_uns = _one(recs, [GUIDE], 20, tables)
    f = [r.split("\t") for r in rows]
    assert n_uns == 3 and units.tolist()[:3] == [-1, -1, -1] and units[3] >= 0
    assert f[0][4] == GUIDE[:7] + "n" + GUIDE[8:] + "AGG" and f[1][4].endswith("ANG") and f[2][4].endswith("AGN") and f[3][4].endswith("NGG")
    assert [x[9] for x in f[:3]] == ["NA"] * 3 and f[3][9] != "NA"
    rows, units, n_uns = _one(recs, [GUIDE], 20, None)
    assert n_uns == 0 and units.tolist() == [-1] * 4 and all(r.split("\t")[9] == "NA" for r in rows)
    rows, units, n_uns = _one([R.make_record(0, g23, g23[:21] + "N" + g23[22:], "AGG", False)], [g23], 23, tables)
    assert n_uns == 0 and units[0] >= 0 and rows[0].split("\t")[4][21] == "n"


def test_cfd_units_equal_compute_cfd_batch():
    """the rows' CFD units against the stand-alone CFD kernel (k_cfd through scoring.compute_cfd_batch, pinned to g5_cfd_edges)
    on the strings the rows print"""
    p = _pool()
    scoring.set_cfd_tables(*p["tables"])
    rows, units, _ = p["want"]
    keep = [i for i in range(len(rows)) if units[i] >= 0]
    P = 3
    wt, sg, pm = [], [], []
    for i in keep:
        f = rows[i].split("\t")
        wt.append(f[3][:-P].upper()); sg.append(f[4][:-P].upper()); pm.append(f[4][-2:])
    vals = scoring.compute_cfd_batch(wt, sg, pm, True)
    n = len(rows)
    rc, blob, off, cfd, n_uns, _nb = R.device_text(p["cols"], p["guides"], 20, "NGG", False, p["row_contig"], p["row_off"], p["names"], None, p["tables"])
    assert rc == _lib.HAWK_OK and len(cfd) == n
    assert cfd[keep].tolist() == [int(round(round(float(v), 4) * 1e4)) for v in vals.tolist()]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_usable():
    good = R.valid_dna_record(GUIDE)
    rows_of, offs = np.zeros(2, np.uint32), np.array([0, 100], dtype=np.uint64)
    tables = synth.cfd_tables()

    def run(recs, order=None):
        return R.device_text(R.columns(recs), [GUIDE], 20, "NGG", False, rows_of, offs, ["chr1"], order, tables)
    cases = [(what, [good, dict(good, **change)], None) for what, change in R.malformed_cases()]
    cases.append(("an order entry >= n", [good, good], np.array([1, 2], dtype=np.uint64)))
    want = R.expected(R.columns([good, good]), [GUIDE], "NGG", False, ["chr1", "chr1"], offs, tables)
    for what, recs, order in cases:
        rc, blob, off, cfd, n_uns, nbytes = run(recs, order)
        assert rc == _lib.HAWK_E_INVALID, what
        assert (n_uns, nbytes) == (0xDEAD, 0xDEAD), what  # the outputs as the caller left them
        _check(R.columns([good, good]), [GUIDE], 20, "NGG", False, rows_of, offs, ["chr1"], want, None, tables)
    # a download without a result to fetch is refused too
    import ctypes as C
    o = np.zeros(3, np.uint64)
    assert _lib.lib().hawk_offtarget_text_download(_lib.context(None), None, o.ctypes.data_as(C.c_void_p), None, None) == _lib.HAWK_E_INVALID


# ---- the product route ----------------------------------------------------------------------------------------------------
def _pam(text, right):
    pam = PAM(text, right, True)
    pam.encode(0)
    return pam


def _both_engines(tmp_path, tag, spacers, pam, genome, coord, mm, bdna, brna, G, right, annotations=None, anncolnames=None):
    out = {}
    for engine in ("objects", "device"):
        d = tmp_path / f"{tag}_{engine}"
        d.mkdir()
        res = estimate_offtargets_spacers(spacers, pam, genome, coord, mm, bdna, brna, G, right, str(d), 0, True, annotations, anncolnames,
                                          engine=engine)
        (f,) = list(d.glob("offtargets_*.tsv"))
        out[engine] = (res, f.read_bytes(), f.name)
    assert out["device"][2] == out["objects"][2]
    assert out["device"][1] == out["objects"][1]
    assert out["device"][0] == out["objects"][0]
    return out["device"]


def _g11_files(tmp_path):
    fx = load_golden("g11_annotation.json.gz")["ngg"]
    paths = []
    for k, t in enumerate(fx["annotation_files"]):
        p = tmp_path / f"ann{k}.bed"
        p.write_text(t)
        paths.append(str(p))
    return paths, list(fx["annotation_colnames"])


@pytest.mark.parametrize("name", ["ngg", "cpf1"])
def test_g10_tables_equal_the_objects_engine(name, tmp_path):
    """the g10 genome and guides: no bulges, bulges of up to 1 and 2, with and without g11's two annotation files (chrO is in
    neither file, chrD1 in both, chrD2 in the second)"""
    fx = load_golden("g10_offtargets.json.gz")[name]
    scoring.set_cfd_tables(*synth.cfd_tables())
    pam = _pam(fx["pam"], fx["right"])
    coord = Coordinate(fx["contig"], fx["startp"], fx["stopp"], 100)
    G = fx["guidelen"]
    genome = GenomeIndex(fx["genome"], G, len(pam), max_bulge=2)
    files, colnames = _g11_files(tmp_path)
    spacers = fx["unique_spacers"]
    for b in (0, 1, 2):
        use = spacers if b < 2 else spacers[:40]
        res, text, _ = _both_engines(tmp_path, f"b{b}", use, pam, genome, coord, 2 if b else fx["mm"], b, b, G, fx["right"])
        assert text.startswith(("\t".join(OTREPCNAMES) + "\n").encode()) and sum(n for n, _c in res.values()) == text.count(b"\n") - 1
        res2, text2, _ = _both_engines(tmp_path, f"b{b}a", use, pam, genome, coord, 2 if b else fx["mm"], b, b, G, fx["right"], files, colnames)
        assert res2 == res and text2.split(b"\n")[0] == ("\t".join(OTREPCNAMES + colnames)).encode()


_SEAMS = {}


def _seam_genome():
    """Three contigs of 20 kb (chrA and chrD1 are in g11's annotation files, zz9 in neither), rows of 1024 bases, 70 guides; sites
    of every kind planted on both strands at every start around a row seam, in the annotated stretch and elsewhere"""
    if not _SEAMS:
        from test_gpu_offtargets import _KINDS, _mutate, _place
        rng = np.random.default_rng(606)
        G, P, piece = 20, 3, 1024
        guides = [synth.random_sequence(rng, G) for _ in range(70)]
        contigs = {}
        n_planted = 0
        for ci, name in enumerate(("chrA", "chrD1", "zz9")):
            g = list(synth.random_sequence(rng, 20_000))
            for j in range(1, 19):
                kind, b = _KINDS[(j + ci) % 5]
                Lw = G + P + (b if kind == "DNA" else -b)
                d = int(rng.integers(0, Lw + 1))  # the window starts d bases in front of the seam: across it, at it
                sp = _mutate(rng, guides[(7 * j + ci) % 70], kind, b, int(rng.integers(0, 3)))
                _place(g, j * piece - d, sp, "TGG", False, (j + ci) % 2 == 1)
                n_planted += 1
            for k in range(6):  # inside the annotated stretch
                kind, b = _KINDS[(k + ci) % 5]
                sp = _mutate(rng, guides[(11 * k + ci) % 70], kind, b, 1)
                _place(g, 460 + 97 * k, sp, "AGG", False, k % 2 == 0)
                n_planted += 1
            contigs[name] = "".join(g)
        _SEAMS.update(contigs=contigs, guides=guides, n_planted=n_planted, index=GenomeIndex(contigs, G, P, piece=piece, max_bulge=2))
    return _SEAMS


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("annotated", [False, True])
def test_seam_genome_tables_equal_the_objects_engine(b, annotated, tmp_path):
    s = _seam_genome()
    scoring.set_cfd_tables(*synth.cfd_tables())
    pam = _pam("NGG", False)
    files, colnames = _g11_files(tmp_path) if annotated else (None, None)
    res, text, _ = _both_engines(tmp_path, "s", s["guides"], pam, s["index"], Coordinate("chrA", 100, 900, 100), 2, b, b, 20, False, files, colnames)
    rows = [ln.split("\t") for ln in text.decode().splitlines()[1:]]
    kinds = {(r[8], int(r[7])) for r in rows}
    assert kinds == {("X", 0)} | {(t, k) for t in ("DNA", "RNA") for k in range(1, b + 1)}
    assert {r[2] for r in rows} == {"+", "-"} and {r[0] for r in rows} == {"chrA", "chrD1", "zz9"}
    assert len(rows) >= s["n_planted"] * (1 + 2 * b) // 5
    if annotated:
        assert any(r[11] != "NA" for r in rows if r[0] == "chrA") and all(r[11] == r[12] == "NA" for r in rows if r[0] == "zz9")


def test_offtarget_arrays_are_the_objects_in_their_order():
    """GenomeIndex.offtarget_arrays: the un-bulged hits in scan()'s order, then the bulged ones in scan_bulges()' order; the
    index's own window is put back"""
    s = _seam_genome()
    idx, guides, pam = s["index"], s["guides"], _pam("NGG", False)
    arr = idx.offtarget_arrays(guides, pam, False, 2, 2, 2)
    assert idx._meta_guidelen == idx.guidelen
    hits = idx.scan(guides, pam, False, 2)
    bulged = idx.scan_bulges(guides, pam, False, 2, 2, 2, engine="device")
    rc, roff, _b, _o, names = idx.row_table()
    got = [(int(g), names[int(rc[r])], int(roff[r]) + int(q), "-" if st else "+", int(m), R.KINDS[int(k)], int(sz), int(gp))
           for g, r, q, st, m, k, sz, gp in zip(arr["guide"], arr["row"], arr["q"], arr["strand"], arr["mm"], arr["kind"], arr["size"], arr["gaps"])]
    want = [(h.guide, h.contig, h.position, h.strand, h.mm, "X", 0, 0) for h in hits] + \
        [(h.guide, h.contig, h.position, h.strand, h.mm, h.bulge_type, h.bulge_size, h.gaps) for h in bulged]
    assert got == want and len(bulged) > 0


def test_text_that_needs_quoting_takes_the_objects_engine(tmp_path, monkeypatch):
    """a label with a quote, a column name with a tab (a BED field itself cannot hold a tab): the device engine hands the call to
    the objects engine, which writes through pandas - same bytes, same result"""
    s = _seam_genome()
    scoring.set_cfd_tables(*synth.cfd_tables())
    from crisprhawk_hip import offtargets as ot_mod
    calls = []
    real = ot_mod.report_offtargets
    monkeypatch.setattr(ot_mod, "report_offtargets", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    bed = tmp_path / "quoted.bed"
    bed.write_text('chrA\t400\t1200\ta"quoted"label\nchrD1\t400\t1200\tplain\n')
    args = (s["guides"][:20], _pam("NGG", False), s["index"], Coordinate("chrA", 100, 900, 100), 2, 0, 0, 20, False)
    _res, text, _ = _both_engines(tmp_path, "q", *args, [str(bed)], None)
    assert len(calls) == 2 and b'"a""quoted""label"' in text  # the objects engine itself, and the device engine's fallback
    calls.clear()
    bed.write_text("chrA\t400\t1200\tplain\n")
    _both_engines(tmp_path, "t", *args, [str(bed)], ["a\tname"])
    assert len(calls) == 2
    calls.clear()
    _both_engines(tmp_path, "p", *args, [str(bed)], ["name"])
    assert len(calls) == 1  # plain text stays on the device engine


def test_zero_hits_write_the_header_alone(tmp_path):
    scoring.set_cfd_tables(*synth.cfd_tables())
    genome = {"chrZ": "A" * 3000}
    res, text, _ = _both_engines(tmp_path, "z", [GUIDE], _pam("NGG", False), genome, Coordinate("chrZ", 100, 900, 100), 2, 1, 1, 20, False)
    assert text == ("\t".join(OTREPCNAMES) + "\n").encode() and res == {GUIDE: (0, "1.0")}


def test_an_unscorable_site_raises_before_any_file(tmp_path):
    scoring.set_cfd_tables(*synth.cfd_tables())
    rng = np.random.default_rng(9)
    g = list(synth.random_sequence(rng, 4000))
    g[1000:1023] = list(GUIDE[:4] + "N" + GUIDE[5:] + "TGG")
    for engine in ("objects", "device"):
        d = tmp_path / engine
        d.mkdir()
        with pytest.raises(CrisprHawkCfdScoreError):
            estimate_offtargets_spacers([GUIDE], _pam("NGG", False), {"chrN": "".join(g)}, Coordinate("chrN", 100, 900, 100), 2, 0, 0, 20, False,
                                        str(d), 0, True, engine=engine)
        assert list(d.iterdir()) == []


def test_search_files_reaches_the_device_engine(tmp_path, monkeypatch):
    from crisprhawk_hip import pipeline, readers
    fx = load_golden("g10_offtargets.json.gz")["ngg"]
    fa, bed, vcf = str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), str(tmp_path / "v.vcf")
    readers.write_fasta(fa, fx["contig"], fx["genome"][fx["contig"]], 60)
    with open(bed, "w") as f:
        f.write(f"{fx['contig']}\t{fx['bed_start']}\t{fx['bed_stop']}\n")
    rows = [[fx["contig"], str(p), ".", r, a, ".", "PASS", f"AF={af:.6g}", "GT"] + [f"{g[0]}|{g[1]}" for g in gts]
            for p, r, a, af, gts in fx["variants"]]
    readers.write_vcf(vcf, fx["contig"], fx["samples"], rows, False)
    calls = []
    real = GenomeIndex.rows_text
    monkeypatch.setattr(GenomeIndex, "rows_text", lambda self, *a, **k: (calls.append(len(a[0]["guide"])), real(self, *a, **k))[1])
    out = tmp_path / "out"
    pipeline.search_files(fa, bed, [vcf], fx["pam"], fx["guidelen"], fx["right"], str(out), cfd_tables=synth.cfd_tables(),
                          estimate_offtargets=fx["genome"], mm=fx["mm"])
    ot_path = out / f"offtargets_{fx['contig']}_{fx['bed_start']}_{fx['bed_stop']}.tsv"
    assert len(calls) == 1 and calls[0] == len(ot_path.read_text().splitlines()) - 1 > 0
    assert sorted(ot_path.read_text().splitlines()) == sorted(fx["nobulge_offtargets_tsv"].splitlines())
