"""The bulged off-target summary without a device: hawk_host_offtarget_bulge_summary runs every (site, guide) pair through the
function the summing sink of k_ot_bulge runs (csrc/hawk_otbulge.h: otb_pair), so the statement of a bulged row's mismatches,
gaps and CFD is held here to the oracle's brute force over every placement (oracle.offtargets_bulges) with the oracle's
compute_cfd on the two aligned strings (tests/ottable_refs.record_strings: a mirror of GenomeIndex._bulge_hit)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bulge_refs as B
import ottable_refs as R
from crisprhawk_hip import _lib, synth
from crisprhawk_hip.genome import encode_guides
from oracle import oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ((True, 1), (True, 2), (False, 1), (False, 2))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def site_windows(genome: str, pam: str, right: bool, spacer: int):
    """the windows of spacer + len(pam) bases that bear the PAM, both strands, in guide orientation (bulge_refs.sites with the
    whole window instead of the spacer): what k_ot_sites writes as site records"""
    P = len(pam)
    L = spacer + P
    g = genome.upper()
    out = []
    for w in range(len(g) - L + 1):
        for strand in (0, 1):
            win = g[w:w + L] if strand == 0 else B.revcomp(g[w:w + L])
            pm = win[:P] if right else win[spacer:]
            if all(q == "N" or (c in "ACGT" and c in B._IUPAC[q]) for c, q in zip(pm, pam)):
                out.append(win)
    return out


def host_summary(windows, guides, pam_len: int, right: bool, max_mm: int, dna: bool, b: int, tables, G=None):
    """hawk_host_offtarget_bulge_summary over windows given as strings: (status, hist, cfd_e4, n_hits, n_unscorable)"""
    enc = [R.encode_window(w) for w in windows]
    code = np.array([c for c, _n in enc], dtype=np.uint64)
    nmask = np.array([n for _c, n in enc], dtype=np.uint32)
    g2 = encode_guides(list(guides)) if len(guides) else np.zeros(0, np.uint64)
    G = len(guides[0]) if G is None else G
    par = _lib.OtParams(0, 0, pam_len, G, int(bool(right)), max_mm)
    hist = np.full((len(guides), max_mm + 1), 0xABCD, dtype=np.uint32)
    cfd = np.full(len(guides), -7, dtype=np.int64)
    mm = pt = None
    if tables is not None:
        mm = np.ascontiguousarray(tables[0], dtype=np.float64).reshape(20, 4, 4)
        pt = np.ascontiguousarray(tables[1], dtype=np.float64).reshape(16)
    nh, nu = C.c_uint64(0xDEAD), C.c_uint64(0xDEAD)
    rc = _lib.lib().hawk_host_offtarget_bulge_summary(_p(code), _p(nmask), C.c_uint64(len(windows)), _p(g2), C.c_uint32(len(guides)), C.byref(par),
                                                      C.c_uint32(1 if dna else 2), C.c_uint32(b), _p(mm), _p(pt), _p(hist), _p(cfd),
                                                      C.byref(nh), C.byref(nu))
    return rc, hist, cfd, nh.value, nu.value


def row_units(window: str, guide: str, gaps: int, dna: bool, b: int, P: int, right: bool, tables):
    """the CFD of one row in 1e-4 units as the table route has it: the oracle's compute_cfd on (grna, spacer, spacer field[-2:])
    of the aligned strings, rounded by Python; None where compute_cfd raises"""
    code, nmask = R.encode_window(window)
    cr, dn, pm = R.record_strings(dict(code=code, nmask=nmask, gaps=gaps, kind=1 if dna else 2, size=b), guide, P, right)
    field = (pm + dn) if right else (dn + pm)
    try:
        return int(round(round(ora.cfd(cr.upper(), dn.upper(), field[-2:], tables[0], tables[1]), 4) * 1e4))
    except ora.OracleError:
        return None


def oracle_summary(contigs, guides, pam: str, right: bool, max_mm: int, tables):
    """{(dna, b): (hist, cfd_e4, n_hits, n_unscorable)} from oracle.offtargets_bulges at bdna = brna = 2"""
    G, P = len(guides[0]), len(pam)
    out = {k: [np.zeros((len(guides), max_mm + 1), np.int64), np.zeros(len(guides), np.int64), 0, 0] for k in KINDS}
    for seq in contigs.values():
        for r in ora.offtargets_bulges(seq, guides, pam, right, max_mm, 2, 2):
            dna, b = int(r["btype"]) == 1, int(r["bsize"])
            L = (G + b if dna else G - b) + P
            win = seq[int(r["pos"]):int(r["pos"]) + L].upper()
            win = B.revcomp(win) if int(r["strand"]) else win
            acc = out[(dna, b)]
            acc[0][int(r["guide"]), int(r["mm"])] += 1
            acc[2] += 1
            if tables is not None:
                u = row_units(win, guides[int(r["guide"])], int(r["gaps"]), dna, b, P, right, tables)
                if u is None:
                    acc[3] += 1
                else:
                    acc[1][int(r["guide"])] += u
    return out


def planted_genome(pam: str, G: int, right: bool, seed: int):
    """two contigs of a few kb with bulged near-copies of eight guides on both strands (every type and size, 0..4 substitutions),
    one copy with an N inside the spacer, one with an IUPAC code, and an N run"""
    rng = np.random.default_rng(seed)
    guides = [B.random_seq(rng, G) for _ in range(8)]
    concrete = B.CONCRETE.get(pam, "TGA")
    contigs = {}
    for name, n in (("a", 5000), ("b", 2501)):
        g = list(B.random_seq(rng, n))
        pos = 40
        while pos + 80 < n:
            gd = guides[int(rng.integers(0, len(guides)))]
            kind, b = (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))[int(rng.integers(0, 4))]
            sp = list(B.mutate(rng, gd, kind, b, int(rng.integers(0, 5))))
            if rng.random() < 0.15:
                sp[int(rng.integers(0, len(sp)))] = "N" if rng.random() < 0.6 else "R"
            B.place(g, pos, "".join(sp), concrete, right, bool(rng.random() < 0.5))
            pos += 64
        g[1500:1530] = "N" * 30
        contigs[name] = "".join(g)
    return contigs, guides


_CASES = {}


def _case(pam: str, G: int, right: bool):
    if (pam, G, right) not in _CASES:
        _CASES[(pam, G, right)] = planted_genome(pam, G, right, 20 + G)
    return _CASES[(pam, G, right)]


def test_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "hawk.h")).read()
    for sym in ("hawk_offtarget_bulge_summary", "hawk_host_offtarget_bulge_summary"):
        assert sym in _lib.EXPORTS
        assert re.search(r"^int " + sym + r"\(", header, re.M), sym
    assert hasattr(_lib.lib(), "hawk_host_offtarget_bulge_summary")


@pytest.mark.parametrize("max_mm", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("pam,G,right", [("NGG", 20, False), ("TTTV", 23, True)])
def test_host_twin_equals_the_oracle(pam, G, right, max_mm):
    """both types, both sizes: histogram, CFD sum, row count and unscorable count equal the oracle's rows'"""
    contigs, guides = _case(pam, G, right)
    tables = synth.cfd_tables()
    want = oracle_summary(contigs, guides, pam, right, max_mm, tables)
    seen_rows = seen_uns = 0
    for dna, b in KINDS:
        wins = [w for seq in contigs.values() for w in site_windows(seq, pam, right, G + b if dna else G - b)]
        rc, hist, cfd, nh, nu = host_summary(wins, guides, len(pam), right, max_mm, dna, b, tables)
        w_hist, w_cfd, w_n, w_uns = want[(dna, b)]
        assert rc == _lib.HAWK_OK
        assert np.array_equal(hist, w_hist), (dna, b)
        assert np.array_equal(cfd, w_cfd), (dna, b)
        assert (nh, nu) == (w_n, w_uns), (dna, b)
        # counts only: the same histogram, the sums zeroed
        rc, hist0, cfd0, nh0, nu0 = host_summary(wins, guides, len(pam), right, max_mm, dna, b, None)
        assert rc == _lib.HAWK_OK and np.array_equal(hist0, w_hist) and not cfd0.any() and (nh0, nu0) == (w_n, 0)
        seen_rows += w_n
        seen_uns += w_uns
    assert seen_rows >= (20 if max_mm else 4)
    if max_mm >= 1:
        assert seen_uns >= 1, "the planted genome must hold a row with an ambiguous base under a lookup"


GUIDE = "ACGTACGTACGTACGTACGT"  # no two neighbours equal


def _one(site: str, pam_site: str, guide: str, dna: bool, b: int, max_mm: int, tables, right: bool = False):
    rc, hist, cfd, nh, nu = host_summary([(pam_site + site) if right else (site + pam_site)], [guide], len(pam_site), right, max_mm, dna, b, tables)
    assert rc == _lib.HAWK_OK
    return hist[0].tolist(), int(cfd[0]), nh, nu


def test_an_n_inside_the_spacer_is_unscorable_and_an_n_is_never_bulged_out():
    tables = synth.cfd_tables()
    # aligned N: a mismatch, a row, counted in hist and as unscorable, nothing added
    site = GUIDE[:6] + "G" + GUIDE[6:]          # one inserted base: DNA 1, no mismatch
    assert _one(site, "TGG", GUIDE, True, 1, 1, tables)[0] == [1, 0]
    with_n = site[:12] + "N" + site[13:]
    hist, cfd, nh, nu = _one(with_n, "TGG", GUIDE, True, 1, 1, tables)
    assert (hist, cfd, nh, nu) == ([0, 1], 0, 1, 1)
    assert B.best_placement(with_n, GUIDE, 1, True, 1)[0] == 1
    # without tables the same row is no error
    assert _one(with_n, "TGG", GUIDE, True, 1, 1, None) == ([0, 1], 0, 1, 0)
    # the N at the bulged position itself: the placement that would give 0 mismatches is no placement
    n_bulged = GUIDE[:6] + "N" + GUIDE[6:]
    assert B.best_placement(n_bulged, GUIDE, 1, True, 0) is None
    assert _one(n_bulged, "TGG", GUIDE, True, 1, 0, tables) == ([0], 0, 0, 0)
    want = B.best_placement(n_bulged, GUIDE, 1, True, 3)
    hist, _cfd, nh, nu = _one(n_bulged, "TGG", GUIDE, True, 1, 3, tables)
    assert want is not None and hist == [int(k == want[0]) for k in range(4)] and (nh, nu) == (1, 1)  # the N is aligned: unscorable


def test_ngn_with_an_ambiguous_base_in_the_pam_key():
    """an N of the PAM accepts an ambiguous genome base; in PAM[-2:] it is under the PAM table's lookup"""
    rng = np.random.default_rng(3)
    tables = synth.cfd_tables()
    guides = [B.random_seq(rng, 20) for _ in range(3)]
    g = list(B.random_seq(rng, 1500))
    B.place(g, 300, B.mutate(rng, guides[0], "RNA", 1, 1), "TGR", False, False)
    B.place(g, 700, B.mutate(rng, guides[1], "DNA", 2, 0), "AGN", False, True)
    B.place(g, 1100, B.mutate(rng, guides[2], "DNA", 1, 1), "TGA", False, False)
    contigs = {"c": "".join(g)}
    want = oracle_summary(contigs, guides, "NGN", False, 2, tables)
    assert sum(v[3] for v in want.values()) >= 2 and sum(int(v[1].sum()) for v in want.values()) > 0
    for dna, b in KINDS:
        wins = site_windows(contigs["c"], "NGN", False, 20 + b if dna else 20 - b)
        rc, hist, cfd, nh, nu = host_summary(wins, guides, 3, False, 2, dna, b, tables)
        w_hist, w_cfd, w_n, w_uns = want[(dna, b)]
        assert rc == _lib.HAWK_OK and np.array_equal(hist, w_hist) and np.array_equal(cfd, w_cfd) and (nh, nu) == (w_n, w_uns)


def test_a_dna_bulge_moves_the_table_index_of_later_mismatches():
    """mm[c] = (c + 1) / 32 for every base pair, PAM entries 1: the CFD of a row with one mismatch names its alignment column"""
    mm = np.ones((20, 4, 4)) * ((np.arange(20) + 1) / 32)[:, None, None]
    tables = (mm, np.ones(16))
    sub = GUIDE[:10] + "A" + GUIDE[11:]                     # guide position 10: G -> A
    assert _one(sub[:3] + "C" + sub[3:], "TGG", GUIDE, True, 1, 1, tables)[:2] == ([0, 1], int(round(12 / 32 * 1e4)))   # column 11
    assert _one(sub[:14] + "C" + sub[14:], "TGG", GUIDE, True, 1, 1, tables)[:2] == ([0, 1], int(round(11 / 32 * 1e4)))  # bulge behind it: column 10
    assert _one(sub[:3] + sub[4:], "TGG", GUIDE, False, 1, 1, tables)[:2] == ([0, 1], int(round(11 / 32 * 1e4)))        # RNA bulge: the guide's own column
    for site, dna in ((sub[:3] + "C" + sub[3:], True), (sub[:3] + sub[4:], False)):
        mm_, gaps = B.best_placement(site, GUIDE, 1, dna, 1)
        assert _one(site, "TGG", GUIDE, dna, 1, 1, tables)[1] == row_units(site + "TGG", GUIDE, gaps, dna, 1, 3, False, tables)


def test_column_twenty_of_a_dna_bulged_row_is_not_in_the_product():
    """G = 20 with a DNA bulge has 21 alignment columns (22 with two): a mismatch in column 20 is a mismatch of the row and no
    factor of its CFD"""
    mm = np.full((20, 4, 4), 0.25)
    tables = (mm, np.ones(16))
    last = GUIDE[:19] + "A"      # guide position 19 -> column 20 behind one DNA bulge
    prev = GUIDE[:18] + "A" + GUIDE[19:]  # guide position 18 -> column 19
    assert _one(last[:5] + "G" + last[5:], "TGG", GUIDE, True, 1, 1, tables)[:2] == ([0, 1], 10000)
    assert _one(prev[:5] + "G" + prev[5:], "TGG", GUIDE, True, 1, 1, tables)[:2] == ([0, 1], 2500)
    assert _one(prev[:5] + "GA" + prev[5:], "TGG", GUIDE, True, 2, 1, tables)[:2] == ([0, 1], 10000)   # two bulges: position 18 -> column 20
    for site, guide, dna, b in ((last[:5] + "G" + last[5:], GUIDE, True, 1), (prev[:5] + "GA" + prev[5:], GUIDE, True, 2)):
        _mm, gaps = B.best_placement(site, guide, b, dna, 1)
        assert _one(site, "TGG", guide, dna, b, 1, tables)[1] == row_units(site + "TGG", guide, gaps, dna, b, 3, False, tables)


@pytest.mark.parametrize("dna", [True, False])
def test_rounding_ties_on_a_bulged_pair(dna):
    """the tables of test_rounding_ties_reach_the_kernel - a row's CFD is an exact binary tie of round(x, 4) or one ulp either side
    of it - on pairs with a bulge behind the mismatch (position 12): site j has one mismatch, at column j"""
    vals = [0.03125, 0.09375, np.nextafter(0.03125, 1.0), np.nextafter(0.03125, 0.0), np.nextafter(0.09375, 1.0), np.nextafter(0.09375, 0.0)]
    mm = np.ones((20, 4, 4))
    for j, v in enumerate(vals):
        mm[j, :, :] = v
    tables = (mm, np.ones(16))
    got = []
    for j in range(6):
        sp = list(GUIDE)
        sp[j] = "ACGT"[("ACGT".index(sp[j]) + 2) % 4]
        site = "".join(sp[:12]) + ("A" if dna else "") + "".join(sp[12 if dna else 13:])
        hist, cfd, nh, nu = _one(site, "AGG", GUIDE, dna, 1, 1, tables)
        assert (hist, nh, nu) == ([0, 1], 1, 0)
        got.append(cfd)
    assert got == [int(round(round(float(v), 4) * 1e4)) for v in vals] == [312, 938, 313, 312, 938, 937]


def test_refusals_leave_the_outputs_untouched():
    tables = synth.cfd_tables()
    win = [GUIDE[:6] + "G" + GUIDE[6:] + "TGG"]

    def status(dna=True, b=1, max_mm=2, tb=tables, guides=(GUIDE,), wins=win, pam_len=3, G=None):
        rc, hist, cfd, nh, nu = host_summary(wins, list(guides), pam_len, False, max_mm, dna, b, tb, G=G)
        if rc != _lib.HAWK_OK:
            assert (hist == 0xABCD).all() and (cfd == -7).all() and (nh, nu) == (0xDEAD, 0xDEAD)
        return rc
    assert status() == _lib.HAWK_OK
    assert status(b=0) == _lib.HAWK_E_INVALID and status(b=3) == _lib.HAWK_E_INVALID
    assert status(max_mm=33) == _lib.HAWK_E_UNSUPPORTED
    assert status(pam_len=1, wins=[win[0][:-2]]) == _lib.HAWK_E_UNSUPPORTED          # tables need PAM[-2:]
    assert status(pam_len=1, wins=[win[0][:-2]], tb=None) == _lib.HAWK_OK
    assert status(guides=("ACGT",), b=2, wins=["ACGTACTGG"]) == _lib.HAWK_E_UNSUPPORTED   # G = 4 leaves no interior pair beside a bulge of 2
    assert status(guides=("ACGTA",), b=2, wins=["ACGTACATGG"]) == _lib.HAWK_OK
    assert status(guides=("A" * 29,), wins=["A" * 33]) == _lib.HAWK_E_UNSUPPORTED           # 29 + 1 + 3 bases: a 33-base window
    assert status(guides=("A" * 28,), wins=["A" * 29 + "TGG"]) == _lib.HAWK_OK
    L = _lib.lib()
    par = _lib.OtParams(0, 0, 3, 20, 0, 2)
    nh, nu = C.c_uint64(5), C.c_uint64(5)
    mm = np.ascontiguousarray(tables[0], dtype=np.float64)
    hist = np.zeros((1, 3), np.uint32)
    g2 = encode_guides([GUIDE])
    # one table without the other; bulge type out of range
    assert L.hawk_host_offtarget_bulge_summary(None, None, C.c_uint64(0), _p(g2), 1, C.byref(par), 1, 1, _p(mm), None, _p(hist), None, C.byref(nh),
                                               C.byref(nu)) == _lib.HAWK_E_INVALID
    for btype in (0, 3):
        assert L.hawk_host_offtarget_bulge_summary(None, None, C.c_uint64(0), _p(g2), 1, C.byref(par), btype, 1, None, None, _p(hist), None,
                                                   C.byref(nh), C.byref(nu)) == _lib.HAWK_E_INVALID
    assert (nh.value, nu.value) == (5, 5)
    # no sites, no guides: zeros, defined
    assert L.hawk_host_offtarget_bulge_summary(None, None, C.c_uint64(0), None, 0, C.byref(par), 2, 2, None, None, None, None, C.byref(nh),
                                               C.byref(nu)) == _lib.HAWK_OK
    assert (nh.value, nu.value) == (0, 0)


def test_summary_route_with_bulges_passes_the_argument_check(tmp_path):
    """offtargets_summary=True is the summary route at any bdna / brna: the call gets past the refusal that offtargets_table=False
    keeps (tests/test_offtarget_summary_host.py) and fails at the first thing it needs after the argument check - the FASTA, which
    is not there.  No genome is given, so nothing here asks for a device: the same failure on every machine."""
    from crisprhawk_hip import pipeline
    for kw in (dict(brna=1), dict(bdna=2, brna=2), dict(bdna=1, offtargets_table=False)):
        with pytest.raises(FileNotFoundError, match="Cannot find input FASTA"):
            pipeline.search_files(str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), [], "NGG", 20, False, str(tmp_path),
                                  offtargets_summary=True, **kw)
    with pytest.raises(ValueError, match="mismatch-only"):
        pipeline.search_files(str(tmp_path / "g.fa"), str(tmp_path / "r.bed"), [], "NGG", 20, False, str(tmp_path),
                              offtargets_table=False, brna=1)
