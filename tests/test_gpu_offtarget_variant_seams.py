"""The variant-enriched off-target scan on the device at the seams its first suite never reaches: window lengths up to the ABI's
32 bases and down to 8, the ALT-window filter (k_ov_filter) across a word, a lane's four words, a wave and a workgroup, the last
window of a row, the counts layout [strand][row][workgroup] with every cell holding its own number, a dense hawk_genome_variants
call (k_ov_fill), calls that add to the planes, k_ov_match with a partly filled last workgroup beside a second LDS chunk of guides,
the PAM rule in guide orientation, and a sharded index.

Every test asserts (a) the device's rows == the host twin's, `==` on sorted raw tuples, (b) the rows as tuples == the brute force
over strings, and (c) timing.n_sites == the number of windows that bear the PAM and hold an ALT allele (offtarget_variant_refs.sites:
what include/hawk.h says n_sites is) - the filter is otherwise seen only through rows, and k_ov_match drops whatever it keeps too
much.  The scenes are offtarget_variant_refs's; test_offtarget_variants_host.py holds them to the brute force without a device."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import offtarget_variant_refs as V
from crisprhawk_hip import _lib
from crisprhawk_hip.genome import OTV_COLUMNS, GenomeIndex, encode_guides, host_variant_scan, variant_entries, variant_records

pytestmark = pytest.mark.gpu

SYSTEMS = (("NGG", 20, False), ("TTTV", 23, True))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def twin():
    """host_variant_scan of a scene, once per (scene, piece, max_mm, guides)"""
    memo = {}

    def run(sc, piece, max_mm, guides=None):
        key = (id(sc), piece, max_mm, None if guides is None else len(guides))
        if key not in memo:
            memo[key] = host_variant_scan(sc.text(), sc.G, sc.P, piece, sc.records, sc.guides if guides is None else guides,
                                          V.make_pam(sc.pam_text, sc.right), sc.right, max_mm, cap=1 << 19)
        return memo[key]
    return run


def _scan(sc, idx, max_mm, twin, piece, guides=None):
    """The three assertions of this file on one scan of `idx`: the device's columns, its rows as tuples, the timing block"""
    use = sc.guides if guides is None else guides
    h, tm = idx.variant_arrays(use, V.make_pam(sc.pam_text, sc.right), sc.right, max_mm)
    hh, _stats = twin(sc, piece, max_mm, guides)
    if (idx.row_lo, idx.row_hi) != (0, idx.n_rows_total):  # a shard lists the rows of its own window starts
        keep = (hh["row"] >= idx.row_lo) & (hh["row"] < idx.row_hi)
        hh = {k: v[keep] for k, v in hh.items()}
    assert V.raw_tuples(h) == V.raw_tuples(hh)                                                   # (a)
    got = V.rows_as_tuples(h, idx.rows, sc.L)
    mine = {(k, q, s) for k, q, s in V.owned(sc.sites(), idx.rows, idx.row_lo, idx.row_hi)}
    want = sc.brute(max_mm, guides)
    if len(mine) != len(sc.sites()):
        at = {(idx.rows[k][0], idx.rows[k][1] + q, s) for k, q, s in mine}
        want = [r for r in want if (r[1], r[2], r[3]) in at]
    assert got == want                                                                           # (b)
    assert tm["n_sites"] == len(mine), (tm["n_sites"], len(mine))                                # (c)
    return h, got, tm


def _index(sc, piece, **kw):
    return GenomeIndex(sc.text(), sc.G, sc.P, piece=piece, variants=sc.records, **kw)


@pytest.mark.parametrize("pam_text,G,right", V.WINDOW_SYSTEMS)
def test_window_lengths(pam_text, G, right, twin):
    """L = 32 (lmask / gmask at their >= 32 branch, ov_rev32 shifting by 0, spmask filling the word, all 64 code bits, window_or
    ending with rem 0), L = 31 (rem 15), L = 8 (three doubling rounds, no remainder), L = 27 with a six-base PAM"""
    sc = V.window_scene(pam_text, G, right)
    idx = _index(sc, V.PIECE)
    assert idx.variant_stats == V.allele_sets(sc.text(), sc.records)[1]
    for max_mm in (0, 1 if G == 6 else 2):
        _h, got, _tm = _scan(sc, idx, max_mm, twin, V.PIECE)
        V.check_claims(sc, got, max_mm)
        assert {s for _g, _c, _p, s, *_r in got} == {0, 1}


@pytest.mark.parametrize("pam_text,G,right,alphabet", V.SEAM_SYSTEMS)
def test_filter_seams_and_counts_layout(pam_text, G, right, alphabet, twin):
    """Windows that start one bit before a boundary with their ALT L - 1 bits behind it, windows that reach one bit across it, and
    perfect sites whose only ALT lies one base outside them - at the end of a word, of a lane's 128 bits, of a wave's 8192 and of
    a workgroup's 32768; every (strand, row, workgroup) cell of the counts holds a number of sites of its own."""
    sc = V.seam_scene(pam_text, G, right, alphabet)
    idx = _index(sc, V.BIG_PIECE)
    assert len(idx.rows) == 8 and idx.ds.stride > 1024 and -(-(idx.ds.stride // 4) // 256) == 2  # bph: workgroups per row
    _h, got, _tm = _scan(sc, idx, 0, twin, V.BIG_PIECE)
    V.check_claims(sc, got, 0)
    cells = Counter((k, q // V.TILE, s) for k, q, s in V.owned(sc.sites(), idx.rows))
    assert len(cells) == 32 and len(set(cells.values())) == 32
    # the rows cell by cell, so that a swapped index of the counts names its cell
    name_row = {r[0]: k for k, r in enumerate(idx.rows)}
    by_cell = lambda rows: {c: [r for r in rows if (name_row[r[1]], r[2] // V.TILE, r[3]) == c] for c in cells}
    have, want = by_cell(got), by_cell(sc.brute(0))
    for c in sorted(cells):
        assert have[c] == want[c] and len(want[c]) > 0, c


@pytest.mark.parametrize("pam_text,G,right", SYSTEMS)
@pytest.mark.parametrize("n", (1285, 8197))
def test_last_window_of_a_row(pam_text, G, right, n, twin):
    """n = 5 mod 128: the last window start lies in the last of a lane's four words and the contig's last base - the needed ALT -
    in the first look-ahead word, which the lane takes from its neighbour (n = 1285) or, as a wave's last lane, from memory (8197)"""
    for strand in (0, 1):
        sc = V.row_end_scene(pam_text, G, right, n, strand)
        idx = _index(sc, V.BIG_PIECE)
        assert len(idx.rows) == 1 and ((n - sc.L) // 32) % 4 == 3 and ((n - 1) // 32) % 4 == 0
        assert ((n - sc.L) // 128) % 64 == (63 if n == 8197 else 9)
        _h, got, _tm = _scan(sc, idx, 1, twin, V.BIG_PIECE)
        V.check_claims(sc, got, 1)


def test_dense_fill_and_a_partly_filled_last_workgroup(twin):
    """k_ov_fill: 600 entries in seven bitmap words (vector atomicOr on one word from many lanes, all four planes of a position)
    among some 400 more.  k_ov_match: more than 256 sites, the last workgroup partly filled, 1100 guides - its dead lanes pass the
    barriers of the second LDS chunk, and the last site has rows there.  Then cap at exactly the rows' number, and one less."""
    sc = V.dense_scene()
    idx = _index(sc, V.BIG_PIECE)
    assert len(idx.rows) == 1
    lens = {k: len(v) for k, v in sc.text().items()}
    entries = variant_entries(lens, idx._geo, variant_records(sc.records))
    assert len(entries[0]) - 3 * V.DENSE_RUN > 256 and Counter((entries[1] // 32).tolist()).most_common(1)[0][1] == 96
    assert idx.variant_stats == V.allele_sets(sc.text(), sc.records)[1] and idx.variant_stats["applied"] > 3 * V.DENSE_RUN + 256
    _h, got, tm = _scan(sc, idx, 0, twin, V.BIG_PIECE)
    V.dense_claims(sc, got)
    V.check_claims(sc, got, 0)
    assert tm["n_sites"] > 256 and tm["n_sites"] % 256 != 0
    few = sc.guides[:40]
    h, got, _tm = _scan(sc, idx, 1, twin, V.BIG_PIECE, guides=few)
    # the C call itself: room for exactly the rows, then for one less
    n_rows = len(h["guide"])
    pam = V.make_pam(sc.pam_text, sc.right)
    g2 = encode_guides(few)
    par = _lib.OtParams(pam.bits, pam.bitsrc, sc.P, sc.G, 0, 1)
    for cap, status in ((n_rows, _lib.HAWK_OK), (n_rows - 1, _lib.HAWK_E_CAPACITY)):
        out = {k: np.full(n_rows, 0xEE, t) for k, t in OTV_COLUMNS}
        n, tm2 = C.c_uint64(0), _lib.OtTiming()
        rc = idx.ds._L.hawk_offtarget_variant_scan(idx.ds._h, C.byref(par), _p(g2), len(g2), *[_p(out[k]) for k, _t in OTV_COLUMNS],
                                                   C.c_uint64(cap), C.byref(n), C.byref(tm2))
        assert rc == status and n.value == n_rows and tm2.n_sites == len(sc.sites())
        if rc == _lib.HAWK_OK:
            assert V.raw_tuples(out) == V.raw_tuples(h)


def test_calls_that_add_to_the_planes(twin):
    """The records in three hawk_genome_variants calls - the two ALTs of one position in different calls - make the index one call
    makes; the plain scan reads the REF planes and sees none of it."""
    sc = V.shard_scene()
    pam = V.make_pam("NGG", False)
    plain, _ = GenomeIndex(sc.text(), sc.G, sc.P, piece=V.PIECE).scan_arrays(sc.guides, pam, False, 2)
    once = _index(sc, V.PIECE)
    h1, got1, tm1 = _scan(sc, once, 2, twin, V.PIECE)
    idx = GenomeIndex(sc.text(), sc.G, sc.P, piece=V.PIECE)
    parts = [idx.add_variants(c) for c in V.split_calls(sc.records)]
    assert all(p["applied"] > 5 for p in parts) and sum(p["applied"] for p in parts) == once.variant_stats["applied"]
    assert idx.variant_stats == once.variant_stats
    h3, got3, tm3 = _scan(sc, idx, 2, twin, V.PIECE)
    assert V.raw_tuples(h3) == V.raw_tuples(h1) and tm3["n_sites"] == tm1["n_sites"]
    V.check_claims(sc, got3, 2)
    for tag in "+-":
        assert sc.placed["two_alts" + tag] in {(g, c, p, s) for g, c, p, s, *_r in got3}
    after, _ = idx.scan_arrays(sc.guides, pam, False, 2)
    assert len(plain["guide"]) > 0
    oa = np.lexsort((plain["strand"], plain["q"], plain["row"], plain["guide"]))
    ob = np.lexsort((after["strand"], after["q"], after["row"], after["guide"]))
    for k in plain:
        assert plain[k].dtype == after[k].dtype and np.array_equal(plain[k][oa], after[k][ob]), k


@pytest.mark.parametrize("max_mm", (0, 1))
def test_pam_rule_in_guide_orientation_and_n_under_the_pam(max_mm, twin):
    sc = V.pam_lowest_scene()
    _h, got, _tm = _scan(sc, _index(sc, V.PIECE), max_mm, twin, V.PIECE)
    V.check_claims(sc, got, max_mm)  # {A, G} reads A and {C, G} reads C on either strand
    sc = V.pam_n_scene()
    h, got, _tm = _scan(sc, _index(sc, V.PIECE), max_mm, twin, V.PIECE)
    V.check_claims(sc, got, max_mm)
    for tag in "+-":
        gi, _contig, pos, strand = sc.placed["under_pam_n" + tag]
        nm = [int(m) for g, q, s, m in zip(h["guide"].tolist(), h["q"].tolist(), h["strand"].tolist(), h["nmask"].tolist()) if (g, q, s) == (gi, pos, strand)]
        assert nm == [1 << sc.pm(0)]
    assert sum(r[0] == 1 for r in got) == (2 if max_mm else 0)  # the N at a spacer base: a mismatch


def test_sharded_index(twin):
    """Three shards on one device: entries numbered from row_lo, rows reported globally, each listed by one shard"""
    sc = V.shard_scene()
    whole = _index(sc, V.PIECE)
    h, _got, tm = _scan(sc, whole, 2, twin, V.PIECE)
    lens = {k: len(v) for k, v in sc.text().items()}
    recs = variant_records(sc.records)
    union, n_sites, applied = [], 0, Counter()
    for r in range(3):
        idx = _index(sc, V.PIECE, shard=(r, 3))
        assert (idx.row_lo, idx.row_hi) == (2 * r, 2 * r + 2) and idx.n_rows_total == 6
        hs, _gs, ts = _scan(sc, idx, 2, twin, V.PIECE)
        assert len(hs["row"]) > 0 and ((hs["row"] >= idx.row_lo) & (hs["row"] < idx.row_hi)).all()
        union += V.raw_tuples(hs)
        n_sites += ts["n_sites"]
        # the counts as variant_entries predicts them: every record is applied, dropped for a reason, or another shard's
        _row, _q, _rb, _ab, _var, dropped, kept = variant_entries(lens, idx._geo, recs, idx.row_lo, idx.row_hi)
        st = idx.variant_stats
        assert st["applied"] + sum(st["dropped"].values()) == len(recs)
        assert st["dropped"]["other_shard"] == dropped["other_shard"] > 0
        assert st["applied"] + sum(st["dropped"][k] for k in ("ref_n", "ref_mismatch")) == len(kept)
        assert all(st["dropped"][k] == whole.variant_stats["dropped"][k] for k in ("not_snv", "unknown_contig", "out_of_contig", "alt_is_ref", "no_row"))
        for name, pos, _ref, _alt in kept:
            applied[(name, pos)] += (name, pos) in idx._var_applied
    assert sorted(union) == V.raw_tuples(h) and len(set(union)) == len(union) and n_sites == tm["n_sites"]
    # the variant in the overlap of rows 1 and 2 - the last row of shard 0, the first of shard 1 - is applied in both
    _gi, contig, pos, _strand = sc.placed["shard_overlap"]
    assert applied[(contig, pos + 10)] == 2 and sum(v for v in applied.values()) > whole.variant_stats["applied"]
