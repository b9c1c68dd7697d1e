"""The off-target scan over a variant-enriched genome without a device: hawk_host_offtarget_variant_scan runs every (window,
strand, guide) through the resolver the kernel runs for its survivors (csrc/hawk_otvar.h: ov_resolve), so the statement of a
variant row - which PAM and spacer positions read an ALT allele, the mismatches, the alt mask - is held here to a brute force
in plain Python over strings (offtarget_variant_refs.brute), on scenes whose cases are placed by construction."""
import os
import subprocess

import numpy as np
import pytest

import offtarget_variant_refs as V
from crisprhawk_hip import _lib
from crisprhawk_hip.genome import host_variant_scan, row_geometry, variant_entries, variant_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMS = (("NGG", 20, False), ("TTTV", 23, True))


def _twin(sc, max_mm, records=None, guides=None):
    contigs = sc.text()
    pam = V.make_pam(sc.pam_text, sc.right)
    h, stats = host_variant_scan(contigs, sc.G, sc.P, V.PIECE, sc.records if records is None else records, sc.guides if guides is None else guides,
                                 pam, sc.right, max_mm, cap=16)  # a small cap: the capacity answer and the second call
    geo = row_geometry({k: len(v) for k, v in contigs.items()}, sc.G, sc.P, V.PIECE, 0, sc.G)
    return h, stats, geo


@pytest.mark.parametrize("pam_text,G,right", SYSTEMS)
@pytest.mark.parametrize("max_mm", (0, 2, 4))
def test_twin_equals_brute_force_on_placed_cases(pam_text, G, right, max_mm):
    sc = V.standard_scene(pam_text, G, right, max_mm)
    want = V.brute(sc.text(), sc.records, sc.guides, pam_text, right, max_mm)
    # the scene holds what it says: every placed case is (or is not) a row of the brute force
    have = {(g, c, p, s) for g, c, p, s, _mm, _w, _a in want}
    for label, must in V.expect_rows(sc, max_mm).items():
        assert (sc.placed[label] in have) == must, label
    assert {s for _g, _c, _p, s, *_r in want} == {0, 1}
    h, stats, geo = _twin(sc, max_mm)
    assert V.rows_as_tuples(h, geo, sc.L) == want
    # every row is reported by the row that owns its window start
    for r, q in zip(h["row"].tolist(), h["q"].tolist()):
        assert q < geo[r][3]
    _sets, ref_stats = V.allele_sets(sc.text(), sc.records)
    ref_stats["dropped"]["no_row"] = 1  # the variant on the contig shorter than a window: applied to nothing
    ref_stats["applied"] -= 1
    assert stats == ref_stats
    d = stats["dropped"]
    assert d["ref_n"] == 2 and d["ref_mismatch"] == 2 and d["alt_is_ref"] == 3 and d["not_snv"] == 2 and d["unknown_contig"] == 1 and d["out_of_contig"] == 1


def test_placed_rows_read_as_designed():
    """The rows themselves, not only their equality: the PAM-creating ALT sets exactly the PAM's bit and leaves the spacer
    REF's; the rescued window reports max_mm mismatches; two ALTs at one position resolve to the guide's."""
    sc = V.standard_scene("NGG", 20, False, 2)
    h, _stats, geo = _twin(sc, 2)
    rows = {(g, c, p, s): (mm, w, a) for g, c, p, s, mm, w, a in V.rows_as_tuples(h, geo, sc.L)}
    for tag in "+-":
        mm, w, a = rows[sc.placed["pam_created" + tag]]
        assert (mm, w, a) == (0, sc.window(0), 1 << 21)
        mm, w, a = rows[sc.placed["mm_rescued" + tag]]
        assert mm == 2 and a == 1 << 3
        mm, w, a = rows[sc.placed["two_alts" + tag]]
        assert (mm, w, a) == (0, sc.window(5), 1 << 6)
        mm, w, a = rows[sc.placed["three_in_window" + tag]]
        assert (mm, a) == (0, (1 << 1) | (1 << 9) | (1 << 15))
        mm, w, a = rows[sc.placed["window_ends" + tag]]
        assert (mm, w, a) == (0, sc.window(6), 1 | (1 << 22))
        mm, w, a = rows[sc.placed["beside_n" + tag]]
        assert mm == 1 and w[12] == "N" and a == 1 << 13
        mm, w, a = rows[sc.placed["pam_n_and_spacer" + tag]]
        assert a == 1 << 4 and w[20] == "T"  # the N of NGG keeps REF's base although an ALT lies under it


def test_no_variants_no_rows_and_alt_zero_rows_are_not_listed():
    sc = V.standard_scene("NGG", 20, False, 4)
    h, stats, _geo = _twin(sc, 4, records=[])
    assert len(h["guide"]) == 0 and stats["applied"] == 0
    h, _stats, _geo = _twin(sc, 4)
    assert len(h["guide"]) and (h["alt"] != 0).all()


def test_variant_in_an_overlap_is_entered_in_both_rows_and_reported_once():
    sc = V.Scene("NGG", 20, False, 11)
    g = sc.guides[0]
    # window start 1020 is owned by row 0 (piece 1024); its variant at 1030 also lies in row 1
    sc.place("overlap", "chr1", 1020, 0, 0, {sc.sp(10): sc.other(g[10])}, {sc.sp(10): g[10]})
    contigs = sc.text()
    lens = {k: len(v) for k, v in contigs.items()}
    geo = row_geometry(lens, 20, 3, V.PIECE, 0, 20)
    row, q, _rb, _ab, var, _dropped, kept = variant_entries(lens, geo, variant_records(sc.records))
    assert sorted(zip(row.tolist(), q.tolist())) == [(0, 1030), (1, 6)] and var.tolist() == [0, 0] and len(kept) == 1
    h, stats, _geo = _twin(sc, 0)
    assert stats["applied"] == 1
    mine = [(r, qq) for gi, r, qq in zip(h["guide"].tolist(), h["row"].tolist(), h["q"].tolist()) if gi == 0]
    assert mine == [(0, 1020)]
    assert V.rows_as_tuples(h, geo, 23) == V.brute(contigs, sc.records, sc.guides, "NGG", False, 0)


def test_random_genomes():
    import random
    rng = random.Random(77)
    for pam_text, G, right in SYSTEMS:
        sc = V.Scene(pam_text, G, right, rng.randrange(1 << 30), lengths=(1500, 1100), n_guides=12)
        # guides cut from the genome so that near-matches exist, then one variant per ~15 bases, some with a wrong REF
        text = sc.text()
        for k in range(12):
            name = rng.choice(list(text))
            s = rng.randrange(len(text[name]) - sc.L)
            w = text[name][s + (sc.P if right else 0):][:G]
            sc.guides[k] = V.revcomp(w) if k & 1 else w
        for name, seq in text.items():
            for pos in range(len(seq)):
                if rng.randrange(15) == 0:
                    ref = seq[pos] if rng.randrange(10) else rng.choice("ACGT")
                    sc.records.append((name, pos, ref, rng.choice(("A", "C", "G", "T", "A,G", "C,T"))))
        for max_mm in (1, 3):
            h, stats, geo = _twin(sc, max_mm)
            assert V.rows_as_tuples(h, geo, sc.L) == V.brute(text, sc.records, sc.guides, pam_text, right, max_mm)
            assert stats == V.allele_sets(text, sc.records)[1]


# ---- the scenes of the device's seam tests (test_gpu_offtarget_variant_seams.py), held here to the brute force without a device: a
# scene that does not hold what it says, or a reference that is wrong, fails on a machine without a GPU --------------------------
def _hold(sc, max_mm, piece, guides=None):
    """the twin's rows of a seam scene == the brute force's, after the brute force and sites() were held to the scene's claims"""
    contigs = sc.text()
    want = sc.brute(max_mm, guides)
    V.check_claims(sc, want, max_mm, None if guides is None else len(guides))
    st = sc.sites()
    assert all((c, p, s) in st for _g, c, p, s, _mm, _w, _a in want)  # a row's window bears the PAM and holds an ALT
    h, stats = host_variant_scan(contigs, sc.G, sc.P, piece, sc.records, sc.guides if guides is None else guides,
                                 V.make_pam(sc.pam_text, sc.right), sc.right, max_mm)
    geo = row_geometry({k: len(v) for k, v in contigs.items()}, sc.G, sc.P, piece, 0, sc.G)
    assert V.rows_as_tuples(h, geo, sc.L) == want
    assert len(V.owned(st, geo)) == len(st)  # every window start that lies in its contig is owned by exactly one row
    return want, stats, geo


@pytest.mark.parametrize("pam_text,G,right", V.WINDOW_SYSTEMS)
@pytest.mark.parametrize("mm_hi", (False, True))
def test_window_length_scenes(pam_text, G, right, mm_hi):
    sc = V.window_scene(pam_text, G, right)
    max_mm = 0 if not mm_hi else 1 if G == 6 else 2
    want, stats, _geo = _hold(sc, max_mm, V.PIECE)
    assert {s for _g, _c, _p, s, *_r in want} == {0, 1} and len(want) >= len(sc.want)
    assert stats == V.allele_sets(sc.text(), sc.records)[1]
    L = sc.L
    if L == 32:
        assert sc.want["w0_31+"][2] == sc.want["w0_31-"][2] == 0x80000001
    assert {sc.want[f"w{i}+"][2] for i in (0, L - 1)} == {1, 1 << (L - 1)}


@pytest.mark.parametrize("pam_text,G,right,alphabet", V.SEAM_SYSTEMS)
def test_filter_seam_scene(pam_text, G, right, alphabet):
    from collections import Counter
    sc = V.seam_scene(pam_text, G, right, alphabet)
    want, stats, geo = _hold(sc, 0, V.BIG_PIECE)
    assert len(geo) == 8 and stats["applied"] == len(sc.records)
    L = sc.L
    for B in V.SEAMS:  # where the seam windows and their ALTs lie
        for tag in "+-":
            assert sc.placed[f"far{B}{tag}"][2] == B - 1 and sc.placed[f"across{B}{tag}"][2] + L - 1 == B
            assert sc.placed[f"after{B}{tag}"][2] + L == B and sc.placed[f"before{B}{tag}"][2] == B + 1
        assert sc.want[f"far{B}+"][2] == 1 << (L - 1) and sc.want[f"far{B}-"][2] == 1
    assert len(sc.absent) == 16
    cells = Counter((r, q // V.TILE, s) for r, q, s in V.owned(sc.sites(), geo))
    assert len(cells) == 32 and len(set(cells.values())) == 32  # every (row, workgroup, strand) holds its own number of sites
    assert Counter((r, q // V.TILE, s) for r, q, s in V.owned([(c, p, s) for _g, c, p, s, *_r in want], geo)).keys() == cells.keys()


@pytest.mark.parametrize("pam_text,G,right", SYSTEMS)
@pytest.mark.parametrize("n", (1285, 8197))
def test_row_end_scenes(pam_text, G, right, n):
    for strand in (0, 1):
        sc = V.row_end_scene(pam_text, G, right, n, strand)
        assert n % 128 == 5 and sc.placed["end"][2:] == (n - sc.L, strand)
        (ref, alt), = [(r, a) for c, p, r, a in sc.records if p == n - 1]
        assert ref != alt and sc.text()["chr1"][n - 1] == ref
        _want, _stats, geo = _hold(sc, 1, V.BIG_PIECE)
        assert len(geo) == 1


def test_dense_scene():
    sc = V.dense_scene()
    n, run = V.DENSE_N, V.DENSE_RUN
    sets, ref_stats = V.allele_sets(sc.text(), sc.records)
    assert (n - run) % 32 == 20 and all(len(a) == 4 for a in sets["chr1"][n - run:]) and len(sc.records) - run > 256
    want, stats, _geo = _hold(sc, 0, V.BIG_PIECE)
    assert stats == ref_stats and stats["dropped"]["ref_mismatch"] > 10
    V.dense_claims(sc, want)
    assert len(want) >= 2 * (run - sc.L + 1) * len(sc.guides)
    _hold(sc, 1, V.BIG_PIECE, guides=sc.guides[:40])


@pytest.mark.parametrize("max_mm", (0, 1))
def test_pam_detail_scenes(max_mm):
    sc = V.pam_lowest_scene()
    _hold(sc, max_mm, V.PIECE)
    assert {w[3] for _mm, w, _a in sc.want.values()} == {"A", "C"}
    for letters in ("AG", "CG"):  # the - strand records state the complements: their lowest + strand letter is the other one
        (alts,) = [a for c, p, r, a in sc.records if p == sc.placed[letters + "-"][2] + sc.L - 1 - 3]
        assert sorted(alts.split(",")) == sorted(V.COMP[x] for x in letters) and V.COMP[min(alts.split(","))] != min(letters)
    sc = V.pam_n_scene()
    want, _stats, _geo = _hold(sc, max_mm, V.PIECE)
    have = {(g, c, p, s): w for g, c, p, s, _mm, w, _a in want}
    for tag in "+-":
        assert have[sc.placed["under_pam_n" + tag]][20] == "N"
        assert (sc.placed["spacer_n" + tag] in have) == (max_mm >= 1)
        assert sc.placed["spacer_n" + tag][1:] in sc.sites()  # a site at either max_mm: only the pair is out of reach


def test_incremental_and_shard_scene():
    """The records dealt into three calls are the records; of three shards over the six rows two hold the overlap's variant"""
    sc = V.shard_scene()
    want, _stats, geo = _hold(sc, 2, V.PIECE)
    calls = V.split_calls(sc.records)
    flat = [r for c in calls for r in c]
    assert sorted(flat) == sorted(variant_records(sc.records)) and all(len(c) > 10 for c in calls)
    for tag in "+-":  # the two ALTs of one position lie in different calls
        _gi, contig, pos, strand = sc.placed["two_alts" + tag]
        at = pos + (sc.L - 1 - 6 if strand else 6)
        assert sorted(sum((contig, at) == r[:2] for r in c) for c in calls) == [0, 1, 1]
    assert V.brute(sc.text(), flat, sc.guides, "NGG", False, 2) == want
    lens = {k: len(v) for k, v in sc.text().items()}
    assert len(geo) == 6
    gi, contig, pos, strand = sc.placed["shard_overlap"]
    rec = [r for r in variant_records(sc.records) if r[:2] == (contig, pos + 10)]
    assert len(rec) == 1
    for r, (lo, hi) in enumerate(((0, 2), (2, 4), (4, 6))):
        row, q, _rb, _ab, _var, dropped, kept = variant_entries(lens, geo, rec, lo, hi)
        assert (row.tolist(), q.tolist(), dropped["other_shard"]) == (([1], [pos + 10 - 1024], 0), ([0], [pos + 10 - 2048], 0), ([], [], 1))[r]


def test_refusals():
    import ctypes as C
    L = _lib.lib()
    n = C.c_uint64(0)
    par = _lib.OtParams(0x0F44, 0, 3, 20, 0, 2)
    assert L.hawk_host_offtarget_variant_scan(None, None, 0, None, None, None, None, None, None, C.c_uint64(0), None, None, None, 0,
                                              None, None, None, None, None, None, None, None, C.c_uint64(0), C.byref(n)) == _lib.HAWK_E_INVALID
    assert L.hawk_host_offtarget_variant_scan(None, None, 0, None, None, None, None, None, None, C.c_uint64(0), None, C.byref(par), None, 0,
                                              None, None, None, None, None, None, None, None, C.c_uint64(0), C.byref(n)) == _lib.HAWK_OK
    wide = _lib.OtParams(0x0F44, 0, 3, 30, 0, 2)
    assert L.hawk_host_offtarget_variant_scan(None, None, 0, None, None, None, None, None, None, C.c_uint64(0), None, C.byref(wide), None, 0,
                                              None, None, None, None, None, None, None, None, C.c_uint64(0), C.byref(n)) == _lib.HAWK_E_UNSUPPORTED
    # a variant entry outside its row
    seq_off = np.array([0, 40], np.uint64)
    ss, se = np.zeros(1, np.int32), np.array([18], np.int32)
    row, q, b = np.zeros(1, np.uint32), np.array([40], np.uint32), np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hawk_host_offtarget_variant_scan(b"A" * 40, p(seq_off), 1, p(ss), p(se), p(row), p(q), p(b), p(b), C.c_uint64(1), None, C.byref(par), None, 0,
                                              None, None, None, None, None, None, None, None, C.c_uint64(0), C.byref(n)) == _lib.HAWK_E_INVALID


def test_exports_and_header():
    text = open(os.path.join(ROOT, "include", "hawk.h")).read()
    for sym in ("hawk_genome_variants", "hawk_offtarget_variant_scan", "hawk_host_offtarget_variant_scan"):
        assert f"int {sym}(" in text and sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)


def test_check_program_builds_and_passes(tmp_path):
    """csrc/otvar_check_main.cpp: the twin against a restatement on letters, as a program of its own (no Python, no device)"""
    csrc = os.path.join(ROOT, "crispr-hawk_amd", "csrc")
    exe = str(tmp_path / "otvar_check")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++17", "-o", exe, os.path.join(csrc, "otvar_check_main.cpp"),
                           os.path.join(csrc, "hawk_hostutil.hip"), "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "otvar_check: ok" in out.stdout, out.stderr
