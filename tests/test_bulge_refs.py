"""The shift-vector statement of the bulged-site selection (tests/bulge_refs.py - what k_ot_bulge computes, on Python ints) held to
the oracle's brute force over every placement (oracle.offtargets_bulges); no device."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bulge_refs as br
from oracle import oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_rows(genome, guides, pam, right, max_mm, bdna, brna):
    return sorted((int(r["guide"]), int(r["strand"]), int(r["pos"]), int(r["mm"]), int(r["btype"]), int(r["bsize"]), int(r["gaps"]))
                  for r in ora.offtargets_bulges(genome, guides, pam, right, max_mm, bdna, brna))


def _oracle_pair(site, guide, b, dna, max_mm):
    """the oracle's row of one (site spacer, guide) pair: the site as a contig of its own, NGG behind it, + strand"""
    rows = [r for r in _oracle_rows(site + "TGG", [guide], "NGG", False, max_mm, b if dna else 0, 0 if dna else b)
            if r[1] == 0 and r[2] == 0 and r[5] == b]
    assert len(rows) <= 1
    return (rows[0][3], rows[0][6]) if rows else None


def _genome(rng, guides, pam_s, right, n, max_mm, n_amb):
    """random sequence with sites of every kind planted for every guide, both strands, and a few ambiguous bases - some inside
    planted sites"""
    g = list(br.random_seq(rng, n))
    slots = rng.choice(n // 48 - 1, size=len(guides) * 8, replace=False).tolist()
    for k, slot in enumerate(slots):
        kind, b = (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))[k % 4]
        sp = br.mutate(rng, guides[k // 8], kind, b, int(rng.integers(0, max_mm + 1)))
        br.place(g, 48 * slot + int(rng.integers(0, 12)), sp, br.CONCRETE[pam_s], right, bool(k // 4 % 2))
    for p in rng.integers(0, n, size=n_amb).tolist():
        g[p] = "NRYK"[p % 4]
    return "".join(g)


@pytest.mark.parametrize("pam_s,G,right,n", [("NGG", 20, False, 4200), ("TTTV", 23, True, 20_000)])  # TTTV is the rarer PAM
@pytest.mark.parametrize("max_mm", [0, 2, 4])
def test_formula_matches_bruteforce_and_prune_loses_nothing(pam_s, G, right, n, max_mm):
    """Both types, b = 1 and 2, both strands, either PAM side, planted sites with mismatches, a guide with a homopolymer run
    (ties), ambiguous bases in and around sites: the ascending walk over the shift vectors and the one-pass form of otb_best give
    exactly the oracle's rows, and no pair the prune rejects has a row - over more than 10^4 pairs."""
    rng = np.random.default_rng(1000 + G + max_mm)
    guides = [br.random_seq(rng, G) for _ in range(6)]
    guides[1] = guides[1][:6] + "AAAA" + guides[1][10:]
    guides[2] = guides[2][:3] + "CC" + guides[2][5:12] + "GGG" + guides[2][15:]
    genome = _genome(rng, guides, pam_s, right, n, max_mm, n // 70)
    want = _oracle_rows(genome, guides, pam_s, right, max_mm, 2, 2)
    rows, pruned, pairs = br.bulge_rows(genome, guides, pam_s, right, max_mm, 2, 2)
    assert pairs >= 10_000 and len(want) > 30 and {(r[4], r[5]) for r in want} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert sorted(rows) == want
    assert sorted(br.bulge_rows(genome, guides, pam_s, right, max_mm, 2, 2, best=br.best_placement_onepass)[0]) == want
    assert len(pruned) > pairs // 2  # the prune does the bulk of the rejecting ...
    assert not pruned & {(r[0], r[1], r[2], r[4], r[5]) for r in want}  # ... and never rejects a pair that has a row


@functools.lru_cache(maxsize=None)
def _near_pairs():
    """1500 pairs that are close to matching (a guide mutated and bulged, so that many placements are near the minimum), each
    with the oracle's row: (site, guide, b, dna, max_mm, row or None)"""
    rng = np.random.default_rng(77)
    out = []
    for it in range(1500):
        G = int(rng.integers(5, 31))
        guide = br.random_seq(rng, G)
        if it % 3 == 0:  # runs of equal bases: ties
            guide = "".join(c for c in guide[:(G + 1) // 2] for _ in range(2))[:G]
        kind, b = (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))[it % 4]
        max_mm = int(rng.integers(0, 5))
        site = list(br.mutate(rng, guide, kind, b, int(rng.integers(0, min(G, max_mm + 2)))))
        if it % 5 == 0:
            site[int(rng.integers(0, len(site)))] = "N"
        site = "".join(site)
        out.append((site, guide, b, kind == "DNA", max_mm, _oracle_pair(site, guide, b, kind == "DNA", max_mm)))
    return out


def test_pairs_near_a_guide_one_by_one():
    """Pairs that are close to matching (a guide mutated and bulged, so that many placements are near the minimum), with and
    without the prune, against the oracle pair by pair."""
    n_rows = 0
    for site, guide, b, dna, max_mm, want in _near_pairs():
        assert br.best_placement(site, guide, b, dna, max_mm) == want
        assert br.best_placement(site, guide, b, dna, max_mm, use_prune=False) == want
        assert br.best_placement_onepass(site, guide, b, dna, max_mm) == want
        n_rows += want is not None
    assert n_rows > 700


def test_ties_go_to_the_smallest_positions():
    guide = "ACGTCG" + "AAAA" + "CGTACGTCAG"  # a run at positions 6..9
    for dna, site, gaps in ((False, guide[:6] + "AAA" + guide[10:], 1 << 6), (True, guide[:6] + "AAAAA" + guide[10:], 1 << 6),
                            (False, guide[:6] + "AA" + guide[10:], (1 << 6) | (1 << 7)), (True, guide[:6] + "AAAAAA" + guide[10:], (1 << 6) | (1 << 7))):
        b = abs(len(site) - len(guide))
        assert br.best_placement(site, guide, b, dna, 0) == (0, gaps) == _oracle_pair(site, guide, b, dna, 0)
        assert br.best_placement_onepass(site, guide, b, dna, 0) == (0, gaps)


def test_ambiguous_bases_aligned_and_at_a_bulge():
    guide = "ACGTCGATGCATCGTACGTC"
    # aligned: one mismatch
    site = guide[:9] + "T" + guide[9:]
    site_n = site[:3] + "N" + site[4:]
    assert br.best_placement(site, guide, 1, True, 1) == (0, 1 << 9)
    assert br.best_placement(site_n, guide, 1, True, 1) == (1, 1 << 9) == _oracle_pair(site_n, guide, 1, True, 1)
    assert br.best_placement(site_n, guide, 1, True, 0) is None and _oracle_pair(site_n, guide, 1, True, 0) is None
    # at the bulge: an ambiguous base is never bulged out, so the neighbouring placement wins (the N then faces a guide base) ...
    site_b = guide[:9] + "N" + guide[9:]
    got = br.best_placement(site_b, guide, 1, True, 2)
    assert got == _oracle_pair(site_b, guide, 1, True, 2) and got is not None and got[0] >= 1 and not (got[1] >> 9) & 1
    site_b2 = site_b[:16] + "T" + site_b[16:]
    got2 = br.best_placement_onepass(site_b2, guide, 2, True, 4)
    assert got2 == _oracle_pair(site_b2, guide, 2, True, 4) == br.best_placement(site_b2, guide, 2, True, 4) and got2 is not None and not (got2[1] >> 9) & 1
    # ... or the site vanishes
    assert br.best_placement(site_b, guide, 1, True, 0) is None and _oracle_pair(site_b, guide, 1, True, 0) is None


@pytest.mark.parametrize("dna", [True, False])
@pytest.mark.parametrize("b", [1, 2])
def test_bulges_at_the_ends_are_no_placements(dna, b):
    """A site whose only exact fit needs a bulge at position 0 or span - 1: absent, or reported with its interior best."""
    guide = "ACGTCGATGCATCGTACGTC"
    for front in (True, False):
        if dna:
            site = ("T" * b + guide) if front else (guide + "A" * b)
        else:
            site = guide[b:] if front else guide[:-b]
        span = max(len(site), len(guide))
        for max_mm in (0, 3, 12):
            got = br.best_placement(site, guide, b, dna, max_mm)
            assert got == _oracle_pair(site, guide, b, dna, max_mm) == br.best_placement_onepass(site, guide, b, dna, max_mm)
            if max_mm == 0:
                assert got is None
            if got is not None:
                assert got[0] > 0 and not got[1] & 1 and not (got[1] >> (span - 1)) & 1
    assert br.best_placement(guide[:1] + "T" * b + guide[1:], guide, b, True, 0) is not None  # the same bases one position in: a row


# ---- the wave queue of k_ot_bulge: which panels fill it ------------------------------------------------------------------------------
def test_vectorised_sites_and_prune_match_the_plain_ones():
    """bulge_refs.sites_np / prune_survivors (what the queue walk is built on) against sites / prune_floor(shift_vectors)"""
    rng = np.random.default_rng(3)
    g = list(br.random_seq(rng, 1400))
    for p in rng.integers(0, len(g), size=25).tolist():
        g[p] = "NRYK"[p % 4]
    g = "".join(g)
    for pam, right, spacer in (("NGG", False, 21), ("NGG", True, 19), ("TTTV", True, 18), ("TTTV", False, 24), ("NNGRRT", False, 22)):
        assert br.sites_np(g, pam, right, spacer) == list(br.sites(g, pam, right, spacer)) != []
    guides = [br.random_seq(rng, 20) for _ in range(40)]
    for dna, b in ((True, 1), (True, 2), (False, 1), (False, 2)):
        sp = [s for _w, _st, s in br.sites_np(g, "NGG", False, 20 + b if dna else 20 - b)]
        sp += [br.mutate(rng, guides[k % 40], "DNA" if dna else "RNA", b, k % 4) for k in range(80)]
        for max_mm in (0, 2, 9):
            keep = br.prune_survivors(sp, guides, b, dna, max_mm)
            want = [[br.prune_floor(br.shift_vectors(s, gd, b, dna)) <= max_mm for gd in guides] for s in sp]
            assert keep.tolist() == want and (max_mm == 9 or 0 < keep.sum() < keep.size)


def test_queue_walk_on_a_hand_made_case():
    """8 sites a wave, 3 guides a chunk: survivors 5, 5 | 8 (flush, 2 left; flush, 2 left) ... counted by hand"""
    guide = "ACGTCGATGCATCGTACGTC"
    near = guide[:9] + guide[10:]               # RNA bulge of 1, no mismatch
    far = "T" * 19
    sites = [near] * 5 + [far] * 3 + [near] * 8 + [near] * 2  # waves of 8: 5, 8 and 2 survivors per matching guide
    other = "GTCAGTCAGTCAGTCAGTCA"
    q = br.queue_walk(sites, [guide, guide, other, guide, other], 1, False, 0, wave=8, chunk=3)
    # wave 0: chunk 0: 5, 10 -> flush, 2 left; chunk 1: 5.  wave 1: 8 -> flush, 0 left, twice; chunk 1: once.  wave 2: 2, 4; 2
    assert (q["flushes"], q["flush_zero"], q["flush_rest"], q["peak"], q["carried"]) == (4, 3, 1, 10, 2)
    assert q["remainders"] == [(0, 0, 2), (0, 1, 5), (1, 0, 0), (1, 1, 0), (2, 0, 4), (2, 1, 2)]


def test_dense_panels_fill_the_wave_queue_and_the_older_panels_never_do():
    """The conditions tests/test_gpu_offtarget_bulges.py puts on its dense panels, without a device - and what those panels add:
    over the inputs of the parameter sweep and of the guide chunk seam no queue of any wave ever holds 64 pairs."""
    guides, contigs, fam_a, fam_b = br.dense_panel()
    assert len(guides) == 1100 and len(fam_a) > 80 and len(fam_b) > 25
    br.assert_queue_is_exercised(br.queue_figures(contigs, guides, "NGG", False, 2, 2, 2))
    guides, contigs = br.every_pair_panel()
    for q in br.queue_figures(contigs, guides, "NGG", False, 20, 1, 1).values():
        assert q["sites"] > 64 and q["flush_zero"] >= len(guides) * (q["sites"] // 64)
    import test_gpu_offtarget_bulges as tg
    old = [(tg._sweep_inputs(pam_s, G, right, max_mm, bdna, brna), pam_s, right, max_mm, bdna, brna)
           for pam_s, G, right in tg._SWEEP["pams"] for max_mm in tg._SWEEP["max_mm"] for bdna, brna in tg._SWEEP["bulges"]]
    old += [(tg._seam_inputs(n), "NGG", False, 2, 1, 0) for n in tg._SEAM_COUNTS]
    assert len(old) == 21
    for (guides, contigs), pam_s, right, max_mm, bdna, brna in old:
        figures = br.queue_figures(contigs, guides, pam_s, right, max_mm, bdna, brna)
        assert len(figures) == min(bdna, 2) + min(brna, 2) and all(q["sites"] > 64 for q in figures.values())
        assert [q["flushes"] for q in figures.values()] == [0] * len(figures)


# ---- otb_best as the compiler builds it (csrc/hawk_otbulge.h through csrc/otbulge_check_main.cpp) -------------------------------------
def _spread(v: int) -> int:
    """bit j -> bit 2 j: the header's layout"""
    return sum(1 << (2 * j) for j in range(v.bit_length()) if (v >> j) & 1)


def test_otb_best_as_compiled(tmp_path):
    """hawk_otbulge.h compiled for the host: the program's own exhaustive comparison with a plain walk, then otb_best's answers for
    the shift vectors of the 1500 near pairs and of 400 more with guides of 28..31 bases (spans up to 32, which no DNA bulge of 2
    reaches on the device) held to the oracle pair by pair."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))
    if cxx is None:
        pytest.skip("no host C++ compiler: neither g++ nor clang++ (PATH, ROCm's llvm/bin) is there")
    src = os.path.join(ROOT, "crispr-hawk_amd", "csrc", "otbulge_check_main.cpp")
    exe = str(tmp_path / "otbulge_check")
    subprocess.run([cxx, "-O2", "-march=native", "-std=c++17", "-pthread", "-o", exe, src], check=True)
    done = subprocess.run([exe, "exhaust"], capture_output=True, text=True)
    assert done.returncode == 0 and "random 1000000 cases" in done.stdout, done.stdout[-2000:]
    pairs = list(_near_pairs())
    rng = np.random.default_rng(2831)
    for it in range(400):
        kind, b = (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))[it % 4]
        G = int(rng.integers(28, 32 - b + 1 if kind == "DNA" else 32))  # span = G + b (DNA) or G (RNA) <= 32
        guide = br.random_seq(rng, G)
        if it % 3 == 0:
            guide = "".join(c for c in guide[:(G + 1) // 2] for _ in range(2))[:G]
        max_mm = int(rng.integers(0, 5))
        site = list(br.mutate(rng, guide, kind, b, int(rng.integers(0, max_mm + 2))))
        if it % 5 == 0:
            site[int(rng.integers(0, len(site)))] = "N"
        site = "".join(site)
        pairs.append((site, guide, b, kind == "DNA", max_mm, _oracle_pair(site, guide, b, kind == "DNA", max_mm)))
    assert {max(len(s), len(g)) for s, g, *_ in pairs[1500:]} >= {29, 30, 31, 32}
    lines = []
    for site, guide, b, dna, max_mm, _want in pairs:
        m = br.shift_vectors(site, guide, b, dna)
        lines.append(" ".join(str(v) for v in [b, max(len(site), len(guide)), br.encode(site)[1] if dna else 0, max_mm] + [_spread(v) for v in m]))
    done = subprocess.run([exe, "cases"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = [tuple(int(v) for v in ln.split()) for ln in done.stdout.splitlines()]
    assert len(got) == len(pairs)
    n_rows = 0
    for (site, guide, b, dna, max_mm, want), (mm, gaps) in zip(pairs, got):
        assert (mm, gaps) == want if want is not None else mm > max_mm, (site, guide, b, dna, max_mm, want, mm, gaps)
        n_rows += want is not None
    assert n_rows > 900 and sum(w is not None for *_x, w in pairs[1500:]) > 150


def test_new_export_is_listed_and_declared():
    from crisprhawk_hip import _lib
    assert "hawk_offtarget_bulges" in _lib.EXPORTS
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hawk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hawk_offtarget_bulges\s*\(", text)
