"""The shift-vector statement of the bulged-site selection (tests/bulge_refs.py - what k_ot_bulge computes, on Python ints) held to
the oracle's brute force over every placement (oracle.offtargets_bulges); no device."""
import os
import re

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


def test_pairs_near_a_guide_one_by_one():
    """Pairs that are close to matching (a guide mutated and bulged, so that many placements are near the minimum), with and
    without the prune, against the oracle pair by pair."""
    rng = np.random.default_rng(77)
    n_rows = 0
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
        want = _oracle_pair(site, guide, b, kind == "DNA", max_mm)
        assert br.best_placement(site, guide, b, kind == "DNA", max_mm) == want
        assert br.best_placement(site, guide, b, kind == "DNA", max_mm, use_prune=False) == want
        assert br.best_placement_onepass(site, guide, b, kind == "DNA", max_mm) == want
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


def test_new_export_is_listed_and_declared():
    from crisprhawk_hip import _lib
    assert "hawk_offtarget_bulges" in _lib.EXPORTS
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hawk.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+hawk_offtarget_bulges\s*\(", text)
