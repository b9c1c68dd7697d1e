"""Bulged off-target sites selected on the device (GenomeIndex.scan_bulges(engine="device") -> hawk_offtarget_bulges -> k_ot_bulge)
against the oracle's brute force over every placement (oracle.offtargets_bulges; both unpinned to CRISPRitz, which is absent):
sorted tuples (guide, type, size, contig, position, strand, mm, gaps).  Small pieces, so windows cross row and tile seams; every
case plants bulged sites, so none is vacuous."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import bulge_refs as br
from crisprhawk_hip import _lib
from crisprhawk_hip.genome import GenomeIndex, decode_window, encode_guides
from crisprhawk_hip.hapset import _p
from crisprhawk_hip.pam import PAM
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

_ALL_KINDS = (("DNA", 1), ("DNA", 2), ("RNA", 1), ("RNA", 2))


def _pam(pam_s, right):
    pam = PAM(pam_s, right, True)
    pam.encode(0)
    return pam


def _want(contigs, guides, pam_s, right, max_mm, bdna, brna):
    ci = {n: i for i, n in enumerate(contigs)}
    rows = [(int(r["guide"]), "DNA" if r["btype"] == 1 else "RNA", int(r["bsize"]), name, int(r["pos"]), "-" if r["strand"] else "+",
             int(r["mm"]), int(r["gaps"])) for name, seq in contigs.items() for r in ora.offtargets_bulges(seq, guides, pam_s, right, max_mm, bdna, brna)]
    return sorted(rows, key=lambda t: (t[0], t[1], t[2], ci[t[3]], t[4], t[5] == "-"))


def _key(h):
    return (h.guide, h.bulge_type, h.bulge_size, h.contig, h.position, h.strand, h.mm, h.gaps)


def _kinds(bdna, brna):
    return [(k, b) for k, b in _ALL_KINDS if b <= (bdna if k == "DNA" else brna)]


def _planted_contigs(rng, guides, pam_s, right, lengths, kinds, max_mm, per=8, seams=()):
    """random contigs with `per` sites per (guide, kind) in slots of their own, both strands, 0 .. max_mm substitutions; `seams`:
    (contig, position) pairs a planted window is laid across"""
    P = br.CONCRETE[pam_s]
    contigs = {name: list(br.random_seq(rng, n)) for name, n in lengths}
    names = list(contigs)
    free = {name: rng.permutation(len(contigs[name]) // 64 - 1).tolist() for name in names}
    k = 0
    for gi, gd in enumerate(guides):
        for kind, b in kinds:
            for j in range(per):
                name = names[k % len(names)] if free[names[k % len(names)]] else max(names, key=lambda nm: len(free[nm]))
                sp = br.mutate(rng, gd, kind, b, int(rng.integers(0, max_mm + 1)))
                br.place(contigs[name], 64 * free[name].pop() + int(rng.integers(0, 20)), sp, P, right, bool(j % 2))
                k += 1
    for j, (name, at) in enumerate(seams):
        kind, b = kinds[j % len(kinds)]
        br.place(contigs[name], at - 3 - 5 * (j % 4), br.mutate(rng, guides[j % len(guides)], kind, b, 0), P, right, bool(j % 2))
    return {name: "".join(g) for name, g in contigs.items()}


# ---- the parameter sweep ---------------------------------------------------------------------------------------------------------
_SWEEP = dict(bulges=[(1, 0), (0, 1), (2, 2)], max_mm=[0, 2, 4], pams=[("NGG", 20, False), ("TTTV", 23, True)])


def _sweep_inputs(pam_s, G, right, max_mm, bdna, brna):
    """(guides, contigs) of one case of the sweep (tests/test_bulge_refs.py walks the wave queue over the same inputs)"""
    rng = np.random.default_rng(500 + G + 10 * max_mm + bdna + 3 * brna)
    guides = [br.random_seq(rng, G) for _ in range(5)]
    guides[1] = guides[1][:6] + "AAAA" + guides[1][10:]
    contigs = _planted_contigs(rng, guides, pam_s, right, (("c1", 30_000), ("c2", 9_001)), _kinds(bdna, brna), max_mm,
                               seams=(("c1", 4096), ("c1", 8192), ("c1", 12288), ("c2", 4096), ("c2", 8192)))
    g = list(contigs["c1"])
    for p in rng.integers(0, len(g), size=15).tolist():
        g[p] = "NRY"[p % 3]
    contigs["c1"] = "".join(g)
    return guides, contigs


@pytest.mark.parametrize("bdna,brna", _SWEEP["bulges"])
@pytest.mark.parametrize("max_mm", _SWEEP["max_mm"])
@pytest.mark.parametrize("pam_s,G,right", _SWEEP["pams"])
def test_device_engine_matches_bruteforce_and_derived(pam_s, G, right, max_mm, bdna, brna):
    """~40 kb over two contigs in pieces of 4096, 5 guides (one with a run of equal bases): the device engine's rows are the brute
    force's, and equal the derived engine's row for row, every BulgeHit field included."""
    guides, contigs = _sweep_inputs(pam_s, G, right, max_mm, bdna, brna)
    want = _want(contigs, guides, pam_s, right, max_mm, bdna, brna)
    assert len(want) > 30 and {(t[1], t[2]) for t in want} == set(_kinds(bdna, brna))
    pam = _pam(pam_s, right)
    idx = GenomeIndex(contigs, G, len(pam_s), piece=4096, max_bulge=bdna)
    got = idx.scan_bulges(guides, pam, right, max_mm, bdna, brna, engine="device")
    assert [_key(h) for h in got] == want
    assert got == idx.scan_bulges(guides, pam, right, max_mm, bdna, brna, engine="derived")
    # the scan ranges are put back: an un-bulged scan afterwards sees its own rows
    assert len(idx.scan(guides, pam, right, 0)) == sum(len(ora.offtargets(seq, guides, pam_s, right, 0)) for seq in contigs.values())
    with pytest.raises(ValueError, match="engine"):
        idx.scan_bulges(guides, pam, right, max_mm, bdna, brna, engine="host")


# ---- dense near-duplicate panels: the wave queue filled, flushed and carried ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense():
    """the dense family panel (bulge_refs.dense_panel), the queue figures of its four launches and the oracle's rows - once"""
    guides, contigs, fam_a, fam_b = br.dense_panel()
    figures = br.queue_figures(contigs, guides, "NGG", False, 2, 2, 2)
    return guides, contigs, fam_a, fam_b, figures, _want(contigs, guides, "NGG", False, 2, 2, 2)


@functools.lru_cache(maxsize=None)
def _dense_device():
    guides, contigs = _dense()[:2]
    idx = GenomeIndex(contigs, 20, 3, piece=1024, max_bulge=2)
    return idx, idx.scan_bulges(guides, _pam("NGG", False), False, 2, 2, 2, engine="device")


def test_dense_family_panels_fill_the_wave_queue():
    """Three tandem contigs of near-copies of two guides (+ strand, its reverse complement, one with more than 256 sites) against
    1100 guides that hold the two families: per guide of a family most lanes of a wave survive the prune, so the queue runs full,
    is flushed with and without a rest, and ends the first guide chunk partly filled - asserted on the queue's arithmetic before
    the device is asked.  The rows are the brute force's, none twice, and equal the derived engine's row for row - for the 117
    family guides and 15 others, since deriving all 1100 guides (3.3 million derived guides for DNA bulges of 2) takes the host
    alone ten seconds; the brute force covers all of them."""
    guides, contigs, fam_a, fam_b, figures, want = _dense()
    assert set(figures) == set(_ALL_KINDS)
    br.assert_queue_is_exercised(figures)
    assert all(q["sites"] > 2 * 256 and q["sites"] % 64 for q in figures.values())  # three workgroups, a partial last wave
    assert len(br.device_site_order({"c3": contigs["c3"]}, "NGG", False, 18)) > 256
    idx, got = _dense_device()
    keys = [_key(h) for h in got]
    assert keys == want and len(want) > 50_000
    assert len({k[:6] for k in keys}) == len(keys)
    sub = sorted(set(fam_a) | set(fam_b) | {0, 1, 2, 1098, 1099} | set(range(600, 610)))
    at = {gi: i for i, gi in enumerate(sub)}
    derived = idx.scan_bulges([guides[i] for i in sub], _pam("NGG", False), False, 2, 2, 2, engine="derived")
    assert [dataclasses.replace(h, guide=at[h.guide]) for h in got if h.guide in at] == derived != []


def test_family_rows_across_the_chunk_seam():
    """In the dense panel guide 1023 (the last of the first chunk) and 1024 (the first of the second) are one near-copy of A, and
    guides 0 and 1099 one guide: identical rows - a queue carried over the chunk change would meet the other chunk's guides."""
    guides, _contigs, fam_a, _fam_b, _figures, _want_rows = _dense()
    _idx, got = _dense_device()
    rows = lambda gi: [_key(h)[1:] + (h.crrna, h.dna, h.pam) for h in got if h.guide == gi]
    assert guides[1023] == guides[1024] and {1023, 1024} <= set(fam_a) and guides[0] == guides[1099]
    assert rows(1023) == rows(1024) and {t[:2] for t in rows(1023)} == set(_ALL_KINDS) and len(rows(1023)) > 100
    assert rows(0) == rows(1099) and {t[:2] for t in rows(0)} == set(_ALL_KINDS)


def test_every_pair_is_a_row():
    """max_mm = G = 20, bulges of 1: nothing is pruned, so every ballot is full, a full wave flushes on every one of the 70 guides
    and leaves 0, and every (site, guide) pair is a row - of both types: a DNA pair would drop out only if all 19 interior
    positions of its site were ambiguous, which three N cannot do; what they do is move the winning placement off themselves."""
    guides, contigs = br.every_pair_panel()
    G = 20
    figures = br.queue_figures(contigs, guides, "NGG", False, G, 1, 1)
    for q in figures.values():
        full = q["sites"] // 64
        assert full >= 1 and q["sites"] % 64 and q["flush_zero"] >= len(guides) * full
        assert all(rem == 0 for wv, _ch, rem in q["remainders"] if wv < full)
    want = _want(contigs, guides, "NGG", False, G, 1, 1)
    idx = GenomeIndex(contigs, G, 3, piece=1024, max_bulge=1)
    got = idx.scan_bulges(guides, _pam("NGG", False), False, G, 1, 1, engine="device")
    assert [_key(h) for h in got] == want
    for kind in ("DNA", "RNA"):
        assert sum(h.bulge_type == kind for h in got) == figures[(kind, 1)]["sites"] * len(guides)
    amb = [h for h in got if h.bulge_type == "DNA" and "N" in h.dna.upper()]
    assert len(amb) >= len(guides) and all(h.dna[h.crrna.index("-")] != "N" for h in amb)


@pytest.mark.parametrize("btype,bsize", [(1, 1), (2, 2)])
def test_capacity_contract_on_a_dense_panel(btype, bsize):
    """The row counter is bumped by the lane that verifies a queued pair, not by the site's own lane: on the dense panel cap one
    below the need returns HAWK_E_CAPACITY with the exact need - the brute force's row count - and the retry the rows of an
    ample run."""
    guides, contigs, _fam_a, _fam_b, _figures, want = _dense()
    pam = _pam("NGG", False)
    idx = GenomeIndex(contigs, 20, 3, piece=1024, max_bulge=2)
    idx._set_window(20 + bsize if btype == 1 else 20 - bsize)
    rc, need, rows = _raw(idx, guides, pam, False, 2, btype, bsize, 1 << 16)
    assert rc == _lib.HAWK_OK and need == len(rows) == sum(t[1:3] == ("DNA" if btype == 1 else "RNA", bsize) for t in want) > 5_000
    assert len({r[:4] for r in rows}) == need  # one row per (guide, site, strand)
    assert _raw(idx, guides, pam, False, 2, btype, bsize, need - 1) == (_lib.HAWK_E_CAPACITY, need, [])
    assert _raw(idx, guides, pam, False, 2, btype, bsize, need) == (_lib.HAWK_OK, need, rows)


# ---- single planted sites: placement edges, ties, the mismatch cut, ambiguity ------------------------------------------------------
_G20 = "ACGTCGATGCATCGTACGTC"  # no two equal neighbours: a planted bulge has no equally good neighbour placement


def _subst(s: str, p: int) -> str:
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + 2) % 4] + s[p + 1:]


def _single_sites(sites, max_mm, bdna=2, brna=2, guide=_G20, piece=1024):
    """each (site spacer, strand) planted 150 bases apart behind a seam-crossing start; returns (got, want, starts)"""
    rng = np.random.default_rng(len(sites) + max_mm)
    g = list(br.random_seq(rng, 1000 + 150 * len(sites) + 200))
    starts = []
    for k, (sp, minus) in enumerate(sites):
        starts.append(1000 + 150 * k)  # the first one lies across the seam at 1024
        br.place(g, starts[-1], sp, "TGG", False, minus)
    contigs = {"c": "".join(g)}
    idx = GenomeIndex(contigs, len(guide), 3, piece=piece, max_bulge=bdna)
    got = [_key(h) for h in idx.scan_bulges([guide], _pam("NGG", False), False, max_mm, bdna, brna, engine="device")]
    return got, _want(contigs, [guide], "NGG", False, max_mm, bdna, brna), starts


def test_placement_edges():
    """The best bulge at position 1, at span - 2, at an adjacent pair and at (1, span - 2), DNA and RNA, each with one mismatch
    elsewhere: reported with exactly the planted mm and gaps."""
    g, G = _G20, 20
    plan = [  # (kind, b, site spacer, gaps)
        ("DNA", 1, g[:1] + "T" + g[1:], 1 << 1),
        ("DNA", 1, g[:G - 1] + "A" + g[G - 1:], 1 << (G - 1)),                     # span = 21: position 19
        ("DNA", 2, g[:7] + "CG" + g[7:], (1 << 7) | (1 << 8)),
        ("DNA", 2, g[:1] + "T" + g[1:G - 1] + "A" + g[G - 1:], (1 << 1) | (1 << G)),  # span = 22: positions 1 and 20
        ("RNA", 1, g[:1] + g[2:], 1 << 1),
        ("RNA", 1, g[:G - 2] + g[G - 1:], 1 << (G - 2)),
        ("RNA", 2, g[:7] + g[9:], (1 << 7) | (1 << 8)),
        ("RNA", 2, g[:1] + g[2:G - 2] + g[G - 1:], (1 << 1) | (1 << (G - 2))),
    ]
    sites = [(_subst(sp, 4 if k % 2 else 12), bool(k % 2)) for k, (_kind, _b, sp, _gaps) in enumerate(plan)]
    got, want, starts = _single_sites(sites, 2)
    assert got == want and len(want) > 8
    for (kind, b, _sp, gaps), (_s, minus), at in zip(plan, sites, starts):
        assert (0, kind, b, "c", at, "-" if minus else "+", 1, gaps) in got


def test_ties_go_to_the_smallest_positions():
    """A site inside a run of equal bases where 4 (b = 1) or more placements tie: the smallest positions are reported."""
    guide = "ACGTCG" + "AAAA" + "CGTACGTCAG"  # the run: positions 6..9
    sites = [(guide[:6] + "AAA" + guide[10:], False), (guide[:6] + "AAAAA" + guide[10:], True), (guide[:6] + "AA" + guide[10:], True),
             (guide[:6] + "AAAAAA" + guide[10:], False)]
    got, want, starts = _single_sites(sites, 1, guide=guide)
    assert got == want
    for (kind, b, gaps), (_s, minus), at in zip((("RNA", 1, 1 << 6), ("DNA", 1, 1 << 6), ("RNA", 2, 3 << 6), ("DNA", 2, 3 << 6)), sites, starts):
        assert (0, kind, b, "c", at, "-" if minus else "+", 0, gaps) in got


def test_mismatch_cut():
    """mm == max_mm is reported; the same site with one more mismatch is not."""
    rna = _G20[:9] + _G20[10:]
    dna = _G20[:9] + "T" + _G20[9:]
    two = lambda s: _subst(_subst(s, 2), 15)
    sites = [(two(rna), False), (_subst(two(rna), 5), False), (two(dna), True), (_subst(two(dna), 5), True)]
    got, want, starts = _single_sites(sites, 2, bdna=1, brna=1)
    assert got == want
    at = {(t[1], t[4]): t for t in got}
    assert at[("RNA", starts[0])][6:] == (2, 1 << 9) and at[("DNA", starts[2])][6:] == (2, 1 << 9)
    assert ("RNA", starts[1]) not in at and ("DNA", starts[3]) not in at


def test_ambiguous_bases():
    """An aligned N counts one mismatch; an N at the otherwise best DNA bulge position is never bulged out: the next-best
    placement wins, or - at max_mm = 0 - the site vanishes."""
    dna = _G20[:9] + "T" + _G20[9:]
    sites = [(dna[:3] + "N" + dna[4:], False), (_G20[:9] + "N" + _G20[9:], False), (dna[:3] + "R" + dna[4:], True), (dna, False)]
    got, want, starts = _single_sites(sites, 2, bdna=1, brna=0)
    assert got == want
    at = {t[4]: t for t in got}
    assert at[starts[0]][6:] == (1, 1 << 9) and at[starts[2]][6:] == (1, 1 << 9) and at[starts[3]][6:] == (0, 1 << 9)
    assert at[starts[1]][6] >= 1 and not (at[starts[1]][7] >> 9) & 1
    got0, want0, _ = _single_sites(sites, 0, bdna=1, brna=0)
    assert got0 == want0 and {t[4] for t in got0} & set(starts) == {starts[3]}


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def test_window_cap_32_bases():
    """NGG, G = 27, bulges of 2: the DNA-bulged windows have 27 + 2 + 3 = 32 bases, the width of the window code; a contig that ends
    piece + one such window - 1 bases long.  One guide base more is refused by the index constructor."""
    rng = np.random.default_rng(27)
    G, max_mm = 27, 2
    guides = [br.random_seq(rng, G) for _ in range(3)]
    n2 = 1024 + 27 + 3 + 2 - 1
    contigs = _planted_contigs(rng, guides, "NGG", False, (("c1", 6000), ("c2", n2)), _ALL_KINDS, max_mm, per=4,
                               seams=(("c1", 1024), ("c1", 2048), ("c1", 3072), ("c1", 4096)))
    g = list(contigs["c2"])
    br.place(g, n2 - 32, br.mutate(rng, guides[0], "DNA", 2, 1), "AGG", False, False)  # the contig's last 32-base window: it starts one base in front of the seam
    contigs["c2"] = "".join(g)
    want = _want(contigs, guides, "NGG", False, max_mm, 2, 2)
    assert len(want) > 30 and {(t[1], t[2]) for t in want} == set(_ALL_KINDS) and any(t[1:5] == ("DNA", 2, "c2", n2 - 32) for t in want)
    idx = GenomeIndex(contigs, G, 3, piece=1024, max_bulge=2)
    assert [_key(h) for h in idx.scan_bulges(guides, _pam("NGG", False), False, max_mm, 2, 2, engine="device")] == want
    with pytest.raises(ValueError, match="32 bases"):
        GenomeIndex(contigs, G + 1, 3, max_bulge=2)


def _no_repeats(rng, n: int) -> str:
    """no two equal neighbours: a planted bulge has no equally good neighbour placement"""
    s = [int(rng.integers(0, 4))]
    while len(s) < n:
        s.append((s[-1] + int(rng.integers(1, 4))) % 4)
    return "".join("ACGT"[c] for c in s)


def _rna_gapped(g: str, *gaps: int) -> str:
    return "".join(c for i, c in enumerate(g) if i not in gaps)


@pytest.mark.parametrize("pam_s,G,right", [("NGG", 29, False), ("TTTV", 28, True)])
def test_rna_bulges_under_a_32_base_window(pam_s, G, right):
    """The widest guides an index takes: G + pamlen = 32 with max_bulge = 0, RNA bulges of 1 and 2 (n = G - 1, G - 2; span = G).
    Planted sites of both sizes on both strands and across piece seams, and on a contig of their own the gaps at position 1, at
    span - 2, at (1, 2), (1, span - 2) and (span / 2, span - 2), the first of them across the seam at 1024: the oracle's rows, the derived engine's
    rows, and the planted (mm, gaps) themselves."""
    rng = np.random.default_rng(G)
    max_mm, P = 2, len(pam_s)
    guides = [_no_repeats(rng, G) for _ in range(3)]
    contigs = _planted_contigs(rng, guides, pam_s, right, (("c1", 5000),), (("RNA", 1), ("RNA", 2)), max_mm, per=4,
                               seams=(("c1", 1024), ("c1", 2048), ("c1", 3072), ("c1", 4096)))
    plan = [(1, (1,)), (1, (G - 2,)), (2, (1, 2)), (2, (1, G - 2)), (2, (G // 2, G - 2))]
    e = list(br.random_seq(rng, 1024 + 150 * len(plan)))
    starts = [1010 + 150 * k for k in range(len(plan))]  # the first window lies across the seam at 1024
    for k, ((b, gaps), at) in enumerate(zip(plan, starts)):
        br.place(e, at, _rna_gapped(guides[0], *gaps), br.CONCRETE[pam_s], right, bool(k % 2))
    contigs["e"] = "".join(e)
    want = _want(contigs, guides, pam_s, right, max_mm, 0, 2)
    assert len(want) > 30 and {(t[1], t[2]) for t in want} == {("RNA", 1), ("RNA", 2)}
    for k, ((b, gaps), at) in enumerate(zip(plan, starts)):
        assert (0, "RNA", b, "e", at, "-" if k % 2 else "+", 0, sum(1 << p for p in gaps)) in want
    pam = _pam(pam_s, right)
    idx = GenomeIndex(contigs, G, P, piece=1024, max_bulge=0)
    assert idx.L == 32
    got = idx.scan_bulges(guides, pam, right, max_mm, 0, 2, engine="device")
    assert [_key(h) for h in got] == want
    assert got == idx.scan_bulges(guides, pam, right, max_mm, 0, 2, engine="derived")
    with pytest.raises(ValueError, match="32 bases"):
        GenomeIndex(contigs, G + 1, P)


def test_entry_accepts_guides_wider_than_the_index_does():
    """hawk_offtarget_bulges takes guides of up to 32 bases as long as the SITE's window has at most 32: guides of 31 bases with
    RNA bulges of 2 and of 30 bases with RNA bulges of 1, on an index built for windows of 29 + 3 bases - which GenomeIndex itself
    would not build for such guides.  Planted sites on both strands and across the seam; the returned columns, as (guide,
    contig position, strand, mm, gaps), are the oracle's rows for the 31- and 30-base guides (the oracle takes guides of up to
    60 bases), and every window column spells the contig's own bases."""
    rng = np.random.default_rng(31)
    pam = _pam("NGG", False)
    g = list(br.random_seq(rng, 4000))
    panels = []
    for G, b, first in ((31, 2, 1000), (30, 1, 2030)):
        guides = [_no_repeats(rng, G) for _ in range(3)]
        for k in range(9):  # 100 bases apart; the first window (32 bases) of either panel lies across a seam (1024, 2048)
            n_mm = k % 3
            br.place(g, first + 100 * k, br.mutate(rng, guides[k % 3], "RNA", b, n_mm), "TGG", False, bool(k % 2))
        # the gaps at the ends of the interior: positions 1 and span - 2 of the guide
        br.place(g, first + 930, _rna_gapped(guides[0], *((1, G - 2) if b == 2 else (1,))), "AGG", False, False)
        br.place(g, first + 980, _rna_gapped(guides[1], *((G // 2, G - 2) if b == 2 else (G - 2,))), "CGG", False, True)
        panels.append((G, b, guides, first))
    seq = "".join(g)
    wants = []
    for G, b, guides, first in panels:
        rows = [r for r in ora.offtargets_bulges(seq, guides, "NGG", False, 2, 0, b) if r["bsize"] == b]
        want = sorted((int(r["guide"]), int(r["pos"]), int(r["strand"]), int(r["mm"]), int(r["gaps"])) for r in rows)
        assert len(want) >= 11
        assert (0, first + 930, 0, 0, (1 << 1) | (1 << (G - 2)) if b == 2 else 1 << 1) in want
        assert (1, first + 980, 1, 0, (1 << (G // 2)) | (1 << (G - 2)) if b == 2 else 1 << (G - 2)) in want
        wants.append(want)
    idx = GenomeIndex({"c": seq}, 29, 3, piece=1024)
    idx._set_window(29)
    for (G, b, guides, first), want in zip(panels, wants):
        rc, n, got = _raw(idx, guides, pam, False, 2, 2, b, 4096, guidelen=G)
        assert rc == _lib.HAWK_OK and n == len(got)
        assert sorted((r[0], idx.rows[r[1]][1] + r[2], r[3], r[4], r[7]) for r in got) == want
        for r in got:
            at = idx.rows[r[1]][1] + r[2]
            assert decode_window(r[5], r[6], 32) == (br.revcomp(seq[at:at + 32]) if r[3] else seq[at:at + 32])


@pytest.mark.parametrize("max_mm", [0, 1])
@pytest.mark.parametrize("G,bmax", [(4, 1), (5, 2)])
def test_shortest_guides(G, bmax, max_mm):
    """G = b + 3, the shortest guides the entry takes (RNA: n = 3 paired positions, one to three interior gap positions), both
    types, on 1.5 kb of random sequence with a few ambiguous bases; G = b + 2 is refused."""
    rng = np.random.default_rng(40 + G)
    g = list(br.random_seq(rng, 1500))
    for p in rng.integers(0, len(g), size=6).tolist():
        g[p] = "NRY"[p % 3]
    contigs = {"c": "".join(g)}
    guides = [br.random_seq(rng, G) for _ in range(6)]
    want = _want(contigs, guides, "NGG", False, max_mm, bmax, bmax)
    assert len(want) > 20 and {(t[1], t[2]) for t in want} == set(_kinds(bmax, bmax))
    pam = _pam("NGG", False)
    idx = GenomeIndex(contigs, G, 3, piece=1024, max_bulge=bmax)
    assert [_key(h) for h in idx.scan_bulges(guides, pam, False, max_mm, bmax, bmax, engine="device")] == want
    if G == 4:
        with pytest.raises(ValueError, match="interior"):
            idx.scan_bulges(guides, pam, False, max_mm, 0, 2, engine="device")
        for btype in (1, 2):
            assert _raw(idx, guides, pam, False, max_mm, btype, 2, 64)[0] == _lib.HAWK_E_UNSUPPORTED                          # 4 = 2 + 2
            assert _raw(idx, [s[:3] for s in guides], pam, False, max_mm, btype, 1, 64, guidelen=3)[0] == _lib.HAWK_E_UNSUPPORTED  # 3 = 1 + 2


@pytest.mark.parametrize("b", [1, 2])
def test_rna_bulged_site_in_a_contig_tail(b):
    """A last piece of L - b bases, too short for an un-bulged window: the RNA-bulged site that fills it is found."""
    rng = np.random.default_rng(31 + b)
    G, P, piece = 20, 3, 1024
    guide = _G20
    site = guide[:9] + guide[9 + b:]
    contigs = {"tail": br.random_seq(rng, piece) + site + "AGG", "short": site + "TGG"}
    assert len(contigs["tail"]) == piece + G + P - b
    want = _want(contigs, [guide], "NGG", False, 1, 0, b)
    idx = GenomeIndex(contigs, G, P, piece=piece)
    got = [_key(h) for h in idx.scan_bulges([guide], _pam("NGG", False), False, 1, 0, b, engine="device")]
    assert got == want
    gaps = sum(1 << (9 + k) for k in range(b))
    assert (0, "RNA", b, "tail", piece, "+", 0, gaps) in got and (0, "RNA", b, "short", 0, "+", 0, gaps) in got


_SEAM_COUNTS = [1023, 1024, 1025]


def _seam_inputs(n_guides):
    rng = np.random.default_rng(n_guides)
    G, max_mm = 20, 2
    guides = [br.random_seq(rng, G) for _ in range(n_guides)]
    guides[-1] = guides[0]
    planted = [guides[i] for i in (0, 1, 511, n_guides - 2)]
    contigs = _planted_contigs(rng, planted, "NGG", False, (("c", 3100),), (("DNA", 1),), max_mm, per=9, seams=(("c", 1024), ("c", 2048)))
    return guides, contigs


@pytest.mark.parametrize("n_guides", _SEAM_COUNTS)
def test_guide_chunk_seam(n_guides):
    """Guide counts around the 1024 guides a workgroup keeps in LDS at a time, DNA bulges of 1 on ~3 kb; the same guide at index 0
    and at the last index gets the same rows."""
    G, max_mm = 20, 2
    guides, contigs = _seam_inputs(n_guides)
    want = _want(contigs, guides, "NGG", False, max_mm, 1, 0)
    assert len(want) > 30 and {0, 1, 511, n_guides - 2, n_guides - 1} <= {t[0] for t in want}
    idx = GenomeIndex(contigs, G, 3, piece=1024, max_bulge=1)
    got = [_key(h) for h in idx.scan_bulges(guides, _pam("NGG", False), False, max_mm, 1, 0, engine="device")]
    assert got == want
    assert [t[1:] for t in got if t[0] == 0] == [t[1:] for t in got if t[0] == n_guides - 1] != []


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
_COLS = (("guide", np.uint32), ("row", np.uint32), ("q", np.uint32), ("strand", np.uint8), ("mm", np.uint8), ("code", np.uint64),
         ("nmask", np.uint32), ("gaps", np.uint64))


def _raw(idx, guides, pam, right, max_mm, btype, bsize, cap, guidelen=None):
    """hawk_offtarget_bulges as the ABI has it: (status, *n_out, the rows written as sorted tuples)"""
    g2 = encode_guides(guides)
    par = _lib.OtParams(pam.bits, pam.bitsrc, len(pam), idx.guidelen if guidelen is None else guidelen, int(bool(right)), max_mm)
    o = {k: np.zeros(max(cap, 1), t) for k, t in _COLS}
    n = C.c_uint64(0)
    rc = idx.ds._L.hawk_offtarget_bulges(idx.ds._h, C.byref(par), _p(g2), len(g2), btype, bsize, *[_p(o[k]) for k, _t in _COLS], C.c_uint64(cap),
                                         C.byref(n), None)
    k = min(int(n.value), cap) if rc == _lib.HAWK_OK else 0
    return rc, int(n.value), sorted(zip(*[o[name][:k].tolist() for name, _t in _COLS]))


def _abi_case():
    rng = np.random.default_rng(8)
    guides = [br.random_seq(rng, 20) for _ in range(4)]
    contigs = _planted_contigs(rng, guides, "NGG", False, (("c", 5000),), (("DNA", 1), ("RNA", 2)), 2, per=6, seams=(("c", 1024),))
    return guides, contigs, GenomeIndex(contigs, 20, 3, piece=1024, max_bulge=2)


@pytest.mark.parametrize("btype,bsize", [(1, 1), (2, 2)])
def test_capacity_contract(btype, bsize):
    """cap one below the need: HAWK_E_CAPACITY with the exact need; the retry returns the rows of a run with ample room; cap = 0
    behaves the same way."""
    guides, contigs, idx = _abi_case()
    pam = _pam("NGG", False)
    idx._set_window(20 + bsize if btype == 1 else 20 - bsize)
    rc, need, rows = _raw(idx, guides, pam, False, 2, btype, bsize, 4096)
    assert rc == _lib.HAWK_OK and need == len(rows) > 20
    assert len({r[:4] for r in rows}) == need  # one row per (guide, site, strand)
    for cap in (need - 1, 0):
        rc, n, none = _raw(idx, guides, pam, False, 2, btype, bsize, cap)
        assert (rc, n, none) == (_lib.HAWK_E_CAPACITY, need, [])
        assert _raw(idx, guides, pam, False, 2, btype, bsize, n) == (_lib.HAWK_OK, need, rows)


def test_abi_refusals():
    guides, contigs, idx = _abi_case()
    pam = _pam("NGG", False)
    idx._set_window(21)
    refused = (_lib.HAWK_E_INVALID, _lib.HAWK_E_UNSUPPORTED)
    for btype, bsize in ((1, 0), (1, 3), (0, 1), (3, 1)):
        assert _raw(idx, guides, pam, False, 2, btype, bsize, 64)[0] == _lib.HAWK_E_INVALID
    assert _raw(idx, [g[:4] for g in guides], pam, False, 2, 2, 2, 64, guidelen=4)[0] in refused   # G - b < 3
    assert _raw(idx, [g + g[:8] for g in guides], pam, False, 2, 1, 2, 64, guidelen=28)[0] in refused  # 28 + 2 + 3 bases
    assert _raw(idx, guides, pam, False, 2, 1, 2, 64)[0] == _lib.HAWK_E_INVALID  # the scan ranges are those of 21 + 3 bases, not 22 + 3
    assert _raw(idx, guides, pam, False, 2, 1, 1, 4096)[0] == _lib.HAWK_OK


def test_nothing_to_find():
    """An index without rows on this rank and an empty guide list return no rows."""
    guides, contigs, idx = _abi_case()
    pam = _pam("NGG", False)
    assert idx.scan_bulges([], pam, False, 2, 2, 2, engine="device") == []
    none = GenomeIndex({"c": contigs["c"][:900]}, 20, 3, piece=1024, max_bulge=2, shard=(1, 2))
    assert none.ds is None and none.scan_bulges(guides, pam, False, 2, 2, 2, engine="device") == []


def test_product_route_takes_the_device_engine(monkeypatch):
    """offtargets.search(..., bdna, brna): the targets rows are those the derived engine gives, and they come from the device engine."""
    from crisprhawk_hip import offtargets
    guides, contigs, idx = _abi_case()
    pam = _pam("NGG", False)
    want = [offtargets.crispritz_report_line(h, guides[h.guide], 3, False) for h in idx.scan(guides, pam, False, 2)] + \
        [offtargets.crispritz_bulge_line(h, 3, False) for h in idx.scan_bulges(guides, pam, False, 2, 1, 1, engine="derived")]
    engines = []
    inner = GenomeIndex.scan_bulges
    monkeypatch.setattr(GenomeIndex, "scan_bulges", lambda self, *a, **kw: (engines.append(kw.get("engine")), inner(self, *a, **kw))[1])
    got = offtargets.search(idx, guides, pam, False, 2, 0, False, bdna=1, brna=1)
    assert got == want and sum(ln.startswith(("DNA", "RNA")) for ln in got) > 10
    assert engines == ["device"]
