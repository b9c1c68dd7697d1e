"""The plane search (hawk_search.hip: k_search_count, k_emit_list, k_search_emit, k_ref_bits, hawk_launch_mscan) on its seams:
the hand-built cases of tests/search_refs.py - each proved on the CPU to sit on the seam it is named after - through
DeviceHapSet(...).search(...) against the oracle.  Counts, coordinates, windows, REF-partner flags and CFDon are compared
bit-exact, and the table is held to its raw order before any sorting: rows ascend by (row, tile, strand, window start), which a
permutation inside a tile would break without changing anything reference_order() shows."""
import numpy as np
import pytest

import search_refs as sr
from crisprhawk_hip import synth
from crisprhawk_hip.hapset import DeviceHapSet, HostHaplotype, PosSegments, segments_from_posmap
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

SEARCH_CASES = list(sr.CASES)
_built = {}


def built(name: str) -> sr.Case:
    """a case and its oracle result, built once and shared by the tests that read it"""
    if name not in _built:
        _built[name] = sr.CASES[name]()
    return _built[name]


def device_set(c: sr.Case) -> DeviceHapSet:
    haps = []
    for seq, pm, r, sc in zip(c.seqs, c.posmaps, c.is_ref, c.scan):
        rel, gen = segments_from_posmap(pm)
        assert np.array_equal(rel.astype(np.int64), sr.segment_starts(pm))  # the restated segment rule is the product's
        haps.append(HostHaplotype(seq, PosSegments(rel, gen, len(seq)), r, sc))
    return DeviceHapSet(haps)


@pytest.mark.parametrize("name", SEARCH_CASES)
def test_search_on_a_seam_against_the_oracle(name):
    c = built(name)
    missing = [frag for frag in sr.REQUIRED[name] if not any(frag in label for label in c.proved)]
    assert not missing and c.in_domain(), (name, missing)
    want = c.want
    bits, bitsrc, _, _ = ora.pam_encode(c.pam)
    score = c.pam == "NGG" and not c.right
    mm, pt = synth.cfd_tables() if score else (None, None)
    ds = device_set(c)
    assert ds.stride == sr.stride_words(max(len(s) for s in c.seqs))
    tab = ds.search(bits, bitsrc, c.pamlen, c.guidelen, c.right, mm, pt)
    assert (tab.n_rows, tab.n_candidates, tab.n_hits) == (len(want.guides), want.n_candidates, want.n_hits)
    # the raw table: (row, tile, strand, window start) ascending, the per-tile row counts the case proved
    q = c.qstart(tab.pos, tab.strand)
    tile = q // sr.TILE
    assert np.array_equal(np.lexsort((q, tab.strand, tile, tab.hap)), np.arange(tab.n_rows)), "rows are not in (row, tile, strand, start) order"
    per = np.bincount(tab.hap.astype(np.int64) * c.bph + tile, minlength=len(c.seqs) * c.bph)
    for (h, t), v in c.tally().items():
        assert per[h * c.bph + t] == v["valid"], (h, t, int(per[h * c.bph + t]), v)
    # the table in the reference's order
    order = tab.reference_order()
    g = want.guides
    for col in ("start", "stop", "hap", "pos", "strand"):
        assert np.array_equal(getattr(tab, col)[order], g[col]), col
    wins = tab.windows()
    assert [wins[i] for i in order] == want.windows
    assert np.array_equal(tab.flags[order], c.expected_flags())
    if score:
        _, _, _, cfd, _ = ora.reverse_and_cfdon(want, c.is_ref, c.guidelen, c.pamlen, mm, pt, decode=False)
        mine = tab.cfdon[order]
        assert np.array_equal(np.isnan(mine), np.isnan(cfd)) and np.array_equal(mine[~np.isnan(cfd)], cfd[~np.isnan(cfd)])
        alt = ~np.asarray(c.is_ref)[g["hap"]]
        assert np.array_equal(np.isnan(cfd[alt]), c.expected_flags()[alt] == 0)  # an alt row scores iff REF has a guide at its key
    else:
        assert np.isnan(tab.cfdon).all()


@pytest.mark.parametrize("name", sr.PAM_SCAN_SETS)
def test_pam_scan_offsets_without_shard_sums(name):
    """hawk_pam_scan scans 2 * n_hap counts through k_mscan1 / k_mscan2 / k_mscan3 (no shard sums): 2, 3 and 5 partials"""
    c = built(name)
    assert sr.pam_scan_partials(len(c.seqs), c.bph) == f"k_mscan1/2/3 {-(-2 * len(c.seqs) // sr.MS_TILE)} partials"
    bits, bitsrc, _, _ = ora.pam_encode(c.pam)
    hits = device_set(c).pam_scan(bits, bitsrc, c.pamlen)
    assert len(hits) == len(c.seqs)
    total = 0
    for h, (f, r) in enumerate(hits):
        wf, wr = ora.scan(ora.encode(c.seqs[h]), c.scan[h][0], c.scan[h][1], bits, bitsrc, c.pamlen)
        assert np.array_equal(f, wf) and np.array_equal(r, wr), h
        total += len(wf) + len(wr)
    assert total == c.want.n_hits > 0
