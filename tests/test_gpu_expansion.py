"""The device haplotype expansion (hawk_expand.hip, hawk_hx.h, hawk_meta.hip) with variants placed ON its seams: tiles of
32768 output positions, words and word quads, the 96 staged records, the staged REF window of 1088 words, alleles of 32
and 33 bases, row ends, rounds of 256 indels and 4096 rows, and the row identity the collapse rests on.  Every expected
value comes from the string-level oracle (oracle.hap_build per chromosome copy, its position map, oracle.scan_bounds,
oracle.posmap_rev); every comparison is bit-exact.  The cases are built by tests/expansion_refs.py, where each one first
proves from the oracle alone that it sits on its seam (tests/test_expansion_refs.py runs that part without a GPU)."""
import numpy as np
import pytest

import expansion_refs as xr
from crisprhawk_hip import _lib
from crisprhawk_hip.expand import HaplotypeBuildError
from crisprhawk_hip.hapset import _p, segments_from_posmap
from crisprhawk_hip.workload import expand_on_device
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

PLANE_CASES = [n for n, f in xr.CASES.items() if n not in ("list_overlap", "list_clamp")]
ERROR_CASES = ["list_overlap", "list_clamp"]


def _first_difference(case, got, want, r, si, c):
    """where a row's planes part from the oracle's, with the tile's geometry: the message of a failed comparison"""
    pl, w = [int(x[0]) for x in np.nonzero(got != want)]
    row = case.row(si, c)
    near = [(int(o), int(n), int(ch)) for o, n, ch in zip(row.o, row.alt_len, row.chain) if abs(int(o) - 32 * w) < 200]
    return (f"{case.name}: row {r} (sample {si} copy {c}, {row.len} bases) plane {pl} word {w} (position {32 * w}, tile {w // xr.HX_TW}): "
            f"got {int(got[pl, w]):#010x} want {int(want[pl, w]):#010x}; tile {xr.tile_index(row, w // xr.HX_TW, len(case.ref))}; "
            f"records (o, alt_len, chain) near: {near}")


def _expand_and_compare(case):
    """Planes, lengths, position-map segments and reverse look-ups of EVERY row (collapsed ones too) against the oracle's
    row of that chromosome copy; kept rows, their sample labels and scan bounds against the oracle's collapse."""
    reg = case.region()
    ds, info, _ms, kept = expand_on_device(reg, case.pamlen, keep_plan=True)
    cols = case.live_columns()
    assert ds.n_hap == 1 + len(cols)
    S = ds.stride
    longest = max([len(case.ref)] + [case.row(si, c).len for si, c in cols])
    assert S == xr.stride_words(longest) and S * 32 >= longest
    got = ds.planes()
    assert int(ds.hap_len[0]) == len(case.ref) and np.array_equal(got[:, 0, :], xr.planes_from_string(case.ref, S)), "REF row"
    # the reverse look-ups the scan bounds start from, straight from the plan (k_rev_lookup)
    hap_len = np.zeros(ds.n_hap, dtype=np.uint32)
    rev0, rev1 = np.zeros(ds.n_hap, dtype=np.int64), np.zeros(ds.n_hap, dtype=np.int64)
    _lib.check(_lib.lib().hawk_xplan_rows(ds.plan._x, _p(hap_len), _p(rev0), _p(rev1)), "hawk_xplan_rows")
    g_lo, g_hi = case.startp + 100, case.stopp - 100
    assert (int(rev0[0]), int(rev1[0])) == (100, len(case.ref) - 101)
    for r, (si, c) in enumerate(cols, 1):
        row = case.row(si, c)
        assert int(ds.hap_len[r]) == int(hap_len[r]) == row.len, (case.name, r)
        want = xr.planes_from_string(row.seq, S)  # the words behind the row, up to the stride, are zero
        if not np.array_equal(got[:, r, :], want):
            pytest.fail(_first_difference(case, got[:, r, :], want, r, si, c))
        seg = ds.host_meta.seg(r)
        assert seg.length == row.len and np.array_equal(seg.full(), row.pm), (case.name, r, "position map")
        rel, gen = row.device_segments()  # the map's breaks plus the one the device opens behind every insertion
        assert np.array_equal(seg.rel, rel) and np.array_equal(seg.gen, gen), (case.name, r, "segments")
        rel, gen = xr.canonical_segments(seg.rel, seg.gen)
        want_rel, want_gen = segments_from_posmap(row.pm)
        assert np.array_equal(rel, want_rel) and np.array_equal(gen, want_gen), (case.name, r, "segments of the oracle's position map")
        assert (int(rev0[r]), int(rev1[r])) == (ora.posmap_rev(row.pm, g_lo), ora.posmap_rev(row.pm, g_hi)), (case.name, r, "reverse look-up")
    haps = case.expected_haplotypes()
    assert len(kept) == len(haps)
    first_row = {}
    for r, (si, c) in enumerate(cols, 1):
        first_row.setdefault(case.row(si, c).seq, r)
    for j, r in enumerate(kept):
        h = haps[j]
        assert r == (0 if j == 0 else first_row[h["seq"]]), (case.name, j, "kept row")
        assert sorted(info[j].samples) == h["samples"], (case.name, j)
        assert tuple(ds.host_meta[r].scan) == ora.scan_bounds(h["posmap"], case.startp, case.stopp, case.pamlen), (case.name, j, "scan")
    return ds, kept, haps


def _search_against_oracle(case, ds, kept, haps):
    """one plain search of the expanded set: the tile metadata installed from the plan agrees with the planes"""
    scan = [ora.scan_bounds(h["posmap"], case.startp, case.stopp, 3) for h in haps]
    hs = ora.HapSet([h["seq"] for h in haps], [h["posmap"] for h in haps], [h["samples"] == ["REF"] for h in haps], scan)
    want = ora.search(hs, "NGG", 20, False)
    bits, bitsrc, _, _ = ora.pam_encode("NGG")
    tab = ds.search(bits, bitsrc, 3, 20, False)
    assert (tab.n_rows, tab.n_candidates, tab.n_hits) == (len(want.guides), want.n_candidates, want.n_hits)
    order = tab.reference_order()
    rowmap = np.full(ds.n_hap, -1, dtype=np.int64)
    rowmap[np.asarray(kept)] = np.arange(len(kept))
    g = want.guides
    assert np.array_equal(rowmap[tab.hap[order]], g["hap"])
    for col in ("start", "stop", "pos", "strand"):
        assert np.array_equal(getattr(tab, col)[order], g[col]), (case.name, col)
    wins = tab.windows()
    assert [wins[i] for i in order] == want.windows


@pytest.mark.parametrize("name", PLANE_CASES)
def test_expansion_on_its_seams_against_the_oracle(name):
    case = xr.CASES[name]()
    assert all(any(frag in label for label in case.proved) for frag in xr.REQUIRED[name])
    ds, kept, haps = _expand_and_compare(case)
    _search_against_oracle(case, ds, kept, haps)
    ds.plan.close()
    ds.close()


@pytest.mark.parametrize("name", ERROR_CASES)
def test_list_check_refuses_one_base_too_many(name):
    """k_list_check: a deletion that covers the next variant's base by one, an indel behind an upstream insertion that ends one
    base past the region's original length - their neighbours one base inside are the case `list_ok` above"""
    case = xr.CASES[name]()
    assert case.expect_error in ("overlap", "clamp") and all(any(f in label for label in case.proved) for f in xr.REQUIRED[name])
    with pytest.raises(HaplotypeBuildError, match="overlapping" if case.expect_error == "overlap" else "clamp"):
        expand_on_device(case.region(), case.pamlen)


def _hashes(case):
    ds, _info, _ms, kept = expand_on_device(case.region(), case.pamlen, keep_plan=True)
    ds2, hashes, _ = ds.plan.run(want_hash=True)
    out = (ds.stride, hashes.copy(), ds.alias.copy(), ds2.planes())
    ds2.close()
    ds.plan.close()
    ds.close()
    return out


def test_content_hash_and_row_identity():
    """k_hx_hash and hawk_hapset_rows_equal: equal cased strings from different variant sets share hash and row, one V bit or
    the last base of the last word keeps rows apart, and a row hashes alike under a wider stride"""
    narrow, wide = xr.CASES["identity"](), xr.CASES["identity_wide"]()
    S_n, h_n, alias_n, planes_n = _hashes(narrow)
    S_w, h_w, alias_w, planes_w = _hashes(wide)
    assert S_w > S_n == xr.stride_words(len(narrow.ref))
    cols = narrow.live_columns()
    assert wide.live_columns()[:len(cols)] == cols and [narrow.copies[s] for s, _ in cols] == [wide.copies[s] for s, _ in cols]
    seqs = [narrow.ref] + [narrow.row(si, c).seq for si, c in cols]
    for alias, h in ((alias_n, h_n), (alias_w, h_w)):
        for i in range(len(seqs)):
            for j in range(i):
                same = seqs[i] == seqs[j]
                assert (tuple(h[i]) == tuple(h[j])) == same, (i, j)
                assert (alias[i] == alias[j]) == same, (i, j)
        assert alias[2] == 1 and [int(alias[r]) for r in (0, 1, 3, 4, 5, 6)] == [0, 1, 3, 4, 5, 6]
    n = len(seqs)
    assert np.array_equal(h_n[:n], h_w[:n]), "rows of equal content hash alike under a wider stride"
    assert np.array_equal(planes_w[:, :n, :S_n], planes_n[:, :n, :]) and not planes_w[:, :n, S_n:].any()
