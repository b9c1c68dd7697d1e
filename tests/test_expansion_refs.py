"""The case builders of tests/test_gpu_expansion.py, checked on the CPU: every case proves from the oracle's strings and
position maps that it sits on the seam it is listed for, the helpers that say so are themselves pinned on small hand-made
inputs, and a case pushed off its seam fails instead of passing."""
import numpy as np
import pytest

import expansion_refs as xr
from oracle import oracle as ora
from util import oracle_haplotypes


def test_the_gpu_module_runs_exactly_these_cases():
    import test_gpu_expansion as tg
    assert sorted(tg.PLANE_CASES + tg.ERROR_CASES) == sorted(xr.CASES) == sorted(xr.REQUIRED)
    assert {"identity", "identity_wide"} <= set(tg.PLANE_CASES)


@pytest.mark.parametrize("name", list(xr.CASES))
def test_every_case_proves_its_seam_from_the_oracle(name):
    case = xr.CASES[name]()
    assert case.name == name and case.proved
    missing = [frag for frag in xr.REQUIRED[name] if not any(frag in label for label in case.proved)]
    assert not missing, (name, missing)
    if case.expect_error is None:
        cols = case.live_columns()
        assert len(cols) == len(case.copies)  # one row per sample here: copy 1 is REF throughout
        for si, c in cols:
            case.row(si, c)  # the oracle accepts every copy, and its output starts are where the prefix sums put them
        haps = case.expected_haplotypes()
        assert haps[0]["samples"] == ["REF"] and haps[0]["seq"] == case.ref
        for h in haps[::max(1, len(haps) // 60)]:  # every row is one the reference can scan: both bounds exist
            lo, hi = ora.scan_bounds(h["posmap"], case.startp, case.stopp, case.pamlen)
            assert 0 <= lo <= hi <= len(h["seq"])
        for si, c in cols[::max(1, len(cols) // 60)]:  # the device's segment list is the map's, one unit-slope break per insertion aside
            rel, gen = xr.canonical_segments(*case.row(si, c).device_segments())
            want = xr.segments_from_posmap(case.row(si, c).pm)
            assert np.array_equal(rel, want[0]) and np.array_equal(gen, want[1])
        if len(case.copies) <= 100:  # the labelling and collapse restated in the helper are tests/util.py's
            want = oracle_haplotypes(case.fixture())
            assert [h["seq"] for h in haps] == [h["seq"] for h in want] and [h["samples"] for h in haps] == [h["samples"] for h in want]
            assert all(np.array_equal(a["posmap"], b["posmap"]) for a, b in zip(haps, want))
    print(f"{name}: {len(case.copies)} samples, {len(case.ref)} bases, {len(case.proved)} seam conditions proved")


def test_a_case_off_its_seam_fails():
    c = xr.Case("drift", 2 * xr.TILE, 1)
    si = c.add([c.ins(100, 2), c.snv(xr.TILE)])  # the upstream insertion moves the SNV off the seam
    with pytest.raises(AssertionError, match="off its seam"):
        c.prove("SNV starts at the seam", int(c.row(si).o[1]) == xr.TILE)
    assert int(c.row(si).o[1]) == xr.TILE + 1 and not c.proved


def test_planes_from_string():
    seq = "ACGTacgtNRn" + "A" * 30
    S = 4
    pl = xr.planes_from_string(seq, S)
    assert pl.shape == (5, S) and pl.dtype == np.uint32 and not pl[:, 2:].any()
    bits = ((pl[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(5, -1)[:, :len(seq)]
    assert np.array_equal(bits[0] | bits[1] << 1 | bits[2] << 2 | bits[3] << 3, ora.encode(seq))
    assert bits[4].astype(bool).tolist() == [ch.islower() for ch in seq]
    assert pl[0, 0] & 0xff == 0b00010001 and pl[4, 0] & 0x7ff == 0b10011110000 and pl[0, 1] == (1 << 9) - 1
    assert xr.stride_words(32) == 4 and xr.stride_words(33) == 4 and xr.stride_words(65) == 8 and xr.stride_words(xr.CAP_LEN) - 3 == 2205


def test_tile_index_restates_the_kernel_on_hand_made_rows():
    c = xr.Case("hand", 2 * xr.TILE + 500, 2)
    si = c.add([c.snv(10), c.dele(xr.TILE - 1, 64), c.snv(xr.TILE + 64), c.ins(xr.TILE + 200, 33)])
    row = c.row(si)
    assert row.o.tolist() == [10, xr.TILE - 1, xr.TILE, xr.TILE + 136] and row.rs.tolist() == [11, xr.TILE + 64, xr.TILE + 65, xr.TILE + 201]
    assert row.len == len(c.ref) - 64 + 32
    t0, t1, t2 = (c.tile(si, wb) for wb in range(3))
    # tile 0: the SNV at 10 starts inside it (o > 0), the deletion's anchor is its last position; nothing at or before 0
    assert (t0["a"], t0["c"], t0["first"], t0["want"], t0["head"], t0["ws"], t0["we"]) == (0, 2, 0, 2, False, 0, ((xr.TILE + 64) >> 5) + 2)
    # tile 1: head = the SNV AT its first position (o <= p_lo), reading REF from behind it; 64 bases were deleted, 32 inserted
    assert (t1["a"], t1["c"], t1["first"], t1["want"], t1["head"]) == (3, 4, 2, 2, True)
    assert t1["raw_ws"] == (xr.TILE + 65) >> 5 and t1["ws"] == t1["raw_ws"] & ~3 and t1["we"] == ((2 * xr.TILE - 1 + 32) >> 5) + 2
    assert t1["fast"] and t2["fast"] and t2["head"] and t2["want"] == 1 and t2["window_clamped"] and not t0["window_clamped"]
    assert not c.tile(si, 3)["live"]
