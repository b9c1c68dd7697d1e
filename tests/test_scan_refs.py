"""tests/scan_refs.py without a GPU: every case of tests/test_gpu_scan_family.py sits on the seam it is named after, the references
are what they claim to be, and the kernels' arithmetic restated in numpy shows what the device test can tell apart: with the wave
reductions as they were before wave_sum64 (two 32-bit halves summed apart) the `big` panel gives wrong offsets on the M1_M23 and WIDE
routes wherever one wave's share of the partials reaches 2^32, the `product` panel never does, and carry-safe reductions give the
reference everywhere."""
import numpy as np
import pytest

import scan_refs as sc
import search_refs as sr

MSCAN = [(g, i) for g in sc.CASES for i in range(len(sc.CASES[g]))]


def test_the_groups_are_the_ones_asked_for():
    ns = {g: [c["n"] for c in cs] for g, cs in sc.CASES.items()}
    assert ns == {"m23": [2_049, 262_144, 262_145, 263_169, 4_194_304], "wide": [4_194_305, 4_194_320, 4_198_399, 4_198_400, 16_777_216],
                  "unaligned": [4_194_305] * 3, "m2_shards": [16_777_217], "m2_chunks": [1_048_576, 1_048_577, 2_097_153]}
    assert sc.GROUPS == ("m23", "wide", "unaligned", "m2_shards", "m2_chunks", "scan2")
    assert sorted(c["shift"] for c in sc.CASES["unaligned"]) == [(0, 1), (1, 0), (1, 1)]
    assert all(c["shards"] for g in ("m23", "wide", "unaligned", "m2_shards") for c in sc.CASES[g]) and not any(c["shards"] for c in sc.CASES["m2_chunks"])
    assert all(c["shift"] == (0, 0) for g in ("m23", "wide", "m2_shards", "m2_chunks") for c in sc.CASES[g])
    panels = lambda g: [set(c["panels"]) for c in sc.CASES[g]]
    every, pb = set(sc.PANELS), {"product", "big"}
    assert panels("m23") == [every - {"big"}] * 2 + [every] * 3 and panels("wide") == [every] * 2 + [pb] * 3
    assert panels("unaligned") == [pb] * 3 and panels("m2_shards") == [pb] and panels("m2_chunks") == [every] * 3
    assert sc.SCAN2_N == (1, 15, 16, 17, 16_383, 16_384, 16_385, 16_400, 32_769)
    assert sc.SCAN2_NDESC == (None, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("group,i", MSCAN)
def test_every_case_sits_on_its_seam(group, i):
    case = sc.CASES[group][i]
    r = sc.check_case(case)
    assert sc.ROUTE_CODE[r["route"]] in (1, 2, 3)
    # what the names promise, from the route's own figures
    if group == "wide":
        assert r["tile"] == 4096 and r["tail"] == {4_194_305: 1, 4_194_320: 16, 4_198_399: 4095, 4_198_400: 4096, 16_777_216: 4096}[case["n"]]
    if group in ("unaligned", "m2_shards", "m2_chunks"):
        assert r["chunks"] == (r["partials"] + 1023) // 1024 and r["last_chunk"] == r["partials"] - 1024 * (r["chunks"] - 1)
    if group == "unaligned":  # aligned, the same n takes the wide pair
        assert sr.scan_route(case["n"], True, True)["route"] == "WIDE"


def test_a_case_off_its_seam_fails():
    case = dict(sc.CASES["wide"][0], n=4_194_304)
    with pytest.raises(AssertionError):
        sc.check_case(case)
    case = dict(sc.CASES["unaligned"][0], shift=(0, 0))
    with pytest.raises(AssertionError):
        sc.check_case(case)


def test_the_panels_and_the_reference():
    c = np.array([3, 0, 5, 1], dtype=np.uint32)
    sh = np.arange(512, dtype=np.uint64)
    off, tot = sc.reference(c, sh)
    assert off.dtype == np.uint64 and off.tolist() == [0, 3, 3, 8] and tot == (9, 0, sum(range(0, 512, 2)), sum(range(1, 512, 2)))
    assert sc.reference(c, None)[1] == (9, 0, 0, 0)
    big = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
    assert sc.reference(big, None)[0].tolist() == [0, 0xFFFFFFFF, 2 * 0xFFFFFFFF]  # 64-bit: nothing wraps
    n = 263_169
    assert np.array_equal(sc.reference(sc.counts_panel("ones", n), None)[0], np.arange(n, dtype=np.uint64))
    p = sc.counts_panel("product", n)
    assert int(p.max()) <= (2 ** 32 - 1) // n < 65_536 and int(p.sum(dtype=np.uint64)) < 2 ** 32 and len(np.unique(p)) > 1000
    assert int(sc.counts_panel("product", 2_049).max()) in range(60_000, 65_537)
    e = sc.counts_panel("edges", n)
    at = np.flatnonzero(e)
    want = sorted(set(range(0, n, 1024)) | set(range(1023, n, 1024)) | {n - 1})
    assert at.tolist() == want and set(e[at].tolist()) == {65_536} and {0, 1023, 1024, 4095, 4096, n - 1} <= set(want)
    for m in (262_145, 16_777_217):
        b = sc.counts_panel("big", m)
        assert int(b.max()) == 65_536 and abs(int(b.sum(dtype=np.uint64)) / (m * 2 ** 15) - 1) < 0.01 and 2 ** 32 < m * 2 ** 15 < 2 ** 40  # about 2^33 ... 2^39
    with pytest.raises(AssertionError):
        sc.counts_panel("big", 262_144)
    assert np.array_equal(sc.counts_panel("big", 262_145), sc.counts_panel("big", 262_145))  # seeded
    s = sc.shard_panel(2_049)
    assert s.dtype == np.uint64 and len(s) == 512 and int(s.max()) < 2 ** 40 and int(s.max()) > 2 ** 39


def test_the_wave_sum_as_it_was_loses_the_carries():
    v = np.zeros(64, dtype=np.uint64)
    v[:2] = 0x80000000  # two lanes whose low halves add up to 2^32
    assert int(sc._wave_sum(v, carry_safe=True)) == 2 ** 32 and int(sc._wave_sum(v, carry_safe=False)) == 0
    v[:] = 0x1_0000_0001
    assert int(sc._wave_sum(v, True)) == int(sc._wave_sum(v, False)) == 64 * 0x1_0000_0001  # no carry: the same


# where one wave's share of the partials in front of the last workgroups reaches 2^32 with counts of 32 768 on average: a thread adds
# `trips` partials of tile x 32 768 each, a wave 64 threads' worth - 2^31 x trips on the 1024-count route, 2^33 x trips on the wide one
SEPARATES = {("m23", 262_145): False, ("m23", 263_169): False, ("m23", 4_194_304): True,
             ("wide", 4_194_305): True, ("wide", 4_194_320): True, ("wide", 4_198_399): True, ("wide", 4_198_400): True, ("wide", 16_777_216): True}


@pytest.mark.parametrize("group,i", [(g, i) for g, i in MSCAN if sc.CASES[g][i]["shift"] in ((0, 0), (1, 1))])
def test_what_the_panels_tell_apart(group, i):
    case = sc.CASES[group][i]
    n, route = case["n"], case["route"]
    fused = route in ("M1_M23", "WIDE")
    for panel in case["panels"]:
        if panel in ("ones", "edges") and n > 300_000:
            continue  # (emulated at the smaller sizes: the arithmetic does not depend on n)
        counts = sc.counts_panel(panel, n)
        want, tot = sc.reference(counts, None)
        was_off, was_keep = sc.emulate(counts, route, carry_safe=False)
        was_right = np.array_equal(was_off, want) and was_keep == tot[0]
        if panel != "big" or not fused:
            assert was_right, (group, n, panel)  # today's domain, and the routes whose second kernel is 64-bit throughout
        else:
            assert was_right != SEPARATES[(group, n)], (group, n)
            if not was_right:  # silently: every offset from the first wrapped prefix on is short by a multiple of 2^32
                bad = np.flatnonzero(was_off != want)
                assert bad[0] % sr.scan_route(n)["tile"] == 0 and was_keep != tot[0]
                assert set(((want[bad] - was_off[bad]) % np.uint64(2 ** 32)).tolist()) == {0}
        if panel == "big":
            now_off, now_keep = sc.emulate(counts, route, carry_safe=True)
            assert np.array_equal(now_off, want) and now_keep == tot[0], (group, n)
    assert not fused or "big" not in case["panels"] or (group, n) in SEPARATES


def test_the_remaining_domain_is_the_tile_sum():
    """carry-safe reductions leave one 32-bit quantity: the scan inside a tile.  Counts of 2^22 fill a 1024-count tile to exactly 2^32"""
    n = 3 * 1024
    ok = np.full(n, 2 ** 22 - 1, dtype=np.uint32)
    off, keep = sc.emulate(ok, "M1_M23", True)
    assert np.array_equal(off, sc.reference(ok, None)[0]) and keep == n * (2 ** 22 - 1)
    over = np.full(n, 2 ** 22, dtype=np.uint32)
    assert sc.emulate(over, "M1_M23", True)[1] == 2 * 2 ** 32 != sc.reference(over, None)[1][0] == 3 * 2 ** 32  # the last tile's total wrapped to 0
    over[:] = 2 ** 23  # ... and the offsets inside a tile from its middle on
    assert not np.array_equal(sc.emulate(over, "M1_M23", True)[0], sc.reference(over, None)[0])


@pytest.mark.parametrize("n_desc", [d for d in sc.SCAN2_NDESC if d])
def test_the_bitmap_reference(n_desc):
    d = sc.scan2_desc(n_desc)
    at = set(np.flatnonzero(d).tolist())
    assert {0, n_desc - 1} <= at and all(i in at for k in (32, 64, 1024) for m in range(k, n_desc + 1, k) for i in (m - 1, m) if i < n_desc)
    assert (len(at) < n_desc or n_desc <= 2) and any(int(x) & 0xFFFFFFFF == 0 for x in d[sorted(at)]) == (len(at) > 1)
    a, b = sc.scan2_counts(17)
    oa, ob, bits = sc.scan2_reference(a, b, d)
    assert len(bits) == n_desc // 32 + 1 and oa[0] == ob[0] == 0 and int(oa[-1]) == int(a.sum(dtype=np.uint64)) and len(oa) == 18
    written = sc.scan2_bits_written(n_desc)
    assert written in (len(bits), len(bits) - 1) and (written == len(bits)) == (n_desc % 1024 != 0)
    for v in range(n_desc):  # bit v of the bitmap <=> desc[v] != 0
        assert (int(bits[v >> 5]) >> (v & 31)) & 1 == (v in at)
    for w in range(len(bits)):  # no other bit in a written word; an unwritten word keeps the sentinel
        if w >= written:
            assert int(bits[w]) == sc.SENTINEL32
        else:
            assert int(bits[w]) >> max(0, min(32, n_desc - 32 * w)) == 0


def test_the_scan2_counts_stay_below_32_bits():
    for n in sc.SCAN2_N:
        a, b = sc.scan2_counts(n)
        assert len(a) == len(b) == n and int(a.sum(dtype=np.uint64)) < 2 ** 32 and int(b.max()) <= 3
        oa, ob, bits = sc.scan2_reference(a, b, None)
        assert bits is None and np.array_equal(np.diff(oa.astype(np.int64)), a) and np.array_equal(np.diff(ob.astype(np.int64)), b)
