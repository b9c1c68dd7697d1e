"""The case builders of tests/test_gpu_vsearch_seams.py, checked on the CPU: every case proves from the oracle's strings, scans and
search that it sits on the seam it is listed for, the restatement of k_vsearch that says so (vsearch_refs.tile_plan) is pinned on
both sides of each of its thresholds, and a case pushed off its seam - or a restatement with one of the kernel's constants moved by
one - fails instead of passing."""
import numpy as np
import pytest

import vsearch_refs as vr
from vsearch_refs import D, I, S

_built = {}


def built(name):
    if name not in _built:
        _built[name] = vr.CASES[name]()
    return _built[name]


def test_the_gpu_module_runs_exactly_these_cases():
    import test_gpu_vsearch_seams as tg
    assert sorted(tg.SEAM_CASES + ["default_route"]) == sorted(vr.CASES) == sorted(vr.REQUIRED)


@pytest.mark.parametrize("name", list(vr.CASES))
def test_every_case_proves_its_seam_from_the_oracle(name):
    c = built(name)
    assert c.name == name and c.proved
    missing = [frag for frag in vr.REQUIRED[name] if not any(frag in label for label in c.proved)]
    assert not missing, (name, missing)
    tally = c.tally()  # asserts: the restated totals over every row and tile are the oracle's n_hits and n_candidates
    rows = c.device_rows()
    assert len(tally) == len(rows) * c.bph and all(tally[(r, t)] == 0 for r, x in enumerate(rows, 1) if not x[3] for t in range(c.bph))
    haps = c.oracle()[0]
    assert haps[0]["samples"] == ["REF"] and haps[0]["seq"] == c.ref and len(haps) == 1 + sum(x[3] for x in rows)
    print(c.summary())


def test_a_case_off_its_seam_fails():
    c = vr.Case("drift", 3000, 1)
    si = c.add([I(500, "AT"), S(1024)])  # the upstream insertion moves the SNV off the map-word seam
    with pytest.raises(AssertionError, match="off its seam"):
        c.prove("SNV on bit 0 of map word 1", int(c.row(si).o[1]) == 1024)
    assert int(c.row(si).o[1]) == 1026 and not c.proved
    with pytest.raises(AssertionError, match="PAM letter"):
        c.plant_row(si, 1026 - 21, 0)  # a PAM letter on an alt base the builder did not choose


def test_case_keeps_variants_as_specs_until_they_are_read():
    c = vr.Case("specs", 3000, 2)
    si = c.add([D(700, 4)])
    c.guide(si, 1000, (0, 1))  # planted after the deletion: row position 1000 is REF position 1004
    row = c.row(si)
    assert c.ref[1004:1006] == "CC" and c.ref[1004 + 21:1004 + 23] == "GG" and row.seq[1000:1002] == "CC"
    assert set(c.ref) - set("AT") == {"C", "G"} and c.ref.count("G") == 2
    assert c.has_row(si, 1000, 0) and c.has_row(si, 1000, 1) and c.is_survivor(si, 1000, 0)
    assert c.region().sequence == c.ref and [v.pos for v in c.region().variants] == sorted(v.pos for v in c.region().variants)


def _plan(specs, tile=0, length=3000, **kw):
    c = vr.Case("hand", length, 3, **kw)
    si = c.add(specs)
    return c, si, c.plan(si, tile)


def test_tile_plan_staging_on_both_sides_of_its_thresholds():
    T = vr.TILE
    for before in (10, 11, 12):  # records in front of the tile-index record
        p = _plan([S(T - 400 + 20 * i) for i in range(before)] + [S(T - 1)], tile=1, length=vr.TWO_TILES)[2]
        assert (p["before"], p["back"], p["start"]) == (before, min(before, 11), max(before - 11, 0))
    for k, (n, every) in ((127, (127, True)), (128, (128, True)), (129, (128, False))):
        p = _plan([S(150 + 20 * i) for i in range(k)], length=3600)[2]
        assert (p["avail"], p["n"], p["all"]) == (k, n, every)
        assert all(p["fast"].values()) == every
    for d, n in ((63, 2), (64, 1)):
        p = _plan([S(500), S(T + d)], length=vr.TWO_TILES)[2]
        assert p["n"] == n and p["avail"] == 2
    for d, last in ((21, True), (22, False)):  # L = 23: o = p_hi + L - 2 | p_hi + L - 1
        p = _plan([S(500), S(T + d)], length=vr.TWO_TILES)[2]
        assert ((vr.HX_TW - 1) in p["words"]) == last


def test_tile_plan_dirty_words_chunks_and_builders():
    # a SNV at bit b of word 10 dirties the starts b - 22 .. b: one word from bit 22 on, two below
    for b, words in ((22, [10]), (21, [9, 10]), (31, [10]), (0, [9, 10])):
        assert _plan([S(320 + b)])[2]["words"] == words
    assert _plan([D(320 + 22, 5)])[2]["words"] == [10] and _plan([I(320 + 22, "ATATATATAT")])[2]["words"] == [10, 11]
    for n_tasks, chunks in ((127, 1), (128, 1), (129, 2), (256, 2), (257, 3)):
        p = _plan([S(32 * (6 + w) + 28) for w in range(n_tasks)], length=32 * (n_tasks + 12) + 400)[2]
        assert (p["n_tasks"], p["n_chunks"], [len(ch["words"]) for ch in p["chunks"]][-1]) == (n_tasks, chunks, n_tasks - 128 * (chunks - 1))
    o = np.array([100, 400]); shift = np.array([0, 0])
    for k, fast in ((32, True), (33, False)):
        assert vr.string_fast(o, np.array([k, 1]), shift - np.array([k - 1, k - 1]), 0, 2, True, 110) == fast  # in force at p0
        assert vr.string_fast(o, np.array([k, 1]), shift - np.array([k - 1, k - 1]), 0, 2, True, 60) == fast   # starting inside
        assert vr.string_fast(o, np.array([k, 1]), shift - np.array([k - 1, k - 1]), 0, 2, True, 100 + k)      # behind the allele
    for d, fast in ((95, False), (96, True)):
        assert vr.string_fast(np.array([100]), np.array([40]), np.array([-39]), 0, 1, True, 100 - d) == fast
    assert not vr.string_fast(np.array([100]), np.array([1]), np.array([0]), 0, 1, False, 50)  # records beyond the staged ones


def test_tile_plan_segments_and_runs():
    for nseg in (63, 64, 65):
        p = _plan([D(400 + 50 * i, 2) for i in range(nseg - 1)], length=6000)[2]
        assert (p["nseg"], p["ovf"]) == (nseg, nseg > 64)
    p = _plan([I(400, "ATA")])[2]
    assert p["nseg"] == 5  # one per inserted base and the one the device opens where REF resumes
    p = _plan([D(1000, 7), S(2000)])[2]
    assert [(r["pa"], r["pb"], r["shift"]) for r in p["runs"]] == [(0, 960, 0), (1024, 1952, 7), (2016, 32 * p["nwt"], 7)]
    assert [r["branch"] for r in p["runs"]] == ["partial", "two", "partial"]


def test_remap_and_prefix_rounds_restated():
    for grid in (1, 7, 8, 9, 15, 16, 17, 64, 1000):
        assert sorted(vr.emit_tile(b, grid) for b in range(grid)) == list(range(grid))
        assert (sorted(vr.emit_tile(b, grid, guard=False) for b in range(grid)) == list(range(grid))) == (grid % 8 == 0 or grid == 1)
    assert [vr.emit_tile(b, 17) for b in range(17)] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15, 16]
    assert vr.prefix_rounds(1024) == [(0, 1024), (1024, 1)] and vr.prefix_rounds(1028) == [(0, 1024), (1024, 5)]
    assert vr.prefix_rounds(2048)[-1] == (2048, 1) and vr.prefix_rounds(1024, closing=False) == [(0, 1024)]
    assert vr.prefix_rounds(1028, closing=False) == vr.prefix_rounds(1028)  # the closing round is lost only at a multiple of 1024


# One of the kernel's constants moved by one in the RESTATEMENT knocks the named case off its seam.  (Moved in the kernel instead:
# the dirty range and the 96-bit cut change the table of the same cases on the device; VC_BACK 10, VC_REACH 63 and `alt_len >= 32`
# change which path serves a word but not the table - a tile's strings need 10 records back, not 11, and reach p_hi + 52 at most -
# and the closing entry of k_ref_hits_prefix is never read; see the module docstring of vsearch_refs.)
@pytest.mark.parametrize("const,value,name", [("VC_BACK", 10, "back_full"), ("VC_BACK", 8, "back_full"), ("VC_REACH", 63, "reach"), ("WINDOW_EDGE", 2, "touch_L23"),
                                              ("FAST_ALLELE", 31, "strings"), ("FAST_SPAN", 97, "strings"), ("VC_MAXV", 127, "staged_128_all"),
                                              ("VC_SLOTS", 127, "tasks_128"), ("NSEG", 63, "segments_64"), ("REF_ROUND", 1023, "stride_1024")])
def test_a_moved_constant_knocks_its_case_off_the_seam(monkeypatch, const, value, name):
    monkeypatch.setattr(vr, const, value)
    try:
        c = vr.CASES[name]()
    except AssertionError:
        return
    assert [frag for frag in vr.REQUIRED[name] if not any(frag in label for label in c.proved)], (const, value, name)
