"""hawk_search and the dictionary build take their `*_ms` fields from the device's wall clock: the kernel that opens an interval
stamps it into a block the status copy brings back (SearchStamp in hawk_api_search.hip, ClResults::begin / ::end), and no timed
event is recorded.  What the fields mean has not changed, so they are checked on every path (planes, per dirty word, per cluster)
and every flow of the table reservation (fresh, speculative, a refused speculative emit, the rerun after a template overflow):
which are set, how they nest, and that none of them can exceed the host's wall time of the call - a stamp left over from an earlier
call, or one that was never written, would.  Then the overlap shapes of test_gpu_search_overlap.py - REF much longer than the
cluster side, the reverse, two attempts in one call - through all three flows on one view, each table against the plane search of
the materialised set: the stamps come from kernels of both streams.  Each case prints its figures (-s)."""
import math
import time

import pytest

from crisprhawk_hip import synth
from crisprhawk_hip.workload import expand_on_device
from test_gpu_clusters import _same_rows
from test_gpu_search_overlap import _Both, _crowded_panel, _few_variants_panel, _panel, _scrub

pytestmark = pytest.mark.gpu

FIELDS = ("count_ms", "offsets_ms", "emit_ms", "emit_list_ms", "total_ms", "v_count_ms", "v_templates_ms", "v_emit_ms", "v_emit_rows_ms")
EVERY_SEARCH = ("count_ms", "offsets_ms", "emit_ms", "total_ms")
# a float32 field is its interval rounded to nearest (relative error <= 2^-24); count + offsets + emit and total add up to twice the
# total at most, so intervals that share their stamps differ by no more than this fraction of the total
F32_SUM = 2.0 ** -23


@pytest.fixture(autouse=True)
def _cluster_path_for_small_panels(monkeypatch):
    monkeypatch.setenv("HAWK_CLUSTER_MIN_SHARE", "0")
    for k in ("HAWK_VIEW_SEARCH", "HAWK_CLUSTER_ROWS0", "HAWK_CLUSTER_MAX_SLOTS"):
        monkeypatch.delenv(k, raising=False)


def _timed(fn):
    """-> (the table, the call's wall time in ms)"""
    t0 = time.perf_counter()
    t = fn()
    return t, (time.perf_counter() - t0) * 1e3


def _search(b, path, pam_s):
    if path == "planes":
        t, wall = _timed(lambda: b.planes(pam_s))
    else:
        t, wall = _timed(lambda: b.view.search(*b.args(pam_s)))
    assert t.timing["v_path"] == {"planes": 0, "words": 1, "cluster": 2}[path]
    return t, wall


def _fields_set(path, rows):
    s = list(EVERY_SEARCH)
    if rows:
        s.append("emit_list_ms")
    if path != "planes":
        s.append("v_count_ms")
        if rows:
            s.append("v_emit_ms")
    if path == "cluster":
        s.append("v_templates_ms")
        if rows:
            s.append("v_emit_rows_ms")
    return s


def _check_timing(name, path, t, wall, shared_stamps):
    tm = t.timing
    print(name, {k: round(tm[k], 5) for k in FIELDS}, "wall_ms", round(wall, 4), "rows", t.n_rows)
    want = _fields_set(path, t.n_rows)
    for k in FIELDS:
        if k in want:
            assert math.isfinite(tm[k]) and tm[k] > 0, k
            assert tm[k] <= wall, k  # (total_ms is the one the issue names; no interval of a call is longer than the call)
        else:
            assert tm[k] == 0, k
    if path == "cluster":
        assert tm["v_templates_ms"] <= tm["v_count_ms"] <= tm["count_ms"]
        if t.n_rows:
            assert tm["v_emit_rows_ms"] <= tm["emit_ms"]
    elif path == "words":
        assert tm["v_count_ms"] <= tm["count_ms"]
    parts, total = tm["count_ms"] + tm["offsets_ms"] + tm["emit_ms"], tm["total_ms"]
    assert parts <= total * (1 + F32_SUM)
    if shared_stamps:  # a speculative emit: the scan ends where the emit begins, on one stamp
        assert abs(parts - total) <= total * F32_SUM


# ---- 1: every path and flow -------------------------------------------------------------------------------------------------
CASES = [(p, f) for p in ("planes", "words", "cluster") for f in ("fresh", "speculative", "refused")] + [("cluster", "retry")]


@pytest.mark.parametrize("path,flow", CASES, ids=[f"{p}-{f}" for p, f in CASES])
def test_timing_fields(path, flow, monkeypatch):
    if path == "words":
        monkeypatch.setenv("HAWK_VIEW_SEARCH", "words")
    b = _Both(_few_variants_panel(seed=9201))
    try:
        if flow == "retry":  # one template row reserved: the first attempt overflows and the call runs a second one
            monkeypatch.setenv("HAWK_CLUSTER_ROWS0", "1")
        t, wall = _search(b, path, "NGG")
        if flow == "speculative":
            t, wall = _search(b, path, "NGG")
        elif flow == "refused":  # a one-base PAM behind NGG: the speculative emit is refused for capacity and runs again
            narrow = t.n_rows
            t, wall = _search(b, path, "N")
            assert t.n_rows > 4 * narrow
        assert t.n_rows > 0
        _check_timing(f"{path}/{flow}", path, t, wall, shared_stamps=flow == "speculative")
    finally:
        b.close()


# ---- 2: back to back, and a search of no rows ---------------------------------------------------------------------------------
def test_second_search_shows_nothing_of_the_first():
    """`N` (every position of both strands) and then NGG on one view, at once: every interval of the second call fits the second
    call's wall time, which an interval that began at a stamp of the first call would not (the first call, with its download, lies
    in between)"""
    b = _Both(_few_variants_panel(seed=9202))
    try:
        t1, wall1 = _search(b, "cluster", "N")
        _check_timing("first (N)", "cluster", t1, wall1, shared_stamps=False)
        t2, wall2 = _search(b, "cluster", "NGG")
        assert 0 < t2.n_rows < t1.n_rows
        _check_timing("second (NGG)", "cluster", t2, wall2, shared_stamps=True)
        _same_rows(b.planes("NGG"), t2)
    finally:
        b.close()


def _no_rows_panel():
    """no GG and no CC anywhere, and four A -> T SNVs, which make none: NGG has no hit on any row"""
    p = _panel(9203, 4_000, 2, edit=lambda s, base: _scrub(s, 0, len(s)))
    made, i = 0, 1_200
    while made < 4:
        if p.seq[i] == "A":
            p.snv(i, {made}, shift=3)
            made, i = made + 1, i + 500
        i += 1
    return p.region()


def test_search_of_no_rows_sets_the_fields_it_always_set():
    b = _Both(_no_rows_panel())
    try:
        for name in ("no rows, fresh", "no rows, speculative"):
            t, wall = _search(b, "cluster", "NGG")
            assert t.n_rows == 0
            _check_timing(name, "cluster", t, wall, shared_stamps=name.endswith("speculative"))
    finally:
        b.close()


# ---- 3: the build's time ------------------------------------------------------------------------------------------------------
def _check_build(name, st, wall):
    print(name, "build_ms", round(st["build_ms"], 5), "wall_ms", round(wall, 4), st)
    assert st["usable"] and st["status"] == 0, st
    assert math.isfinite(st["build_ms"]) and 0 < st["build_ms"] <= wall


def test_build_ms():
    b = _Both(_few_variants_panel(seed=9204))
    try:
        for it in range(2):
            _none, wall = _timed(b.ds.plan.rebuild_dictionary)
            _check_build(f"rebuild {it}", b.ds.plan.cluster_stats(), wall)
    finally:
        b.close()


def test_build_ms_of_a_repeated_attempt():
    """the panel of test_gpu_vsearch.test_cluster_dictionary_outgrows_its_first_hash_table - the one route the product library has to
    a repeated attempt: the first build of a plan of private variants (a rebuild sizes its table from the first build's count and is
    not repeated).  The repeat clears the result block and cuts no rows again: build_ms runs from the first attempt's begin."""
    reg = synth.make_region(9001, "chrU", 2_050_000, 20_000, 2_020_000)
    synth.add_phased_variants(reg, 9002, 400_000, 8, frac_snv=0.9, frac_del=0.05, max_indel=2, af_min=1 / 16, af_max=1 / 16)
    ds, _info, _ms, _kept = expand_on_device(reg, 3, keep_plan=True)
    try:
        _view, wall = _timed(ds.plan.view)  # the first build
        st = ds.plan.cluster_stats()
        assert st["distinct"] > 1 << max(16, (st["instances"] // 2 - 1).bit_length()), st  # more clusters than the first table's slots
        _check_build("repeated attempt", st, wall)
        _none, wall = _timed(ds.plan.rebuild_dictionary)
        _check_build("rebuild behind it", ds.plan.cluster_stats(), wall)
    finally:
        ds.plan.close()
        ds.close()


# ---- 4: the overlap shapes, every flow on one view ------------------------------------------------------------------------------
def _ref_long_panel():
    """60 kb of REF against two private SNVs (test_side_outlasts_main_and_the_next_call_follows_at_once)"""
    p = _panel(9001, 60_000, 2)
    p.snv(20_000, {0})
    p.snv(41_000, {3})
    return p.region()


@pytest.mark.parametrize("shape", ["ref_long", "clusters_long", "retry"])
def test_overlap_shapes(shape, monkeypatch):
    b = _Both({"ref_long": _ref_long_panel, "clusters_long": _crowded_panel, "retry": _few_variants_panel}[shape]())
    try:
        if shape == "retry":
            monkeypatch.setenv("HAWK_CLUSTER_ROWS0", "1")
        want = b.planes("NGG")
        for name in ("fresh", "speculative"):
            t, wall = _search(b, "cluster", "NGG")
            _same_rows(want, t)
            _check_timing(f"{shape}/{name}", "cluster", t, wall, shared_stamps=name == "speculative")
        wide, wall = _search(b, "cluster", "N")  # ... and a refused speculative emit: both forks and joins twice in one call
        _same_rows(b.planes("N"), wide)
        _check_timing(f"{shape}/refused", "cluster", wide, wall, shared_stamps=False)
    finally:
        b.close()
