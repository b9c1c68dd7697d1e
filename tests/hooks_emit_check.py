"""Run by tests/test_gpu_emit_handover.py in a process of its own, one per group, with CRISPRHAWK_HIP_LIB naming libhawk_hip_hooks.so:
only that library has hawk_hook_cs_emit / hawk_hook_cs_emit_geometry (hawk_hooks_emit.hip), which run k_cs_emit_rows
(hawk_launch_cs_emit_rows behind hawk_launch_mscan over the wave sums, as a search queues them) on instance records and template
rows of this script's making.  A record is what k_cs_count leaves per instance: {rows, first template row, haplotype row <<
HAWK_ROW_HAP_SHIFT, position}.

The reference is a numpy gather-copy: row k of instance i = template row tb[i] + k, word 0 plus the position (an int32 add,
wrapping), word 1 ORed with the shifted haplotype row.  Every comparison is == on the 16 words of every row; the 16 guard rows
behind the table's capacity must keep the sentinel.  W (instances per wave) and C (rows per chunk) come from the library, so the
seams follow the instantiation the launcher keeps.

usage: hooks_emit_check.py <group>      (n_inst | wave_totals | span | capacity)"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd"), HERE]

from crisprhawk_hip import _lib  # noqa: E402

GROUPS = ("n_inst", "wave_totals", "span", "capacity")
GUARD_ROWS = 16
SENTINEL32 = 0xA5A5A5A5


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bind():
    L = _lib.lib()
    L.hawk_hook_cs_emit_geometry.restype = C.c_int
    L.hawk_hook_cs_emit_geometry.argtypes = [C.POINTER(C.c_uint32)] * 4
    L.hawk_hook_cs_emit.restype = C.c_int
    L.hawk_hook_cs_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_int)]
    return L


def geometry(L):
    w, c, sh, mh = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.check(L.hawk_hook_cs_emit_geometry(C.byref(w), C.byref(c), C.byref(sh), C.byref(mh)), "hawk_hook_cs_emit_geometry")
    return w.value, c.value, sh.value, mh.value


def template_rows(rng, n):
    """n rows of 16 words: word 0 over the whole 32-bit range (so the position add wraps and carries into bit 31), word 1 with the
    haplotype bits clear, as k_cs_templates leaves it; the first rows pin the carries by hand"""
    t = rng.integers(0, 1 << 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
    t[:, 1] &= np.uint32(0x1FF)
    t[0, 0], t[1, 0], t[2, 0], t[3, 0] = 0x7FFFFFFF, 0, 0xFFFFFFFF, 0x80000000
    return t


def records(rng, cnt, n_trows, hap_shift, max_hap):
    """one record per instance for the row counts `cnt`: template stretches anywhere in the rows, haplotype rows up to the last
    one a packed row can name, positions over the whole int32 range (negative ones included)"""
    cnt = np.asarray(cnt, dtype=np.uint32)
    n = len(cnt)
    tb = (rng.random(n) * (n_trows - cnt.astype(np.int64))).astype(np.uint32)
    hap = rng.integers(0, max_hap, size=n, dtype=np.uint32)
    hap[rng.random(n) < 0.1] = max_hap - 1
    pos = rng.integers(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)
    small = rng.random(n) < 0.5
    pos[small] = rng.integers(-3, 4, size=int(small.sum()))
    tb[small & (cnt <= 1)] %= 4  # the hand-made carries: 0x7fffffff + 1, 0 - 1, 0xffffffff + 1, 0x80000000 - 1 among them
    rec = np.empty((n, 4), dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = cnt, tb, hap << np.uint32(hap_shift), pos.view(np.uint32)
    return rec


def reference(rec, trows):
    cnt = rec[:, 0].astype(np.int64)
    total = int(cnt.sum())
    first = np.cumsum(cnt) - cnt
    k = np.arange(total, dtype=np.int64) - np.repeat(first, cnt)
    out = trows[np.repeat(rec[:, 1].astype(np.int64), cnt) + k].copy()
    out[:, 0] = ((out[:, 0].astype(np.int64) + np.repeat(rec[:, 3].view(np.int32).astype(np.int64), cnt)) & 0xFFFFFFFF).astype(np.uint32)
    out[:, 1] |= np.repeat(rec[:, 2], cnt)
    return out


def emit(L, ctx, rec, trows, cap, t_count=None, t_cap=None):
    """-> (table u32 [cap][16], guard u32 [16][16], status)"""
    rec = np.ascontiguousarray(rec)
    table = np.zeros((max(cap, 1), 16), dtype=np.uint32)
    guard = np.zeros((GUARD_ROWS, 16), dtype=np.uint32)
    status = C.c_int(12345)
    t_cap = len(trows) if t_cap is None else t_cap
    t_count = len(trows) if t_count is None else t_count
    rc = L.hawk_hook_cs_emit(ctx, _ptr(rec), len(rec), _ptr(trows), len(trows), t_count, t_cap, cap, _ptr(table), _ptr(guard), C.byref(status))
    _lib.check(rc, "hawk_hook_cs_emit")
    return table[:cap], guard, status.value


def first_difference(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    i = int(bad[0])
    return f"{len(bad)} of {len(want)} rows differ, the first at {i}: {[hex(int(x)) for x in got[i]]} for {[hex(int(x)) for x in want[i]]}"


def check_full(L, ctx, label, rec, trows):
    """capacity = the row total: every row as the reference has it, status 0, guard untouched"""
    want = reference(rec, trows)
    table, guard, status = emit(L, ctx, rec, trows, len(want))
    print(f"{label}: {len(rec)} instances, {len(want)} rows, status {status}", flush=True)
    assert status == 0, (label, status)
    assert np.array_equal(table, want), (label, first_difference(table, want))
    assert (guard == np.uint32(SENTINEL32)).all(), (label, "guard rows written")
    return want


def wave_counts(rng, W, total, zero_ends=True):
    """row counts of one wave's W instances with the given total; the wave's first and last instance have none"""
    cnt = np.zeros(W, dtype=np.uint32)
    if total:
        inner = np.arange(1, W - 1) if zero_ends else np.arange(W)
        np.add.at(cnt, rng.choice(inner, size=total), 1)
    return cnt


def run(group) -> int:
    L = bind()
    ctx = _lib.context(0)
    W, CH, hap_shift, max_hap = geometry(L)
    print(f"instances per wave {W}, rows per chunk {CH}, haplotype shift {hap_shift}, haplotype rows < {max_hap}", flush=True)
    assert W % 64 == 0 and W >= 64 and CH >= 16
    rng = np.random.default_rng(20240611)
    n_trows = max(4096, 4 * CH)
    trows = template_rows(rng, n_trows)
    done = 0
    if group == "n_inst":
        for n in sorted({1, 63, 64, 65, W - 1, W, W + 1, 4 * W - 1, 4 * W, 4 * W + 1}):
            cnt = rng.integers(0, 6, size=n).astype(np.uint32)
            cnt[-1] = 3  # the last instance, beside the clamped lanes, has rows
            check_full(L, ctx, ("n_inst", n), records(rng, cnt, n_trows, hap_shift, max_hap), trows)
            done += 1
        # the refusals of the entry point (no launch)
        one = records(rng, [1], n_trows, hap_shift, max_hap)
        out, st = np.zeros((GUARD_ROWS, 16), dtype=np.uint32), C.c_int(0)
        assert L.hawk_hook_cs_emit(ctx, _ptr(one), 0, _ptr(trows), n_trows, 0, n_trows, 1, _ptr(out), _ptr(out), C.byref(st)) == _lib.HAWK_E_INVALID
        bad = one.copy()
        bad[0, 1] = n_trows  # a template stretch past the rows
        assert L.hawk_hook_cs_emit(ctx, _ptr(bad), 1, _ptr(trows), n_trows, 0, n_trows, 1, _ptr(out), _ptr(out), C.byref(st)) == _lib.HAWK_E_INVALID
    elif group == "wave_totals":
        # a wave's row total on either side of one, two and three chunks (both register buffers, the loop's odd and even exits),
        # between two waves with rows; total 0 is the wave of no rows between them.  Instances of no rows at the wave's ends.
        for total in (0, 1, CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH + 1):
            cnt = np.concatenate([wave_counts(rng, W, CH + 5), wave_counts(rng, W, total), wave_counts(rng, W, 2 * CH + 3, zero_ends=False)])
            check_full(L, ctx, ("wave_total", total), records(rng, cnt, n_trows, hap_shift, max_hap), trows)
            done += 1
        # ... and as the table's last wave, cut short by the instance count
        for total in (1, CH, 2 * CH + 1):
            cnt = np.concatenate([wave_counts(rng, W, 7), wave_counts(rng, W, total)[: W - 37]])
            cnt[-1] += W  # what the cut took stays out; the last instance has rows
            check_full(L, ctx, ("last_wave_total", total), records(rng, cnt, n_trows, hap_shift, max_hap), trows)
            done += 1
    elif group == "span":
        # one instance of 2 C + 7 rows: a single instance spans three chunks; alone in its wave, then among others
        for others in (0, 2):
            cnt = np.full(2 * W, others, dtype=np.uint32)
            cnt[W // 2 + 1] = 2 * CH + 7
            cnt[W + 5] = 2 * CH + 7
            rec = records(rng, cnt, n_trows, hap_shift, max_hap)
            rec[W // 2 + 1, 2] = np.uint32((max_hap - 1) << hap_shift)  # the last haplotype row a packed row can name
            rec[W // 2 + 1, 3] = np.int32(-(1 << 31)).view(np.uint32)
            want = check_full(L, ctx, ("span", others), rec, trows)
            assert (want[:, 1] >> np.uint32(hap_shift)).max() == max_hap - 1
            done += 1
    elif group == "capacity":
        cnt = np.concatenate([wave_counts(rng, W, CH + 9), wave_counts(rng, W, 0), wave_counts(rng, W, 2 * CH + 1), wave_counts(rng, W, 0)])
        rec = records(rng, cnt, n_trows, hap_shift, max_hap)
        want = check_full(L, ctx, ("capacity", "exact"), rec, trows)
        done += 1
        # one row short: the wave that would write past the capacity writes nothing and says so, the waves in front are complete
        table, guard, status = emit(L, ctx, rec, trows, len(want) - 1)
        print(f"capacity one short: status {status}", flush=True)
        assert status == _lib.HAWK_E_CAPACITY, status
        assert (guard == np.uint32(SENTINEL32)).all(), "guard rows written"
        head = CH + 9
        assert np.array_equal(table[:head], want[:head]), first_difference(table[:head], want[:head])
        assert (table[head:] == np.uint32(SENTINEL32)).all(), "the refused wave wrote rows"
        done += 1
        # the template counter above its reservation (the search that is rerun): nothing written at all
        table, guard, status = emit(L, ctx, rec, trows, len(want), t_count=n_trows + 1, t_cap=n_trows)
        print(f"template overflow: status {status}", flush=True)
        assert status == 0, status
        assert (table == np.uint32(SENTINEL32)).all() and (guard == np.uint32(SENTINEL32)).all(), "rows written behind a template overflow"
        done += 1
        # ... and exactly at it: the table
        table, guard, status = emit(L, ctx, rec, trows, len(want), t_count=n_trows, t_cap=n_trows)
        assert status == 0 and np.array_equal(table, want) and (guard == np.uint32(SENTINEL32)).all()
        done += 1
    return done


def main() -> int:
    assert os.path.basename(_lib.LIB_PATH) == "libhawk_hip_hooks.so", _lib.LIB_PATH
    group = sys.argv[1]
    assert group in GROUPS, group
    done = run(group)
    assert done
    print(f"hooks ok: {group} {done} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
