"""Run by tests/test_gpu_scan_family.py in a process of its own, one per group, with CRISPRHAWK_HIP_LIB naming libhawk_hip_hooks.so:
only that library has hawk_hook_mscan / hawk_hook_scan2_u32 (hawk_hooks_scan.hip), which run hawk_launch_mscan and
hawk_launch_scan2_u32 on buffers of this script's making.  The product reaches those launchers only through whole searches and
dictionary builds, i.e. at small sizes and on aligned pool blocks; here every route of the offset scan runs at the sizes where its
loops take another trip (tests/scan_refs.py names each case and what it is for), with counts whose total is far beyond 32 bits.

Every case asserts, all of it == on integers: the route the library took, the offsets against np.cumsum in uint64, the 16 guard
words behind the last offset untouched, and the totals.

usage: hooks_scan_check.py <group>      (m23 | wide | unaligned | m2_shards | m2_chunks | scan2)"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "crispr-hawk_amd"), HERE]

import scan_refs as sc  # noqa: E402
from crisprhawk_hip import _lib  # noqa: E402


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bind():
    L = _lib.lib()
    L.hawk_hook_mscan.restype = C.c_int
    L.hawk_hook_mscan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int)]
    L.hawk_hook_scan2_u32.restype = C.c_int
    L.hawk_hook_scan2_u32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def mscan(L, ctx, counts, shards, shift):
    """-> (offsets u64 [n], guard u64 [16], totals (4 ints), route)"""
    n = len(counts)
    off, guard, tot = np.zeros(n, dtype=np.uint64), np.zeros(sc.GUARD, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    route = C.c_int(-1)
    rc = L.hawk_hook_mscan(ctx, _ptr(counts), n, _ptr(shards) if shards is not None else None, shift[0], shift[1], _ptr(off), _ptr(guard),
                           _ptr(tot), C.byref(route))
    _lib.check(rc, "hawk_hook_mscan")
    return off, guard, tuple(int(x) for x in tot), route.value


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    return f"{len(bad)} of {len(want)} differ, the first at {i}: {int(got[i])} for {int(want[i])}"


def run_mscan(group) -> int:
    L = bind()
    ctx = _lib.context(0)
    # the refusal (no launch): n == 0
    one = np.ones(1, dtype=np.uint32)
    route = C.c_int(-1)
    out = np.zeros(sc.GUARD, dtype=np.uint64)
    assert L.hawk_hook_mscan(ctx, _ptr(one), 0, None, 0, 0, _ptr(out), _ptr(out), _ptr(out), C.byref(route)) == _lib.HAWK_E_INVALID
    done = 0
    for case in sc.CASES[group]:
        sc.check_case(case)
        n = case["n"]
        shards = sc.shard_panel(n) if case["shards"] else None
        for panel in case["panels"]:
            label = (group, n, panel, case["shift"])
            counts = sc.counts_panel(panel, n)
            want, want_tot = sc.reference(counts, shards)
            off, guard, tot, route = mscan(L, ctx, counts, shards, case["shift"])
            print(f"{label}: route {route}, n_keep {tot[0]} (reference {want_tot[0]})", flush=True)
            assert route == sc.ROUTE_CODE[case["route"]], (label, route)
            assert np.array_equal(off, want), (label, first_difference(off, want))
            assert (guard == np.uint64(sc.SENTINEL64)).all(), (label, [hex(int(g)) for g in guard])
            assert tot == want_tot, (label, tot, want_tot)
            done += 1
    return done


def run_scan2() -> int:
    L = bind()
    ctx = _lib.context(0)
    done = 0
    for n in sc.SCAN2_N:
        a, b = sc.scan2_counts(n)
        for n_desc in sc.SCAN2_NDESC:
            desc = sc.scan2_desc(n_desc) if n_desc else None
            want_a, want_b, want_bits = sc.scan2_reference(a, b, desc)
            off_a = np.zeros(n + 1 + sc.GUARD, dtype=np.uint32)
            off_b = np.zeros(n + 1 + sc.GUARD, dtype=np.uint32)
            bits = np.zeros((n_desc or 0) // 32 + 2, dtype=np.uint32)
            rc = L.hawk_hook_scan2_u32(ctx, _ptr(a), _ptr(b), n, _ptr(desc) if n_desc else None, n_desc or 0, _ptr(off_a), _ptr(off_b), _ptr(bits))
            _lib.check(rc, "hawk_hook_scan2_u32")
            label = ("scan2", n, n_desc)
            for got, want in ((off_a, want_a), (off_b, want_b)):
                assert np.array_equal(got[:n + 1], want), (label, first_difference(got[:n + 1], want))
                assert (got[n + 1:] == sc.SENTINEL32).all(), (label, got[n + 1:].tolist())
            if n_desc:
                assert np.array_equal(bits[:-1], want_bits), (label, first_difference(bits[:-1], want_bits))
                assert int(bits[-1]) == sc.SENTINEL32, (label, hex(int(bits[-1])))
            done += 1
    print(f"scan2: {done} launches", flush=True)
    return done


def main() -> int:
    assert os.path.basename(_lib.LIB_PATH) == "libhawk_hip_hooks.so", _lib.LIB_PATH
    group = sys.argv[1]
    assert group in sc.GROUPS, group
    done = run_scan2() if group == "scan2" else run_mscan(group)
    assert done
    print(f"hooks ok: {group} {done} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
