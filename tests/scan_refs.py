"""References and cases for the offset scans called on their own (tests/hooks_scan_check.py through the hooks library's
hawk_hook_mscan / hawk_hook_scan2_u32; tests/test_scan_refs.py checks everything here without a GPU):

  * hawk_launch_mscan (hawk_search.hip): u32 counts -> u64 exclusive offsets + totals.  The reference is np.cumsum in uint64; with
    shard sums n_cand / n_hits are the sums of the even / odd shard entries, without them 0; n_keep_fwd is always 0.
  * hawk_launch_scan2_u32 (hawk_meta.hip): two u32 count arrays -> n + 1 u32 offsets each, and the bitmap of desc != 0.

CASES names, per group, every (n, shard sums, pointer shifts, panels) with the route and the figures it is there for; a case whose n
drifts off its seam fails in check_case().  emulate() restates the kernels' arithmetic in numpy - the 32-bit scan inside a workgroup
tile, and the wave reductions either as they were (two 32-bit halves summed apart: the carries out of the low half are lost) or
carry-safe (wave_sum64) - which is how the CPU test shows that the `big` panel tells the two apart and `product` does not."""
import zlib

import numpy as np

import search_refs as sr

U32, U64 = np.uint32, np.uint64
SENTINEL64 = 0xA5A5A5A5A5A5A5A5  # what the hooks fill every output word with
SENTINEL32 = 0xA5A5A5A5
GUARD = 16                       # guard words behind the last element
ROUTE_CODE = {"ONE": 0, "M1_M23": 1, "WIDE": 2, "M1_M2_M3": 3}  # HAWK_MSCAN_* (hawk_device.h)
MAX_COUNT = 65_536               # rows of one tile: the largest count the product produces
PANELS = ("ones", "product", "edges", "big")
BIG_MIN_N = 262_145


def _seed(*key) -> int:
    return zlib.crc32(":".join(str(k) for k in key).encode())


def counts_panel(panel: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(_seed(panel, n))
    if panel == "ones":  # offsets == arange
        return np.ones(n, dtype=U32)
    if panel == "product":  # today's domain: the total stays below 2^32
        return rng.integers(0, min(MAX_COUNT, (2 ** 32 - 1) // n) + 1, n, dtype=np.int64).astype(U32)
    if panel == "edges":  # the first and the last entry of every workgroup tile (1024, and with them 4096), and the last count
        c = np.zeros(n, dtype=U32)
        c[0::1024] = MAX_COUNT
        c[1023::1024] = MAX_COUNT
        c[n - 1] = MAX_COUNT
        return c
    if panel == "big":  # every count in the product's range, the total far beyond 32 bits
        assert n >= BIG_MIN_N
        return rng.integers(0, MAX_COUNT + 1, n, dtype=np.int64).astype(U32)
    raise KeyError(panel)


def shard_panel(n: int) -> np.ndarray:
    """256 (candidates, hits) pairs below 2^40"""
    return np.random.default_rng(_seed("shards", n)).integers(0, 2 ** 40, 512, dtype=np.int64).astype(U64)


def reference(counts: np.ndarray, shards) -> tuple:
    """-> (offsets u64 [n], (n_keep, n_keep_fwd, n_cand, n_hits))"""
    inc = np.cumsum(counts, dtype=U64)
    off = inc - counts.astype(U64)
    cand, hits = (int(shards[0::2].sum(dtype=U64)), int(shards[1::2].sum(dtype=U64))) if shards is not None else (0, 0)
    return off, (int(inc[-1]), 0, cand, hits)


# ---- the kernels' arithmetic -------------------------------------------------------------------------------------------------
def _wave_sum(v: np.ndarray, carry_safe: bool) -> np.ndarray:
    """v [..., 64] u64 -> the wave's sum: exact modulo 2^64, or the two 32-bit halves summed apart, each modulo 2^32"""
    if carry_safe:
        return v.sum(-1, dtype=U64)
    m = U64(0xFFFFFFFF)
    lo = (v & m).sum(-1, dtype=U64) & m
    hi = (v >> U64(32)).sum(-1, dtype=U64) & m
    return lo + (hi << U64(32))


def emulate(counts: np.ndarray, route: str, carry_safe: bool) -> tuple:
    """k_mscan1 + k_mscan23, k_mscan1w + k_mscan23w or k_mscan1 / 2 / 3 thread by thread -> (offsets u64 [n], n_keep)"""
    assert route in ("M1_M23", "WIDE", "M1_M2_M3")
    n = len(counts)
    tile = sr.MSW_TILE if route == "WIDE" else sr.MS_TILE
    ipt, nb = tile // 256, -(-n // tile)
    c = np.zeros(nb * tile, dtype=U32)
    c[:n] = counts
    th = c.reshape(nb, 256, ipt)  # [workgroup][thread][its consecutive counts]
    # first kernel: a thread's counts in 64 bits, the wave's sum, the four waves added by 64-bit atomics
    partial = _wave_sum(th.sum(-1, dtype=U64).reshape(nb, 4, 64), carry_safe).sum(-1, dtype=U64)
    if route == "M1_M2_M3":  # k_mscan2: 64-bit throughout
        pre = np.cumsum(partial, dtype=U64) - partial
        n_keep = int(partial.sum(dtype=U64))
    else:  # every workgroup adds up the partials before its own: thread t takes partial[t], partial[t + 256], ...
        rows = -(-nb // 256)
        P = np.zeros(rows * 256, dtype=U64)
        P[:nb] = partial
        P = P.reshape(rows, 256)
        C0 = np.cumsum(P, axis=0, dtype=U64) - P
        b = np.arange(nb)
        q, r = b // 256, b % 256
        val = C0[q] + np.where(np.arange(256)[None, :] < r[:, None], P[q], U64(0))
        pre = _wave_sum(val.reshape(nb, 4, 64), carry_safe).sum(-1, dtype=U64)
    # inside the tile: block_excl_scan over the threads' sums in 32 bits, then 64-bit additions inside the thread
    tsum = th.sum(-1, dtype=U32)
    inc = np.cumsum(tsum, axis=1, dtype=U32)
    ex = (inc - tsum).astype(U64)
    inthread = np.cumsum(th, axis=-1, dtype=U64) - th
    off = (pre[:, None, None] + ex[:, :, None] + inthread).reshape(-1)[:n]
    if route != "M1_M2_M3":
        n_keep = int(pre[-1] + U64(inc[-1, -1]))
    return off, n_keep


# ---- hawk_launch_scan2_u32 -----------------------------------------------------------------------------------------------------
SCAN2_N = (1, 15, 16, 17, 16_383, 16_384, 16_385, 16_400, 32_769)
SCAN2_NDESC = (None, 1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049)


def scan2_counts(n: int) -> tuple:
    rng = np.random.default_rng(_seed("scan2", n))
    a = rng.integers(0, min(MAX_COUNT, (2 ** 32 - 1) // n) + 1, n, dtype=np.int64).astype(U32)
    b = rng.integers(0, 4, n, dtype=np.int64).astype(U32)
    return a, b


def scan2_desc(n_desc: int) -> np.ndarray:
    """64-bit describers, 0 except at 0, n_desc - 1 and both sides of every multiple of 32 (and with them of 64 and 1024); the
    values that are set have their bits in the low half, the high half or both"""
    d = np.zeros(n_desc, dtype=U64)
    at = sorted({0, n_desc - 1} | {i for k in range(32, n_desc + 1, 32) for i in (k - 1, k) if i < n_desc})
    vals = (1, 1 << 32, 1 << 63, 0xFFFFFFFFFFFFFFFF, 0x80000000)
    for j, i in enumerate(at):
        d[i] = vals[j % len(vals)]
    return d


def scan2_bits_written(n_desc: int) -> int:
    """words of the bitmap the kernel writes: it has n_desc / 32 + 1, a workgroup covers 1024 describers = 32 words, and whichever
    of its words lie inside the bitmap are written (the word behind the last describer only when a workgroup reaches it)"""
    return min(n_desc // 32 + 1, 32 * (-(-n_desc // 1024)))


def scan2_reference(a: np.ndarray, b: np.ndarray, desc) -> tuple:
    """-> (off_a u32 [n + 1], off_b u32 [n + 1], bitmap u32 [n_desc / 32 + 1] with SENTINEL32 where nothing is written, or None)"""
    def off(c):
        inc = np.cumsum(c, dtype=U64)
        assert int(inc[-1]) < 2 ** 32
        return np.concatenate(([0], inc)).astype(U32)
    bits = None
    if desc is not None:
        n_desc = len(desc)
        written = scan2_bits_written(n_desc)
        flags = np.zeros(written * 32, dtype=np.uint8)
        m = min(n_desc, written * 32)
        flags[:m] = desc[:m] != 0
        assert m == n_desc  # every describer's bit lies in a written word
        bits = np.full(n_desc // 32 + 1, SENTINEL32, dtype=U32)
        bits[:written] = np.packbits(flags, bitorder="little").view("<u4")
    return off(a), off(b), bits


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _case(n, panels, route, shards=True, shift=(0, 0), **figures):
    return dict(n=n, panels=tuple(panels), route=route, shards=shards, shift=shift, figures=figures)


ALL, PB = PANELS, ("product", "big")
CASES = {
    # k_mscan1 + k_mscan23: 3 partials; 256 (the prefix loop's single full trip); 257; 258 (a second trip); 4096 (16 trips)
    "m23": [
        _case(2_049, ALL[:3], "M1_M23", partials=3, trips=1, tail=1),
        _case(262_144, ALL[:3], "M1_M23", partials=256, trips=1, tail=1024),
        _case(262_145, ALL, "M1_M23", partials=257, trips=1, tail=1),
        _case(263_169, ALL, "M1_M23", partials=258, trips=2, tail=1),
        _case(4_194_304, ALL, "M1_M23", partials=4096, trips=16, tail=1024),
    ],
    # k_mscan1w + k_mscan23w: the last workgroup holds one count / one full thread / all but one count / every count; 4096 partials
    "wide": [
        _case(4_194_305, ALL, "WIDE", partials=1025, trips=4, tail=1),
        _case(4_194_320, ALL, "WIDE", partials=1025, trips=4, tail=16),
        _case(4_198_399, PB, "WIDE", partials=1025, trips=4, tail=4095),
        _case(4_198_400, PB, "WIDE", partials=1025, trips=4, tail=4096),
        _case(16_777_216, PB, "WIDE", partials=4096, trips=16, tail=4096),
    ],
    # the wide range with a pointer off its 16-byte boundary: k_mscan1 / 2 / 3 WITH shard sums, 5 chunks, the last of one partial
    "unaligned": [
        _case(4_194_305, PB, "M1_M2_M3", shift=s, partials=4097, chunks=5, last_chunk=1, tail=1) for s in ((1, 0), (0, 1), (1, 1))
    ],
    # beyond the wide range
    "m2_shards": [
        _case(16_777_217, PB, "M1_M2_M3", partials=16_385, chunks=17, last_chunk=1, tail=1),
    ],
    # k_mscan2's carry loop without shard sums: one full chunk; a second chunk of one partial; three chunks
    "m2_chunks": [
        _case(1_048_576, ALL, "M1_M2_M3", shards=False, partials=1024, chunks=1, last_chunk=1024, tail=1024),
        _case(1_048_577, ALL, "M1_M2_M3", shards=False, partials=1025, chunks=2, last_chunk=1, tail=1),
        _case(2_097_153, ALL, "M1_M2_M3", shards=False, partials=2049, chunks=3, last_chunk=1, tail=1),
    ],
}
GROUPS = tuple(CASES) + ("scan2",)


def check_case(case: dict) -> dict:
    """the case sits on the seam it is named after: the route and every figure, from sr.scan_route -> the route's figures"""
    r = sr.scan_route(case["n"], case["shards"], case["shift"] == (0, 0))
    assert r["route"] == case["route"], (case, r)
    for k, v in case["figures"].items():
        assert r[k] == v, (case, k, r)
    assert all(p in PANELS for p in case["panels"]) and ("big" not in case["panels"] or case["n"] >= BIG_MIN_N)
    return r
