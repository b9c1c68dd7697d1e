// hawk_resolve.hip - the unphased branch of retrieve_guides (search_guides.py:463-480) and remove_redundant_guides (340-369) on
// the guide table in HBM: k_ur_refkeys + a radix sort list REF's rows by (start, strand); k_ur_count takes every row's counts
// after the PAM re-check and after the redundancy rule and raises the declines; an exclusive scan turns the kept counts into
// offsets; k_ur_fill writes kept guide o as (source row, five window slices), one thread per output.  Every rule is a function of
// hawk_resolve.h, which hawk_host_resolve_unphased applies on the host.  Integer only; the digit loops diverge by nature (a
// lane's trip count is its row's W, the work per position depends on whether the position is ambiguous).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>

#include "hawk_device.h"

__device__ __forceinline__ UrRow ur_load(const UrDev& d, uint64_t i) {
  UrRow r;
  r.hap = gc_hap(d.c, i); r.pos = gc_pos(d.c, i); r.strand = gc_strand(d.c, i); r.flags = gc_flags(d.c, i);
  r.hap_len = r.hap < d.n_hap ? d.hap_len[r.hap] : 0u;
#pragma unroll
  for (int pl = 0; pl < UR_PLANES; ++pl) r.win[pl] = gc_win(d.c, pl, i);
  return r;
}

// The REF guide that shares (start, strand) with row i, if one exists: REF's row there (flags bit 0 says it has one; the sorted
// list says which) must itself be valid and keep its PAM.  True: refwin holds its window's planes.
__device__ __forceinline__ bool ur_partner(const UrDev& d, uint64_t i, const UrRow& row, uint64_t* refwin) {
  if (!(row.flags & 1u) || (row.hap < d.n_hap && d.is_ref[row.hap])) return false;
  const uint64_t want = (uint64_t)gc_start(d.c, i) * 2u + row.strand;
  uint64_t lo = 0, hi = d.n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (d.ref_key[mid] < want) lo = mid + 1; else hi = mid;
  }
  if (lo >= d.n || d.ref_key[lo] != want) return false;
  const UrRow pr = ur_load(d, d.ref_row[lo]);
  UrCounts pc;
  if (ur_counts(pr, d.g, d.al, pr.win, false, &pc) != UR_DECL_NONE || pc.total == 0) return false;  // (a decline there is raised by REF's own thread)
#pragma unroll
  for (int pl = 0; pl < 4; ++pl) refwin[pl] = pr.win[pl];
  return true;
}

__global__ __launch_bounds__(256) void k_ur_refkeys(UrDev d, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  const uint32_t h = gc_hap(d.c, i);
  key[i] = (h < d.n_hap && d.is_ref[h]) ? (uint64_t)gc_start(d.c, i) * 2u + gc_strand(d.c, i) : UR_SAT;
  val[i] = (uint32_t)i;
}

// One thread per row.  decline: atomicMin of row << 8 | reason, so the FIRST declining row is reported whatever the schedule.
// totals[0] += resolved, totals[1] += kept (a wave's sum, one atomic per wave).
__global__ __launch_bounds__(256) void k_ur_count(UrDev d, uint32_t* __restrict__ n_resolved, uint32_t* __restrict__ n_kept,
                                                  unsigned long long* __restrict__ decline, unsigned long long* __restrict__ totals) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long res = 0, kept = 0;
  if (i < d.n) {
    const UrRow row = ur_load(d, i);
    uint64_t refwin[4] = {0, 0, 0, 0};
    const bool has = ur_partner(d, i, row, refwin);
    UrCounts c;
    int why = ur_counts(row, d.g, d.al, refwin, has, &c);
    const bool is_ref = row.hap < d.n_hap && d.is_ref[row.hap];
    if (!why && is_ref && c.total > 1) why = UR_DECL_REF_AMBIG;
    if (!why && c.total > UR_MAX_ROW) why = UR_DECL_ROW_SIZE;
    if (why) {
      atomicMin(decline, (unsigned long long)i << 8 | (unsigned long long)why);
      c.total = 0; c.drop = 0;
    }
    res = c.total; kept = c.total - c.drop;
    n_resolved[i] = (uint32_t)res;
    n_kept[i] = (uint32_t)kept;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) { res += __shfl_down(res, off, 64); kept += __shfl_down(kept, off, 64); }
  if ((threadIdx.x & 63) == 0 && (res | kept)) { atomicAdd(&totals[0], res); atomicAdd(&totals[1], kept); }
}

// One thread per kept guide of the batch: output o0 + t lies in the source row r with offsets[r] <= o < offsets[r + 1] (rows
// [r0, r1) make the batch).  The stores of a wave are 64 consecutive words of each of the six output arrays.
__global__ __launch_bounds__(256) void k_ur_fill(UrDev d, const uint32_t* __restrict__ n_resolved, const uint32_t* __restrict__ n_kept,
                                                 const uint64_t* __restrict__ offsets, uint64_t r0, uint64_t r1, uint64_t o0, uint64_t n_out,
                                                 uint32_t* __restrict__ out_src, uint64_t* __restrict__ out_win, uint64_t out_stride) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_out || t >= out_stride) return;
  const uint64_t o = o0 + t;
  uint64_t lo = r0, hi = r1;  // last r in [r0, r1) with offsets[r] <= o
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= o) lo = mid; else hi = mid;
  }
  const UrRow row = ur_load(d, lo);
  uint64_t refwin[4] = {0, 0, 0, 0};
  const bool has = ur_partner(d, lo, row, refwin);
  const uint32_t total = n_resolved[lo], kept = n_kept[lo];
  const uint64_t jk = o - offsets[lo];
  uint64_t w[UR_PLANES] = {0, 0, 0, 0, 0};
  if (jk < kept) ur_unrank(row, d.g, d.al, refwin, has, total, total - kept, (uint32_t)jk, w);
  out_src[t] = (uint32_t)lo;
#pragma unroll
  for (int pl = 0; pl < UR_PLANES; ++pl) out_win[(size_t)pl * out_stride + t] = w[pl];
}

struct UrWiden {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

size_t hawk_ur_temp_bytes(uint64_t n) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 64,
                                  (hipStream_t)0);
  auto in = rocprim::make_transform_iterator((const uint32_t*)nullptr, UrWiden());
  (void)rocprim::exclusive_scan(nullptr, b, in, (uint64_t*)nullptr, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), (hipStream_t)0);
  return std::max(a, b);
}

// keys / vals: [2][n] ping-pong; the sorted list ends up in keys + n / vals + n
int hawk_launch_ur_refsort(hipStream_t st, const UrDev& d, void* temp, size_t temp_bytes, uint64_t* keys, uint32_t* vals) {
  if (!d.n) return 0;
  hipLaunchKernelGGL(k_ur_refkeys, dim3((unsigned)((d.n + 255) / 256)), dim3(256), 0, st, d, keys, vals);
  size_t tb = temp_bytes;
  return rocprim::radix_sort_pairs(temp, tb, keys, keys + d.n, vals, vals + d.n, (size_t)d.n, 0, 64, st) == hipSuccess ? 0 : -2;
}

void hawk_launch_ur_count(hipStream_t st, const UrDev& d, uint32_t* n_resolved, uint32_t* n_kept, unsigned long long* decline,
                          unsigned long long* totals) {
  if (!d.n) return;
  hipLaunchKernelGGL(k_ur_count, dim3((unsigned)((d.n + 255) / 256)), dim3(256), 0, st, d, n_resolved, n_kept, decline, totals);
}

// offsets[n + 1] <- exclusive 64-bit sums of n_kept[0 .. n] (n_kept[n] must be 0: offsets[n] is the total)
int hawk_launch_ur_offsets(hipStream_t st, const uint32_t* n_kept, uint64_t n, void* temp, size_t temp_bytes, uint64_t* offsets) {
  size_t tb = temp_bytes;
  auto in = rocprim::make_transform_iterator(n_kept, UrWiden());
  return rocprim::exclusive_scan(temp, tb, in, offsets, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>(), st) == hipSuccess ? 0 : -2;
}

void hawk_launch_ur_fill(hipStream_t st, const UrDev& d, const uint32_t* n_resolved, const uint32_t* n_kept, const uint64_t* offsets, uint64_t r0,
                         uint64_t r1, uint64_t o0, uint64_t n_out, uint32_t* out_src, uint64_t* out_win, uint64_t out_stride) {
  if (!n_out) return;
  hipLaunchKernelGGL(k_ur_fill, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, d, n_resolved, n_kept, offsets, r0, r1, o0, n_out, out_src,
                     out_win, out_stride);
}
