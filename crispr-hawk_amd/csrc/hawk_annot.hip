// hawk_annot.hip - the BED annotation join: every query interval x the features of one (file, contig, label kind) -> the
// comma-joined labels of the overlapping features in file order, or "NA" (annotation.py:373-462, offtargets.py:407-444 of the
// reference: one tabix fetch + one Python join per guide / off-target row).
//
//   overlap (tabix, 0-based half-open on both sides; parity unpinned: pysam absent):  fs < qe && fe > qs
//
// Features arrive sorted by start (tabix's own precondition; the reader refuses anything else).  At create:
//   k_ann_scan1/2/3<max>   rmax[i] = max(end[0..i])  - non-decreasing, so "first feature that can still reach qs" is a binary search
//   k_ann_blockmax         bmax[b] = max(end[64 b .. 64 b + 63])
// Per query batch, in the library's count -> scan -> fill shape (no atomics for places):
//   k_ann_count            hi = first fs >= qe, lo = first rmax > qs (two binary searches), then the walk lo..hi keeping fe > qs and
//                          stepping over a whole 64-feature block whose bmax <= qs: a 2 Mb gene in front of ten thousand exons costs
//                          a query inside it one step per 64 exons, not one per exon.  Leaves the row's bytes.
//   k_ann_scan1/2/3<sum>   exclusive scan of the rows' bytes in 64 bits (a C4 column passes 2^32 bytes of text)
//   k_ann_fill             the same walk, writing labels and commas (or NA) at the row's offset
//
// One thread per query.  Every caller's neighbouring queries are neighbours on the genome (report groups come in (start, stop)
// order or nearly, the off-target table is sorted by (chrom, position)), so the lanes of a wave search and walk the same cache
// lines and their output rows are adjacent.  That is an assumption about speed alone: any order of queries gives the same rows.
#include <hip/hip_runtime.h>

#include "hawk_device.h"

#define ANN_BLOCK 256
#define ANN_IPT 8  // elements per thread in the scans: 2048 per workgroup

namespace {

template <class T, bool MAX>
__device__ inline T ann_op(T a, T b) { return MAX ? (a > b ? a : b) : (T)(a + b); }

// inclusive scan of one value per thread over the workgroup (4 waves: shuffles inside a wave, the wave totals through LDS);
// *excl = what precedes the thread, *total = the workgroup's value
template <class T, bool MAX>
__device__ inline T ann_block_scan(T v, T* lds /* [ANN_BLOCK / 64] */, T ident, T* excl, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const T o = (T)__shfl_up((long long)v, d, 64);
    if (lane >= d) v = ann_op<T, MAX>(o, v);
  }
  T before = (T)__shfl_up((long long)v, 1, 64);
  if (lane == 0) before = ident;
  if (lane == 63) lds[w] = v;
  __syncthreads();
  T add = ident, tot = ident;
  for (int k = 0; k < ANN_BLOCK / 64; ++k) {
    if (k < w) add = ann_op<T, MAX>(add, lds[k]);
    tot = ann_op<T, MAX>(tot, lds[k]);
  }
  __syncthreads();  // lds may be written again
  *excl = ann_op<T, MAX>(add, before);
  *total = tot;
  return ann_op<T, MAX>(add, v);
}

template <class T, bool MAX>
__global__ __launch_bounds__(ANN_BLOCK) void k_ann_scan1(const T* __restrict__ in, uint64_t n, T ident, T* __restrict__ partial) {
  __shared__ T lds[ANN_BLOCK / 64];
  const uint64_t base = ((uint64_t)blockIdx.x * ANN_BLOCK + threadIdx.x) * ANN_IPT;
  T acc = ident;
  for (int k = 0; k < ANN_IPT; ++k)
    if (base + k < n) acc = ann_op<T, MAX>(acc, in[base + k]);
  T excl, tot;
  (void)ann_block_scan<T, MAX>(acc, lds, ident, &excl, &tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup: partial[b] <- what precedes workgroup b, chunk after chunk with a running carry
template <class T, bool MAX>
__global__ __launch_bounds__(ANN_BLOCK) void k_ann_scan2(T* __restrict__ partial, uint64_t nb, T ident) {
  __shared__ T lds[ANN_BLOCK / 64];
  T carry = ident;
  for (uint64_t c = 0; c < nb; c += ANN_BLOCK) {
    const uint64_t i = c + threadIdx.x;
    const T v = i < nb ? partial[i] : ident;
    T excl, tot;
    (void)ann_block_scan<T, MAX>(v, lds, ident, &excl, &tot);
    if (i < nb) partial[i] = ann_op<T, MAX>(carry, excl);
    carry = ann_op<T, MAX>(carry, tot);
  }
}

// MAX: out[i] = max(in[0..i]) (inclusive).  Sum: out[i] = sum(in[0..i)) (exclusive) and out[n] = the total; in == out is allowed
// (a thread holds its elements in registers before it writes them, and no other thread reads them).
template <class T, bool MAX>
__global__ __launch_bounds__(ANN_BLOCK) void k_ann_scan3(const T* in, uint64_t n, T ident, const T* __restrict__ partial, T* out) {
  __shared__ T lds[ANN_BLOCK / 64];
  const uint64_t base = ((uint64_t)blockIdx.x * ANN_BLOCK + threadIdx.x) * ANN_IPT;
  T v[ANN_IPT];
  T acc = ident;
  for (int k = 0; k < ANN_IPT; ++k) {
    v[k] = base + k < n ? in[base + k] : ident;
    acc = ann_op<T, MAX>(acc, v[k]);
  }
  T excl, tot;
  (void)ann_block_scan<T, MAX>(acc, lds, ident, &excl, &tot);
  T run = ann_op<T, MAX>(partial[blockIdx.x], excl);  // the workgroups before, then the threads before
  for (int k = 0; k < ANN_IPT; ++k) {
    if (base + k >= n) break;
    if (MAX) {
      run = ann_op<T, MAX>(run, v[k]);
      out[base + k] = run;
    } else {
      out[base + k] = run;
      run = ann_op<T, MAX>(run, v[k]);
      if (base + k + 1 == n) out[n] = run;
    }
  }
}

// bmax[b] = max(end[64 b .. 64 b + 63]): one wave per 64-feature block
__global__ __launch_bounds__(ANN_BLOCK) void k_ann_blockmax(const int64_t* __restrict__ end, uint64_t n, int64_t* __restrict__ bmax) {
  const uint64_t i = (uint64_t)blockIdx.x * ANN_BLOCK + threadIdx.x;
  long long v = i < n ? (long long)end[i] : (long long)INT64_MIN;
  for (int d = 32; d; d >>= 1) {
    const long long o = __shfl_down(v, d, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0 && i < n) bmax[i >> 6] = (int64_t)v;
}

// first i in [0, n) with a[i] >= key (STRICT: a[i] > key), n when there is none; a is non-decreasing
template <bool STRICT>
__device__ inline uint64_t ann_first(const int64_t* __restrict__ a, uint64_t n, int64_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    const int64_t x = a[mid];
    if (STRICT ? x > key : x >= key) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the walk both passes share: f(i) for every feature i overlapping [s, e), ascending (= file order); returns the steps taken
template <class F>
__device__ inline uint32_t ann_walk(const AnnDev& A, int64_t s, int64_t e, F f) {
  const uint64_t hi = ann_first<false>(A.start, A.n, e);
  uint64_t i = ann_first<true>(A.rmax, A.n, s);
  uint32_t steps = 0;
  while (i < hi) {
    ++steps;
    if ((i & 63) == 0 && A.bmax[i >> 6] <= s) { i += 64; continue; }
    if (A.end[i] > s) f(i);
    ++i;
  }
  return steps;
}

__global__ __launch_bounds__(ANN_BLOCK) void k_ann_count(AnnDev A, const int64_t* __restrict__ qs, const int64_t* __restrict__ qe, uint64_t nq,
                                                          uint64_t* __restrict__ bytes, unsigned long long* __restrict__ totals /* [2] */) {
  __shared__ unsigned long long lds[ANN_BLOCK / 64];
  const uint64_t q = (uint64_t)blockIdx.x * ANN_BLOCK + threadIdx.x;
  unsigned long long cnt = 0, steps = 0;
  if (q < nq) {
    uint64_t b = 0;
    steps = ann_walk(A, qs[q], qe[q], [&](uint64_t i) { ++cnt; b += A.loff[i + 1] - A.loff[i]; });
    bytes[q] = cnt ? b + (cnt - 1) : 2;  // labels + commas, or NA
  }
  // overlaps and walk steps of the batch: summed per workgroup, one atomic each (totals, not places)
  unsigned long long ex, tc, ts;
  (void)ann_block_scan<unsigned long long, false>(cnt, lds, 0ull, &ex, &tc);
  (void)ann_block_scan<unsigned long long, false>(steps, lds, 0ull, &ex, &ts);
  if (threadIdx.x == 0) {
    if (tc) atomicAdd(&totals[0], tc);
    if (ts) atomicAdd(&totals[1], ts);
  }
}

__global__ __launch_bounds__(ANN_BLOCK) void k_ann_fill(AnnDev A, const int64_t* __restrict__ qs, const int64_t* __restrict__ qe, uint64_t nq,
                                                         const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const uint64_t q = (uint64_t)blockIdx.x * ANN_BLOCK + threadIdx.x;
  if (q >= nq) return;
  uint8_t* w = out + off[q];
  uint64_t cnt = 0;  // overlaps so far: a label may be empty, so what has been written says nothing about them
  ann_walk(A, qs[q], qe[q], [&](uint64_t i) {
    if (cnt++) *w++ = ',';
    const uint64_t a = A.loff[i], b = A.loff[i + 1];
    for (uint64_t k = a; k < b; ++k) *w++ = A.blob[k];
  });
  if (!cnt) { w[0] = 'N'; w[1] = 'A'; }
}

template <class T, bool MAX>
void ann_scan(hipStream_t st, const T* in, uint64_t n, T ident, T* partial, T* out) {
  const uint64_t nb = hawk_ann_scan_blocks(n);
  hipLaunchKernelGGL((k_ann_scan1<T, MAX>), dim3((unsigned)nb), dim3(ANN_BLOCK), 0, st, in, n, ident, partial);
  hipLaunchKernelGGL((k_ann_scan2<T, MAX>), dim3(1), dim3(ANN_BLOCK), 0, st, partial, nb, ident);
  hipLaunchKernelGGL((k_ann_scan3<T, MAX>), dim3((unsigned)nb), dim3(ANN_BLOCK), 0, st, in, n, ident, (const T*)partial, out);
}

}  // namespace

uint64_t hawk_ann_scan_blocks(uint64_t n) { return (n + (uint64_t)ANN_BLOCK * ANN_IPT - 1) / ((uint64_t)ANN_BLOCK * ANN_IPT); }

void hawk_launch_ann_index(hipStream_t st, const int64_t* end, uint64_t n, int64_t* partial, int64_t* rmax, int64_t* bmax) {
  if (!n) return;
  ann_scan<int64_t, true>(st, end, n, INT64_MIN, partial, rmax);
  hipLaunchKernelGGL(k_ann_blockmax, dim3((unsigned)((n + ANN_BLOCK - 1) / ANN_BLOCK)), dim3(ANN_BLOCK), 0, st, end, n, bmax);
}

void hawk_launch_ann_count(hipStream_t st, const AnnDev& A, const int64_t* qs, const int64_t* qe, uint64_t nq, uint64_t* off,
                           unsigned long long* totals) {
  if (!nq) return;
  hipLaunchKernelGGL(k_ann_count, dim3((unsigned)((nq + ANN_BLOCK - 1) / ANN_BLOCK)), dim3(ANN_BLOCK), 0, st, A, qs, qe, nq, off, totals);
}

void hawk_launch_ann_offsets(hipStream_t st, uint64_t* off, uint64_t nq, uint64_t* partial) {
  if (!nq) return;
  ann_scan<uint64_t, false>(st, off, nq, (uint64_t)0, partial, off);
}

void hawk_launch_ann_fill(hipStream_t st, const AnnDev& A, const int64_t* qs, const int64_t* qe, uint64_t nq, const uint64_t* off, uint8_t* out) {
  if (!nq) return;
  hipLaunchKernelGGL(k_ann_fill, dim3((unsigned)((nq + ANN_BLOCK - 1) / ANN_BLOCK)), dim3(ANN_BLOCK), 0, st, A, qs, qe, nq, off, out);
}
