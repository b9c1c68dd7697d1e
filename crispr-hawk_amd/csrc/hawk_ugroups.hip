// hawk_ugroups.hip - the kept guides of an unphased resolution (hawk_resolve.hip's fill pass, in HBM) grouped as the guide report
// merges them (reports.report_from_guides): k_ug_keys builds every guide's key words, finds its REF partner in the handle's
// (start, strand)-sorted REF list and writes CFDon and the G/C counts; an LSD sequence of radix sorts over (key word, index) -
// (hap << 32 | pos) first, so that every group is left in emission order - orders the guides by their full keys, exactly;
// k_ug_heads flags where the key changes and where, inside a group, the haplotype changes; two exclusive scans number the groups
// and the members; k_ug_emit writes the group columns from each head and the CSR member list.  Every rule is a function of
// hawk_ugroups.h, which hawk_host_unphased_groups applies on the host.  One thread per guide throughout; a wave's loads and
// stores are 64 consecutive words of each array except where they follow the sorted order (the gathers of the sort passes, the
// neighbour compare of the heads, the representative's columns).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <utility>

#include "hawk_device.h"

__global__ __launch_bounds__(256) void k_ug_keys(UgDev u, UgWork w, uint32_t* __restrict__ idx, int* __restrict__ status) {
  __shared__ double s_cfd[UG_CFD_MM + UG_CFD_PAM];
  if (u.cfd) {
    for (int t = threadIdx.x; t < UG_CFD_MM + UG_CFD_PAM; t += 256) s_cfd[t] = u.cfd[t];
    __syncthreads();
  }
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= u.n) return;
  const uint64_t i = u.src_row[k];
  const int64_t start = gc_start(u.c, i), stop = gc_stop(u.c, i);
  const uint32_t strand = gc_strand(u.c, i), hap = gc_hap(u.c, i), pos = gc_pos(u.c, i);
  const bool origin = hap < u.n_hap && u.is_ref[hap];
  uint64_t win[UG_PLANES], key[UG_KEY_WORDS];
#pragma unroll
  for (int pl = 0; pl < UG_PLANES; ++pl) win[pl] = u.win[(uint64_t)pl * u.n + k];
  ug_key(u.g, start, stop, strand, origin, win, key);
#pragma unroll
  for (int q = 0; q < UG_KEY_WORDS; ++q) w.keyw[(uint64_t)q * u.n + k] = key[q];
  w.hp[k] = ((uint64_t)hap << 32) | pos;
  idx[k] = (uint32_t)k;
  w.gc[k] = (uint16_t)ug_gc(win, strand, u.g);
  double score = __longlong_as_double(0x7ff8000000000000ll);
  if (u.cfd) {  // the REF partner: the one kept guide of REF's row at the same (start, strand)
    const uint64_t want = (uint64_t)start * 2u + strand;
    uint64_t lo = 0, hi = u.n_rows;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (u.ref_key[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo < u.n_rows && u.ref_key[lo] == want) {
      const uint64_t rr = u.ref_row[lo];
      const uint64_t ko = u.row_off[rr];
      if (u.row_kept[rr] && ko < u.n) {
        uint64_t core[4], rcore[4];
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) { core[pl] = ug_core(win[pl], u.g); rcore[pl] = ug_core(u.win[(uint64_t)pl * u.n + ko], u.g); }
        bool err;
        score = ug_cfdon(core, rcore, strand, u.g, s_cfd, s_cfd + UG_CFD_MM, &err);
        if (err) { score = __longlong_as_double(0x7ff8000000000000ll); atomicExch(status, -5 /* HAWK_E_CFD */); }
      }
    }
  }
  w.cfdon[k] = score;
}

__global__ __launch_bounds__(256) void k_ug_gather(const uint64_t* __restrict__ word, const uint32_t* __restrict__ order, uint64_t n,
                                                   uint64_t* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = word[order[j]];
}

// gflag[j]: sorted guide j opens a group (its key differs from its predecessor's); mflag[j]: it opens a member (a group, or a new
// haplotype inside one - the guides of a group lie sorted by haplotype)
__global__ __launch_bounds__(256) void k_ug_heads(UgWork w, uint64_t n, const uint32_t* __restrict__ order, uint32_t* __restrict__ gflag,
                                                  uint32_t* __restrict__ mflag) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  uint32_t hg = 1, hm = 1;
  if (j) {
    const uint64_t a = order[j], b = order[j - 1];
    bool same = true;
#pragma unroll
    for (int q = 0; q < UG_KEY_WORDS; ++q) same = same && w.keyw[(uint64_t)q * n + a] == w.keyw[(uint64_t)q * n + b];
    hg = same ? 0u : 1u;
    hm = (hg || (w.hp[a] >> 32) != (w.hp[b] >> 32)) ? 1u : 0u;
  }
  gflag[j] = hg;
  mflag[j] = hm;
}

__global__ __launch_bounds__(256) void k_ug_emit(UgDev u, UgWork w, const uint32_t* __restrict__ order, const uint32_t* __restrict__ gflag,
                                                 const uint32_t* __restrict__ mflag, const uint64_t* __restrict__ gidx,
                                                 const uint64_t* __restrict__ midx, UgOut o) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= u.n) return;
  if (j == u.n - 1) o.member_off[o.n_groups] = o.n_members;
  if (!mflag[j]) return;
  const uint64_t k = order[j], m = midx[j];
  const uint64_t hp = w.hp[k];
  if (m < o.n_members) o.member_hap[m] = (uint32_t)(hp >> 32);
  if (!gflag[j]) return;
  const uint64_t g = gidx[j];
  if (g >= o.n_groups) return;
  const uint64_t i = u.src_row[k];
  o.member_off[g] = m;
  o.rep_src_row[g] = (uint32_t)i;
  o.hap[g] = (uint32_t)(hp >> 32);
  o.pos[g] = (uint32_t)hp;
  o.strand[g] = (uint8_t)(w.keyw[(uint64_t)1 * u.n + k] >> 1);
  o.is_ref[g] = (uint8_t)(w.keyw[(uint64_t)1 * u.n + k] & 1u);
  o.start[g] = ug_unbias(w.keyw[k]);
  o.stop[g] = ug_unbias(w.keyw[(uint64_t)2 * u.n + k]);
  o.cfdon[g] = w.cfdon[k];
#pragma unroll
  for (int pl = 0; pl < UG_PLANES; ++pl) o.win[(uint64_t)pl * o.n_groups + g] = u.win[(uint64_t)pl * u.n + k];
  const uint32_t gc = w.gc[k];
  o.gc_num[g] = (uint8_t)(gc & 0xffu);
  o.gc_den[g] = (uint8_t)(gc >> 8);
}

static inline dim3 ug_grid(uint64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// room for the sort passes and for the two scans (hawk_launch_ur_offsets over n + 1 flags)
size_t hawk_ug_temp_bytes(uint64_t n) {
  size_t need = hawk_ur_temp_bytes(n);
  for (unsigned end_bit : {2u, 64u}) {
    size_t a = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0,
                                    end_bit, (hipStream_t)0);
    need = std::max(need, a);
  }
  return need;
}

void hawk_launch_ug_keys(hipStream_t st, const UgDev& u, const UgWork& w, uint32_t* idx, int* status) {
  if (!u.n) return;
  hipLaunchKernelGGL(k_ug_keys, ug_grid(u.n), dim3(256), 0, st, u, w, idx, status);
}

const uint32_t* hawk_launch_ug_sort(hipStream_t st, const UgDev& u, const UgWork& w, void* temp, size_t temp_bytes, uint64_t* keys_a, uint64_t* keys_b,
                                    uint32_t* vals_a, uint32_t* vals_b) {
  const uint64_t n = u.n;
  if (!n) return vals_a;
  uint32_t *cur = vals_a, *other = vals_b;
  size_t tb = temp_bytes;
  // the tie-break first: stable passes above it leave every group ordered by (hap, pos, kept index)
  if (rocprim::radix_sort_pairs(temp, tb, (const uint64_t*)w.hp, keys_b, (const uint32_t*)cur, other, (size_t)n, 0, 64, st) != hipSuccess) return nullptr;
  std::swap(cur, other);
  const unsigned core_bits = (unsigned)ug_key_width(u.g);
  for (int q = UG_KEY_WORDS - 1; q >= 0; --q) {  // least significant word first
    const unsigned end_bit = q >= 3 ? core_bits : (q == 1 ? 2u : 64u);
    hipLaunchKernelGGL(k_ug_gather, ug_grid(n), dim3(256), 0, st, (const uint64_t*)(w.keyw + (uint64_t)q * n), (const uint32_t*)cur, n, keys_a);
    tb = temp_bytes;
    if (rocprim::radix_sort_pairs(temp, tb, (const uint64_t*)keys_a, keys_b, (const uint32_t*)cur, other, (size_t)n, 0, end_bit, st) != hipSuccess) return nullptr;
    std::swap(cur, other);
  }
  return cur;
}

void hawk_launch_ug_heads(hipStream_t st, const UgWork& w, uint64_t n, const uint32_t* order, uint32_t* gflag, uint32_t* mflag) {
  if (!n) return;
  hipLaunchKernelGGL(k_ug_heads, ug_grid(n), dim3(256), 0, st, w, n, order, gflag, mflag);
}

void hawk_launch_ug_emit(hipStream_t st, const UgDev& u, const UgWork& w, const uint32_t* order, const uint32_t* gflag, const uint32_t* mflag,
                         const uint64_t* gidx, const uint64_t* midx, const UgOut& o) {
  if (!u.n) return;
  hipLaunchKernelGGL(k_ug_emit, ug_grid(u.n), dim3(256), 0, st, u, w, order, gflag, mflag, gidx, midx, o);
}
