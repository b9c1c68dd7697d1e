// hawk_ubuild.hip - the whole-region IUPAC rows of an unphased VCF, built on the device from the genotype text (the rules
// themselves: hawk_ubuild.h; the host builder they restate: haplotypes.add_variants_unphased, reference haplotypes.py:370-712).
//
//   k_gt_parse_unphased  k_gt_parse's record walk (gt_parse_record, hawk_gtparse.h: one definition, instantiated per separator)
//                        with the unphased genotype rule: "a/b" into two bytes, everything else through ub_gt_classify.
//   k_ub_count / k_ub_fill  one ascending carried-variant list per SAMPLE: a wave takes 64 neighbouring samples (lane = sample,
//                        so a variant's 64 code pairs are one coalesced 128-byte read), variants are tested 64 at a time against
//                        both codes and the ballots kept; the fill pass turns them into the lists.
//   k_ub_sig             one wave per sample: the 128-bit signature of its merged (position, bits) sites, from the lists alone.
//   k_ub_rows            one thread per 128 positions (four words) of one target row across the five planes: REF's words are
//                        loaded as 16-byte vectors, the list entries inside the stretch are found by a binary search over the
//                        ascending list, ub_apply is applied and the five vectors are written once.  No atomics on the planes,
//                        no second pass over a row; loads and stores are coalesced along the row.
#include "hawk_bits.h"
#include "hawk_gtparse.h"
#include "hawk_ubuild.h"

struct GtClassifyUnphased {
  __device__ uint32_t operator()(const uint8_t* text, uint64_t s, uint64_t hi) const { return ub_gt_classify(text, s, hi); }
};
__global__ __launch_bounds__(256) void k_gt_parse_unphased(const uint8_t* __restrict__ text, const uint64_t* __restrict__ line_off,
                                                           const uint64_t* __restrict__ gt_off, uint32_t n_samples,
                                                           uint8_t* __restrict__ codes, uint8_t* __restrict__ flags) {
  gt_parse_record<(uint8_t)'/'>(text, line_off, gt_off, n_samples, codes, flags, GtClassifyUnphased());
}

// ballots[sample][chunk] = which of variants 64*chunk .. +63 the sample carries; count[sample] (zeroed by the launcher).
#define UB_CPW 4
__global__ __launch_bounds__(256) void k_ub_count(const uint8_t* __restrict__ codes, uint32_t n_samples, const uint32_t* __restrict__ var_line,
                                                  const uint8_t* __restrict__ var_allele, uint32_t n_var, uint32_t n_chunk,
                                                  unsigned long long* __restrict__ ballots, uint32_t* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 64u + lane;
  const uint32_t ch0 = (blockIdx.y * 4u + (threadIdx.x >> 6)) * UB_CPW;
  if (ch0 >= n_chunk) return;  // wave-uniform
  const bool live = s < n_samples;
  const uint16_t* pairs = reinterpret_cast<const uint16_t*>(codes);  // [line][n_samples] code pairs: code0 | code1 << 8
  uint32_t cnt = 0;
  for (uint32_t ch = ch0; ch < ch0 + UB_CPW && ch < n_chunk; ++ch) {
    unsigned long long b = 0;
    const uint32_t j0 = ch * 64u, nj = j0 + 64u <= n_var ? 64u : n_var - j0;
    const uint32_t jl = j0 + (lane < nj ? lane : 0u);
    const uint32_t my_line = var_line[jl], my_allele = var_allele[jl];
    uint16_t c[64];
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) {
      const uint32_t line = (uint32_t)__builtin_amdgcn_readlane((int)my_line, jj);
      c[jj] = (live && (uint32_t)jj < nj) ? pairs[(size_t)line * n_samples + s] : (uint16_t)0;  // a filler only: `carried` needs jj < nj
    }
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) {
      const uint32_t al = (uint32_t)__builtin_amdgcn_readlane((int)my_allele, jj);
      const bool carried = (uint32_t)jj < nj && ub_carried(c[jj] & 0xffu, c[jj] >> 8, al);
      b |= (unsigned long long)carried << jj;
    }
    if (live) ballots[(size_t)s * n_chunk + ch] = b;
    cnt += (uint32_t)__popcll(b);
  }
  if (live && cnt) atomicAdd(&count[s], cnt);
}

__global__ __launch_bounds__(256) void k_ub_fill(uint32_t n_samples, uint32_t n_chunk, const unsigned long long* __restrict__ ballots,
                                                 const uint64_t* __restrict__ off, uint32_t* __restrict__ idx) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= n_samples) return;  // wave-uniform
  uint64_t o = off[s];
  for (uint32_t ch = 0; ch < n_chunk; ++ch) {
    const unsigned long long b = ballots[(size_t)s * n_chunk + ch];
    if (b == 0) continue;  // wave-uniform
    if ((b >> lane) & 1ull) idx[o + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = ch * 64u + lane;
    o += (uint64_t)__popcll(b);
  }
}

// sig[sample][2]: ub_sig_add over the sample's merged sites.  A lane takes the entries that open a site (the entry before it
// lies at another position) and gathers the site's other entries itself: two or three at the most in practice.
__global__ __launch_bounds__(256) void k_ub_sig(uint32_t n_samples, const uint64_t* __restrict__ off, const uint32_t* __restrict__ idx,
                                                const uint32_t* __restrict__ var_off, const uint8_t* __restrict__ var_mask,
                                                const uint8_t* __restrict__ var_ref, unsigned long long* __restrict__ sig,
                                                unsigned long long* __restrict__ decline) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= n_samples) return;  // wave-uniform
  const uint64_t lo = off[s], hi = off[s + 1];
  uint64_t s0 = 0, s1 = 0;
  for (uint64_t e = lo + lane; e < hi; e += 64u) {
    const uint32_t j = idx[e], pos = var_off[j];
    if (e > lo && var_off[idx[e - 1]] == pos) continue;
    const uint32_t refbit = 1u << var_ref[j];
    uint32_t bits = refbit;
    for (uint64_t f = e; f < hi; ++f) {
      const uint32_t k = idx[f];
      if (var_off[k] != pos) break;
      const uint32_t own = 1u << var_ref[k];  // (hawk_host_unphased_rows: the same three lines)
      if (!ub_site_add(own, &bits, var_mask[k])) atomicMin(decline, (unsigned long long)k);
      bits |= (uint32_t)var_mask[k] | own;
    }
    ub_sig_add(pos, bits, &s0, &s1);
  }
  s0 = wave_sum64(s0);
  s1 = wave_sum64(s1);
  if (lane == 0) { sig[2ull * s] = s0; sig[2ull * s + 1] = s1; }
}

// a thread's four words of one plane, as one 16-byte access; the words stay in registers (every index below is a compile-time one)
__device__ __forceinline__ void ub_load4(const uint32_t* p, uint32_t (&w)[4]) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
__device__ __forceinline__ void ub_store4(uint32_t* p, const uint32_t (&w)[4]) { *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]); }

// Target row first_row + r takes REF's words and the sites of sample row_sample[r].  S is a multiple of four words and every plane
// is 16-byte aligned (hawk_hapset_create), so a thread's four words are one vector.  Bits past the row's length are REF's, and
// REF's are zero (k_pack): a target row is as long as REF.
__global__ __launch_bounds__(256) void k_ub_rows(uint32_t* __restrict__ pA, uint32_t* __restrict__ pC, uint32_t* __restrict__ pG,
                                                 uint32_t* __restrict__ pT, uint32_t* __restrict__ pV, uint32_t S, uint32_t ref_row,
                                                 uint32_t first_row, uint64_t n_quads /* n_rows * S / 4 */, const uint32_t* __restrict__ row_sample,
                                                 const uint64_t* __restrict__ off, const uint32_t* __restrict__ idx,
                                                 const uint32_t* __restrict__ var_off, const uint8_t* __restrict__ var_mask,
                                                 const uint8_t* __restrict__ var_ref, unsigned long long* __restrict__ decline) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_quads) return;
  const uint32_t qpr = S / 4u;
  const uint32_t r = (uint32_t)(t / qpr), q = (uint32_t)(t % qpr);
  const size_t src = (size_t)ref_row * S + 4u * q, dst = (size_t)(first_row + r) * S + 4u * q;
  uint32_t ref[UB_PLANES][4], row[UB_PLANES][4];
  ub_load4(pA + src, ref[0]); ub_load4(pC + src, ref[1]); ub_load4(pG + src, ref[2]); ub_load4(pT + src, ref[3]); ub_load4(pV + src, ref[4]);
#pragma unroll
  for (int pl = 0; pl < UB_PLANES; ++pl)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) row[pl][kk] = ref[pl][kk];
  const uint32_t smp = row_sample[r];
  uint64_t lo = off[smp];
  const uint64_t end = off[smp + 1];
  const uint32_t p0 = q * 128u;
  {  // first entry at or behind p0
    uint64_t hi = end;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if (var_off[idx[mid]] < p0) lo = mid + 1; else hi = mid;
    }
  }
  for (; lo < end; ++lo) {
    const uint32_t j = idx[lo], p = var_off[j];
    if (p >= p0 + 128u) break;
    const uint32_t k = (p - p0) >> 5, bit = p & 31u, mask = var_mask[j], refbase = var_ref[j];
    bool ok = true;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // the entry's word, chosen by a compare per word: no register is indexed at run time
      if (k != (uint32_t)kk) continue;
      uint32_t r5[UB_PLANES], w5[UB_PLANES];
#pragma unroll
      for (int pl = 0; pl < UB_PLANES; ++pl) { r5[pl] = ref[pl][kk]; w5[pl] = row[pl][kk]; }
      ok = ub_apply(r5, w5, bit, mask, refbase);
#pragma unroll
      for (int pl = 0; pl < UB_PLANES; ++pl) row[pl][kk] = w5[pl];
    }
    if (!ok) atomicMin(decline, (unsigned long long)j);
  }
  ub_store4(pA + dst, row[0]); ub_store4(pC + dst, row[1]); ub_store4(pG + dst, row[2]); ub_store4(pT + dst, row[3]); ub_store4(pV + dst, row[4]);
}

void hawk_launch_gt_parse_unphased(hipStream_t st, const uint8_t* text, const uint64_t* line_off, const uint64_t* gt_off, uint64_t n_lines,
                                   uint32_t n_samples, uint8_t* codes, uint8_t* flags) {
  if (n_lines) hipLaunchKernelGGL(k_gt_parse_unphased, dim3((unsigned)n_lines), dim3(256), 0, st, text, line_off, gt_off, n_samples, codes, flags);
}
void hawk_launch_ub_count(hipStream_t st, const uint8_t* codes, uint32_t n_samples, const uint32_t* var_line, const uint8_t* var_allele,
                          uint32_t n_var, unsigned long long* ballots, uint32_t* count /* [n_samples] */) {
  const uint32_t n_chunk = (n_var + 63u) / 64u;
  (void)hipMemsetAsync(count, 0, (size_t)n_samples * 4, st);
  hipLaunchKernelGGL(k_ub_count, dim3((n_samples + 63u) / 64u, (n_chunk + 4u * UB_CPW - 1u) / (4u * UB_CPW)), dim3(256), 0, st, codes, n_samples,
                     var_line, var_allele, n_var, n_chunk, ballots, count);
}
void hawk_launch_ub_fill(hipStream_t st, uint32_t n_samples, uint32_t n_var, const unsigned long long* ballots, const uint64_t* off, uint32_t* idx) {
  hipLaunchKernelGGL(k_ub_fill, dim3((n_samples + 3u) / 4u), dim3(256), 0, st, n_samples, (n_var + 63u) / 64u, ballots, off, idx);
}
void hawk_launch_ub_sig(hipStream_t st, const UbLists& l, unsigned long long* sig, unsigned long long* decline) {
  hipLaunchKernelGGL(k_ub_sig, dim3((l.n_samples + 3u) / 4u), dim3(256), 0, st, l.n_samples, l.off, l.idx, l.var_off, l.var_mask, l.var_ref, sig,
                     decline);
}
void hawk_launch_ub_rows(hipStream_t st, uint32_t* const* plane, uint32_t S, uint32_t ref_row, uint32_t first_row, uint32_t n_rows,
                         const uint32_t* row_sample, const UbLists& l, unsigned long long* decline) {
  const uint64_t n_quads = (uint64_t)n_rows * (S / 4u);
  if (!n_quads) return;
  hipLaunchKernelGGL(k_ub_rows, dim3((unsigned)((n_quads + 255u) / 256u)), dim3(256), 0, st, plane[0], plane[1], plane[2], plane[3], plane[4], S,
                     ref_row, first_row, n_quads, row_sample, l.off, l.idx, l.var_off, l.var_mask, l.var_ref, decline);
}
