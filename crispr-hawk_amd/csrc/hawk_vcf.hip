// hawk_vcf.hip — f3: VCF sample columns -> allele codes -> carried-variant lists, on the device.
//
// Reference: VariantRecord.read_vcf_line -> _genotypes_to_samples (variant.py:286-311, 558-619) splits
// every genotype string of every record in Python (2504 samples x 31 k records per Mb), and
// compute_haplotypes_phased (haplotypes.py:132-159) turns the per-variant sample sets into per-sample
// variant lists.  Here the raw text of the records goes to HBM once:
//   k_gt_parse   one workgroup per record: tabs are counted per 16-byte chunk, a workgroup scan gives
//                every chunk the index of its first field, and the thread that owns a field start parses
//                "a|b" (multi-digit alleles, '.' = missing, anything behind ':' ignored) into two bytes
//                codes[record][2*sample + copy]: 0 REF, k = k-th ALT, 255 missing;
//   k_gt_count / k_gt_fill   one wave per chromosome copy (column): variants are tested 64 at a time
//                (codes[line(j)][col] == allele(j)), the ballots kept; the fill pass turns them into the
//                ascending carried-variant list of the column plus, per entry, its offset in the
//                haplotype being built (r0 + running sum of the length changes): exactly the lists
//                hawk_xplan_create_gt expands in place.
#include "hawk_bits.h"
#include "hawk_gtparse.h"

// flags per record, OR-ed over its first n_samples fields (g = a field up to its first ':'):
//   1 = g is not exactly two '|'-separated parts: unphased separator, haploid, three or more parts, empty (what
//       _parse_genotype_phased, variant.py:514-520, refuses before it looks at an allele);
//   2 = field count != n_samples;
//   4 = one of the first two parts of g (split at '|' if g holds one, else at '/') is neither '.' nor all digits; its code
//       stays 255.  "0|1/2" and "|1" are two '|'-parts of which one is no number: 4 alone, as int() fails there in the reference.
// Any field that is not a plain "a|b" goes through gt_classify, which states this rule byte by byte (oracle.vcf_genotype_codes
// is the same statement in Python); returns flags | code0 << 8 | code1 << 16.  Allele numbers clamp at 254.
__device__ __noinline__ uint32_t gt_classify(const uint8_t* __restrict__ text, uint64_t s, uint64_t hi) {
  uint64_t e = s;
  uint32_t nbar = 0, nslash = 0;
  for (; e < hi && text[e] != '\t' && text[e] != ':'; ++e) {
    nbar += text[e] == '|';
    nslash += text[e] == '/';
  }
  const bool has_sep = nbar || nslash;
  const uint8_t sep = nbar ? (uint8_t)'|' : (uint8_t)'/';
  const uint32_t nparts = (nbar ? nbar : nslash) + 1u;
  uint32_t fl = nbar == 1u ? 0u : 1u, v[2] = {255u, 255u};
  uint64_t p = s;
  for (uint32_t c = 0; c < 2u && c < nparts; ++c) {
    uint64_t q = p;
    while (q < e && !(has_sep && text[q] == sep)) ++q;
    if (!(q - p == 1 && text[p] == '.')) {
      bool num = q > p;
      uint32_t x = 0;
      for (uint64_t t = p; t < q; ++t) {
        const uint8_t ch = text[t];
        if (ch < '0' || ch > '9') { num = false; break; }
        x = x * 10u + (ch - '0');
        if (x > 254u) x = 254u;
      }
      if (num) v[c] = x; else fl |= 4u;
    }
    p = q + 1;
  }
  return fl | v[0] << 8 | v[1] << 16;
}

struct GtClassifyPhased {
  __device__ uint32_t operator()(const uint8_t* text, uint64_t s, uint64_t hi) const { return gt_classify(text, s, hi); }
};
// the record walk itself: gt_parse_record (hawk_gtparse.h), shared with k_gt_parse_unphased (hawk_ubuild.hip)
__global__ __launch_bounds__(256) void k_gt_parse(const uint8_t* __restrict__ text, const uint64_t* __restrict__ line_off,
                                                  const uint64_t* __restrict__ gt_off, uint32_t n_samples,
                                                  uint8_t* __restrict__ codes, uint8_t* __restrict__ flags) {
  gt_parse_record<(uint8_t)'|'>(text, line_off, gt_off, n_samples, codes, flags, GtClassifyPhased());
}

// ballots[col][chunk] = which of variants 64*chunk .. +63 the column carries;
// col_count[col], col_count[n_cols + col]: carried variants, carried indels (var_chain != 0) of the column (zeroed by the launcher).
// A wave takes 64 neighbouring columns and GT_CPW chunks of variants: lane = column, so a variant's 64 codes are one coalesced
// 64-byte read and every lane shifts its own ballot word together (the first version gave a wave one column and its lanes 64
// variants - 64 cache lines per load for 64 bytes of use: 0.74 ms on C3 where the matrix is 155 MB).
#define GT_CPW 4
__global__ __launch_bounds__(256) void k_gt_count(const uint8_t* __restrict__ codes, uint32_t n_cols, const uint32_t* __restrict__ var_line,
                                                  const uint8_t* __restrict__ var_allele, const int32_t* __restrict__ var_chain, uint32_t n_var,
                                                  uint32_t n_chunk, unsigned long long* __restrict__ ballots, uint32_t* __restrict__ col_count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t col = blockIdx.x * 64u + lane;
  const uint32_t ch0 = (blockIdx.y * 4u + (threadIdx.x >> 6)) * GT_CPW;
  if (ch0 >= n_chunk) return;  // wave-uniform
  const bool live = col < n_cols;
  uint32_t cnt = 0, cnt_indel = 0;
  for (uint32_t ch = ch0; ch < ch0 + GT_CPW && ch < n_chunk; ++ch) {
    unsigned long long b = 0, bi = 0;
    const uint32_t j0 = ch * 64u, nj = j0 + 64u <= n_var ? 64u : n_var - j0;
    // the chunk's 64 variants: line, allele and chain read once by the lanes, handed round by v_readlane (compile-time lane: the loop
    // is unrolled) - the 64 byte loads of a lane then depend on nothing but each other's issue
    const uint32_t jl = j0 + (lane < nj ? lane : 0u);
    const uint32_t my_line = var_line[jl], my_meta = (uint32_t)var_allele[jl] | (var_chain[jl] != 0 ? 0x100u : 0u);
    uint8_t c[64];
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) {
      const uint32_t line = (uint32_t)__builtin_amdgcn_readlane((int)my_line, jj);
      c[jj] = (live && (uint32_t)jj < nj) ? codes[(size_t)line * n_cols + col] : (uint8_t)254;  // a filler only: no ballot bit comes from it (`carried` needs jj < nj, stores and counts need `live`)
    }
#pragma unroll
    for (int jj = 0; jj < 64; ++jj) {
      const uint32_t meta = (uint32_t)__builtin_amdgcn_readlane((int)my_meta, jj);
      const bool carried = (uint32_t)jj < nj && c[jj] == (uint8_t)(meta & 0xffu);
      b |= (unsigned long long)carried << jj;
      bi |= (unsigned long long)(carried && (meta & 0x100u)) << jj;
    }
    if (live) ballots[(size_t)col * n_chunk + ch] = b;
    cnt += (uint32_t)__popcll(b);
    cnt_indel += (uint32_t)__popcll(bi);
  }
  if (live && cnt) atomicAdd(&col_count[col], cnt);
  if (live && cnt_indel) atomicAdd(&col_count[n_cols + col], cnt_indel);
}

__global__ __launch_bounds__(256) void k_gt_fill(uint32_t n_cols, const int32_t* __restrict__ var_r0, const int32_t* __restrict__ var_chain,
                                                 uint32_t n_var, uint32_t n_chunk, const unsigned long long* __restrict__ ballots,
                                                 const uint64_t* __restrict__ col_off, uint32_t* __restrict__ hv_idx,
                                                 int32_t* __restrict__ hv_o, int64_t* __restrict__ col_delta,
                                                 const uint64_t* __restrict__ indel_off, uint32_t* __restrict__ indel_entry) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t col = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (col >= n_cols) return;
  uint64_t o = col_off[col];
  uint64_t io = indel_off[col];  // where this column's carried indels are listed (by entry index: position-map segments come from them)
  int64_t run = 0;  // sum of the length changes of the variants already placed
  for (uint32_t ch = 0; ch < n_chunk; ++ch) {
    const unsigned long long b = ballots[(size_t)col * n_chunk + ch];
    if (b == 0) continue;  // wave-uniform
    const uint32_t j = ch * 64u + lane;
    const bool carried = (b >> lane) & 1ull;
    const int32_t chn = carried ? var_chain[j] : 0;
    const uint32_t inc = wave_incl_scan((uint32_t)chn);  // two's complement: sums of signed values
    const uint32_t rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (carried) {
      hv_idx[o + rank] = j;
      hv_o[o + rank] = (int32_t)((int64_t)var_r0[j] + run + (int64_t)(int32_t)(inc - (uint32_t)chn));
    }
    const unsigned long long bi = __ballot(chn != 0);
    if (chn != 0) indel_entry[io + (uint32_t)__popcll(bi & ((1ull << lane) - 1ull))] = (uint32_t)(o + rank);
    io += (uint64_t)__popcll(bi);
    run += (int64_t)(int32_t)__builtin_amdgcn_readlane((int)inc, 63);
    o += (uint64_t)__popcll(b);
  }
  if (lane == 0) col_delta[col] = run;
}

void hawk_launch_gt_parse(hipStream_t st, const uint8_t* text, const uint64_t* line_off, const uint64_t* gt_off, uint64_t n_lines,
                          uint32_t n_samples, uint8_t* codes, uint8_t* flags) {
  if (n_lines) hipLaunchKernelGGL(k_gt_parse, dim3((unsigned)n_lines), dim3(256), 0, st, text, line_off, gt_off, n_samples, codes, flags);
}
void hawk_launch_gt_count(hipStream_t st, const uint8_t* codes, uint32_t n_cols, const uint32_t* var_line, const uint8_t* var_allele,
                          const int32_t* var_chain, uint32_t n_var, unsigned long long* ballots, uint32_t* col_count /* [2 * n_cols] */) {
  const uint32_t n_chunk = (n_var + 63u) / 64u;
  (void)hipMemsetAsync(col_count, 0, (size_t)2 * n_cols * 4, st);
  hipLaunchKernelGGL(k_gt_count, dim3((n_cols + 63u) / 64u, (n_chunk + 4u * GT_CPW - 1u) / (4u * GT_CPW)), dim3(256), 0, st, codes, n_cols, var_line,
                     var_allele, var_chain, n_var, n_chunk, ballots, col_count);
}
void hawk_launch_gt_fill(hipStream_t st, uint32_t n_cols, const int32_t* var_r0, const int32_t* var_chain, uint32_t n_var,
                         const unsigned long long* ballots, const uint64_t* col_off, uint32_t* hv_idx, int32_t* hv_o, int64_t* col_delta,
                         const uint64_t* indel_off, uint32_t* indel_entry) {
  const uint32_t n_chunk = (n_var + 63u) / 64u;
  hipLaunchKernelGGL(k_gt_fill, dim3((n_cols + 3u) / 4u), dim3(256), 0, st, n_cols, var_r0, var_chain, n_var, n_chunk, ballots, col_off,
                     hv_idx, hv_o, col_delta, indel_off, indel_entry);
}
