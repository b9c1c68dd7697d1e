// hawk_uwin.hip - the indel-window rows of an unphased VCF, built on the device from the genotype codes and the per-sample SNV
// lists hawk_ubuild_lists leaves in HBM (the rules themselves: hawk_uwin.h; the host builder they restate:
// haplotypes.unphased_indel_windows).
//
//   k_uw_count      one wave per indel allele: lanes take 64 samples at a time in the order of their sorted names (the permutation
//                   the host passes), the code pair of (record, sample) goes through ub_carried and the ballots are kept and
//                   counted.  Lane 0 checks the geometry and the bases of an indel somebody carries.
//   k_uw_instances  the same walk over the kept ballots: the carriers become instance records (indel, sample, the [lo, hi) entry
//                   range of the sample's ascending SNV list inside the window - two binary searches) behind the indel's offset, so
//                   instances come out ordered by (indel, name rank) without an atomic or a sort.
//   k_uw_sig        one thread per instance: the signature over its surviving sites and the indel's ref check.
//   k_uw_group      one thread per instance: the FIRST instance of its indel with an equal signature whose surviving sites are
//                   equal one by one (uw_same_row) is its row's head - itself, if there is none.  Equality is an equivalence, so the
//                   heads in instance order are the distinct rows in first-seen order, whatever the signatures are: a collision
//                   costs a comparison, never a merge.
//   k_uw_fill       one thread per 128 positions (four words) of one window row across the five planes: each word is put together
//                   from REF's words shifted by a (before the anchor), the alt's bases (pool) and REF's words shifted by a - grow
//                   (behind the span), then the carrier's surviving sites are OR-ed in at their mapped bit.  The five vectors are
//                   written once, as 16-byte stores; REF's words are read unaligned, word by word (a row is seven words).  The
//                   launcher clears the rows first: what lies past a row's length is zero, as k_pack leaves it.
#include "hawk_bits.h"
#include "hawk_device.h"

__device__ __forceinline__ UwLists uw_lists(const UbLists& l) { return UwLists{l.idx, l.var_off, l.var_mask, l.var_ref}; }
__device__ __forceinline__ int uw_geom_of(const UwDev& d, uint32_t w, UwGeom* g) { return uw_geometry(d.off[w], d.ref_len[w], d.alt_len[w], d.L, g); }
__device__ __forceinline__ void uw_decline(unsigned long long* decline, uint32_t w, int reason) {
  atomicMin(decline, ((unsigned long long)w << 8) | (unsigned long long)reason);
}

__global__ __launch_bounds__(256) void k_uw_count(const uint8_t* __restrict__ codes, UwDev d, unsigned long long* __restrict__ ballots,
                                                  uint32_t* __restrict__ count, unsigned long long* __restrict__ decline) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= d.n_indel) return;  // wave-uniform
  const uint32_t ns = d.n_samples, n_chunk = (ns + 63u) / 64u, al = d.allele[w];
  const uint16_t* pairs = reinterpret_cast<const uint16_t*>(codes) + (size_t)d.line[w] * ns;  // code0 | code1 << 8 per sample
  uint32_t cnt = 0;
  for (uint32_t ch = 0; ch < n_chunk; ++ch) {
    const uint32_t r = ch * 64u + lane;
    bool carried = false;
    if (r < ns) {
      const uint32_t p = pairs[d.rank_sample[r]];
      carried = ub_carried(p & 0xffu, p >> 8, al);
    }
    const unsigned long long b = __ballot(carried);
    if (lane == 0) ballots[(size_t)w * n_chunk + ch] = b;
    cnt += (uint32_t)__popcll(b);
  }
  if (lane != 0) return;
  count[w] = cnt;
  if (!cnt) return;  // an indel nobody carries builds nothing, whatever it looks like
  UwGeom g;
  const int why = uw_geom_of(d, w, &g);
  if (why) uw_decline(decline, w, why);
  else if (!uw_bases_ok(d.pool + d.pool_off[w], d.ref_len[w] + d.alt_len[w])) uw_decline(decline, w, UB_DECL_INDEL_BASE);
}

__global__ __launch_bounds__(256) void k_uw_instances(UwDev d, UbLists ul, const unsigned long long* __restrict__ ballots) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (w >= d.n_indel) return;  // wave-uniform
  const uint32_t n_chunk = (d.n_samples + 63u) / 64u;
  UwGeom g;
  const bool fits = uw_geom_of(d, w, &g) == UB_DECL_NONE;  // (declined by k_uw_count otherwise: the records are never read)
  const UwLists l = uw_lists(ul);
  uint64_t k0 = d.inst_off[w];
  for (uint32_t ch = 0; ch < n_chunk; ++ch) {
    const unsigned long long b = ballots[(size_t)w * n_chunk + ch];
    if (b == 0) continue;  // wave-uniform
    if ((b >> lane) & 1ull) {
      const uint64_t k = k0 + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      const uint32_t s = d.rank_sample[ch * 64u + lane];
      uint64_t lo = 0, hi = 0;
      if (fits) {
        lo = uw_lower_bound(l, ul.off[s], ul.off[s + 1], g.a);
        hi = uw_lower_bound(l, lo, ul.off[s + 1], g.b + 1u);
      }
      d.inst_indel[k] = w; d.inst_sample[k] = s; d.inst_lo[k] = lo; d.inst_hi[k] = hi;
    }
    k0 += (uint64_t)__popcll(b);
  }
}

__global__ __launch_bounds__(256) void k_uw_sig(UwDev d, UbLists ul, unsigned long long* __restrict__ sig, unsigned long long* __restrict__ decline) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= d.n_inst) return;
  const uint32_t w = d.inst_indel[k];
  UwGeom g;
  if (uw_geom_of(d, w, &g)) return;
  const UwLists l = uw_lists(ul);
  uint64_t s0, s1;
  uw_signature(l, g, d.inst_lo[k], d.inst_hi[k], &s0, &s1);
  sig[2 * k] = s0; sig[2 * k + 1] = s1;
  if (uw_check_ref(l, g, d.inst_lo[k], d.inst_hi[k], d.ref, d.pool + d.pool_off[w])) uw_decline(decline, w, UB_DECL_REF);
}

__global__ __launch_bounds__(256) void k_uw_group(UwDev d, UbLists ul, const unsigned long long* __restrict__ sig, uint32_t* __restrict__ head) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k >= d.n_inst) return;
  const uint32_t w = d.inst_indel[k];
  UwGeom g;
  uint64_t h = k;
  if (uw_geom_of(d, w, &g) == UB_DECL_NONE) {
    const UwLists l = uw_lists(ul);
    const unsigned long long s0 = sig[2 * k], s1 = sig[2 * k + 1];
    for (uint64_t c = d.inst_off[w]; c < k; ++c) {
      if (sig[2 * c] != s0 || sig[2 * c + 1] != s1) continue;
      if (uw_same_row(l, g, d.inst_lo[c], d.inst_hi[c], d.inst_lo[k], d.inst_hi[k])) { h = c; break; }
    }
  }
  head[k] = (uint32_t)h;
}

// REF's 32 bits of one plane from region offset s on (s may lie before the row: those bits are masked off by the caller)
__device__ __forceinline__ uint32_t uw_ref_word(const uint32_t* __restrict__ p, uint32_t S, int64_t s) {
  const int64_t wi = s >> 5;
  const uint32_t sh = (uint32_t)(s & 31);
  const uint32_t lo = (wi >= 0 && wi < (int64_t)S) ? p[wi] : 0u, hi = (wi + 1 >= 0 && wi + 1 < (int64_t)S) ? p[wi + 1] : 0u;
  return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
}
// the bits of a word starting at row position P that lie before row position x
__device__ __forceinline__ uint32_t uw_below(uint32_t x, uint32_t P) { return x <= P ? 0u : (x >= P + 32u ? 0xffffffffu : (1u << (x - P)) - 1u); }

__global__ __launch_bounds__(256) void k_uw_fill(uint32_t* __restrict__ pA, uint32_t* __restrict__ pC, uint32_t* __restrict__ pG, uint32_t* __restrict__ pT,
                                                 uint32_t* __restrict__ pV, uint32_t S, uint32_t ref_row, uint32_t first_row, uint32_t qpr,
                                                 uint64_t n_quads /* n_rows * qpr */, const uint32_t* __restrict__ row_inst, UwDev d, UbLists ul) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= n_quads) return;
  const uint32_t r = (uint32_t)(t / qpr), q = (uint32_t)(t % qpr);
  const uint32_t k = row_inst[r], w = d.inst_indel[k];
  UwGeom g;
  if (uw_geom_of(d, w, &g)) return;
  const uint32_t p0 = q * 128u;
  if (p0 >= g.rowlen || 4u * q + 4u > S) return;  // the cleared words stand
  const size_t src = (size_t)ref_row * S;
  const uint32_t* const ref[UB_PLANES] = {pA + src, pC + src, pG + src, pT + src, pV + src};
  const uint8_t* alt = d.pool + d.pool_off[w] + d.ref_len[w];
  const uint32_t e = g.i + g.alt_len;  // the first row position behind the alt
  uint32_t row[UB_PLANES][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const uint32_t P = p0 + 32u * (uint32_t)kk;
    const uint32_t live = uw_below(g.rowlen, P), before = uw_below(g.i, P) & live, behind = ~uw_below(e, P) & live;
#pragma unroll
    for (int pl = 0; pl < UB_PLANES; ++pl) {
      uint32_t v = 0;
      if (before) v |= uw_ref_word(ref[pl], S, (int64_t)g.a + P) & before;
      if (behind) v |= uw_ref_word(ref[pl], S, (int64_t)g.a + P - g.grow) & behind;
      row[pl][kk] = v;
    }
    const uint32_t x0 = g.i > P ? g.i : P, x1 = e < P + 32u ? e : P + 32u;
    for (uint32_t x = x0; x < x1; ++x) {  // the alt's bases inside this word: one bit of one base plane, and the V bit
      const uint32_t base = alt[x - g.i], bit = 1u << (x - P);
      row[0][kk] |= base == 0u ? bit : 0u; row[1][kk] |= base == 1u ? bit : 0u; row[2][kk] |= base == 2u ? bit : 0u; row[3][kk] |= base == 3u ? bit : 0u;
      row[4][kk] |= bit;
    }
  }
  const UwLists l = uw_lists(ul);
  uint64_t en = d.inst_lo[k];
  const uint64_t hi = d.inst_hi[k];
  uint32_t off, bits;
  while (uw_next_surviving(l, g, &en, hi, &off, &bits)) {
    const uint32_t pos = uw_site_pos(g, off);
    if (pos < p0 || pos >= p0 + 128u) continue;
    const uint32_t kw = (pos - p0) >> 5, bit = pos & 31u;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // the site's word, chosen by a compare per word: no register is indexed at run time
      if (kw != (uint32_t)kk) continue;
#pragma unroll
      for (int pl = 0; pl < 4; ++pl) row[pl][kk] |= ((bits >> pl) & 1u) << bit;
      row[4][kk] |= 1u << bit;
    }
  }
  const size_t dst = (size_t)(first_row + r) * S + 4u * q;
  *reinterpret_cast<uint4*>(pA + dst) = make_uint4(row[0][0], row[0][1], row[0][2], row[0][3]);
  *reinterpret_cast<uint4*>(pC + dst) = make_uint4(row[1][0], row[1][1], row[1][2], row[1][3]);
  *reinterpret_cast<uint4*>(pG + dst) = make_uint4(row[2][0], row[2][1], row[2][2], row[2][3]);
  *reinterpret_cast<uint4*>(pT + dst) = make_uint4(row[3][0], row[3][1], row[3][2], row[3][3]);
  *reinterpret_cast<uint4*>(pV + dst) = make_uint4(row[4][0], row[4][1], row[4][2], row[4][3]);
}

void hawk_launch_uw_count(hipStream_t st, const uint8_t* codes, const UwDev& d, unsigned long long* ballots, uint32_t* count, unsigned long long* decline) {
  if (d.n_indel) hipLaunchKernelGGL(k_uw_count, dim3((d.n_indel + 3u) / 4u), dim3(256), 0, st, codes, d, ballots, count, decline);
}
void hawk_launch_uw_instances(hipStream_t st, const UwDev& d, const UbLists& l, const unsigned long long* ballots) {
  if (d.n_indel) hipLaunchKernelGGL(k_uw_instances, dim3((d.n_indel + 3u) / 4u), dim3(256), 0, st, d, l, ballots);
}
void hawk_launch_uw_sig(hipStream_t st, const UwDev& d, const UbLists& l, unsigned long long* sig, unsigned long long* decline) {
  if (d.n_inst) hipLaunchKernelGGL(k_uw_sig, dim3((unsigned)((d.n_inst + 255u) / 256u)), dim3(256), 0, st, d, l, sig, decline);
}
void hawk_launch_uw_group(hipStream_t st, const UwDev& d, const UbLists& l, const unsigned long long* sig, uint32_t* head) {
  if (d.n_inst) hipLaunchKernelGGL(k_uw_group, dim3((unsigned)((d.n_inst + 255u) / 256u)), dim3(256), 0, st, d, l, sig, head);
}
void hawk_launch_uw_fill(hipStream_t st, uint32_t* const* plane, uint32_t S, uint32_t ref_row, uint32_t first_row, uint32_t n_rows, uint32_t qpr,
                         const uint32_t* row_inst, const UwDev& d, const UbLists& l) {
  const uint64_t n_quads = (uint64_t)n_rows * qpr;
  if (!n_quads) return;
  hipLaunchKernelGGL(k_uw_fill, dim3((unsigned)((n_quads + 255u) / 256u)), dim3(256), 0, st, plane[0], plane[1], plane[2], plane[3], plane[4], S, ref_row,
                     first_row, qpr, n_quads, row_inst, d, l);
}
