// hawk_otvar.hip - the off-target scan over a variant-enriched genome: the sites only an ALT allele makes.
//
// Beside its one-hot REF planes an index holds four ALLELE planes (hawk_genome_variants): bit q of plane b = base b is in the
// allele set of position q, i.e. REF's one-hot planes with the ALT bases of the added SNVs OR-ed in (ALT alone = allele & ~REF).
// The plain scan (hawk_offtarget.hip) never reads them.  The rule that resolves a window against a guide is hawk_otvar.h's.
//   k_ov_fill     one variant entry per lane: compared against the one-hot REF planes, its ALT bit set by a vector atomicOr
//   k_scan_raw    (hawk_kernels.hip, unchanged) over the allele planes: pam_match intersects a PAM nibble with whatever bits a
//                 position holds, so on multi-bit planes its hit bitmap IS "every PAM position's allele set meets the PAM's set"
//   k_ov_filter   keeps the window starts whose [q, q + L) holds an ALT bit; recounts them per workgroup for the offset scan
//   k_ov_sites    hit bits -> 40-byte site records: REF's code and ambiguity mask, the four allele masks, in guide orientation
//   k_ov_match    all pairs, one site per lane, guides through LDS as their four one-hot planes; a pair within max_mm
//                 mismatches is resolved (ov_resolve) and appended when an ALT base is part of it
#include "hawk_bits.h"
#include "hawk_otvar.h"

__device__ __forceinline__ uint32_t ov_rev32(uint32_t v, int L) { return __brev(v) >> (32 - L); }
__device__ __forceinline__ uint64_t ov_spread(uint32_t x) {  // the 32 bits of x at the even positions of a 64-bit word
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}
__device__ __forceinline__ uint32_t ov_gather_even(uint64_t v) {  // the even bits of v as a 32-bit word
  v &= 0x5555555555555555ull;
  v = (v | (v >> 1)) & 0x3333333333333333ull;
  v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
  v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
  v = (v | (v >> 16)) & 0x00000000ffffffffull;
  return (uint32_t)v;
}

// The caller has checked every entry: row < n_hap, q < hap_len[row], ref and alt in 0..3.
__global__ __launch_bounds__(HAWK_BLOCK) void k_ov_fill(HapSetDev hs, OvPlanes al, const uint32_t* __restrict__ row,
                                                         const uint32_t* __restrict__ q, const uint8_t* __restrict__ ref,
                                                         const uint8_t* __restrict__ alt, uint64_t n, uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * HAWK_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t w = (size_t)row[i] * hs.S + (q[i] >> 5);
  const uint32_t bit = 1u << (q[i] & 31u);
  const uint32_t r = ref[i], a = alt[i];
  uint8_t st = HAWK_OV_APPLIED;
  if (hs.plane[4][w] & bit) st = HAWK_OV_REF_N;
  else if (!(hs.plane[r][w] & bit)) st = HAWK_OV_REF_MISMATCH;
  else if (a == r) st = HAWK_OV_ALT_IS_REF;
  else atomicOr(al.p[a] + w, bit);
  status[i] = st;
}
void hawk_launch_ov_fill(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const uint32_t* row, const uint32_t* q, const uint8_t* ref,
                         const uint8_t* alt, uint64_t n, uint8_t* status) {
  if (n) hipLaunchKernelGGL(k_ov_fill, dim3((uint32_t)((n + HAWK_BLOCK - 1) / HAWK_BLOCK)), dim3(HAWK_BLOCK), 0, st, hs, al, row, q, ref, alt, n, status);
}

// One workgroup per 1024-word tile of a row, as k_scan_raw: bit q of keepF / keepR survives iff an ALT bit lies in [q, q + L).
// counts: [strand][row][workgroup] survivors, the layout k_scan_raw wrote.
__global__ __launch_bounds__(HAWK_BLOCK) void k_ov_filter(HapSetDev hs, OvPlanes al, int L, uint32_t bph, uint32_t* __restrict__ keepF,
                                                           uint32_t* __restrict__ keepR, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_acc[2];
  const uint32_t h = blockIdx.x / bph, blk = blockIdx.x % bph;
  const uint32_t u = blk * HAWK_BLOCK + threadIdx.x;
  const bool active = u < hs.S / 4;
  const size_t rowbase = (size_t)h * hs.S;
  if (threadIdx.x < 2) s_acc[threadIdx.x] = 0;
  uint32_t any[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    uint32_t R[6], A[6];
    load6(hs.plane[b] + rowbase, u, hs.S, active, R);
    load6(al.p[b] + rowbase, u, hs.S, active, A);
#pragma unroll
    for (int k = 0; k < 6; ++k) any[k] |= A[k] & ~R[k];
  }
  window_or(any, L);
  uint32_t cF = 0, cR = 0;
  if (active) {
    uint4 kf = *reinterpret_cast<const uint4*>(keepF + rowbase + 4 * (size_t)u);
    uint4 kr = *reinterpret_cast<const uint4*>(keepR + rowbase + 4 * (size_t)u);
    kf.x &= any[0]; kf.y &= any[1]; kf.z &= any[2]; kf.w &= any[3];
    kr.x &= any[0]; kr.y &= any[1]; kr.z &= any[2]; kr.w &= any[3];
    *reinterpret_cast<uint4*>(keepF + rowbase + 4 * (size_t)u) = kf;
    *reinterpret_cast<uint4*>(keepR + rowbase + 4 * (size_t)u) = kr;
    cF = __popc(kf.x) + __popc(kf.y) + __popc(kf.z) + __popc(kf.w);
    cR = __popc(kr.x) + __popc(kr.y) + __popc(kr.z) + __popc(kr.w);
  }
  const uint32_t w0 = wave_sum(cF | (cR << 16));  // per-wave sums <= 8192 each
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) { atomicAdd(&s_acc[0], w0 & 0xffffu); atomicAdd(&s_acc[1], w0 >> 16); }
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[(size_t)h * bph + blk] = s_acc[0];
    counts[((size_t)hs.n_hap + h) * bph + blk] = s_acc[1];
  }
}
void hawk_launch_ov_filter(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const ScanParams& p, uint32_t* keepF, uint32_t* keepR,
                           uint32_t* counts) {
  hipLaunchKernelGGL(k_ov_filter, dim3(hs.n_hap * p.bph), dim3(HAWK_BLOCK), 0, st, hs, al, (int)p.L, p.bph, keepF, keepR, counts);
}

// As k_ot_sites, with the allele masks beside REF's window.
__global__ __launch_bounds__(HAWK_BLOCK) void k_ov_sites(HapSetDev hs, OvPlanes al, ScanParams p, const uint32_t* __restrict__ keepF,
                                                          const uint32_t* __restrict__ keepR, const uint64_t* __restrict__ offsets,
                                                          OvSite* __restrict__ sites) {
  __shared__ uint32_t s_w[HAWK_BLOCK / WAVE];
  const uint32_t h = blockIdx.x / p.bph, blk = blockIdx.x % p.bph;
  const uint32_t u = blk * HAWK_BLOCK + threadIdx.x;
  const bool active = u < hs.S / 4;
  const size_t rowbase = (size_t)h * hs.S;
  const int L = p.L;
  const uint32_t lmask = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const uint32_t* keep = s ? keepR : keepF;
    uint4 kw = make_uint4(0, 0, 0, 0);
    if (active) kw = *reinterpret_cast<const uint4*>(keep + rowbase + 4 * (size_t)u);
    const uint32_t c = __popc(kw.x) + __popc(kw.y) + __popc(kw.z) + __popc(kw.w);
    uint32_t tot;
    const uint32_t ex = block_excl_scan<HAWK_BLOCK / WAVE>(c, s_w, &tot);
    if (tot == 0) continue;  // workgroup-uniform
    uint64_t o = offsets[((size_t)s * hs.n_hap + h) * p.bph + blk] + ex;
    const uint32_t w[4] = {kw.x, kw.y, kw.z, kw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t x = w[k];
      while (x) {
        const uint32_t j = (uint32_t)__builtin_ctz(x);
        x &= x - 1;
        const uint32_t q = (4 * u + k) * 32 + j;
        uint32_t r[4], m[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          r[b] = ext_glb(hs.plane[b] + rowbase, q).lo & lmask;
          m[b] = ext_glb(al.p[b] + rowbase, q).lo & lmask;
        }
        uint32_t nm = ext_glb(hs.plane[4] + rowbase, q).lo & lmask;
        if (s) {  // guide orientation = reverse complement of the + strand window
          const uint32_t r0 = ov_rev32(r[3], L), r1 = ov_rev32(r[2], L), r2 = ov_rev32(r[1], L), r3 = ov_rev32(r[0], L);
          const uint32_t m0 = ov_rev32(m[3], L), m1 = ov_rev32(m[2], L), m2 = ov_rev32(m[1], L), m3 = ov_rev32(m[0], L);
          r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3;
          m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3;
          nm = ov_rev32(nm, L);
        }
        OvSite st;
        st.code = ov_spread(r[1] | r[3]) | (ov_spread(r[2] | r[3]) << 1);  // base i at bits 2i,2i+1: A0 C1 G2 T3
        st.nmask = nm;
        st.am[0] = m[0]; st.am[1] = m[1]; st.am[2] = m[2]; st.am[3] = m[3];
        st.q = q | ((uint32_t)s << 31);
        st.row = h;
        st.pad = 0;
        sites[o++] = st;
      }
    }
  }
}
void hawk_launch_ov_sites(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const ScanParams& p, const uint32_t* keepF,
                          const uint32_t* keepR, const uint64_t* offsets, OvSite* sites) {
  hipLaunchKernelGGL(k_ov_sites, dim3(hs.n_hap * p.bph), dim3(HAWK_BLOCK), 0, st, hs, al, p, keepF, keepR, offsets, sites);
}

// ---- hit sinks: operator()(the site's ambiguity mask, q | strand << 31 and row, guide index, the resolved pair)
struct OvListSink {
  OvHit* __restrict__ hits;
  uint64_t cap;
  unsigned long long* __restrict__ n_hits;
  __device__ __forceinline__ void operator()(uint32_t nmask, uint32_t q, uint32_t row, uint32_t guide, const OvResolved& r) const {
    const unsigned long long o = atomicAdd(n_hits, 1ull);  // the compiler aggregates this per wave; it keeps counting past cap
    if (o < cap) {  // the record as two 16-byte stores (hits: 32-byte records in a pool block), not a struct built in scratch
      uint4* dst = reinterpret_cast<uint4*>(hits + o);
      dst[0] = make_uint4((uint32_t)r.code, (uint32_t)(r.code >> 32), nmask, r.alt);
      dst[1] = make_uint4(q, row, guide, (uint32_t)r.mm);
    }
  }
};

// All pairs.  Each thread owns one site; the guides stream through LDS in chunks of OV_GCHUNK, each widened ONCE - when it is
// stored - to its four one-hot planes at the window's spacer positions (16 bytes, read by every lane at the same address: an LDS
// broadcast).  Per pair: the positions where the guide's base is in the site's allele set, popcount of the rest.
#define OV_GCHUNK 1024
template <class Sink>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ov_match(const OvSite* __restrict__ sites, uint64_t n_sites,
                                                          const uint64_t* __restrict__ guides, uint32_t n_guides, OvGeom g, int max_mm,
                                                          Sink sink) {
  __shared__ uint4 s_g[OV_GCHUNK];
  const uint64_t i = (uint64_t)blockIdx.x * HAWK_BLOCK + threadIdx.x;
  const int sp0 = g.right ? g.P : 0;
  const uint32_t gmask = g.G >= 32 ? 0xffffffffu : ((1u << g.G) - 1u);
  const uint32_t spmask = gmask << sp0;
  uint64_t code = 0;
  uint32_t nmask = 0, q = 0, row = 0, am[4] = {0, 0, 0, 0};
  bool live = false;
  if (i < n_sites) {
    const OvSite st = sites[i];
    code = st.code; nmask = st.nmask; q = st.q; row = st.row;
    am[0] = st.am[0]; am[1] = st.am[1]; am[2] = st.am[2]; am[3] = st.am[3];
    live = __popc(nmask & spmask) <= max_mm;  // more ambiguous bases than allowed mismatches: no guide can match
  }
  for (uint32_t g0 = 0; g0 < n_guides; g0 += OV_GCHUNK) {
    const uint32_t ng = n_guides - g0 < OV_GCHUNK ? n_guides - g0 : OV_GCHUNK;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < ng; t += HAWK_BLOCK) {
      const uint64_t c = guides[g0 + t];
      const uint32_t b0 = ov_gather_even(c), b1 = ov_gather_even(c >> 1);
      s_g[t] = make_uint4((~b1 & ~b0 & gmask) << sp0, (~b1 & b0 & gmask) << sp0, (b1 & ~b0 & gmask) << sp0, (b1 & b0 & gmask) << sp0);
    }
    __syncthreads();
    if (!live) continue;
    for (uint32_t t = 0; t < ng; ++t) {
      const uint4 gp = s_g[t];
      const uint32_t hit = (am[0] & gp.x) | (am[1] & gp.y) | (am[2] & gp.z) | (am[3] & gp.w);
      if (__popc(~hit & spmask) > max_mm) continue;
      const OvResolved r = ov_resolve(code, nmask, am, guides[g0 + t], g);
      if (r.ok && r.mm <= max_mm && r.alt) sink(nmask, q, row, g0 + t, r);
    }
  }
}
void hawk_launch_ov_match(hipStream_t st, const OvSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, const OvGeom& g,
                          int max_mm, OvHit* hits, uint64_t cap, unsigned long long* n_hits) {
  if (!n_sites || !n_guides) return;
  hipLaunchKernelGGL(k_ov_match<OvListSink>, dim3((uint32_t)((n_sites + HAWK_BLOCK - 1) / HAWK_BLOCK)), dim3(HAWK_BLOCK), 0, st, sites, n_sites,
                     guides, n_guides, g, max_mm, OvListSink{hits, cap, n_hits});
}
