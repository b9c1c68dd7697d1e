// hawk_otbulge.hip - K7: bulged off-target sites (the -bDNA / -bRNA arguments of the CRISPRitz call) selected where the site is.
//
// k_ot_bulge<B, DNA> works on the site records of a scan whose window is Gs + pamlen bases, Gs = G + B (DNA bulge: the site's
// spacer is B bases longer than the guide) or G - B (RNA bulge).  One launch = one (type, size).  As in k_ot_match a thread owns a
// site and the guides stream through LDS in OT_GCHUNK pieces, every lane reading the same word (broadcast).  Per pair:
//   prune   the B + 1 shift vectors m_k (hawk_otbulge.h) are formed and ANDed: a position set in all of them mismatches under
//           every placement, so more than max_mm such positions reject the pair - exactly, no placement is lost;
//   queue   the lanes whose pair survives append (lane, guide) to the wave's queue in LDS (ballot + mbcnt), and whenever the queue
//           holds 64 entries the wave verifies them one per lane: the placement loop then runs with every lane busy instead of
//           one lane walking it while 63 wait.  What is left at the end of a guide chunk is verified before the chunk is replaced;
//   verify  otb_best: fewest mismatches, ties to the smallest gap tuple, no ambiguous site base bulged out;
//   sink    rows within max_mm go to hits[] behind an atomic counter that keeps counting past `cap` (the caller retries).
// Integer / bitwise throughout, wave64, no MFMA shape.
#include "hawk_bits.h"
#include "hawk_otbulge.h"

#define OT_GCHUNK 1024  // as hawk_offtarget.hip
#define OTB_NW (HAWK_BLOCK / WAVE)

// spread the 32 bits of x to the even bit positions of a 64-bit word
__device__ __forceinline__ uint64_t otb_spread(uint32_t x) {
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

// The shift vectors of one pair.  code / nmsp: the site's spacer (Gs bases from bit 0, nothing above), g: the guide (G bases).
// even = the even bits of the n = min(G, Gs) positions of the shorter sequence.
template <int B, bool DNA>
__device__ __forceinline__ void otb_vectors(uint64_t code, uint32_t nmsp, uint64_t g, uint64_t even, uint64_t (&m)[B + 1]) {
#pragma unroll
  for (int k = 0; k <= B; ++k) {
    const uint64_t x = DNA ? (g ^ (code >> (2 * k))) : (code ^ (g >> (2 * k)));
    m[k] = ((x | (x >> 1)) | otb_spread(DNA ? (nmsp >> k) : nmsp)) & even;
  }
}

template <int B, bool DNA>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_bulge(const OtSite* __restrict__ sites, uint64_t n_sites,
                                                          const uint64_t* __restrict__ guides, uint32_t n_guides, int G, int sp0,
                                                          int max_mm, OtBulgeHit* __restrict__ hits, uint64_t cap,
                                                          unsigned long long* __restrict__ n_hits) {
  __shared__ uint64_t s_g[OT_GCHUNK];
  __shared__ uint64_t s_code[OTB_NW][WAVE];
  __shared__ uint32_t s_nm[OTB_NW][WAVE];
  __shared__ uint32_t s_q[OTB_NW][2 * WAVE];  // (guide index in the chunk) << 6 | lane; never more than 63 + 64 entries
  const uint32_t wv = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const uint64_t i0 = (uint64_t)blockIdx.x * HAWK_BLOCK + wv * WAVE;  // the wave's first site
  const uint64_t i = i0 + lane;
  const int Gs = DNA ? G + B : G - B, n = DNA ? G : Gs, span = n + B;
  const uint64_t even = (n >= 32 ? ~0ull : otb_low(n)) & OTB_EVEN;
  uint64_t code = 0;
  uint32_t nmsp = 0;
  bool live = false;
  if (i < n_sites) {
    const OtSite st = sites[i];
    code = (st.code >> (2 * sp0)) & (Gs >= 32 ? ~0ull : otb_low(Gs));
    nmsp = (st.nmask >> sp0) & (Gs >= 32 ? 0xffffffffu : ((1u << Gs) - 1u));
    live = true;
  }
  s_code[wv][lane] = code;
  s_nm[wv][lane] = nmsp;
  // what the prune needs of the site, per shift: its code moved down (DNA) and its ambiguity bits at the even positions
  uint64_t ck[B + 1], nk[B + 1];
#pragma unroll
  for (int k = 0; k <= B; ++k) {
    ck[k] = DNA ? (code >> (2 * k)) : code;
    nk[k] = otb_spread(DNA ? (nmsp >> k) : nmsp);
  }
  {  // ambiguous bases alone may already be too many for any guide
    uint64_t a = nk[0];
#pragma unroll
    for (int k = 1; k <= B; ++k) a &= nk[k];
    live = live && __popcll(a & even) <= max_mm;
  }
  uint32_t qn = 0;  // entries in the wave's queue (wave-uniform)

  // entry e of the queue, verified by this lane
  auto verify = [&](uint32_t e, uint32_t g0) {
    const uint32_t l = e & (WAVE - 1), t = e >> 6;
    uint64_t m[B + 1];
    const uint32_t nm = s_nm[wv][l];
    otb_vectors<B, DNA>(s_code[wv][l], nm, s_g[t], even, m);
    const OtbBest r = otb_best(m, B, span, DNA ? nm : 0u, max_mm);
    if (r.mm <= max_mm) {
      const unsigned long long o = atomicAdd(n_hits, 1ull);
      if (o < cap) {
        OtBulgeHit hh;
        hh.site = i0 + l; hh.guide = g0 + t; hh.mm = (uint32_t)r.mm; hh.gaps = r.gaps; hh.pad = 0;
        hits[o] = hh;
      }
    }
  };

  for (uint32_t g0 = 0; g0 < n_guides; g0 += OT_GCHUNK) {
    const uint32_t ng = n_guides - g0 < OT_GCHUNK ? n_guides - g0 : OT_GCHUNK;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < ng; t += HAWK_BLOCK) s_g[t] = guides[g0 + t];
    __syncthreads();
    if (i0 >= n_sites) continue;  // wave-uniform: a wave without sites only helps with the loads and the barriers
#pragma unroll 1
    for (uint32_t t = 0; t < ng; ++t) {
      const uint64_t g = s_g[t];
      uint64_t a = even;
#pragma unroll
      for (int k = 0; k <= B; ++k) {
        const uint64_t x = DNA ? (g ^ ck[k]) : (ck[k] ^ (g >> (2 * k)));
        a &= (x | (x >> 1)) | nk[k];
      }
      const bool keep = live && __popcll(a) <= max_mm;
      const unsigned long long bal = __ballot(keep);
      if (bal == 0) continue;  // wave-uniform
      if (keep) s_q[wv][qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = (t << 6) | lane;
      qn += (uint32_t)__popcll(bal);
      if (qn >= WAVE) {
        qn -= WAVE;
        __builtin_amdgcn_wave_barrier();
        verify(s_q[wv][qn + lane], g0);
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (qn) {  // the chunk's guides leave LDS: verify what is queued
      __builtin_amdgcn_wave_barrier();
      if (lane < qn) verify(s_q[wv][lane], g0);
      __builtin_amdgcn_wave_barrier();
      qn = 0;
    }
  }
}

void hawk_launch_ot_bulge(hipStream_t st, const OtSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, int guidelen,
                          int sp0, int max_mm, int dna, int bsize, OtBulgeHit* hits, uint64_t cap, unsigned long long* n_hits) {
  if (!n_sites || !n_guides) return;
  const dim3 grid((uint32_t)((n_sites + HAWK_BLOCK - 1) / HAWK_BLOCK)), block(HAWK_BLOCK);
#define OTB_LAUNCH(B, D) \
  hipLaunchKernelGGL((k_ot_bulge<B, D>), grid, block, 0, st, sites, n_sites, guides, n_guides, guidelen, sp0, max_mm, hits, cap, n_hits)
  if (dna) {
    if (bsize == 1) OTB_LAUNCH(1, true); else OTB_LAUNCH(2, true);
  } else {
    if (bsize == 1) OTB_LAUNCH(1, false); else OTB_LAUNCH(2, false);
  }
#undef OTB_LAUNCH
}

__global__ __launch_bounds__(256) void k_ot_bulge_gather(const OtSite* __restrict__ sites, const OtBulgeHit* __restrict__ hits, uint64_t n_hits,
                                                         OtSite* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_hits) out[i] = sites[hits[i].site];
}
void hawk_launch_ot_bulge_gather(hipStream_t st, const OtSite* sites, const OtBulgeHit* hits, uint64_t n_hits, OtSite* out) {
  if (n_hits) hipLaunchKernelGGL(k_ot_bulge_gather, dim3((uint32_t)((n_hits + 255) / 256)), dim3(256), 0, st, sites, hits, n_hits, out);
}
