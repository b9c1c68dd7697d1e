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
//   sink    what becomes of a row within max_mm is the kernel's Sink (a template parameter, as in hawk_offtarget.hip): OtbListSink
//           appends it to hits[] behind an atomic counter that keeps counting past `cap` (the caller retries); OtbSumSink adds it
//           to the per-guide histogram and CFD sum of hawk_offtarget_bulge_summary, which holds nothing sized by the hits.
// Integer / bitwise throughout (the summary's CFD product is fp64), wave64, no MFMA shape.
#include "hawk_bits.h"
#include "hawk_otbulge.h"

#define OT_GCHUNK 1024  // as hawk_offtarget.hip
#define OTB_NW (HAWK_BLOCK / WAVE)

// ---- pair sinks.  pair<B, DNA>(sites, site index, guide index, the guide's code, the site's spacer code / ambiguity bits as the
// wave holds them in LDS, even, G, span, max_mm): verify one queued pair and do with its row what the call is for.
// The list: the row goes to hits[] (hawk_offtarget_bulges).
struct OtbListSink {
  OtBulgeHit* __restrict__ hits;
  uint64_t cap;
  unsigned long long* __restrict__ n_hits;
  template <int B, bool DNA>
  __device__ __forceinline__ void pair(const OtSite* __restrict__, uint64_t site, uint32_t guide, uint64_t g, uint64_t code, uint32_t nm,
                                       uint64_t even, int, int span, int max_mm) const {
    uint64_t m[B + 1];
    otb_vectors<B, DNA>(code, nm, g, even, m);
    const OtbBest r = otb_best(m, B, span, DNA ? nm : 0u, max_mm);
    if (r.mm <= max_mm) {
      const unsigned long long o = atomicAdd(n_hits, 1ull);
      if (o < cap) {
        OtBulgeHit hh;
        hh.site = site; hh.guide = guide; hh.mm = (uint32_t)r.mm; hh.gaps = r.gaps; hh.pad = 0;
        hits[o] = hh;
      }
    }
  }
};

// The summary (hawk_offtarget_bulge_summary): the row is consumed where it is found, as OtSumSink (hawk_offtarget.hip) consumes a
// mismatch-only hit - hist[guide][mm] += 1 and, with tables, cfd_e4[guide] += the row's CFD in units of 1e-4.  The site record is
// read back (it is in L2 from the wave's own first read) and otb_pair (hawk_otbulge.h) states the pair from the record's window:
// the function the host twin runs, the units ot_text_row gives the table's row.  An unscorable row counts in hist and in
// counters[1] and adds nothing.  Integer sums: no order of the atomics, no sharding changes them.  Nothing here is sized by the hits.
// The spacer code, ambiguity bits, `even` and `span` the wave holds are NOT used here (unnamed parameters): otb_pair cuts the spacer
// out of the record's window and forms the vectors itself, so that kernel and host twin run one statement of a pair; the second
// otb_vectors + otb_best per queued pair is the price (10.4 ms against the list's 9.8 ms on the r05 panel).
struct OtbSumSink : OtBulgeSummary {  // hawk_device.h: tab, hist, cfd_e4, counters, stride, pamlen, right
  template <int B, bool DNA>
  __device__ __forceinline__ void pair(const OtSite* __restrict__ sites, uint64_t site, uint32_t guide, uint64_t g, uint64_t, uint32_t,
                                       uint64_t, int G, int, int max_mm) const {
    const OtSite st = sites[site];
    const OtbPair r = otb_pair_t<B, DNA>(st.code, st.nmask, g, G, pamlen, right, max_mm, tab);
    if (r.mm > max_mm) return;
    atomicAdd(counters, 1ull);
    atomicAdd(hist + (size_t)guide * stride + (uint32_t)r.mm, 1u);
    if (r.units == OT_TEXT_UNSCORABLE) atomicAdd(counters + 1, 1ull);
    else if (r.units > 0) atomicAdd(cfd_e4 + guide, (unsigned long long)r.units);
  }
};

template <int B, bool DNA, class Sink>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_bulge(const OtSite* __restrict__ sites, uint64_t n_sites,
                                                          const uint64_t* __restrict__ guides, uint32_t n_guides, int G, int sp0,
                                                          int max_mm, Sink sink) {
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
    sink.template pair<B, DNA>(sites, i0 + l, g0 + t, s_g[t], s_code[wv][l], s_nm[wv][l], even, G, span, max_mm);
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
  const OtbListSink sink{hits, cap, n_hits};
#define OTB_LAUNCH(B, D, S) \
  hipLaunchKernelGGL((k_ot_bulge<B, D, S>), grid, block, 0, st, sites, n_sites, guides, n_guides, guidelen, sp0, max_mm, sink)
  if (dna) {
    if (bsize == 1) OTB_LAUNCH(1, true, OtbListSink); else OTB_LAUNCH(2, true, OtbListSink);
  } else {
    if (bsize == 1) OTB_LAUNCH(1, false, OtbListSink); else OTB_LAUNCH(2, false, OtbListSink);
  }
}

// The same kernel with the summary's sink (hawk_offtarget_bulge_summary).
void hawk_launch_ot_bulge_sum(hipStream_t st, const OtSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, int guidelen,
                              int sp0, int max_mm, int dna, int bsize, const OtBulgeSummary& sm) {
  if (!n_sites || !n_guides) return;
  const dim3 grid((uint32_t)((n_sites + HAWK_BLOCK - 1) / HAWK_BLOCK)), block(HAWK_BLOCK);
  const OtbSumSink sink{sm};
  if (dna) {
    if (bsize == 1) OTB_LAUNCH(1, true, OtbSumSink); else OTB_LAUNCH(2, true, OtbSumSink);
  } else {
    if (bsize == 1) OTB_LAUNCH(1, false, OtbSumSink); else OTB_LAUNCH(2, false, OtbSumSink);
  }
#undef OTB_LAUNCH
}
