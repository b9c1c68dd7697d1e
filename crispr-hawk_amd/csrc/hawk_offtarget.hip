// hawk_offtarget.hip — K7: mismatch-tolerant off-target enumeration on the GPU.
//
// Replaces the reference's external call `crispritz.py search <index> pam.txt guides.txt -mm M
// -bDNA 0 -bRNA 0` (offtargets.py:222-293; CRISPRitz 2.6.6 is not vendored, so the semantics
// are restated from the call site and from the fields the reference consumes, offtarget.py:
// 77-101): every genome window, both strands, whose PAM positions hold an unambiguous base
// inside the PAM's IUPAC set and whose spacer differs from a guide in at most `max_mm`
// positions (an ambiguous genome base counts as a mismatch).
//
// The genome is a plane set like the haplotypes (contigs cut into equal rows on the host),
// made one-hot: A,C,G,T planes keep only unambiguous bases, plane 4 marks ambiguous ones.
//   k_ot_onehot   planes -> one-hot + ambiguity mask (once per genome)
//   k_scan_raw    (hawk_kernels.hip) PAM hits of both strands as bitmaps, indexed by window start
//   k_ot_sites    hit bits -> site records: the guidelen+pamlen window in guide orientation
//                 (strand 1 reverse-complemented) as a 2-bit code + ambiguity mask
//   k_ot_match    all pairs site x guide: XOR, fold to one bit per base, popcount, <= max_mm
//                 survivors appended through a wave-aggregated atomic (small guide sets)
//   k_ot_match_seeded  pigeonhole filter: with the spacer cut into max_mm + 1 blocks, a pair within max_mm
//                 mismatches agrees exactly in one block; the guides are bucketed per block by the block's
//                 bases (host, counting sort), a site compares only against the buckets its own blocks name:
//                 ~ (max_mm + 1) / 4^blocklen of the all-pairs work (max_mm = 7, where pair seeds do not fit)
//   k_ot_match_pairs   the same with max_mm + 2 blocks and the guides bucketed per PAIR of blocks (max_mm <= 6)
//   k_ot_gather   hit sites -> compact array for one download
// What a match kernel does with a hit is its Sink (a template parameter): OtListSink appends it to hits[] for
// hawk_offtarget_scan; OtSumSink consumes it where it is found - per-guide mismatch histogram and the sum of the sites' CFD in
// units of 1e-4 - for hawk_offtarget_summary, which therefore holds nothing that grows with the number of hits.
#include "hawk_bits.h"

// reverse the low L (<= 32) bits
__device__ __forceinline__ uint32_t rev32(uint32_t v, int L) { return __brev(v) >> (32 - L); }
// spread the 32 bits of x to the even bit positions of a 64-bit word
__device__ __forceinline__ uint64_t spread(uint32_t x) {
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000ffff0000ffffull;
  v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
  v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_onehot(uint32_t* pA, uint32_t* pC, uint32_t* pG, uint32_t* pT, uint32_t* pV,
                                                           uint64_t nwords) {
  const uint64_t i = (uint64_t)blockIdx.x * HAWK_BLOCK + threadIdx.x;
  if (i >= nwords) return;
  const uint32_t a = pA[i], c = pC[i], g = pG[i], t = pT[i];
  const uint32_t multi = (a & c) | ((a | c) & (g | t)) | (g & t);  // two or more planes set: N, R, Y, ...
  pA[i] = a & ~multi; pC[i] = c & ~multi; pG[i] = g & ~multi; pT[i] = t & ~multi;
  pV[i] = multi;
}
void hawk_launch_ot_onehot(hipStream_t st, uint32_t* const* plane, uint64_t nwords) {
  if (!nwords) return;
  hipLaunchKernelGGL(k_ot_onehot, dim3((uint32_t)((nwords + HAWK_BLOCK - 1) / HAWK_BLOCK)), dim3(HAWK_BLOCK), 0, st, plane[0],
                     plane[1], plane[2], plane[3], plane[4], nwords);
}

// one workgroup per 1024-word tile of a genome row, as k_emit_hits: bit q of keepF/keepR = a
// window starting at q has its PAM (strand 0: fwd pattern, strand 1: reverse complement).
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_sites(HapSetDev hs, ScanParams p, const uint32_t* __restrict__ keepF,
                                                          const uint32_t* __restrict__ keepR,
                                                          const uint64_t* __restrict__ offsets, OtSite* __restrict__ sites) {
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
        uint32_t a = ext_glb(hs.plane[0] + rowbase, q).lo & lmask, cc = ext_glb(hs.plane[1] + rowbase, q).lo & lmask;
        uint32_t g = ext_glb(hs.plane[2] + rowbase, q).lo & lmask, t = ext_glb(hs.plane[3] + rowbase, q).lo & lmask;
        uint32_t nm = ext_glb(hs.plane[4] + rowbase, q).lo & lmask;
        if (s) {  // guide orientation = reverse complement of the + strand window
          const uint32_t ra = rev32(t, L), rc = rev32(g, L), rg = rev32(cc, L), rt = rev32(a, L);
          a = ra; cc = rc; g = rg; t = rt; nm = rev32(nm, L);
        }
        (void)a;
        OtSite st;
        st.code = spread(cc | t) | (spread(g | t) << 1);  // base i at bits 2i,2i+1: A0 C1 G2 T3
        st.nmask = nm;
        st.q = q | ((uint32_t)s << 31);
        st.row = h;
        sites[o++] = st;
      }
    }
  }
}
void hawk_launch_ot_sites(hipStream_t st, const HapSetDev& hs, const ScanParams& p, const uint32_t* keepF, const uint32_t* keepR,
                          const uint64_t* offsets, OtSite* sites) {
  hipLaunchKernelGGL(k_ot_sites, dim3(hs.n_hap * p.bph), dim3(HAWK_BLOCK), 0, st, hs, p, keepF, keepR, offsets, sites);
}

// ---- hit sinks.  operator()(site index, guide index, the guide's 2-bit code, mismatches); the guide index is taken by reference
// so that a sink which may drop the hit (OtListSink past cap) does not load it first.
struct OtListSink {
  OtHit* __restrict__ hits;
  uint64_t cap;
  unsigned long long* __restrict__ n_hits;
  __device__ __forceinline__ void operator()(uint64_t site, const uint32_t& guide, uint64_t, int mm) const {
    const unsigned long long o = atomicAdd(n_hits, 1ull);  // the compiler aggregates this per wave
    if (o < cap) { OtHit hh; hh.site = site; hh.guide = guide; hh.mm = (uint32_t)mm; hits[o] = hh; }
  }
};

// ot_round_e4 - round(x, 4) of Python as an integer number of 1e-4 units - is hawk_ottext.h's: the rows of the off-targets table
// round with the same function.

// The summary's sink.  Per hit: hist[guide][mm] += 1 and, with tables, cfd_e4[guide] += round(CFD(guide, site), 4) * 1e4 with the CFD
// formed as compute_cfd forms it (cfdscore.py:53-95; the string form is k_cfd, hawk_kernels.hip): a left-to-right fp64 product
// over the positions i < min(G, 20) where guide and site differ, times the entry of the site's PAM[-2:].  tab = mm[20][4][4]
// ([position][guide base][site base], the r<wt>:d<revcomp(sg)> key already folded into the layout) + pam[16].  A site with an
// ambiguous base under a lookup - among the first min(G, 20) spacer bases, where it always differs from the guide, or in PAM[-2:]
// - is the reference's KeyError: counted in counters[1], still in hist, nothing added to cfd_e4.  Integer sums: the result does
// not depend on the order of the atomics nor on how a genome is sharded.  The site record is read back per hit (hits are rare
// next to candidates; the record is in L2 from the kernel's own first read).
struct OtSumSink : OtSummary {  // hawk_device.h: sites, tab, hist, cfd_e4, counters, stride, sp0, pam2, ncmp
  __device__ __forceinline__ void operator()(uint64_t site, const uint32_t& guide, uint64_t gcode, int mm) const {
    const uint32_t g = guide;
    atomicAdd(counters, 1ull);  // one address: aggregated per wave by the compiler
    atomicAdd(hist + (size_t)g * stride + (uint32_t)mm, 1u);
    if (!tab) return;
    const OtSite st = sites[site];
    if (((st.nmask >> sp0) & ((1u << ncmp) - 1u)) | ((st.nmask >> pam2) & 3u)) { atomicAdd(counters + 1, 1ull); return; }
    const uint64_t sc = st.code >> (2 * sp0);
    const uint64_t x = sc ^ gcode;
    uint64_t d = (x | (x >> 1)) & 0x5555555555555555ull & ((1ull << (2 * ncmp)) - 1ull);
    double s = 1.0;
    while (d) {  // ascending position
      const int b = __builtin_ctzll(d);
      d &= d - 1;
      s *= tab[((b >> 1) * 4 + (int)((gcode >> b) & 3u)) * 4 + (int)((sc >> b) & 3u)];
    }
    const uint32_t pp = (uint32_t)(st.code >> (2 * pam2)) & 15u;
    s *= tab[320 + 4 * (pp & 3u) + (pp >> 2)];
    atomicAdd(cfd_e4 + g, (unsigned long long)ot_round_e4(s));
  }
};

// All pairs.  Each thread owns one site; the guides stream through LDS in chunks and are read
// by every lane at the same address (LDS broadcast, conflict-free).  Per pair: XOR the 2-bit
// codes, fold each base's two bits into one, add the ambiguity bits, popcount.
#define OT_GCHUNK 1024
template <class Sink>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_match(const OtSite* __restrict__ sites, uint64_t n_sites,
                                                          const uint64_t* __restrict__ guides, uint32_t n_guides, int guidelen,
                                                          int sp0, int max_mm, Sink sink) {
  __shared__ uint64_t s_g[OT_GCHUNK];
  const uint64_t i = (uint64_t)blockIdx.x * HAWK_BLOCK + threadIdx.x;
  const bool have = i < n_sites;
  uint64_t code = 0;
  uint32_t nmsp = 0;
  const uint64_t smask = guidelen >= 32 ? ~0ull : ((1ull << (2 * guidelen)) - 1ull);
  bool live = false;
  if (have) {
    const OtSite st = sites[i];
    code = (st.code >> (2 * sp0)) & smask;
    nmsp = (st.nmask >> sp0) & (guidelen >= 32 ? 0xffffffffu : ((1u << guidelen) - 1u));
    live = __popc(nmsp) <= max_mm;  // more ambiguous bases than allowed mismatches: no guide can match
  }
  const uint64_t nm2 = spread(nmsp);  // ambiguity bits at the even positions, like the folded XOR
  for (uint32_t g0 = 0; g0 < n_guides; g0 += OT_GCHUNK) {
    const uint32_t ng = n_guides - g0 < OT_GCHUNK ? n_guides - g0 : OT_GCHUNK;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < ng; t += HAWK_BLOCK) s_g[t] = guides[g0 + t];
    __syncthreads();
    if (!live) continue;
    for (uint32_t t = 0; t < ng; ++t) {
      const uint64_t x = code ^ s_g[t];
      const uint64_t m = ((x | (x >> 1)) & 0x5555555555555555ull) | nm2;
      const int mm = __popcll(m);
      if (mm <= max_mm) sink(i, g0 + t, s_g[t], mm);
    }
  }
}

// Seeded match.  Each thread owns one site and visits, per block, the bucket of guides whose key bases equal the
// site's (a gather from the L2-resident bucketed guide table).  A pair that agrees in the key bases of several
// blocks is met several times; it is reported at the first of them.
template <class Sink>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_match_seeded(const OtSite* __restrict__ sites, uint64_t n_sites, OtSeeds sd,
                                                                 const uint32_t* __restrict__ goff, const uint64_t* __restrict__ gcode,
                                                                 const uint32_t* __restrict__ gid, uint32_t n_guides, int guidelen,
                                                                 int sp0, int max_mm, Sink sink) {
  const uint64_t i = (uint64_t)blockIdx.x * HAWK_BLOCK + threadIdx.x;
  if (i >= n_sites) return;
  const OtSite st = sites[i];
  const uint64_t smask = guidelen >= 32 ? ~0ull : ((1ull << (2 * guidelen)) - 1ull);
  const uint64_t code = (st.code >> (2 * sp0)) & smask;
  const uint32_t nmsp = (st.nmask >> sp0) & (guidelen >= 32 ? 0xffffffffu : ((1u << guidelen) - 1u));
  if (__popc(nmsp) > max_mm) return;  // more ambiguous bases than allowed mismatches: no guide can match
  const uint64_t nm2 = spread(nmsp);
  for (int b = 0; b < sd.nb; ++b) {  // wave-uniform
    const int ks = sd.start[b], kl = sd.klen[b];
    if ((nmsp >> ks) & ((1u << kl) - 1u)) continue;  // an ambiguous base among the key bases: this block cannot agree
    const uint32_t key = (uint32_t)(code >> (2 * ks)) & ((1u << (2 * kl)) - 1u);
    const uint32_t lo = goff[sd.off_base[b] + key], hi = goff[sd.off_base[b] + key + 1];
    const uint64_t* gc = gcode + (size_t)b * n_guides;
    const uint32_t* gi = gid + (size_t)b * n_guides;
    for (uint32_t t = lo; t < hi; ++t) {
      const uint64_t x = code ^ gc[t];
      const uint64_t m = ((x | (x >> 1)) & 0x5555555555555555ull) | nm2;
      const int mm = __popcll(m);
      if (mm > max_mm) continue;
      bool earlier = false;
      for (int j = 0; j < b; ++j) earlier = earlier || (m & sd.pmask2[j]) == 0;
      if (earlier) continue;
      sink(i, gi[t], gc[t], mm);
    }
  }
}

// Pair seeds, candidates dealt evenly.  A wave takes 64 sites.  Per pair of blocks every lane looks its site's bucket up (two
// adjacent offsets); the wave's candidates - the concatenation of the 64 buckets - are then walked 64 at a time, candidate c by lane
// c: a 6-step search over the lanes' exclusive counts (LDS) names the owning site, whose code comes out of LDS, and the guide codes of
// consecutive candidates are consecutive words of the bucketed table.  No lane idles because its own bucket is shorter than a
// neighbour's (the per-lane bucket walks of the single-block seeded kernels ran at a third of their lanes: profiles/r03_c5_pmc.json).
// A pair that agrees in more than two blocks is met in several tables and reported in the first (lowest two agreeing blocks).
template <class Sink>
__global__ __launch_bounds__(HAWK_BLOCK) void k_ot_match_pairs(const OtSite* __restrict__ sites, uint64_t n_sites, OtPairSeeds sd,
                                                                const uint32_t* __restrict__ goff, const uint64_t* __restrict__ gcode,
                                                                const uint32_t* __restrict__ gid, uint32_t n_guides, int guidelen,
                                                                int sp0, int max_mm, Sink sink) {
  __shared__ uint64_t s_code[HAWK_BLOCK / WAVE][WAVE], s_nm2[HAWK_BLOCK / WAVE][WAVE];
  __shared__ uint32_t s_ex[HAWK_BLOCK / WAVE][WAVE + 1], s_lo[HAWK_BLOCK / WAVE][WAVE];
  const uint32_t wv = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const uint64_t i0 = (uint64_t)blockIdx.x * HAWK_BLOCK + wv * WAVE;  // the wave's first site
  if (i0 >= n_sites) return;                                            // wave-uniform; no workgroup barrier below
  const uint64_t i = i0 + lane;
  const uint64_t smask = guidelen >= 32 ? ~0ull : ((1ull << (2 * guidelen)) - 1ull);
  uint64_t code = 0;
  uint32_t nmsp = 0xffffffffu;
  if (i < n_sites) {
    const OtSite st = sites[i];
    code = (st.code >> (2 * sp0)) & smask;
    nmsp = (st.nmask >> sp0) & (guidelen >= 32 ? 0xffffffffu : ((1u << guidelen) - 1u));
  }
  const bool live = i < n_sites && __popc(nmsp) <= max_mm;  // more ambiguous bases than allowed mismatches: no guide can match
  const uint64_t nm2 = spread(nmsp);
  s_code[wv][lane] = code;
  s_nm2[wv][lane] = nm2;
  uint32_t blk_ok = 0;  // bit b: no ambiguous base among block b's key bases
  for (int b = 0; b < sd.nb; ++b) blk_ok |= (((nmsp >> sd.start[b]) & ((1u << sd.klen[b]) - 1u)) == 0 ? 1u : 0u) << b;
  __builtin_amdgcn_wave_barrier();
  // (Tried and dropped, same 5.9 ms at the full C5 size: all 15 tables' look-ups in flight before the first is used - in registers,
  // 73 VGPRs, or staged through LDS, 8.2 ms.  The wave's life is the chain per table - scan, owner search in LDS, guide load - at
  // ~19 candidates per table and wave; profiles/r04_c5_pmc.json.)
#pragma unroll 1
  for (int p = 0; p < sd.n_pairs; ++p) {  // wave-uniform
    {
    const int bi = sd.pi[p], bj = sd.pj[p];
    uint32_t lo = 0, cnt = 0;
    if (live && ((blk_ok >> bi) & 1u) && ((blk_ok >> bj) & 1u)) {
      const uint32_t ki = (uint32_t)(code >> (2 * sd.start[bi])) & ((1u << (2 * sd.klen[bi])) - 1u);
      const uint32_t kj = (uint32_t)(code >> (2 * sd.start[bj])) & ((1u << (2 * sd.klen[bj])) - 1u);
      const uint32_t* o = goff + sd.off_base[p] + (ki | (kj << (2 * sd.klen[bi])));
      lo = o[0];
      cnt = o[1] - lo;
    }
    const uint32_t inc = wave_incl_scan(cnt);
    const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
    if (T != 0) {
    s_ex[wv][lane] = inc - cnt;
    s_lo[wv][lane] = lo;
    __builtin_amdgcn_wave_barrier();
    const uint64_t* __restrict__ gc = gcode + (size_t)p * n_guides;
    const uint32_t* __restrict__ gi = gid + (size_t)p * n_guides;
#pragma unroll 1
    for (uint32_t c0 = 0; c0 < T; c0 += WAVE) {
      const uint32_t c = c0 + lane;
      if (c < T) {
        uint32_t l = 0;
#pragma unroll
        for (uint32_t step = WAVE / 2; step; step >>= 1) l += (s_ex[wv][l + step] <= c) ? step : 0u;  // the last lane whose candidates start at or before c
        const uint32_t t = s_lo[wv][l] + (c - s_ex[wv][l]);
        const uint64_t gct = gc[t];
        const uint64_t x = s_code[wv][l] ^ gct;
        const uint64_t m = ((x | (x >> 1)) & 0x5555555555555555ull) | s_nm2[wv][l];
        const int mm = __popcll(m);
        if (mm <= max_mm) {
          // the blocks that agree, lowest first: this table is the pair's first iff they are (bi, bj)
          int first = -1, second = -1;
          for (int b = 0; b < sd.nb; ++b)
            if ((m & sd.pmask2[b]) == 0) { if (first < 0) first = b; else if (second < 0) second = b; }
          if (first == bi && second == bj) sink(i0 + l, gi[t], gct, mm);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    }
    }
  }
}

// The plan's match kernel with a sink: one thread per site whichever the kernel.
template <class Sink>
static void ot_match_launch(hipStream_t st, const OtMatchPlan& m, const Sink& sink) {
  if (!m.n_sites || !m.n_guides) return;
  const dim3 grid((uint32_t)((m.n_sites + HAWK_BLOCK - 1) / HAWK_BLOCK)), block(HAWK_BLOCK);
  switch (m.kind) {
    case OT_MATCH_PAIRS:
      hipLaunchKernelGGL(k_ot_match_pairs<Sink>, grid, block, 0, st, m.sites, m.n_sites, m.ps, m.goff, m.gcode, m.gid, m.n_guides,
                         m.guidelen, m.sp0, m.max_mm, sink);
      break;
    case OT_MATCH_SEEDED:
      hipLaunchKernelGGL(k_ot_match_seeded<Sink>, grid, block, 0, st, m.sites, m.n_sites, m.sd, m.goff, m.gcode, m.gid, m.n_guides,
                         m.guidelen, m.sp0, m.max_mm, sink);
      break;
    case OT_MATCH_ALL:
      hipLaunchKernelGGL(k_ot_match<Sink>, grid, block, 0, st, m.sites, m.n_sites, m.guides, m.n_guides, m.guidelen, m.sp0, m.max_mm, sink);
      break;
  }
}
void hawk_launch_ot_match(hipStream_t st, const OtMatchPlan& m, OtHit* hits, uint64_t cap, unsigned long long* n_hits) {
  ot_match_launch(st, m, OtListSink{hits, cap, n_hits});
}
void hawk_launch_ot_match_sum(hipStream_t st, const OtMatchPlan& m, const OtSummary& sm) { ot_match_launch(st, m, OtSumSink{sm}); }

template <class Hit>
__global__ __launch_bounds__(256) void k_ot_gather(const OtSite* __restrict__ sites, const Hit* __restrict__ hits, uint64_t n_hits,
                                                   OtSite* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_hits) out[i] = sites[hits[i].site];
}
template <class Hit>
void hawk_launch_ot_gather(hipStream_t st, const OtSite* sites, const Hit* hits, uint64_t n_hits, OtSite* out) {
  if (n_hits) hipLaunchKernelGGL(k_ot_gather<Hit>, dim3((uint32_t)((n_hits + 255) / 256)), dim3(256), 0, st, sites, hits, n_hits, out);
}
template void hawk_launch_ot_gather<OtHit>(hipStream_t, const OtSite*, const OtHit*, uint64_t, OtSite*);
template void hawk_launch_ot_gather<OtBulgeHit>(hipStream_t, const OtSite*, const OtBulgeHit*, uint64_t, OtSite*);
