// hawk_rows.h - what "a surviving window start becomes a guide row" means, once, for the three searches that must write the same
// table: the plane search (hawk_search.hip), the per-dirty-word search of a plan view (hawk_vsearch.hip) and the per-distinct-
// cluster search (hawk_csearch.hip).  Geometry masks, padded window -> spacer+PAM core, the REF partner at the same (start,
// strand) and the redundancy verdict, CFDon, the staged position map, and the two row stores (GuideCols columns, 64-byte
// template rows).  All __device__ __forceinline__: a caller keeps its own load scheduling by where it places the calls.
#pragma once
#include "hawk_bits.h"

#define NSEG 64    // position-map segments staged per tile
__device__ __forceinline__ int seg_find(const uint32_t* s_rel, int n, uint32_t rel) {
  int lo = 0, hi = n;  // last j in [0,n) with s_rel[j] <= rel (s_rel[0] <= every rel of the tile)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s_rel[mid] <= rel) lo = mid; else hi = mid;
  }
  return lo;
}
// reverse the low L bits of a slice (bit i <-> bit L-1-i), 32 < L <= 64 or L <= 32
__device__ __forceinline__ W2 rev_bits(W2 v, int L) {
  const uint32_t rl = __brev(v.hi), rh = __brev(v.lo);  // 64-bit reversal
  const uint32_t sh = (uint32_t)(64 - L);               // then shift right by 64 - L (0 <= sh < 64)
  if (sh == 0) return W2{rl, rh};
  if (sh < 32) return W2{fsh(rl, rh, sh), rh >> sh};
  return W2{sh == 32 ? rh : rh >> (sh - 32), 0u};
}

// K4: CFDon on the 5'->3' guide.  Strand-1 slices are first turned into the 5'->3' guide (reverse the L
// bits, swap A<->T and C<->G planes = reverse complement), after which both strands read spacer base t at
// bit t and PAM[-2:] at bits L-2, L-1.  Only positions where REF and this guide differ contribute, visited
// in ascending t so the fp64 product is formed exactly as cfdscore.py:78-95 forms it.
__device__ __forceinline__ double cfdon_from_slices(const W2 (&core)[4], const W2 (&rcore)[4], uint32_t s, int L,
                                                    uint32_t cfdmask, const double* s_cfd, bool& err) {
  W2 g[4], r[4];
  if (s) {
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) { g[pl] = rev_bits(core[3 - pl], L); r[pl] = rev_bits(rcore[3 - pl], L); }
  } else {
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) { g[pl] = core[pl]; r[pl] = rcore[pl]; }
  }
  // spacer positions 0..min(guidelen,20)-1 all sit in the low word
  uint32_t diff = ((g[0].lo ^ r[0].lo) | (g[1].lo ^ r[1].lo) | (g[2].lo ^ r[2].lo) | (g[3].lo ^ r[3].lo)) & cfdmask;
  // a lookup needs both bases to be exactly one of A,C,G,T (else KeyError in the reference)
  const uint32_t g2 = (g[0].lo & g[1].lo) | ((g[0].lo | g[1].lo) & (g[2].lo | g[3].lo)) | (g[2].lo & g[3].lo);
  const uint32_t r2 = (r[0].lo & r[1].lo) | ((r[0].lo | r[1].lo) & (r[2].lo | r[3].lo)) | (r[2].lo & r[3].lo);
  err = (diff & (g2 | r2)) != 0;
  const uint32_t gb0 = g[1].lo | g[3].lo, gb1 = g[2].lo | g[3].lo;  // base index bits: A0 C1 G2 T3
  const uint32_t rb0 = r[1].lo | r[3].lo, rb1 = r[2].lo | r[3].lo;
  double score = 1.0;
  while (diff && !err) {
    const uint32_t t = (uint32_t)__builtin_ctz(diff);
    diff &= diff - 1;
    const uint32_t a = ((rb0 >> t) & 1u) | (((rb1 >> t) & 1u) << 1);
    const uint32_t b = ((gb0 >> t) & 1u) | (((gb1 >> t) & 1u) << 1);
    score *= s_cfd[(t * 4 + a) * 4 + b];
  }
  if (!err) {
    const int o0 = L - 2, o1 = L - 1;  // PAM[-2:] (wave-uniform positions)
    uint32_t c0 = 0, c1 = 0;
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
      c0 |= (((o0 < 32 ? g[pl].lo : g[pl].hi) >> (o0 & 31)) & 1u) << pl;
      c1 |= (((o1 < 32 ? g[pl].lo : g[pl].hi) >> (o1 & 31)) & 1u) << pl;
    }
    const int p0 = base_index(c0), p1 = base_index(c1);
    if (p0 < 0 || p1 < 0) err = true;
    else score *= s_cfd[320 + 4 * p0 + p1];
  }
  return err ? __longlong_as_double(0x7ff8000000000000ll) : score;
}

// ---- geometry: computed once per kernel --------------------------------------------------------------------------------
// window start q, spacer+PAM = L bits (the core), padded window = W = L + 2 * HAWK_PAD bits, 32 < W <= 64: the low word of a
// window is whole
struct RowGeom {
  int L, W;
  uint32_t mlo, mhi;  // the core's L bits as two word masks
  uint32_t whi;       // the window's high word
  uint32_t cfdmask;   // spacer positions CFD looks at: min(guidelen, 20)
};
__device__ __forceinline__ RowGeom row_geom(const ScanParams& p, const GuideParams& gp) {
  RowGeom g;
  g.L = p.L; g.W = p.L + 2 * HAWK_PAD;
  g.mlo = g.L >= 32 ? 0xffffffffu : ((1u << g.L) - 1u); g.mhi = g.L <= 32 ? 0u : ((1u << (g.L - 32)) - 1u);
  g.whi = g.W >= 64 ? 0xffffffffu : ((1u << (g.W - 32)) - 1u);
  g.cfdmask = (1u << (gp.guidelen < 20 ? gp.guidelen : 20)) - 1u;
  return g;
}
// the spacer+PAM core is the (masked) padded window without its pads
__device__ __forceinline__ W2 core_of_window(const W2& win, const RowGeom& g) {
  return W2{fsh(win.lo, win.hi, HAWK_PAD) & g.mlo, (win.hi >> HAWK_PAD) & g.mhi};
}
// 64 bits starting at bit `off` (0 <= off < 32) of a 96-bit string held as three words
__device__ __forceinline__ W2 ext96(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t off) { return W2{fsh(x0, x1, off), fsh(x1, x2, off)}; }
// the five padded windows and four cores of the window start at bit bpos of a word's 96-bit strings (bit 0 = the word's first
// start - HAWK_PAD); X(pl, k) is word k of plane pl's string, wherever the caller keeps it
template <class F>
__device__ __forceinline__ void row_slices(F X, uint32_t bpos, const RowGeom& g, W2 (&win)[5], W2 (&core)[4]) {
#pragma unroll
  for (int pl = 0; pl < 5; ++pl) {
    win[pl] = ext96(X(pl, 0), X(pl, 1), X(pl, 2), bpos);
    win[pl].hi &= g.whi;
    if (pl < 4) core[pl] = core_of_window(win[pl], g);
  }
}

// ---- the REF partner (search_guides.py:340-369) --------------------------------------------------------------------------
// A REF guide shares (start, strand) iff REF has a candidate window starting at qr = start - startp (REF's position map is the
// identity): one bit of the per-strand bitmaps of k_ref_bits.  The row is redundant iff REF's four code planes agree with its
// core as well.  In two halves: the probe issues the loads, the verdict consumes them - what a caller puts between the two
// (another survivor's probe) is in flight together with them.
struct RefProbe {
  bool inr;       // qr inside the bitmaps (else qr = 0: the loads stay in bounds and are ignored)
  uint32_t qr, rw;
  W2 rcore[4];
};
__device__ __forceinline__ RefProbe ref_probe_bit(const RefInfo& ri, int64_t start, uint32_t s) {
  RefProbe pr;
  const int64_t qr64 = start - ri.startp;
  pr.inr = qr64 >= 0 && qr64 < (int64_t)ri.n_bits;
  pr.qr = pr.inr ? (uint32_t)qr64 : 0u;
  pr.rw = (s ? ri.bits[1] : ri.bits[0])[pr.qr >> 5];
  return pr;
}
__device__ __forceinline__ bool probe_has_ref(const RefProbe& pr) { return pr.inr && ((pr.rw >> (pr.qr & 31u)) & 1u); }
__device__ __forceinline__ void ref_probe_cores(RefProbe& pr, const uint32_t* const* ref_planes) {
#pragma unroll
  for (int pl = 0; pl < 4; ++pl) pr.rcore[pl] = ext_glb(ref_planes[pl], pr.qr);
}
// bitmap word and REF's four cores, whether or not the bit turns out set: one round trip instead of two
__device__ __forceinline__ RefProbe ref_probe(const RefInfo& ri, const uint32_t* const* ref_planes, int64_t start, uint32_t s) {
  RefProbe pr = ref_probe_bit(ri, start, s);
  ref_probe_cores(pr, ref_planes);
  return pr;
}
// true: the row is REF's guide again (remove_redundant_guides).  rcore = REF's core, or the row's own where REF has no guide.
__device__ __forceinline__ bool ref_verdict(const RefProbe& pr, const W2 (&core)[4], const RowGeom& g, W2 (&rcore)[4], bool& has_ref) {
  has_ref = probe_has_ref(pr);
  bool same = has_ref;
#pragma unroll
  for (int pl = 0; pl < 4; ++pl) {
    rcore[pl] = pr.rcore[pl];
    rcore[pl].lo &= g.mlo; rcore[pl].hi &= g.mhi;  // (masked in place: built as a new W2, k_vsearch takes 2 VGPRs and 1.4 % more)
    same = same && rcore[pl].lo == core[pl].lo && rcore[pl].hi == core[pl].hi;
    if (!has_ref) rcore[pl] = core[pl];
  }
  return same;
}

// CFDon of a row: NaN ("NA") without a REF partner or when not asked for; a non-ACGT base under a lookup is an error under
// score_cfdon == 1 and NaN under score_cfdon == 2
__device__ __forceinline__ double row_cfdon(const GuideParams& gp, bool has_ref, const W2 (&core)[4], const W2 (&rcore)[4], uint32_t s,
                                            const RowGeom& g, const double* s_cfd, int* status) {
  double score = __longlong_as_double(0x7ff8000000000000ll);
  if (gp.score_cfdon && has_ref) {
    bool err;
    score = cfdon_from_slices(core, rcore, s, g.L, g.cfdmask, s_cfd, err);
    if (err && gp.score_cfdon == 1) atomicExch(status, -5 /* HAWK_E_CFD */);
  }
  return score;
}

// ---- position map (haplotype.py:90-159) from the segments a tile staged in LDS ---------------------------------------------
// unused slots of s_segrel hold 0xffffffff: a fixed six-step search needs no bounds
__device__ __forceinline__ int64_t posmap_staged(const uint32_t* s_segrel, const int64_t* s_seggen, uint32_t rel) {
  uint32_t sj = 0;
#pragma unroll
  for (uint32_t step = NSEG / 2; step; step >>= 1) sj += (s_segrel[sj + step] <= rel) ? step : 0u;
  return s_seggen[sj] + (int64_t)(rel - s_segrel[sj]);
}
// start = posmap[q] and stop = posmap[q + L] (search_guides.py:260-280) over the nloc staged segments; no second search when no
// segment starts inside the window
__device__ __forceinline__ void posmap_staged_span(const uint32_t* s_segrel, const int64_t* s_seggen, int nloc, uint32_t q, int L, int64_t& start,
                                                   int64_t& stop) {
  const int j = seg_find(s_segrel, nloc, q);
  start = s_seggen[j] + (int64_t)(q - s_segrel[j]);
  if (j + 1 >= nloc || s_segrel[j + 1] > q + (uint32_t)L) stop = start + L;
  else { const int j2 = seg_find(s_segrel, nloc, q + (uint32_t)L); stop = s_seggen[j2] + (int64_t)(q + (uint32_t)L - s_segrel[j2]); }
}

// ---- the two row stores ----------------------------------------------------------------------------------------------------
// row o of a columnar table: window start q of haplotype row h, strand s.  pos names the spacer's first base (the PAM leads on
// strand 0 of a right-sided PAM and on strand 1 of a left-sided one).
__device__ __forceinline__ void cols_store(const GuideCols& out, uint64_t o, uint32_t h, uint32_t q, uint32_t s, int64_t start, int64_t stop,
                                           bool has_ref, const W2 (&win)[5], double score, const ScanParams& p, int* status) {
  if (o >= out.cap) { atomicExch(status, -3 /* HAWK_E_CAPACITY: offsets and counts disagree */); return; }
  const bool pamfirst = (p.right != 0) != (s != 0);
  out.hap[o] = h;
  out.pos[o] = pamfirst ? q : q + (uint32_t)p.guidelen;
  out.strand[o] = (uint8_t)s;
  out.start[o] = start;
  out.stop[o] = stop;
  out.flags[o] = has_ref ? 1 : 0;
#pragma unroll
  for (int pl = 0; pl < HAWK_PLANES; ++pl) out.win[(size_t)pl * out.cap + o] = (uint64_t)win[pl].lo | ((uint64_t)win[pl].hi << 32);
  out.cfdon[o] = score;
}

// A template row of the cluster search, 64 bytes = one L2 sector pair, and with words 0 and 1 patched a row of the packed table:
//   a = {pos - o_first (packed: pos), strand | has_ref << 1 (packed: | haplotype row << HAWK_ROW_HAP_SHIFT), start - startp, stop - start}
//   b = {cfdon (two words), win0}   c = {win1, win2}   d = {win3, win4}
// o_first: the row position of the cluster's first allele.  THE place that packs one; k_cs_emit_rows, k_rows_pack / k_rows_unpack
// and k_cc_mini read or restate this order.
struct __attribute__((aligned(16))) CsRow { uint4 a, b, c, d; };
static_assert(sizeof(CsRow) == 64, "template row layout");
__device__ __forceinline__ void template_row_store(CsRow* __restrict__ trows, uint64_t k, uint64_t t_cap, uint32_t q, int32_t o_first, uint32_t s,
                                                   int64_t start, int64_t stop, int64_t startp, bool has_ref, const W2 (&win)[5], double score,
                                                   const ScanParams& p, int* status) {
  if (k >= t_cap) { atomicExch(status, -3 /* HAWK_E_CAPACITY: more rows than window starts */); return; }
  const bool pamfirst = (p.right != 0) != (s != 0);
  const int64_t ds = start - startp, de = stop - start;
  if (ds < INT32_MIN || ds > INT32_MAX || de < INT32_MIN || de > INT32_MAX) atomicExch(status, -7 /* HAWK_E_UNSUPPORTED */);
  const uint64_t sc = (uint64_t)__double_as_longlong(score);
  uint4* __restrict__ tp = reinterpret_cast<uint4*>(trows + k);
  tp[0] = make_uint4((uint32_t)((int32_t)(pamfirst ? q : q + (uint32_t)p.guidelen) - o_first), s | (has_ref ? 2u : 0u), (uint32_t)(int32_t)ds,
                     (uint32_t)(int32_t)de);
  tp[1] = make_uint4((uint32_t)sc, (uint32_t)(sc >> 32), win[0].lo, win[0].hi);
  tp[2] = make_uint4(win[1].lo, win[1].hi, win[2].lo, win[2].hi);
  tp[3] = make_uint4(win[3].lo, win[3].hi, win[4].lo, win[4].hi);
}
