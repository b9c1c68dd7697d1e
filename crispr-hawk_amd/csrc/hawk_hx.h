// hawk_hx.h - records of an expansion plan and the word builder shared by the expansion kernel (hawk_expand.hip) and the
// search that runs straight from a plan (hawk_vsearch.hip), and the (row, tile) workgroup's staging and word assembly shared by the
// expansion kernel and the text kernel (hawk_haptext.hip).  See hawk_expand.hip for what the records mean.
#pragma once
#include "hawk_bits.h"

#define HX_TW 1024        // output words a workgroup builds: 32768 positions, four consecutive words per thread
#define HX_MAXV 96        // carried variants staged per workgroup (32 B each; more: the rest from global memory)
#define HX_RW (HX_TW + 64)  // REF words staged per plane: the tile's image in REF plus up to 2048 net deleted bases

// o: output start; rs = r0 + span: where REF resumes behind the alt allele; m: the first 32 alt bases as plane bits
struct __attribute__((aligned(16))) HxVar { int32_t o; uint32_t rs; uint32_t alt_len; uint32_t alt_off; uint32_t m[4]; };
// what a workgroup of k_hx_build starts from: one 16-byte scalar load
struct __attribute__((aligned(16))) HxTile {
  uint32_t first_lo, first_hi;  // index (over all rows) of the first record to stage
  uint32_t n_flags;             // records to stage | HX_FITS | HX_ALL
  uint32_t ws;                  // first REF word of the staged window (a multiple of 4)
};
#define HX_FITS (1u << 31)  // the tile's REF image fits the staged window
#define HX_ALL (1u << 30)   // every record the tile needs is staged
#define HX_HEAD (1u << 29)  // the first staged record starts at or before the tile (otherwise the tile starts in unmodified REF)

__device__ __forceinline__ uint32_t hx_low(int n) { return n >= 32 ? 0xffffffffu : (n > 0 ? (1u << n) - 1u : 0u); }

// NW consecutive 32-base words of one row, starting at output position p0 (any position >= 0).  FAST: every record the
// words need is among the n staged ones `s_v`; otherwise records beyond the staged ones come from global memory
// (`first[j]`, j < j_end = the row's records from `first` on).  Records are addressed locally: j = 0 is the first staged
// one.  `ref32(pl, r)` returns 32 bits of REF plane pl from bit r (the caller decides where REF lives).
//
// A word is written as: REF copied under the mapping in force at its first position (the allele of variant k reaching
// into the word first, if it does), then one round per variant starting inside the word - its alt bases shifted out of
// the record's plane bits over what is there, and only when the variant changes the mapping (an indel; a SNV does not)
// the rest of the word copied again.  A round is ~40 instructions; the first version looped over pieces (copy, allele,
// copy ...: three rounds of both branches per variant, 1000 vector instructions per wave).
template <bool FAST, int NW, class RefFn>
__device__ __forceinline__ void hx_words_t(const uint8_t* __restrict__ alt_codes, const HxVar* __restrict__ s_v,
                                           const HxVar* __restrict__ first, int n, int j_end /* records of the row from `first` on */,
                                           bool head, int32_t p0, int32_t len, RefFn ref32,
                                           uint32_t (&oA)[NW], uint32_t (&oC)[NW], uint32_t (&oG)[NW], uint32_t (&oT)[NW], uint32_t (&oV)[NW]) {
  auto getv = [&](int j) -> HxVar { return FAST || j < n ? s_v[j] : first[j]; };
  // FAST: a variant behind the staged ones starts behind everything the words read - all that matters about it
  auto geto = [&](int j) -> int32_t {
    if (FAST) return j < n ? s_v[j].o : 0x7fffffff;
    return j < n ? s_v[j].o : (j < j_end ? first[j].o : 0x7fffffff);
  };
  // k: local index of the last carried variant with o <= p0 (-1: none; only possible when the first staged record
  // starts behind p0).  Records before the first staged one start before it.
  int a = head ? 1 : 0, b = FAST ? n : j_end;
  while (a < b) { const int m = (a + b) >> 1; if (geto(m) <= p0) a = m + 1; else b = m; }
  int k = a - 1;
  // the stretch in force, reloaded when k moves: alt allele [v.o, v_end), behind it REF copied with r = r_base + p
  HxVar v;
  v.o = 0; v.rs = 0; v.alt_len = 0; v.alt_off = 0; v.m[0] = v.m[1] = v.m[2] = v.m[3] = 0;
  int32_t v_end = 0, r_base = 0, next_o = 0x7fffffff;  // k < 0: an empty allele at position 0, REF copied 1:1
  auto load = [&]() {
    if (k >= 0) {
      v = getv(k);
      v_end = v.o + (int32_t)v.alt_len;
      r_base = (int32_t)v.rs - v_end;
    }
    next_o = geto(k + 1);  // output start of the following variant
  };
  load();
#pragma unroll
  for (int wi = 0; wi < NW; ++wi) {
    const int32_t wp0 = p0 + 32 * wi;
    const int32_t wend = wp0 + 32 < len ? wp0 + 32 : len;
    if (next_o <= wp0) { ++k; load(); }  // a variant starting exactly at the word
    uint32_t xA = 0, xC = 0, xG = 0, xT = 0, xV = 0;
    int32_t cs = 0;  // first bit of the word the REF copy fills
    if (wp0 < v_end) {  // the allele of variant k reaches into (or starts at) the word
      const int src = wp0 - v.o, na = v_end - wp0;
      const uint32_t am = hx_low(na);
      if (v.alt_len <= 32u) {
        xA = (v.m[0] >> src) & am; xC = (v.m[1] >> src) & am; xG = (v.m[2] >> src) & am; xT = (v.m[3] >> src) & am;
      } else {  // an insertion longer than a word: base by base from the allele text
        for (int32_t q = wp0; q < v_end && q < wend; ++q) {
          const uint32_t c = alt_codes[v.alt_off + (uint32_t)(q - v.o)], bit = 1u << (q - wp0);
          if (c & 1u) xA |= bit; if (c & 2u) xC |= bit; if (c & 4u) xG |= bit; if (c & 8u) xT |= bit;
        }
      }
      xV = am;
      cs = na;
    }
    if (cs < 32) {
      const uint32_t r = (uint32_t)(r_base + wp0 + cs);
      xA |= ref32(0, r) << cs; xC |= ref32(1, r) << cs; xG |= ref32(2, r) << cs; xT |= ref32(3, r) << cs;
    }
    while (next_o < wend) {  // one round per variant starting inside the word
      const int32_t rb_prev = r_base;
      ++k; load();
      const int s = v.o - wp0;  // 1 .. 31
      const uint32_t am = hx_low((int)v.alt_len) << s;
      if (v.alt_len <= 32u) {
        xA = (xA & ~am) | (v.m[0] << s); xC = (xC & ~am) | (v.m[1] << s); xG = (xG & ~am) | (v.m[2] << s); xT = (xT & ~am) | (v.m[3] << s);
      } else {
        xA &= ~am; xC &= ~am; xG &= ~am; xT &= ~am;
        for (int32_t q = v.o; q < wend; ++q) {  // the allele covers the rest of the word
          const uint32_t c = alt_codes[v.alt_off + (uint32_t)(q - v.o)], bit = 1u << (q - wp0);
          if (c & 1u) xA |= bit; if (c & 2u) xC |= bit; if (c & 4u) xG |= bit; if (c & 8u) xT |= bit;
        }
      }
      xV |= am;
      const int e = v_end - wp0;  // where REF resumes
      if (r_base != rb_prev && e < 32) {  // an indel: the rest of the word maps elsewhere
        const uint32_t cm = 0xffffffffu << e, r = v.rs;
        xA = (xA & ~cm) | (ref32(0, r) << e); xC = (xC & ~cm) | (ref32(1, r) << e);
        xG = (xG & ~cm) | (ref32(2, r) << e); xT = (xT & ~cm) | (ref32(3, r) << e);
      }
    }
    const uint32_t wm = hx_low(wend - wp0);  // the row ends inside (or before) the word
    oA[wi] = xA & wm; oC[wi] = xC & wm; oG[wi] = xG & wm; oT[wi] = xT & wm; oV[wi] = xV & wm;
  }
}

// Staged REF word i of a plane lives at (i & 3) * HX_RW / 4 + (i >> 2): a thread owns four consecutive output words, so
// the lanes of a wave read words 4 apart - a 4-way bank conflict in the natural layout, consecutive banks in this one.
__device__ __forceinline__ uint32_t hx_slot(uint32_t i) { return (i & 3u) * (HX_RW / 4) + (i >> 2); }

struct HxArgs {
  const uint32_t* ref[4];
  uint32_t ref_S;
  const HxVar* recs;
  const uint8_t* alt_codes;
};

// The four words of one thread (hx_words_t, hawk_hx.h).  FAST: every record the tile needs and its whole REF image are in
// LDS (the usual tile); otherwise records beyond the staged ones and / or the REF words come from global memory.
template <bool FAST>
__device__ __forceinline__ void hx_words(const HxArgs& g, const HxVar* __restrict__ s_v, const uint32_t (*__restrict__ s_ref)[HX_RW],
                                         const HxVar* __restrict__ first, int n, int j_end /* records of the row from `first` on */,
                                         bool head, bool staged, uint32_t ws, int32_t p0, int32_t len,
                                         uint32_t (&oA)[4], uint32_t (&oC)[4], uint32_t (&oG)[4], uint32_t (&oT)[4], uint32_t (&oV)[4]) {
  // 32 bits of REF plane pl from bit r.  A read under a mapping that a later variant of the word replaces, or of bits
  // past the end of the row, may point outside what exists: the word index is clamped, the bits are overwritten / masked.
  auto ref32 = [&](int pl, uint32_t r) -> uint32_t {
    if (FAST || staged) {
      uint32_t w = (r >> 5) - ws;
      w = w < HX_RW - 2 ? w : HX_RW - 2;
      return fsh(s_ref[pl][hx_slot(w)], s_ref[pl][hx_slot(w + 1)], r & 31u);
    }
    const uint32_t w = (r >> 5) < g.ref_S - 3 ? (r >> 5) : g.ref_S - 3;
    return ext_glb(g.ref[pl], (w << 5) | (r & 31u)).lo;
  };
  hx_words_t<FAST, 4>(g.alt_codes, s_v, first, n, j_end, head, p0, len, ref32, oA, oC, oG, oT, oV);
}

// One thread's part of a (row, tile) workgroup of HAWK_BLOCK threads, shared by k_hx_build (the words go to the planes) and
// k_hx_text (hawk_haptext.hip: the words become letters): the tile's records and its image in the REF planes are staged in LDS
// (two independent coalesced loads, in flight together), the workgroup waits once, then the thread builds the four words from
// w0 - zero where the row has ended.  Every thread of the workgroup must call it (it holds a barrier).
__device__ __forceinline__ void hx_tile_quad(const HxArgs& g, const uint64_t* __restrict__ hv_off, uint32_t h, const HxTile t, int32_t len, uint32_t w0,
                                             HxVar* __restrict__ s_v, uint32_t (*__restrict__ s_ref)[HX_RW],
                                             uint32_t (&oA)[4], uint32_t (&oC)[4], uint32_t (&oG)[4], uint32_t (&oT)[4], uint32_t (&oV)[4]) {
  const int n = (int)(t.n_flags & 0xffffu);
  const bool staged = (t.n_flags & HX_FITS) != 0, all = (t.n_flags & HX_ALL) != 0, head = (t.n_flags & HX_HEAD) != 0;
  const uint32_t ws = t.ws;
  const HxVar* first = g.recs + (((uint64_t)t.first_hi << 32) | t.first_lo);
  if (staged) {  // the REF words the tile's copies read: 16-byte loads, each word to its swizzled slot
    for (uint32_t i = threadIdx.x; i < HX_RW / 4; i += HAWK_BLOCK) {
      const uint32_t w = ws + 4 * i + 4 <= g.ref_S ? ws + 4 * i : g.ref_S - 4;  // rows are whole 16-byte quads
#pragma unroll
      for (int pl = 0; pl < 4; ++pl) {
        const uint4 q = *reinterpret_cast<const uint4*>(g.ref[pl] + w);
        s_ref[pl][i] = q.x; s_ref[pl][HX_RW / 4 + i] = q.y; s_ref[pl][2 * (HX_RW / 4) + i] = q.z; s_ref[pl][3 * (HX_RW / 4) + i] = q.w;
      }
    }
  }
  if ((int)threadIdx.x < n) s_v[threadIdx.x] = first[threadIdx.x];  // n <= HX_MAXV < workgroup size
  __syncthreads();
  const int32_t p0 = (int32_t)(w0 * 32u);
  if (w0 * 32u < (uint32_t)len) {  // (unsigned: the words of a tile may lie behind the stride, past 2^31 positions)
    if (staged && all) {
      hx_words<true>(g, s_v, s_ref, first, n, n, head, true, ws, p0, len, oA, oC, oG, oT, oV);
    } else {  // more records than LDS holds start inside the tile (one every 200 nt over all of it), or a long REF image
      const int j_end = (int)(g.recs + hv_off[h + 1] - first);
      hx_words<false>(g, s_v, s_ref, first, n, j_end, head, staged, ws, p0, len, oA, oC, oG, oT, oV);
    }
  }
}
