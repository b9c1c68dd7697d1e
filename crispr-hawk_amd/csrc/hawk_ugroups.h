// hawk_ugroups.h - what the kept guides of an unphased resolution (hawk_resolve.h) become in the guide report
// (reports.report_from_guides, scoring.cfdon_score): the key the report merges on, CFDon against the REF guide at the same
// (start, strand), and the G/C counts of a spacer - stated ONCE for the host (hawk_host_unphased_groups, hawk_hostutil.hip) and
// the device (k_ug_keys / k_ug_heads / k_ug_emit, hawk_ugroups.hip).
//
//   guide k    (source row src_row[k], window win[0..4][k]) with the table row's start, stop, strand, hap, pos.
//   key        UG_KEY_WORDS 64-bit words, compared most significant first:
//                [0] start (sign bit flipped: ascending as signed)   [1] strand * 2 + origin (the row's haplotype is REF)
//                [2] stop (sign bit flipped)   [3 .. 7] the case-preserving core: planes A, C, G, T, case at window offsets
//                [10 - fl, W - 10 + fr), shifted down to bit 0.  fl / fr are flank_up / flank_down in GUIDE orientation, as
//                hawk_table_collapse_ex defines them: on strand 1 the guide's 5' side is the window's high side, so fl = down and
//                fr = up there.  (0, 0): the plain report; (4, 3): the k-mer the model scorers read.
//              Two guides share a group iff all words are equal.  Groups come out ascending by the words in this order.  (The
//              rounded CFDon of report_from_guides' key is a function of these words.)
//   tie        inside a group the guides are ordered by (hap << 32 | pos, k): the reference's emission order inside one (start,
//              strand), k ascending = combination order.  The first is the representative; the member list holds each
//              haplotype once, ascending.
//   CFDon      cfdon_from_slices (hawk_rows.h) on uint64_t slices: strand-1 cores become the 5'->3' guide (reverse the L bits,
//              swap A<->T and C<->G), then only the positions among the first min(guidelen, 20) where REF and the guide differ
//              contribute, in ascending position, one fp64 multiply each, then PAM[-2:] (bits L - 2, L - 1) - the same product
//              in the same order, products only.  A base under a lookup that is not one of A C G T: *err.
//   GC         of the spacer inside the + strand core (behind the PAM when right XOR strand), as hawk_table_collapse counts:
//              num = C, G, S; den = num + A, T, W.
// No device code and no state here: the header compiles as plain C++ too.
#pragma once
#include <stdint.h>

#ifndef HAWK_HD
#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif
#endif

#define UG_PAD 10
#define UG_PLANES 5
#define UG_KEY_WORDS 8
#define UG_MAX_FLANK 10u
#define UG_CFD_MM 320  // [20][4][4]: position, REF base, guide base
#define UG_CFD_PAM 16
#define UG_BYTES_PER_GUIDE 44ull  // what the fill pass writes per kept guide: src_row + five window slices

struct UgGeom {
  int32_t guidelen, pamlen, right, W, L;
  int32_t up, down;  // flank_up / flank_down, guide orientation
};

HAWK_HD inline uint64_t ug_low_mask(int n) { return n >= 64 ? ~0ull : (n <= 0 ? 0ull : ((1ull << n) - 1ull)); }
HAWK_HD inline uint64_t ug_bias(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
HAWK_HD inline int64_t ug_unbias(uint64_t v) { return (int64_t)(v ^ 0x8000000000000000ull); }
// bits the core words of a key occupy (the sort passes stop there)
HAWK_HD inline int ug_key_width(const UgGeom& g) { return g.L + g.up + g.down; }

// the key of a guide: start / stop / strand of its row, origin = the row's haplotype is REF, win = its five window slices
HAWK_HD inline void ug_key(const UgGeom& g, int64_t start, int64_t stop, uint32_t strand, bool origin, const uint64_t* win, uint64_t* key) {
  const int fl = strand ? g.down : g.up, fr = strand ? g.up : g.down;
  const uint64_t m = ug_low_mask(g.L + fl + fr);
  key[0] = ug_bias(start);
  key[1] = (uint64_t)(strand ? 2u : 0u) | (origin ? 1u : 0u);
  key[2] = ug_bias(stop);
  for (int pl = 0; pl < UG_PLANES; ++pl) key[3 + pl] = (win[pl] >> (UG_PAD - fl)) & m;
}

// the L-bit spacer + PAM core of a window plane
HAWK_HD inline uint64_t ug_core(uint64_t w, const UgGeom& g) { return (w >> UG_PAD) & ug_low_mask(g.L); }
// reverse the low L bits (bit i <-> bit L - 1 - i), 1 <= L <= 64
HAWK_HD inline uint64_t ug_rev_bits(uint64_t v, int L) {
  v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
  v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
  v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
  v = ((v >> 8) & 0x00ff00ff00ff00ffull) | ((v & 0x00ff00ff00ff00ffull) << 8);
  v = ((v >> 16) & 0x0000ffff0000ffffull) | ((v & 0x0000ffff0000ffffull) << 16);
  v = (v >> 32) | (v << 32);
  return L >= 64 ? v : v >> (64 - L);
}
HAWK_HD inline int ug_base_index(uint32_t code) {  // A, C, G, T -> 0 .. 3, anything else -1
  if (code == 0 || (code & (code - 1u))) return -1;
  return code == 1u ? 0 : code == 2u ? 1 : code == 4u ? 2 : 3;
}
HAWK_HD inline uint32_t ug_ctz32(uint32_t v) {  // v != 0
  uint32_t t = 0;
  while (!((v >> t) & 1u)) ++t;
  return t;
}

// CFDon of a guide against its REF partner.  core / rcore: the four code planes of the two L-bit cores on the + strand
// (ug_core); mm[320] / pam[16] the tables.  *err: a lookup met a base that is not one of A C G T (the value is then NaN's place:
// the caller decides).
HAWK_HD inline double ug_cfdon(const uint64_t* core, const uint64_t* rcore, uint32_t strand, const UgGeom& g, const double* mm, const double* pam,
                               bool* err) {
  uint64_t gd[4], rf[4];
  for (int pl = 0; pl < 4; ++pl) {
    gd[pl] = strand ? ug_rev_bits(core[3 - pl], g.L) : core[pl];
    rf[pl] = strand ? ug_rev_bits(rcore[3 - pl], g.L) : rcore[pl];
  }
  const uint32_t cfdmask = (uint32_t)ug_low_mask(g.guidelen < 20 ? g.guidelen : 20);
  const uint32_t g0 = (uint32_t)gd[0], g1 = (uint32_t)gd[1], g2 = (uint32_t)gd[2], g3 = (uint32_t)gd[3];
  const uint32_t r0 = (uint32_t)rf[0], r1 = (uint32_t)rf[1], r2 = (uint32_t)rf[2], r3 = (uint32_t)rf[3];
  uint32_t diff = ((g0 ^ r0) | (g1 ^ r1) | (g2 ^ r2) | (g3 ^ r3)) & cfdmask;
  const uint32_t gm = (g0 & g1) | ((g0 | g1) & (g2 | g3)) | (g2 & g3);  // positions with more than one base
  const uint32_t rm = (r0 & r1) | ((r0 | r1) & (r2 | r3)) | (r2 & r3);
  bool bad = (diff & (gm | rm)) != 0;
  const uint32_t gb0 = g1 | g3, gb1 = g2 | g3, rb0 = r1 | r3, rb1 = r2 | r3;  // base index bits: A0 C1 G2 T3
  double score = 1.0;
  while (diff && !bad) {
    const uint32_t t = ug_ctz32(diff);
    diff &= diff - 1;
    const uint32_t a = ((rb0 >> t) & 1u) | (((rb1 >> t) & 1u) << 1);
    const uint32_t b = ((gb0 >> t) & 1u) | (((gb1 >> t) & 1u) << 1);
    score *= mm[(t * 4 + a) * 4 + b];
  }
  if (!bad) {
    uint32_t c0 = 0, c1 = 0;
    for (int pl = 0; pl < 4; ++pl) {
      c0 |= (uint32_t)((gd[pl] >> (g.L - 2)) & 1u) << pl;
      c1 |= (uint32_t)((gd[pl] >> (g.L - 1)) & 1u) << pl;
    }
    const int p0 = ug_base_index(c0), p1 = ug_base_index(c1);
    if (p0 < 0 || p1 < 0) bad = true;
    else score *= pam[4 * p0 + p1];
  }
  *err = bad;
  return score;
}

HAWK_HD inline uint32_t ug_popc64(uint64_t v) {
  v = v - ((v >> 1) & 0x5555555555555555ull);
  v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
  v = (v + (v >> 4)) & 0x0f0f0f0f0f0f0f0full;
  return (uint32_t)((v * 0x0101010101010101ull) >> 56);
}
// G/C counts of the spacer of a window: num | den << 8
HAWK_HD inline uint32_t ug_gc(const uint64_t* win, uint32_t strand, const UgGeom& g) {
  const bool pamfirst = (g.right != 0) != (strand != 0);
  const int sh = UG_PAD + (pamfirst ? g.pamlen : 0);
  const uint64_t m = ug_low_mask(g.guidelen);
  const uint64_t A = (win[0] >> sh) & m, C = (win[1] >> sh) & m, G = (win[2] >> sh) & m, T = (win[3] >> sh) & m;
  const uint64_t gc = (C | G) & ~(A | T), at = (A | T) & ~(C | G);
  return ug_popc64(gc) | (ug_popc64(gc | at) << 8);
}

// geometry and flanks the kernels and the twin refuse alike: 0 fine, 1 invalid, 2 unsupported
HAWK_HD inline int ug_check_geom(const UgGeom& g, uint32_t up, uint32_t down) {
  if (g.guidelen < 1 || g.pamlen < 1 || g.pamlen > 16 || g.W != g.guidelen + g.pamlen + 2 * UG_PAD || g.L != g.guidelen + g.pamlen) return 1;
  if (g.W > 64 || up > UG_MAX_FLANK || down > UG_MAX_FLANK) return 2;
  return 0;
}
