// hawk_otbulge.h - a bulged (site, guide) pair stated once: its shift vectors, the placement selection and (otb_pair) the row the
// pair makes - mismatches, gaps and the CFD of the off-targets table's row.  Shared by k_ot_bulge (hawk_otbulge.hip), by the host
// twin of the bulged summary (hawk_host_offtarget_bulge_summary, hawk_hostutil.hip) and by the host programs that check it against
// plain restatements (otbulge_check_main.cpp, otbsum_check_main.cpp).  Plain C++: no device types.
//
// A bulge of b bases aligns a LONGER sequence of span = n + b positions (DNA bulge: the site spacer; RNA bulge: the guide) with a
// SHORTER one of n positions (DNA: the guide; RNA: the site spacer); b interior positions 1 .. span - 2 of the longer one - the
// gaps - face nothing.  Position j of the shorter one faces position j + k of the longer one, k = the gaps in front of it, so the
// mismatches of every placement are read off b + 1 shift vectors
//   m[k], bit 2 j set <=> shorter[j] differs from longer[j + k], or the site base of the two is ambiguous     (j < n)
// (one bit per base at the even positions, as the folded XOR of two 2-bit codes leaves it).  With gaps p (b = 1) or p1 < p2 (b = 2):
//   b = 1:  popc(m0 & low(p))  + popc(m1 & ~low(p))
//   b = 2:  popc(m0 & low(p1)) + popc(m1 & low(p2 - 1) & ~low(p1)) + popc(m2 & ~low(p2 - 1))         low(x) = positions < x
// The winner is the placement with the fewest mismatches, ties to the lexicographically smallest gap tuple
// (oracle/hawk_oracle.c: ora_offtargets_bulges).
#pragma once
#include <stdint.h>

#include "hawk_ottext.h"

#ifdef __HIPCC__
#define OTB_HD __host__ __device__ inline __attribute__((always_inline))  // __forceinline__, spelt out: hawk_hostutil.hip includes no HIP header
#else
#define OTB_HD inline
#endif

#define OTB_EVEN 0x5555555555555555ull
OTB_HD uint64_t otb_low(int x) { return (1ull << (2 * x)) - 1ull; }  // positions < x, x <= 31
OTB_HD int otb_popc(uint64_t v) { return __builtin_popcountll(v); }
// the lower bound every placement shares: a position that mismatches under every shift mismatches wherever the gaps are
OTB_HD int otb_floor(const uint64_t* m, int b) {
  uint64_t a = m[0];
  for (int k = 1; k <= b; ++k) a &= m[k];
  return otb_popc(a);
}

struct OtbBest { int mm; uint32_t gaps; };  // mm > max_mm: no placement within max_mm

// `forbid` bit p: position p of the longer sequence may not be a gap (DNA bulges: an ambiguous site base is never bulged out).
// b = 1 walks p upwards and keeps a strictly smaller count.  b = 2 does not walk the (span - 2)(span - 3) / 2 pairs: with
//   e(x) = popc(m0 & low(x)) - popc(m1 & low(x)),  d(y) = popc(m1 & low(y)) - popc(m2 & low(y)),  y = p2 - 1 >= p1,
// the count of (p1, p2) is e(p1) + popc(m2) + d(p2 - 1), so the best p2 of a p1 is the first minimum of d over [p1, span - 3]: one
// pass downwards keeps that running minimum (taking an equal value moves it to the smaller p2) and the best total (taking an
// equal total moves it to the smaller p1) - the pair the upward walk with "strictly smaller" ends on.
OTB_HD OtbBest otb_best(const uint64_t* m, int b, int span, uint32_t forbid, int max_mm) {
  OtbBest r;
  r.mm = max_mm + 1;
  r.gaps = 0;
  if (b == 1) {
    const int t1 = otb_popc(m[1]);
    for (int p = 1; p <= span - 2; ++p) {
      const uint64_t lo = otb_low(p);
      const int mm = otb_popc(m[0] & lo) + t1 - otb_popc(m[1] & lo);
      if (mm < r.mm && !((forbid >> p) & 1u)) { r.mm = mm; r.gaps = 1u << p; }
    }
    return r;
  }
  const int t2 = otb_popc(m[2]), none = 1 << 20;
  int dmin = none, arg = 0;
  for (int x = span - 3; x >= 1; --x) {
    const uint64_t lo = otb_low(x);
    const int c0 = otb_popc(m[0] & lo), c1 = otb_popc(m[1] & lo), c2 = otb_popc(m[2] & lo);
    const int d = c1 - c2;
    if (d <= dmin && !((forbid >> (x + 1)) & 1u)) { dmin = d; arg = x; }  // p2 = x + 1
    if (dmin != none && !((forbid >> x) & 1u)) {                          // p1 = x
      const int mm = c0 - c1 + t2 + dmin;
      if (mm <= r.mm) { r.mm = mm; r.gaps = (1u << x) | (1u << (arg + 1)); }
    }
  }
  return r;
}

// spread the 32 bits of x to the even bit positions of a 64-bit word
OTB_HD uint64_t otb_spread(uint32_t x) {
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
OTB_HD void otb_vectors(uint64_t code, uint32_t nmsp, uint64_t g, uint64_t even, uint64_t (&m)[B + 1]) {
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int k = 0; k <= B; ++k) {
    const uint64_t x = DNA ? (g ^ (code >> (2 * k))) : (code ^ (g >> (2 * k)));
    m[k] = ((x | (x >> 1)) | otb_spread(DNA ? (nmsp >> k) : nmsp)) & even;
  }
}

// The row of one pair, from the site's WINDOW as a site record holds it (wcode / wnmask: Gs + P bases in guide orientation,
// Gs = G + B for a DNA bulge, G - B for an RNA bulge; the PAM in front when `right`) and the guide's code: the placement otb_best
// selects and, when it is within max_mm, the CFD of the row the off-targets table prints for it - ot_text_row (hawk_ottext.h) on
// the record the pair makes, its text discarded, so the units are the table's by construction.  mm > max_mm: no row (gaps and
// units mean nothing).  units: OT_TEXT_NA without tables, OT_TEXT_UNSCORABLE as ot_text_row has it.
// Needs B + 3 <= G <= 32 and Gs + P <= 32 (hawk_offtarget_bulges' refusals).
struct OtbPair { int mm; uint32_t gaps; long long units; };

template <int B, bool DNA>
OTB_HD OtbPair otb_pair_t(uint64_t wcode, uint32_t wnmask, uint64_t g, int G, int P, int right, int max_mm, const double* tab) {
  const int Gs = DNA ? G + B : G - B, n = DNA ? G : Gs, span = n + B, sp0 = right ? P : 0;
  const uint64_t even = (n >= 32 ? ~0ull : otb_low(n)) & OTB_EVEN;
  const uint64_t code = (wcode >> (2 * sp0)) & (Gs >= 32 ? ~0ull : otb_low(Gs));
  const uint32_t nmsp = (wnmask >> sp0) & (Gs >= 32 ? 0xffffffffu : ((1u << Gs) - 1u));
  uint64_t m[B + 1];
  otb_vectors<B, DNA>(code, nmsp, g, even, m);
  const OtbBest r = otb_best(m, B, span, DNA ? nmsp : 0u, max_mm);
  OtbPair out;
  out.mm = r.mm; out.gaps = r.gaps; out.units = OT_TEXT_NA;
  if (r.mm > max_mm) return out;
  OtTextRec rec;
  rec.guide = 0; rec.row = 0; rec.q = 0; rec.nmask = wnmask; rec.code = wcode; rec.gaps = r.gaps;
  rec.strand = 0; rec.mm = (uint8_t)r.mm; rec.kind = DNA ? 1 : 2; rec.size = (uint8_t)B;
  OtTextFmt f;
  f.G = (uint32_t)G; f.P = (uint32_t)P; f.right = right ? 1u : 0u;
  for (int k = 0; k < 32; ++k) f.pam[k] = 'N';  // the nominal PAM is text only
  OtTextDiscard sink;
  out.units = ot_text_row(rec, g, nullptr, 0, 0, f, tab, sink);
  return out;
}

// the same with the bulge as arguments: b 1..2
OTB_HD OtbPair otb_pair(uint64_t wcode, uint32_t wnmask, uint64_t g, int G, int P, int right, int b, bool dna, int max_mm, const double* tab) {
  if (dna) return b == 1 ? otb_pair_t<1, true>(wcode, wnmask, g, G, P, right, max_mm, tab) : otb_pair_t<2, true>(wcode, wnmask, g, G, P, right, max_mm, tab);
  return b == 1 ? otb_pair_t<1, false>(wcode, wnmask, g, G, P, right, max_mm, tab) : otb_pair_t<2, false>(wcode, wnmask, g, G, P, right, max_mm, tab);
}
