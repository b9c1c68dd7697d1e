// hawk_otbulge.h - the placement selection of a bulged (site, guide) pair, shared by k_ot_bulge (hawk_otbulge.hip) and by the host
// program that checks it against a plain walk over the placements (otbulge_check_main.cpp; plain C++: no device types).
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

#ifdef __HIPCC__
#define OTB_HD __host__ __device__ __forceinline__
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
