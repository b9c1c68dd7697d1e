// hawk_otvar.h - one genome window of a variant-enriched index resolved against one guide, stated ONCE for the device
// (k_ov_match, hawk_otvar.hip) and the host (hawk_host_offtarget_variant_scan, hawk_hostutil.hip; otvar_check_main.cpp).
//
// The index holds, per position, an ALLELE SET = {REF base} + {ALT bases of the SNVs added at it}; a position whose REF base is
// ambiguous (N / IUPAC) holds the empty set and stays ambiguous.  Genotypes and phasing are not consulted: every allele is taken
// to exist in somebody, and every combination of alleles inside a window to exist on one chromosome - the enriched-genome
// semantics of CRISPRitz add-variants, an UPPER BOUND on the sites a population carries.
//
// A window of G + P bases in guide orientation (strand - reverse-complemented) is resolved position by position:
//   PAM position     satisfied iff allele set and the PAM's IUPAC set intersect; a PAM 'N' is satisfied by any position, an
//                    ambiguous one included, as in the plain scan.  Resolved base: REF's if REF is in the PAM's set, else the
//                    lowest allele (A < C < G < T, guide orientation) of the intersection.
//   spacer position  resolved base: the guide's if it is in the allele set, else REF's - a mismatch.  An ambiguous position is
//                    a mismatch, as in the plain scan.
//   mm  = mismatches of the resolved spacer;  alt = bit i set where the resolved base differs from REF's.
// A variant row exists iff every PAM position is satisfied, mm <= max_mm and alt != 0 (alt == 0 is the plain scan's row).
// Plain C++: no device types.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif

struct OvGeom {
  uint64_t pam_fwd;      // the PAM as the guide reads it: first base in the most significant of its P nibbles (A1 C2 G4 T8)
  int32_t G, P, right;   // spacer bases, PAM bases, PAM in front of the spacer
};
struct OvResolved {
  uint64_t code;  // the resolved window, base i at bits 2i, 2i + 1 (A0 C1 G2 T3); an ambiguous position keeps REF's code bits
  uint32_t alt;   // bit i: the resolved base is not REF's
  int32_t mm;     // mismatches of the resolved spacer
  int32_t ok;     // every PAM position is satisfied
};

// rcode / nmask: REF's window (2-bit code, ambiguity mask); am[b] bit i: base b is in the allele set of window position i;
// gcode: the guide's spacer, base j at bits 2j, 2j + 1.
HAWK_HD inline __attribute__((always_inline)) OvResolved ov_resolve(uint64_t rcode, uint32_t nmask, const uint32_t (&am)[4], uint64_t gcode, const OvGeom g) {
  OvResolved r;
  r.code = rcode; r.alt = 0; r.mm = 0; r.ok = 1;
  const int sp0 = g.right ? g.P : 0, pam0 = g.right ? 0 : g.G;
  const uint32_t a0 = am[0], a1 = am[1], a2 = am[2], a3 = am[3];
  for (int k = 0; k < g.P; ++k) {
    const int i = pam0 + k;
    const uint32_t nib = (uint32_t)(g.pam_fwd >> (4 * (g.P - 1 - k))) & 15u;
    if (nib == 15u) continue;  // any position, REF stays
    const uint32_t set = ((a0 >> i) & 1u) | (((a1 >> i) & 1u) << 1) | (((a2 >> i) & 1u) << 2) | (((a3 >> i) & 1u) << 3);
    const uint32_t both = set & nib;
    if (!both) { r.ok = 0; continue; }
    const uint32_t rb = (uint32_t)(rcode >> (2 * i)) & 3u;
    if (!((nmask >> i) & 1u) && ((nib >> rb) & 1u)) continue;  // REF is in the PAM's set
    uint32_t b = 0;
    while (!((both >> b) & 1u)) ++b;
    r.code = (r.code & ~(3ull << (2 * i))) | ((uint64_t)b << (2 * i));
    r.alt |= 1u << i;
  }
  for (int j = 0; j < g.G; ++j) {
    const int i = sp0 + j;
    const uint32_t gb = (uint32_t)(gcode >> (2 * j)) & 3u, rb = (uint32_t)(rcode >> (2 * i)) & 3u;
    // the position's allele set as a nibble, shifted by the guide's base: no register array indexed by a lane's value
    const uint32_t set = ((a0 >> i) & 1u) | (((a1 >> i) & 1u) << 1) | (((a2 >> i) & 1u) << 2) | (((a3 >> i) & 1u) << 3);
    if (((nmask >> i) & 1u) || !((set >> gb) & 1u)) { ++r.mm; continue; }
    if (gb != rb) {
      r.code = (r.code & ~(3ull << (2 * i))) | ((uint64_t)gb << (2 * i));
      r.alt |= 1u << i;
    }
  }
  return r;
}

// bit i of the result: window position i holds an allele that is not REF's
HAWK_HD inline uint32_t ov_alt_positions(uint64_t rcode, uint32_t nmask, const uint32_t (&am)[4], int L) {
  uint32_t out = 0;
  for (int i = 0; i < L; ++i) {
    const uint32_t rb = (uint32_t)(rcode >> (2 * i)) & 3u;
    for (uint32_t b = 0; b < 4; ++b)
      if (((am[b] >> i) & 1u) && (((nmask >> i) & 1u) || b != rb)) out |= 1u << i;
  }
  return out;
}

// statuses of one entry of hawk_genome_variants / of the host twin's variant list
#define HAWK_OV_APPLIED 0
#define HAWK_OV_REF_N 1         // the index holds N or another non-ACGT base at the position
#define HAWK_OV_REF_MISMATCH 2  // the stated REF base is not the index's
#define HAWK_OV_ALT_IS_REF 3
