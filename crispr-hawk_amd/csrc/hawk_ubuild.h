// hawk_ubuild.h - the whole-region rows of an unphased VCF (haplotypes.py:370-712 of the reference, add_variants_unphased for the
// SNV set): which genotype carries which allele, what a carried SNV does to REF's plane bits, and the signature rows are grouped
// on before any plane is written - stated ONCE for the host (hawk_host_unphased_rows, hawk_hostutil.hip) and the device
// (k_gt_parse_unphased, k_ub_sig, k_ub_rows: hawk_ubuild.hip).
//
//   genotype   g = a sample column up to its first ':'.  Well formed: exactly two '/'-separated parts and no '|', each part '.' or
//              all ASCII digits.  codes: part 0 -> column 2s, part 1 -> column 2s + 1; 0 REF, k = k-th ALT, 255 for '.', allele
//              numbers clamp at 254.  Flags: 1 = not exactly two '/'-parts or a '|' in g (haploid, three parts, phased, empty);
//              4 = one of the first two '/'-parts is neither '.' nor all digits (its code stays 255).
//   carrier    a sample carries allele k of a record iff one of its two codes is k (_genotypes_to_samples(phased=False), slot 0:
//              0/1, 1/0, 1/1, ./1 and 1/2 carry allele 1; 1/2 carries allele 2 as well).
//   site       at a position where a sample carries SNVs the A/C/G/T bits are REF's OR-ed with every carried alt's and the V
//              (lower-case) bit is set: IUPAC_ENCODER[IUPACTABLE[refnt] U alt] applied record after record, whatever the order
//              (OR is idempotent and commutative).  REF must hold exactly the record's ref base there, upper case: else the
//              builder declines.
//   signature  128 bits over the merged (position, bits) sites of a sample: a sum of per-site hashes (sites have distinct
//              positions, so the sum is a hash of the set) - rows with different signatures differ, rows with equal ones are
//              compared exactly by the caller.
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

#define UB_PLANES 5
#define UB_MISSING 255u
#define UB_CLAMP 254u
#define UB_MAX_ENTRIES 0xffffffffull
// why the builder declines (hawk.h: HAWK_UBUILD_*)
#define UB_DECL_NONE 0
#define UB_DECL_GENOTYPE 1    // a record flag of the unphased parse (1, 2 or 4)
#define UB_DECL_MNV 2         // an equal-length allele longer than one base
#define UB_DECL_BASE 3        // an alt or ref base outside A/C/G/T
#define UB_DECL_REF 4         // REF does not hold exactly the record's ref base at a site
#define UB_DECL_OUTSIDE 5     // an SNV outside the region
#define UB_DECL_ENTRIES 6     // more than 2^32 - 1 list entries
#define UB_DECL_REPEAT 7      // a sample carries an alt twice at one position: the host builder's encoder fails there

// One genotype column text[s, hi) (ends at a tab, a ':' or hi): flags | code0 << 8 | code1 << 16.
HAWK_HD inline uint32_t ub_gt_classify(const uint8_t* text, uint64_t s, uint64_t hi) {
  uint64_t e = s;
  uint32_t nbar = 0, nslash = 0;
  for (; e < hi && text[e] != '\t' && text[e] != ':'; ++e) {
    nbar += text[e] == '|';
    nslash += text[e] == '/';
  }
  uint32_t fl = (nslash == 1u && nbar == 0u) ? 0u : 1u, v[2] = {UB_MISSING, UB_MISSING};
  uint64_t p = s;
  for (uint32_t c = 0; c < 2u && c <= nslash; ++c) {
    uint64_t q = p;
    while (q < e && text[q] != '/') ++q;
    if (!(q - p == 1 && text[p] == '.')) {
      bool num = q > p;
      uint32_t x = 0;
      for (uint64_t t = p; t < q; ++t) {
        const uint8_t ch = text[t];
        if (ch < '0' || ch > '9') { num = false; break; }
        x = x * 10u + (uint32_t)(ch - '0');
        if (x > UB_CLAMP) x = UB_CLAMP;
      }
      if (num) v[c] = x; else fl |= 4u;
    }
    p = q + 1;
  }
  return fl | v[0] << 8 | v[1] << 16;
}

HAWK_HD inline bool ub_carried(uint32_t code0, uint32_t code1, uint32_t allele) { return code0 == allele || code1 == allele; }

// index 0-3 of an upper-case A C G T, else 255
HAWK_HD inline uint32_t ub_base_index(uint8_t ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 255u; }

// One carried SNV on bit `bit` of the five words of a row: ref5 = REF's words (never the row's own: two alleles at one position
// both see REF), row5 = the words being built.  false: REF does not hold exactly base `refbase` (0-3), upper case, there.
HAWK_HD inline bool ub_apply(const uint32_t* ref5, uint32_t* row5, uint32_t bit, uint32_t alt_mask, uint32_t refbase) {
  const uint32_t nib = ((ref5[0] >> bit) & 1u) | (((ref5[1] >> bit) & 1u) << 1) | (((ref5[2] >> bit) & 1u) << 2) | (((ref5[3] >> bit) & 1u) << 3);
  if (nib != (1u << refbase) || ((ref5[4] >> bit) & 1u)) return false;
  for (uint32_t pl = 0; pl < 4; ++pl) row5[pl] |= ((alt_mask >> pl) & 1u) << bit;
  row5[4] |= 1u << bit;
  return true;
}

// One more carried alt at a site whose bits so far are *acc (REF's bit to begin with), in list order.  false: the alt is among
// them already - a record the sample carries twice, or alt == ref behind another allele - where the host builder's sequential
// IUPAC_ENCODER look-up fails ("ACC" is no key); alt == ref as the site's first allele passes there and here.
HAWK_HD inline bool ub_site_add(uint32_t refbit, uint32_t* acc, uint32_t alt_mask) {
  if ((alt_mask & *acc) && !(*acc == refbit && alt_mask == refbit)) return false;
  *acc |= alt_mask;
  return true;
}

HAWK_HD inline uint64_t ub_mix(uint64_t x) {  // splitmix64's finaliser
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
// One merged site (its offset in the region, REF's bit OR-ed with the carried alts' bits) added to a signature.
HAWK_HD inline void ub_sig_add(uint32_t pos, uint32_t bits, uint64_t* s0, uint64_t* s1) {
  const uint64_t k = ((uint64_t)pos << 4) | (bits & 15u);
  *s0 += ub_mix(k);
  *s1 += ub_mix(k ^ 0xa5a5a5a5a5a5a5a5ull);
}
