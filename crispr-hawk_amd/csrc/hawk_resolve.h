// hawk_resolve.h - what an IUPAC-encoded window of an unphased haplotype resolves to (search_guides.py:163-257, 340-369, 463-480):
// the options of one window position, a row's counts, the j-th kept combination as five window-slice words and the compare against
// the REF guide's core - stated ONCE for the host (hawk_host_resolve_unphased, hawk_hostutil.hip) and the device (k_ur_count /
// k_ur_fill, hawk_resolve.hip).
//
//   row        (hap, pos, strand, win[5], flags) of the guide table; W = guidelen + pamlen + 20; r = right XOR strand; window base
//              0 is haplotype position p0 = pos - 10 (r) or pos - guidelen - 10.
//   valid      is_pamhit_valid: pos + guidelen + pamlen + 10 < hap_len (r; STRICT: a window that ends with the haplotype is in
//              the table and yields nothing) or pos - guidelen - 10 >= 0.  An invalid row yields nothing and is never looked at.
//   options    a position with one base (popcount of its A/C/G/T mask == 1) has one option: itself, case kept.  With several, the
//              allele entries of (hap, p0 + i) - k (ref, alt, pos) tuples - give popcount * k options: the set bases in A, C, G,
//              T order, each once per entry, upper case when the base is that entry's ref and lower case otherwise (an entry
//              whose ref is not one base: UR_NO_SINGLE, always lower).  No entries for the position: the call declines.
//   PAM        the PAM slice sits at window offsets [idx, idx + pamlen), idx = 10 (r) or W - 10 - pamlen; pattern nibble t is
//              taken from pam.bits (strand 0) or pam.bitsrc (strand 1), first base in the most significant nibble; an option
//              passes when the nibble is 0 or holds its base.  The test reads one position at a time, so it THINS THE OPTION
//              LIST of a PAM position (the bases outside the nibble go, the order stays) and the kept combinations are the plain
//              mixed-radix product of the thinned lists, leftmost position slowest (itertools.product): n_resolved = left * Vp *
//              right, the j-th survivor is digit-decoded from j.  Nothing is enumerated to be discarded.
//   redundant  a combination of a non-REF row whose (start, strand) a REF guide shares and whose upper-cased core (offsets [10,
//              W - 10)) is the REF guide's: those are exactly the combinations that pick an option with REF's base at every core
//              position (any option in the pads), n_drop = product of those option counts.  ur_unrank walks the positions left to
//              right and skips that sub-product while the prefix still agrees with REF, so the kept ones come out in enumeration
//              order without a scan.
// Counts are 64-bit and saturate (UR_SAT); a row above UR_MAX_ROW combinations declines.  No device code and no state here: the
// header compiles as plain C++ too.
#pragma once
#include <stdint.h>

#ifndef HAWK_HD
#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif
#endif

#define UR_PAD 10
#define UR_PLANES 5
#define UR_NO_SINGLE 255
#define UR_SAT 0xffffffffffffffffull
#define UR_MAX_ROW 0xffffffffull
#define UR_OUT_BYTES 44ull  // one kept guide: src_row + five window slices
// why a call declines (hawk.h: HAWK_RESOLVE_*)
#define UR_DECL_NONE 0
#define UR_DECL_NO_ENTRY 1   // an ambiguous position without allele entries (the reference's KeyError)
#define UR_DECL_MULTI_REF 2  // more than one haplotype flagged REF
#define UR_DECL_REF_AMBIG 3  // a REF row with more than one combination (the reference's "Duplicate REF guide")
#define UR_DECL_ROW_SIZE 4   // a row above 2^32 - 1 combinations
#define UR_DECL_BATCH 5      // a row whose kept guides do not fit the batch budget

struct UrAlleles {
  const uint64_t* key;  // [n_keys] sorted hap << 32 | rel
  const uint32_t* off;  // [n_keys + 1] CSR into ref
  const uint8_t* ref;   // per entry: its ref base 0-3 (A C G T), or UR_NO_SINGLE
  uint64_t n_keys;
};
struct UrGeom {
  uint64_t pam_fwd, pam_rev;
  int32_t guidelen, pamlen, right, W;
};
struct UrRow {
  uint32_t hap, pos, strand, flags, hap_len;
  uint64_t win[UR_PLANES];
};
// one window position after the PAM thinning: its options are the set bases of `mask` in A, C, G, T order, k times each
struct UrPos {
  uint32_t mask, k, e0, amb, lower;
};

HAWK_HD inline uint64_t ur_mul_sat(uint64_t a, uint64_t b) {
  unsigned long long r;
  if (a == UR_SAT || b == UR_SAT) return (a == 0 || b == 0) ? 0 : UR_SAT;
  return __builtin_mul_overflow((unsigned long long)a, (unsigned long long)b, &r) ? UR_SAT : (uint64_t)r;
}
HAWK_HD inline uint32_t ur_popc4(uint32_t m) { return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u); }
HAWK_HD inline bool ur_row_r(const UrRow& row, const UrGeom& g) { return (g.right != 0) != (row.strand != 0); }
HAWK_HD inline int64_t ur_row_p0(const UrRow& row, const UrGeom& g) {
  return ur_row_r(row, g) ? (int64_t)row.pos - UR_PAD : (int64_t)row.pos - g.guidelen - UR_PAD;
}
HAWK_HD inline bool ur_row_valid(const UrRow& row, const UrGeom& g) {
  if (ur_row_r(row, g)) return (int64_t)row.pos + g.guidelen + g.pamlen + UR_PAD < (int64_t)row.hap_len;
  return (int64_t)row.pos - g.guidelen - UR_PAD >= 0;
}
HAWK_HD inline int ur_pam_idx(const UrRow& row, const UrGeom& g) { return ur_row_r(row, g) ? UR_PAD : g.W - UR_PAD - g.pamlen; }
HAWK_HD inline uint32_t ur_mask_at(const uint64_t* win, int i) {
  return (uint32_t)((win[0] >> i) & 1u) | ((uint32_t)((win[1] >> i) & 1u) << 1) | ((uint32_t)((win[2] >> i) & 1u) << 2) |
         ((uint32_t)((win[3] >> i) & 1u) << 3);
}
// index of (hap, rel) in the allele table, or -1
HAWK_HD inline int64_t ur_find(const UrAlleles& al, uint32_t hap, int64_t rel) {
  if (rel < 0 || rel > 0xffffffffll) return -1;
  const uint64_t want = ((uint64_t)hap << 32) | (uint64_t)rel;
  uint64_t lo = 0, hi = al.n_keys;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (al.key[mid] < want) lo = mid + 1; else hi = mid;
  }
  return (lo < al.n_keys && al.key[lo] == want) ? (int64_t)lo : -1;
}
// position i of the row's window; false: an ambiguous position without allele entries (or no base at all)
HAWK_HD inline bool ur_pos(const UrRow& row, const UrGeom& g, const UrAlleles& al, int i, UrPos* p) {
  const uint32_t m = ur_mask_at(row.win, i);
  const uint32_t pc = ur_popc4(m);
  p->mask = m; p->k = 1; p->e0 = 0; p->amb = 0; p->lower = (uint32_t)((row.win[4] >> i) & 1u);
  if (pc == 0) return false;
  if (pc > 1) {
    const int64_t j = ur_find(al, row.hap, ur_row_p0(row, g) + i);
    if (j < 0) return false;
    p->amb = 1; p->e0 = al.off[j]; p->k = al.off[j + 1] - al.off[j];
  }
  const int t = i - ur_pam_idx(row, g);
  if (t >= 0 && t < g.pamlen) {
    const uint32_t pn = (uint32_t)(((row.strand ? g.pam_rev : g.pam_fwd) >> (4 * (g.pamlen - 1 - t))) & 0xFu);
    if (pn) p->mask &= pn;
  }
  return true;
}
HAWK_HD inline uint32_t ur_radix(const UrPos& p) { return ur_popc4(p.mask) * p.k; }
// option o of a position (o < ur_radix): its base 0-3 and case
HAWK_HD inline void ur_option(const UrPos& p, const UrAlleles& al, uint32_t o, uint32_t* base, uint32_t* lower) {
  uint32_t nth = o / p.k, b = 0;
  for (; b < 4; ++b)
    if ((p.mask >> b) & 1u) { if (!nth) break; --nth; }
  *base = b;
  *lower = p.amb ? (al.ref[p.e0 + o % p.k] != b ? 1u : 0u) : p.lower;
}
HAWK_HD inline bool ur_is_pad(const UrGeom& g, int i) { return i < UR_PAD || i >= g.W - UR_PAD; }
// options of a position that the redundancy rule reads as "REF's": all of a pad, those with a base of refmask in the core
HAWK_HD inline uint32_t ur_agree(const UrPos& p, const UrGeom& g, int i, uint32_t refmask) {
  return ur_is_pad(g, i) ? ur_radix(p) : ur_popc4(p.mask & refmask) * p.k;
}

struct UrCounts {
  uint64_t left, vp, right, total;  // combinations left of the PAM slice, valid PAM combinations, right of it, their product
  uint64_t drop;                    // combinations whose core is REF's (0 without a REF guide)
};
// The counts of a row.  refwin: the four code planes of the REF guide's window at the same (start, strand), read when has_ref (a
// flag, not a null pointer: the device keeps the words in registers).  Returns
// UR_DECL_NONE or UR_DECL_NO_ENTRY; an invalid row counts 0 everywhere.
HAWK_HD inline int ur_counts(const UrRow& row, const UrGeom& g, const UrAlleles& al, const uint64_t* refwin, bool has_ref, UrCounts* c) {
  c->left = c->vp = c->right = 1; c->total = 0; c->drop = 0;
  if (!ur_row_valid(row, g)) { c->left = c->vp = c->right = 0; return UR_DECL_NONE; }
  const int idx = ur_pam_idx(row, g);
  uint64_t drop = has_ref ? 1 : 0;
  for (int i = 0; i < g.W; ++i) {
    UrPos p;
    if (!ur_pos(row, g, al, i, &p)) return UR_DECL_NO_ENTRY;
    const uint64_t rad = ur_radix(p);
    if (i < idx) c->left = ur_mul_sat(c->left, rad);
    else if (i < idx + g.pamlen) c->vp = ur_mul_sat(c->vp, rad);
    else c->right = ur_mul_sat(c->right, rad);
    if (has_ref) drop = ur_mul_sat(drop, ur_agree(p, g, i, ur_mask_at(refwin, i)));
  }
  c->total = ur_mul_sat(ur_mul_sat(c->left, c->vp), c->right);
  c->drop = drop < c->total ? drop : c->total;
  return UR_DECL_NONE;
}
// The jk-th kept combination of a row (jk < total - drop; total <= UR_MAX_ROW, so every suffix product fits 32 bits) as five
// window-slice words.  refwin / has_ref as in ur_counts (no REF guide, or drop == 0: nothing is skipped).
HAWK_HD inline void ur_unrank(const UrRow& row, const UrGeom& g, const UrAlleles& al, const uint64_t* refwin, bool has_ref, uint32_t total, uint32_t drop,
                              uint32_t jk, uint64_t* out) {
  uint64_t w[UR_PLANES] = {0, 0, 0, 0, 0};
  uint32_t T = total, M = drop;
  bool tight = has_ref && drop != 0;
  for (int i = 0; i < g.W; ++i) {
    UrPos p;
    (void)ur_pos(row, g, al, i, &p);
    const uint32_t rad = ur_radix(p);
    uint32_t o = 0;
    T = rad ? T / rad : 0;
    if (tight) {
      const uint32_t refmask = ur_mask_at(refwin, i);
      const bool pad = ur_is_pad(g, i);
      const uint32_t ag = ur_agree(p, g, i, refmask);
      M = ag ? M / ag : 0;
      for (o = 0; o + 1 < rad; ++o) {
        uint32_t b, lw;
        ur_option(p, al, o, &b, &lw);
        const uint32_t sub = T - ((pad || ((refmask >> b) & 1u)) ? M : 0u);
        if (jk < sub) break;
        jk -= sub;
      }
    } else if (T) {
      o = jk / T;
      jk -= o * T;
    }
    if (o >= rad) o = rad ? rad - 1 : 0;
    uint32_t b = 0, lw = p.lower;
    if (rad) ur_option(p, al, o, &b, &lw);
    if (tight && !ur_is_pad(g, i) && !((ur_mask_at(refwin, i) >> b) & 1u)) tight = false;
    for (uint32_t pl = 0; pl < 4; ++pl)  // (no indexing by b: the words stay in registers)
      if (b == pl) w[pl] |= 1ull << i;
    if (lw) w[4] |= 1ull << i;
  }
  for (int pl = 0; pl < UR_PLANES; ++pl) out[pl] = w[pl];
}
// upper-cased core of a window equal to REF's (remove_redundant_guides)
HAWK_HD inline bool ur_core_equal(const uint64_t* win, const uint64_t* refwin, const UrGeom& g) {
  const int L = g.W - 2 * UR_PAD;
  const uint64_t m = (L >= 64 ? ~0ull : ((1ull << L) - 1ull)) << UR_PAD;
  for (int pl = 0; pl < 4; ++pl)
    if ((win[pl] ^ refwin[pl]) & m) return false;
  return true;
}
// a well-formed allele table (host arrays): keys strictly ascending, offsets from 0 ascending, ref bytes 0-3 or UR_NO_SINGLE
inline bool ur_check_alleles(const UrAlleles& al) {
  if (!al.n_keys) return true;
  if (!al.key || !al.off || al.off[0] != 0) return false;
  for (uint64_t i = 0; i < al.n_keys; ++i)
    if ((i && al.key[i] <= al.key[i - 1]) || al.off[i + 1] < al.off[i]) return false;
  if (al.off[al.n_keys] && !al.ref) return false;
  for (uint32_t e = 0; e < al.off[al.n_keys]; ++e)
    if (al.ref[e] > 3 && al.ref[e] != UR_NO_SINGLE) return false;
  return true;
}
// geometry the kernels and the twin refuse alike: 0 fine, 1 invalid, 2 unsupported
HAWK_HD inline int ur_check_geom(const UrGeom& g) {
  if (g.guidelen < 1 || g.pamlen < 1 || g.pamlen > 16 || g.W != g.guidelen + g.pamlen + 2 * UR_PAD) return 1;
  if (g.W > 64) return 2;
  return 0;
}
