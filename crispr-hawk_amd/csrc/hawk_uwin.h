// hawk_uwin.h - the indel-window rows of an unphased VCF (haplotypes.unphased_indel_windows over Haplotype.add_variants_unphased:
// per indel allele inside the region and per carrier, the region cut to 100 nt either side of the indel, with the indel and the
// carrier's SNVs inside that window) - stated ONCE for the host (hawk_host_unphased_windows, hawk_hostutil.hip) and the device
// (k_uw_instances, k_uw_sig, k_uw_group, k_uw_fill: hawk_uwin.hip).
//
//   indel      one ALT allele of unequal length after adjust_multiallelic: o = its offset in the region (of L bases), a deletion has
//              a one-base alt and a ref of span = |grow| + 1 bases, an insertion a one-base ref (span 1) and grow + 1 alt bases.
//   geometry   the window is region offsets a = max(0, o - 100) .. b = min(L - 1, o - grow + 100); wlen = b - a + 1; the finished
//              row is rowlen = wlen + grow long; i = o - a is the anchor's place in it.  An unclamped window gives rowlen 201.
//   sites      a carrier's merged SNV sites (hawk_ubuild.h) with offset in [a, b].  A site is APPLIED iff off - a < rowlen (the
//              position map is sized for the finished row: an SNV in the last |grow| bases of a deletion window is listed in the
//              labels and never written).  An applied site at the anchor or inside a deletion's span is written and then overwritten
//              by the indel; every other applied site SURVIVES, at row position off - a before the anchor, off - a + grow behind.
//   row        source [a, o) | the alt, every base lower case (V bit) | source [o + span, b], with the surviving sites OR-ed in.
//   ref check  every ref base of the indel must be among the letters the row holds at [o, o + span) before the indel goes in:
//              REF's base where no applied site lies (exactly: A/C/G/T, upper case), the site's bits where one does.
//   signature  ub_sig_add over the SURVIVING sites (region offset, bits): two carriers of one indel have equal rows iff those sets
//              are equal - the signature proposes, the caller compares the sets exactly.
// No device code and no state here: the header compiles as plain C++ too.
#pragma once
#include "hawk_ubuild.h"

#define UW_FLANK 100u
#define UB_DECL_WINDOW 8      // hawk.h: HAWK_UBUILD_WINDOW - the indel does not fit the window the host builder cuts
#define UB_DECL_INDEL_BASE 9  // hawk.h: HAWK_UBUILD_INDEL_BASE - a base of the indel's ref or alt outside A/C/G/T

struct UwGeom {
  uint32_t o, a, b, wlen, rowlen, i, span, alt_len;
  int32_t grow;
};

// The window of an indel at offset o (< L) with ref_len / alt_len bases; UB_DECL_NONE, or why the builder declines it.
HAWK_HD inline int uw_geometry(uint32_t o, uint32_t ref_len, uint32_t alt_len, uint32_t L, UwGeom* g) {
  if (!ref_len || !alt_len || ref_len == alt_len || o >= L) return UB_DECL_WINDOW;
  const int64_t grow = (int64_t)alt_len - (int64_t)ref_len;
  const uint32_t span = grow > 0 ? 1u : (uint32_t)(-grow) + 1u;
  if (ref_len != span) return UB_DECL_REF;  // a ref the builder's length comparison never matches (an alt of a deletion longer than one base)
  if (grow > (int64_t)UW_FLANK) return UB_DECL_WINDOW;
  const int64_t a = o > UW_FLANK ? (int64_t)o - UW_FLANK : 0;
  int64_t b = (int64_t)o - grow + UW_FLANK;
  if (b > (int64_t)L - 1) b = (int64_t)L - 1;
  if ((int64_t)o > b) return UB_DECL_WINDOW;
  const int64_t wlen = b - a + 1, rowlen = wlen + grow, i = (int64_t)o - a;
  if (rowlen <= 0 || i >= rowlen || i + span > wlen) return UB_DECL_WINDOW;  // the position map skips the indel / it runs past the window
  g->o = o; g->a = (uint32_t)a; g->b = (uint32_t)b; g->wlen = (uint32_t)wlen; g->rowlen = (uint32_t)rowlen; g->i = (uint32_t)i;
  g->span = span; g->alt_len = alt_len; g->grow = (int32_t)grow;
  return UB_DECL_NONE;
}

#define UW_SKIPPED 0u    // listed in the labels, never written
#define UW_COVERED 1u    // written, then overwritten by the indel: in the labels, and at the anchor in the allele table
#define UW_SURVIVES 2u
HAWK_HD inline uint32_t uw_site_state(const UwGeom& g, uint32_t off) {  // off in [g.a, g.b]
  if (off - g.a >= g.rowlen) return UW_SKIPPED;
  return (off >= g.o && off < g.o + g.span) ? UW_COVERED : UW_SURVIVES;
}
// the row position of a surviving site (and the allele-table key of the anchor's: off == o maps to i)
HAWK_HD inline uint32_t uw_site_pos(const UwGeom& g, uint32_t off) { return off <= g.o ? off - g.a : (uint32_t)((int64_t)(off - g.a) + g.grow); }

// Where row position p (< rowlen) comes from: a region offset (>= 0), or -(1 + k) for base k of the alt.
HAWK_HD inline int64_t uw_source(const UwGeom& g, uint32_t p) {
  if (p < g.i) return (int64_t)g.a + p;
  if (p < g.i + g.alt_len) return -(int64_t)(1u + (p - g.i));
  return (int64_t)g.a + p - g.grow;
}

// One ref base (0-3) of the indel against what the row holds there: REF's byte, and the bits of the applied site at that
// position (0: none).
HAWK_HD inline bool uw_ref_ok(uint8_t ref_byte, uint32_t site_bits, uint32_t base) {
  if (site_bits) return (site_bits >> base) & 1u;
  return ub_base_index(ref_byte) == base;
}

// ---- a carrier's entries [e, hi) of the ascending per-sample lists (hawk_ubuild_lists), walked site by site
struct UwLists {
  const uint32_t* idx;      // the lists' entries: variant indices
  const uint32_t* var_off;  // [n_var] offset in the region, ascending
  const uint8_t* var_mask;  // [n_var] the alt's 4-bit mask
  const uint8_t* var_ref;   // [n_var] the ref base 0-3
};
// The merged site that opens at entry *e: its offset and bits (every entry's ref bit and alt, as k_ub_sig merges them); *e moves
// behind it.  false: no entry left.
HAWK_HD inline bool uw_next_site(const UwLists& l, uint64_t* e, uint64_t hi, uint32_t* off, uint32_t* bits) {
  if (*e >= hi) return false;
  const uint32_t pos = l.var_off[l.idx[*e]];
  uint32_t acc = 0;
  for (; *e < hi && l.var_off[l.idx[*e]] == pos; ++*e) acc |= (uint32_t)l.var_mask[l.idx[*e]] | (1u << l.var_ref[l.idx[*e]]);
  *off = pos; *bits = acc;
  return true;
}
HAWK_HD inline bool uw_next_surviving(const UwLists& l, const UwGeom& g, uint64_t* e, uint64_t hi, uint32_t* off, uint32_t* bits) {
  while (uw_next_site(l, e, hi, off, bits))
    if (uw_site_state(g, *off) == UW_SURVIVES) return true;
  return false;
}
// The first entry of [lo, hi) whose offset is at least `off`.
HAWK_HD inline uint64_t uw_lower_bound(const UwLists& l, uint64_t lo, uint64_t hi, uint32_t off) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (l.var_off[l.idx[mid]] < off) lo = mid + 1; else hi = mid;
  }
  return lo;
}
HAWK_HD inline void uw_signature(const UwLists& l, const UwGeom& g, uint64_t lo, uint64_t hi, uint64_t* s0, uint64_t* s1) {
  uint32_t off, bits;
  *s0 = *s1 = 0;
  while (uw_next_surviving(l, g, &lo, hi, &off, &bits)) ub_sig_add(off, bits, s0, s1);
}
// Two carriers of ONE indel give the same row: their surviving sites are equal, one by one.
HAWK_HD inline bool uw_same_row(const UwLists& l, const UwGeom& g, uint64_t lo_a, uint64_t hi_a, uint64_t lo_b, uint64_t hi_b) {
  uint32_t off_a, bits_a, off_b, bits_b;
  for (;;) {
    const bool more_a = uw_next_surviving(l, g, &lo_a, hi_a, &off_a, &bits_a), more_b = uw_next_surviving(l, g, &lo_b, hi_b, &off_b, &bits_b);
    if (!more_a || !more_b) return more_a == more_b;
    if (off_a != off_b || bits_a != bits_b) return false;
  }
}
// The indel's ref (ref_base[span], 0-3 each) against what a carrier's row holds at [o, o + span): UB_DECL_NONE or UB_DECL_REF.
HAWK_HD inline int uw_check_ref(const UwLists& l, const UwGeom& g, uint64_t lo, uint64_t hi, const uint8_t* ref /* REF's bytes */,
                                const uint8_t* ref_base) {
  for (uint32_t t = 0; t < g.span; ++t) {
    if (ub_base_index(ref[g.o + t]) == ref_base[t]) continue;  // (an applied site there holds REF's bit too)
    uint64_t e = uw_lower_bound(l, lo, hi, g.o + t);
    uint32_t off = 0, bits = 0;
    const bool site = uw_next_site(l, &e, hi, &off, &bits) && off == g.o + t && uw_site_state(g, off) != UW_SKIPPED;
    if (!uw_ref_ok(ref[g.o + t], site ? bits : 0u, ref_base[t])) return UB_DECL_REF;
  }
  return UB_DECL_NONE;
}
// every base of the indel's ref and alt is 0-3 (pool holds ub_base_index of the ref's bases, then of the alt's)
HAWK_HD inline bool uw_bases_ok(const uint8_t* pool, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (pool[k] > 3u) return false;
  return true;
}
