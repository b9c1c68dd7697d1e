// hawk_ottext.h - one off-target hit record -> the text of its row of offtargets_{contig}_{start}_{stop}.tsv, stated ONCE for
// the host (hawk_host_offtarget_text, hawk_hostutil.hip) and the device (k_ot_text_len / k_ot_text_fill, hawk_ottext.hip).
//
// The row is what this chain of the package prints for the hit (offtargets.py:41-53, 530-544 of the reference):
//   GenomeIndex._bulge_hit / hits_from_arrays -> crispritz_bulge_line / crispritz_report_line -> Offtarget.report_line
//   -> the _tsv_float columns of offtargets_table
// eleven fields joined by tabs, no newline:
//   chrom  position  strand  grna  spacer  pam  mm  bulge_size  bulg_type  cfd  elevation
// A record is {guide, row, q, strand, mm, code, nmask, gaps, kind 0 = X / 1 = DNA / 2 = RNA, size 0..2}: the columns of
// hawk_offtarget_scan / hawk_offtarget_bulges.  The window (code / nmask, guide orientation) has Gs + pamlen bases with
// Gs = G + size (DNA bulge), G - size (RNA bulge) or G; its PAM stands in front when `right` is set.
//
// The emitter writes through a sink (put(byte)): with OtTextCount it gives the row's length, with OtTextBytes the row - the
// length pass and the fill pass are the same function and cannot drift apart; with OtTextDiscard what is left is the row's CFD,
// which is how the bulged summary (otb_pair, hawk_otbulge.h) gets the table's units without restating them.  No device code here: the header compiles as
// plain C++ too (the host-only sanitizer builds of hawk_hostutil.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif

// round(x, 4) of Python as an integer number of 1e-4 units: the nearest integer to the EXACT product x * 1e4, exact ties to
// even (float_round -> dtoa mode 3 is correctly rounded on the binary value).  With k = floor(fl(x * 1e4)) the answer is k or
// k + 1, decided by the sign of x * 1e4 - (k + 0.5), which one fma gives exactly in sign (the difference of two doubles below
// 2^53 is far above the underflow range, so a non-zero exact residual never rounds to zero); zero is a true tie.
HAWK_HD inline long long ot_round_e4(double x) {
  const double k = __builtin_floor(x * 1e4);
  const double r = __builtin_fma(x, 1e4, -(k + 0.5));
  const long long ki = (long long)k;
  if (r > 0.0) return ki + 1;
  if (r < 0.0) return ki;
  return ki + (ki & 1);
}

struct OtTextRec {
  uint32_t guide, row, q, nmask;
  uint64_t code, gaps;
  uint8_t strand, mm, kind, size;
};

// what every row of a call shares
struct OtTextFmt {
  uint32_t G, P, right;  // guide length, PAM length, PAM in front
  uint8_t pam[32];       // the NOMINAL PAM's text (P bytes)
};

#define OT_TEXT_NA (-1)          // no tables: the cfd column is NA
#define OT_TEXT_UNSCORABLE (-2)  // an ambiguous base under a table lookup (k_cfd's error): NA, and the caller raises

struct OtTextCount {
  uint64_t n = 0;
  HAWK_HD void put(uint8_t) { ++n; }
};
struct OtTextBytes {
  uint8_t* w;
  HAWK_HD void put(uint8_t c) { *w++ = c; }
};
struct OtTextDiscard {  // the row's CFD alone (otb_pair, hawk_otbulge.h): the text goes nowhere
  HAWK_HD void put(uint8_t) {}
};

// the site's spacer length; 0 for a record no row can be made of
HAWK_HD inline uint32_t ot_text_gs(const OtTextFmt& f, uint32_t kind, uint32_t size) {
  if (kind == 1) return f.G + size;
  if (kind == 2) return f.G > size ? f.G - size : 0;
  return f.G;
}

// A record the emitter may be given: kind 0..2, size 0 for X and 1..2 for a bulge, the window within 32 bases, the bulge
// positions interior (1 .. span - 2 with span = Gs for DNA bulges, G for RNA bulges) and as many as `size`.
HAWK_HD inline bool ot_text_valid(const OtTextRec& r, const OtTextFmt& f) {
  if (r.kind > 2 || r.size > 2 || (r.kind == 0) != (r.size == 0)) return false;
  const uint32_t Gs = ot_text_gs(f, r.kind, r.size);
  if (Gs == 0 || Gs + f.P > 32 || f.G > 32) return false;
  if (r.kind == 0) return r.gaps == 0;
  const uint32_t span = r.kind == 1 ? Gs : f.G;
  if (span < 3) return false;
  const uint64_t interior = ((span >= 64 ? ~0ull : (1ull << (span - 1)) - 1ull)) & ~1ull;  // bits 1 .. span - 2
  if (r.gaps & ~interior) return false;
  return (uint32_t)__builtin_popcountll(r.gaps) == r.size;
}

// The hit columns of a call (n entries each) and the check both entry points make before anything is written: every record
// valid, every index a row follows inside its table.  Host only.
struct OtTextCols {
  const uint32_t *guide, *row, *q, *nmask;
  const uint64_t *code, *gaps;
  const uint8_t *strand, *mm, *kind, *size;
};
inline OtTextRec ot_text_rec(const OtTextCols& c, uint64_t i) {
  OtTextRec r;
  r.guide = c.guide[i]; r.row = c.row[i]; r.q = c.q[i]; r.nmask = c.nmask[i]; r.code = c.code[i]; r.gaps = c.gaps[i];
  r.strand = c.strand[i]; r.mm = c.mm[i]; r.kind = c.kind[i]; r.size = c.size[i];
  return r;
}
inline bool ot_text_check(uint64_t n, const OtTextCols& c, const OtTextFmt& f, uint32_t n_guides, const uint32_t* row_contig,
                          uint32_t n_table_rows, const uint8_t* name_blob, const uint64_t* name_off, uint32_t n_contigs,
                          const uint64_t* order) {
  if (!n) return true;
  if (!c.guide || !c.row || !c.q || !c.nmask || !c.code || !c.gaps || !c.strand || !c.mm || !c.kind || !c.size || !row_contig ||
      !name_off || !n_guides || !n_table_rows || !n_contigs)
    return false;
  for (uint64_t i = 0; i < n; ++i) {
    const OtTextRec r = ot_text_rec(c, i);
    if (!ot_text_valid(r, f) || r.guide >= n_guides || r.row >= n_table_rows) return false;
    if (order && order[i] >= n) return false;
  }
  for (uint32_t t = 0; t < n_table_rows; ++t)
    if (row_contig[t] >= n_contigs) return false;
  if (name_off[0] != 0) return false;
  for (uint32_t k = 0; k < n_contigs; ++k)
    if (name_off[k + 1] < name_off[k]) return false;
  return !(name_off[n_contigs] && !name_blob);
}

template <class Sink>
HAWK_HD inline void ot_text_dec(Sink& s, uint64_t v) {
  uint64_t div = 1;  // no digit buffer: nothing here may end in scratch memory
  while (v / div >= 10) div *= 10;
  for (; div; div /= 10) s.put((uint8_t)('0' + (int)((v / div) % 10)));
}

HAWK_HD inline uint8_t ot_text_letter(uint32_t code2) { return (uint8_t)(0x54474341u >> (8 * (code2 & 3u))); }  // "ACGT"

// index of a base letter in the CFD tables (A0 C1 G2 T3, any case), -1 for anything else
HAWK_HD inline int ot_text_base(uint8_t c) {
  switch (c & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

// The row of record `r` (valid: ot_text_valid) of guide code `gcode` (2 bits per base, A0 C1 G2 T3) at `pos` on the contig
// `name`.  tab = mm[20][4][4] ([alignment column][guide base][site base]) + pam[16], or NULL.  Returns the row's CFD rounded
// to 4 decimals in units of 1e-4, OT_TEXT_NA without tables, OT_TEXT_UNSCORABLE where compute_cfd would fail.
//
// The CFD is compute_cfd (cfdscore.py:53-95) as k_cfd states it on the strings the chain above hands it - wildtype = the grna
// field's spacer, sg = the spacer field's: a left-to-right fp64 product over the first min(columns, 20) ALIGNMENT columns,
// skipping those where the bases are equal or either side is '-', times the entry of the last two characters of the spacer
// field.  The table's position index is the alignment column: a DNA bulge moves the index of every later mismatch by one.
template <class Sink>
HAWK_HD inline long long ot_text_row(const OtTextRec& r, uint64_t gcode, const uint8_t* name, uint64_t name_len, uint64_t pos,
                                     const OtTextFmt& f, const double* tab, Sink& s) {
  const uint32_t G = f.G, P = f.P, Gs = ot_text_gs(f, r.kind, r.size);
  const uint32_t ncol = r.kind == 1 ? Gs : G;     // alignment columns
  const uint32_t sp0 = f.right ? P : 0;           // the site spacer's first base in the window
  const uint32_t pm0 = f.right ? 0 : Gs;          // the observed PAM's
  const bool dna = r.kind == 1, rna = r.kind == 2;
  for (uint64_t k = 0; k < name_len; ++k) s.put(name[k]);
  s.put('\t');
  ot_text_dec(s, pos);
  s.put('\t');
  s.put(r.strand ? '-' : '+');
  s.put('\t');
  // grna: the guide with '-' at the DNA-bulge columns, joined with the nominal PAM
  if (f.right) for (uint32_t k = 0; k < P; ++k) s.put(f.pam[k]);
  {
    uint32_t si = 0, gi = 0;
    for (uint32_t c = 0; c < ncol; ++c) {
      if (dna && ((r.gaps >> si) & 1)) { s.put('-'); ++si; continue; }
      s.put(ot_text_letter((uint32_t)((gcode >> (2 * gi)))));
      if (!(rna && ((r.gaps >> gi) & 1))) ++si;
      ++gi;
    }
  }
  if (!f.right) for (uint32_t k = 0; k < P; ++k) s.put(f.pam[k]);
  s.put('\t');
  // spacer: the site, mismatches in lower case, '-' at the RNA-bulge columns, joined with the OBSERVED PAM; the CFD's product
  // runs along the same columns.  c1 / c2: the last two characters written (the PAM table's key).
  double score = 1.0;
  bool bad = false;
  uint8_t c1 = 0, c2 = 0;
  if (f.right)
    for (uint32_t k = 0; k < P; ++k) {
      const uint8_t ch = (r.nmask >> (pm0 + k)) & 1 ? 'N' : ot_text_letter((uint32_t)((r.code >> (2 * (pm0 + k)))));
      s.put(ch); c1 = c2; c2 = ch;
    }
  {
    uint32_t si = 0, gi = 0;
    for (uint32_t c = 0; c < ncol; ++c) {
      uint8_t ch;
      if (rna && ((r.gaps >> gi) & 1)) {
        ch = '-'; ++gi;
      } else {
        const uint32_t w = sp0 + si;
        const bool amb = (r.nmask >> w) & 1;
        const uint32_t sb = (uint32_t)(r.code >> (2 * w)) & 3u;
        ch = amb ? 'N' : ot_text_letter(sb);
        if (dna && ((r.gaps >> si) & 1)) {
          ++si;  // a bulged base faces no guide base: printed as it is
        } else {
          const uint32_t gb = (uint32_t)(gcode >> (2 * gi)) & 3u;
          if (amb || sb != gb) {
            ch |= 0x20;
            if (tab && c < 20) {
              if (amb) bad = true; else score *= tab[(c * 4 + gb) * 4 + sb];
            }
          }
          ++si; ++gi;
        }
      }
      s.put(ch); c1 = c2; c2 = ch;
    }
  }
  if (!f.right)
    for (uint32_t k = 0; k < P; ++k) {
      const uint8_t ch = (r.nmask >> (pm0 + k)) & 1 ? 'N' : ot_text_letter((uint32_t)((r.code >> (2 * (pm0 + k)))));
      s.put(ch); c1 = c2; c2 = ch;
    }
  s.put('\t');
  for (uint32_t k = 0; k < P; ++k) s.put(f.pam[k]);
  s.put('\t');
  ot_text_dec(s, r.mm);
  s.put('\t');
  ot_text_dec(s, r.size);
  s.put('\t');
  if (dna) { s.put('D'); s.put('N'); s.put('A'); } else if (rna) { s.put('R'); s.put('N'); s.put('A'); } else s.put('X');
  s.put('\t');
  long long units = OT_TEXT_NA;
  if (tab) {
    const int p0 = ot_text_base(c1), p1 = ot_text_base(c2);
    if (bad || p0 < 0 || p1 < 0) units = OT_TEXT_UNSCORABLE;
    else units = ot_round_e4(score * tab[320 + 4 * p0 + p1]);
  }
  if (units < 0) {
    s.put('N'); s.put('A');
  } else {
    // repr(float(str(round(x, 4)))): the integer part, '.', up to four decimals without trailing zeros, at least one
    uint32_t fr = (uint32_t)(units % 10000);
    ot_text_dec(s, (uint64_t)(units / 10000));
    s.put('.');
    int nd = 4;
    while (nd > 1 && fr % 10 == 0) { fr /= 10; --nd; }
    uint32_t div = 1;
    for (int k = 1; k < nd; ++k) div *= 10;
    for (; div; div /= 10) s.put((uint8_t)('0' + (fr / div) % 10));
  }
  s.put('\t');
  s.put('N'); s.put('A');
  return units;
}
