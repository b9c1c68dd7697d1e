// hawk_gnomad.h - one data line of a gnomAD sites VCF -> its line of the population-genotype VCF, stated ONCE for the host
// (hawk_host_gnomad_lines, hawk_hostutil.hip) and the device (k_gn_scan / k_gn_text_len / k_gn_text_fill, hawk_gnomad.hip).
//
// What the reference does per record (converter.py of the reference: _convert 246-250, _asses_genotype 148-174,
// _format_vrecord 185-214), restated on the raw text:
//   keep rule   with keep off, a record whose FILTER, split at ';', has no token exactly PASS is dropped; nothing else of it is
//               examined (gn_filter_pass)
//   entries     INFO is `key=value` entries between ';'; an entry starts behind the tab that opens INFO or behind a ';'
//               (gn_entry_start); a key matches only at an entry start and only when '=' follows directly - or the entry ends
//               there, which is the key without a value (gn_key_at).  A key that occurs twice: the FIRST occurrence is read.
//               That is UNPINNED (pysam absent; htslib keeps one of them, which one is its business).
//   value       a comma list read left to right as any(ac > 0 ...) reads the tuple pysam would hand over: a count > 0 makes the
//               population observed and ENDS the reading; a '.' met before that is the reference's `None > 0` TypeError; an
//               entry that is no optionally signed run of 1..10 digits (empty included) is nothing htslib would hand over as an
//               integer.  Both are errors (gn_value).  So "3,." is observed and ".,3" an error; 0, 00 and -3 are not positive.
//   the line    CHROM POS ID REF ALT copied as they stand, QUAL and AF from the caller's strings (float32 text is made on the
//               host), FILTER copied except "." -> "" (";".join([]) is not None), "AF=", "GT", one 0/1 or 0/0 per key (gn_line).
//               With no AF entry: "0.0" once per ALT allele.
//
// The emitter writes through a sink (put(byte)), as hawk_ottext.h does: GnCount gives the length, GnBytes the bytes, so the
// length pass and the fill pass cannot drift apart.  No device code here: the header compiles as plain C++ too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif

#define GN_DROPPED 1u
#define GN_KEY_ABSENT 2u
#define GN_BAD_VALUE 4u
#define GN_FEW_FIELDS 8u
#define GN_ALT_MISSING 16u
#define GN_BAD_POS 32u

#define GN_MAX_KEYS 31      // user keys; slot 31 of the scan is the AF entry
#define GN_MAX_KEY_LEN 255
#define GN_MAX_KEY_BYTES 2048  // all keys together (they sit in LDS during the scan)
#define GN_ABSENT 0xffffffffu

// Host only: what both entry points check before anything is read: the keys, then that the offsets cut the text into whole lines
inline bool gn_args_ok(const uint8_t* text, uint64_t text_len, const uint64_t* line_off, uint64_t n_lines, const uint8_t* key_blob,
                       const uint64_t* key_off, uint32_t n_keys) {
  if (n_keys > GN_MAX_KEYS || !key_off || key_off[0] != 0) return false;
  for (uint32_t k = 0; k < n_keys; ++k) {
    if (key_off[k + 1] <= key_off[k] || key_off[k + 1] - key_off[k] > GN_MAX_KEY_LEN || !key_blob) return false;
    for (uint64_t b = key_off[k]; b < key_off[k + 1]; ++b)
      if (key_blob[b] == ';' || key_blob[b] == '=' || key_blob[b] == '\t') return false;
  }
  if (key_off[n_keys] > GN_MAX_KEY_BYTES) return false;
  if (text_len && (!text || text[text_len - 1] != '\n')) return false;
  if (!n_lines) return true;
  if (!text || !line_off) return false;
  for (uint64_t i = 0; i < n_lines; ++i) {
    const uint64_t a = line_off[i], b = line_off[i + 1];
    if (b > text_len || b <= a || b - a > 0xffffffffull || text[b - 1] != '\n') return false;
  }
  return true;
}

struct GnCount {
  uint64_t n = 0;
  HAWK_HD void put(uint8_t) { ++n; }
};
struct GnBytes {
  uint8_t* w;
  HAWK_HD void put(uint8_t c) { *w++ = c; }
};

// does an INFO entry start at a byte whose predecessor is `prev`?  (the caller knows the byte lies in INFO)
HAWK_HD inline bool gn_entry_start(uint8_t prev) { return prev == '\t' || prev == ';'; }

// does a byte end an INFO entry / the INFO field?
HAWK_HD inline bool gn_entry_end(uint8_t c) { return c == ';' || c == '\t'; }

// Key `key[0, klen)` at the entry start p of a record whose text ends at hi (its line end, '\r' and '\n' excluded):
//   0 not this key, 1 the key with '=' behind it (its value starts at p + klen + 1), 2 the key with the entry ending there
HAWK_HD inline int gn_key_at(const uint8_t* t, uint64_t p, uint64_t hi, const uint8_t* key, uint32_t klen) {
  if (p + klen > hi) return 0;
  for (uint32_t k = 0; k < klen; ++k)
    if (t[p + k] != key[k]) return 0;
  if (p + klen == hi) return 2;
  const uint8_t c = t[p + klen];
  return c == '=' ? 1 : (gn_entry_end(c) ? 2 : 0);
}

// The value that starts at v (ends at ';', a tab or hi): 0 no count above zero, 1 one found, 2 an error before one was found.
HAWK_HD inline int gn_value(const uint8_t* t, uint64_t v, uint64_t hi) {
  uint64_t p = v;
  for (;;) {
    // one comma entry [p, q)
    uint64_t q = p;
    while (q < hi && t[q] != ',' && !gn_entry_end(t[q])) ++q;
    if (q - p == 1 && t[p] == '.') return 2;  // None > 0
    uint64_t d = p;
    if (d < q && (t[d] == '-' || t[d] == '+')) ++d;
    const bool neg = d > p && t[p] == '-';
    const uint64_t nd = q - d;
    if (nd == 0 || nd > 10) return 2;
    bool nonzero = false;
    for (uint64_t k = d; k < q; ++k) {
      if (t[k] < '0' || t[k] > '9') return 2;
      nonzero |= t[k] != '0';
    }
    if (nonzero && !neg) return 1;
    if (q >= hi || t[q] != ',') return 0;
    p = q + 1;
  }
}

// FILTER = t[a, b): has it a ';'-token that is exactly PASS?
HAWK_HD inline bool gn_filter_pass(const uint8_t* t, uint64_t a, uint64_t b) {
  uint64_t p = a;
  for (;;) {
    uint64_t q = p;
    while (q < b && t[q] != ';') ++q;
    if (q - p == 4 && t[p] == 'P' && t[p + 1] == 'A' && t[p + 2] == 'S' && t[p + 3] == 'S') return true;
    if (q >= b) return false;
    p = q + 1;
  }
}

// POS = t[a, b): digits only, at least one
HAWK_HD inline bool gn_pos_ok(const uint8_t* t, uint64_t a, uint64_t b) {
  if (b <= a) return false;
  for (uint64_t k = a; k < b; ++k)
    if (t[k] < '0' || t[k] > '9') return false;
  return true;
}

// The flags of a record with at least eight fields from what the scan found (fo: its field offsets, len: its length without
// the line end): the keep rule first - a dropped record carries that flag alone -, then ALT ".", POS, and the keys' findings
// (absent / bad: any key absent, any value in error).
HAWK_HD inline uint32_t gn_record_flags(const uint8_t* rec, const uint32_t* fo, uint32_t keep, bool absent, bool bad) {
  if (!keep && !gn_filter_pass(rec, fo[6], fo[7] - 1u)) return GN_DROPPED;
  uint32_t fl = 0;
  if (fo[5] - 1u - fo[4] == 1u && rec[fo[4]] == '.') fl |= GN_ALT_MISSING;
  if (!gn_pos_ok(rec, fo[1], fo[2] - 1u)) fl |= GN_BAD_POS;
  if (absent) fl |= GN_KEY_ABSENT;
  if (bad) fl |= GN_BAD_VALUE;
  return fl;
}

// The spans of QUAL and of the AF value, as the per-record results carry them: {offset, length} relative to the record `rec` of
// `len` bytes (line end excluded).  af_pos: where the first entry with the key AF starts (GN_ABSENT: none); commas: those in ALT.
// Without an AF entry the length is GN_ABSENT and the first word the number of ALT alleles; "AF" without '=' is an empty value.
HAWK_HD inline void gn_spans(const uint8_t* rec, const uint32_t* fo, uint32_t len, bool full, uint32_t af_pos, uint32_t commas,
                             uint32_t* qual_span, uint32_t* af_span) {
  const uint32_t q0 = fo[5], q1 = full ? fo[6] - 1u : len;
  qual_span[0] = q0;
  qual_span[1] = q1 > q0 ? q1 - q0 : 0u;
  uint32_t a0 = commas + 1u, a1 = GN_ABSENT;
  if (full && af_pos != GN_ABSENT) {
    const uint8_t af[2] = {'A', 'F'};
    a0 = af_pos + 2u; a1 = 0;
    if (gn_key_at(rec, af_pos, len, af, 2) == 1) {
      a0 = af_pos + 3u;
      uint32_t q = a0;
      while (q < len && !gn_entry_end(rec[q])) ++q;
      a1 = q - a0;
    }
  }
  af_span[0] = a0;
  af_span[1] = a1;
}

// The output line of a record without flags.  rec: the record's first byte; fo: its eight field offsets; mask bit k: key k
// observed; qual / af: the caller's strings; af_present: the record has an AF entry (else "0.0" per ALT allele, n_alt of them).
template <class Sink>
HAWK_HD inline void gn_line(const uint8_t* rec, const uint32_t* fo, uint32_t mask, uint32_t n_keys, const uint8_t* qual, uint64_t qual_len,
                            const uint8_t* af, uint64_t af_len, bool af_present, uint32_t n_alt, Sink& s) {
  for (uint32_t k = fo[0]; k < fo[5]; ++k) s.put(rec[k]);  // CHROM POS ID REF ALT and the tab behind each
  for (uint64_t k = 0; k < qual_len; ++k) s.put(qual[k]);
  s.put('\t');
  const uint32_t f0 = fo[6], f1 = fo[7] - 1u;
  if (!(f1 - f0 == 1u && rec[f0] == '.'))
    for (uint32_t k = f0; k < f1; ++k) s.put(rec[k]);
  s.put('\t');
  s.put('A'); s.put('F'); s.put('=');
  if (af_present) {
    for (uint64_t k = 0; k < af_len; ++k) s.put(af[k]);
  } else {
    for (uint32_t a = 0; a < n_alt; ++a) {
      if (a) s.put(',');
      s.put('0'); s.put('.'); s.put('0');
    }
  }
  s.put('\t'); s.put('G'); s.put('T');
  for (uint32_t k = 0; k < n_keys; ++k) {
    s.put('\t'); s.put('0'); s.put('/'); s.put((mask >> k) & 1u ? '1' : '0');
  }
  s.put('\n');
}
