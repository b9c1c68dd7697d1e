// hawk_effects.h - what population variants do to a guide: score deltas against the REF guide of the same (start, strand), the
// worst delta per position, the ranking, guide types - stated ONCE for the host (hawk_host_effects, hawk_hostutil.hip) and the
// device (k_fx_* in hawk_effects.hip).  The data stage behind the reference's graphical_reports.py, on report groups.
//
//   score     the report prints round(score, 4) and the reference takes its deltas from the printed text: fx_round4 gives that
//             double from the unrounded score (k / 10^4 with k Python's correctly rounded, half-even choice on the exact binary
//             value).  NaN stays NaN.  Exact for |x| < 2^38; beyond that (no score gets there) x comes back unchanged.
//   position  groups of one (start, strand): contiguous in collapse order.  A position is named by the index of its first group
//             (its HEAD); per-position results sit at the head's index.
//   delta     with a REF group at the position (the first in report order, should there be several): score - ref_score for
//             every group of the position, REF included; without one: 0.0.  abs_delta = |delta|.
//   valid     alternatives the ranking looks at: signed family (score_cfdon) alt groups with score < ref_score (a NaN on either
//             side fails), absolute family (azimuth, rs3, deepcpf1) all alt groups.  Positions without REF are not ranked.
//   worst     no valid alternative: 0.0.  Signed: min(delta).  Absolute: Python's max() over abs_delta in report order, a left
//             fold with `>`: NaN iff the FIRST alternative's value is NaN, else the maximum of the non-NaN values - stated in
//             that closed form (FxWorst), which does not depend on the order the alternatives are met in.
//   ranking   signed ascending, absolute descending, NaN last.  The reference sorts with pandas' single-column sort_values,
//             which is not stable: inside a run of equal worst deltas ITS order is undefined.  OURS is the position's first
//             appearance in report order (fx_before) - the one order here that is this project's own.
//   type      0 ref; else 1 spacer and PAM hold a lower-case base, 2 spacer only, 3 PAM only, FX_TYPE_UNKNOWN neither; read from
//             the case plane of the window's core as the report shows it (strand 1 reverse-complemented, `right` swapping the
//             slices - only WHICH slice matters for the question).  A group counts once per (start, stop, strand, cased sgRNA,
//             cased pam): a later group in report order with the same text is a duplicate (collapse flanks can make those).
//
// No device code and no state here: the header compiles as plain C++ too.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HAWK_HD __host__ __device__
#else
#define HAWK_HD
#endif

// The doubles below are pinned bit for bit: no operation of fx_round4 or of a delta may be fused with a neighbour (the device
// compiler contracts a * b + c across statements by default, and folds a subtraction into the last step of a division).
#if defined(__clang__)
#define FX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FX_NO_CONTRACT
#endif

#define FX_PAD 10               // HAWK_PAD: the window slice is [core - 10, core + L + 10)
#define FX_PLANES 5
#define FX_MAX_K 64             // the product asks for 25
#define FX_SAMPLE_CAP 65536u    // distinct sample ids a group's bitmap holds (8 KiB of LDS); more is HAWK_E_UNSUPPORTED
#define FX_SHORT_LIST 16u       // sample entries up to which one thread counts a group's distinct samples
#define FX_NONE 0xffffffffu
#define FX_TYPE_UNKNOWN 255
#define FX_SIGNED 0
#define FX_ABSOLUTE 1

// the group columns, in collapse order (start, strand, group)
struct FxCols {
  uint64_t n_groups, win_stride;
  const int64_t* start;
  const int64_t* stop;
  const uint8_t* strand;
  const uint64_t* win;          // [5][win_stride]
  const uint64_t* member_off;   // [n_groups + 1]
  const uint32_t* member_hap;   // haplotype row of every member, group after group
  const uint8_t* is_ref;        // [n_groups] the group's origin: that of its first member's haplotype row
  const uint64_t* hap_off;      // [n_hap + 1] CSR: haplotype row -> sample ids (REF rows empty)
  const uint32_t* sample_id;
  const uint32_t* rank;         // report rank of every group
  uint32_t n_hap, n_sample_ids, guidelen, pamlen, right;
};

HAWK_HD inline double fx_round4(double x) {
  FX_NO_CONTRACT
  if (!(fabs(x) < 274877906944.0)) return x;  // NaN, inf, |x| >= 2^38
  const double hi = x * 1e4, lo = fma(x, 1e4, -hi);  // x * 10^4 = hi + lo exactly (10^4 is exact)
  double k = rint(hi);                                // half-even on hi; |hi - k| <= 0.5 and hi - k is exact
  const double r = hi - k;
  // |r| < 0.5: r is at least one ulp(hi) away from 0.5 and |lo| <= ulp(hi) / 2 - k stands.  |r| == 0.5: lo decides, and an exact
  // tie (lo == 0) keeps rint's even k.
  if (r == 0.5) { if (lo > 0) k += 1.0; else if (lo == 0 && fmod(k, 2.0) != 0.0) k += 1.0; }
  else if (r == -0.5) { if (lo < 0) k -= 1.0; else if (lo == 0 && fmod(k, 2.0) != 0.0) k -= 1.0; }
  return k / 1e4;  // correctly rounded: the double that parsing the printed text gives
}

// score - ref_score; a NaN comes out as THE quiet NaN (which operand's sign and payload a subtraction hands on differs between
// the host's and the device's instruction sets)
HAWK_HD inline double fx_delta(double score, double ref_score) {
  FX_NO_CONTRACT
  const double d = score - ref_score;
  if (d == d) return d;
  union { uint64_t u; double d; } q;
  q.u = 0x7ff8000000000000ull;
  return q.d;
}

HAWK_HD inline bool fx_same_pos(const FxCols& c, uint64_t a, uint64_t b) { return c.start[a] == c.start[b] && c.strand[a] == c.strand[b]; }
HAWK_HD inline bool fx_is_ref(const FxCols& c, uint64_t g) { return c.is_ref[g] != 0; }
HAWK_HD inline uint64_t fx_head(const FxCols& c, uint64_t g) {
  while (g > 0 && fx_same_pos(c, g - 1, g)) --g;
  return g;
}
HAWK_HD inline uint64_t fx_end(const FxCols& c, uint64_t h) {
  uint64_t e = h + 1;
  while (e < c.n_groups && fx_same_pos(c, h, e)) ++e;
  return e;
}
HAWK_HD inline uint64_t fx_core_mask(const FxCols& c) { return ((c.guidelen + c.pamlen >= 64 ? 0ull : (1ull << (c.guidelen + c.pamlen))) - 1ull) << FX_PAD; }

// bit 0: the spacer holds a lower-case base, bit 1: the PAM does
HAWK_HD inline uint32_t fx_case_bits(const FxCols& c, uint64_t g) {
  const uint64_t v = (c.win[(uint64_t)4 * c.win_stride + g] >> FX_PAD);
  const bool pamfirst = (c.right != 0) != (c.strand[g] != 0);  // in window order
  const uint64_t first = pamfirst ? c.pamlen : c.guidelen, L = c.guidelen + c.pamlen;
  const uint64_t lo = v & ((1ull << first) - 1ull), hi = (v >> first) & ((1ull << (L - first)) - 1ull);
  const bool sp = pamfirst ? hi != 0 : lo != 0, pm = pamfirst ? lo != 0 : hi != 0;
  return (sp ? 1u : 0u) | (pm ? 2u : 0u);
}
HAWK_HD inline uint8_t fx_guide_type(bool is_ref, uint32_t case_bits) {
  if (is_ref) return 0;
  return case_bits == 3 ? 1 : case_bits == 1 ? 2 : case_bits == 2 ? 3 : FX_TYPE_UNKNOWN;
}
// the same (stop, cased sgRNA, cased pam) at one position
HAWK_HD inline bool fx_same_guide(const FxCols& c, uint64_t a, uint64_t b) {
  if (c.stop[a] != c.stop[b]) return false;
  const uint64_t m = fx_core_mask(c);
  for (int p = 0; p < FX_PLANES; ++p)
    if ((c.win[(uint64_t)p * c.win_stride + a] ^ c.win[(uint64_t)p * c.win_stride + b]) & m) return false;
  return true;
}
// an earlier group in report order shows the same guide
HAWK_HD inline bool fx_is_dup(const FxCols& c, uint64_t g, uint64_t h) {
  for (uint64_t j = h; j < c.n_groups && (j == h || fx_same_pos(c, h, j)); ++j)
    if (j != g && c.rank[j] < c.rank[g] && fx_same_guide(c, j, g)) return true;
  return false;
}

HAWK_HD inline bool fx_valid_alt(int family, double score, double ref_score) { return family == FX_ABSOLUTE || score < ref_score; }

// the worst delta of a position as a fold that takes the valid alternatives in ANY order
struct FxWorst {
  uint32_t n, first_rank;  // valid alternatives, the report rank of the first of them
  double first, best;      // the first one's value; min(delta) / max of the non-NaN abs_delta
  bool any;                // `best` holds a value
};
HAWK_HD inline FxWorst fx_worst_empty() { FxWorst w; w.n = 0; w.first_rank = FX_NONE; w.first = 0.0; w.best = 0.0; w.any = false; return w; }
HAWK_HD inline void fx_worst_add(FxWorst& w, int family, double delta, uint32_t rank) {
  const double v = family == FX_ABSOLUTE ? fabs(delta) : delta;
  ++w.n;
  if (rank < w.first_rank) { w.first_rank = rank; w.first = v; }
  if (v == v && (!w.any || (family == FX_ABSOLUTE ? v > w.best : v < w.best))) { w.best = v; w.any = true; }
}
HAWK_HD inline double fx_worst_value(const FxWorst& w, int family) {
  if (w.n == 0) return 0.0;
  if (family == FX_ABSOLUTE) return w.first != w.first ? w.first : w.best;
  return w.best;  // a valid alternative of the signed family has score < ref_score: its delta is no NaN
}

// one position, by its head: the REF group, the valid alternatives, the worst delta, its first appearance in the report
struct FxPosition {
  uint32_t ref, n_valid, first_rank;
  double ref_score, worst;
};
HAWK_HD inline uint32_t fx_find_ref(const FxCols& c, uint64_t h, uint64_t e) {
  uint32_t ref = FX_NONE;
  for (uint64_t j = h; j < e; ++j)
    if (fx_is_ref(c, j) && (ref == FX_NONE || c.rank[j] < c.rank[ref])) ref = (uint32_t)j;
  return ref;
}
HAWK_HD inline FxPosition fx_position(const FxCols& c, const double* score, int family, uint64_t h, uint64_t e) {
  FxPosition p;
  p.ref = fx_find_ref(c, h, e);
  p.first_rank = FX_NONE;
  p.ref_score = p.ref == FX_NONE ? 0.0 : fx_round4(score[p.ref]);
  FxWorst w = fx_worst_empty();
  for (uint64_t j = h; j < e; ++j) {
    if (c.rank[j] < p.first_rank) p.first_rank = c.rank[j];
    if (p.ref == FX_NONE || fx_is_ref(c, j)) continue;
    const double s = fx_round4(score[j]);
    if (fx_valid_alt(family, s, p.ref_score)) fx_worst_add(w, family, fx_delta(s, p.ref_score), c.rank[j]);
  }
  p.n_valid = w.n;
  p.worst = fx_worst_value(w, family) + 0.0;  // (-0.0 never ranks apart from 0.0)
  return p;
}

// the ranking: an order-preserving 64-bit image of the worst delta (NaN last either way), then the first report rank
HAWK_HD inline uint64_t fx_key(int family, double worst) {
  if (worst != worst) return 0xfffffffffffffffeull;
  union { double d; uint64_t u; } x;
  x.d = family == FX_ABSOLUTE ? -worst + 0.0 : worst + 0.0;  // descending = ascending on the negated value
  return (x.u >> 63) ? ~x.u : x.u | 0x8000000000000000ull;
}
struct FxEntry {
  uint64_t key;
  uint32_t rank, head;  // head == FX_NONE: no entry
};
HAWK_HD inline bool fx_before(const FxEntry& a, const FxEntry& b) { return a.key < b.key || (a.key == b.key && a.rank < b.rank); }

// ---- host only: what the passes rest on, checked where the arrays are host arrays (0 ok, 1 invalid, 2 unsupported)
inline int fx_check_sizes(uint64_t n_groups, uint32_t n_sample_ids, uint32_t guidelen, uint32_t pamlen) {
  if (guidelen == 0 || pamlen == 0) return 1;
  if (guidelen + pamlen + 2 * FX_PAD > 64 || n_groups >= 0xfffffffeull || n_sample_ids > FX_SAMPLE_CAP) return 2;
  return 0;
}
inline int fx_check_rank(const uint32_t* rank, uint64_t n_groups) {  // a permutation of [0, n_groups)
  if (n_groups && !rank) return 1;
  uint64_t* seen = n_groups ? new uint64_t[(n_groups + 63) / 64]() : nullptr;
  int rc = 0;
  for (uint64_t g = 0; g < n_groups && !rc; ++g) {
    if (rank[g] >= n_groups || (seen[rank[g] >> 6] >> (rank[g] & 63)) & 1) rc = 1;
    else seen[rank[g] >> 6] |= 1ull << (rank[g] & 63);
  }
  delete[] seen;
  return rc;
}
inline int fx_check_samples(const uint64_t* hap_off, const uint32_t* sample_id, uint32_t n_hap, uint32_t n_sample_ids) {
  if (!hap_off || hap_off[0] != 0) return 1;
  for (uint32_t h = 0; h < n_hap; ++h)
    if (hap_off[h + 1] < hap_off[h]) return 1;
  if (hap_off[n_hap] && !sample_id) return 1;
  for (uint64_t i = 0; i < hap_off[n_hap]; ++i)
    if (sample_id[i] >= n_sample_ids) return 1;
  return 0;
}
inline int fx_check_cols(const FxCols& c) {
  int rc = fx_check_sizes(c.n_groups, c.n_sample_ids, c.guidelen, c.pamlen);
  if (rc) return rc;
  if ((rc = fx_check_samples(c.hap_off, c.sample_id, c.n_hap, c.n_sample_ids))) return rc;
  if (c.n_groups == 0) return 0;
  if (!c.start || !c.stop || !c.strand || !c.win || !c.member_off || !c.member_hap || c.win_stride < c.n_groups) return 1;
  if ((rc = fx_check_rank(c.rank, c.n_groups))) return rc;
  if (c.member_off[0] != 0) return 1;
  for (uint64_t g = 0; g < c.n_groups; ++g) {
    if (c.member_off[g + 1] <= c.member_off[g] || c.strand[g] > 1) return 1;  // (a group has a first member: its origin)
    if (g && (c.start[g] < c.start[g - 1] || (c.start[g] == c.start[g - 1] && c.strand[g] < c.strand[g - 1]))) return 1;
  }
  for (uint64_t i = 0; i < c.member_off[c.n_groups]; ++i)
    if (c.member_hap[i] >= c.n_hap) return 1;
  return 0;
}
