// resolve_check_main.cpp - hawk_host_resolve_unphased (hawk_resolve.h through hawk_hostutil.hip) under the sanitizers, as a program
// of its own (make asan-resolve): the seam panel of the device tests - k = 2 at a 3-letter code, a 4-letter code, a multi-base ref,
// an ambiguous position in each part of the window, a thinned PAM position on both strands of a left- and a right-sided PAM, W =
// 64, W = 33 and the one-base guide (W = 24), a window that ends with its haplotype, keys with and without a REF partner, REF last - in heap
// buffers of exactly their size, checked against a plain walk over the strings (an odometer over the options, the PAM re-checked
// on the text, the redundancy rule on upper-cased cores); then the declines and the refusals.
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/hawk.h"

static int fails = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
  } while (0)

template <class T> static T* exact(const std::vector<T>& v) {  // a heap block of exactly the bytes (at least one, never read)
  T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
  if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
template <class T> static T* room(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

static uint32_t mask_of(char c) {
  static const char* letters = "?ACMGRSVTWYHKDBN";
  const char* p = strchr(letters, toupper((unsigned char)c));
  return p ? (uint32_t)(p - letters) : 0u;
}
static int popc(uint32_t m) { return __builtin_popcount(m); }
static std::string revcomp_pattern(const std::string& pam) {
  std::string out;
  for (auto it = pam.rbegin(); it != pam.rend(); ++it) {
    const uint32_t m = mask_of(*it);
    const uint32_t r = ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3);
    out.push_back("?ACMGRSVTWYHKDBN"[r]);
  }
  return out;
}
static uint64_t pack_pam(const std::string& s) {
  uint64_t v = 0;
  for (char c : s) v = (v << 4) | mask_of(c);
  return v;
}

struct Entry { std::string ref; };
struct Hap {
  std::string seq;
  bool is_ref;
  int64_t g0;                                  // genomic position of base 0 (identity position map)
  std::map<uint32_t, std::vector<Entry>> va;   // position -> allele entries
};
struct Row { uint32_t hap, pos, strand; };
struct Case {
  std::string pam;
  int guidelen;
  bool right;
  std::vector<Hap> haps;
  std::vector<Row> rows;
  int W() const { return guidelen + (int)pam.size() + 20; }
};
struct Guide { uint32_t row; std::string seq; };

// the plain walk: every combination of every valid row in product order, PAM re-checked on the text, then the redundancy rule
static bool walk(const Case& c, std::vector<Guide>* kept, std::vector<uint32_t>* n_res) {
  const int pl = (int)c.pam.size(), W = c.W();
  const std::string rc = revcomp_pattern(c.pam);
  std::vector<std::vector<std::string>> per_row(c.rows.size());
  for (size_t i = 0; i < c.rows.size(); ++i) {
    const Row& r = c.rows[i];
    const Hap& h = c.haps[r.hap];
    const bool rr = c.right != (r.strand != 0);
    const int64_t p0 = rr ? (int64_t)r.pos - 10 : (int64_t)r.pos - c.guidelen - 10;
    const bool valid = rr ? (int64_t)r.pos + c.guidelen + pl + 10 < (int64_t)h.seq.size() : p0 >= 0;
    if (!valid) continue;
    std::vector<std::string> opts(W);
    for (int k = 0; k < W; ++k) {
      const char ch = h.seq[p0 + k];
      const uint32_t m = mask_of(ch);
      if (popc(m) == 0) return false;
      if (popc(m) == 1) { opts[k] = std::string(1, ch); continue; }
      auto it = h.va.find((uint32_t)(p0 + k));
      if (it == h.va.end()) return false;
      for (int b = 0; b < 4; ++b)
        if ((m >> b) & 1u)
          for (const Entry& e : it->second) opts[k].push_back(e.ref == std::string(1, "ACGT"[b]) ? "ACGT"[b] : "acgt"[b]);
    }
    const int idx = rr ? 10 : W - 10 - pl;
    const std::string& pat = r.strand ? rc : c.pam;
    std::vector<size_t> d(W, 0);
    bool empty = false;
    for (int k = 0; k < W; ++k) empty = empty || opts[k].empty();
    while (!empty) {
      std::string s(W, '?');
      for (int k = 0; k < W; ++k) s[k] = opts[k][d[k]];
      bool ok = true;
      for (int t = 0; t < pl; ++t) ok = ok && (mask_of(pat[t]) & mask_of(s[idx + t]));
      if (ok) per_row[i].push_back(s);
      int k = W - 1;
      for (; k >= 0; --k) { if (++d[k] < opts[k].size()) break; d[k] = 0; }
      if (k < 0) break;
    }
  }
  auto upper_core = [&](const std::string& s) {
    std::string u = s.substr(10, W - 20);
    for (char& ch : u) ch = (char)toupper((unsigned char)ch);
    return u;
  };
  auto start_of = [&](const Row& r) {
    const bool rr = c.right != (r.strand != 0);
    return c.haps[r.hap].g0 + (rr ? (int64_t)r.pos : (int64_t)r.pos - c.guidelen);
  };
  n_res->assign(c.rows.size(), 0);
  for (size_t i = 0; i < c.rows.size(); ++i) {
    (*n_res)[i] = (uint32_t)per_row[i].size();
    const Row& r = c.rows[i];
    const std::string* refseq = nullptr;
    if (!c.haps[r.hap].is_ref)
      for (size_t j = 0; j < c.rows.size(); ++j)
        if (c.haps[c.rows[j].hap].is_ref && c.rows[j].strand == r.strand && start_of(c.rows[j]) == start_of(r) && !per_row[j].empty()) refseq = &per_row[j][0];
    for (const std::string& s : per_row[i])
      if (!refseq || upper_core(s) != upper_core(*refseq)) kept->push_back({(uint32_t)i, s});
  }
  return true;
}

struct Packed {
  hawk_resolve_columns c;
  hawk_resolve_alleles a;
  std::vector<void*> owned;
  ~Packed() { for (void* p : owned) free(p); }
  template <class T> T* keep(const std::vector<T>& v) { T* p = exact(v); owned.push_back(p); return p; }
};
static void pack(const Case& c, Packed* P) {
  const size_t n = c.rows.size();
  const int W = c.W();
  std::vector<uint32_t> hap, pos, hap_len, off{0};
  std::vector<uint8_t> strand, flags, is_ref, ref;
  std::vector<int64_t> start;
  std::vector<uint64_t> win(5 * n, 0), key;
  for (const Hap& h : c.haps) { hap_len.push_back((uint32_t)h.seq.size()); is_ref.push_back(h.is_ref ? 1 : 0); }
  auto start_of = [&](const Row& r) {
    const bool rr = c.right != (r.strand != 0);
    return c.haps[r.hap].g0 + (rr ? (int64_t)r.pos : (int64_t)r.pos - c.guidelen);
  };
  for (size_t i = 0; i < n; ++i) {
    const Row& r = c.rows[i];
    const bool rr = c.right != (r.strand != 0);
    const int64_t p0 = rr ? (int64_t)r.pos - 10 : (int64_t)r.pos - c.guidelen - 10;
    hap.push_back(r.hap); pos.push_back(r.pos); strand.push_back((uint8_t)r.strand); start.push_back(start_of(r));
    uint8_t f = 0;
    for (const Row& q : c.rows)
      if (c.haps[q.hap].is_ref && q.strand == r.strand && start_of(q) == start_of(r)) f = 1;
    flags.push_back(f);
    for (int k = 0; k < W; ++k) {
      const char ch = c.haps[r.hap].seq[p0 + k];
      const uint32_t code = mask_of(ch) | (islower((unsigned char)ch) ? 16u : 0u);
      for (int p = 0; p < 5; ++p)
        if ((code >> p) & 1u) win[p * n + i] |= 1ull << k;
    }
  }
  for (size_t h = 0; h < c.haps.size(); ++h)
    for (const auto& kv : c.haps[h].va) {
      key.push_back(((uint64_t)h << 32) | kv.first);
      for (const Entry& e : kv.second) ref.push_back(e.ref.size() == 1 && strchr("ACGT", e.ref[0]) ? (uint8_t)(strchr("ACGT", e.ref[0]) - "ACGT") : 255);
      off.push_back((uint32_t)ref.size());
    }
  memset(&P->c, 0, sizeof(P->c));
  P->c.n_rows = n; P->c.win_stride = n;
  P->c.hap = P->keep(hap); P->c.pos = P->keep(pos); P->c.strand = P->keep(strand); P->c.start = P->keep(start); P->c.flags = P->keep(flags);
  P->c.win = P->keep(win); P->c.hap_len = P->keep(hap_len); P->c.hap_is_ref = P->keep(is_ref);
  P->c.pam_fwd = pack_pam(c.pam); P->c.pam_rev = pack_pam(revcomp_pattern(c.pam));
  P->c.n_hap = (uint32_t)c.haps.size(); P->c.guidelen = (uint32_t)c.guidelen; P->c.pamlen = (uint32_t)c.pam.size(); P->c.right = c.right ? 1 : 0;
  P->a.n_keys = key.size(); P->a.key = P->keep(key); P->a.off = P->keep(off); P->a.ref = P->keep(ref);
}

static std::string decode(const uint64_t* win, uint64_t stride, uint64_t k, int W) {
  std::string s(W, '?');
  for (int i = 0; i < W; ++i) {
    uint32_t code = 0;
    for (int p = 0; p < 5; ++p) code |= (uint32_t)((win[p * stride + k] >> i) & 1u) << p;
    s[i] = "?ACMGRSVTWYHKDBN?acmgrsvtwyhkdbn"[code];
  }
  return s;
}

// the twin on a case in buffers of exactly their size, against the walk
static void run(const Case& c, const char* what, size_t want_guides = (size_t)-1) {
  std::vector<Guide> want;
  std::vector<uint32_t> want_res;
  CHECK(walk(c, &want, &want_res));
  Packed P;
  pack(c, &P);
  const size_t n = c.rows.size();
  uint32_t *res = room<uint32_t>(n), *kept = room<uint32_t>(n);
  uint64_t n_out = 0, n_res = 0;
  hawk_resolve_decline d;
  int rc = hawk_host_resolve_unphased(&P.c, &P.a, 0, res, kept, nullptr, nullptr, 0, &n_out, &n_res, &d);
  CHECK(rc == HAWK_OK && d.reason == 0 && n_out == want.size());
  if (want_guides != (size_t)-1) CHECK(want.size() == want_guides);
  uint32_t* src = room<uint32_t>(n_out);
  uint64_t* win = room<uint64_t>(5 * n_out);
  rc = hawk_host_resolve_unphased(&P.c, &P.a, 0, res, kept, src, win, n_out, &n_out, &n_res, &d);
  CHECK(rc == HAWK_OK);
  uint64_t sum = 0;
  for (size_t i = 0; i < n; ++i) { CHECK(res[i] == want_res[i]); sum += want_res[i]; }
  CHECK(sum == n_res);
  bool same = n_out == want.size();
  for (size_t k = 0; same && k < n_out; ++k) same = src[k] == want[k].row && decode(win, n_out, k, c.W()) == want[k].seq;
  if (!same) { fprintf(stderr, "FAILED case %s: the kept guides differ from the walk\n", what); ++fails; }
  if (n_out) {  // one output too few: refused with the need reported, nothing written past the buffer
    uint64_t need = 0;
    CHECK(hawk_host_resolve_unphased(&P.c, &P.a, 0, nullptr, nullptr, src, win, n_out - 1, &need, nullptr, &d) == HAWK_E_CAPACITY && d.reason == 0 && need == n_out);
  }
  free(res); free(kept); free(src); free(win);
}

static int declines(const Case& c, uint64_t batch, int* reason, int64_t* row) {
  Packed P;
  pack(c, &P);
  uint64_t n_out = 0;
  hawk_resolve_decline d;
  const int rc = hawk_host_resolve_unphased(&P.c, &P.a, batch, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d);
  *reason = d.reason; *row = d.row;
  return rc;
}

static std::string background(size_t n, const char* ab, uint32_t seed) {
  std::string s(n, ab[0]);
  for (size_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; s[i] = ab[(seed >> 16) & 1u]; }
  return s;
}
static Hap variant_of(const Hap& ref, std::map<uint32_t, std::pair<char, std::vector<Entry>>> edits) {
  Hap h = ref;
  h.is_ref = false;
  for (auto& kv : edits) { h.seq[kv.first] = kv.second.first; if (!kv.second.second.empty()) h.va[kv.first] = kv.second.second; }
  return h;
}
static char other(char c) { return c == 'A' ? 'T' : 'A'; }

int main() {
  const std::vector<Entry> AG{{"A"}};
  {  // options: k = 2 at a 3-letter code, a 4-letter code, a multi-base ref
    Hap ref{background(300, "AT", 1), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq[190] = 'A'; ref.seq[185] = 'A'; ref.seq[180] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{190, {'d', {{"A"}, {"A"}}}}}), variant_of(ref, {{185, {'n', {{"A"}}}}}),
                                variant_of(ref, {{180, {'r', {{"AT"}}}}})}, {{0, 200, 0}, {1, 200, 0}, {2, 200, 0}, {3, 200, 0}}};
    run(c, "options", 1 + 4 + 3 + 1);
  }
  {  // an ambiguous position in the left pad, the spacer, the first and last PAM base (thinned to its G) and the right pad
    Hap ref{background(300, "AT", 2), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq[173] = 'A'; ref.seq[195] = 'A'; ref.seq[208] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{173, {'w', AG}}, {195, {'r', AG}}, {200, {'r', AG}}, {202, {'r', {{"G"}}}}, {208, {'w', AG}}})},
           {{0, 200, 0}, {1, 200, 0}}};
    run(c, "positions", 1 + 12);
    c.haps = {c.haps[1], c.haps[0]};   // REF last: the same guides (the list order is Python's business)
    c.rows = {{0, 200, 0}, {1, 200, 0}};
    run(c, "ref last", 12 + 1);
    c.haps[1].is_ref = false;          // no REF at all: nothing is dropped
    run(c, "no partner", 16 + 1);
  }
  {  // strand 1 of a left-sided PAM (stored right), thinned PAM positions on both strands
    Hap ref{background(400, "AT", 3), true, 7000, {}};
    ref.seq.replace(160, 3, "AGG"); ref.seq.replace(260, 3, "CCA"); ref.seq[150] = 'A'; ref.seq[270] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{150, {'r', AG}}, {161, {'k', {{"G"}}}}, {270, {'r', AG}}, {261, {'m', {{"C"}}}}})},
           {{0, 160, 0}, {0, 260, 1}, {1, 160, 0}, {1, 260, 1}}};
    run(c, "strands left", 1 + 1 + 1 + 1);
  }
  {  // a right-sided PAM: strand 0 stored right, strand 1 not; V and B thin an n
    Hap ref{background(400, "CG", 4), true, 9000, {}};
    ref.seq.replace(150, 4, "TTTC"); ref.seq.replace(280, 4, "GAAA");
    Case c{"TTTV", 23, true, {ref, variant_of(ref, {{153, {'n', {{"C"}}}}, {160, {'s', {{"C"}}}}, {280, {'n', {{"G"}}}}, {270, {'s', {{"C"}}}}})},
           {{0, 150, 0}, {0, 280, 1}, {1, 150, 0}, {1, 280, 1}}};
    run(c, "strands right");
  }
  for (int guidelen : {41, 10, 1}) {  // W = 64, W = 33 (the first window longer than a word) and the smallest guide: one base, W = 24
    Hap ref{background(460, "AT", 5), true, 100, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq.replace(300, 3, "CCA");
    const uint32_t l0 = 200 - guidelen - 10, r0 = 212, l1 = 290, r1 = 300 + 3 + guidelen + 9;  // first and last base of either window
    Case c{"NGG", guidelen, false, {ref, variant_of(ref, {{l0, {'w', {{std::string(1, ref.seq[l0])}}}}, {199, {'w', {{std::string(1, ref.seq[199])}}}},
                                                               {r0, {'w', {{std::string(1, ref.seq[r0])}}}}, {l1, {'w', {{std::string(1, ref.seq[l1])}}}},
                                                               {303, {'w', {{std::string(1, ref.seq[303])}}}}, {r1, {'w', {{std::string(1, ref.seq[r1])}}}}})},
           {{0, 200, 0}, {0, 300, 1}, {1, 200, 0}, {1, 300, 1}}};
    run(c, guidelen == 41 ? "widest" : guidelen == 10 ? "w33" : "shortest", 1 + 1 + 4 + 4);
  }
  {  // a window that ends with its haplotype: a row, not valid, no guides; one base more and it resolves
    Hap ref{background(300, "AT", 7), true, 5000, {}};
    ref.seq.replace(200, 3, "CCA"); ref.seq[215] = 'A';
    Hap w1{ref.seq.substr(150, 83), false, 5150, {}}, w2{ref.seq.substr(150, 84), false, 5150, {}};
    w1.seq[65] = 'r'; w1.va[65] = AG; w2.seq[65] = 'r'; w2.va[65] = AG;
    Case c{"NGG", 20, false, {ref, w1, w2}, {{0, 200, 1}, {1, 50, 1}, {2, 50, 1}}};
    run(c, "haplotype end", 1 + 0 + 1);
  }
  {  // zero rows
    Case c{"NGG", 20, false, {Hap{background(100, "AT", 8), true, 0, {}}}, {}};
    run(c, "empty", 0);
  }
  // ---- the declines
  int reason; int64_t row;
  Hap ref{background(300, "AT", 9), true, 5000, {}};
  ref.seq.replace(200, 3, "AGG");
  {
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{190, {'g', {}}}, {185, {'N', {}}}})}, {{0, 200, 0}, {1, 200, 0}}};
    CHECK(declines(c, 0, &reason, &row) == HAWK_E_UNSUPPORTED && reason == HAWK_RESOLVE_NO_ENTRY && row == 1);
    c.haps[1].seq[185] = 'A'; c.haps[1].is_ref = true;
    CHECK(declines(c, 0, &reason, &row) == HAWK_E_UNSUPPORTED && reason == HAWK_RESOLVE_MULTI_REF && row == -1);
    Case a{"NGG", 20, false, {variant_of(ref, {{190, {'w', {{std::string(1, ref.seq[190])}}}}})}, {{0, 200, 0}}};
    a.haps[0].is_ref = true;
    CHECK(declines(a, 0, &reason, &row) == HAWK_E_UNSUPPORTED && reason == HAWK_RESOLVE_REF_AMBIG && row == 0);
  }
  {
    std::map<uint32_t, std::pair<char, std::vector<Entry>>> edits;
    for (uint32_t p = 171; p < 200; ++p) edits[p] = {'w', {{std::string(1, ref.seq[p])}}};
    for (uint32_t p : {200u, 205u, 207u}) edits[p] = {'w', {{std::string(1, ref.seq[p])}}};
    Case c{"NGG", 20, false, {ref, variant_of(ref, edits)}, {{0, 200, 0}, {1, 200, 0}}};   // 2^32 combinations: one too many
    CHECK(declines(c, 0, &reason, &row) == HAWK_E_CAPACITY && reason == HAWK_RESOLVE_ROW_SIZE && row == 1);
    Hap all = ref;
    all.is_ref = false;
    for (uint32_t p = 170; p < 213; ++p) { all.seq[p] = 'n'; all.va[p] = {{"A"}, {"A"}}; }   // 8^43: the count saturates
    Case s{"NGG", 20, false, {ref, all}, {{0, 200, 0}, {1, 200, 0}}};
    CHECK(declines(s, 0, &reason, &row) == HAWK_E_CAPACITY && reason == HAWK_RESOLVE_ROW_SIZE && row == 1);
  }
  {
    std::map<uint32_t, std::pair<char, std::vector<Entry>>> edits;
    for (uint32_t p = 190; p < 200; ++p) edits[p] = {'w', {{std::string(1, ref.seq[p])}}};
    Case c{"NGG", 20, false, {ref, variant_of(ref, edits)}, {{0, 200, 0}, {1, 200, 0}}};
    CHECK(declines(c, 1023 * 44, &reason, &row) == HAWK_OK && reason == 0);
    CHECK(declines(c, 1023 * 44 - 1, &reason, &row) == HAWK_E_CAPACITY && reason == HAWK_RESOLVE_BATCH && row == 1);
    run(c, "1023 of 1024", 1 + 1023);
  }
  {  // the refusals: malformed allele tables, bad geometry, missing arguments
    Case c{"NGG", 20, false, {ref}, {{0, 200, 0}}};
    Packed P;
    pack(c, &P);
    uint64_t n_out = 0;
    hawk_resolve_decline d;
    const uint64_t k_dup[2] = {5, 5}, k_desc[2] = {5, 4}, k_ok[2] = {4, 5};
    const uint32_t o_ok[3] = {0, 1, 2}, o_bad[3] = {0, 2, 1};
    const uint8_t r_ok[2] = {0, 255}, r_bad[2] = {0, 7};
    hawk_resolve_alleles a{2, k_dup, o_ok, r_ok};
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
    a.key = k_desc;
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
    a.key = k_ok; a.off = o_bad;
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
    a.off = o_ok; a.ref = r_bad;
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
    a.ref = r_ok;
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_OK && n_out == 1);
    CHECK(hawk_host_resolve_unphased(&P.c, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &d) == HAWK_E_INVALID);
    CHECK(hawk_host_resolve_unphased(nullptr, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
    hawk_resolve_columns wide = P.c;
    wide.guidelen = 42;   // W = 65
    CHECK(hawk_host_resolve_unphased(&wide, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_UNSUPPORTED);
    wide.guidelen = 0;
    CHECK(hawk_host_resolve_unphased(&wide, &a, 0, nullptr, nullptr, nullptr, nullptr, 0, &n_out, nullptr, &d) == HAWK_E_INVALID);
  }
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("resolve_check: ok\n");
  return 0;
}
