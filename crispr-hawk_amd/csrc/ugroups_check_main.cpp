// ugroups_check_main.cpp - hawk_host_unphased_groups (hawk_ugroups.h through hawk_hostutil.hip) under the sanitizers, as a program
// of its own (make asan-ugroups): scenes of the device tests - two haplotypes sharing a core, ambiguous positions all in the pads
// and all in the core, both strands of a left- and a right-sided PAM, W = 64, W = 33 and the one-base guide, a key without a REF
// partner, a REF row that keeps nothing - resolved by hawk_host_resolve_unphased (which resolve_check_main.cpp holds to its own
// walk), then grouped in heap buffers of exactly their size and checked against a plain walk over the decoded strings: a map keyed
// by (start, stop, strand, origin, cased slice), CFDon as a product over the reversed strings; then the refusals.
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <tuple>
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

static const char* LETTERS = "?ACMGRSVTWYHKDBN";
static uint32_t mask_of(char c) {
  const char* p = strchr(LETTERS, toupper((unsigned char)c));
  return p ? (uint32_t)(p - LETTERS) : 0u;
}
static std::string revcomp_pattern(const std::string& pam) {
  std::string out;
  for (auto it = pam.rbegin(); it != pam.rend(); ++it) {
    const uint32_t m = mask_of(*it);
    out.push_back(LETTERS[((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3)]);
  }
  return out;
}
static uint64_t pack_pam(const std::string& s) {
  uint64_t v = 0;
  for (char c : s) v = (v << 4) | mask_of(c);
  return v;
}

struct Hap {
  std::string seq;
  bool is_ref;
  int64_t g0;                                       // genomic position of base 0 (identity position map)
  std::map<uint32_t, std::vector<std::string>> va;  // position -> ref of each allele entry
};
struct Row { uint32_t hap, pos, strand; };
struct Case {
  std::string pam;
  int guidelen;
  bool right;
  std::vector<Hap> haps;
  std::vector<Row> rows;
  int L() const { return guidelen + (int)pam.size(); }
  int W() const { return L() + 20; }
};

struct Packed {
  hawk_resolve_columns c;
  hawk_resolve_alleles a;
  int64_t* stop;
  std::vector<void*> owned;
  ~Packed() { for (void* p : owned) free(p); }
  template <class T> T* keep(const std::vector<T>& v) { T* p = exact(v); owned.push_back(p); return p; }
};
static void pack(const Case& c, Packed* P) {
  const size_t n = c.rows.size();
  const int W = c.W();
  std::vector<uint32_t> hap, pos, hap_len, off{0};
  std::vector<uint8_t> strand, flags, is_ref, ref;
  std::vector<int64_t> start, stop;
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
    hap.push_back(r.hap); pos.push_back(r.pos); strand.push_back((uint8_t)r.strand); start.push_back(start_of(r)); stop.push_back(start_of(r) + c.L());
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
      for (const std::string& e : kv.second) ref.push_back(e.size() == 1 && strchr("ACGT", e[0]) ? (uint8_t)(strchr("ACGT", e[0]) - "ACGT") : 255);
      off.push_back((uint32_t)ref.size());
    }
  memset(&P->c, 0, sizeof(P->c));
  P->c.n_rows = n; P->c.win_stride = n;
  P->c.hap = P->keep(hap); P->c.pos = P->keep(pos); P->c.strand = P->keep(strand); P->c.start = P->keep(start); P->c.flags = P->keep(flags);
  P->c.win = P->keep(win); P->c.hap_len = P->keep(hap_len); P->c.hap_is_ref = P->keep(is_ref);
  P->stop = P->keep(stop);
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
static std::string upper(std::string s) { for (char& ch : s) ch = (char)toupper((unsigned char)ch); return s; }
static std::string revcomp(const std::string& s) {
  std::string o;
  for (auto it = s.rbegin(); it != s.rend(); ++it) o.push_back(*it == 'A' ? 'T' : *it == 'C' ? 'G' : *it == 'G' ? 'C' : *it == 'T' ? 'A' : 'N');
  return o;
}
static int base_of(char ch) { const char* p = strchr("ACGT", ch); return p ? (int)(p - "ACGT") : -1; }

static std::vector<double> tables() {  // [320] + [16], a fixed LCG
  std::vector<double> t(336);
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (double& v : t) { s = s * 6364136223846793005ull + 1442695040888963407ull; v = (double)(s >> 11) / 9007199254740992.0; }
  return t;
}

struct WantGroup {
  uint32_t rep_row, hap, pos, strand;
  int64_t start, stop;
  bool origin;
  double cfdon;
  std::string window;
  uint32_t gc_num, gc_den;
  std::vector<uint32_t> members;
};

// the plain walk over the decoded strings of the kept guides
static std::vector<WantGroup> walk(const Case& c, const Packed& P, const uint32_t* src, const std::vector<std::string>& seqs, int up, int down,
                                   const double* mm, const double* pt) {
  const int W = c.W(), L = c.L(), pl = (int)c.pam.size();
  std::map<std::pair<int64_t, int>, std::string> refguide;
  for (size_t k = 0; k < seqs.size(); ++k) {
    const uint32_t i = src[k];
    if (c.haps[P.c.hap[i]].is_ref) refguide[{P.c.start[i], P.c.strand[i]}] = seqs[k];
  }
  // key order as documented: start, strand, origin, stop, then the slice's planes A, C, G, T, case as integers (bit 0 = leftmost)
  typedef std::tuple<int64_t, int, int, int64_t, std::vector<uint64_t>> Key;
  std::map<Key, std::vector<std::tuple<uint32_t, uint32_t, size_t>>> groups;
  for (size_t k = 0; k < seqs.size(); ++k) {
    const uint32_t i = src[k];
    const int strand = P.c.strand[i];
    const int fl = strand ? down : up, fr = strand ? up : down;
    const std::string slice = seqs[k].substr(10 - fl, L + fl + fr);
    std::vector<uint64_t> planes(5, 0);
    for (size_t j = 0; j < slice.size(); ++j) {
      const uint32_t code = mask_of(slice[j]) | (islower((unsigned char)slice[j]) ? 16u : 0u);
      for (int p = 0; p < 5; ++p)
        if ((code >> p) & 1u) planes[p] |= 1ull << j;
    }
    groups[Key(P.c.start[i], strand, c.haps[P.c.hap[i]].is_ref ? 1 : 0, P.stop[i], planes)].emplace_back(P.c.hap[i], P.c.pos[i], k);
  }
  std::vector<WantGroup> out;
  for (auto& kv : groups) {
    std::sort(kv.second.begin(), kv.second.end());
    const size_t k = std::get<2>(kv.second[0]);
    const uint32_t i = src[k];
    WantGroup g;
    g.rep_row = i; g.hap = P.c.hap[i]; g.pos = P.c.pos[i]; g.strand = P.c.strand[i]; g.start = P.c.start[i]; g.stop = P.stop[i];
    g.origin = c.haps[g.hap].is_ref; g.window = seqs[k];
    const std::string core = seqs[k].substr(10, W - 20);
    g.cfdon = std::nan("");
    auto it = refguide.find({g.start, (int)g.strand});
    if (mm && it != refguide.end()) {
      std::string gd = upper(core), rf = upper(it->second.substr(10, W - 20));
      if (g.strand) { gd = revcomp(gd); rf = revcomp(rf); }
      double s = 1.0;
      for (int t = 0; t < std::min(c.guidelen, 20); ++t)
        if (gd[t] != rf[t]) s *= mm[(t * 4 + base_of(rf[t])) * 4 + base_of(gd[t])];
      g.cfdon = s * pt[4 * base_of(gd[L - 2]) + base_of(gd[L - 1])];
    }
    const bool pamfirst = c.right != (g.strand != 0);
    const std::string spacer = pamfirst ? core.substr(pl) : core.substr(0, c.guidelen);
    g.gc_num = g.gc_den = 0;
    for (char ch : spacer) {
      if (strchr("CGScgs", ch)) { ++g.gc_num; ++g.gc_den; }
      else if (strchr("ATWUatwu", ch)) ++g.gc_den;
    }
    std::set<uint32_t> hs;
    for (auto& m : kv.second) hs.insert(std::get<0>(m));
    g.members.assign(hs.begin(), hs.end());
    out.push_back(g);
  }
  return out;
}

static bool same_double(double a, double b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, 8) == 0; }

// resolve a case, group it at one flank in buffers of exactly their size, compare with the walk; returns the number of groups
static size_t run(const Case& c, const char* what, int up, int down, bool with_tables, size_t want_kept = (size_t)-1) {
  Packed P;
  pack(c, &P);
  uint64_t nk = 0, nres = 0;
  hawk_resolve_decline d;
  CHECK(hawk_host_resolve_unphased(&P.c, &P.a, 0, nullptr, nullptr, nullptr, nullptr, 0, &nk, &nres, &d) == HAWK_OK);
  if (want_kept != (size_t)-1) CHECK(nk == want_kept);
  uint32_t* src = room<uint32_t>(nk);
  uint64_t* win = room<uint64_t>(5 * nk);
  CHECK(hawk_host_resolve_unphased(&P.c, &P.a, 0, nullptr, nullptr, src, win, nk, &nk, &nres, &d) == HAWK_OK);
  std::vector<std::string> seqs;
  for (uint64_t k = 0; k < nk; ++k) seqs.push_back(decode(win, nk, k, c.W()));
  const std::vector<double> tab = tables();
  double *mm = nullptr, *pt = nullptr;
  if (with_tables) { mm = exact(std::vector<double>(tab.begin(), tab.begin() + 320)); pt = exact(std::vector<double>(tab.begin() + 320, tab.end())); }
  const std::vector<WantGroup> want = walk(c, P, src, seqs, up, down, mm, pt);
  uint64_t ng = 0, nm = 0;
  int rc = hawk_host_unphased_groups(&P.c, P.stop, src, win, nk, nk, mm, pt, (uint32_t)up, (uint32_t)down, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ng, &nm);
  size_t want_members = 0;
  for (const WantGroup& g : want) want_members += g.members.size();
  CHECK(rc == HAWK_OK && ng == want.size() && nm == want_members);
  uint32_t *rep = room<uint32_t>(ng), *hap = room<uint32_t>(ng), *pos = room<uint32_t>(ng), *mh = room<uint32_t>(nm);
  uint8_t *strand = room<uint8_t>(ng), *isr = room<uint8_t>(ng), *gn = room<uint8_t>(ng), *gd = room<uint8_t>(ng);
  int64_t *start = room<int64_t>(ng), *stop = room<int64_t>(ng);
  double* cfd = room<double>(ng);
  uint64_t *ow = room<uint64_t>(5 * ng), *mo = room<uint64_t>(ng + 1);
  rc = hawk_host_unphased_groups(&P.c, P.stop, src, win, nk, nk, mm, pt, (uint32_t)up, (uint32_t)down, ng, nm, rep, hap, pos, strand, start, stop, isr, cfd, ow,
                                 gn, gd, mo, mh, &ng, &nm);
  CHECK(rc == HAWK_OK);
  bool same = rc == HAWK_OK && ng == want.size() && mo[ng] == nm;
  for (size_t g = 0; same && g < ng; ++g) {
    const WantGroup& w = want[g];
    same = rep[g] == w.rep_row && hap[g] == w.hap && pos[g] == w.pos && strand[g] == w.strand && start[g] == w.start && stop[g] == w.stop &&
           isr[g] == (w.origin ? 1 : 0) && same_double(cfd[g], w.cfdon) && decode(ow, ng, g, c.W()) == w.window && gn[g] == w.gc_num && gd[g] == w.gc_den &&
           mo[g + 1] - mo[g] == w.members.size();
    for (size_t m = 0; same && m < w.members.size(); ++m) same = mh[mo[g] + m] == w.members[m];
  }
  if (!same) { fprintf(stderr, "FAILED case %s (flank %d, %d%s): the groups differ from the walk\n", what, up, down, with_tables ? ", tables" : ""); ++fails; }
  if (ng) {  // one group too few, one member too few: refused with the need reported, nothing written past the buffers
    uint64_t a = 0, b = 0;
    CHECK(hawk_host_unphased_groups(&P.c, P.stop, src, win, nk, nk, mm, pt, (uint32_t)up, (uint32_t)down, ng - 1, nm, rep, hap, pos, strand, start, stop, isr,
                                    cfd, ow, gn, gd, mo, mh, &a, &b) == HAWK_E_CAPACITY && a == ng && b == nm);
    CHECK(hawk_host_unphased_groups(&P.c, P.stop, src, win, nk, nk, mm, pt, (uint32_t)up, (uint32_t)down, ng, nm - 1, rep, hap, pos, strand, start, stop, isr,
                                    cfd, ow, gn, gd, mo, mh, &a, &b) == HAWK_E_CAPACITY && a == ng && b == nm);
  }
  for (void* p : {(void*)src, (void*)win, (void*)rep, (void*)hap, (void*)pos, (void*)mh, (void*)strand, (void*)isr, (void*)gn, (void*)gd, (void*)start,
                  (void*)stop, (void*)cfd, (void*)ow, (void*)mo, (void*)mm, (void*)pt})
    free(p);
  return ng;
}
static void run_all(const Case& c, const char* what, size_t want_kept = (size_t)-1) {
  for (int t = 0; t < 2; ++t) { run(c, what, 0, 0, t != 0, want_kept); run(c, what, 4, 3, t != 0, want_kept); }
}

static std::string background(size_t n, const char* ab, uint32_t seed) {
  std::string s(n, ab[0]);
  for (size_t i = 0; i < n; ++i) { seed = seed * 1664525u + 1013904223u; s[i] = ab[(seed >> 16) & 1u]; }
  return s;
}
typedef std::map<uint32_t, std::pair<char, std::vector<std::string>>> Edits;
static Hap variant_of(const Hap& ref, const Edits& edits) {
  Hap h = ref;
  h.is_ref = false;
  for (auto& kv : edits) { h.seq[kv.first] = kv.second.first; if (!kv.second.second.empty()) h.va[kv.first] = kv.second.second; }
  return h;
}

int main() {
  const std::vector<std::string> A{"A"};
  {  // two haplotypes with the same variant base in one spacer: one group, two members
    Hap ref{background(300, "AT", 1), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq[190] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{190, {'r', A}}}), variant_of(ref, {{190, {'r', A}}})}, {{0, 200, 0}, {1, 200, 0}, {2, 200, 0}}};
    run_all(c, "shared core", 3);
    CHECK(run(c, "shared core", 0, 0, true) == 2);
  }
  {  // ten two-way positions in the pads behind a fixed variant base: 1024 kept guides, one core
    Hap ref{background(300, "AT", 2), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq[190] = 'A';
    Edits e{{190, {'g', {}}}};
    for (uint32_t p : {175u, 176u, 177u, 178u, 179u, 203u, 204u, 205u, 206u, 207u}) e[p] = {'w', {std::string(1, ref.seq[p])}};
    Case c{"NGG", 20, false, {ref, variant_of(ref, e)}, {{0, 200, 0}, {1, 200, 0}}};
    run_all(c, "pads", 1 + 1024);
    CHECK(run(c, "pads", 0, 0, true) == 2 && run(c, "pads", 4, 3, true) == 1 + 128 && run(c, "pads", 10, 10, false) == 1 + 1024);
  }
  {  // ten two-way positions in the spacer: every kept guide a group of its own; with and without a REF partner
    Hap ref{background(300, "AT", 3), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG");
    Edits e;
    for (uint32_t p = 180; p < 190; ++p) e[p] = {'w', {std::string(1, ref.seq[p])}};
    Case c{"NGG", 20, false, {ref, variant_of(ref, e)}, {{0, 200, 0}, {1, 200, 0}}};
    run_all(c, "core", 1 + 1023);
    CHECK(run(c, "core", 0, 0, true) == 1 + 1023);
    c.haps[0].is_ref = false;  // no REF at all: nothing dropped, every CFDon NaN
    run_all(c, "core, no partner", 1 + 1024);
  }
  {  // strand 1 of a left-sided PAM, thinned PAM positions on both strands
    Hap ref{background(400, "AT", 4), true, 7000, {}};
    ref.seq.replace(160, 3, "AGG"); ref.seq.replace(260, 3, "CCA"); ref.seq[150] = 'A'; ref.seq[270] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{150, {'r', A}}, {161, {'k', {"G"}}}, {270, {'r', A}}, {261, {'m', {"C"}}}})},
           {{0, 160, 0}, {0, 260, 1}, {1, 160, 0}, {1, 260, 1}}};
    run_all(c, "strands left", 4);
  }
  {  // a right-sided PAM: strand 0 stored right, strand 1 not
    Hap ref{background(400, "CG", 5), true, 9000, {}};
    ref.seq.replace(150, 4, "TTTC"); ref.seq.replace(280, 4, "GAAA");
    Case c{"TTTV", 23, true, {ref, variant_of(ref, {{153, {'n', {"C"}}}, {160, {'s', {"C"}}}, {280, {'n', {"G"}}}, {270, {'s', {"C"}}}})},
           {{0, 150, 0}, {0, 280, 1}, {1, 150, 0}, {1, 280, 1}}};
    run_all(c, "strands right");
  }
  for (int guidelen : {41, 10, 1}) {  // W = 64, W = 33 and the one-base guide (W = 24), ambiguous first and last window bases
    Hap ref{background(460, "AT", 6), true, 100, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq.replace(300, 3, "CCA");
    const uint32_t l0 = 200 - guidelen - 10, r0 = 212, l1 = 290, r1 = 300 + 3 + guidelen + 9;
    Edits e;
    for (uint32_t p : {l0, 199u, r0, l1, 303u, r1}) e[p] = {'w', {std::string(1, ref.seq[p])}};
    Case c{"NGG", guidelen, false, {ref, variant_of(ref, e)}, {{0, 200, 0}, {0, 300, 1}, {1, 200, 0}, {1, 300, 1}}};
    run_all(c, guidelen == 41 ? "widest" : guidelen == 10 ? "w33" : "shortest", 1 + 1 + 4 + 4);
    run(c, "flank 10", 10, 10, true);
    run(c, "flank 10, 0", 10, 0, true);
  }
  {  // a REF row whose window ends with REF: it keeps nothing and is no partner; the longer copy's guides score NaN
    Hap ref{background(300, "AT", 7), true, 5000, {}};
    ref.seq.replace(200, 3, "CCA"); ref.seq[215] = 'A';
    Hap copy = variant_of(ref, {{215, {'r', A}}});
    ref.seq = ref.seq.substr(0, 233);
    Case c{"NGG", 20, false, {ref, copy}, {{0, 200, 1}, {1, 200, 1}}};
    run_all(c, "short REF", 0 + 2);
  }
  {  // zero rows, zero kept guides
    Case c{"NGG", 20, false, {Hap{background(100, "AT", 8), true, 0, {}}}, {}};
    run_all(c, "empty", 0);
  }
  {  // the refusals
    Hap ref{background(300, "AT", 9), true, 5000, {}};
    ref.seq.replace(200, 3, "AGG"); ref.seq[190] = 'A';
    Case c{"NGG", 20, false, {ref, variant_of(ref, {{190, {'r', A}}})}, {{0, 200, 0}, {1, 200, 0}}};
    Packed P;
    pack(c, &P);
    const uint32_t src[2] = {0, 1}, back[2] = {1, 0}, far[2] = {0, 2};
    uint64_t win[10], ng = 0, nm = 0;
    for (int p = 0; p < 5; ++p) { win[2 * p] = P.c.win[2 * p]; win[2 * p + 1] = P.c.win[2 * p + 1] & ~(p < 4 && p != 2 ? 1ull << 20 : 0ull); }
    const std::vector<double> tab = tables();
#define UGCALL(cols, st, s, up, dn, a, b) \
  hawk_host_unphased_groups(cols, st, s, win, 2, 2, tab.data(), tab.data() + 320, up, dn, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, \
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, a, b)
    CHECK(UGCALL(&P.c, P.stop, src, 0, 0, &ng, &nm) == HAWK_OK && ng == 2 && nm == 2);
    CHECK(UGCALL(&P.c, P.stop, src, 11, 0, &ng, &nm) == HAWK_E_UNSUPPORTED);
    CHECK(UGCALL(&P.c, P.stop, src, 0, 11, &ng, &nm) == HAWK_E_UNSUPPORTED);
    CHECK(UGCALL(&P.c, P.stop, back, 0, 0, &ng, &nm) == HAWK_E_INVALID);
    CHECK(UGCALL(&P.c, P.stop, far, 0, 0, &ng, &nm) == HAWK_E_INVALID);
    CHECK(UGCALL(&P.c, nullptr, src, 0, 0, &ng, &nm) == HAWK_E_INVALID);
    CHECK(UGCALL(nullptr, P.stop, src, 0, 0, &ng, &nm) == HAWK_E_INVALID);
    CHECK(UGCALL(&P.c, P.stop, src, 0, 0, nullptr, &nm) == HAWK_E_INVALID);
    CHECK(hawk_host_unphased_groups(&P.c, P.stop, src, win, 2, 2, tab.data(), nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ng, &nm) == HAWK_E_INVALID);
    hawk_resolve_columns wide = P.c;
    wide.guidelen = 42;  // W = 65
    CHECK(UGCALL(&wide, P.stop, src, 0, 0, &ng, &nm) == HAWK_E_UNSUPPORTED);
    wide.guidelen = 0;
    CHECK(UGCALL(&wide, P.stop, src, 0, 0, &ng, &nm) == HAWK_E_INVALID);
    win[1] |= 1ull << 20; win[3] |= 1ull << 20;  // an A and a C at one spacer position of the variant's guide where REF has one base
    CHECK(UGCALL(&P.c, P.stop, src, 0, 0, &ng, &nm) == HAWK_E_CFD);
#undef UGCALL
  }
  if (fails) { fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  printf("ugroups_check: ok\n");
  return 0;
}
