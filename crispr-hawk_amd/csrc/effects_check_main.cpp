// effects_check_main.cpp - hawk_host_effects / hawk_host_round4 (hawk_effects.h through hawk_hostutil.hip) under the sanitizers, as a
// program of its own (make asan-effects): the seam panel of the device tests - positions of 1, 2, 63, 64, 65 groups over 513 groups,
// no REF / REF only / REF last, member lists of 1 .. 4097 rows, sample ids up to the cap - 1, the report in reverse order, K = 1,
// 25, 64, candidates, zero groups - in heap buffers of exactly their size, checked against a plain restatement; then the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <set>
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

struct Panel {
  uint32_t guidelen = 20, pamlen = 3, right = 0, n_ids = 0;
  std::vector<int64_t> start, stop;
  std::vector<uint8_t> strand, hap_is_ref{1};
  std::vector<uint64_t> win[5], member_off{0}, hap_off{0, 0};
  std::vector<uint32_t> member_hap, sample_id, rank;
  std::vector<double> score;
  uint32_t hap(std::vector<uint32_t> ids) {
    for (uint32_t i : ids) { sample_id.push_back(i); n_ids = std::max(n_ids, i + 1); }
    hap_off.push_back(sample_id.size());
    hap_is_ref.push_back(0);
    return (uint32_t)hap_is_ref.size() - 1;
  }
  void group(int64_t s, uint8_t st, double sc, const std::vector<uint32_t>& mem, uint64_t lower_bits, uint64_t c_bits) {
    start.push_back(s); stop.push_back(s + 23); strand.push_back(st); score.push_back(sc);
    for (uint32_t h : mem) member_hap.push_back(h);
    member_off.push_back(member_hap.size());
    // plane 0 = A, plane 1 = C (IUPAC nibble bits), plane 4 = lower case; the core starts at bit 10
    const uint64_t core = (1ull << 23) - 1;
    win[0].push_back(((core & ~c_bits) << 10) | 0x3ff); win[1].push_back((c_bits & core) << 10); win[2].push_back(0); win[3].push_back(0);
    win[4].push_back((lower_bits & core) << 10);
  }
  size_t n() const { return start.size(); }
};

struct Out {
  hawk_effects_out o;
  size_t G, K;
  Out(size_t g, size_t k, size_t alt_cap) : G(g), K(k) {
    o.score = room<double>(g); o.delta = room<double>(g); o.abs_delta = room<double>(g); o.n_samples = room<uint32_t>(g);
    o.type = room<uint8_t>(g); o.dup = room<uint8_t>(g); o.position = room<uint32_t>(g); o.pos_ref = room<uint32_t>(g);
    o.pos_worst = room<double>(g); o.pos_nvalid = room<uint32_t>(g); o.pos_first_rank = room<uint32_t>(g);
    o.chosen = room<uint32_t>(k); o.alt_off = room<uint64_t>(k + 1); o.alt_group = room<uint32_t>(alt_cap); o.counts = room<uint64_t>(8);
  }
  ~Out() {
    free(o.score); free(o.delta); free(o.abs_delta); free(o.n_samples); free(o.type); free(o.dup); free(o.position); free(o.pos_ref);
    free(o.pos_worst); free(o.pos_nvalid); free(o.pos_first_rank); free(o.chosen); free(o.alt_off); free(o.alt_group); free(o.counts);
  }
};

struct Cols {
  hawk_effects_columns c;
  std::vector<void*> held;
  template <class T> const T* keep(const std::vector<T>& v) { T* p = exact(v); held.push_back(p); return p; }
  Cols(const Panel& p) {
    memset(&c, 0, sizeof(c));
    c.n_groups = p.n(); c.win_stride = p.n();
    c.start = keep(p.start); c.stop = keep(p.stop); c.strand = keep(p.strand);
    std::vector<uint64_t> w;
    for (int k = 0; k < 5; ++k) w.insert(w.end(), p.win[k].begin(), p.win[k].end());
    c.win = keep(w); c.cfdon = keep(p.score); c.member_off = keep(p.member_off); c.member_hap = keep(p.member_hap);
    c.hap_is_ref = keep(p.hap_is_ref); c.hap_off = keep(p.hap_off); c.sample_id = keep(p.sample_id); c.rank = keep(p.rank);
    c.n_hap = (uint32_t)p.hap_is_ref.size(); c.n_sample_ids = p.n_ids; c.guidelen = p.guidelen; c.pamlen = p.pamlen; c.right = p.right;
  }
  ~Cols() { for (void* q : held) free(q); }
};

static double py_round4_slow(double x) {  // through the decimal text, as the report is read back
  char buf[64];
  snprintf(buf, sizeof buf, "%.4f", x);  // glibc prints the exact binary value correctly rounded, ties to even
  return strtod(buf, nullptr);
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static void check_panel(const Panel& p, int family, uint32_t K, const std::vector<std::pair<int64_t, uint8_t>>& cands) {
  Cols C(p);
  const size_t G = p.n();
  Out out(G, K, G);
  std::vector<int64_t> cs; std::vector<uint8_t> ct;
  for (auto& c : cands) { cs.push_back(c.first); ct.push_back(c.second); }
  int64_t* d_cs = exact(cs); uint8_t* d_ct = exact(ct);
  uint32_t n_chosen = 0; uint64_t n_alts = 0;
  const int rc = hawk_host_effects(&C.c, family, nullptr, d_cs, d_ct, (uint32_t)cs.size(), K, &out.o, G, &n_chosen, &n_alts);
  CHECK(rc == HAWK_OK);
  // a plain restatement, position by position
  std::vector<double> rs(G);
  for (size_t g = 0; g < G; ++g) { rs[g] = py_round4_slow(p.score[g]); CHECK(std::isnan(rs[g]) ? std::isnan(out.o.score[g]) : rs[g] == out.o.score[g]); }
  struct Pos { size_t h, e; uint32_t ref, first; double worst; std::vector<uint32_t> alts; };
  std::vector<Pos> pos;
  for (size_t h = 0; h < G;) {
    size_t e = h + 1;
    while (e < G && p.start[e] == p.start[h] && p.strand[e] == p.strand[h]) ++e;
    Pos q{h, e, 0xffffffffu, 0xffffffffu, 0.0, {}};
    for (size_t j = h; j < e; ++j) {
      q.first = std::min(q.first, p.rank[j]);
      if (p.hap_is_ref[p.member_hap[p.member_off[j]]] && (q.ref == 0xffffffffu || p.rank[j] < p.rank[q.ref])) q.ref = (uint32_t)j;
    }
    for (size_t j = h; j < e; ++j) {
      CHECK(out.o.position[j] == h);
      const double d = q.ref == 0xffffffffu ? 0.0 : rs[j] - rs[q.ref];
      CHECK(std::isnan(d) ? std::isnan(out.o.delta[j]) : (d == out.o.delta[j] && std::fabs(d) == out.o.abs_delta[j]));
      if (q.ref != 0xffffffffu && !p.hap_is_ref[p.member_hap[p.member_off[j]]] && (family == HAWK_FX_ABSOLUTE || rs[j] < rs[q.ref])) q.alts.push_back((uint32_t)j);
    }
    std::sort(q.alts.begin(), q.alts.end(), [&](uint32_t a, uint32_t b) { return p.rank[a] < p.rank[b]; });
    if (!q.alts.empty()) {  // the fold as Python runs it, in report order
      double w = family == HAWK_FX_ABSOLUTE ? std::fabs(rs[q.alts[0]] - rs[q.ref]) : rs[q.alts[0]] - rs[q.ref];
      for (size_t k = 1; k < q.alts.size(); ++k) {
        const double v = family == HAWK_FX_ABSOLUTE ? std::fabs(rs[q.alts[k]] - rs[q.ref]) : rs[q.alts[k]] - rs[q.ref];
        if (family == HAWK_FX_ABSOLUTE ? v > w : v < w) w = v;
      }
      q.worst = w;
    }
    CHECK(out.o.pos_ref[h] == q.ref && out.o.pos_nvalid[h] == q.alts.size() && out.o.pos_first_rank[h] == q.first);
    CHECK(std::isnan(q.worst) ? std::isnan(out.o.pos_worst[h]) : q.worst == out.o.pos_worst[h]);
    pos.push_back(q);
    h = e;
  }
  CHECK(out.o.counts[5] == pos.size());
  // distinct samples, by a set
  for (size_t g = 0; g < G; ++g) {
    std::set<uint32_t> s;
    if (!p.hap_is_ref[p.member_hap[p.member_off[g]]])
      for (uint64_t m = p.member_off[g]; m < p.member_off[g + 1]; ++m)
        for (uint64_t e = p.hap_off[p.member_hap[m]]; e < p.hap_off[p.member_hap[m] + 1]; ++e) s.insert(p.sample_id[e]);
    CHECK(out.o.n_samples[g] == s.size());
  }
  // the ranking: candidates, then a stable sort of the others by (NaN last, worst in the family's direction, first rank)
  std::vector<const Pos*> others;
  std::vector<uint32_t> want;
  for (auto& c : cands) {
    uint32_t at = 0xffffffffu;
    for (auto& q : pos) if (q.ref != 0xffffffffu && p.start[q.h] == c.first && p.strand[q.h] == c.second) at = (uint32_t)q.h;
    want.push_back(at);
  }
  for (auto& q : pos) {
    bool is_c = false;
    for (auto& c : cands) is_c = is_c || (p.start[q.h] == c.first && p.strand[q.h] == c.second);
    if (q.ref != 0xffffffffu && !is_c) others.push_back(&q);
  }
  std::sort(others.begin(), others.end(), [&](const Pos* a, const Pos* b) {
    const bool an = std::isnan(a->worst), bn = std::isnan(b->worst);
    if (an != bn) return bn;
    if (!an && a->worst != b->worst) return family == HAWK_FX_ABSOLUTE ? a->worst > b->worst : a->worst < b->worst;
    return a->first < b->first;
  });
  for (size_t i = 0; i < others.size() && want.size() < K; ++i) want.push_back((uint32_t)others[i]->h);
  CHECK(n_chosen == want.size());
  uint64_t at = 0;
  for (size_t i = 0; i < want.size() && i < n_chosen; ++i) {
    CHECK(out.o.chosen[i] == want[i] && out.o.alt_off[i] == at);
    if (want[i] == 0xffffffffu) continue;
    for (auto& q : pos)
      if (q.h == want[i])
        for (uint32_t j : q.alts) { CHECK(at < n_alts && out.o.alt_group[at] == j); ++at; }
  }
  CHECK(n_alts == at && out.o.alt_off[n_chosen] == at);
  free(d_cs); free(d_ct);
}

static Panel positions_panel(uint32_t seed, int order_kind) {
  Panel p;
  std::vector<uint32_t> haps;
  for (uint32_t i = 0; i < 40; ++i) haps.push_back(p.hap({i}));
  std::vector<int> sizes{1, 2, 63, 64, 65};
  auto total = [&] { int t = 0; for (int s : sizes) t += s; return t; };
  while (total() + 3 <= 252) sizes.push_back(3);
  sizes.push_back(260 - total());
  while (total() + 3 <= 509) sizes.push_back(3);
  sizes.push_back(513 - total());
  uint32_t n = 0;
  for (size_t k = 0; k < sizes.size(); ++k) {
    int kind = (int)(k % 5);
    if (sizes[k] == 1) kind = k % 2 ? 2 : 0;
    const int ref_at = kind == 2 ? -1 : kind == 4 ? sizes[k] - 1 : 0;
    for (int j = 0; j < sizes[k]; ++j) {
      ++n;
      double sc = (lcg(seed) % 8) / 8.0 + (lcg(seed) % 5 == 0 ? 1e-5 : 0.0) + (lcg(seed) % 7 == 0 ? 0.00005 : 0.0);
      if (lcg(seed) % 20 == 0) sc = NAN;
      if (j == ref_at) p.group(1000 + 7 * (int64_t)(k / 2), k % 2, sc, {0}, 0, 0);
      else p.group(1000 + 7 * (int64_t)(k / 2), k % 2, sc, {haps[lcg(seed) % 40], haps[lcg(seed) % 40]}, 1ull << (n % 23), n);
    }
  }
  const size_t G = p.n();
  p.rank.resize(G);
  for (size_t g = 0; g < G; ++g) p.rank[g] = (uint32_t)(order_kind == 0 ? g : G - 1 - g);
  if (order_kind == 2)
    for (size_t g = G - 1; g > 0; --g) std::swap(p.rank[g], p.rank[lcg(seed) % (g + 1)]);
  return p;
}

static Panel samples_panel(uint32_t n_names) {
  Panel p;
  for (uint32_t i = 0; i < n_names; ++i) p.hap({i});  // row 1 + i names sample i
  const uint32_t three = p.hap({5, 6, 7}), b0 = p.hap({9}), b1 = p.hap({9});
  p.group(50, 0, 1.0, {0}, 0, 0);
  uint32_t n = 0;
  auto alt = [&](std::vector<uint32_t> m) { ++n; p.group(50, 0, 0.5, m, 1ull << (n % 23), n); };
  for (uint32_t size : {1u, 2u, 63u, 64u, 65u, 4097u, 16u, 17u}) {
    std::vector<uint32_t> m;
    for (uint32_t i = 0; i < size; ++i) m.push_back(100 + i);
    alt(m);
  }
  alt({1, 32, 33, 64, 65, n_names});
  alt({three}); alt({three, 6, 7}); alt({b0, b1}); alt({b0, b1, 10});
  p.rank.resize(p.n());
  for (size_t g = 0; g < p.n(); ++g) p.rank[g] = (uint32_t)g;
  return p;
}

int main() {
  {  // the rounding: the decimal text route, ties, their neighbours
    std::vector<double> x{0.03125, 0.09375, -0.03125, 0.0, -0.0, 1.0, 0.99995, 5e-5, 2.5e-5, 1e-300, 123456.78905, -1e-5};
    for (int k = 1; k < 4096; k += 2) { x.push_back(k / 4096.0); x.push_back(std::nextafter(k / 4096.0, 1.0)); x.push_back(std::nextafter(k / 4096.0, 0.0)); }
    for (int k = 0; k < 3000; ++k) x.push_back((2 * k + 1) / 20000.0);
    uint32_t s = 7;
    for (int k = 0; k < 20000; ++k) x.push_back(lcg(s) / 16777216.0);
    double* in = exact(x); double* out = room<double>(x.size());
    CHECK(hawk_host_round4(in, x.size(), out) == HAWK_OK);
    for (size_t i = 0; i < x.size(); ++i) {
      const double w = py_round4_slow(x[i]);
      if (memcmp(&w, &out[i], 8) != 0 && !(w == 0.0 && out[i] == 0.0)) { fprintf(stderr, "round4(%a) = %a, want %a\n", x[i], out[i], w); ++fails; }
    }
    double nan = NAN, r = 0;
    CHECK(hawk_host_round4(&nan, 1, &r) == HAWK_OK && std::isnan(r));
    free(in); free(out);
  }
  for (int order_kind = 0; order_kind < 3; ++order_kind) {
    const Panel p = positions_panel(11 + order_kind, order_kind);
    for (int family : {HAWK_FX_SIGNED, HAWK_FX_ABSOLUTE})
      for (uint32_t K : {1u, 25u, 64u}) check_panel(p, family, K, {});
    check_panel(p, HAWK_FX_SIGNED, 25, {{p.start[400], p.strand[400]}, {p.start[7], p.strand[7]}, {1, 0}});
    check_panel(p, HAWK_FX_ABSOLUTE, 64, {{p.start[200], p.strand[200]}});
  }
  {
    const Panel p = samples_panel(HAWK_FX_SAMPLE_CAP);
    check_panel(p, HAWK_FX_SIGNED, 25, {});
    Panel big = samples_panel(HAWK_FX_SAMPLE_CAP + 2);  // ids up to the cap + 1: refused, not miscounted
    Cols C(big);
    Out out(big.n(), 25, big.n());
    uint32_t nc; uint64_t na;
    CHECK(hawk_host_effects(&C.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 25, &out.o, big.n(), &nc, &na) == HAWK_E_UNSUPPORTED);
  }
  {  // zero groups; then the refusals
    Panel e;
    check_panel(e, HAWK_FX_SIGNED, 25, {});
    Panel p = positions_panel(3, 0);
    Cols C(p);
    Out out(p.n(), 64, p.n());
    uint32_t nc; uint64_t na;
    int64_t cs[2] = {1, 2}; uint8_t ct[2] = {0, 0};
    CHECK(hawk_host_effects(&C.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 0, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    CHECK(hawk_host_effects(&C.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 65, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    CHECK(hawk_host_effects(&C.c, HAWK_FX_SIGNED, nullptr, cs, ct, 2, 1, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    CHECK(hawk_host_effects(&C.c, 2, nullptr, nullptr, nullptr, 0, 25, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    CHECK(hawk_host_effects(&C.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 64, &out.o, 0, &nc, &na) == HAWK_E_CAPACITY && na > 0);
    Panel q = positions_panel(3, 0);
    q.rank[5] = q.rank[6];  // no permutation
    Cols Cq(q);
    CHECK(hawk_host_effects(&Cq.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 25, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    Panel u = positions_panel(3, 0);
    std::swap(u.start[0], u.start[300]);  // not in collapse order
    Cols Cu(u);
    CHECK(hawk_host_effects(&Cu.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 25, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    Panel m = positions_panel(3, 0);
    m.member_hap[10] = (uint32_t)m.hap_is_ref.size();  // a member row past the haplotype rows
    Cols Cm(m);
    CHECK(hawk_host_effects(&Cm.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 25, &out.o, p.n(), &nc, &na) == HAWK_E_INVALID);
    Panel w = positions_panel(3, 0);
    w.guidelen = 42;  // 42 + 3 + 20 bases fit no 64-bit window
    Cols Cw(w);
    CHECK(hawk_host_effects(&Cw.c, HAWK_FX_SIGNED, nullptr, nullptr, nullptr, 0, 25, &out.o, p.n(), &nc, &na) == HAWK_E_UNSUPPORTED);
  }
  if (fails) { fprintf(stderr, "effects_check: %d check(s) failed\n", fails); return 1; }
  printf("effects_check ok\n");
  return 0;
}
