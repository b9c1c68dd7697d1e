// uwin_check_main.cpp - hawk_host_unphased_windows (hawk_uwin.h through hawk_hostutil.hip) under the sanitizers, as a program of
// its own (make asan-uwin): the seam panel of the device tests - indels at offsets 100 / 131 / 132 / 133 and clamped at 0 / 1 / 31 /
// 32 / 33 / 99, indels within 100 of the region's end and a deletion whose ref ends on the last base, insertions of 1 / 31 / 32 /
// 33 / 64 / 100 and deletions of 1 / 31 / 32 / 33 / 64 bases, 1 / 63 / 64 / 65 / 129 carriers walked in a scrambled name order, SNVs
// everywhere in the windows (the anchor, the span, the tail a deletion's position map does not reach) - in heap buffers of exactly
// their size, checked against a plain walk over strings (the window cut out, the carrier's letters written where the position map
// reaches, the indel spliced in, equal strings of one indel merged first-seen); then forged signatures, the declines and the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hawk.h"
#include "hawk_uwin.h"

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

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}
static uint32_t base_of(char c) { return (uint32_t)(strchr("ACGT", c) - "ACGT"); }

struct Indel { uint32_t off, ref_len, alt_len; std::string ref, alt; };
struct Scene {
  std::string ref;
  uint32_t ns = 0, n_lines = 0;
  std::vector<uint32_t> v_off;            // SNVs, ascending; SNV j is record j, allele 1
  std::vector<uint8_t> v_mask, v_ref;
  std::vector<Indel> indels;              // indel k is record n_snv + k, allele 1
  std::vector<uint8_t> codes;
  std::vector<uint32_t> rank_sample;
  uint8_t& code(uint32_t line, uint32_t s, int c) { return codes[((size_t)line * ns + s) * 2 + c]; }
  bool carries(uint32_t line, uint32_t s) const { return codes[((size_t)line * ns + s) * 2] == 1 || codes[((size_t)line * ns + s) * 2 + 1] == 1; }
};

static Scene scene(uint32_t L, uint32_t ns, const std::vector<std::pair<uint32_t, int>>& indels /* offset, grow */, uint32_t snv_every, uint32_t carry_pct) {
  Scene s;
  s.ns = ns;
  for (uint32_t i = 0; i < L; ++i) s.ref.push_back("ACGT"[rnd(4)]);
  for (uint32_t o = rnd(snv_every); o < L; o += 1 + rnd(2 * snv_every)) {
    s.v_off.push_back(o); s.v_ref.push_back((uint8_t)base_of(s.ref[o])); s.v_mask.push_back((uint8_t)(1u << ((base_of(s.ref[o]) + 1 + rnd(3)) % 4)));
  }
  for (const auto& in : indels) {
    Indel d;
    d.off = in.first;
    if (in.second > 0) { d.ref = s.ref.substr(d.off, 1); d.alt = d.ref; for (int k = 0; k < in.second; ++k) d.alt.push_back("ACGT"[rnd(4)]); }
    else { d.ref = s.ref.substr(d.off, (size_t)(1 - in.second)); d.alt = d.ref.substr(0, 1); }
    d.ref_len = (uint32_t)d.ref.size(); d.alt_len = (uint32_t)d.alt.size();
    s.indels.push_back(d);
  }
  s.n_lines = (uint32_t)(s.v_off.size() + s.indels.size());
  s.codes.assign((size_t)s.n_lines * ns * 2, 0);
  for (uint32_t line = 0; line < s.n_lines; ++line)
    for (uint32_t smp = 0; smp < ns; ++smp) {
      if (rnd(100) >= carry_pct) continue;
      switch (rnd(4)) {
        case 0: s.code(line, smp, 1) = 1; break;
        case 1: s.code(line, smp, 0) = 1; break;
        case 2: s.code(line, smp, 0) = s.code(line, smp, 1) = 1; break;
        default: s.code(line, smp, 0) = 255; s.code(line, smp, 1) = 1; break;
      }
    }
  for (uint32_t r = 0; r < ns; ++r) s.rank_sample.push_back(r);
  for (uint32_t r = ns; r > 1; --r) std::swap(s.rank_sample[r - 1], s.rank_sample[rnd(r)]);  // names that do not sort in column order
  return s;
}

// the plain walk: per indel, per carrier in name order, the row as a string; equal strings of one indel merged, first seen first
struct Walked { std::vector<std::string> rows; std::vector<std::vector<uint32_t>> members; };
static Walked walk(const Scene& s) {
  static const char* low = "?acmgrsvtwyhkdbn";
  Walked w;
  const int64_t L = (int64_t)s.ref.size();
  for (uint32_t k = 0; k < s.indels.size(); ++k) {
    const Indel& d = s.indels[k];
    const int64_t grow = (int64_t)d.alt_len - d.ref_len, o = d.off;
    const int64_t a = std::max<int64_t>(0, o - 100), b = std::min<int64_t>(L - 1, o - grow + 100);
    const int64_t final_len = b - a + 1 + grow, span = grow > 0 ? 1 : 1 - grow;
    const size_t first = w.rows.size();
    for (uint32_t r = 0; r < s.ns; ++r) {
      const uint32_t smp = s.rank_sample[r];
      if (!s.carries((uint32_t)s.v_off.size() + k, smp)) continue;
      std::string win = s.ref.substr((size_t)a, (size_t)(b - a + 1));
      std::vector<uint32_t> bits(win.size(), 0);
      for (uint32_t j = 0; j < s.v_off.size(); ++j) {
        const int64_t p = (int64_t)s.v_off[j] - a;
        if (p < 0 || (int64_t)s.v_off[j] > b || !s.carries(j, smp) || p >= final_len) continue;  // outside, not carried, past the position map
        bits[p] |= (1u << s.v_ref[j]) | s.v_mask[j];
        win[p] = low[bits[p]];
      }
      std::string alt = d.alt;
      for (char& ch : alt) ch = (char)(ch | 0x20);
      const std::string row = win.substr(0, (size_t)(o - a)) + alt + win.substr((size_t)(o - a + span));
      size_t at = first;
      while (at < w.rows.size() && w.rows[at] != row) ++at;
      if (at == w.rows.size()) { w.rows.push_back(row); w.members.emplace_back(); }
      w.members[at].push_back(smp);
    }
  }
  return w;
}

struct Buffers {  // every input in a heap block of exactly its size
  hawk_uwin_input in;
  hawk_uwin_lists lists;
  std::vector<void*> held;
  template <class T> T* keep(T* p) { held.push_back((void*)p); return p; }
  ~Buffers() { for (void* p : held) free(p); }
};
static void fill(const Scene& s, Buffers* B) {
  std::vector<uint32_t> line, off, ref_len, alt_len, pool_off;
  std::vector<uint8_t> allele, pool;
  for (uint32_t k = 0; k < s.indels.size(); ++k) {
    const Indel& d = s.indels[k];
    line.push_back((uint32_t)s.v_off.size() + k); allele.push_back(1); off.push_back(d.off); ref_len.push_back(d.ref_len); alt_len.push_back(d.alt_len);
    pool_off.push_back((uint32_t)pool.size());
    for (char ch : d.ref + d.alt) pool.push_back((uint8_t)ub_base_index((uint8_t)ch));
  }
  std::vector<uint64_t> sample_off(1, 0);
  std::vector<uint32_t> idx;
  for (uint32_t smp = 0; smp < s.ns; ++smp) {
    for (uint32_t j = 0; j < s.v_off.size(); ++j)
      if (s.carries(j, smp)) idx.push_back(j);
    sample_off.push_back(idx.size());
  }
  std::vector<char> ref(s.ref.begin(), s.ref.end());
  hawk_uwin_input& in = B->in;
  in.n_indel = (uint32_t)s.indels.size(); in.region_len = (uint32_t)s.ref.size();
  in.line = B->keep(exact(line)); in.allele = B->keep(exact(allele)); in.off = B->keep(exact(off)); in.ref_len = B->keep(exact(ref_len));
  in.alt_len = B->keep(exact(alt_len)); in.pool_off = B->keep(exact(pool_off)); in.pool = B->keep(exact(pool)); in.pool_len = pool.size();
  in.rank_sample = B->keep(exact(s.rank_sample)); in.ref = B->keep(exact(ref));
  hawk_uwin_lists& l = B->lists;
  l.codes = B->keep(exact(s.codes)); l.n_lines = s.n_lines; l.n_samples = s.ns; l.n_var = (uint32_t)s.v_off.size();
  l.sample_off = B->keep(exact(sample_off)); l.list_idx = B->keep(exact(idx)); l.var_off = B->keep(exact(s.v_off));
  l.var_mask = B->keep(exact(s.v_mask)); l.var_ref = B->keep(exact(s.v_ref));
}

static void check_scene(const Scene& s, const char* name, bool forge) {
  const Walked want = walk(s);
  Buffers B;
  fill(s, &B);
  hawk_uwin_rows out;
  memset(&out, 0, sizeof(out));
  hawk_ubuild_decline dec;
  int rc = hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec);  // the counts
  CHECK(rc == HAWK_OK && dec.reason == 0);
  if (rc != HAWK_OK) { fprintf(stderr, "  scene %s: status %d reason %d\n", name, rc, dec.reason); return; }
  CHECK(out.n_rows == want.rows.size());
  uint64_t n_members = 0, n_seq = 0;
  for (const auto& m : want.members) n_members += m.size();
  for (const auto& r : want.rows) n_seq += r.size();
  CHECK(out.n_inst == n_members && out.n_seq == n_seq);
  const uint64_t ni = out.n_inst, nr = out.n_rows;
  std::vector<uint64_t> forged(2 * ni, 7);
  out.inst_cap = ni; out.row_cap = nr; out.seq_cap = out.n_seq;
  out.inst_off = room<uint64_t>(s.indels.size() + 1); out.inst_sample = room<uint32_t>(ni); out.inst_lo = room<uint64_t>(ni); out.inst_hi = room<uint64_t>(ni);
  out.sig = room<uint64_t>(2 * ni); out.head = room<uint32_t>(ni); out.seqs = room<char>(out.n_seq); out.seq_off = room<uint64_t>(nr + 1);
  uint64_t* fs = exact(forged);
  out.forged_sig = forge ? fs : nullptr;
  rc = hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec);
  CHECK(rc == HAWK_OK);
  if (rc == HAWK_OK && out.n_rows == want.rows.size() && out.n_inst == n_members) {
    uint64_t r = 0;
    std::vector<std::vector<uint32_t>> members(nr);
    std::vector<uint64_t> row_of(ni, 0);
    for (uint64_t k = 0; k < ni; ++k) {
      CHECK(out.head[k] <= k);
      if (out.head[k] == k) row_of[k] = r++;
      else row_of[k] = row_of[out.head[k]];
      members[row_of[k]].push_back(out.inst_sample[k]);
      CHECK(out.sig[2 * k] == out.sig[2 * out.head[k]] && out.sig[2 * k + 1] == out.sig[2 * out.head[k] + 1]);
    }
    CHECK(r == nr);
    for (uint64_t q = 0; q < nr; ++q) {
      CHECK(std::string(out.seqs + out.seq_off[q], out.seqs + out.seq_off[q + 1]) == want.rows[q]);
      CHECK(members[q] == want.members[q]);
    }
    if (fails) fprintf(stderr, "  scene %s\n", name);
  }
  // one element short: the capacity is checked before anything is written
  if (ni) { out.inst_cap = ni - 1; CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_CAPACITY); out.inst_cap = ni; }
  if (nr) { out.row_cap = nr - 1; CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_CAPACITY); out.row_cap = nr; }
  if (out.n_seq) { out.seq_cap = out.n_seq - 1; CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_CAPACITY); }
  free(out.inst_off); free(out.inst_sample); free(out.inst_lo); free(out.inst_hi); free(out.sig); free(out.head); free(out.seqs); free(out.seq_off); free(fs);
}

static void check_declines() {
  hawk_uwin_rows out;
  hawk_ubuild_decline dec;
  {  // an insertion longer than the flank; carried by nobody it is never looked at
    Scene s = scene(500, 3, {{250, 101}}, 20, 0);
    Buffers B; fill(s, &B); memset(&out, 0, sizeof(out));
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_OK && out.n_inst == 0);
    s.code((uint32_t)s.v_off.size(), 1, 0) = 1;
    Buffers C; fill(s, &C);
    CHECK(hawk_host_unphased_windows(&C.in, &C.lists, &out, &dec) == HAWK_E_UNSUPPORTED && dec.reason == UB_DECL_WINDOW && dec.var == 0);
  }
  {  // a base outside A/C/G/T in the alt
    Scene s = scene(500, 3, {{100, -2}, {250, 2}}, 20, 100);
    s.indels[1].alt[1] = 'N';
    Buffers B; fill(s, &B); memset(&out, 0, sizeof(out));
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_UNSUPPORTED && dec.reason == UB_DECL_INDEL_BASE && dec.var == 1);
  }
  {  // a deletion's ref that REF does not hold, with no SNV of the carrier there
    Scene s = scene(500, 2, {{250, -3}}, 1000, 100);
    s.v_off.clear(); s.v_mask.clear(); s.v_ref.clear();
    s.n_lines = 1; s.codes.assign((size_t)2 * 2, 1);
    s.indels[0].ref[2] = "ACGT"[(base_of(s.ref[252]) + 1) % 4];
    Buffers B; fill(s, &B); memset(&out, 0, sizeof(out));
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_UNSUPPORTED && dec.reason == UB_DECL_REF && dec.var == 0);
  }
  {  // a deletion that runs past the region; an indel whose two alleles are both longer than one base
    Scene s = scene(300, 2, {{295, -2}}, 30, 100);
    s.indels[0].ref_len = 9; s.indels[0].ref = s.ref.substr(295) + "ACGT";
    Buffers B; fill(s, &B); memset(&out, 0, sizeof(out));
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_UNSUPPORTED && dec.reason == UB_DECL_WINDOW);
    Scene t = scene(300, 2, {{100, -2}}, 30, 100);
    t.indels[0].alt += "A"; t.indels[0].alt_len = 2;
    Buffers C; fill(t, &C);
    CHECK(hawk_host_unphased_windows(&C.in, &C.lists, &out, &dec) == HAWK_E_UNSUPPORTED && dec.reason == UB_DECL_REF);
  }
  {  // refusals: a rank that is no sample, a rank twice, a record the block does not have, a pool range past the pool
    Scene s = scene(400, 4, {{200, 3}}, 20, 50);
    Buffers B; fill(s, &B); memset(&out, 0, sizeof(out));
    const_cast<uint32_t*>(B.in.rank_sample)[0] = 4;
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_INVALID);
    const_cast<uint32_t*>(B.in.rank_sample)[0] = B.in.rank_sample[1];
    CHECK(hawk_host_unphased_windows(&B.in, &B.lists, &out, &dec) == HAWK_E_INVALID);
    Buffers C; fill(s, &C);
    const_cast<uint32_t*>(C.in.line)[0] = s.n_lines;
    CHECK(hawk_host_unphased_windows(&C.in, &C.lists, &out, &dec) == HAWK_E_INVALID);
    Buffers D; fill(s, &D);
    D.in.pool_len -= 1;
    CHECK(hawk_host_unphased_windows(&D.in, &D.lists, &out, &dec) == HAWK_E_INVALID);
    CHECK(hawk_host_unphased_windows(nullptr, &D.lists, &out, &dec) == HAWK_E_INVALID);
  }
}

int main() {
  typedef std::vector<std::pair<uint32_t, int>> V;
  check_scene(scene(500, 3, V{{100, 2}, {131, -3}, {132, 4}, {133, -5}}, 12, 60), "starts", false);
  check_scene(scene(400, 3, V{{0, -1}, {1, 1}, {31, -3}, {32, 4}, {33, -5}, {99, 6}}, 9, 60), "clamped starts", false);
  check_scene(scene(600, 4, V{{594, -5}, {550, 7}, {500, -4}, {499, 2}, {598, 1}}, 9, 60), "right clamp", false);
  check_scene(scene(1300, 3, V{{120, 1}, {310, 31}, {500, 32}, {690, 33}, {880, 64}, {1070, 100}}, 15, 70), "insertions", false);
  check_scene(scene(1300, 3, V{{120, -1}, {350, -31}, {580, -32}, {810, -33}, {1040, -64}}, 7, 70), "deletions", false);
  check_scene(scene(400, 3, V{{26, 1}, {27, 1}, {28, 1}, {58, 1}, {59, 1}, {60, 1}, {300, -3}}, 11, 60), "row lengths", false);
  for (uint32_t ns : {1u, 63u, 64u, 65u, 129u}) {
    check_scene(scene(500, ns, V{{250, -2}}, 25, 100), "every sample carries", false);
    check_scene(scene(500, ns, V{{250, 3}, {260, -6}}, 6, 45), "carriers", ns == 65u);
  }
  check_scene(scene(700, 12, V{{300, -6}}, 2, 50), "dense SNVs around a deletion", false);
  check_scene(scene(700, 12, V{{300, 5}}, 2, 50), "dense SNVs around an insertion", true);
  check_scene(scene(300, 5, V{}, 10, 50), "no indel", false);
  check_scene(scene(300, 5, V{{100, 2}, {150, -2}}, 1000, 50), "no SNV", true);
  for (int round = 0; round < 40; ++round) {
    V v;
    const uint32_t L = 250 + rnd(900);
    for (uint32_t k = 0, n = 1 + rnd(5); k < n; ++k) {
      const int grow = rnd(2) ? (int)(1 + rnd(40)) : -(int)(1 + rnd(40));
      v.push_back({rnd(L - 45), grow});  // (a deletion of 40 bases still ends inside the region)
    }
    check_scene(scene(L, 1 + rnd(70), v, 3 + rnd(20), 20 + rnd(80)), "random", round % 3 == 0);
  }
  check_declines();
  if (fails) { fprintf(stderr, "uwin_check: %d failures\n", fails); return 1; }
  printf("uwin_check: ok\n");
  return 0;
}
