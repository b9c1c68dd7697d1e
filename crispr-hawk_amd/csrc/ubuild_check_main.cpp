// ubuild_check_main.cpp - hawk_host_unphased_rows (hawk_ubuild.h through hawk_hostutil.hip) under the sanitizers, as a program of
// its own (make asan-ubuild): the seam panel of the device tests - SNVs at offsets 0, 31, 32, 33, L - 1 and in the last word, L =
// 32k - 1 / 32k / 32k + 1 and L = 960, several alts at one position, 1 / 63 / 64 / 65 / 129 samples, 0 / 1 / 63 / 64 / 65 / 256 /
// 257 variants, samples without an SNV between carriers, equal rows that are not adjacent, all rows equal - in heap buffers of
// exactly their size, checked against a plain walk over strings (one string per carrier, the letters merged one record after the
// other, equal strings merged first-seen); then ub_gt_classify on the genotype forms, the declines and the refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/hawk.h"
#include "hawk_ubuild.h"

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

struct Scene {
  std::string ref;
  uint32_t ns = 0;
  std::vector<uint32_t> line, off;
  std::vector<uint8_t> allele, mask, refb, codes;  // codes[n_lines][2 * ns]; one line per variant here, allele 1 or 2
  uint32_t n_lines = 0;
  void variant(uint32_t o, uint32_t alt_k, uint8_t al = 1) {  // the alt is the alt_k-th base after REF's
    const uint32_t r = (uint32_t)(strchr("ACGT", ref[o]) - "ACGT");
    line.push_back(n_lines++); off.push_back(o); allele.push_back(al); refb.push_back((uint8_t)r); mask.push_back((uint8_t)(1u << ((r + alt_k) % 4u)));
    codes.resize((size_t)n_lines * 2 * ns, 0);
  }
  void gt(uint32_t var, uint32_t s, uint8_t a, uint8_t b) { codes[((size_t)line[var] * ns + s) * 2] = a; codes[((size_t)line[var] * ns + s) * 2 + 1] = b; }
  void sort() {  // by offset, stable, as the caller's variant table is
    std::vector<uint32_t> o(off.size());
    for (uint32_t i = 0; i < o.size(); ++i) o[i] = i;
    std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return off[a] < off[b]; });
    auto pick = [&](auto& v) { auto w = v; for (uint32_t i = 0; i < o.size(); ++i) v[i] = w[o[i]]; };
    pick(line); pick(off); pick(allele); pick(mask); pick(refb);
  }
};

static Scene make(uint32_t L, uint32_t ns, uint32_t nv, uint32_t density_pct, bool seams) {
  Scene s;
  s.ns = ns;
  for (uint32_t i = 0; i < L; ++i) s.ref.push_back("ACGT"[rnd(4)]);
  std::vector<uint32_t> offs;
  if (seams)
    for (uint32_t o : {0u, 31u, 32u, 33u, 32u * ((L + 31u) / 32u - 1u), L - 1u}) offs.push_back(o);
  while (offs.size() < nv) offs.push_back(rnd(L));
  offs.resize(nv);
  for (uint32_t v = 0; v < nv; ++v) s.variant(offs[v], 1 + rnd(3), (uint8_t)(1 + rnd(2)));
  for (uint32_t v = 0; v < nv; ++v)
    for (uint32_t smp = 0; smp < ns; ++smp) {
      if (rnd(100) >= density_pct) { if (rnd(4) == 0) s.gt(v, smp, 255, 0); continue; }
      const uint8_t al = s.allele[v];
      switch (rnd(4)) {
        case 0: s.gt(v, smp, 0, al); break;
        case 1: s.gt(v, smp, al, 0); break;
        case 2: s.gt(v, smp, al, al); break;
        default: s.gt(v, smp, 255, al); break;
      }
    }
  s.sort();
  return s;
}

// the plain walk: one string per carrier; nullptr when some sample carries an alt that is already in its letter
static bool walk(const Scene& s, std::vector<std::string>* rows, std::vector<std::vector<uint32_t>>* members) {
  static const char* up = "?ACMGRSVTWYHKDBN";
  std::vector<std::string> seen;
  for (uint32_t smp = 0; smp < s.ns; ++smp) {
    std::string row = s.ref;
    std::vector<uint32_t> bits(s.ref.size(), 0);
    bool any = false;
    for (uint32_t v = 0; v < s.off.size(); ++v) {
      const uint8_t* c = &s.codes[((size_t)s.line[v] * s.ns + smp) * 2];
      if (c[0] != s.allele[v] && c[1] != s.allele[v]) continue;
      any = true;
      const uint32_t o = s.off[v], r = 1u << s.refb[v];
      if (!bits[o]) bits[o] = r;
      if ((bits[o] & s.mask[v]) && !(bits[o] == r && s.mask[v] == r)) return false;
      bits[o] |= s.mask[v];
      row[o] = (char)(up[bits[o]] | 0x20);
    }
    if (!any) continue;
    size_t k = std::find(seen.begin(), seen.end(), row) - seen.begin();
    if (k == seen.size()) { seen.push_back(row); members->emplace_back(); }
    (*members)[k].push_back(smp);
  }
  *rows = seen;
  return true;
}

static int run(const Scene& s, hawk_ubuild_rows* out, hawk_ubuild_decline* dec, uint8_t* codes, uint32_t* line, uint8_t* allele, uint32_t* off,
               uint8_t* mask, uint8_t* refb, char* ref) {
  hawk_ubuild_input in;
  in.codes = codes; in.n_lines = s.n_lines; in.n_samples = s.ns; in.n_var = (uint32_t)s.off.size();
  in.var_line = line; in.var_allele = allele; in.var_off = off; in.var_mask = mask; in.var_ref = refb;
  in.ref = ref; in.ref_len = (uint32_t)s.ref.size(); in.row_base = 1;
  return hawk_host_unphased_rows(&in, out, dec);
}

static void check_scene(const Scene& s, const char* name) {
  uint8_t* codes = exact(s.codes); uint32_t* line = exact(s.line); uint8_t* allele = exact(s.allele); uint32_t* off = exact(s.off);
  uint8_t* mask = exact(s.mask); uint8_t* refb = exact(s.refb);
  std::vector<char> refv(s.ref.begin(), s.ref.end());
  char* ref = exact(refv);
  std::vector<std::string> rows;
  std::vector<std::vector<uint32_t>> members;
  const bool fine = walk(s, &rows, &members);
  hawk_ubuild_rows out;
  memset(&out, 0, sizeof(out));
  hawk_ubuild_decline dec;
  int rc = run(s, &out, &dec, codes, line, allele, off, mask, refb, ref);
  if (!fine) {
    CHECK(rc == HAWK_E_UNSUPPORTED && dec.reason == HAWK_UBUILD_REPEAT && dec.var >= 0);
  } else {
    CHECK(rc == HAWK_OK && dec.reason == 0);
    CHECK(out.n_rows == rows.size());
    if (rc == HAWK_OK && out.n_rows == rows.size()) {
      const uint64_t L = s.ref.size(), nr = out.n_rows;
      // the allele entries of the first members: exactly that many
      out.row_cap = nr; out.entry_cap = out.n_entries;
      out.seqs = room<char>(nr * L); out.member_off = room<uint32_t>(nr + 1); out.member_sample = room<uint32_t>(out.n_members);
      out.sample_off = room<uint64_t>((size_t)s.ns + 1); out.list_idx = room<uint32_t>(out.n_entries); out.sig = room<uint64_t>((size_t)s.ns * 2);
      rc = run(s, &out, &dec, codes, line, allele, off, mask, refb, ref);
      CHECK(rc == HAWK_OK);
      uint64_t n_al = 0;
      for (uint64_t k = 0; k < nr && rc == HAWK_OK; ++k) {
        CHECK(std::string(out.seqs + k * L, L) == rows[k]);
        CHECK(out.member_off[k + 1] - out.member_off[k] == members[k].size());
        for (size_t m = 0; m < members[k].size(); ++m) CHECK(out.member_sample[out.member_off[k] + m] == members[k][m]);
        const uint32_t h = members[k][0];
        n_al += out.sample_off[h + 1] - out.sample_off[h];
      }
      for (uint32_t smp = 0; smp < s.ns && rc == HAWK_OK; ++smp)
        for (uint64_t e = out.sample_off[smp]; e + 1 < out.sample_off[smp + 1]; ++e) CHECK(out.list_idx[e] < out.list_idx[e + 1]);
      hawk_ubuild_rows al;
      memset(&al, 0, sizeof(al));
      al.entry_cap = n_al;
      al.al_key = room<uint64_t>(out.n_keys); al.al_off = room<uint32_t>(out.n_keys + 1); al.al_ref = room<uint8_t>(n_al);
      rc = run(s, &al, &dec, codes, line, allele, off, mask, refb, ref);
      CHECK(rc == HAWK_OK && al.n_keys == out.n_keys);
      uint64_t ki = 0;
      for (uint64_t k = 0; k < nr && rc == HAWK_OK; ++k)   // one key per lower-case letter of the row, ascending
        for (uint64_t p = 0; p < L; ++p)
          if (rows[k][p] >= 'a') {
            CHECK(ki < al.n_keys && al.al_key[ki] == (((uint64_t)(1 + k) << 32) | p));
            if (ki < al.n_keys) {
              CHECK(al.al_off[ki + 1] > al.al_off[ki]);
              for (uint32_t e = al.al_off[ki]; e < al.al_off[ki + 1]; ++e) CHECK("ACGT"[al.al_ref[e]] == s.ref[p]);
            }
            ++ki;
          }
      CHECK(ki == al.n_keys && (al.n_keys == 0 || al.al_off[al.n_keys] == n_al));
      if (n_al) {  // one entry too few: refused, nothing written past the buffers
        al.entry_cap = n_al - 1;
        CHECK(run(s, &al, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_CAPACITY);
      }
      free(al.al_key); free(al.al_off); free(al.al_ref);
      free(out.seqs); free(out.member_off); free(out.member_sample); free(out.sample_off); free(out.list_idx); free(out.sig);
    }
  }
  if (fails) fprintf(stderr, "  (scene %s)\n", name);
  free(codes); free(line); free(allele); free(off); free(mask); free(refb); free(ref);
}

static uint32_t classify(const char* g) {
  std::vector<uint8_t> t(g, g + strlen(g));
  uint8_t* p = exact(t);
  const uint32_t r = ub_gt_classify(p, 0, t.size());
  free(p);
  return r;
}

int main() {
  // ---- the genotype rule: flags | code0 << 8 | code1 << 16
  CHECK(classify("0/1") == (0u | 0u << 8 | 1u << 16) && classify("1/0") == (1u << 8) && classify("./1") == (255u << 8 | 1u << 16));
  CHECK(classify("1/.") == (1u << 8 | 255u << 16) && classify("./.") == (255u << 8 | 255u << 16) && classify("10/2:35") == (10u << 8 | 2u << 16));
  CHECK(classify("0/300") == (254u << 16) && classify("0/1:a/b|c") == (1u << 16));
  CHECK((classify("1") & 0xff) == 1 && (classify("0/1/1") & 0xff) == 1 && (classify("0|1") & 0xff) == 5 && (classify("0/1|2") & 0xff) == 5);
  CHECK((classify("") & 0xff) == 5 && (classify("a/1") & 0xff) == 4 && (classify("/1") & 0xff) == 4 && (classify("0/1/1") >> 8) == (0u | 1u << 8));
  // ---- the seam panel
  char name[64];
  for (uint32_t L : {959u, 960u, 1023u, 1024u, 1025u})
    for (uint32_t ns : {1u, 3u}) {
      snprintf(name, sizeof name, "seams L=%u ns=%u", L, ns);
      check_scene(make(L, ns, 12, 60, true), name);
    }
  for (uint32_t ns : {63u, 64u, 65u, 129u}) { snprintf(name, sizeof name, "samples %u", ns); check_scene(make(500, ns, 9, 30, false), name); }
  for (uint32_t nv : {0u, 1u, 63u, 64u, 65u, 256u, 257u}) { snprintf(name, sizeof name, "variants %u", nv); check_scene(make(1300, 4, nv, 50, false), name); }
  for (int rep = 0; rep < 40; ++rep) { snprintf(name, sizeof name, "dense %d", rep); check_scene(make(64 + rnd(40), 1 + rnd(9), 30 + rnd(60), 40, false), name); }
  {  // equal rows that are not adjacent, samples without an SNV between them, then all rows equal
    Scene s;
    s.ns = 7; s.ref = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT";
    s.variant(3, 1); s.variant(32, 2); s.variant(39, 3);
    for (uint32_t smp : {0u, 2u, 5u}) { s.gt(0, smp, 0, 1); s.gt(1, smp, 1, 1); }
    s.gt(2, 3, 255, 1); s.gt(2, 6, 1, 0);
    check_scene(s, "equal rows");
    Scene t = s;
    for (uint32_t smp = 0; smp < t.ns; ++smp) { t.gt(0, smp, 0, 1); t.gt(1, smp, 0, 0); t.gt(2, smp, 0, 0); }
    check_scene(t, "all equal");
  }
  // ---- declines and refusals
  {
    Scene s;
    s.ns = 2; s.ref = "ACGTACGTAC";
    s.variant(4, 1); s.variant(9, 1);
    s.gt(0, 0, 0, 1); s.gt(1, 1, 1, 1);
    hawk_ubuild_rows out;
    hawk_ubuild_decline dec;
    uint8_t* codes = exact(s.codes); uint32_t* line = exact(s.line); uint8_t* allele = exact(s.allele); uint32_t* off = exact(s.off);
    uint8_t* mask = exact(s.mask); uint8_t* refb = exact(s.refb);
    std::vector<char> refv(s.ref.begin(), s.ref.end());
    char* ref = exact(refv);
    memset(&out, 0, sizeof(out));
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_OK && out.n_rows == 2 && out.n_keys == 2);
    off[1] = 10;   // one past REF's end
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_UNSUPPORTED && dec.reason == HAWK_UBUILD_OUTSIDE && dec.var == 1);
    off[1] = 9; refb[1] = 0;   // REF holds C there
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_UNSUPPORTED && dec.reason == HAWK_UBUILD_REF && dec.var == 1);
    codes[(1 * 2 + 1) * 2] = 0; codes[(1 * 2 + 1) * 2 + 1] = 0;   // nobody carries it: not looked at
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_OK && out.n_rows == 1);
    refb[1] = 4;
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_INVALID);
    refb[1] = 1; off[1] = 3;   // offsets that descend
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_INVALID);
    off[1] = 9; line[1] = 2;
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_INVALID);
    line[1] = 1;
    out.seqs = room<char>(1);   // a buffer without its capacity
    out.row_cap = 0;
    CHECK(run(s, &out, &dec, codes, line, allele, off, mask, refb, ref) == HAWK_E_CAPACITY);
    free(out.seqs);
    CHECK(hawk_host_unphased_rows(nullptr, &out, &dec) == HAWK_E_INVALID);
    free(codes); free(line); free(allele); free(off); free(mask); free(refb); free(ref);
  }
  if (fails) { fprintf(stderr, "ubuild_check: %d check(s) failed\n", fails); return 1; }
  printf("ubuild_check: ok\n");
  return 0;
}
