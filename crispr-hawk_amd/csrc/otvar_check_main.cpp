// otvar_check_main.cpp - hawk_host_offtarget_variant_scan (hawk_hostutil.hip, through ov_resolve of hawk_otvar.h) as the host
// compiler builds it, held to a plain restatement on letters.  `make asan-otvar` compiles this file and hawk_hostutil.hip with
// -fsanitize=address,undefined and runs it.  Not part of the library, nothing here is loaded into Python.
// The restatement knows no bit mask: per position a REF letter and a set of letters; a window is cut out of them, turned into
// guide orientation letter by letter, and resolved against the guide's letters by the rules of include/hawk.h.
//   placed   an ALT that creates the GG of NGG; an ALT under the N of NGG alone (no row); an ALT that removes the one mismatch
//            too many; an ALT no guide carries; two ALTs at one position; variants on an N, with a wrong REF, with ALT = REF
//   random   400 genomes of 150 .. 400 letters (N sprinkled in) in one to three rows, SNVs at one per ~12 bases, 6 guides planted
//            near windows, NGG / 20, TTTV / 23 in front, TTTV / 28 in front (32 bases: every bit of the masks and the code) and
//            NG / 6 (8 bases), max_mm 0 .. 4, output buffers of exactly the rows' number
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/hawk.h"

namespace {
const char* ACGT = "ACGT";
int base_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
std::string iupac_set(char c) {
  switch (c) {
    case 'A': return "A"; case 'C': return "C"; case 'G': return "G"; case 'T': return "T"; case 'N': return "ACGT";
    case 'R': return "AG"; case 'Y': return "CT"; case 'S': return "CG"; case 'W': return "AT"; case 'K': return "GT";
    case 'M': return "AC"; case 'B': return "CGT"; case 'D': return "AGT"; case 'H': return "ACT"; case 'V': return "ACG";
  }
  return "";
}
bool in(const std::string& s, char c) { return s.find(c) != std::string::npos; }

struct Var { uint32_t row, q; char ref, alt; };
// guide, row, q, strand, mm, resolved window, alt mask
typedef std::tuple<uint32_t, uint32_t, uint32_t, int, int, std::string, uint32_t> Row;

struct Case {
  std::vector<std::string> rows;
  std::vector<std::pair<int, int>> own;  // window starts each row owns
  std::vector<Var> vars;
  std::vector<std::string> guides;
  std::string pam;
  bool right;
  int max_mm;
};

std::vector<Row> restate(const Case& c, std::vector<int>* status) {
  const int G = (int)c.guides[0].size(), P = (int)c.pam.size(), L = G + P;
  std::vector<std::vector<std::string>> sets(c.rows.size());
  for (size_t h = 0; h < c.rows.size(); ++h)
    for (char ch : c.rows[h]) sets[h].push_back(base_of(ch) >= 0 ? std::string(1, ch) : std::string());
  for (const Var& v : c.vars) {
    const char r = c.rows[v.row][v.q];
    int st = 0;
    if (base_of(r) < 0) st = 1;
    else if (r != v.ref) st = 2;
    else if (v.alt == v.ref) st = 3;
    else if (!in(sets[v.row][v.q], v.alt)) sets[v.row][v.q] += v.alt;
    status->push_back(st);
  }
  std::vector<Row> out;
  for (size_t h = 0; h < c.rows.size(); ++h)
    for (int q = c.own[h].first; q < c.own[h].second; ++q)
      for (int s = 0; s < 2; ++s) {
        std::string ref(L, 'N');
        std::vector<std::string> al(L);
        for (int i = 0; i < L; ++i) {
          const int at = q + (s ? L - 1 - i : i);
          const char r = c.rows[h][at];
          ref[i] = base_of(r) < 0 ? 'N' : (s ? comp(r) : r);
          for (char a : sets[h][at]) al[i] += s ? comp(a) : a;
        }
        for (size_t gi = 0; gi < c.guides.size(); ++gi) {
          std::string res = ref;
          uint32_t alt = 0;
          int mm = 0;
          bool ok = true;
          for (int k = 0; k < P; ++k) {
            const int i = (c.right ? 0 : G) + k;
            if (c.pam[k] == 'N') continue;
            const std::string ps = iupac_set(c.pam[k]);
            std::string both;
            for (const char* b = ACGT; *b; ++b)
              if (in(ps, *b) && in(al[i], *b)) both += *b;
            if (both.empty()) { ok = false; break; }
            if (ref[i] != 'N' && in(ps, ref[i])) continue;
            res[i] = both[0];
            alt |= 1u << i;
          }
          if (!ok) continue;
          for (int j = 0; j < G; ++j) {
            const int i = (c.right ? P : 0) + j;
            const char g = c.guides[gi][j];
            if (in(al[i], g)) { res[i] = g; if (g != ref[i]) alt |= 1u << i; }
            else ++mm;
          }
          if (mm <= c.max_mm && alt) out.emplace_back((uint32_t)gi, (uint32_t)h, (uint32_t)q, s, mm, res, alt);
        }
      }
  return out;
}

uint64_t pam_bits(const std::string& pam) {
  uint64_t v = 0;
  for (char ch : pam) {
    uint64_t nib = 0;
    for (char b : iupac_set(ch)) nib |= 1ull << base_of(b);
    v = (v << 4) | nib;
  }
  return v;
}

int run(const Case& c, const char* name) {
  const int G = (int)c.guides[0].size(), P = (int)c.pam.size(), L = G + P;
  std::vector<int> want_st;
  std::vector<Row> want = restate(c, &want_st);
  std::sort(want.begin(), want.end());
  std::string blob;
  std::vector<uint64_t> off(1, 0);
  std::vector<int32_t> ss, se;
  for (size_t h = 0; h < c.rows.size(); ++h) {
    blob += c.rows[h];
    off.push_back(blob.size());
    ss.push_back(c.own[h].first);
    se.push_back(c.own[h].second);
  }
  std::vector<uint32_t> vr, vq;
  std::vector<uint8_t> vref, valt;
  for (const Var& v : c.vars) { vr.push_back(v.row); vq.push_back(v.q); vref.push_back((uint8_t)base_of(v.ref)); valt.push_back((uint8_t)base_of(v.alt)); }
  std::vector<uint8_t> vst(c.vars.size());
  std::vector<uint64_t> g2;
  for (const std::string& g : c.guides) {
    uint64_t v = 0;
    for (int j = 0; j < G; ++j) v |= (uint64_t)base_of(g[j]) << (2 * j);
    g2.push_back(v);
  }
  hawk_ot_params par = {pam_bits(c.pam), 0, (uint32_t)P, (uint32_t)G, c.right ? 1u : 0u, (uint32_t)c.max_mm};
  uint64_t n = 0;
  auto call = [&](uint64_t cap, uint32_t* og, uint32_t* orow, uint32_t* oq, uint8_t* os, uint8_t* om, uint64_t* oc, uint32_t* on, uint32_t* oa) {
    return hawk_host_offtarget_variant_scan(blob.data(), off.data(), (uint32_t)c.rows.size(), ss.data(), se.data(), vr.data(), vq.data(), vref.data(),
                                            valt.data(), c.vars.size(), vst.data(), &par, g2.data(), (uint32_t)g2.size(), og, orow, oq, os, om, oc, on,
                                            oa, cap, &n);
  };
  int rc = call(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc != (want.empty() ? HAWK_OK : HAWK_E_CAPACITY) || n != want.size()) {
    fprintf(stderr, "%s: count pass: status %d, %" PRIu64 " rows, want %zu\n", name, rc, n, want.size());
    return 1;
  }
  for (size_t i = 0; i < vst.size(); ++i)
    if (vst[i] != want_st[i]) { fprintf(stderr, "%s: variant %zu: status %d, want %d\n", name, i, vst[i], want_st[i]); return 1; }
  // buffers of exactly the rows' number: a write past them is the sanitizer's to find
  std::vector<uint32_t> og(n), orow(n), oq(n), on(n), oa(n);
  std::vector<uint8_t> os(n), om(n);
  std::vector<uint64_t> oc(n);
  rc = call(n, og.data(), orow.data(), oq.data(), os.data(), om.data(), oc.data(), on.data(), oa.data());
  if (rc != HAWK_OK) { fprintf(stderr, "%s: fill pass: status %d\n", name, rc); return 1; }
  std::vector<Row> got;
  for (uint64_t i = 0; i < n; ++i) {
    std::string w(L, 'N');
    for (int k = 0; k < L; ++k)
      if (!((on[i] >> k) & 1u)) w[k] = ACGT[(oc[i] >> (2 * k)) & 3u];
    got.emplace_back(og[i], orow[i], oq[i], (int)os[i], (int)om[i], w, oa[i]);
  }
  std::sort(got.begin(), got.end());
  if (got != want) {
    for (size_t i = 0; i < got.size(); ++i)
      if (got[i] != want[i]) {
        fprintf(stderr, "%s: row %zu: guide %u row %u q %u strand %d mm %d %s alt %x, want guide %u row %u q %u strand %d mm %d %s alt %x\n", name, i,
                std::get<0>(got[i]), std::get<1>(got[i]), std::get<2>(got[i]), std::get<3>(got[i]), std::get<4>(got[i]), std::get<5>(got[i]).c_str(),
                std::get<6>(got[i]), std::get<0>(want[i]), std::get<1>(want[i]), std::get<2>(want[i]), std::get<3>(want[i]), std::get<4>(want[i]),
                std::get<5>(want[i]).c_str(), std::get<6>(want[i]));
        break;
      }
    return 1;
  }
  return 0;
}

Case one_row(const std::string& genome, std::vector<Var> vars, std::vector<std::string> guides, const std::string& pam, bool right, int max_mm) {
  Case c;
  const int L = (int)(guides[0].size() + pam.size());
  c.rows = {genome};
  c.own = {{0, std::max(0, (int)genome.size() - L + 1)}};
  c.vars = std::move(vars); c.guides = std::move(guides); c.pam = pam; c.right = right; c.max_mm = max_mm;
  return c;
}
}  // namespace

int main() {
  int bad = 0;
  const std::string g20 = "ACGTTGCAAGCTTAGGCTAA", pad = "TTTTTTTTTT";
  // the built-in case: guide + AGA; an ALT G at the last base makes AGG, the middle base lies under the N of NGG
  {
    const std::string genome = pad + g20 + "AGA" + pad;
    const uint32_t at = (uint32_t)(pad.size() + g20.size());
    std::vector<Row> dummy;
    Case c = one_row(genome, {{0, at + 2, 'A', 'G'}}, {g20}, "NGG", false, 0);
    std::vector<int> st;
    const std::vector<Row> want = restate(c, &st);
    if (want.size() != 1 || std::get<2>(want[0]) != pad.size() || std::get<6>(want[0]) != (1u << 22)) { fprintf(stderr, "restatement: the PAM-creating ALT\n"); ++bad; }
    bad += run(c, "alt creates the PAM");
    c = one_row(genome, {{0, at + 1, 'G', 'C'}}, {g20}, "NGG", false, 0);  // under the N only: REF stays, AGA is no PAM
    bad += run(c, "alt under the PAM's N");
    std::string g1 = genome;
    g1[at + 2] = 'G';  // a REF PAM, and one spacer mismatch an ALT removes
    g1[pad.size() + 5] = 'A';
    c = one_row(g1, {{0, (uint32_t)pad.size() + 5, 'A', 'G'}, {0, (uint32_t)pad.size() + 5, 'A', 'T'}, {0, (uint32_t)pad.size() + 7, 'A', 'C'}}, {g20}, "NGG", false, 0);
    bad += run(c, "alt removes the mismatch; two ALTs at one position; an ALT no guide carries");
    std::string g2 = g1;
    g2[pad.size() + 9] = 'N';
    c = one_row(g2, {{0, (uint32_t)pad.size() + 9, 'G', 'C'}, {0, (uint32_t)pad.size() + 8, 'C', 'T'}, {0, (uint32_t)pad.size() + 10, 'C', 'C'},
                     {0, (uint32_t)pad.size() + 5, 'A', 'G'}}, {g20}, "NGG", false, 2);
    bad += run(c, "variants on an N, with a wrong REF, with ALT = REF");
  }
  std::mt19937_64 rng(20240611);
  static const struct { const char* pam; int G; bool right; } systems[4] = {{"NGG", 20, false}, {"TTTV", 23, true}, {"TTTV", 28, true}, {"NG", 6, false}};
  for (int it = 0; it < 400; ++it) {
    const bool cpf = systems[it & 3].right;
    const std::string pam = systems[it & 3].pam;
    const int G = systems[it & 3].G, L = G + (int)pam.size();
    Case c;
    c.pam = pam; c.right = cpf; c.max_mm = (int)(rng() % 5);
    const int n_rows = 1 + (int)(rng() % 3);
    for (int h = 0; h < n_rows; ++h) {
      const int len = 150 + (int)(rng() % 251);
      std::string s(len, 'A');
      for (char& ch : s) ch = rng() % 40 == 0 ? 'N' : ACGT[rng() % 4];
      c.rows.push_back(s);
      c.own.push_back({(int)(rng() % 5), len - L + 1 - (int)(rng() % 5)});
    }
    for (int g = 0; g < 6; ++g) {  // guides cut out of the rows (either strand) and spoiled in up to three places
      const std::string& s = c.rows[rng() % n_rows];
      const int q = (int)(rng() % (s.size() - L));
      std::string w = s.substr(q + (cpf ? (int)pam.size() : 0), G);
      if (rng() & 1) { std::reverse(w.begin(), w.end()); for (char& ch : w) ch = comp(ch); }
      for (char& ch : w) if (base_of(ch) < 0) ch = 'A';
      for (int k = (int)(rng() % 4); k > 0; --k) w[rng() % G] = ACGT[rng() % 4];
      c.guides.push_back(w);
    }
    for (int h = 0; h < n_rows; ++h)
      for (uint32_t q = 0; q < c.rows[h].size(); ++q)
        if (rng() % 12 == 0) {
          const char r = c.rows[h][q];
          const char ref = rng() % 10 == 0 ? ACGT[rng() % 4] : (base_of(r) < 0 ? 'A' : r);
          c.vars.push_back({(uint32_t)h, q, ref, ACGT[rng() % 4]});
        }
    char name[32];
    snprintf(name, sizeof(name), "random %d", it);
    bad += run(c, name);
  }
  if (bad) { fprintf(stderr, "otvar_check: %d case(s) failed\n", bad); return 1; }
  printf("otvar_check: ok\n");
  return 0;
}
