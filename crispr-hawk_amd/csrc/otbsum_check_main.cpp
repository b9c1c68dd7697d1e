// otbsum_check_main.cpp - otb_pair (hawk_otbulge.h: the row a bulged (site, guide) pair makes - mismatches, gaps, CFD units) and
// hawk_host_offtarget_bulge_summary (hawk_hostutil.hip: its sums) as the host compiler builds them, held to a plain restatement on
// letters.  `make asan-otbsum` compiles this file and hawk_hostutil.hip with -fsanitize=address,undefined and runs it.  Not part
// of the library, nothing here is loaded into Python.
// The restatement knows no shift vector and no record: it walks every placement of the gaps in ascending order of the gap tuple,
// counts the mismatches of the aligned letters ("strictly smaller wins"; an N of the site mismatches, an N is never bulged out of
// the site), writes the winner's two aligned strings and takes the CFD on them - a left-to-right product over the first 20
// columns where the letters differ and neither is '-', times the entry of the last two characters of site + PAM (PAM + site when
// the PAM stands in front).  Rounding to 1e-4 units alone is shared (ot_round_e4, which tests/test_offtarget_summary_host.py holds
// to Python's round).
//   exhaustive  b = 1: G = 4 and 5, b = 2: G = 5 and 6, DNA and RNA, every site over a small alphabet with N against every guide
//               over a smaller one, max_mm in {0, 1, G}.  Exhaustive in (site, guide) only: PAM behind / in front, the site's PAM
//               and tables / no tables are dealt out by the pair's index, one combination per pair; the random pass draws them freely
//   random      2 x 10^5 planted pairs at G = 20 .. 29 with windows of up to 32 bases, N anywhere, max_mm 0 .. 6 and G
//   sums        the host twin over 300 sites x 7 guides per kind against the restatement's sums, buffers of exactly their size
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/hawk.h"
#include "hawk_otbulge.h"

namespace {
int base_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

struct Row { bool any; int mm; uint32_t gaps; long long units; };

// site: the site's spacer (Gs letters of ACGTN), pam: the site's own PAM (P letters), guide: G letters of ACGT
Row restate(const std::string& site, const std::string& pam, const std::string& guide, bool right, int b, bool dna, int max_mm, const double* tab) {
  const int G = (int)guide.size(), Gs = (int)site.size(), span = dna ? Gs : G;
  const std::string& longer = dna ? site : guide;
  const std::string& shorter = dna ? guide : site;
  Row best = {false, 1 << 20, 0, OT_TEXT_NA};
  for (int p1 = 1; p1 <= span - 2; ++p1)
    for (int p2 = (b == 2 ? p1 + 1 : p1); p2 <= (b == 2 ? span - 2 : p1); ++p2) {
      if (dna && (site[p1] == 'N' || site[p2] == 'N')) continue;
      int mm = 0, j = 0;
      for (int i = 0; i < span; ++i) {
        if (i == p1 || i == p2) continue;
        const char s = dna ? longer[i] : shorter[j], g = dna ? shorter[j] : longer[i];
        mm += (s == 'N' || s != g);
        ++j;
      }
      if (mm < best.mm) { best.any = true; best.mm = mm; best.gaps = (1u << p1) | (1u << p2); }
    }
  if (!best.any || best.mm > max_mm) { best.any = false; return best; }
  std::string cr, dn;  // the aligned strings: the guide with '-' at DNA bulges, the site with '-' at RNA bulges
  for (int i = 0, j = 0; i < span; ++i) {
    const bool gap = (best.gaps >> i) & 1u;
    if (dna) { cr += gap ? '-' : guide[j]; dn += site[i]; }
    else { cr += guide[i]; dn += gap ? '-' : site[j]; }
    if (!gap) ++j;
  }
  if (!tab) return best;
  double score = 1.0;
  bool bad = false;
  for (int c = 0; c < span && c < 20; ++c) {
    if (cr[c] == '-' || dn[c] == '-' || cr[c] == dn[c]) continue;
    if (base_of(dn[c]) < 0) bad = true;
    else score *= tab[(c * 4 + base_of(cr[c])) * 4 + base_of(dn[c])];
  }
  const std::string field = right ? pam + dn : dn + pam;
  const int k0 = base_of(field[field.size() - 2]), k1 = base_of(field[field.size() - 1]);
  if (bad || k0 < 0 || k1 < 0) best.units = OT_TEXT_UNSCORABLE;
  else best.units = ot_round_e4(score * tab[320 + 4 * k0 + k1]);
  return best;
}

void encode(const std::string& s, uint64_t* code, uint32_t* nmask) {
  *code = 0; *nmask = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    const int k = base_of(s[i]);
    if (k < 0) *nmask |= 1u << i; else *code |= (uint64_t)k << (2 * i);
  }
}

unsigned long long n_cases = 0, n_rows = 0, n_unscorable = 0;

bool check(const std::string& site, const std::string& pam, const std::string& guide, bool right, int b, bool dna, int max_mm, const double* tab) {
  uint64_t wcode, gcode;
  uint32_t wnmask, gn;
  encode(right ? pam + site : site + pam, &wcode, &wnmask);
  encode(guide, &gcode, &gn);
  const Row want = restate(site, pam, guide, right, b, dna, max_mm, tab);
  const OtbPair got = otb_pair(wcode, wnmask, gcode, (int)guide.size(), (int)pam.size(), right ? 1 : 0, b, dna, max_mm, tab);
  ++n_cases;
  n_rows += want.any;
  n_unscorable += want.any && want.units == OT_TEXT_UNSCORABLE;
  const bool ok = want.any ? (got.mm == want.mm && got.gaps == want.gaps && got.units == want.units) : got.mm > max_mm;
  if (!ok)
    printf("DISAGREE %s b %d right %d max_mm %d tables %d site %s pam %s guide %s: otb_pair mm %d gaps 0x%x units %lld, restatement %s mm %d gaps 0x%x units %lld\n",
           dna ? "DNA" : "RNA", b, (int)right, max_mm, tab != nullptr, site.c_str(), pam.c_str(), guide.c_str(), got.mm, got.gaps, got.units,
           want.any ? "row" : "none", want.mm, want.gaps, want.units);
  return ok;
}

std::string word(uint64_t v, int n, const char* alphabet, int k) {
  std::string s(n, 'A');
  for (int i = 0; i < n; ++i) { s[i] = alphabet[v % k]; v /= k; }
  return s;
}
uint64_t ipow(uint64_t a, int n) { uint64_t r = 1; while (n--) r *= a; return r; }

int exhaustive(const double* tab) {
  const struct { int b, G; const char* sa; int sk; const char* ga; int gk; } plans[] = {
      {1, 4, "ACGTN", 5, "ACGT", 4}, {1, 5, "ACTN", 4, "ACT", 3}, {2, 5, "ACTN", 4, "AC", 2}, {2, 6, "ACN", 3, "AC", 2}};
  const char* pams[] = {"GG", "GN", "TA"};
  for (const auto& pl : plans)
    for (int dna = 0; dna < 2; ++dna) {
      const int Gs = dna ? pl.G + pl.b : pl.G - pl.b;
      const uint64_t ns = ipow(pl.sk, Gs), ng = ipow(pl.gk, pl.G);
      for (uint64_t s = 0; s < ns; ++s) {
        const std::string site = word(s, Gs, pl.sa, pl.sk);
        for (uint64_t g = 0; g < ng; ++g) {
          const std::string guide = word(g, pl.G, pl.ga, pl.gk);
          const int mms[3] = {0, 1, pl.G};
          const bool right = (s + g) & 1;
          for (int max_mm : mms)
            if (!check(site, pams[(s + 3 * g) % 3], guide, right, pl.b, dna != 0, max_mm, (s ^ g) % 5 ? tab : nullptr)) return 1;
        }
      }
    }
  printf("otbsum check: exhaustive %llu cases, %llu rows, %llu unscorable\n", n_cases, n_rows, n_unscorable);
  return 0;
}

// a site near the guide: substitutions, then b interior letters inserted (DNA) or deleted (RNA), then a few N
std::string planted(std::mt19937_64& rng, const std::string& guide, int b, bool dna, int n_sub, int n_amb) {
  std::string s = guide;
  for (int k = 0; k < n_sub; ++k) s[rng() % s.size()] = "ACGT"[rng() % 4];
  for (int k = 0; k < b; ++k) {
    if (dna) s.insert(s.begin() + 1 + (long)(rng() % (s.size() - 1)), "ACGT"[rng() % 4]);
    else s.erase(s.begin() + 1 + (long)(rng() % (s.size() - 2)));
  }
  for (int k = 0; k < n_amb; ++k) s[rng() % s.size()] = 'N';
  return s;
}
std::string random_word(std::mt19937_64& rng, int n) {
  std::string s(n, 'A');
  for (char& c : s) c = "ACGT"[rng() % 4];
  return s;
}

int random_cases(const double* tab) {
  std::mt19937_64 rng(20261019);
  n_cases = n_rows = n_unscorable = 0;
  for (int it = 0; it < 200000; ++it) {
    const int b = 1 + (int)(rng() & 1), P = 2 + (int)(rng() % 2);
    const bool dna = (rng() >> 8) & 1, right = (rng() >> 9) & 1;
    const int gmax = dna ? 32 - P - b : 32 - P;  // the site's window has at most 32 bases
    const int G = gmax < 29 ? gmax - (int)(rng() % 3) : 20 + (int)(rng() % 10);
    const std::string guide = random_word(rng, G);
    const std::string site = (it % 16 == 5) ? random_word(rng, dna ? G + b : G - b)
                                             : planted(rng, guide, b, dna, (int)(rng() % 5), (it % 4 == 1) ? (int)(rng() % 3) : 0);
    std::string pam = random_word(rng, P);
    if (it % 32 == 7) pam[P - 1 - (int)(rng() % 2)] = 'N';
    const int max_mm = (it % 8 == 7) ? G : (int)(rng() % 7);
    if (!check(site, pam, guide, right, b, dna, max_mm, it % 6 ? tab : nullptr)) return 1;
  }
  printf("otbsum check: random %llu cases at G 20..29, %llu rows, %llu unscorable\n", n_cases, n_rows, n_unscorable);
  return n_rows > 50000 && n_unscorable > 100 ? 0 : 1;
}

int sums(const double* tab) {
  std::mt19937_64 rng(7);
  for (int kind = 0; kind < 4; ++kind)
    for (int with_tab = 0; with_tab < 2; ++with_tab) {
      const bool dna = kind < 2, right = kind & 1;
      const int b = 1 + (kind & 1), G = 20, P = 3, max_mm = 3, Gs = dna ? G + b : G - b;
      const uint32_t ng = 7;
      const uint64_t ns = 300;
      std::vector<std::string> guides, sites, pams;
      for (uint32_t g = 0; g < ng; ++g) guides.push_back(g == 6 ? guides[0] : random_word(rng, G));  // a duplicate
      for (uint64_t i = 0; i < ns; ++i) {
        sites.push_back(planted(rng, guides[rng() % ng], b, dna, (int)(rng() % 4), i % 9 == 0));
        pams.push_back(random_word(rng, P));
        if ((int)sites.back().size() != Gs) return 1;
      }
      std::vector<uint64_t> code(ns), g2(ng);
      std::vector<uint32_t> nmask(ns), hist((size_t)ng * (max_mm + 1), 77u), want_hist((size_t)ng * (max_mm + 1), 0u);
      std::vector<int64_t> cfd(ng, -5), want_cfd(ng, 0);
      uint64_t want_hits = 0, want_uns = 0, hits = 9, uns = 9;
      for (uint64_t i = 0; i < ns; ++i) encode(right ? pams[i] + sites[i] : sites[i] + pams[i], &code[i], &nmask[i]);
      for (uint32_t g = 0; g < ng; ++g) { uint32_t gn; encode(guides[g], &g2[g], &gn); }
      const double* tb = with_tab ? tab : nullptr;
      for (uint64_t i = 0; i < ns; ++i)
        for (uint32_t g = 0; g < ng; ++g) {
          const Row r = restate(sites[i], pams[i], guides[g], right, b, dna, max_mm, tb);
          if (!r.any) continue;
          ++want_hits;
          ++want_hist[(size_t)g * (max_mm + 1) + r.mm];
          if (r.units == OT_TEXT_UNSCORABLE) ++want_uns; else if (r.units > 0) want_cfd[g] += r.units;
        }
      hawk_ot_params par = {0, 0, (uint32_t)P, (uint32_t)G, right ? 1u : 0u, (uint32_t)max_mm};
      const int rc = hawk_host_offtarget_bulge_summary(code.data(), nmask.data(), ns, g2.data(), ng, &par, dna ? 1 : 2, (uint32_t)b, tb,
                                                       tb ? tb + 320 : nullptr, hist.data(), cfd.data(), &hits, &uns);
      if (rc != HAWK_OK || hits != want_hits || uns != want_uns || hist != want_hist || cfd != want_cfd || want_hits < 50 ||
          (with_tab && want_uns == 0)) {
        printf("DISAGREE sums kind %d tables %d: rc %d hits %" PRIu64 " / %" PRIu64 " unscorable %" PRIu64 " / %" PRIu64 "\n", kind, with_tab, rc, hits,
               want_hits, uns, want_uns);
        return 1;
      }
      // refusals leave the outputs as they are
      uint64_t h2 = 123, u2 = 456;
      std::vector<uint32_t> keep = hist;
      if (hawk_host_offtarget_bulge_summary(code.data(), nmask.data(), ns, g2.data(), ng, &par, 3, (uint32_t)b, nullptr, nullptr, hist.data(),
                                            cfd.data(), &h2, &u2) != HAWK_E_INVALID ||
          hawk_host_offtarget_bulge_summary(code.data(), nmask.data(), ns, g2.data(), ng, &par, 1, 3, nullptr, nullptr, hist.data(), cfd.data(), &h2,
                                            &u2) != HAWK_E_INVALID ||
          hawk_host_offtarget_bulge_summary(code.data(), nmask.data(), ns, g2.data(), ng, &par, 1, 1, tab, nullptr, hist.data(), cfd.data(), &h2,
                                            &u2) != HAWK_E_INVALID ||
          h2 != 123 || u2 != 456 || hist != keep) {
        printf("DISAGREE refusals kind %d\n", kind);
        return 1;
      }
    }
  printf("otbsum check: the host twin's sums equal the restatement's for 4 kinds, with and without tables\n");
  return 0;
}
}  // namespace

int main() {
  std::mt19937_64 rng(99);
  std::vector<double> tab(336);
  for (double& v : tab) v = (double)(rng() % 10001) / 1e4;  // entries in 0 .. 1 in steps of 1e-4, some of them 0
  for (int k = 0; k < 8; ++k) tab[rng() % 320] = k % 2 ? 0.03125 : 0.09375;  // exact binary ties of the rounding
  for (int k = 320; k < 336; ++k) tab[k] = k % 3 ? 1.0 : 0.5;
  if (exhaustive(tab.data())) return 1;
  if (random_cases(tab.data())) return 1;
  return sums(tab.data());
}
