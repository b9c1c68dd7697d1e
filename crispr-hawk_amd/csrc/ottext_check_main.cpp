// ottext_check_main.cpp - a stand-alone run of the host emitter of the off-targets table (hawk_host_offtarget_text,
// hawk_hostutil.hip) for a sanitizer build: `make asan-ottext` compiles this file and hawk_hostutil.hip with
// -fsanitize=address,undefined and runs the program.  A few thousand random records of every kind, with and without `order`
// and tables, each into a blob of EXACTLY the size the length pass named (a byte too many is a heap overflow the sanitizer
// sees), then every malformed record, which must be refused with the outputs untouched.  Not part of the library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/hawk.h"

namespace {
struct Cols {
  std::vector<uint32_t> guide, row, q, nmask;
  std::vector<uint64_t> code, gaps;
  std::vector<uint8_t> strand, mm, kind, size;
  void push(uint32_t g, uint32_t r, uint32_t qq, uint8_t st, uint8_t m, uint64_t c, uint32_t nm, uint64_t gp, uint8_t k, uint8_t s) {
    guide.push_back(g); row.push_back(r); q.push_back(qq); strand.push_back(st); mm.push_back(m); code.push_back(c); nmask.push_back(nm);
    gaps.push_back(gp); kind.push_back(k); size.push_back(s);
  }
};
struct Call {
  hawk_ot_params p;
  std::vector<uint64_t> guides2;
  std::vector<uint32_t> row_contig;
  std::vector<uint64_t> row_off, name_off;
  std::vector<uint8_t> names;
  const char* pam;
};
int run(const Cols& c, const Call& k, const uint64_t* order, const double* mmt, const double* pt, std::vector<uint8_t>* blob,
        std::vector<uint64_t>* off, std::vector<int64_t>* cfd, uint64_t* nb, uint64_t* nu, bool fill) {
  const uint64_t n = c.guide.size();
  return hawk_host_offtarget_text(n, c.guide.data(), c.row.data(), c.q.data(), c.strand.data(), c.mm.data(), c.code.data(), c.nmask.data(),
                                  c.gaps.data(), c.kind.data(), c.size.data(), k.guides2.data(), (uint32_t)k.guides2.size(), &k.p,
                                  k.row_contig.data(), k.row_off.data(), (uint32_t)k.row_contig.size(), k.names.data(), k.name_off.data(),
                                  (uint32_t)k.name_off.size() - 1, k.pam, order, mmt, pt, fill ? blob->data() : nullptr,
                                  fill ? blob->size() : 0, off->data(), cfd->data(), nb, nu);
}
}  // namespace

int main() {
  std::mt19937_64 rng(20261018);
  auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  double mmt[320], pt[16];
  for (double& v : mmt) v = (double)below(10001) / 1e4;
  for (double& v : pt) v = (double)below(10001) / 1e4;
  int failures = 0;
  uint64_t rows_total = 0, bytes_total = 0;
  for (int cfg = 0; cfg < 4; ++cfg) {
    Call k;
    const uint32_t G = cfg == 0 ? 20 : cfg == 1 ? 23 : cfg == 2 ? 27 : 26, P = cfg == 0 || cfg == 2 ? 3 : 4;
    k.p = hawk_ot_params{0, 0, P, G, (uint32_t)(cfg & 1), 0};
    k.pam = P == 3 ? "NGG" : "TTTV";
    for (int g = 0; g < 7; ++g) k.guides2.push_back(rng() & ((1ull << (2 * G)) - 1));
    const char* nm[4] = {"c", "chr12", "a_contig_of_28_bytes_in_all_", nullptr};
    std::vector<uint8_t> longname(300, 'L');
    k.name_off.push_back(0);
    for (int i = 0; i < 4; ++i) {
      if (nm[i]) k.names.insert(k.names.end(), nm[i], nm[i] + strlen(nm[i])); else k.names.insert(k.names.end(), longname.begin(), longname.end());
      k.name_off.push_back(k.names.size());
    }
    for (uint32_t r = 0; r < 9; ++r) { k.row_contig.push_back(r % 4); k.row_off.push_back(r == 8 ? (1ull << 33) + 5 : below(1ull << 30)); }
    Cols c;
    const uint64_t n = 1500;
    for (uint64_t i = 0; i < n; ++i) {
      const uint8_t kind = (uint8_t)below(3), size = kind ? (uint8_t)(1 + below(2)) : 0;
      const uint32_t Gs = kind == 1 ? G + size : kind == 2 ? G - size : G, span = kind == 1 ? Gs : G;
      uint64_t gaps = 0;
      while ((uint32_t)__builtin_popcountll(gaps) < size) gaps |= 1ull << (1 + below(span - 2));
      const uint32_t W = Gs + P;
      const uint64_t code = rng() & (W >= 32 ? ~0ull : (1ull << (2 * W)) - 1);
      uint32_t nmask = 0;
      if (below(4) == 0) nmask = 1u << below(W);
      c.push((uint32_t)below(k.guides2.size()), (uint32_t)below(9), (uint32_t)below(1ull << 31), (uint8_t)below(2), (uint8_t)below(8), code, nmask,
             gaps, kind, size);
    }
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = below(n);  // repeats allowed
    for (int variant = 0; variant < 4; ++variant) {
      const uint64_t* od = variant & 1 ? order.data() : nullptr;
      const bool tables = variant & 2;
      std::vector<uint64_t> off(n + 1), off2(n + 1);
      std::vector<int64_t> cfd(n), cfd2(n);
      std::vector<uint8_t> blob;
      uint64_t nb = 0, nu = 0, nb2 = 0, nu2 = 0;
      int rc = run(c, k, od, tables ? mmt : nullptr, tables ? pt : nullptr, &blob, &off, &cfd, &nb, &nu, false);
      if (rc != HAWK_E_CAPACITY || off[n] != nb) { printf("length pass: rc %d\n", rc); ++failures; continue; }
      blob.assign(nb, 0);
      rc = run(c, k, od, tables ? mmt : nullptr, tables ? pt : nullptr, &blob, &off2, &cfd2, &nb2, &nu2, true);
      if (rc != HAWK_OK || nb2 != nb || nu2 != nu || off2 != off || cfd2 != cfd) { printf("fill pass: rc %d\n", rc); ++failures; continue; }
      for (uint64_t i = 0; i < n; ++i) {  // ten tabs per row, none of the zero bytes the blob started with
        int tabs = 0;
        for (uint64_t b = off[i]; b < off[i + 1]; ++b) { tabs += blob[b] == '\t'; if (!blob[b]) ++failures; }
        if (tabs != 10) ++failures;
      }
      if (!tables && nu) ++failures;
      rows_total += n; bytes_total += nb;
    }
    // malformed records: the call is refused and nothing is written
    struct Bad { const char* what; uint8_t kind, size; uint64_t gaps; uint32_t row, guide; };
    const Bad bad[] = {{"kind 3", 3, 1, 2, 0, 0}, {"size 3", 1, 3, 14, 0, 0}, {"bulge without size", 1, 0, 0, 0, 0}, {"size without bulge", 0, 1, 2, 0, 0},
                       {"gap at 0", 1, 1, 1, 0, 0}, {"gap at the last position", 1, 1, 1ull << G, 0, 0}, {"gap beyond the span", 2, 1, 1ull << 50, 0, 0},
                       {"popcount above size", 1, 1, 6, 0, 0}, {"popcount below size", 2, 2, 4, 0, 0}, {"row beyond the table", 0, 0, 0, 9, 0},
                       {"guide beyond the guides", 0, 0, 0, 0, 7}, {"X with gaps", 0, 0, 4, 0, 0}};
    for (const Bad& b : bad) {
      Cols m;
      m.push(0, 0, 5, 0, 0, 0x1234567, 0, 0, 0, 0);
      m.push(b.guide, b.row, 5, 0, 0, 0x1234567, 0, b.gaps, b.kind, b.size);
      std::vector<uint64_t> off(3, 77);
      std::vector<int64_t> cfd(2, 77);
      std::vector<uint8_t> blob(4096, 77);
      uint64_t nb = 77, nu = 77;
      const int rc = run(m, k, nullptr, mmt, pt, &blob, &off, &cfd, &nb, &nu, true);
      bool touched = nb != 77 || nu != 77;
      for (uint64_t v : off) touched |= v != 77;
      for (int64_t v : cfd) touched |= v != 77;
      for (uint8_t v : blob) touched |= v != 77;
      if (rc != HAWK_E_INVALID || touched) { printf("%s: rc %d, outputs %s\n", b.what, rc, touched ? "written" : "untouched"); ++failures; }
    }
    {
      Cols m;
      m.push(0, 0, 5, 0, 0, 0x1234567, 0, 0, 0, 0);
      const uint64_t od[1] = {1};
      std::vector<uint64_t> off(2, 77);
      std::vector<int64_t> cfd(1, 77);
      std::vector<uint8_t> blob(512, 77);
      uint64_t nb = 77, nu = 77;
      if (run(m, k, od, nullptr, nullptr, &blob, &off, &cfd, &nb, &nu, true) != HAWK_E_INVALID || off[0] != 77 || nb != 77) { printf("order entry >= n accepted\n"); ++failures; }
    }
  }
  printf("ottext check: %llu rows, %llu bytes, %d failures\n", (unsigned long long)rows_total, (unsigned long long)bytes_total, failures);
  return failures ? 1 : 0;
}
