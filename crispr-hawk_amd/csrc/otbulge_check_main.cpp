// otbulge_check_main.cpp - otb_best (hawk_otbulge.h) as the host compiler builds it, held to a plain walk over every placement.
// Nothing of the device side is included.  `make asan-otbulge` compiles this file with -fsanitize=address,undefined and runs
// `exhaust`; tests/test_bulge_refs.py builds it without sanitizers, runs `exhaust` and feeds `cases`.  Not part of the library.
//   exhaust  b = 1 (n = 3 .. 9) and b = 2 (n = 3 .. 6), span = n + b: every m[0 .. b] over the n positions (even bits), every
//            `forbid` mask over the interior positions 1 .. span - 2 (all forbidden included), max_mm in {0, 1, n}; then 10^6
//            random cases at spans 29 .. 32, sparse and dense vectors.  The first disagreement is printed and the exit code is 1.
//   cases    lines of `b span forbid max_mm m0 m1 [m2]` on stdin (any base strtoull takes), `mm gaps` per line on stdout: otb_best's
//            answer as it is, no logic of its own.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "hawk_otbulge.h"

namespace {
// The mismatches of one placement, position by position: the longer sequence is walked, a gap faces nothing, position j of the
// shorter one faces position i = j + k of the longer one and contributes the bit of m[k] at j.
int walk_count(const uint64_t* m, int span, uint32_t gaps) {
  int mm = 0, j = 0;
  for (int i = 0; i < span; ++i) {
    if ((gaps >> i) & 1u) continue;
    mm += (int)((m[i - j] >> (2 * j)) & 1u);
    ++j;
  }
  return mm;
}

struct Ref { int mm; uint32_t gaps; bool any; };
// every allowed gap tuple in ascending lexicographic order, a strictly smaller count kept - for long spans, where a count per
// position and tuple is too slow for 10^6 cases: counts of whole ranges come from running sums built bit by bit (no mask, no
// popcount); the winner's count is then walked position by position as well
Ref walk_best_sums(const uint64_t* m, int b, int span, uint32_t forbid) {
  const int n = span - b;
  int pre[3][34];
  for (int k = 0; k <= b; ++k) {
    pre[k][0] = 0;
    for (int j = 0; j < n; ++j) pre[k][j + 1] = pre[k][j] + (int)((m[k] >> (2 * j)) & 1u);
  }
  Ref r = {1 << 20, 0, false};
  for (int p1 = 1; p1 <= span - 2; ++p1) {
    if ((forbid >> p1) & 1u) continue;
    if (b == 1) {
      const int mm = pre[0][p1] + pre[1][n] - pre[1][p1];
      if (mm < r.mm) { r.mm = mm; r.gaps = 1u << p1; r.any = true; }
      continue;
    }
    for (int p2 = p1 + 1; p2 <= span - 2; ++p2) {
      if ((forbid >> p2) & 1u) continue;
      const int mm = pre[0][p1] + pre[1][p2 - 1] - pre[1][p1] + pre[2][n] - pre[2][p2 - 1];
      if (mm < r.mm) { r.mm = mm; r.gaps = (1u << p1) | (1u << p2); r.any = true; }
    }
  }
  if (r.any && walk_count(m, span, r.gaps) != r.mm) { r.mm = -1; }  // the two walks disagree: reported as a failure below
  return r;
}

uint64_t spread(uint32_t x) {  // bit j -> bit 2 j
  uint64_t v = 0;
  for (int j = 0; j < 32; ++j) v |= (uint64_t)((x >> j) & 1u) << (2 * j);
  return v;
}

// mm must agree whenever either side is within max_mm, gaps whenever there is a row
bool agree(const OtbBest& got, const Ref& want, int max_mm) {
  const bool row = want.any && want.mm <= max_mm;
  if (want.mm < 0) return false;
  if (!row) return got.mm > max_mm;
  return got.mm == want.mm && got.gaps == want.gaps;
}
int report(const uint64_t* m, int b, int span, uint32_t forbid, int max_mm, const OtbBest& got, const Ref& want) {
  printf("DISAGREE b %d span %d forbid 0x%x max_mm %d m0 0x%" PRIx64 " m1 0x%" PRIx64 " m2 0x%" PRIx64 ": otb_best mm %d gaps 0x%x, walk %s mm %d gaps 0x%x\n",
         b, span, forbid, max_mm, m[0], m[1], b == 2 ? m[2] : 0, got.mm, got.gaps, want.any ? "has" : "none", want.mm, want.gaps);
  return 1;
}

// one slice of the exhaustive part: the m[0] of residue `part` modulo `parts`.  The count of every tuple is walked once per
// (m[0], m[1], m[2]) and kept; the walk over the allowed tuples of a `forbid` mask reads the kept counts in the same order.
struct Slice { unsigned long long cases = 0, rows = 0; int failed = 0; };
void exhaust_slice(int b, int n, uint32_t part, uint32_t parts, std::mutex* mu, Slice* out) {
  const int span = n + b;
  const uint32_t nv = 1u << n, nf = 1u << (span - 2);
  uint32_t tup[64];
  int cnt[64], nt = 0;
  for (int p1 = 1; p1 <= span - 2; ++p1) {
    if (b == 1) { tup[nt++] = 1u << p1; continue; }
    for (int p2 = p1 + 1; p2 <= span - 2; ++p2) tup[nt++] = (1u << p1) | (1u << p2);
  }
  uint64_t m[3] = {0, 0, 0};
  unsigned long long cases = 0, rows = 0;  // summed here: the slices of the threads are neighbours in memory
  for (uint32_t v0 = part; v0 < nv; v0 += parts)
    for (uint32_t v1 = 0; v1 < nv; ++v1)
      for (uint32_t v2 = 0; v2 < (b == 2 ? nv : 1u); ++v2) {
        m[0] = spread(v0); m[1] = spread(v1); m[2] = spread(v2);
        for (int t = 0; t < nt; ++t) cnt[t] = walk_count(m, span, tup[t]);
        for (uint32_t f = 0; f < nf; ++f) {
          const uint32_t forbid = f << 1;  // interior positions 1 .. span - 2
          Ref want = {1 << 20, 0, false};
          for (int t = 0; t < nt; ++t)
            if (!(tup[t] & forbid) && cnt[t] < want.mm) { want.mm = cnt[t]; want.gaps = tup[t]; want.any = true; }
          const int mms[3] = {0, 1, n};
          for (int max_mm : mms) {
            const OtbBest got = otb_best(m, b, span, forbid, max_mm);
            if (!agree(got, want, max_mm)) {
              std::lock_guard<std::mutex> lk(*mu);
              out->failed = report(m, b, span, forbid, max_mm, got, want);
              return;
            }
            ++cases;
            rows += got.mm <= max_mm;
          }
        }
      }
  out->cases = cases;
  out->rows = rows;
}

int exhaust() {
  unsigned long long cases = 0, rows = 0;
  const uint32_t parts = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  std::mutex mu;
  for (int b = 1; b <= 2; ++b) {
    for (int n = 3; n <= (b == 1 ? 9 : 6); ++n) {
      std::vector<Slice> sl(parts);
      std::vector<std::thread> th;
      for (uint32_t k = 0; k < parts; ++k) th.emplace_back(exhaust_slice, b, n, k, parts, &mu, &sl[k]);
      for (std::thread& t : th) t.join();
      for (const Slice& s : sl) {
        if (s.failed) return 1;
        cases += s.cases; rows += s.rows;
      }
    }
  }
  printf("otbulge check: exhaustive %llu cases, %llu with a row\n", cases, rows);
  std::mt19937_64 rng(20261018);
  cases = rows = 0;
  for (int it = 0; it < 1000000; ++it) {
    const int b = 1 + (int)(rng() & 1), span = 29 + (int)(rng() % 4), n = span - b;
    const uint64_t keep = ((1ull << (2 * n)) - 1ull) & OTB_EVEN;
    uint64_t m[3] = {0, 0, 0};
    const int style = it % 4;  // 0 sparse, 1 dense, 2 mixed, 3 near-equal vectors (many ties)
    for (int k = 0; k <= b; ++k) {
      uint64_t v = rng();
      if (style == 0 || (style == 2 && k == 0)) v &= rng() & rng();
      if (style == 1 || (style == 2 && k == 1)) v |= rng() | rng();
      if (style == 3) v = k ? (m[0] ^ (1ull << (2 * (rng() % n)))) : (v & rng() & rng() & rng());
      m[k] = v & keep;
    }
    uint32_t forbid = 0;
    switch ((it / 4) % 4) {
      case 0: break;
      case 1: forbid = 1u << (rng() % span); break;
      case 2: forbid = (uint32_t)(rng() & rng()); break;
      default: forbid = (it % 64 == 12) ? 0xffffffffu : (uint32_t)(rng() | rng()); break;
    }
    if (span < 32) forbid &= (1u << span) - 1u;
    const int max_mm = (it % 8 == 7) ? n : (int)(rng() % 7);
    const Ref want = walk_best_sums(m, b, span, forbid);
    const OtbBest got = otb_best(m, b, span, forbid, max_mm);
    if (!agree(got, want, max_mm)) return report(m, b, span, forbid, max_mm, got, want);
    ++cases;
    rows += got.mm <= max_mm;
  }
  printf("otbulge check: random %llu cases at spans 29..32, %llu with a row\n", cases, rows);
  return 0;
}

int cases_mode() {
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    uint64_t v[7] = {0, 0, 0, 0, 0, 0, 0};
    int k = 0;
    char* s = line;
    for (; k < 7; ++k) {
      char* e = nullptr;
      v[k] = strtoull(s, &e, 0);
      if (e == s) break;
      s = e;
    }
    if (k == 0) continue;  // an empty line
    const int b = (int)v[0], span = (int)v[1];
    if (b < 1 || b > 2 || k != 5 + b || span < b + 3 || span > 32) { fprintf(stderr, "bad line: %s", line); return 2; }
    const OtbBest r = otb_best(v + 4, b, span, (uint32_t)v[2], (int)v[3]);
    printf("%d %u\n", r.mm, r.gaps);
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "exhaust")) return exhaust();
  if (argc == 2 && !strcmp(argv[1], "cases")) return cases_mode();
  fprintf(stderr, "usage: %s exhaust | cases < lines\n", argv[0]);
  return 2;
}
