// hawk_hostutil.hip — host-side helpers of the report assembly.  No device code: the guide report's
// `samples` and `haplotype_id` columns list every carrier of every report row (C3: 28 M entries, ~330 MB of text);
// joining them is a ragged byte gather that Python cannot do at memory speed, so it lives here, multi-threaded.
#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdlib>
#include <string>
#include <cstring>
#include <thread>
#include <atomic>
#include <vector>

#include "../../include/hawk.h"
#include "hawk_ottext.h"
#include "hawk_otbulge.h"
#include "hawk_otvar.h"
#include "hawk_gnomad.h"
#include "hawk_effects.h"
#include "hawk_resolve.h"
#include "hawk_ugroups.h"
#include "hawk_ubuild.h"
#include "hawk_uwin.h"
#include "hawk_inflate.h"

namespace {
template <class F> void par_groups(uint64_t n_groups, F f) {
  unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
  if (n_groups < 4096) nt = 1;
  const uint64_t per = (n_groups + nt - 1) / nt;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t)
    th.emplace_back([=] { f(std::min<uint64_t>(n_groups, t * per), std::min<uint64_t>(n_groups, (t + 1) * per)); });
  f(0, std::min<uint64_t>(n_groups, per));
  for (auto& x : th) x.join();
}
template <class F> void par_groups_any(uint64_t n, F f) {  // the same split for few, heavy items
  const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n, std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
  const uint64_t per = (n + nt - 1) / nt;
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back([=] { f(std::min<uint64_t>(n, t * per), std::min<uint64_t>(n, (t + 1) * per)); });
  f(0, std::min<uint64_t>(n, per));
  for (auto& x : th) x.join();
}
inline unsigned dec_len(uint32_t v) { unsigned n = 1; while (v >= 10) { v /= 10; ++n; } return n; }
inline uint8_t* put_dec(uint8_t* w, uint32_t v) {
  char tmp[12]; int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) *w++ = (uint8_t)tmp[--n];
  return w;
}
}  // namespace

extern "C" {

// For every group g the items item_label[group_off[g] .. group_off[g+1]) name byte strings pool[pool_off[l] .. pool_off[l+1]);
// the group's output is those strings joined by `sep`.  out_off[n_groups + 1] receives the byte offsets of the groups in
// `out` (always written); the bytes are written when `out` is non-NULL and out_cap suffices, else HAWK_E_CAPACITY with
// the required size in out_off[n_groups].
int hawk_host_ragged_join(const uint32_t* item_label, const uint64_t* group_off, uint64_t n_groups, const uint8_t* pool,
                          const uint64_t* pool_off, uint64_t n_labels, uint8_t sep, uint8_t* out, uint64_t out_cap,
                          uint64_t* out_off) {
  if (!group_off || !out_off || (group_off[n_groups] && (!item_label || !pool || !pool_off))) return HAWK_E_INVALID;
  const uint64_t n_items = group_off[n_groups];
  for (uint64_t g = 0; g < n_groups; ++g)
    if (group_off[g + 1] < group_off[g]) return HAWK_E_INVALID;
  unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
  if (n_groups < 4096) nt = 1;
  const uint64_t per = (n_groups + nt - 1) / nt;
  // pass 1: sizes
  std::vector<int> bad(nt, 0);
  auto size_pass = [&](unsigned t) {
    const uint64_t g0 = std::min<uint64_t>(n_groups, t * per), g1 = std::min<uint64_t>(n_groups, g0 + per);
    for (uint64_t g = g0; g < g1; ++g) {
      uint64_t sz = 0;
      for (uint64_t i = group_off[g]; i < group_off[g + 1]; ++i) {
        const uint32_t l = item_label[i];
        if (l >= n_labels) { bad[t] = 1; return; }
        sz += pool_off[l + 1] - pool_off[l] + 1;
      }
      out_off[g + 1] = sz ? sz - 1 : 0;  // separators between items only
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(size_pass, t);
    size_pass(0);
    for (auto& x : th) x.join();
  }
  for (int b : bad) if (b) return HAWK_E_INVALID;
  out_off[0] = 0;
  for (uint64_t g = 0; g < n_groups; ++g) out_off[g + 1] += out_off[g];
  (void)n_items;
  if (!out) return HAWK_OK;
  if (out_off[n_groups] > out_cap) return HAWK_E_CAPACITY;
  auto write_pass = [&](unsigned t) {
    const uint64_t g0 = std::min<uint64_t>(n_groups, t * per), g1 = std::min<uint64_t>(n_groups, g0 + per);
    for (uint64_t g = g0; g < g1; ++g) {
      uint8_t* w = out + out_off[g];
      for (uint64_t i = group_off[g]; i < group_off[g + 1]; ++i) {
        const uint32_t l = item_label[i];
        const uint64_t n = pool_off[l + 1] - pool_off[l];
        if (i != group_off[g]) *w++ = sep;
        memcpy(w, pool + pool_off[l], n);
        w += n;
      }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(write_pass, t);
  write_pass(0);
  for (auto& x : th) x.join();
  return HAWK_OK;
}


// Per group: the sorted set of the items its member haplotypes carry, joined by `sep` (collapse_haplotype_ids,
// reports.py:845-857, and the unphased form of collapse_samples).  Haplotype h carries items hap_item[hap_item_off[h] ..
// hap_item_off[h+1]), each an index into the label pool whose order IS the sort order.
int hawk_host_group_join(const uint64_t* member_off, const uint32_t* member_hap, uint64_t n_groups, const uint64_t* hap_item_off,
                         const uint32_t* hap_item, uint64_t n_haps, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_labels,
                         uint8_t sep, uint8_t* out, uint64_t out_cap, uint64_t* out_off) {
  if (!member_off || !out_off || !hap_item_off || (member_off[n_groups] && (!member_hap || !pool_off))) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < member_off[n_groups]; ++i) if (member_hap[i] >= n_haps) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < hap_item_off[n_haps]; ++i) if (hap_item[i] >= n_labels) return HAWK_E_INVALID;
  auto run = [&](bool write) {
    par_groups(n_groups, [&, write](uint64_t g0, uint64_t g1) {
      std::vector<uint32_t> items;
      for (uint64_t g = g0; g < g1; ++g) {
        items.clear();
        bool sorted = true;
        for (uint64_t i = member_off[g]; i < member_off[g + 1]; ++i) {
          const uint32_t h = member_hap[i];
          for (uint64_t k = hap_item_off[h]; k < hap_item_off[h + 1]; ++k) {
            if (!items.empty() && hap_item[k] < items.back()) sorted = false;
            items.push_back(hap_item[k]);
          }
        }
        if (!sorted) std::sort(items.begin(), items.end());
        items.erase(std::unique(items.begin(), items.end()), items.end());
        if (!write) {
          uint64_t sz = 0;
          for (uint32_t l : items) sz += pool_off[l + 1] - pool_off[l] + 1;
          out_off[g + 1] = sz ? sz - 1 : 0;
        } else {
          uint8_t* w = out + out_off[g];
          bool first = true;
          for (uint32_t l : items) {
            if (!first) *w++ = sep;
            first = false;
            const uint64_t n = pool_off[l + 1] - pool_off[l];
            memcpy(w, pool + pool_off[l], n);
            w += n;
          }
        }
      }
    });
  };
  run(false);
  out_off[0] = 0;
  for (uint64_t g = 0; g < n_groups; ++g) out_off[g + 1] += out_off[g];
  if (!out) return HAWK_OK;
  if (out_off[n_groups] > out_cap) return HAWK_E_CAPACITY;
  run(true);
  return HAWK_OK;
}

// The `samples` column of a phased panel (reports.py:767-810: sorted unique `sample:a|b` entries, then one entry per sample
// with the per-copy maxima, samples in the order of their first entry).  Haplotype h carries entries hap_ent[...]; entry e
// belongs to sample ent_sample[e] (samples numbered in that first-entry order) with alleles ent_a1[e] | ent_a2[e];
// ent_ok[e] = 0 marks an entry that is not `name:int|int`.  group_flags[g]: bit 0 = the group holds an ok (phased) entry,
// bit 1 = it holds one that is not.  A group with only such entries gets them joined as they are (entry strings in ent_pool);
// a group mixing both kinds gets an empty string (the caller resolves it).
int hawk_host_group_samples(const uint64_t* member_off, const uint32_t* member_hap, uint64_t n_groups, const uint64_t* hap_ent_off,
                            const uint32_t* hap_ent, uint64_t n_haps, const uint32_t* ent_sample, const uint16_t* ent_a1,
                            const uint16_t* ent_a2, const uint8_t* ent_ok, uint64_t n_entries, const uint8_t* name_pool,
                            const uint64_t* name_off, uint64_t n_samples, const uint8_t* ent_pool, const uint64_t* ent_pool_off,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* group_flags) {
  if (!member_off || !out_off || !hap_ent_off || !group_flags || (member_off[n_groups] && (!member_hap || !name_off))) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < member_off[n_groups]; ++i) if (member_hap[i] >= n_haps) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < hap_ent_off[n_haps]; ++i) if (hap_ent[i] >= n_entries) return HAWK_E_INVALID;
  for (uint64_t e = 0; e < n_entries; ++e) if (ent_sample[e] >= n_samples) return HAWK_E_INVALID;
  struct Ent { uint32_t s; uint16_t a, b; };
  auto run = [&](bool write) {
    par_groups(n_groups, [&, write](uint64_t g0, uint64_t g1) {
      std::vector<Ent> v;
      std::vector<uint32_t> raw;
      for (uint64_t g = g0; g < g1; ++g) {
        v.clear();
        raw.clear();
        bool sorted = true;
        uint8_t fl = 0;
        for (uint64_t i = member_off[g]; i < member_off[g + 1]; ++i) {
          const uint32_t h = member_hap[i];
          for (uint64_t k = hap_ent_off[h]; k < hap_ent_off[h + 1]; ++k) {
            const uint32_t e = hap_ent[k];
            fl |= ent_ok[e] ? 1 : 2;
            if (!v.empty() && ent_sample[e] < v.back().s) sorted = false;
            v.push_back(Ent{ent_sample[e], ent_a1[e], ent_a2[e]});
            raw.push_back(e);
          }
        }
        group_flags[g] = fl;
        if (fl == 2) {  // no phased entry at all (e.g. the REF group): the sorted unique entries as they are
          std::sort(raw.begin(), raw.end());
          raw.erase(std::unique(raw.begin(), raw.end()), raw.end());
          if (!write) {
            uint64_t sz = 0;
            for (uint32_t e : raw) sz += ent_pool_off[e + 1] - ent_pool_off[e] + 1;
            out_off[g + 1] = sz ? sz - 1 : 0;
          } else {
            uint8_t* w = out + out_off[g];
            bool first = true;
            for (uint32_t e : raw) {
              if (!first) *w++ = ',';
              first = false;
              const uint64_t len = ent_pool_off[e + 1] - ent_pool_off[e];
              memcpy(w, ent_pool + ent_pool_off[e], len);
              w += len;
            }
          }
          continue;
        }
        if (fl & 2) { if (!write) out_off[g + 1] = 0; continue; }
        if (!sorted) std::stable_sort(v.begin(), v.end(), [](const Ent& x, const Ent& y) { return x.s < y.s; });
        size_t n = 0;  // merge neighbours of one sample: per-copy maxima
        for (size_t i = 0; i < v.size(); ++i) {
          if (n && v[n - 1].s == v[i].s) { v[n - 1].a = std::max(v[n - 1].a, v[i].a); v[n - 1].b = std::max(v[n - 1].b, v[i].b); }
          else v[n++] = v[i];
        }
        if (!write) {
          uint64_t sz = 0;
          for (size_t i = 0; i < n; ++i) sz += name_off[v[i].s + 1] - name_off[v[i].s] + 1 + dec_len(v[i].a) + 1 + dec_len(v[i].b) + 1;
          out_off[g + 1] = sz ? sz - 1 : 0;
        } else {
          uint8_t* w = out + out_off[g];
          for (size_t i = 0; i < n; ++i) {
            if (i) *w++ = ',';
            const uint64_t len = name_off[v[i].s + 1] - name_off[v[i].s];
            memcpy(w, name_pool + name_off[v[i].s], len);
            w += len;
            *w++ = ':';
            w = put_dec(w, v[i].a);
            *w++ = '|';
            w = put_dec(w, v[i].b);
          }
        }
      }
    });
  };
  run(false);
  out_off[0] = 0;
  for (uint64_t g = 0; g < n_groups; ++g) out_off[g + 1] += out_off[g];
  if (!out) return HAWK_OK;
  if (out_off[n_groups] > out_cap) return HAWK_E_CAPACITY;
  run(true);
  return HAWK_OK;
}

}  // extern "C"

// ---- the guide report as TSV text, written straight to its file ---------------------------------------------------------
// The report of a C3 search is 2.2 x 10^5 rows and 0.64 GB of text (the `samples` / `haplotype_id` columns list every carrier of
// every row).  Python needs seconds to turn columns into row strings and the rows into a file; here the columns arrive as they
// are kept - constants, fixed-width byte matrices, ragged byte columns, integers, vocabulary indices - and the rows are
// laid out in two parallel passes (lengths, then bytes) directly in a shared mapping of the output file.
namespace {
inline unsigned dec_len64(int64_t v) {
  unsigned n = v < 0 ? 1u : 0u;
  uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1u : (uint64_t)v;
  do { u /= 10; ++n; } while (u);
  return n;
}
inline uint8_t* put_dec64(uint8_t* w, int64_t v) {
  char tmp[24]; int n = 0;
  uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1u : (uint64_t)v;
  do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
  if (v < 0) *w++ = '-';
  while (n) *w++ = (uint8_t)tmp[--n];
  return w;
}
inline uint64_t field_len(const hawk_tsv_col& c, uint64_t r) {
  switch (c.kind) {
    case HAWK_TSV_CONST: return c.width;
    case HAWK_TSV_FIXED: return c.width;
    case HAWK_TSV_RAGGED: return c.off[r + 1] - c.off[r];
    case HAWK_TSV_INT64: return dec_len64(static_cast<const int64_t*>(c.data)[r]);
    default: { const uint32_t k = static_cast<const uint32_t*>(c.data)[r]; return c.off[k + 1] - c.off[k]; }
  }
}
inline uint8_t* field_put(const hawk_tsv_col& c, uint64_t r, uint8_t* w) {
  switch (c.kind) {
    case HAWK_TSV_CONST: memcpy(w, c.data, c.width); return w + c.width;
    case HAWK_TSV_FIXED: memcpy(w, static_cast<const uint8_t*>(c.data) + r * c.width, c.width); return w + c.width;
    case HAWK_TSV_RAGGED: { const uint64_t n = c.off[r + 1] - c.off[r]; memcpy(w, static_cast<const uint8_t*>(c.data) + c.off[r], n); return w + n; }
    case HAWK_TSV_INT64: return put_dec64(w, static_cast<const int64_t*>(c.data)[r]);
    default: {
      const uint32_t k = static_cast<const uint32_t*>(c.data)[r];
      const uint64_t n = c.off[k + 1] - c.off[k];
      memcpy(w, static_cast<const uint8_t*>(c.pool) + c.off[k], n);
      return w + n;
    }
  }
}
}  // namespace
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
extern "C" {

int hawk_host_tsv_write(const char* path, const char* header, uint64_t header_len, uint64_t n_rows, const uint64_t* order, uint32_t n_cols,
                        const hawk_tsv_col* cols, uint64_t* bytes_out) {
  if (!path || !n_cols || !cols || (header_len && !header)) return HAWK_E_INVALID;
  for (uint32_t c = 0; c < n_cols; ++c) {
    const hawk_tsv_col& k = cols[c];
    if (k.kind > HAWK_TSV_VOCAB) return HAWK_E_INVALID;
    if (n_rows && k.kind != HAWK_TSV_CONST && !k.data) return HAWK_E_INVALID;
    if ((k.kind == HAWK_TSV_RAGGED || k.kind == HAWK_TSV_VOCAB) && !k.off) return HAWK_E_INVALID;
    if (k.kind == HAWK_TSV_VOCAB && !k.pool && k.n_vocab) return HAWK_E_INVALID;
    if (k.kind == HAWK_TSV_CONST && k.width && !k.data) return HAWK_E_INVALID;
  }
  if (order) for (uint64_t i = 0; i < n_rows; ++i) if (order[i] >= n_rows) return HAWK_E_INVALID;
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c].kind == HAWK_TSV_VOCAB) {
      const uint32_t* idx = static_cast<const uint32_t*>(cols[c].data);
      for (uint64_t i = 0; i < n_rows; ++i) if (idx[i] >= cols[c].n_vocab) return HAWK_E_INVALID;
    }
  // pass 1: bytes of every output row (fields + tabs + newline)
  std::vector<uint64_t> row_off(n_rows + 1, 0);
  par_groups(n_rows, [&](uint64_t i0, uint64_t i1) {
    for (uint64_t i = i0; i < i1; ++i) {
      const uint64_t r = order ? order[i] : i;
      uint64_t sz = n_cols;  // n_cols - 1 tabs + the newline
      for (uint32_t c = 0; c < n_cols; ++c) sz += field_len(cols[c], r);
      row_off[i + 1] = sz;
    }
  });
  row_off[0] = header_len;
  for (uint64_t i = 0; i < n_rows; ++i) row_off[i + 1] += row_off[i];
  const uint64_t total = row_off[n_rows];
  if (bytes_out) *bytes_out = total;
  const int fd = open(path, O_RDWR | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return HAWK_E_INVALID;
  if (total == 0) { close(fd); return HAWK_OK; }
  // The rows are laid out in anonymous memory (huge pages where the system grants them: first-touch faults of 4 KB pages were
  // a third of the pass) and leave through parallel pwrite()s.  Measured on the GPU box's overlay file system, 0.63 GB of report:
  // a shared mapping of the file 0.47 s, this 0.22 s, the layout alone 0.16 s (tools/_tsv_probe.py, round 4).
  uint8_t* out = static_cast<uint8_t*>(mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
  if (out == MAP_FAILED) { close(fd); return HAWK_E_INVALID; }
#ifdef MADV_HUGEPAGE
  (void)madvise(out, total, MADV_HUGEPAGE);
#endif
  if (header_len) memcpy(out, header, header_len);
  par_groups(n_rows, [&](uint64_t i0, uint64_t i1) {
    for (uint64_t i = i0; i < i1; ++i) {
      const uint64_t r = order ? order[i] : i;
      uint8_t* w = out + row_off[i];
      for (uint32_t c = 0; c < n_cols; ++c) {
        w = field_put(cols[c], r, w);
        *w++ = c + 1 == n_cols ? '\n' : '\t';
      }
    }
  });
  int rc = HAWK_OK;
  const uint64_t n_chunks = (total + (1u << 22) - 1) >> 22;  // 4 MB pieces
  std::vector<int> bad(1, 0);
  auto put = [&](uint64_t c0, uint64_t c1) {
    uint64_t done = c0 << 22;
    const uint64_t end = std::min<uint64_t>(total, c1 << 22);
    while (done < end) {
      const ssize_t k = pwrite(fd, out + done, end - done, (off_t)done);
      if (k <= 0) { bad[0] = 1; return; }
      done += (uint64_t)k;
    }
  };
  if (n_chunks >= 16) par_groups_any(n_chunks, put); else put(0, n_chunks);
  if (bad[0]) rc = HAWK_E_INVALID;
  munmap(out, total);
  if (close(fd) != 0) rc = HAWK_E_INVALID;
  return rc;
}

// ---- the line index of a VCF text (f3: readers.VCF) ------------------------------------------------------------------------
// A 2504-sample VCF is ~10 kB per record; the reader's index pass (where does every record start, what is its POS, where do its
// sample columns begin) walks every byte of it once.  numpy did that at ~1.5 GB/s on one core; here the text - the reader maps the
// file - is cut into pieces, one thread each: newlines counted, then every line's fields located.
//   line_start[i]   offset of line i (header lines included), line_start[n_lines] = end of the last line (= len)
//   pos[i]          POS of a record, -1 for a header line ('#'), -2 for a malformed record (no second tab / non-digit POS)
//   gt_off[i]       offset of the record's first sample column (behind its 9th tab), 0 when the line has fewer than 9 tabs
//   chrom_len[i]    bytes of the record's CHROM field
// *n_lines: lines found (the text must end with a newline); with cap too small nothing but *n_lines is written and
// HAWK_E_CAPACITY is returned.  *multi_contig: 1 when two records differ in CHROM.
int hawk_host_vcf_index(const uint8_t* text, uint64_t len, uint64_t cap, uint64_t* line_start, int64_t* pos, uint64_t* gt_off,
                        uint32_t* chrom_len, uint64_t* n_lines, uint32_t* multi_contig) {
  if (!n_lines || (len && !text)) return HAWK_E_INVALID;
  if (len && text[len - 1] != '\n') return HAWK_E_INVALID;
  unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
  if (len < (1u << 22)) nt = 1;
  const uint64_t per = (len + nt - 1) / nt;
  std::vector<uint64_t> cnt(nt + 1, 0);
  auto count = [&](unsigned t) {
    const uint64_t a = std::min<uint64_t>(len, t * per), b = std::min<uint64_t>(len, a + per);
    uint64_t c = 0;
    const uint8_t* p = text + a;
    const uint8_t* e = text + b;
    while (p < e) { const void* q = memchr(p, '\n', (size_t)(e - p)); if (!q) break; ++c; p = static_cast<const uint8_t*>(q) + 1; }
    cnt[t + 1] = c;
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(count, t);
    count(0);
    for (auto& x : th) x.join();
  }
  for (unsigned t = 0; t < nt; ++t) cnt[t + 1] += cnt[t];
  const uint64_t n = cnt[nt];
  *n_lines = n;
  if (n > cap) return HAWK_E_CAPACITY;
  if (!n) return HAWK_OK;
  if (!line_start || !pos || !gt_off || !chrom_len) return HAWK_E_INVALID;
  auto fill = [&](unsigned t) {  // line k + 1 starts behind the k-th newline
    const uint64_t a = std::min<uint64_t>(len, t * per), b = std::min<uint64_t>(len, a + per);
    uint64_t k = cnt[t];
    const uint8_t* p = text + a;
    const uint8_t* e = text + b;
    while (p < e) {
      const void* q = memchr(p, '\n', (size_t)(e - p));
      if (!q) break;
      p = static_cast<const uint8_t*>(q) + 1;
      line_start[++k] = (uint64_t)(p - text);
    }
  };
  line_start[0] = 0;
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(fill, t);
    fill(0);
    for (auto& x : th) x.join();
  }
  par_groups(n, [&](uint64_t i0, uint64_t i1) {
    for (uint64_t i = i0; i < i1; ++i) {
      const uint8_t* p = text + line_start[i];
      const uint8_t* e = text + line_start[i + 1] - 1;  // the newline
      gt_off[i] = 0; chrom_len[i] = 0;
      if (p == e) { pos[i] = -1; continue; }        // empty line: skipped like a header
      if (*p == '#') { pos[i] = -1; continue; }
      const uint8_t* t1 = static_cast<const uint8_t*>(memchr(p, '\t', (size_t)(e - p)));
      const uint8_t* t2 = t1 ? static_cast<const uint8_t*>(memchr(t1 + 1, '\t', (size_t)(e - t1 - 1))) : nullptr;
      if (!t1 || !t2 || t2 == t1 + 1 || t2 - t1 > 19) { pos[i] = -2; continue; }
      int64_t v = 0;
      bool ok = true;
      for (const uint8_t* q = t1 + 1; q < t2; ++q) { if (*q < '0' || *q > '9') { ok = false; break; } v = v * 10 + (*q - '0'); }
      if (!ok) { pos[i] = -2; continue; }
      pos[i] = v;
      chrom_len[i] = (uint32_t)(t1 - p);
      const uint8_t* q = t2;  // the 2nd tab; seven more end the FORMAT column
      int tabs = 2;
      while (tabs < 9) {
        q = static_cast<const uint8_t*>(memchr(q + 1, '\t', (size_t)(e - q - 1)));
        if (!q) break;
        ++tabs;
      }
      if (q && tabs == 9) gt_off[i] = (uint64_t)(q + 1 - text);
    }
  });
  if (multi_contig) {
    *multi_contig = 0;
    uint64_t f = n;
    for (uint64_t i = 0; i < n; ++i) if (pos[i] >= 0) { f = i; break; }
    if (f < n) {
      const uint8_t* c0 = text + line_start[f];
      const uint32_t l0 = chrom_len[f];
      par_groups(n, [&](uint64_t i0, uint64_t i1) {
        for (uint64_t i = i0; i < i1; ++i)
          if (pos[i] >= 0 && (chrom_len[i] != l0 || memcmp(text + line_start[i], c0, l0) != 0)) { *multi_contig = 1; return; }
      });
    }
  }
  return HAWK_OK;
}


// ---- which of a haplotype's variants a guide shows (annotation.py:246-284, polish_guide_variants) ----------------------------
// The report's variant_id / af columns: for a row whose candidate variants are all SNVs the assembly answers in bulk (numpy); a
// row with an indel among them - or a position map that is not linear over the guide - needs the reference's own walk over the
// guide's positions, which took 25 us of Python per row (C3: 10^4 rows, a quarter of a second).  Here the walk itself, for all
// such rows at once:
//   row k: spacer + PAM `cores[k]` (L cased bytes, + strand), haplotype row hap[k] whose position map is segments
//   [seg_start[h], seg_start[h + 1]) of (seg_rel, seg_gen), first guide position pivot[k], genomic `stop[k]`, candidates
//   cand_var[cand_off[k] .. cand_off[k + 1]) - variant indices, ascending, no duplicates.
//   variant v: adjusted position t_pos[v], alleles ref / alt (pools), name_rank[v] = rank of its id in string order.
// Output: out_var[out_off[k] .. out_off[k + 1]) = the variants the guide shows, in id order (out_var holds cand_off[n] entries at
// most); need_python[k] = 1 where the reference's code would trip its own assertion (annotation.py:185-189) - the caller runs
// its Python mirror on those rows, which raises as the reference does.
namespace {
inline bool is_upper(uint8_t c) { return c >= 'A' && c <= 'Z'; }
inline bool is_lower(uint8_t c) { return c >= 'a' && c <= 'z'; }
inline uint8_t to_upper(uint8_t c) { return is_lower(c) ? (uint8_t)(c - 32) : c; }
}  // namespace
namespace {
struct PolishTables {
  uint32_t L;
  const uint64_t* seg_start; const uint32_t* seg_rel; const int64_t* seg_gen;
  const int64_t* t_pos; const uint8_t* ref_pool; const uint64_t* ref_off; const uint8_t* alt_pool; const uint64_t* alt_off;
  const uint32_t* name_rank;
};
// one row of annotation.polish_guide_variants: the candidates `cand` (ascending variant indices, no duplicates) the guide g shows,
// written to w in id order; returns their number, or -1 where the reference's own assertion would fire
inline int polish_one(const PolishTables& T, const uint8_t* g, uint32_t hap, int64_t pivot, int64_t stop, const uint32_t* cand, uint32_t n_cand,
                      uint32_t* w) {
  const uint32_t L = T.L;
  int64_t gen[64];
  // genomic position of every guide position: PosSegments.lookup (last segment with rel <= p)
  const uint64_t s0 = T.seg_start[hap], s1 = T.seg_start[hap + 1];
  uint64_t j = s0;
  {
    uint64_t lo = s0, hi = s1;  // last j in [s0, s1) with seg_rel[j] <= pivot (seg_rel[s0] = 0)
    const int64_t p0 = pivot < 0 ? 0 : pivot;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if ((int64_t)T.seg_rel[mid] <= p0) lo = mid; else hi = mid; }
    j = lo;
  }
  for (uint32_t i = 0; i < L; ++i) {
    const int64_t p = pivot + i;
    while (j + 1 < s1 && (int64_t)T.seg_rel[j + 1] <= p) ++j;
    gen[i] = T.seg_gen[j] + (p - (int64_t)T.seg_rel[j]);
  }
  uint32_t m = 0;
  for (uint32_t i = 0; i < L; ++i) {
    uint32_t offset = 0;
    for (uint32_t c = 0; c < n_cand; ++c) {
      const uint32_t v = cand[c];
      if (T.t_pos[v] != gen[i]) continue;
      const uint64_t rl = T.ref_off[v + 1] - T.ref_off[v], al = T.alt_off[v + 1] - T.alt_off[v];
      const uint8_t* alt = T.alt_pool + T.alt_off[v];
      const bool is_snv = rl == al;
      if (!is_snv) offset = rl < al ? (uint32_t)(al - rl) : 0u;
      const uint32_t sl = std::min<uint32_t>(offset + 1, L - i);  // seg = guidepam[i : i + offset + 1]
      const uint8_t* seg = g + i;
      bool show = false;
      if (!is_snv) {  // _check_insertion
        if (i == 0) {
          // _find_insertion_stop asserts a lower-case first base and at least one base that is not upper case
          bool all_up = true;
          for (uint32_t q = 0; q < sl; ++q) all_up = all_up && is_upper(seg[q]);
          if (is_upper(seg[0]) || all_up) return -1;
          uint32_t st = 0;
          for (uint32_t q = 0; q < sl; ++q) if (is_upper(seg[q])) { st = q; break; }
          bool ends = st <= al;  // alt.endswith(seg.upper()[:st])
          for (uint32_t q = 0; q < st && ends; ++q) ends = alt[al - st + q] == to_upper(seg[q]);
          show = ends;
        }
        if (!show && gen[i] == stop && sl <= al) {  // alt.startswith(seg.upper())
          bool starts = true;
          for (uint32_t q = 0; q < sl && starts; ++q) starts = alt[q] == to_upper(seg[q]);
          show = starts;
        }
      }
      if (!show) {  // seg.islower() and seg.upper() == alt
        bool low = true;
        for (uint32_t q = 0; q < sl; ++q) low = low && is_lower(seg[q]);
        if (low && sl == al) {
          bool eq = true;
          for (uint32_t q = 0; q < sl && eq; ++q) eq = alt[q] == to_upper(seg[q]);
          show = eq;
        }
      }
      if (show) {
        bool dup = false;
        for (uint32_t q = 0; q < m; ++q) dup = dup || w[q] == v;
        if (!dup) w[m++] = v;
      }
    }
  }
  std::sort(w, w + m, [&](uint32_t x, uint32_t y) { return T.name_rank[x] < T.name_rank[y]; });
  return (int)m;
}
// out_var[off[k] ..) -> out_var[out_off[k] ..), in place (rows only move towards the front)
inline void polish_compact(uint64_t n, const uint64_t* off, const std::vector<uint32_t>& cnt, uint64_t* out_off, uint32_t* out_var) {
  out_off[0] = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t src = off[k], dst = out_off[k];
    if (dst != src) memmove(out_var + dst, out_var + src, (size_t)cnt[k] * 4);
    out_off[k + 1] = dst + cnt[k];
  }
}
}  // namespace
int hawk_host_polish_rows(uint64_t n, uint32_t L, const uint8_t* cores, const uint32_t* hap, const int64_t* pivot, const int64_t* stop,
                          const uint64_t* cand_off, const uint32_t* cand_var, const uint64_t* seg_start, const uint32_t* seg_rel,
                          const int64_t* seg_gen, uint64_t n_haps, const int64_t* t_pos, const uint8_t* ref_pool, const uint64_t* ref_off,
                          const uint8_t* alt_pool, const uint64_t* alt_off, uint32_t n_var, const uint32_t* name_rank, uint64_t* out_off,
                          uint32_t* out_var, uint8_t* need_python) {
  if (!n) { if (out_off) out_off[0] = 0; return HAWK_OK; }
  if (!cores || !hap || !pivot || !stop || !cand_off || !seg_start || !seg_rel || !seg_gen || !t_pos || !ref_off || !alt_off || !name_rank ||
      !out_off || !out_var || !need_python || !L || L > 64)
    return HAWK_E_INVALID;
  for (uint64_t k = 0; k < n; ++k) if (hap[k] >= n_haps || cand_off[k + 1] < cand_off[k]) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < cand_off[n]; ++i) if (cand_var[i] >= n_var) return HAWK_E_INVALID;
  const PolishTables T{L, seg_start, seg_rel, seg_gen, t_pos, ref_pool, ref_off, alt_pool, alt_off, name_rank};
  std::vector<uint32_t> cnt(n, 0);
  par_groups(n, [&](uint64_t k0, uint64_t k1) {
    for (uint64_t k = k0; k < k1; ++k) {
      const int m = polish_one(T, cores + k * L, hap[k], pivot[k], stop[k], cand_var + cand_off[k], (uint32_t)(cand_off[k + 1] - cand_off[k]),
                               out_var + cand_off[k]);
      need_python[k] = m < 0;
      cnt[k] = m < 0 ? 0u : (uint32_t)m;
    }
  });
  polish_compact(n, cand_off, cnt, out_off, out_var);
  return HAWK_OK;
}

int hawk_host_variant_window(uint64_t n, const uint32_t* hap, const int64_t* p_lo, const int64_t* p_hi, const uint64_t* var_off,
                             const int64_t* var_idx, const int64_t* t_pos, uint64_t n_haps, uint32_t n_var, uint64_t* first, uint32_t* count) {
  if (!n) return HAWK_OK;
  if (!hap || !p_lo || !p_hi || !var_off || !var_idx || !t_pos || !first || !count) return HAWK_E_INVALID;
  std::atomic<int> bad{0};
  par_groups(n_haps, [&](uint64_t h0, uint64_t h1) {  // every row's list: valid indices, ascending positions
    for (uint64_t h = h0; h < h1 && !bad.load(std::memory_order_relaxed); ++h) {
      if (var_off[h + 1] < var_off[h]) { bad = 1; break; }
      int64_t prev = INT64_MIN;
      for (uint64_t k = var_off[h]; k < var_off[h + 1]; ++k) {
        const int64_t v = var_idx[k];
        if (v < 0 || v >= (int64_t)n_var) { bad = 1; break; }
        if (t_pos[v] < prev) { bad = 2; break; }
        prev = t_pos[v];
      }
    }
  });
  if (bad.load() == 1) return HAWK_E_INVALID;
  if (bad.load() == 2) return HAWK_E_UNSUPPORTED;  // (the caller sorts, or takes its own route)
  for (uint64_t k = 0; k < n; ++k) if (hap[k] >= n_haps) return HAWK_E_INVALID;
  par_groups(n, [&](uint64_t k0, uint64_t k1) {
    for (uint64_t k = k0; k < k1; ++k) {
      const uint64_t b0 = var_off[hap[k]], b1 = var_off[hap[k] + 1];
      uint64_t lo = b0, hi = b1;  // first entry with position >= p_lo
      while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (t_pos[var_idx[mid]] < p_lo[k]) lo = mid + 1; else hi = mid; }
      const uint64_t a = lo;
      hi = b1;                    // first entry with position > p_hi
      while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (t_pos[var_idx[mid]] <= p_hi[k]) lo = mid + 1; else hi = mid; }
      first[k] = a;
      count[k] = (uint32_t)(lo - a);
    }
  });
  return HAWK_OK;
}

int hawk_host_polish_windows(uint64_t n, uint32_t L, const uint8_t* cores, const uint32_t* hap, const int64_t* pivot, const int64_t* stop,
                             const uint64_t* first, const uint64_t* cand_off, const int64_t* var_idx, uint64_t n_idx, const uint64_t* seg_start,
                             const uint32_t* seg_rel, const int64_t* seg_gen, uint64_t n_haps, const int64_t* t_pos, const uint8_t* ref_pool,
                             const uint64_t* ref_off, const uint8_t* alt_pool, const uint64_t* alt_off, uint32_t n_var, const uint32_t* name_rank,
                             uint64_t* out_off, uint32_t* out_var, uint8_t* need_python) {
  if (!n) { if (out_off) out_off[0] = 0; return HAWK_OK; }
  if (!cores || !hap || !pivot || !stop || !first || !cand_off || !var_idx || !seg_start || !seg_rel || !seg_gen || !t_pos || !ref_off || !alt_off ||
      !name_rank || !out_off || !out_var || !need_python || !L || L > 64)
    return HAWK_E_INVALID;
  for (uint64_t k = 0; k < n; ++k)
    if (hap[k] >= n_haps || cand_off[k + 1] < cand_off[k] || first[k] + (cand_off[k + 1] - cand_off[k]) > n_idx) return HAWK_E_INVALID;
  const PolishTables T{L, seg_start, seg_rel, seg_gen, t_pos, ref_pool, ref_off, alt_pool, alt_off, name_rank};
  std::vector<uint32_t> cnt(n, 0);
  std::atomic<int> bad{0};
  par_groups(n, [&](uint64_t k0, uint64_t k1) {
    std::vector<uint32_t> cand;
    for (uint64_t k = k0; k < k1; ++k) {
      const uint64_t nc = cand_off[k + 1] - cand_off[k];
      cand.resize(nc);
      for (uint64_t c = 0; c < nc; ++c) {
        const int64_t v = var_idx[first[k] + c];
        if (v < 0 || v >= (int64_t)n_var) { bad = 1; cand[c] = 0; } else cand[c] = (uint32_t)v;
      }
      std::sort(cand.begin(), cand.end());
      const uint32_t nu = (uint32_t)(std::unique(cand.begin(), cand.end()) - cand.begin());
      const int m = polish_one(T, cores + k * L, hap[k], pivot[k], stop[k], cand.data(), nu, out_var + cand_off[k]);
      need_python[k] = m < 0;
      cnt[k] = m < 0 ? 0u : (uint32_t)m;
    }
  });
  if (bad.load()) return HAWK_E_INVALID;
  polish_compact(n, cand_off, cnt, out_off, out_var);
  return HAWK_OK;
}


// ---- the rows of the off-targets table on the host ---------------------------------------------------------------------------
// hawk_offtarget_text without a device: the same checks, the same ot_text_row (hawk_ottext.h), one thread.  It is what holds the
// emitter to the fixtures on a machine without a GPU; the product writes its table through the kernels.
int hawk_host_offtarget_text(uint64_t n, const uint32_t* guide, const uint32_t* row, const uint32_t* q, const uint8_t* strand,
                             const uint8_t* mm, const uint64_t* code, const uint32_t* nmask, const uint64_t* gaps, const uint8_t* kind,
                             const uint8_t* size, const uint64_t* guides2, uint32_t n_guides, const hawk_ot_params* p,
                             const uint32_t* row_contig, const uint64_t* row_off, uint32_t n_table_rows, const uint8_t* name_blob,
                             const uint64_t* name_off, uint32_t n_contigs, const char* pam_text, const uint64_t* order,
                             const double* cfd_mm, const double* cfd_pam, uint8_t* blob, uint64_t blob_cap, uint64_t* off, int64_t* cfd_e4,
                             uint64_t* n_bytes, uint64_t* n_unscorable) {
  if (!p || !off || !n_bytes || !n_unscorable || !cfd_mm != !cfd_pam || (p->pamlen && !pam_text)) return HAWK_E_INVALID;
  if (n && (!guides2 || !row_off || !cfd_e4)) return HAWK_E_INVALID;
  if (p->guidelen == 0 || p->guidelen > 32 || p->guidelen + p->pamlen > 32) return HAWK_E_UNSUPPORTED;
  if (cfd_mm && p->pamlen < 2) return HAWK_E_UNSUPPORTED;
  OtTextFmt fmt;
  memset(&fmt, 0, sizeof(fmt));
  fmt.G = p->guidelen; fmt.P = p->pamlen; fmt.right = p->right ? 1u : 0u;
  for (uint32_t k = 0; k < p->pamlen; ++k) fmt.pam[k] = (uint8_t)pam_text[k];
  const OtTextCols cols = {guide, row, q, nmask, code, gaps, strand, mm, kind, size};
  if (!ot_text_check(n, cols, fmt, n_guides, row_contig, n_table_rows, name_blob, name_off, n_contigs, order)) return HAWK_E_INVALID;
  double tab[336];
  if (cfd_mm) { memcpy(tab, cfd_mm, 320 * sizeof(double)); memcpy(tab + 320, cfd_pam, 16 * sizeof(double)); }
  const double* tb = cfd_mm ? tab : nullptr;
  // the length pass and the fill pass: one function, two sinks
  auto emit = [&](uint64_t i, auto& sink) {
    const OtTextRec r = ot_text_rec(cols, order ? order[i] : i);
    const uint32_t c = row_contig[r.row];
    return ot_text_row(r, guides2[r.guide], name_blob + name_off[c], name_off[c + 1] - name_off[c], row_off[r.row] + r.q, fmt, tb, sink);
  };
  uint64_t total = 0, uns = 0;
  off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) {
    OtTextCount cnt;
    const long long u = emit(i, cnt);
    cfd_e4[i] = u < 0 ? -1 : u;
    uns += u == OT_TEXT_UNSCORABLE;
    total += cnt.n;
    off[i + 1] = total;
  }
  *n_bytes = total;
  *n_unscorable = uns;
  if (!blob || blob_cap < total) return total ? HAWK_E_CAPACITY : HAWK_OK;
  for (uint64_t i = 0; i < n; ++i) {
    OtTextBytes w;
    w.w = blob + off[i];
    (void)emit(i, w);
  }
  return HAWK_OK;
}

// ---- the bulged off-target summary on the host ----------------------------------------------------------------------------------
// hawk_offtarget_bulge_summary without a device: the site windows are given (code / nmask as a site record holds them), every
// (site, guide) pair goes through otb_pair (hawk_otbulge.h) - the function the kernel's summing sink runs - in a plain loop, and
// the rows are summed as the kernel sums them.
int hawk_host_offtarget_bulge_summary(const uint64_t* code, const uint32_t* nmask, uint64_t n_sites, const uint64_t* guides2, uint32_t n_guides,
                                      const hawk_ot_params* p, uint32_t bulge_type, uint32_t bulge_size, const double* cfd_mm,
                                      const double* cfd_pam, uint32_t* out_hist, int64_t* out_cfd_e4, uint64_t* n_hits, uint64_t* n_unscorable) {
  if (!p || !n_hits || !n_unscorable || (n_guides && (!guides2 || !out_hist)) || (n_sites && (!code || !nmask)) || !cfd_mm != !cfd_pam ||
      (cfd_mm && n_guides && !out_cfd_e4))
    return HAWK_E_INVALID;
  if (bulge_type < 1 || bulge_type > 2 || bulge_size < 1 || bulge_size > 2) return HAWK_E_INVALID;
  if ((cfd_mm && p->pamlen < 2) || p->max_mm > 32) return HAWK_E_UNSUPPORTED;
  const bool dna = bulge_type == 1;
  const uint32_t G = p->guidelen;
  if (G > 32 || G < bulge_size + 3) return HAWK_E_UNSUPPORTED;
  if ((dna ? G + bulge_size : G - bulge_size) + p->pamlen > 32) return HAWK_E_UNSUPPORTED;
  double tab[336];
  if (cfd_mm) { memcpy(tab, cfd_mm, 320 * sizeof(double)); memcpy(tab + 320, cfd_pam, 16 * sizeof(double)); }
  const uint32_t stride = p->max_mm + 1;
  uint64_t hits = 0, uns = 0;
  if (n_guides) memset(out_hist, 0, (size_t)n_guides * stride * 4);
  if (n_guides && out_cfd_e4) memset(out_cfd_e4, 0, (size_t)n_guides * 8);
  for (uint64_t i = 0; i < n_sites; ++i)
    for (uint32_t g = 0; g < n_guides; ++g) {
      const OtbPair r = otb_pair(code[i], nmask[i], guides2[g], (int)G, (int)p->pamlen, p->right ? 1 : 0, (int)bulge_size, dna, (int)p->max_mm,
                                 cfd_mm ? tab : nullptr);
      if (r.mm > (int)p->max_mm) continue;
      ++hits;
      ++out_hist[(size_t)g * stride + (uint32_t)r.mm];
      if (r.units == OT_TEXT_UNSCORABLE) ++uns;
      else if (r.units > 0) out_cfd_e4[g] += r.units;
    }
  *n_hits = hits;
  *n_unscorable = uns;
  return HAWK_OK;
}

// ---- the off-target scan over a variant-enriched genome on the host ------------------------------------------------------------
// hawk_genome_variants + hawk_offtarget_variant_scan without a device: the rows' text, the variant entries and the guides go
// through ov_resolve (hawk_otvar.h) - the function k_ov_match runs for its survivors - in plain loops, every (window, strand,
// guide).  Rows come out in (row, q, strand, guide) order.
int hawk_host_offtarget_variant_scan(const char* seqs, const uint64_t* seq_off, uint32_t n_rows, const int32_t* scan_start,
                                     const int32_t* scan_stop, const uint32_t* v_row, const uint32_t* v_q, const uint8_t* v_ref,
                                     const uint8_t* v_alt, uint64_t n_var, uint8_t* v_status, const hawk_ot_params* p, const uint64_t* guides2,
                                     uint32_t n_guides, uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand,
                                     uint8_t* out_mm, uint64_t* out_code, uint32_t* out_nmask, uint32_t* out_alt, uint64_t cap, uint64_t* n_out) {
  if (!p || !n_out || (n_rows && (!seqs || !seq_off || !scan_start || !scan_stop)) || (n_var && (!v_row || !v_q || !v_ref || !v_alt)) ||
      (n_guides && !guides2))
    return HAWK_E_INVALID;
  if (p->guidelen == 0 || p->guidelen + p->pamlen > 32 || p->pamlen == 0 || p->pamlen > 16) return HAWK_E_UNSUPPORTED;
  const int G = (int)p->guidelen, P = (int)p->pamlen, L = G + P;
  for (uint32_t k = 0; k < p->pamlen; ++k)
    if (((p->pam_fwd >> (4 * k)) & 15u) == 0) return HAWK_E_INVALID;  // every PAM position is an IUPAC code
  std::vector<uint64_t> len(n_rows);
  for (uint32_t h = 0; h < n_rows; ++h) {
    if (seq_off[h + 1] < seq_off[h]) return HAWK_E_INVALID;
    len[h] = seq_off[h + 1] - seq_off[h];
    if (scan_start[h] < 0 || scan_stop[h] > (int64_t)len[h]) return HAWK_E_INVALID;
    if (scan_stop[h] > scan_start[h] && (uint64_t)scan_stop[h] - 1 + (uint64_t)L > len[h]) return HAWK_E_INVALID;
  }
  for (uint64_t i = 0; i < n_var; ++i)
    if (v_row[i] >= n_rows || v_q[i] >= len[v_row[i]] || v_ref[i] > 3 || v_alt[i] > 3) return HAWK_E_INVALID;
  // per base: REF's code (4: ambiguous) and the allele set as a nibble
  const uint64_t total = n_rows ? seq_off[n_rows] - seq_off[0] : 0;
  std::vector<uint8_t> rbase(total), aset(total);
  for (uint64_t i = 0; i < total; ++i) {
    uint8_t b = 4;
    switch (seqs[seq_off[0] + i] & 0xDF) { case 'A': b = 0; break; case 'C': b = 1; break; case 'G': b = 2; break; case 'T': b = 3; break; default: break; }
    rbase[i] = b;
    aset[i] = b < 4 ? (uint8_t)(1u << b) : 0;
  }
  for (uint64_t i = 0; i < n_var; ++i) {
    const uint64_t at = seq_off[v_row[i]] - seq_off[0] + v_q[i];
    uint8_t st = HAWK_OV_APPLIED;
    if (rbase[at] == 4) st = HAWK_OV_REF_N;
    else if (rbase[at] != v_ref[i]) st = HAWK_OV_REF_MISMATCH;
    else if (v_alt[i] == v_ref[i]) st = HAWK_OV_ALT_IS_REF;
    else aset[at] |= (uint8_t)(1u << v_alt[i]);
    if (v_status) v_status[i] = st;
  }
  OvGeom g;
  g.pam_fwd = p->pam_fwd; g.G = G; g.P = P; g.right = p->right ? 1 : 0;
  uint64_t n = 0;
  for (uint32_t h = 0; h < n_rows; ++h) {
    const uint64_t base = seq_off[h] - seq_off[0];
    for (int64_t q = scan_start[h]; q < scan_stop[h]; ++q)
      for (int s = 0; s < 2; ++s) {
        uint64_t rcode = 0;
        uint32_t nmask = 0, am[4] = {0, 0, 0, 0};
        for (int i = 0; i < L; ++i) {  // guide orientation: strand 1 is the reverse complement of the + strand window
          const uint64_t at = base + (uint64_t)q + (uint64_t)(s ? L - 1 - i : i);
          const uint8_t b = rbase[at], a = aset[at];
          if (b == 4) nmask |= 1u << i;
          else rcode |= (uint64_t)(s ? 3 - b : b) << (2 * i);
          for (int x = 0; x < 4; ++x)
            if ((a >> x) & 1) am[s ? 3 - x : x] |= 1u << i;
        }
        if (!ov_alt_positions(rcode, nmask, am, L)) continue;  // no ALT allele in the window: the plain scan's
        for (uint32_t gi = 0; gi < n_guides; ++gi) {
          const OvResolved r = ov_resolve(rcode, nmask, am, guides2[gi], g);
          if (!r.ok || r.mm > (int)p->max_mm || !r.alt) continue;
          if (n < cap) {
            if (out_guide) out_guide[n] = gi;
            if (out_row) out_row[n] = h;
            if (out_q) out_q[n] = (uint32_t)q;
            if (out_strand) out_strand[n] = (uint8_t)s;
            if (out_mm) out_mm[n] = (uint8_t)r.mm;
            if (out_code) out_code[n] = r.code;
            if (out_nmask) out_nmask[n] = nmask;
            if (out_alt) out_alt[n] = r.alt;
          }
          ++n;
        }
      }
  }
  *n_out = n;
  return n > cap ? HAWK_E_CAPACITY : HAWK_OK;
}

// ---- gnomAD sites records -> population-genotype lines on the host ------------------------------------------------------------
// hawk_gnomad_scan + hawk_gnomad_text without a device: the same checks and the same functions of hawk_gnomad.h, one thread, one
// record after the other.  Where the kernel finds entry starts by sweeping chunks, this walks INFO from ';' to ';'; what an entry
// start, a key match, a value, a flag and a line ARE is the header's.
namespace {
struct GnHostRec {
  uint32_t fo[8], mask, flags, qual[2], af[2];
};
inline GnHostRec gn_host_scan(const uint8_t* text, uint64_t lo, uint64_t end, const uint8_t* key_blob, const uint64_t* key_off, uint32_t n_keys,
                              uint32_t keep) {
  GnHostRec R;
  uint64_t hi = end;
  while (hi > lo && (text[hi - 1] == '\n' || text[hi - 1] == '\r')) --hi;
  const uint8_t* rec = text + lo;
  const uint32_t len = (uint32_t)(hi - lo);
  for (uint32_t& f : R.fo) f = len;
  R.fo[0] = 0;
  uint32_t tabs = 0, info_hi = len, commas = 0;
  for (uint32_t p = 0; p < len; ++p) {
    if (rec[p] == '\t') {
      if (++tabs < 8) R.fo[tabs] = p + 1;
      else { info_hi = p; break; }
    } else if (tabs == 4 && rec[p] == ',') ++commas;
  }
  const bool full = tabs >= 7;
  uint32_t pos[32];
  for (uint32_t& q : pos) q = GN_ABSENT;
  const uint8_t afkey[2] = {'A', 'F'};
  if (full) {
    uint32_t p = R.fo[7];
    while (p < info_hi) {  // an entry starts at p: behind the tab that opens INFO or behind a ';'
      for (uint32_t j = 0; j < n_keys; ++j)
        if (pos[j] == GN_ABSENT && gn_key_at(rec, p, len, key_blob + key_off[j], (uint32_t)(key_off[j + 1] - key_off[j]))) pos[j] = p;
      if (pos[31] == GN_ABSENT && gn_key_at(rec, p, len, afkey, 2)) pos[31] = p;
      while (p < info_hi && rec[p] != ';') ++p;
      ++p;
    }
  }
  bool absent = false, bad = false;
  uint32_t mask = 0;
  for (uint32_t j = 0; full && j < n_keys; ++j) {
    if (pos[j] == GN_ABSENT) { absent = true; continue; }
    const uint32_t kl = (uint32_t)(key_off[j + 1] - key_off[j]);
    const int v = gn_key_at(rec, pos[j], len, key_blob + key_off[j], kl) == 1 ? gn_value(rec, (uint64_t)pos[j] + kl + 1, len) : 2;
    if (v == 1) mask |= 1u << j;
    if (v == 2) bad = true;
  }
  R.flags = full ? gn_record_flags(rec, R.fo, keep, absent, bad) : GN_FEW_FIELDS;
  R.mask = R.flags ? 0u : mask;
  gn_spans(rec, R.fo, len, full, pos[31], commas, R.qual, R.af);
  return R;
}
}  // namespace

int hawk_host_gnomad_lines(const uint8_t* text, uint64_t text_len, const uint64_t* line_off, uint64_t n_lines, const uint8_t* key_blob,
                           const uint64_t* key_off, uint32_t n_keys, int keep, uint32_t* mask, uint8_t* flags, uint32_t* field_off,
                           uint32_t* qual_span, uint32_t* af_span, const uint8_t* pool_blob, const uint64_t* pool_off, uint8_t* blob,
                           uint64_t blob_cap, uint64_t* off, uint64_t* n_bytes, uint64_t* n_kept) {
  if (!n_bytes || !n_kept || !gn_args_ok(text, text_len, line_off, n_lines, key_blob, key_off, n_keys)) return HAWK_E_INVALID;
  std::vector<GnHostRec> recs(n_lines);
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n_lines; ++i) {
    recs[i] = gn_host_scan(text, line_off[i], line_off[i + 1], key_blob, key_off, n_keys, keep ? 1u : 0u);
    kept += recs[i].flags == 0;
  }
  if (pool_off) {  // checked before anything is written
    if (pool_off[0] != 0) return HAWK_E_INVALID;
    for (uint64_t j = 0; j < 2 * kept; ++j)
      if (pool_off[j + 1] < pool_off[j]) return HAWK_E_INVALID;
    if (pool_off[2 * kept] && !pool_blob) return HAWK_E_INVALID;
  }
  for (uint64_t i = 0; i < n_lines; ++i) {
    const GnHostRec& R = recs[i];
    if (mask) mask[i] = R.mask;
    if (flags) flags[i] = (uint8_t)R.flags;
    if (field_off) memcpy(field_off + i * 8, R.fo, 32);
    if (qual_span) memcpy(qual_span + i * 2, R.qual, 8);
    if (af_span) memcpy(af_span + i * 2, R.af, 8);
  }
  *n_kept = kept;
  *n_bytes = 0;
  if (!pool_off) return HAWK_OK;
  // the length pass and the fill pass: one function, two sinks
  auto emit = [&](uint64_t i, uint64_t k, auto& sink) {
    const GnHostRec& R = recs[i];
    gn_line(text + line_off[i], R.fo, R.mask, n_keys, pool_blob + pool_off[k], pool_off[k + 1] - pool_off[k], pool_blob + pool_off[kept + k],
            pool_off[kept + k + 1] - pool_off[kept + k], R.af[1] != GN_ABSENT, R.af[0], sink);
  };
  uint64_t total = 0, k = 0;
  std::vector<uint64_t> o(n_lines + 1, 0);
  for (uint64_t i = 0; i < n_lines; ++i) {
    if (recs[i].flags == 0) {
      GnCount c;
      emit(i, k++, c);
      total += c.n;
    }
    o[i + 1] = total;
  }
  if (off) memcpy(off, o.data(), (n_lines + 1) * 8);
  *n_bytes = total;
  if (!blob || blob_cap < total) return total ? HAWK_E_CAPACITY : HAWK_OK;
  k = 0;
  for (uint64_t i = 0; i < n_lines; ++i) {
    if (recs[i].flags) continue;
    GnBytes w;
    w.w = blob + o[i];
    emit(i, k++, w);
  }
  return HAWK_OK;
}

// ---- float32 text as Python prints it -----------------------------------------------------------------------------------------
namespace {
// str(float(numpy.float32(float(entry)))) appended to `out`; false when entry is no finite decimal number
inline bool f32_repr_one(const uint8_t* s, uint32_t n, std::string& out) {
  if (n == 0 || n > 400) return false;
  char buf[408];
  bool digit = false;
  for (uint32_t k = 0; k < n; ++k) {
    const char c = (char)s[k];
    if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return false;  // no nan, inf, hex, blanks
    digit |= c >= '0' && c <= '9';
    buf[k] = c;
  }
  if (!digit) return false;
  buf[n] = 0;
  char* end = nullptr;
  const double parsed = strtod(buf, &end);
  if (end != buf + n) return false;
  const float f = (float)parsed;
  if (!std::isfinite(f)) return false;
  const double d = (double)f;
  char sci[40];
  const auto r = std::to_chars(sci, sci + sizeof(sci) - 1, d, std::chars_format::scientific);  // shortest digits that round-trip
  if (r.ec != std::errc()) return false;
  *r.ptr = 0;
  // [-]d[.ddd]e[+-]XX -> the digits and the position of the decimal point behind the first of them
  const char* p = sci;
  if (*p == '-') { out.push_back('-'); ++p; }
  char dig[24];
  int nd = 0;
  for (; p < r.ptr && *p != 'e'; ++p)
    if (*p != '.') dig[nd++] = *p;
  const int decpt = (int)strtol(p + 1, nullptr, 10) + 1;
  while (nd > 1 && dig[nd - 1] == '0') --nd;
  if (decpt > -4 && decpt <= 16) {  // repr's fixed notation, ".0" behind integers
    if (decpt <= 0) {
      out.append("0.");
      out.append((size_t)-decpt, '0');
      out.append(dig, (size_t)nd);
    } else if (decpt >= nd) {
      out.append(dig, (size_t)nd);
      out.append((size_t)(decpt - nd), '0');
      out.append(".0");
    } else {
      out.append(dig, (size_t)decpt);
      out.push_back('.');
      out.append(dig + decpt, (size_t)(nd - decpt));
    }
  } else {
    out.push_back(dig[0]);
    if (nd > 1) { out.push_back('.'); out.append(dig + 1, (size_t)(nd - 1)); }
    const int e = decpt - 1, ae = e < 0 ? -e : e;
    out.push_back('e');
    out.push_back(e < 0 ? '-' : '+');
    if (ae < 10) out.push_back('0');
    out.append(std::to_string(ae));
  }
  return true;
}
}  // namespace

int hawk_host_f32_repr(const uint8_t* text, const uint64_t* start, const uint32_t* len, uint64_t n, const char* missing, uint8_t* out,
                       uint64_t out_cap, uint64_t* out_off, uint8_t* status, uint32_t threads) {
  if (!out_off || (n && (!start || !len || !status || !missing))) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < n; ++i)
    if (len[i] != 0xffffffffu && len[i] && !text) return HAWK_E_INVALID;
  unsigned nt = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
  nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min(nt, 32u), n / 2048 + 1));
  const uint64_t per = (n + nt - 1) / nt;
  std::vector<std::string> part(nt);
  auto work = [&](unsigned t) {
    std::string& o = part[t];
    const uint64_t i0 = std::min<uint64_t>(n, t * per), i1 = std::min<uint64_t>(n, i0 + per);
    for (uint64_t i = i0; i < i1; ++i) {
      const size_t at = o.size();
      bool ok = true;
      if (len[i] != 0xffffffffu) {
        const uint8_t* s = text + start[i];
        uint32_t p = 0;
        for (;;) {  // one comma entry [p, q)
          uint32_t q = p;
          while (q < len[i] && s[q] != ',') ++q;
          if (q - p == 1 && s[p] == '.') o.append(missing);
          else if (!f32_repr_one(s + p, q - p, o)) { ok = false; break; }
          if (q >= len[i]) break;
          o.push_back(',');
          p = q + 1;
        }
      }
      if (!ok) o.resize(at);
      status[i] = ok ? 0 : 1;
      out_off[i + 1] = o.size() - at;
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
  }
  out_off[0] = 0;
  for (uint64_t i = 0; i < n; ++i) out_off[i + 1] += out_off[i];
  const uint64_t total = out_off[n];
  if (!out || out_cap < total) return total ? HAWK_E_CAPACITY : HAWK_OK;
  uint64_t at = 0;
  for (unsigned t = 0; t < nt; ++t) {
    memcpy(out + at, part[t].data(), part[t].size());
    at += part[t].size();
  }
  return HAWK_OK;
}

// ---- variant effects on the host: the loops of k_fx_* over host arrays, every rule from hawk_effects.h
static FxCols fx_cols_of(const hawk_effects_columns* c) {
  FxCols f;
  f.n_groups = c->n_groups; f.win_stride = c->win_stride; f.start = c->start; f.stop = c->stop; f.strand = c->strand; f.win = c->win;
  f.member_off = c->member_off; f.member_hap = c->member_hap; f.is_ref = nullptr; f.hap_off = c->hap_off; f.sample_id = c->sample_id;
  f.rank = c->rank; f.n_hap = c->n_hap; f.n_sample_ids = c->n_sample_ids; f.guidelen = c->guidelen; f.pamlen = c->pamlen; f.right = c->right;
  return f;
}

int hawk_host_round4(const double* x, uint64_t n, double* out) {
  if (n && (!x || !out)) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) out[i] = fx_round4(x[i]);
  return HAWK_OK;
}

int hawk_host_effects(const hawk_effects_columns* cols, int family, const double* score, const int64_t* cand_start,
                      const uint8_t* cand_strand, uint32_t n_cand, uint32_t K, const hawk_effects_out* out, uint64_t alt_cap,
                      uint32_t* n_chosen, uint64_t* n_alts) {
  if (!cols || !out || !n_chosen || !n_alts) return HAWK_E_INVALID;
  *n_chosen = 0; *n_alts = 0;
  if ((family != FX_SIGNED && family != FX_ABSOLUTE) || K < 1 || K > FX_MAX_K || n_cand > K || (n_cand && (!cand_start || !cand_strand)))
    return HAWK_E_INVALID;
  FxCols c = fx_cols_of(cols);
  const int bad = fx_check_cols(c);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  const uint64_t G = c.n_groups;
  if (G && !cols->hap_is_ref) return HAWK_E_INVALID;
  std::vector<uint8_t> origin(G);
  for (uint64_t g = 0; g < G; ++g) origin[g] = cols->hap_is_ref[c.member_hap[c.member_off[g]]];
  c.is_ref = origin.data();
  if (!score) score = cols->cfdon;
  if (G && !score) return HAWK_E_INVALID;
  uint64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<uint32_t> head(G), pref(G, FX_NONE), pnv(G, 0), pfr(G, FX_NONE);
  std::vector<double> pworst(G, 0.0), rs(G);
  std::vector<uint64_t> seen((c.n_sample_ids + 63) / 64 + 1);
  for (uint64_t g = 0; g < G; ++g) {
    const uint64_t h = fx_head(c, g);
    head[g] = (uint32_t)h;
    const bool ref = fx_is_ref(c, g);
    const uint8_t type = fx_guide_type(ref, fx_case_bits(c, g));
    const bool dup = fx_is_dup(c, g, h);
    if (!dup) ++counts[type == FX_TYPE_UNKNOWN ? 4 : type];
    if (h == g) ++counts[5];
    uint32_t ns = 0;
    if (!ref) {  // distinct samples over the member rows' labels
      uint64_t entries = 0;
      for (uint64_t m = c.member_off[g]; m < c.member_off[g + 1]; ++m)
        for (uint64_t e = c.hap_off[c.member_hap[m]]; e < c.hap_off[c.member_hap[m] + 1]; ++e, ++entries) {
          const uint32_t id = c.sample_id[e];
          if (!((seen[id >> 6] >> (id & 63)) & 1)) { seen[id >> 6] |= 1ull << (id & 63); ++ns; }
        }
      for (uint64_t m = c.member_off[g]; m < c.member_off[g + 1]; ++m)
        for (uint64_t e = c.hap_off[c.member_hap[m]]; e < c.hap_off[c.member_hap[m] + 1]; ++e) seen[c.sample_id[e] >> 6] = 0;
      if (c.member_off[g + 1] - c.member_off[g] > FX_SHORT_LIST || entries > FX_SHORT_LIST) ++counts[6];
    }
    rs[g] = fx_round4(score[g]);
    if (out->n_samples) out->n_samples[g] = ns;
    if (out->type) out->type[g] = type;
    if (out->dup) out->dup[g] = dup ? 1 : 0;
    if (out->position) out->position[g] = (uint32_t)h;
    if (out->score) out->score[g] = rs[g];
  }
  std::vector<FxEntry> ranked;
  for (uint64_t h = 0; h < G; ++h) {
    if (head[h] != h) continue;
    const uint64_t e = fx_end(c, h);
    const FxPosition p = fx_position(c, score, family, h, e);
    pref[h] = p.ref; pworst[h] = p.worst; pnv[h] = p.n_valid; pfr[h] = p.first_rank;
    for (uint64_t j = h; j < e; ++j) {
      const double d = p.ref == FX_NONE ? 0.0 : fx_delta(rs[j], p.ref_score);
      if (out->delta) out->delta[j] = d;
      if (out->abs_delta) out->abs_delta[j] = fabs(d);
    }
    if (p.ref == FX_NONE) continue;
    bool is_cand = false;
    for (uint32_t k = 0; k < n_cand; ++k) is_cand = is_cand || (cand_start[k] == c.start[h] && cand_strand[k] == c.strand[h]);
    if (!is_cand) ranked.push_back(FxEntry{fx_key(family, p.worst), p.first_rank, (uint32_t)h});
  }
  for (uint64_t g = 0; g < G; ++g) {
    if (out->pos_ref) out->pos_ref[g] = pref[g];
    if (out->pos_worst) out->pos_worst[g] = pworst[g];
    if (out->pos_nvalid) out->pos_nvalid[g] = pnv[g];
    if (out->pos_first_rank) out->pos_first_rank[g] = pfr[g];
  }
  const size_t take = std::min<size_t>(K - n_cand, ranked.size());
  std::partial_sort(ranked.begin(), ranked.begin() + take, ranked.end(), fx_before);
  std::vector<uint32_t> chosen;
  for (uint32_t k = 0; k < n_cand; ++k) {
    uint32_t at = FX_NONE;
    for (uint64_t h = 0; h < G; ++h)
      if (head[h] == h && pref[h] != FX_NONE && cand_start[k] == c.start[h] && cand_strand[k] == c.strand[h]) at = (uint32_t)h;
    chosen.push_back(at);
  }
  for (size_t i = 0; i < take; ++i) chosen.push_back(ranked[i].head);
  *n_chosen = (uint32_t)chosen.size();
  uint64_t total = 0;
  for (uint32_t h : chosen) total += h == FX_NONE ? 0 : pnv[h];
  *n_alts = total;
  if (out->counts) memcpy(out->counts, counts, sizeof(counts));
  for (size_t i = 0; i < chosen.size(); ++i)
    if (out->chosen) out->chosen[i] = chosen[i];
  if (out->alt_group && total > alt_cap) return HAWK_E_CAPACITY;
  uint64_t at = 0;
  for (size_t i = 0; i < chosen.size(); ++i) {
    if (out->alt_off) out->alt_off[i] = at;
    const uint32_t h = chosen[i];
    if (h == FX_NONE) continue;
    std::vector<uint32_t> alts;
    const double ref_score = rs[pref[h]];
    for (uint64_t j = h, e = fx_end(c, h); j < e; ++j)
      if (!fx_is_ref(c, j) && fx_valid_alt(family, rs[j], ref_score)) alts.push_back((uint32_t)j);
    std::sort(alts.begin(), alts.end(), [&](uint32_t a, uint32_t b) { return c.rank[a] < c.rank[b]; });
    for (uint32_t j : alts) {
      if (out->alt_group) out->alt_group[at] = j;
      ++at;
    }
  }
  if (out->alt_off) out->alt_off[chosen.size()] = at;
  return HAWK_OK;
}

// ---- unphased IUPAC windows (hawk_resolve.h): the host twin of hawk_table_resolve_unphased
static UrRow ur_host_row(const hawk_resolve_columns* c, uint64_t i) {
  UrRow r;
  r.hap = c->hap[i]; r.pos = c->pos[i]; r.strand = c->strand[i]; r.flags = c->flags[i];
  r.hap_len = r.hap < c->n_hap ? c->hap_len[r.hap] : 0u;
  for (int pl = 0; pl < UR_PLANES; ++pl) r.win[pl] = c->win[(uint64_t)pl * c->win_stride + i];
  return r;
}

int hawk_host_resolve_unphased(const hawk_resolve_columns* cols, const hawk_resolve_alleles* alleles, uint64_t batch_bytes,
                               uint32_t* row_resolved, uint32_t* row_kept, uint32_t* src_row, uint64_t* win, uint64_t out_cap,
                               uint64_t* n_out, uint64_t* n_resolved, hawk_resolve_decline* decline) {
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->row = -1; }
  if (!cols || !alleles || !n_out) return HAWK_E_INVALID;
  *n_out = 0;
  if (n_resolved) *n_resolved = 0;
  const uint64_t n = cols->n_rows;
  UrGeom g;
  g.pam_fwd = cols->pam_fwd; g.pam_rev = cols->pam_rev; g.guidelen = (int32_t)cols->guidelen; g.pamlen = (int32_t)cols->pamlen;
  g.right = cols->right ? 1 : 0; g.W = g.guidelen + g.pamlen + 2 * UR_PAD;
  if (cols->guidelen > 64 || cols->pamlen > 64) return HAWK_E_INVALID;
  const int bad = ur_check_geom(g);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  if (n && (!cols->hap || !cols->pos || !cols->strand || !cols->start || !cols->flags || !cols->win || !cols->hap_len || !cols->hap_is_ref ||
            cols->win_stride < n || n > 0xffffffffull))
    return HAWK_E_INVALID;
  UrAlleles al;
  al.key = alleles->key; al.off = alleles->off; al.ref = alleles->ref; al.n_keys = alleles->n_keys;
  if (!ur_check_alleles(al)) return HAWK_E_INVALID;
  for (uint64_t i = 0; i < n; ++i)
    if (cols->hap[i] >= cols->n_hap || cols->strand[i] > 1) return HAWK_E_INVALID;
  auto declined = [&](int reason, int64_t row) {
    if (decline) { decline->reason = reason; decline->row = row; }
    return (reason == UR_DECL_ROW_SIZE || reason == UR_DECL_BATCH) ? HAWK_E_CAPACITY : HAWK_E_UNSUPPORTED;
  };
  uint32_t n_ref = 0;
  for (uint32_t h = 0; h < cols->n_hap; ++h) n_ref += cols->hap_is_ref[h] ? 1u : 0u;
  if (n && n_ref > 1) return declined(UR_DECL_MULTI_REF, -1);
  std::vector<std::pair<uint64_t, uint32_t>> ref;  // (start * 2 + strand, row) of REF's rows, sorted
  for (uint64_t i = 0; i < n; ++i)
    if (cols->hap_is_ref[cols->hap[i]]) ref.emplace_back((uint64_t)cols->start[i] * 2u + cols->strand[i], (uint32_t)i);
  std::sort(ref.begin(), ref.end());
  auto partner = [&](uint64_t i, const UrRow& row, uint64_t* refwin) {
    if (!(row.flags & 1u) || cols->hap_is_ref[row.hap]) return false;
    const uint64_t want = (uint64_t)cols->start[i] * 2u + row.strand;
    auto it = std::lower_bound(ref.begin(), ref.end(), std::make_pair(want, (uint32_t)0));
    if (it == ref.end() || it->first != want) return false;
    const UrRow pr = ur_host_row(cols, it->second);
    UrCounts pc;
    if (ur_counts(pr, g, al, pr.win, false, &pc) != UR_DECL_NONE || pc.total == 0) return false;
    for (int pl = 0; pl < 4; ++pl) refwin[pl] = pr.win[pl];
    return true;
  };
  std::vector<uint32_t> res(n), kept(n);
  uint64_t total = 0, total_res = 0;
  const uint64_t bcap = batch_bytes / UR_OUT_BYTES;
  for (uint64_t i = 0; i < n; ++i) {
    const UrRow row = ur_host_row(cols, i);
    uint64_t refwin[4] = {0, 0, 0, 0};
    const bool has = partner(i, row, refwin);
    UrCounts c;
    int why = ur_counts(row, g, al, refwin, has, &c);
    if (!why && cols->hap_is_ref[row.hap] && c.total > 1) why = UR_DECL_REF_AMBIG;
    if (!why && c.total > UR_MAX_ROW) why = UR_DECL_ROW_SIZE;
    if (why) return declined(why, (int64_t)i);
    res[i] = (uint32_t)c.total; kept[i] = (uint32_t)(c.total - c.drop);
    total += kept[i]; total_res += res[i];
  }
  if (batch_bytes)
    for (uint64_t i = 0; i < n; ++i)
      if (kept[i] > bcap) return declined(UR_DECL_BATCH, (int64_t)i);
  *n_out = total;
  if (n_resolved) *n_resolved = total_res;
  if (row_resolved) std::copy(res.begin(), res.end(), row_resolved);
  if (row_kept) std::copy(kept.begin(), kept.end(), row_kept);
  if (!src_row && !win) return HAWK_OK;
  if (out_cap < total) return HAWK_E_CAPACITY;
  uint64_t o = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (!kept[i]) continue;
    const UrRow row = ur_host_row(cols, i);
    uint64_t refwin[4] = {0, 0, 0, 0}, w[UR_PLANES];
    const bool has = partner(i, row, refwin);
    for (uint32_t jk = 0; jk < kept[i]; ++jk, ++o) {
      ur_unrank(row, g, al, refwin, has, res[i], res[i] - kept[i], jk, w);
      if (has && ur_core_equal(w, refwin, g)) return HAWK_E_INVALID;  // the rule itself, on the words: a kept guide is never REF's core
      if (src_row) src_row[o] = (uint32_t)i;
      if (win)
        for (int pl = 0; pl < UR_PLANES; ++pl) win[(uint64_t)pl * out_cap + o] = w[pl];
    }
  }
  return HAWK_OK;
}

// ---- report groups of the kept guides (hawk_ugroups.h): the host twin of hawk_resolve_groups
int hawk_host_unphased_groups(const hawk_resolve_columns* cols, const int64_t* stop, const uint32_t* src_row, const uint64_t* win,
                              uint64_t n_kept, uint64_t win_stride, const double* cfd_mm, const double* cfd_pam, uint32_t flank_up,
                              uint32_t flank_down, uint64_t group_cap, uint64_t member_cap, uint32_t* rep_src_row, uint32_t* hap,
                              uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* out_stop, uint8_t* is_ref, double* cfdon,
                              uint64_t* out_win, uint8_t* gc_num, uint8_t* gc_den, uint64_t* member_off, uint32_t* member_hap,
                              uint64_t* n_groups, uint64_t* n_members) {
  if (n_groups) *n_groups = 0;
  if (n_members) *n_members = 0;
  if (!cols || !n_groups || !n_members || (cfd_mm && !cfd_pam)) return HAWK_E_INVALID;
  if (cols->guidelen > 64 || cols->pamlen > 64) return HAWK_E_INVALID;
  UgGeom g;
  g.guidelen = (int32_t)cols->guidelen; g.pamlen = (int32_t)cols->pamlen; g.right = cols->right ? 1 : 0;
  g.L = g.guidelen + g.pamlen; g.W = g.L + 2 * UG_PAD; g.up = (int32_t)flank_up; g.down = (int32_t)flank_down;
  const int bad = ug_check_geom(g, flank_up, flank_down);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  const uint64_t n = n_kept, nr = cols->n_rows;
  if (n > 0xffffffffull) return HAWK_E_UNSUPPORTED;
  if (n && (!src_row || !win || !stop || win_stride < n || !cols->hap || !cols->pos || !cols->strand || !cols->start || !cols->hap_is_ref ||
            nr > 0xffffffffull))
    return HAWK_E_INVALID;
  for (uint64_t k = 0; k < n; ++k)
    if (src_row[k] >= nr || cols->hap[src_row[k]] >= cols->n_hap || cols->strand[src_row[k]] > 1 || (k && src_row[k] < src_row[k - 1])) return HAWK_E_INVALID;
  // REF's kept guides by (start, strand): hawk_table_resolve_unphased declines a REF row of more than one
  std::vector<std::pair<uint64_t, uint64_t>> ref;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = src_row[k];
    if (cols->hap_is_ref[cols->hap[i]]) ref.emplace_back((uint64_t)cols->start[i] * 2u + cols->strand[i], k);
  }
  std::sort(ref.begin(), ref.end());
  struct Item { uint64_t key[UG_KEY_WORDS], hp, k; };
  std::vector<Item> items(n);
  std::vector<double> score(n, std::nan(""));
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = src_row[k];
    uint64_t w[UG_PLANES];
    for (int pl = 0; pl < UG_PLANES; ++pl) w[pl] = win[(uint64_t)pl * win_stride + k];
    Item& it = items[k];
    ug_key(g, cols->start[i], stop[i], cols->strand[i], cols->hap_is_ref[cols->hap[i]] != 0, w, it.key);
    it.hp = ((uint64_t)cols->hap[i] << 32) | cols->pos[i];
    it.k = k;
    if (!cfd_mm) continue;
    const uint64_t want = (uint64_t)cols->start[i] * 2u + cols->strand[i];
    auto p = std::lower_bound(ref.begin(), ref.end(), std::make_pair(want, (uint64_t)0));
    if (p == ref.end() || p->first != want) continue;
    uint64_t core[4], rcore[4];
    for (int pl = 0; pl < 4; ++pl) { core[pl] = ug_core(w[pl], g); rcore[pl] = ug_core(win[(uint64_t)pl * win_stride + p->second], g); }
    bool err;
    score[k] = ug_cfdon(core, rcore, cols->strand[i], g, cfd_mm, cfd_pam, &err);
    if (err) return HAWK_E_CFD;
  }
  std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
    for (int q = 0; q < UG_KEY_WORDS; ++q)
      if (a.key[q] != b.key[q]) return a.key[q] < b.key[q];
    return a.hp != b.hp ? a.hp < b.hp : a.k < b.k;
  });
  uint64_t ng = 0, nm = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const bool hg = !j || memcmp(items[j].key, items[j - 1].key, sizeof(items[j].key)) != 0;
    ng += hg ? 1 : 0;
    nm += (hg || (items[j].hp >> 32) != (items[j - 1].hp >> 32)) ? 1 : 0;
  }
  *n_groups = ng; *n_members = nm;
  const bool any = rep_src_row || hap || pos || strand || start || out_stop || is_ref || cfdon || out_win || gc_num || gc_den || member_off || member_hap;
  if (!any) return HAWK_OK;
  if (group_cap < ng || member_cap < nm) return HAWK_E_CAPACITY;
  uint64_t gi = 0, mi = 0;
  for (uint64_t j = 0; j < n; ++j) {
    const Item& it = items[j];
    const bool hg = !j || memcmp(it.key, items[j - 1].key, sizeof(it.key)) != 0;
    const bool hm = hg || (it.hp >> 32) != (items[j - 1].hp >> 32);
    if (hg) {
      const uint64_t k = it.k, i = src_row[k];
      uint64_t w[UG_PLANES];
      for (int pl = 0; pl < UG_PLANES; ++pl) w[pl] = win[(uint64_t)pl * win_stride + k];
      const uint32_t gc = ug_gc(w, cols->strand[i], g);
      if (rep_src_row) rep_src_row[gi] = (uint32_t)i;
      if (hap) hap[gi] = (uint32_t)(it.hp >> 32);
      if (pos) pos[gi] = (uint32_t)it.hp;
      if (strand) strand[gi] = (uint8_t)(it.key[1] >> 1);
      if (is_ref) is_ref[gi] = (uint8_t)(it.key[1] & 1u);
      if (start) start[gi] = ug_unbias(it.key[0]);
      if (out_stop) out_stop[gi] = ug_unbias(it.key[2]);
      if (cfdon) cfdon[gi] = score[k];
      if (out_win)
        for (int pl = 0; pl < UG_PLANES; ++pl) out_win[(uint64_t)pl * group_cap + gi] = w[pl];
      if (gc_num) gc_num[gi] = (uint8_t)(gc & 0xffu);
      if (gc_den) gc_den[gi] = (uint8_t)(gc >> 8);
      if (member_off) member_off[gi] = mi;
      ++gi;
    }
    if (hm) {
      if (member_hap) member_hap[mi] = (uint32_t)(it.hp >> 32);
      ++mi;
    }
  }
  if (member_off) member_off[ng] = nm;
  return HAWK_OK;
}

// ---- the whole-region rows of an unphased VCF (hawk_ubuild.h): the host twin of hawk_ubuild_lists / _signatures / _fill
int hawk_host_unphased_rows(const hawk_ubuild_input* in, hawk_ubuild_rows* out, hawk_ubuild_decline* decline) {
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->var = -1; }
  if (!in || !out) return HAWK_E_INVALID;
  out->n_rows = out->n_members = out->n_entries = out->n_keys = 0;
  const uint32_t ns = in->n_samples, nv = in->n_var;
  if (!ns || (in->n_lines && !in->codes) || (in->ref_len && !in->ref) ||
      (nv && (!in->var_line || !in->var_allele || !in->var_off || !in->var_mask || !in->var_ref)))
    return HAWK_E_INVALID;
  auto declined = [&](int reason, int64_t var) {
    if (decline) { decline->reason = reason; decline->var = var; }
    return reason == UB_DECL_ENTRIES ? HAWK_E_CAPACITY : HAWK_E_UNSUPPORTED;
  };
  for (uint32_t j = 0; j < nv; ++j) {
    if (in->var_line[j] >= in->n_lines || in->var_allele[j] == 0 || in->var_allele[j] == 255 || in->var_ref[j] > 3 || in->var_mask[j] > 15 ||
        (j && in->var_off[j] < in->var_off[j - 1]))
      return HAWK_E_INVALID;
  }
  for (uint32_t j = 0; j < nv; ++j)
    if (in->var_off[j] >= in->ref_len) return declined(UB_DECL_OUTSIDE, j);
  // the lists: per sample, ascending variant indices; REF is checked where a variant is carried, as the fill kernel does
  std::vector<uint64_t> off((size_t)ns + 1, 0);
  std::vector<uint32_t> idx;
  int64_t bad_ref = -1;
  for (uint32_t s = 0; s < ns; ++s) {
    for (uint32_t j = 0; j < nv; ++j) {
      const uint8_t* c = in->codes + ((size_t)in->var_line[j] * ns + s) * 2u;
      if (!ub_carried(c[0], c[1], in->var_allele[j])) continue;
      idx.push_back(j);
      if (ub_base_index((uint8_t)in->ref[in->var_off[j]]) != in->var_ref[j] && (bad_ref < 0 || (int64_t)j < bad_ref)) bad_ref = j;
    }
    off[s + 1] = idx.size();
    if (off[s + 1] > UB_MAX_ENTRIES) return declined(UB_DECL_ENTRIES, -1);
  }
  if (bad_ref >= 0) return declined(UB_DECL_REF, bad_ref);
  // merged sites and signatures; rows merge on the exact site sequence, first carrier first
  typedef std::vector<std::pair<uint32_t, uint32_t>> Sites;
  std::vector<Sites> sites(ns);
  std::vector<uint64_t> sig((size_t)ns * 2, 0);
  int64_t repeat = -1;
  for (uint32_t s = 0; s < ns; ++s) {
    for (uint64_t e = off[s]; e < off[s + 1]; ++e) {
      const uint32_t j = idx[e], refbit = 1u << in->var_ref[j];
      if (sites[s].empty() || sites[s].back().first != in->var_off[j]) sites[s].emplace_back(in->var_off[j], refbit);
      if (!ub_site_add(refbit, &sites[s].back().second, in->var_mask[j]) && (repeat < 0 || (int64_t)j < repeat)) repeat = j;
      sites[s].back().second |= (uint32_t)in->var_mask[j] | refbit;  // the expression k_ub_sig uses: every entry's ref bit and alt
    }
    for (const auto& st : sites[s]) ub_sig_add(st.first, st.second, &sig[2 * (size_t)s], &sig[2 * (size_t)s + 1]);
  }
  if (repeat >= 0) return declined(UB_DECL_REPEAT, repeat);
  std::vector<uint32_t> head;                 // first carrier of every distinct row
  std::vector<std::vector<uint32_t>> members;
  for (uint32_t s = 0; s < ns; ++s) {
    if (sites[s].empty()) continue;
    size_t k = 0;
    for (; k < head.size(); ++k)
      if (sig[2 * (size_t)head[k]] == sig[2 * (size_t)s] && sig[2 * (size_t)head[k] + 1] == sig[2 * (size_t)s + 1] && sites[head[k]] == sites[s]) break;
    if (k == head.size()) { head.push_back(s); members.emplace_back(); }
    members[k].push_back(s);
  }
  const uint64_t nr = head.size();
  uint64_t nm = 0, nk = 0, ne = 0;
  for (uint64_t k = 0; k < nr; ++k) { nm += members[k].size(); nk += sites[head[k]].size(); ne += off[head[k] + 1] - off[head[k]]; }
  out->n_rows = nr; out->n_members = nm; out->n_entries = idx.size(); out->n_keys = nk;
  if ((out->seqs || out->member_off) && out->row_cap < nr) return HAWK_E_CAPACITY;
  if (out->list_idx && out->entry_cap < idx.size()) return HAWK_E_CAPACITY;
  if ((out->al_key || out->al_off || out->al_ref) && out->entry_cap < ne) return HAWK_E_CAPACITY;
  if (out->sample_off) std::copy(off.begin(), off.end(), out->sample_off);
  if (out->list_idx) std::copy(idx.begin(), idx.end(), out->list_idx);
  if (out->sig) std::copy(sig.begin(), sig.end(), out->sig);
  static const char kCode[] = "?acmgrsvtwyhkdbn";  // a carried site is lower case
  uint64_t mi = 0, ki = 0, ei = 0;
  for (uint64_t k = 0; k < nr; ++k) {
    const uint32_t h = head[k];
    if (out->seqs) {
      char* row = out->seqs + k * (uint64_t)in->ref_len;
      memcpy(row, in->ref, in->ref_len);
      for (const auto& st : sites[h]) row[st.first] = kCode[st.second & 15u];
    }
    if (out->member_off) out->member_off[k] = (uint32_t)mi;
    for (uint32_t s : members[k]) {
      if (out->member_sample) out->member_sample[mi] = s;
      ++mi;
    }
    // the allele table of the first member: one key per carried position, one entry per carried allele there
    uint64_t e = off[h];
    for (const auto& st : sites[h]) {
      if (out->al_key) out->al_key[ki] = ((uint64_t)(in->row_base + k) << 32) | st.first;
      if (out->al_off) out->al_off[ki] = (uint32_t)ei;
      for (; e < off[h + 1] && in->var_off[idx[e]] == st.first; ++e, ++ei)
        if (out->al_ref) out->al_ref[ei] = in->var_ref[idx[e]];
      ++ki;
    }
  }
  if (out->member_off) out->member_off[nr] = (uint32_t)mi;
  if (out->al_off) out->al_off[nk] = (uint32_t)ei;
  return HAWK_OK;
}

// ---- the indel-window rows of an unphased VCF (hawk_uwin.h): the host twin of hawk_uwin_instances / _signatures / _group / _fill
int hawk_host_unphased_windows(const hawk_uwin_input* in, const hawk_uwin_lists* lists, hawk_uwin_rows* out, hawk_ubuild_decline* decline) {
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->var = -1; }
  if (!in || !lists || !out) return HAWK_E_INVALID;
  out->n_inst = out->n_rows = out->n_seq = 0;
  const uint32_t ni = in->n_indel, ns = lists->n_samples, L = in->region_len;
  if (!ns || !L || !in->ref || !in->rank_sample || !lists->sample_off || (lists->n_lines && !lists->codes)) return HAWK_E_INVALID;
  if (ni && (!in->line || !in->allele || !in->off || !in->ref_len || !in->alt_len || !in->pool_off || !in->pool)) return HAWK_E_INVALID;
  const uint64_t ne = lists->sample_off[ns];
  if (ne && (!lists->list_idx || !lists->var_off || !lists->var_mask || !lists->var_ref)) return HAWK_E_INVALID;
  for (uint32_t s = 0; s < ns; ++s)
    if (lists->sample_off[s + 1] < lists->sample_off[s]) return HAWK_E_INVALID;
  for (uint64_t e = 0; e < ne; ++e)
    if (lists->list_idx[e] >= lists->n_var || lists->var_off[lists->list_idx[e]] >= L || lists->var_ref[lists->list_idx[e]] > 3 ||
        lists->var_mask[lists->list_idx[e]] > 15)
      return HAWK_E_INVALID;
  for (uint32_t k = 0; k < ni; ++k)
    if (in->line[k] >= lists->n_lines || in->allele[k] == 0 || in->allele[k] == 255 ||
        (uint64_t)in->pool_off[k] + in->ref_len[k] + in->alt_len[k] > in->pool_len)
      return HAWK_E_INVALID;
  {
    std::vector<uint8_t> seen(ns, 0);
    for (uint32_t r = 0; r < ns; ++r) {
      if (in->rank_sample[r] >= ns || seen[in->rank_sample[r]]) return HAWK_E_INVALID;
      seen[in->rank_sample[r]] = 1;
    }
  }
  auto declined = [&](int reason, int64_t indel) {
    if (decline) { decline->reason = reason; decline->var = indel; }
    return HAWK_E_UNSUPPORTED;
  };
  const UwLists l{lists->list_idx, lists->var_off, lists->var_mask, lists->var_ref};
  // instances in (indel, name rank) order; an indel nobody carries is never looked at
  std::vector<uint64_t> inst_off((size_t)ni + 1, 0), lo, hi;
  std::vector<uint32_t> inst_indel, inst_sample;
  std::vector<UwGeom> geom(ni);
  for (uint32_t k = 0; k < ni; ++k) {
    bool checked = false;
    for (uint32_t r = 0; r < ns; ++r) {
      const uint32_t s = in->rank_sample[r];
      const uint8_t* c = lists->codes + ((size_t)in->line[k] * ns + s) * 2u;
      if (!ub_carried(c[0], c[1], in->allele[k])) continue;
      if (!checked) {
        const int why = uw_geometry(in->off[k], in->ref_len[k], in->alt_len[k], L, &geom[k]);
        if (why) return declined(why, k);
        if (!uw_bases_ok(in->pool + in->pool_off[k], in->ref_len[k] + in->alt_len[k])) return declined(UB_DECL_INDEL_BASE, k);
        checked = true;
      }
      const uint64_t a = uw_lower_bound(l, lists->sample_off[s], lists->sample_off[s + 1], geom[k].a);
      inst_indel.push_back(k); inst_sample.push_back(s);
      lo.push_back(a); hi.push_back(uw_lower_bound(l, a, lists->sample_off[s + 1], geom[k].b + 1u));
    }
    inst_off[k + 1] = inst_indel.size();
  }
  const uint64_t n = inst_indel.size();
  if (n >= 0xffffffffull) return HAWK_E_CAPACITY;
  std::vector<uint64_t> sig(2 * n, 0);
  for (uint64_t k = 0; k < n; ++k) {
    const UwGeom& g = geom[inst_indel[k]];
    uw_signature(l, g, lo[k], hi[k], &sig[2 * k], &sig[2 * k + 1]);
    if (uw_check_ref(l, g, lo[k], hi[k], (const uint8_t*)in->ref, in->pool + in->pool_off[inst_indel[k]])) return declined(UB_DECL_REF, inst_indel[k]);
  }
  const uint64_t* gs = out->forged_sig ? out->forged_sig : sig.data();
  std::vector<uint32_t> head(n);
  uint64_t nr = 0, nseq = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const UwGeom& g = geom[inst_indel[k]];
    uint64_t h = k;
    for (uint64_t c = inst_off[inst_indel[k]]; c < k; ++c)
      if (gs[2 * c] == gs[2 * k] && gs[2 * c + 1] == gs[2 * k + 1] && uw_same_row(l, g, lo[c], hi[c], lo[k], hi[k])) { h = c; break; }
    head[k] = (uint32_t)h;
    if (h == k) { ++nr; nseq += g.rowlen; }
  }
  out->n_inst = n; out->n_rows = nr; out->n_seq = nseq;
  if ((out->inst_sample || out->inst_lo || out->inst_hi || out->sig || out->head) && out->inst_cap < n) return HAWK_E_CAPACITY;
  if (out->seq_off && out->row_cap < nr) return HAWK_E_CAPACITY;
  if (out->seqs && out->seq_cap < nseq) return HAWK_E_CAPACITY;
  if (out->inst_off) std::copy(inst_off.begin(), inst_off.end(), out->inst_off);
  if (out->inst_sample) std::copy(inst_sample.begin(), inst_sample.end(), out->inst_sample);
  if (out->inst_lo) std::copy(lo.begin(), lo.end(), out->inst_lo);
  if (out->inst_hi) std::copy(hi.begin(), hi.end(), out->inst_hi);
  if (out->sig) std::copy(sig.begin(), sig.end(), out->sig);
  if (out->head) std::copy(head.begin(), head.end(), out->head);
  static const char kLower[] = "?acmgrsvtwyhkdbn";
  uint64_t ri = 0, si = 0;
  for (uint64_t k = 0; k < n; ++k) {
    if (head[k] != k) continue;
    const UwGeom& g = geom[inst_indel[k]];
    if (out->seq_off) out->seq_off[ri] = si;
    if (out->seqs) {
      char* row = out->seqs + si;
      const uint8_t* alt = in->pool + in->pool_off[inst_indel[k]] + in->ref_len[inst_indel[k]];
      for (uint32_t p = 0; p < g.rowlen; ++p) {
        const int64_t src = uw_source(g, p);
        row[p] = src >= 0 ? in->ref[src] : "acgt"[alt[-src - 1]];
      }
      uint64_t e = lo[k];
      uint32_t off, bits;
      while (uw_next_surviving(l, g, &e, hi[k], &off, &bits)) row[uw_site_pos(g, off)] = kLower[bits & 15u];
    }
    ++ri; si += g.rowlen;
  }
  if (out->seq_off) out->seq_off[nr] = si;
  return HAWK_OK;
}

// ---- BGZF members -> text on the host: the decoder of hawk_inflate.h as one lane, the members handed out to `threads` threads
int hawk_host_bgzf_inflate(const uint8_t* in, uint64_t in_bytes, const uint64_t* c_off, const uint64_t* u_off, uint32_t n_members,
                           uint8_t* out, uint8_t* status, uint32_t threads) {
  if (!bz_args_ok(in, in_bytes, c_off, u_off, n_members, out, status)) return HAWK_E_INVALID;
  if (!n_members) return HAWK_OK;
  unsigned nt = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
  nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min(nt, 32u), n_members));
  std::atomic<uint32_t> next(0), failed(0);
  auto work = [&]() {
    BzTables tables;
    for (;;) {
      const uint32_t k = next.fetch_add(1);
      if (k >= n_members) break;
      status[k] = (uint8_t)bz_inflate_member<BzHost>(in + c_off[k], c_off[k + 1] - c_off[k], out + u_off[k], u_off[k + 1] - u_off[k], &tables);
      if (status[k] != HAWK_BZ_OK) failed.fetch_add(1);
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
  }
  return failed.load() ? HAWK_E_INVALID : HAWK_OK;
}

}  // extern "C"
