// hawk_api_offtarget.hip - C ABI: the off-target scan (K7), its per-guide summary and its hits as the rows of the off-targets table
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "hawk_host.h"

// The spacer cut into nb blocks of G / nb bases (the first G % nb one longer); a block's key is its first <= kmax bases.
static void ot_blocks(int G, int nb, int kmax, int32_t* start, int32_t* klen, uint64_t* pmask2) {
  int startb = 0;
  for (int b = 0; b < nb; ++b) {
    const int len = G / nb + (b < G % nb ? 1 : 0), kl = std::min(len, kmax);
    start[b] = startb; klen[b] = kl;
    for (int t = 0; t < kl; ++t) pmask2[b] |= 1ull << (2 * (startb + t));
    startb += len;
  }
}

// The bucketed guide tables of the seeded match kernels, one counting sort per table t: its bucket offsets (4^key_bases(t) + 1)
// back to back in otoff from off_base[t], the guides' codes and ids in bucket order in row t of otcode / otid ([n_tables][n_guides]).
// A bucket keeps its guides in input order.
template <class KeyBases, class KeyOf>
static int ot_seed_tables(hawk_hapset* hs, const uint64_t* guides2, uint32_t n_guides, int n_tables, uint32_t* off_base,
                          KeyBases key_bases, KeyOf key_of) {
  std::vector<uint32_t> goff, keys(n_guides);
  std::vector<uint64_t> gcode((size_t)n_tables * n_guides, 0);
  std::vector<uint32_t> gid((size_t)n_tables * n_guides, 0);
  for (int t = 0; t < n_tables; ++t) {
    const uint32_t nkeys = 1u << (2 * key_bases(t));
    off_base[t] = (uint32_t)goff.size();
    std::vector<uint32_t> cnt(nkeys + 1, 0);
    for (uint32_t g = 0; g < n_guides; ++g) ++cnt[(keys[g] = key_of(t, guides2[g])) + 1];
    for (uint32_t v = 0; v < nkeys; ++v) cnt[v + 1] += cnt[v];
    goff.insert(goff.end(), cnt.begin(), cnt.end());
    std::vector<uint32_t> cur(cnt.begin(), cnt.end() - 1);
    for (uint32_t g = 0; g < n_guides; ++g) {
      const uint32_t slot = cur[keys[g]]++;
      gcode[(size_t)t * n_guides + slot] = guides2[g];
      gid[(size_t)t * n_guides + slot] = g;
    }
  }
  int rc;
  if ((rc = hs->otoff.reserve(goff.size() * 4)) || (rc = hs->otcode.reserve(gcode.size() * 8)) || (rc = hs->otid.reserve(gid.size() * 4)))
    return rc;
  hipStream_t st = hs->ctx->stream;
  HIPCHK(hipMemcpyAsync(hs->otoff.p, goff.data(), goff.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(hs->otcode.p, gcode.data(), gcode.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(hs->otid.p, gid.data(), gid.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));  // the host vectors go out of scope
  return HAWK_OK;
}

// The front half the four entry points share: argument checks, the choice of the match kernel and its bucketed guide tables, PAM
// scan -> site records (events 0..3 recorded), guides uploaded, the first 64 bytes of `misc` zeroed.  `m` names the kernel chosen
// and everything it reads: a caller hands it to a match launcher (hawk_device.h) with its sink, or its sites and guides to k_ot_bulge.
struct OtFront {
  hawk_ctx* ctx;
  OtMatchPlan m;
};
// `want_seeds` false: all pairs whatever the guide count, no bucketed tables (ot_bulge_front, whose p->guidelen is the SITE's spacer).
static int ot_front(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides, OtFront* f, bool want_seeds = true) {
  if (!hs || !p || !hs->has_meta || (n_guides && !guides2)) return HAWK_E_INVALID;
  if (hs->vplan) return HAWK_E_INVALID;  // a plan view holds no planes
  if (p->guidelen + p->pamlen > 32 || p->guidelen == 0) return HAWK_E_UNSUPPORTED;  // window code = 2 bits x 32
  hawk_ctx* ctx = f->ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  ScanParams sp;
  int rc = make_scan_params(hs, p->pam_fwd, p->pam_rev, p->pamlen, p->guidelen, p->right, false, &sp);
  if (rc) return rc;
  // windows are indexed by their start q: strand 0 stores the + strand as the guide reads it,
  // strand 1 the mirror image (same convention as the search, search_guides.py:538)
  sp.poF = p->right ? 0 : (int32_t)p->guidelen;
  sp.poR = p->right ? (int32_t)p->guidelen : 0;
  const HapSetDev d = make_dev(hs);
  const size_t words = (size_t)hs->n_hap * hs->S;
  const uint64_t ncnt = (uint64_t)hs->n_hap * 2 * sp.bph;
  if ((rc = hs->keepF.reserve(words * 4)) || (rc = hs->keepR.reserve(words * 4)) || (rc = hs->counts.reserve(ncnt * 4)) ||
      (rc = hs->offsets.reserve((ncnt + 1) * 8)) || (rc = hs->totals.reserve(sizeof(ScanTotals))) ||
      (rc = hs->partial.reserve((ncnt / 1024 + 2) * 8)) || (rc = hs->misc.reserve(512 * 8 + 64)) ||
      (rc = hs->guides.reserve(std::max<size_t>((size_t)n_guides * 8, 16))))
    return rc;
  // The match kernel is a function of (n_guides, max_mm, G) alone.  Pigeonhole seeds pay with enough guides to bucket and blocks
  // of at least two bases: pair seeds (max_mm + 2 blocks, k_ot_match_pairs) where they fit, else single-block seeds (max_mm + 1
  // blocks, k_ot_match_seeded).  All pairs otherwise; HAWK_OT_ALLPAIRS=1 (read per call) forces them, the reference the parity
  // tests compare the seeded kernels against.
  const char* e_all = getenv("HAWK_OT_ALLPAIRS");
  const int G = (int)p->guidelen, nb = (int)p->max_mm + 1;
  const bool seeded = want_seeds && !(e_all && e_all[0] == '1') && n_guides >= 64 && nb <= OT_MAX_BLOCKS && nb * 2 <= G;
  const bool pairs = seeded && nb + 1 <= OT_MAX_BLOCKS;  // (max_mm + 2 <= G follows from 2 (max_mm + 1) <= G)
  OtMatchPlan& m = f->m;
  memset(&m, 0, sizeof(m));
  m.kind = pairs ? OT_MATCH_PAIRS : seeded ? OT_MATCH_SEEDED : OT_MATCH_ALL;
  m.n_guides = n_guides; m.guidelen = G; m.sp0 = p->right ? (int)p->pamlen : 0; m.max_mm = (int)p->max_mm;
  OtSeeds& sd = m.sd;
  OtPairSeeds& ps = m.ps;
  if (pairs) {
    ps.nb = nb + 1;
    ot_blocks(G, ps.nb, 4, ps.start, ps.klen, ps.pmask2);
    for (int bi = 0; bi < ps.nb; ++bi)
      for (int bj = bi + 1; bj < ps.nb; ++bj) { ps.pi[ps.n_pairs] = (uint8_t)bi; ps.pj[ps.n_pairs] = (uint8_t)bj; ++ps.n_pairs; }
    // pair q's key: the key bases of block pi[q], then those of block pj[q]
    rc = ot_seed_tables(hs, guides2, n_guides, ps.n_pairs, ps.off_base, [&](int q) { return ps.klen[ps.pi[q]] + ps.klen[ps.pj[q]]; },
                        [&](int q, uint64_t c) {
                          const int bi = ps.pi[q], bj = ps.pj[q];
                          const uint32_t ki = (uint32_t)(c >> (2 * ps.start[bi])) & ((1u << (2 * ps.klen[bi])) - 1u);
                          const uint32_t kj = (uint32_t)(c >> (2 * ps.start[bj])) & ((1u << (2 * ps.klen[bj])) - 1u);
                          return ki | (kj << (2 * ps.klen[bi]));
                        });
  } else if (seeded) {
    sd.nb = nb;
    ot_blocks(G, nb, 6, sd.start, sd.klen, sd.pmask2);
    rc = ot_seed_tables(hs, guides2, n_guides, nb, sd.off_base, [&](int b) { return sd.klen[b]; },
                        [&](int b, uint64_t c) { return (uint32_t)(c >> (2 * sd.start[b])) & ((1u << (2 * sd.klen[b])) - 1u); });
  }
  if (rc) return rc;
  hipEvent_t* ev = ctx->ev;
  if (n_guides) HIPCHK(hipMemcpyAsync(hs->guides.p, guides2, (size_t)n_guides * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(hs->misc.p, 0, 64, ctx->stream));
  HIPCHK(hipEventRecord(ev[0], ctx->stream));
  hawk_launch_scan_raw(ctx->stream, d, sp, hs->keepF.as<uint32_t>(), hs->keepR.as<uint32_t>(), hs->counts.as<uint32_t>());
  hawk_launch_mscan(ctx->stream, hs->counts.as<uint32_t>(), ncnt, hs->partial.as<unsigned long long>(), nullptr,
                    hs->offsets.as<uint64_t>(), hs->totals.as<ScanTotals>());
  HIPCHK(hipEventRecord(ev[1], ctx->stream));
  HIPCHK(hipGetLastError());
  ScanTotals tot;
  HIPCHK(hipMemcpyAsync(&tot, hs->totals.p, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const uint64_t nsites = m.n_sites = tot.n_keep;
  if ((rc = hs->sites.reserve(std::max<uint64_t>(nsites, 1) * sizeof(OtSite)))) return rc;
  HIPCHK(hipEventRecord(ev[2], ctx->stream));
  if (nsites) hawk_launch_ot_sites(ctx->stream, d, sp, hs->keepF.as<uint32_t>(), hs->keepR.as<uint32_t>(),
                                   hs->offsets.as<uint64_t>(), hs->sites.as<OtSite>());
  HIPCHK(hipEventRecord(ev[3], ctx->stream));
  m.sites = hs->sites.as<OtSite>(); m.guides = hs->guides.as<uint64_t>();
  m.goff = hs->otoff.as<uint32_t>(); m.gcode = hs->otcode.as<uint64_t>(); m.gid = hs->otid.as<uint32_t>();
  return HAWK_OK;
}
// events 0..4 -> hawk_ot_timing; the match kernel ran between events m0 and 4
static void ot_timing(hawk_hapset* hs, uint64_t nsites, hawk_ot_timing* timing, int m0 = 3) {
  if (!timing) return;
  hipEvent_t* ev = hs->ctx->ev;
  memset(timing, 0, sizeof(*timing));
  (void)hipEventElapsedTime(&timing->scan_ms, ev[0], ev[1]);
  (void)hipEventElapsedTime(&timing->sites_ms, ev[2], ev[3]);
  (void)hipEventElapsedTime(&timing->match_ms, ev[m0], ev[4]);
  (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[4]);
  timing->n_sites = nsites;
  uint64_t pos = 0;
  for (uint32_t h = 0; h < hs->n_hap; ++h) pos += (uint64_t)std::max(0, hs->scan_stop[h] - hs->scan_start[h]);
  timing->scanned_positions = pos;
}

// The summaries' block in hs->otsum, sized by the guides alone: counters[2] | cfd_e4[n_guides] | CFD tables[336] |
// hist[n_guides][stride].  No hits / othit buffer and no cap on this path: a hit ends in these sums inside the kernel that finds
// it.  otsum_begin reserves the block, zeroes it, uploads the tables (both or neither) on the stream, points the sink's shared
// fields (OtSumOut) into it and records event 5: the zeroing and the upload are not the kernel's time.  otsum_end, after the
// kernel: event 4, one download, synchronise, the caller's outputs and the timing.
struct OtSumBlock {
  char* base;
  size_t off_tab, off_hist, bytes;
  uint32_t n_guides, stride;
  bool tables;
};
// The summaries' argument rules.
static int ot_sum_args(const hawk_ot_params* p, uint32_t n_guides, const double* cfd_mm, const double* cfd_pam, const uint32_t* out_hist,
                       const int64_t* out_cfd_e4, const uint64_t* n_hits, const uint64_t* n_unscorable) {
  if (!n_hits || !n_unscorable || (n_guides && !out_hist) || !cfd_mm != !cfd_pam || (cfd_mm && n_guides && !out_cfd_e4)) return HAWK_E_INVALID;
  if (p && ((cfd_mm && p->pamlen < 2) || p->max_mm > 32)) return HAWK_E_UNSUPPORTED;  // the PAM table is keyed by PAM[-2:]; a window has <= 32 bases
  return HAWK_OK;
}
static int otsum_begin(hawk_hapset* hs, uint32_t n_guides, uint32_t stride, const double* cfd_mm, const double* cfd_pam, OtSumBlock* b,
                       OtSumOut* sm) {
  hipStream_t st = hs->ctx->stream;
  b->n_guides = n_guides; b->stride = stride; b->tables = cfd_mm != nullptr;
  b->off_tab = 16 + (size_t)n_guides * 8;
  b->off_hist = b->off_tab + 336 * 8;
  b->bytes = b->off_hist + (size_t)n_guides * stride * 4;
  int rc;
  if ((rc = hs->otsum.reserve(b->bytes))) return rc;
  b->base = hs->otsum.as<char>();
  HIPCHK(hipMemsetAsync(b->base, 0, b->bytes, st));
  if (cfd_mm) {
    HIPCHK(hipMemcpyAsync(b->base + b->off_tab, cfd_mm, 320 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->base + b->off_tab + 320 * 8, cfd_pam, 16 * 8, hipMemcpyHostToDevice, st));
  }
  sm->counters = reinterpret_cast<unsigned long long*>(b->base);
  sm->cfd_e4 = reinterpret_cast<unsigned long long*>(b->base + 16);
  sm->tab = cfd_mm ? reinterpret_cast<const double*>(b->base + b->off_tab) : nullptr;
  sm->hist = reinterpret_cast<uint32_t*>(b->base + b->off_hist);
  sm->stride = stride;
  HIPCHK(hipEventRecord(hs->ctx->ev[5], st));
  return HAWK_OK;
}
static int otsum_end(hawk_hapset* hs, const OtFront& f, const OtSumBlock& b, uint32_t* out_hist, int64_t* out_cfd_e4, uint64_t* n_hits,
                     uint64_t* n_unscorable, hawk_ot_timing* timing) {
  hipStream_t st = hs->ctx->stream;
  HIPCHK(hipEventRecord(hs->ctx->ev[4], st));
  HIPCHK(hipGetLastError());
  // one download: everything but the tables would do, the block is small either way
  std::vector<char> host(b.bytes);
  HIPCHK(hipMemcpyAsync(host.data(), b.base, b.bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t cnt[2];
  memcpy(cnt, host.data(), 16);
  *n_hits = cnt[0];
  *n_unscorable = cnt[1];
  if (b.n_guides) {
    memcpy(out_hist, host.data() + b.off_hist, (size_t)b.n_guides * b.stride * 4);
    if (out_cfd_e4 && b.tables) memcpy(out_cfd_e4, host.data() + 16, (size_t)b.n_guides * 8);
    else if (out_cfd_e4) memset(out_cfd_e4, 0, (size_t)b.n_guides * 8);
  }
  ot_timing(hs, f.m.n_sites, timing, 5);
  return HAWK_OK;
}

// The front of the two bulged entry points: p->guidelen is the GUIDE's, the window scan is about the site's spacer.  Refusals in
// this order: type / size (INVALID), lengths (UNSUPPORTED), then metadata, view, scan ranges and what ot_front refuses.
static bool otb_kind_ok(uint32_t bulge_type, uint32_t bulge_size) { return bulge_type >= 1 && bulge_type <= 2 && bulge_size >= 1 && bulge_size <= 2; }
static int ot_bulge_front(hawk_hapset* hs, const hawk_ot_params* p, uint32_t bulge_type, uint32_t bulge_size, const uint64_t* guides2,
                          uint32_t n_guides, OtFront* f, int* G_out, int* dna_out) {
  if (!hs || !p || !otb_kind_ok(bulge_type, bulge_size)) return HAWK_E_INVALID;
  const bool dna = bulge_type == 1;
  const uint32_t G = p->guidelen;
  if (G > 32 || G < bulge_size + 3) return HAWK_E_UNSUPPORTED;  // a guide code is 2 bits x 32; two end bases and one interior base stay paired
  hawk_ot_params ps = *p;
  const uint32_t Gs = ps.guidelen = dna ? G + bulge_size : G - bulge_size;  // the site's spacer: what the window scan is about
  if (Gs + p->pamlen > 32) return HAWK_E_UNSUPPORTED;
  // the rows' scan ranges must be those of windows of Gs + pamlen bases (hawk_hapset_set_meta): a window that starts inside a
  // range set for a shorter window would reach past its row
  if (!hs->has_meta || hs->vplan) return HAWK_E_INVALID;  // a plan view holds no planes
  for (uint32_t h = 0; h < hs->n_hap; ++h)
    if (hs->scan_stop[h] > hs->scan_start[h] && (int64_t)hs->scan_stop[h] - 1 + Gs + p->pamlen > (int64_t)hs->hap_len[h]) return HAWK_E_INVALID;
  *G_out = (int)G;
  *dna_out = dna ? 1 : 0;
  return ot_front(hs, &ps, guides2, n_guides, f, false);
}

// What follows a list sink's kernel, Hit = OtHit or OtBulgeHit: event 4, the count read back (*n_out; HAWK_E_CAPACITY past `cap`),
// the timing, then the hits and their sites - gathered into a compact array on the device - in two downloads behind one
// synchronise, scattered into the columns asked for (each may be null; `gaps` exists for bulged hits only).
struct OtCols {
  uint32_t *guide, *row, *q;
  uint8_t *strand, *mm;
  uint64_t* code;
  uint32_t* nmask;
  uint64_t* gaps;
};
template <class Hit>
static int ot_download(hawk_hapset* hs, const OtFront& f, const OtCols& o, uint64_t cap, uint64_t* n_out, hawk_ot_timing* timing) {
  hipStream_t st = f.ctx->stream;
  HIPCHK(hipEventRecord(f.ctx->ev[4], st));
  HIPCHK(hipGetLastError());
  unsigned long long nh = 0;
  HIPCHK(hipMemcpyAsync(&nh, hs->misc.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *n_out = nh;
  ot_timing(hs, f.m.n_sites, timing);
  if (nh > cap) return HAWK_E_CAPACITY;
  if (!nh) return HAWK_OK;
  std::vector<Hit> hh(nh);
  std::vector<OtSite> ss(nh);
  int rc;
  if ((rc = hs->othit.reserve(nh * sizeof(OtSite)))) return rc;
  hawk_launch_ot_gather(st, f.m.sites, hs->hits.as<Hit>(), nh, hs->othit.as<OtSite>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hh.data(), hs->hits.p, nh * sizeof(Hit), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(ss.data(), hs->othit.p, nh * sizeof(OtSite), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t i = 0; i < nh; ++i) {
    if (o.guide) o.guide[i] = hh[i].guide;
    if (o.row) o.row[i] = ss[i].row;
    if (o.q) o.q[i] = ss[i].q & 0x7fffffffu;
    if (o.strand) o.strand[i] = (uint8_t)(ss[i].q >> 31);
    if (o.mm) o.mm[i] = (uint8_t)hh[i].mm;
    if (o.code) o.code[i] = ss[i].code;
    if (o.nmask) o.nmask[i] = ss[i].nmask;
    if constexpr (std::is_same<Hit, OtBulgeHit>::value)
      if (o.gaps) o.gaps[i] = hh[i].gaps;
  }
  return HAWK_OK;
}

extern "C" {

// ---------------------------------------------------------------------------- K7 off-targets
int hawk_genome_finalize(hawk_hapset* rows) {
  if (!rows || rows->vplan) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(rows->ctx->device));
  hawk_launch_ot_onehot(rows->ctx->stream, rows->plane, (uint64_t)rows->n_hap * rows->S);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(rows->ctx->stream));
  rows->finalized = true;
  return HAWK_OK;
}

int hawk_offtarget_scan(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                        uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand, uint8_t* out_mm,
                        uint64_t* out_code, uint32_t* out_nmask, uint64_t cap, uint64_t* n_out, hawk_ot_timing* timing) {
  if (!n_out) return HAWK_E_INVALID;
  OtFront f;
  int rc = ot_front(hs, p, guides2, n_guides, &f);
  if (rc) return rc;
  if ((rc = hs->hits.reserve(std::max<uint64_t>(cap, 1) * sizeof(OtHit)))) return rc;
  hawk_launch_ot_match(f.ctx->stream, f.m, hs->hits.as<OtHit>(), cap, hs->misc.as<unsigned long long>());
  return ot_download<OtHit>(hs, f, {out_guide, out_row, out_q, out_strand, out_mm, out_code, out_nmask, nullptr}, cap, n_out, timing);
}

int hawk_offtarget_bulges(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides, uint32_t bulge_type,
                          uint32_t bulge_size, uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand,
                          uint8_t* out_mm, uint64_t* out_code, uint32_t* out_nmask, uint64_t* out_gaps, uint64_t cap, uint64_t* n_out,
                          hawk_ot_timing* timing) {
  if (!n_out) return HAWK_E_INVALID;
  OtFront f;
  int G, dna;
  int rc = ot_bulge_front(hs, p, bulge_type, bulge_size, guides2, n_guides, &f, &G, &dna);
  if (rc) return rc;
  // sized by the rows asked for and (ot_front) by the guides: nothing here grows with the placements
  if ((rc = hs->hits.reserve(std::max<uint64_t>(cap, 1) * sizeof(OtBulgeHit)))) return rc;
  hawk_launch_ot_bulge(f.ctx->stream, f.m.sites, f.m.n_sites, f.m.guides, n_guides, G, f.m.sp0, f.m.max_mm, dna, (int)bulge_size,
                       hs->hits.as<OtBulgeHit>(), cap, hs->misc.as<unsigned long long>());
  return ot_download<OtBulgeHit>(hs, f, {out_guide, out_row, out_q, out_strand, out_mm, out_code, out_nmask, out_gaps}, cap, n_out, timing);
}

int hawk_offtarget_summary(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides, const double* cfd_mm,
                           const double* cfd_pam, uint32_t* out_hist, int64_t* out_cfd_e4, uint64_t* n_hits, uint64_t* n_unscorable,
                           hawk_ot_timing* timing) {
  int rc = ot_sum_args(p, n_guides, cfd_mm, cfd_pam, out_hist, out_cfd_e4, n_hits, n_unscorable);
  if (rc) return rc;
  OtFront f;
  if ((rc = ot_front(hs, p, guides2, n_guides, &f))) return rc;
  OtSumBlock blk;
  OtSummary sm;
  if ((rc = otsum_begin(hs, n_guides, p->max_mm + 1, cfd_mm, cfd_pam, &blk, &sm))) return rc;
  sm.sites = f.m.sites;
  sm.sp0 = f.m.sp0;
  sm.pam2 = (p->right ? 0 : f.m.guidelen) + (int)p->pamlen - 2;
  sm.ncmp = std::min(f.m.guidelen, 20);
  hawk_launch_ot_match_sum(f.ctx->stream, f.m, sm);
  return otsum_end(hs, f, blk, out_hist, out_cfd_e4, n_hits, n_unscorable, timing);
}

int hawk_offtarget_bulge_summary(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides, uint32_t bulge_type,
                                 uint32_t bulge_size, const double* cfd_mm, const double* cfd_pam, uint32_t* out_hist, int64_t* out_cfd_e4,
                                 uint64_t* n_hits, uint64_t* n_unscorable, hawk_ot_timing* timing) {
  // a missing handle and a bulge that is none are refused before the summaries' UNSUPPORTED
  if (!hs || !p || !otb_kind_ok(bulge_type, bulge_size)) return HAWK_E_INVALID;
  int rc = ot_sum_args(p, n_guides, cfd_mm, cfd_pam, out_hist, out_cfd_e4, n_hits, n_unscorable);
  if (rc) return rc;
  OtFront f;
  int G, dna;
  if ((rc = ot_bulge_front(hs, p, bulge_type, bulge_size, guides2, n_guides, &f, &G, &dna))) return rc;
  OtSumBlock blk;
  OtBulgeSummary sm;
  if ((rc = otsum_begin(hs, n_guides, p->max_mm + 1, cfd_mm, cfd_pam, &blk, &sm))) return rc;
  sm.pamlen = (int32_t)p->pamlen;
  sm.right = p->right ? 1 : 0;
  hawk_launch_ot_bulge_sum(f.ctx->stream, f.m.sites, f.m.n_sites, f.m.guides, n_guides, G, f.m.sp0, f.m.max_mm, dna, (int)bulge_size, sm);
  return otsum_end(hs, f, blk, out_hist, out_cfd_e4, n_hits, n_unscorable, timing);
}

// ---------------------------------------------------------------------------- the off-targets table as text (hawk_ottext.hip)
// The rows of the last hawk_offtarget_text of a context, in HBM until hawk_offtarget_text_download fetches them.
namespace {
struct OtTextState {
  DevBuf off, out, cfd, partial, cnt;
  uint64_t n = 0, bytes = 0;
  bool has_result = false;
};
std::mutex g_ott_mu;
std::map<hawk_ctx*, OtTextState> g_ott;
OtTextState* ott_state(hawk_ctx* ctx) {
  std::lock_guard<std::mutex> g(g_ott_mu);
  return &g_ott[ctx];
}
}  // namespace

}  // extern "C"
void hawk_ottext_forget(hawk_ctx* ctx) {
  std::lock_guard<std::mutex> g(g_ott_mu);
  auto it = g_ott.find(ctx);
  if (it == g_ott.end()) return;
  for (DevBuf* b : {&it->second.off, &it->second.out, &it->second.cfd, &it->second.partial, &it->second.cnt}) b->release();
  g_ott.erase(it);
}
extern "C" {

int hawk_offtarget_text(hawk_ctx* ctx, uint64_t n, const uint32_t* guide, const uint32_t* row, const uint32_t* q, const uint8_t* strand,
                        const uint8_t* mm, const uint64_t* code, const uint32_t* nmask, const uint64_t* gaps, const uint8_t* kind,
                        const uint8_t* size, const uint64_t* guides2, uint32_t n_guides, const hawk_ot_params* p,
                        const uint32_t* row_contig, const uint64_t* row_off, uint32_t n_table_rows, const uint8_t* name_blob,
                        const uint64_t* name_off, uint32_t n_contigs, const char* pam_text, const uint64_t* order, const double* cfd_mm,
                        const double* cfd_pam, uint64_t* n_bytes, uint64_t* n_unscorable, hawk_ot_text_timing* timing) {
  if (!ctx || !p || !n_bytes || !n_unscorable || !cfd_mm != !cfd_pam || (p->pamlen && !pam_text)) return HAWK_E_INVALID;
  if (n && (!guides2 || !row_off)) return HAWK_E_INVALID;
  if (p->guidelen == 0 || p->guidelen > 32 || p->guidelen + p->pamlen > 32) return HAWK_E_UNSUPPORTED;  // a window code is 2 bits x 32
  if (cfd_mm && p->pamlen < 2) return HAWK_E_UNSUPPORTED;  // as hawk_offtarget_summary: the PAM table is keyed by PAM[-2:]
  OtTextFmt fmt;
  memset(&fmt, 0, sizeof(fmt));
  fmt.G = p->guidelen; fmt.P = p->pamlen; fmt.right = p->right ? 1u : 0u;
  for (uint32_t k = 0; k < p->pamlen; ++k) fmt.pam[k] = (uint8_t)pam_text[k];
  // every index a kernel would follow is checked here, before anything is written
  const OtTextCols cols = {guide, row, q, nmask, code, gaps, strand, mm, kind, size};
  if (!ot_text_check(n, cols, fmt, n_guides, row_contig, n_table_rows, name_blob, name_off, n_contigs, order)) return HAWK_E_INVALID;
  OtTextState* S = ott_state(ctx);
  S->has_result = false;
  *n_bytes = 0;
  *n_unscorable = 0;
  if (timing) memset(timing, 0, sizeof(*timing));
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  int rc;
  if ((rc = S->off.reserve((n + 1) * 8)) || (rc = S->cfd.reserve(std::max<uint64_t>(n, 1) * 8)) ||
      (rc = S->partial.reserve(std::max<uint64_t>(hawk_ann_scan_blocks(n), 1) * 8)) || (rc = S->cnt.reserve(8)))
    return rc;
  if (!n) {
    HIPCHK(hipMemsetAsync(S->off.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    S->n = 0; S->bytes = 0; S->has_result = true;
    return HAWK_OK;
  }
  // the inputs of this call: back to the pool when it returns (the stream is drained by then)
  PoolScope tmp;
  OtTextDev A;
  memset(&A, 0, sizeof(A));
  A.fmt = fmt;
  A.n = n;
  const uint64_t nbytes_names = name_off[n_contigs];
  uint32_t *d_guide, *d_row, *d_q, *d_nmask, *d_rc;
  uint64_t *d_code, *d_gaps, *d_order = nullptr, *d_g2, *d_roff, *d_noff;
  uint8_t *d_strand, *d_mm, *d_kind, *d_size, *d_names;
  double* d_tab = nullptr;
  TEMPCHK(tmp, &d_guide, n * 4); TEMPCHK(tmp, &d_row, n * 4); TEMPCHK(tmp, &d_q, n * 4); TEMPCHK(tmp, &d_nmask, n * 4);
  TEMPCHK(tmp, &d_code, n * 8); TEMPCHK(tmp, &d_gaps, n * 8);
  TEMPCHK(tmp, &d_strand, n); TEMPCHK(tmp, &d_mm, n); TEMPCHK(tmp, &d_kind, n); TEMPCHK(tmp, &d_size, n);
  if (order) TEMPCHK(tmp, &d_order, n * 8);
  TEMPCHK(tmp, &d_g2, (size_t)n_guides * 8);
  TEMPCHK(tmp, &d_rc, (size_t)n_table_rows * 4); TEMPCHK(tmp, &d_roff, (size_t)n_table_rows * 8);
  TEMPCHK(tmp, &d_names, std::max<uint64_t>(nbytes_names, 1)); TEMPCHK(tmp, &d_noff, ((size_t)n_contigs + 1) * 8);
  if (cfd_mm) TEMPCHK(tmp, &d_tab, 336 * 8);
  HIPCHK(hipMemsetAsync(S->cnt.p, 0, 8, st));
  HIPCHK(hipEventRecord(ev[0], st));
#define OTT_UP(dstp, srcp, bytes) HIPCHK(hipMemcpyAsync((dstp), (srcp), (bytes), hipMemcpyHostToDevice, st))
  OTT_UP(d_guide, guide, n * 4); OTT_UP(d_row, row, n * 4); OTT_UP(d_q, q, n * 4); OTT_UP(d_nmask, nmask, n * 4);
  OTT_UP(d_code, code, n * 8); OTT_UP(d_gaps, gaps, n * 8);
  OTT_UP(d_strand, strand, n); OTT_UP(d_mm, mm, n); OTT_UP(d_kind, kind, n); OTT_UP(d_size, size, n);
  if (order) OTT_UP(d_order, order, n * 8);
  OTT_UP(d_g2, guides2, (size_t)n_guides * 8);
  OTT_UP(d_rc, row_contig, (size_t)n_table_rows * 4); OTT_UP(d_roff, row_off, (size_t)n_table_rows * 8);
  if (nbytes_names) OTT_UP(d_names, name_blob, nbytes_names);
  OTT_UP(d_noff, name_off, ((size_t)n_contigs + 1) * 8);
  if (cfd_mm) { OTT_UP(d_tab, cfd_mm, 320 * 8); OTT_UP(d_tab + 320, cfd_pam, 16 * 8); }
#undef OTT_UP
  A.guide = d_guide; A.row = d_row; A.q = d_q; A.nmask = d_nmask; A.code = d_code; A.gaps = d_gaps;
  A.strand = d_strand; A.mm = d_mm; A.kind = d_kind; A.size = d_size; A.order = d_order; A.guides2 = d_g2;
  A.row_contig = d_rc; A.row_off = d_roff; A.names = d_names; A.name_off = d_noff; A.tab = d_tab;
  HIPCHK(hipEventRecord(ev[1], st));
  hawk_launch_ot_text_len(st, A, S->off.as<uint64_t>(), S->cfd.as<int64_t>(), S->cnt.as<unsigned long long>());
  HIPCHK(hipEventRecord(ev[2], st));
  hawk_launch_ann_offsets(st, S->off.as<uint64_t>(), n, S->partial.as<uint64_t>());
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&tot[0], S->off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[1], S->cnt.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the blob's size decides its allocation
  if ((rc = S->out.reserve(std::max<uint64_t>(tot[0], 1)))) return rc;
  HIPCHK(hipEventRecord(ev[4], st));
  hawk_launch_ot_text_fill(st, A, S->off.as<uint64_t>(), S->out.as<uint8_t>());
  HIPCHK(hipEventRecord(ev[5], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  S->n = n; S->bytes = tot[0]; S->has_result = true;
  *n_bytes = tot[0];
  *n_unscorable = tot[1];
  if (timing) {
    (void)hipEventElapsedTime(&timing->upload_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&timing->len_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&timing->scan_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&timing->fill_ms, ev[4], ev[5]);
    (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[5]);
    timing->out_bytes = tot[0];
    timing->n_rows = n;
  }
  return HAWK_OK;
}

int hawk_offtarget_text_download(hawk_ctx* ctx, uint8_t* blob, uint64_t* off, int64_t* cfd_e4, float* download_ms) {
  if (!ctx || !off) return HAWK_E_INVALID;
  OtTextState* S = ott_state(ctx);
  if (!S->has_result || (S->bytes && !blob) || (S->n && !cfd_e4)) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (S->bytes) HIPCHK(hipMemcpyAsync(blob, S->out.p, S->bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(off, S->off.p, (S->n + 1) * 8, hipMemcpyDeviceToHost, st));
  if (S->n) HIPCHK(hipMemcpyAsync(cfd_e4, S->cfd.p, S->n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipStreamSynchronize(st));
  if (download_ms) (void)hipEventElapsedTime(download_ms, ctx->ev[0], ctx->ev[1]);
  // the workspace goes back to the caching allocator: the table of a bulged search is tens of MB
  S->has_result = false;
  S->out.release(); S->off.release(); S->cfd.release(); S->partial.release();
  return HAWK_OK;
}

}  // extern "C"
