// hawk_api_otvar.hip - C ABI: SNVs added to a genome index and the off-target scan over the enriched genome (include/hawk.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hawk_host.h"

static OvPlanes ov_planes(const hawk_hapset* hs) {
  OvPlanes al;
  for (int b = 0; b < 4; ++b) al.p[b] = hs->ovplane[b].as<uint32_t>();
  return al;
}

extern "C" {

int hawk_genome_variants(hawk_hapset* rows, const uint32_t* row, const uint32_t* q, const uint8_t* ref, const uint8_t* alt, uint64_t n,
                         uint8_t* status, uint64_t* n_applied, uint64_t* n_dropped) {
  if (!rows || rows->vplan || !rows->finalized || !n_applied || !n_dropped || (n && (!row || !q || !ref || !alt))) return HAWK_E_INVALID;
  // every index the kernel follows is checked here, before anything is written
  for (uint64_t i = 0; i < n; ++i)
    if (row[i] >= rows->n_hap || q[i] >= rows->hap_len[row[i]] || ref[i] > 3 || alt[i] > 3) return HAWK_E_INVALID;
  hawk_ctx* ctx = rows->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t words = (size_t)rows->n_hap * rows->S;
  int rc;
  if (!rows->has_variants) {  // the allele planes start as REF's one-hot planes: every allele set holds its REF base
    for (int b = 0; b < 4; ++b) {
      if ((rc = rows->ovplane[b].reserve(words * 4))) return rc;
      HIPCHK(hipMemcpyAsync(rows->ovplane[b].p, rows->plane[b], words * 4, hipMemcpyDeviceToDevice, st));
    }
    rows->has_variants = true;
  }
  *n_applied = 0;
  *n_dropped = 0;
  if (!n) { HIPCHK(hipStreamSynchronize(st)); return HAWK_OK; }
  PoolScope tmp;
  uint32_t *d_row, *d_q;
  uint8_t *d_ref, *d_alt, *d_st;
  TEMPCHK(tmp, &d_row, n * 4); TEMPCHK(tmp, &d_q, n * 4); TEMPCHK(tmp, &d_ref, n); TEMPCHK(tmp, &d_alt, n); TEMPCHK(tmp, &d_st, n);
  HIPCHK(hipMemcpyAsync(d_row, row, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_q, q, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ref, ref, n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_alt, alt, n, hipMemcpyHostToDevice, st));
  hawk_launch_ov_fill(st, make_dev(rows), ov_planes(rows), d_row, d_q, d_ref, d_alt, n, d_st);
  HIPCHK(hipGetLastError());
  std::vector<uint8_t> h_st(n);
  HIPCHK(hipMemcpyAsync(h_st.data(), d_st, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint64_t ok = 0;
  for (uint64_t i = 0; i < n; ++i) ok += h_st[i] == HAWK_OV_APPLIED;
  *n_applied = ok;
  *n_dropped = n - ok;
  if (status) memcpy(status, h_st.data(), n);
  return HAWK_OK;
}

int hawk_offtarget_variant_scan(hawk_hapset* hs, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides, uint32_t* out_guide,
                                uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand, uint8_t* out_mm, uint64_t* out_code,
                                uint32_t* out_nmask, uint32_t* out_alt, uint64_t cap, uint64_t* n_out, hawk_ot_timing* timing) {
  if (!hs || !p || !n_out || !hs->has_meta || hs->vplan || !hs->has_variants || (n_guides && !guides2)) return HAWK_E_INVALID;
  if (p->guidelen + p->pamlen > 32 || p->guidelen == 0) return HAWK_E_UNSUPPORTED;  // window code = 2 bits x 32
  // the rows' scan ranges must be those of windows of guidelen + pamlen bases: a window never reaches past its row
  for (uint32_t h = 0; h < hs->n_hap; ++h)
    if (hs->scan_stop[h] > hs->scan_start[h] && (int64_t)hs->scan_stop[h] - 1 + p->guidelen + p->pamlen > (int64_t)hs->hap_len[h]) return HAWK_E_INVALID;
  hawk_ctx* ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ScanParams sp;
  int rc = make_scan_params(hs, p->pam_fwd, p->pam_rev, p->pamlen, p->guidelen, p->right, false, &sp);
  if (rc) return rc;
  sp.poF = p->right ? 0 : (int32_t)p->guidelen;  // windows are indexed by their start, as in ot_front (hawk_api_offtarget.hip)
  sp.poR = p->right ? (int32_t)p->guidelen : 0;
  const OvPlanes al = ov_planes(hs);
  const HapSetDev d = make_dev(hs);
  HapSetDev du = d;  // the PAM scan reads the allele planes: "intersects" on positions that hold several bases
  for (int b = 0; b < 4; ++b) du.plane[b] = al.p[b];
  const size_t words = (size_t)hs->n_hap * hs->S;
  const uint64_t ncnt = (uint64_t)hs->n_hap * 2 * sp.bph;
  if ((rc = hs->keepF.reserve(words * 4)) || (rc = hs->keepR.reserve(words * 4)) || (rc = hs->counts.reserve(ncnt * 4)) ||
      (rc = hs->offsets.reserve((ncnt + 1) * 8)) || (rc = hs->totals.reserve(sizeof(ScanTotals))) ||
      (rc = hs->partial.reserve((ncnt / 1024 + 2) * 8)) || (rc = hs->ovstamp.reserve(64 + 8)) ||
      (rc = hs->guides.reserve(std::max<size_t>((size_t)n_guides * 8, 16))) ||
      (rc = hs->ovhits.reserve(std::max<uint64_t>(cap, 1) * sizeof(OvHit))))
    return rc;
  // ovstamp: the row counter, then the device's wall clock at the stage boundaries - begin, scan done, sites begin, sites done, match done
  unsigned long long* cnt = hs->ovstamp.as<unsigned long long>();
  unsigned long long* stamp = cnt + 1;
  if (n_guides) HIPCHK(hipMemcpyAsync(hs->guides.p, guides2, (size_t)n_guides * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(hs->ovstamp.p, 0, 64 + 8, st));
  hawk_launch_stamp(st, stamp + 0);
  hawk_launch_scan_raw(st, du, sp, hs->keepF.as<uint32_t>(), hs->keepR.as<uint32_t>(), hs->counts.as<uint32_t>());
  hawk_launch_ov_filter(st, d, al, sp, hs->keepF.as<uint32_t>(), hs->keepR.as<uint32_t>(), hs->counts.as<uint32_t>());
  hawk_launch_mscan(st, hs->counts.as<uint32_t>(), ncnt, hs->partial.as<unsigned long long>(), nullptr, hs->offsets.as<uint64_t>(),
                    hs->totals.as<ScanTotals>());
  hawk_launch_stamp(st, stamp + 1);
  HIPCHK(hipGetLastError());
  ScanTotals tot;
  HIPCHK(hipMemcpyAsync(&tot, hs->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the number of sites decides their allocation
  const uint64_t nsites = tot.n_keep;
  if ((rc = hs->ovsites.reserve(std::max<uint64_t>(nsites, 1) * sizeof(OvSite)))) return rc;
  hawk_launch_stamp(st, stamp + 2);
  if (nsites) hawk_launch_ov_sites(st, d, al, sp, hs->keepF.as<uint32_t>(), hs->keepR.as<uint32_t>(), hs->offsets.as<uint64_t>(), hs->ovsites.as<OvSite>());
  hawk_launch_stamp(st, stamp + 3);
  OvGeom g;
  g.pam_fwd = p->pam_fwd; g.G = (int32_t)p->guidelen; g.P = (int32_t)p->pamlen; g.right = p->right ? 1 : 0;
  hawk_launch_ov_match(st, hs->ovsites.as<OvSite>(), nsites, hs->guides.as<uint64_t>(), n_guides, g, (int)p->max_mm, hs->ovhits.as<OvHit>(), cap, cnt);
  hawk_launch_stamp(st, stamp + 4);
  HIPCHK(hipGetLastError());
  unsigned long long h_blk[6] = {0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h_blk, hs->ovstamp.p, sizeof(h_blk), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t nh = h_blk[0];
  *n_out = nh;
  if (timing) {
    memset(timing, 0, sizeof(*timing));
    timing->scan_ms = hawk_stamp_ms(ctx, h_blk[1], h_blk[2]);
    timing->sites_ms = hawk_stamp_ms(ctx, h_blk[3], h_blk[4]);
    timing->match_ms = hawk_stamp_ms(ctx, h_blk[4], h_blk[5]);
    timing->total_ms = hawk_stamp_ms(ctx, h_blk[1], h_blk[5]);
    timing->n_sites = nsites;
    uint64_t pos = 0;
    for (uint32_t h = 0; h < hs->n_hap; ++h) pos += (uint64_t)std::max(0, hs->scan_stop[h] - hs->scan_start[h]);
    timing->scanned_positions = pos;
  }
  if (nh > cap) return HAWK_E_CAPACITY;
  if (!nh) return HAWK_OK;
  std::vector<OvHit> hh(nh);
  HIPCHK(hipMemcpyAsync(hh.data(), hs->ovhits.p, nh * sizeof(OvHit), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t i = 0; i < nh; ++i) {
    if (out_guide) out_guide[i] = hh[i].guide;
    if (out_row) out_row[i] = hh[i].row;
    if (out_q) out_q[i] = hh[i].q & 0x7fffffffu;
    if (out_strand) out_strand[i] = (uint8_t)(hh[i].q >> 31);
    if (out_mm) out_mm[i] = (uint8_t)hh[i].mm;
    if (out_code) out_code[i] = hh[i].code;
    if (out_nmask) out_nmask[i] = hh[i].nmask;
    if (out_alt) out_alt[i] = hh[i].alt;
  }
  return HAWK_OK;
}

}  // extern "C"
