// hawk_api_ugroups.hip - C ABI: the kept guides of a hawk_resolve handle turned into report groups on the device
// (hawk_ugroups.hip) behind an opaque result.  hawk_resolve_groups takes the handle in place of hawk_resolve_download: it gives
// the fill pass device room (hawk_resolve_download copies every batch to wherever it is pointed), runs keys -> sort passes ->
// heads -> two scans, reads the two totals back (they size the result), and emits.  The result owns its buffers.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "hawk_host.h"

// (struct hawk_ugroups, UG_NBUF: hawk_host.h - hawk_effects_create_ugroups in hawk_api_effects.hip reads the result too)
static void ug_release(hawk_ugroups* g) {
  for (DevBuf& b : g->b) b.release();
  delete g;
}

extern "C" {

int hawk_resolve_groups(hawk_resolve* r, const double* cfd_mm, const double* cfd_pam, uint32_t flank_up, uint32_t flank_down,
                        hawk_ugroups** out, uint64_t* n_groups, uint64_t* n_members, hawk_ugroups_timing* timing) {
  if (out) *out = nullptr;
  if (n_groups) *n_groups = 0;
  if (n_members) *n_members = 0;
  if (!r || !out || !r->hs || (cfd_mm && !cfd_pam)) return HAWK_E_INVALID;
  UgGeom g;
  g.guidelen = r->g.guidelen; g.pamlen = r->g.pamlen; g.right = r->g.right; g.W = r->g.W; g.L = g.guidelen + g.pamlen;
  g.up = (int32_t)flank_up; g.down = (int32_t)flank_down;
  const int bad = ug_check_geom(g, flank_up, flank_down);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  if (r->downloaded || r->gen != r->hs->cols_gen) return HAWK_E_INVALID;
  const uint64_t n = r->n_kept;
  if (n > 0xffffffffull) return HAWK_E_UNSUPPORTED;
  hawk_ctx* ctx = r->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  hawk_ugroups* G = new (std::nothrow) hawk_ugroups();
  if (!G) return HAWK_E_OOM;
  G->ctx = ctx;
  G->n_hap = r->hs->n_hap; G->guidelen = g.guidelen; G->pamlen = g.pamlen; G->right = g.right; G->has_cfd = cfd_mm != nullptr;
  memset(&G->tm, 0, sizeof(G->tm));
  G->tm.n_kept = n;
  if (!n) {  // a valid, empty result
    r->downloaded = true;
    if (timing) *timing = G->tm;
    *out = G;
    return HAWK_OK;
  }
  // (the stream is drained before anything goes back to the pool: kernels on these blocks may still be queued)
  auto fail = [&](int code) { (void)hipStreamSynchronize(st); ug_release(G); return code; };
  auto hipfail = [&](hipError_t e, const char* what) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_resolve_groups: %s: %s", what, hipGetErrorString(e));
    return fail(HAWK_E_HIP);
  };
  const size_t temp_bytes = hawk_ug_temp_bytes(n);
  PoolScope tmp;
  uint32_t *d_src, *vals_a, *vals_b, *gflag, *mflag;
  uint64_t *d_win, *keys_a, *keys_b, *gidx, *midx;
  UgWork w;
  double* d_cfd = nullptr;
  int* d_status;
  void* d_temp;
  if (tmp.alloc((void**)&d_src, n * 4) || tmp.alloc((void**)&d_win, n * 8 * UG_PLANES) || tmp.alloc((void**)&w.keyw, n * 8 * UG_KEY_WORDS) ||
      tmp.alloc((void**)&w.hp, n * 8) || tmp.alloc((void**)&w.cfdon, n * 8) || tmp.alloc((void**)&w.gc, n * 2) || tmp.alloc((void**)&keys_a, n * 8) ||
      tmp.alloc((void**)&keys_b, n * 8) || tmp.alloc((void**)&vals_a, n * 4) || tmp.alloc((void**)&vals_b, n * 4) ||
      tmp.alloc((void**)&gflag, (n + 1) * 4) || tmp.alloc((void**)&mflag, (n + 1) * 4) || tmp.alloc((void**)&gidx, (n + 1) * 8) ||
      tmp.alloc((void**)&midx, (n + 1) * 8) || tmp.alloc((void**)&d_status, 64) || tmp.alloc(&d_temp, temp_bytes + 8) ||
      (cfd_mm && tmp.alloc((void**)&d_cfd, (UG_CFD_MM + UG_CFD_PAM) * 8)))
    return fail(HAWK_E_OOM);
  // the fill pass, batch by batch, into the device arrays (stride n); it drains the stream and marks the handle
  hawk_resolve_timing rtm;
  int rc = hawk_resolve_download(r, d_src, d_win, nullptr, nullptr, &rtm);
  if (rc) return fail(rc);
  G->tm.fill_ms = rtm.fill_ms; G->tm.n_batches = rtm.n_batches;
  hipError_t e = hipSuccess;
  if (cfd_mm) {
    e = hipMemcpyAsync(d_cfd, cfd_mm, UG_CFD_MM * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_cfd + UG_CFD_MM, cfd_pam, UG_CFD_PAM * 8, hipMemcpyHostToDevice, st);
  }
  if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, 64, st);
  if (e == hipSuccess) e = hipMemsetAsync(gflag + n, 0, 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(mflag + n, 0, 4, st);
  if (e != hipSuccess) return hipfail(e, "upload");
  UgDev u = {};
  u.c = r->cols; u.is_ref = r->hs->d_is_ref; u.n_hap = r->hs->n_hap; u.n_rows = r->n_rows;
  u.ref_key = r->rkeys.as<uint64_t>() + r->n_rows; u.ref_row = r->rvals.as<uint32_t>() + r->n_rows;
  u.row_kept = r->kept.as<uint32_t>(); u.row_off = r->off.as<uint64_t>();
  u.n = n; u.src_row = d_src; u.win = d_win; u.cfd = d_cfd; u.g = g;
  (void)hipEventRecord(ev[0], st);
  hawk_launch_ug_keys(st, u, w, vals_a, d_status);
  (void)hipEventRecord(ev[1], st);
  const uint32_t* order = hawk_launch_ug_sort(st, u, w, d_temp, temp_bytes, keys_a, keys_b, vals_a, vals_b);
  if (!order) return hipfail(hipGetLastError(), "sort passes");
  (void)hipEventRecord(ev[2], st);
  hawk_launch_ug_heads(st, w, n, order, gflag, mflag);
  if (hawk_launch_ur_offsets(st, gflag, n, d_temp, temp_bytes, gidx) || hawk_launch_ur_offsets(st, mflag, n, d_temp, temp_bytes, midx))
    return hipfail(hipGetLastError(), "scans");
  (void)hipEventRecord(ev[3], st);
  if ((e = hipGetLastError()) != hipSuccess) return hipfail(e, "keys / heads");
  uint64_t tot[2] = {0, 0};
  int status = 0;
  if ((e = hipMemcpyAsync(&tot[0], gidx + n, 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(&tot[1], midx + n, 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess)
    return hipfail(e, "totals");
  if (status) return fail(status);
  const uint64_t ng = tot[0], nm = tot[1];
  if (!ng || ng > n || nm < ng || nm > n) return fail(HAWK_E_INVALID);  // the scans and the flags disagree: never seen
  const size_t sizes[UG_NBUF] = {ng * 4, ng * 4, ng * 4, ng, ng * 8, ng * 8, ng, ng * 8, ng * 8 * UG_PLANES, ng, ng, (ng + 1) * 8, nm * 4};
  for (int i = 0; i < UG_NBUF; ++i)
    if (G->b[i].reserve(sizes[i])) return fail(HAWK_E_OOM);
  UgOut o;
  o.rep_src_row = G->b[0].as<uint32_t>(); o.hap = G->b[1].as<uint32_t>(); o.pos = G->b[2].as<uint32_t>(); o.strand = G->b[3].as<uint8_t>();
  o.start = G->b[4].as<int64_t>(); o.stop = G->b[5].as<int64_t>(); o.is_ref = G->b[6].as<uint8_t>(); o.cfdon = G->b[7].as<double>();
  o.win = G->b[8].as<uint64_t>(); o.gc_num = G->b[9].as<uint8_t>(); o.gc_den = G->b[10].as<uint8_t>(); o.member_off = G->b[11].as<uint64_t>();
  o.member_hap = G->b[12].as<uint32_t>(); o.n_groups = ng; o.n_members = nm;
  (void)hipEventRecord(ev[4], st);
  hawk_launch_ug_emit(st, u, w, order, gflag, mflag, gidx, midx, o);
  (void)hipEventRecord(ev[5], st);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) return hipfail(e, "emit");
  (void)hipEventElapsedTime(&G->tm.keys_ms, ev[0], ev[1]);
  (void)hipEventElapsedTime(&G->tm.sort_ms, ev[1], ev[2]);
  (void)hipEventElapsedTime(&G->tm.heads_ms, ev[2], ev[3]);
  (void)hipEventElapsedTime(&G->tm.emit_ms, ev[4], ev[5]);
  G->tm.total_ms = G->tm.fill_ms + G->tm.keys_ms + G->tm.sort_ms + G->tm.heads_ms + G->tm.emit_ms;
  G->tm.n_groups = ng; G->tm.n_members = nm;
  G->n_groups = ng; G->n_members = nm;
  if (n_groups) *n_groups = ng;
  if (n_members) *n_members = nm;
  if (timing) *timing = G->tm;
  *out = G;
  return HAWK_OK;
}

int hawk_ugroups_download(hawk_ugroups* g, uint32_t* rep_src_row, uint32_t* hap, uint32_t* pos, uint8_t* strand, int64_t* start,
                          int64_t* stop, uint8_t* is_ref, double* cfdon, uint64_t* win, uint8_t* gc_num, uint8_t* gc_den,
                          uint64_t* member_off, uint32_t* member_hap) {
  if (!g) return HAWK_E_INVALID;
  const uint64_t ng = g->n_groups, nm = g->n_members;
  if (!ng) {
    if (member_off) {
      HIPCHK(hipSetDevice(g->ctx->device));
      const uint64_t zero = 0;
      HIPCHK(hipMemcpy(member_off, &zero, 8, hipMemcpyDefault));  // (host or device destination)
    }
    return HAWK_OK;
  }
  HIPCHK(hipSetDevice(g->ctx->device));
  hipStream_t st = g->ctx->stream;
  void* dst[UG_NBUF] = {rep_src_row, hap, pos, strand, start, stop, is_ref, cfdon, win, gc_num, gc_den, member_off, member_hap};
  const size_t sizes[UG_NBUF] = {ng * 4, ng * 4, ng * 4, ng, ng * 8, ng * 8, ng, ng * 8, ng * 8 * UG_PLANES, ng, ng, (ng + 1) * 8, nm * 4};
  hipError_t e = hipSuccess;
  for (int i = 0; i < UG_NBUF && e == hipSuccess; ++i)
    if (dst[i] && sizes[i]) e = hipMemcpyAsync(dst[i], g->b[i].p, sizes[i], hipMemcpyDefault, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_ugroups_download: %s", hipGetErrorString(e));
    return HAWK_E_HIP;
  }
  return HAWK_OK;
}

void hawk_ugroups_free(hawk_ugroups* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->ctx->stream);
  ug_release(g);
}

}  // extern "C"
