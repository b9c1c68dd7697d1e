// hawk_api_resolve.hip - C ABI: the unphased IUPAC windows of a guide table resolved on the device (hawk_resolve.hip) behind an
// opaque handle.  hawk_table_resolve_unphased runs REF's key sort, the count pass and the offsets scan and reads the offsets back
// (they decide the batches and tell the caller how much room the result needs); hawk_resolve_download runs the fill pass in batches
// of whole rows and copies every batch straight into the caller's arrays.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "hawk_host.h"

// (struct hawk_resolve, ur_dev: hawk_host.h - hawk_api_ugroups.hip reads the handle too)
static void ur_release(hawk_resolve* r) {
  for (DevBuf* b : {&r->key, &r->aoff, &r->ref, &r->rkeys, &r->rvals, &r->res, &r->kept, &r->off}) b->release();
  delete r;
}

extern "C" {

int hawk_table_resolve_unphased(hawk_table* t, const hawk_resolve_alleles* alleles, uint64_t pam_fwd, uint64_t pam_rev, hawk_resolve** out,
                                uint64_t* n_kept, uint64_t* n_resolved, hawk_resolve_decline* decline, hawk_resolve_timing* timing) {
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->row = -1; }
  if (out) *out = nullptr;
  if (!t || !alleles || !out || !t->hs || hawk_table_stale(t) || !t->hs->has_meta) return HAWK_E_INVALID;
  hawk_hapset* hs = t->hs;
  hawk_ctx* ctx = hs->ctx;
  const uint64_t n = t->n_rows;
  if (n > 0xffffffffull) return HAWK_E_UNSUPPORTED;
  UrGeom g;
  g.pam_fwd = pam_fwd; g.pam_rev = pam_rev; g.guidelen = (int32_t)t->guidelen; g.pamlen = (int32_t)t->pamlen; g.right = t->right ? 1 : 0;
  g.W = g.guidelen + g.pamlen + 2 * UR_PAD;
  const int bad = ur_check_geom(g);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  UrAlleles hal;
  hal.key = alleles->key; hal.off = alleles->off; hal.ref = alleles->ref; hal.n_keys = alleles->n_keys;
  if (!ur_check_alleles(hal)) return HAWK_E_INVALID;
  auto declined = [&](int reason, int64_t row) {
    if (decline) { decline->reason = reason; decline->row = row; }
    return (reason == UR_DECL_ROW_SIZE || reason == UR_DECL_BATCH) ? HAWK_E_CAPACITY : HAWK_E_UNSUPPORTED;
  };
  if (n && hs->n_ref_rows > 1) return declined(UR_DECL_MULTI_REF, -1);
  uint64_t budget = 256ull << 20;
  if (const char* e = getenv("HAWK_RESOLVE_BATCH_BYTES")) {  // read per call
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e && v) budget = v;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  hawk_resolve* r = new (std::nothrow) hawk_resolve();
  if (!r) return HAWK_E_INVALID;
  r->ctx = ctx; r->hs = hs; r->gen = t->gen; r->cols = t->cols; r->g = g; r->n_rows = n; r->bcap = budget / UR_OUT_BYTES;
  memset(&r->tm, 0, sizeof(r->tm));
  // (the stream is drained first: copies into this call's host arrays and kernels on its pool blocks may still be queued)
  auto fail = [&](int code) { (void)hipStreamSynchronize(st); ur_release(r); return code; };
  auto hipfail = [&](hipError_t e, const char* what) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_table_resolve_unphased: %s: %s", what, hipGetErrorString(e));
    return fail(HAWK_E_HIP);
  };
  const uint64_t nk = hal.n_keys, ne = nk ? hal.off[nk] : 0;
  r->n_keys = nk;
  const size_t temp_bytes = hawk_ur_temp_bytes(n);
  PoolScope tmp;
  unsigned long long* d_misc;  // [0] decline, [1] resolved, [2] kept
  void* d_temp;
  int rc;
  if ((rc = r->key.reserve(nk * 8 + 8)) || (rc = r->aoff.reserve((nk + 1) * 4)) || (rc = r->ref.reserve(ne + 8)) || (rc = r->rkeys.reserve(2 * n * 8 + 8)) ||
      (rc = r->rvals.reserve(2 * n * 4 + 8)) || (rc = r->res.reserve((n + 1) * 4)) || (rc = r->kept.reserve((n + 1) * 4)) ||
      (rc = r->off.reserve((n + 1) * 8)) || (rc = tmp.alloc((void**)&d_misc, 64)) || (rc = tmp.alloc(&d_temp, temp_bytes + 8)))
    return fail(rc);
  uint32_t *d_res = r->res.as<uint32_t>(), *d_kept = r->kept.as<uint32_t>();
  uint64_t* d_off = r->off.as<uint64_t>();
  hipError_t e = hipEventRecord(ev[0], st);
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  };
  up(r->key.p, hal.key, nk * 8);
  if (nk) up(r->aoff.p, hal.off, (nk + 1) * 4);
  up(r->ref.p, hal.ref, ne);
  if (e == hipSuccess) e = hipMemsetAsync(d_misc, 0xff, 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_misc + 1, 0, 56, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_kept, 0, (n + 1) * 4, st);
  if (e != hipSuccess) return hipfail(e, "upload");
  const UrDev d = ur_dev(r);
  (void)hipEventRecord(ev[1], st);
  if (hawk_launch_ur_refsort(st, d, d_temp, temp_bytes, r->rkeys.as<uint64_t>(), r->rvals.as<uint32_t>())) return hipfail(hipGetLastError(), "REF key sort");
  (void)hipEventRecord(ev[2], st);
  hawk_launch_ur_count(st, d, d_res, d_kept, d_misc, d_misc + 1);
  (void)hipEventRecord(ev[3], st);
  if (hawk_launch_ur_offsets(st, d_kept, n, d_temp, temp_bytes, d_off)) return hipfail(hipGetLastError(), "offsets scan");
  (void)hipEventRecord(ev[4], st);
  if ((e = hipGetLastError()) != hipSuccess) return hipfail(e, "count pass");
  // the offsets decide the batches: one read-back of 8 bytes per row, with the counts the caller will ask for
  unsigned long long misc[3];
  r->h_off.assign(n + 1, 0);
  r->h_cnt.assign(2 * n + 1, 0);
  if (n && ((e = hipMemcpyAsync(r->h_cnt.data(), d_res, n * 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipMemcpyAsync(r->h_cnt.data() + n, d_kept, n * 4, hipMemcpyDeviceToHost, st)) != hipSuccess))
    return hipfail(e, "counts");
  if ((e = hipMemcpyAsync(r->h_off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(misc, d_misc, sizeof(misc), hipMemcpyDeviceToHost, st)) != hipSuccess)
    return hipfail(e, "offsets");
  (void)hipEventRecord(ev[5], st);
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return hipfail(e, "offsets");
  if (misc[0] != ~0ull) {
    ur_release(r);
    return declined((int)(misc[0] & 0xff), (int64_t)(misc[0] >> 8));
  }
  const uint64_t total = r->h_off[n];
  if (total != misc[2]) return fail(HAWK_E_INVALID);  // the scan and the count pass disagree: never seen
  for (uint64_t i = 0; i < n; ++i)
    if (r->h_cnt[n + i] > r->bcap) { ur_release(r); return declined(UR_DECL_BATCH, (int64_t)i); }
  r->n_kept = total; r->n_resolved = misc[1];
  (void)hipEventElapsedTime(&r->tm.upload_ms, ev[0], ev[1]);
  (void)hipEventElapsedTime(&r->tm.refsort_ms, ev[1], ev[2]);
  (void)hipEventElapsedTime(&r->tm.count_ms, ev[2], ev[3]);
  (void)hipEventElapsedTime(&r->tm.scan_ms, ev[3], ev[4]);
  (void)hipEventElapsedTime(&r->tm.total_ms, ev[0], ev[5]);
  r->tm.n_rows = n; r->tm.n_resolved = misc[1]; r->tm.n_kept = total;
  if (n_kept) *n_kept = total;
  if (n_resolved) *n_resolved = misc[1];
  if (timing) *timing = r->tm;
  *out = r;
  return HAWK_OK;
}

int hawk_resolve_download(hawk_resolve* r, uint32_t* src_row, uint64_t* win, uint32_t* row_resolved, uint32_t* row_kept, hawk_resolve_timing* timing) {
  if (!r) return HAWK_E_INVALID;
  const uint64_t n = r->n_rows, total = r->n_kept;
  if (row_resolved && n) memcpy(row_resolved, r->h_cnt.data(), n * 4);
  if (row_kept && n) memcpy(row_kept, r->h_cnt.data() + n, n * 4);
  hawk_resolve_timing tm = r->tm;
  if (total && (src_row || win)) {
    if (r->gen != r->hs->cols_gen) return HAWK_E_INVALID;  // a later search on the set has overwritten the rows
    hawk_ctx* ctx = r->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t cap = total < r->bcap ? total : r->bcap;  // outputs of the largest batch
    PoolScope tmp;
    uint32_t* d_src; uint64_t* d_win;
    TEMPCHK(tmp, &d_src, cap * 4);
    TEMPCHK(tmp, &d_win, cap * 8 * UR_PLANES);
    const UrDev d = ur_dev(r);
    const std::vector<uint64_t>& off = r->h_off;
    hipError_t e = hipEventRecord(ctx->ev[0], st);
    for (uint64_t r0 = 0; r0 < n && e == hipSuccess;) {
      uint64_t r1 = r0 + 1;  // whole rows while they fit
      while (r1 < n && off[r1 + 1] - off[r0] <= cap) ++r1;
      const uint64_t o0 = off[r0], m = off[r1] - o0;
      if (m) {
        hawk_launch_ur_fill(st, d, r->res.as<uint32_t>(), r->kept.as<uint32_t>(), r->off.as<uint64_t>(), r0, r1, o0, m, d_src, d_win, cap);
        e = hipGetLastError();
        if (e == hipSuccess && src_row) e = hipMemcpyAsync(src_row + o0, d_src, m * 4, hipMemcpyDefault, st);
        for (int pl = 0; pl < UR_PLANES && e == hipSuccess && win; ++pl)
          e = hipMemcpyAsync(win + (uint64_t)pl * total + o0, d_win + (uint64_t)pl * cap, m * 8, hipMemcpyDefault, st);
        ++tm.n_batches;
      }
      r0 = r1;
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
    const hipError_t es = hipStreamSynchronize(st);  // on every path: the batch buffers go back to the pool when this returns
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
      snprintf(hawk_hip_err_buf(), 256, "hawk_resolve_download: %s", hipGetErrorString(e));
      return HAWK_E_HIP;
    }
    (void)hipEventElapsedTime(&tm.fill_ms, ctx->ev[0], ctx->ev[1]);
    tm.total_ms += tm.fill_ms;
    r->downloaded = true;  // (hawk_resolve_groups takes a handle once, in place of this call)
  }
  if (timing) *timing = tm;
  return HAWK_OK;
}

void hawk_resolve_free(hawk_resolve* r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  (void)hipStreamSynchronize(r->ctx->stream);
  ur_release(r);
}

}  // extern "C"
