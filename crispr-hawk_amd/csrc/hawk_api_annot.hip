// hawk_api_annot.hip - C ABI: the BED annotation join (hawk_annot.hip) behind an opaque handle per (file, contig, label kind)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "hawk_host.h"

struct hawk_annot {
  hawk_ctx* ctx;
  uint64_t n;
  DevBuf start, end, rmax, bmax, loff, blob;  // the feature table
  DevBuf qs, qe, off, out, partial, totals;   // workspace of one batch; the batch's share returns to the pool on download
  bool has_result = false;                    // off / out hold the rows of the last query, not yet downloaded
  uint64_t res_nq = 0, res_bytes = 0;
};

static AnnDev ann_dev(const hawk_annot* a) {
  AnnDev d;
  d.start = a->start.as<int64_t>(); d.end = a->end.as<int64_t>(); d.rmax = a->rmax.as<int64_t>(); d.bmax = a->bmax.as<int64_t>();
  d.loff = a->loff.as<uint64_t>(); d.blob = a->blob.as<uint8_t>(); d.n = a->n;
  return d;
}

static void annot_release(hawk_annot* a) {
  for (DevBuf* b : {&a->start, &a->end, &a->rmax, &a->bmax, &a->loff, &a->blob, &a->qs, &a->qe, &a->off, &a->out, &a->partial, &a->totals})
    b->release();
  delete a;
}

extern "C" {

int hawk_annot_create(hawk_ctx* ctx, const int64_t* start, const int64_t* end, const uint8_t* label_blob, const uint64_t* label_off,
                      uint64_t n, hawk_annot** out, float* index_ms) {
  if (!ctx || !out || (n && (!start || !end || !label_off))) return HAWK_E_INVALID;
  // what the searches rest on: starts in non-decreasing order (the walk's bounds), end >= start, label offsets that only grow
  for (uint64_t i = 0; i < n; ++i) {
    if (end[i] < start[i] || (i && start[i] < start[i - 1]) || label_off[i + 1] < label_off[i]) return HAWK_E_INVALID;
  }
  if (n && (label_off[0] != 0 || (label_off[n] && !label_blob))) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hawk_annot* a = new (std::nothrow) hawk_annot();
  if (!a) return HAWK_E_INVALID;
  a->ctx = ctx;
  a->n = n;
  if (index_ms) *index_ms = 0.f;
  if (n) {
    const uint64_t lbytes = label_off[n], nblk = (n + 63) / 64;
    int rc;
    if ((rc = a->start.reserve(n * 8)) || (rc = a->end.reserve(n * 8)) || (rc = a->rmax.reserve(n * 8)) || (rc = a->bmax.reserve(nblk * 8)) ||
        (rc = a->loff.reserve((n + 1) * 8)) || (rc = a->blob.reserve(std::max<uint64_t>(lbytes, 1))) ||
        (rc = a->partial.reserve(hawk_ann_scan_blocks(n) * 8))) {
      annot_release(a);
      return rc;
    }
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(a->start.p, start, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(a->end.p, end, n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(a->loff.p, label_off, (n + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && lbytes) e = hipMemcpyAsync(a->blob.p, label_blob, lbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[0], st);
    if (e == hipSuccess) {
      hawk_launch_ann_index(st, a->end.as<int64_t>(), n, a->partial.as<int64_t>(), a->rmax.as<int64_t>(), a->bmax.as<int64_t>());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the caller's arrays may go once this returns
    if (e != hipSuccess) {
      snprintf(hawk_hip_err_buf(), 256, "hawk_annot_create: %s", hipGetErrorString(e));
      annot_release(a);
      return HAWK_E_HIP;
    }
    if (index_ms) (void)hipEventElapsedTime(index_ms, ctx->ev[0], ctx->ev[1]);
  }
  *out = a;
  return HAWK_OK;
}

void hawk_annot_free(hawk_annot* a) {
  if (!a) return;
  (void)hipSetDevice(a->ctx->device);
  (void)hipStreamSynchronize(a->ctx->stream);
  annot_release(a);
}

int hawk_annot_query(hawk_annot* a, const int64_t* qstart, const int64_t* qstop, uint64_t nq, uint64_t* n_bytes, uint64_t* n_overlaps,
                     hawk_annot_timing* timing) {
  if (!a || !n_bytes || (nq && (!qstart || !qstop))) return HAWK_E_INVALID;
  *n_bytes = 0;
  a->has_result = false;
  if (n_overlaps) *n_overlaps = 0;
  if (timing) memset(timing, 0, sizeof(*timing));
  hawk_ctx* ctx = a->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  int rc;
  if ((rc = a->qs.reserve(nq * 8)) || (rc = a->qe.reserve(nq * 8)) || (rc = a->off.reserve((nq + 1) * 8)) ||
      (rc = a->partial.reserve(std::max<uint64_t>(hawk_ann_scan_blocks(nq), hawk_ann_scan_blocks(a->n)) * 8)) || (rc = a->totals.reserve(16)))
    return rc;
  HIPCHK(hipMemsetAsync(a->totals.p, 0, 16, st));  // overlaps, walk steps
  HIPCHK(hipEventRecord(ev[0], st));
  if (nq) {
    HIPCHK(hipMemcpyAsync(a->qs.p, qstart, nq * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(a->qe.p, qstop, nq * 8, hipMemcpyHostToDevice, st));
  } else {
    HIPCHK(hipMemsetAsync(a->off.p, 0, 8, st));
  }
  const AnnDev d = ann_dev(a);
  HIPCHK(hipEventRecord(ev[1], st));
  hawk_launch_ann_count(st, d, a->qs.as<int64_t>(), a->qe.as<int64_t>(), nq, a->off.as<uint64_t>(), a->totals.as<unsigned long long>());
  HIPCHK(hipEventRecord(ev[2], st));
  hawk_launch_ann_offsets(st, a->off.as<uint64_t>(), nq, a->partial.as<uint64_t>());
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  uint64_t tot[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(tot, a->totals.p, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot[2], a->off.as<uint64_t>() + nq, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the blob's size decides its allocation
  const uint64_t nbytes = tot[2];
  if ((rc = a->out.reserve(std::max<uint64_t>(nbytes, 1)))) return rc;
  HIPCHK(hipEventRecord(ev[4], st));
  hawk_launch_ann_fill(st, d, a->qs.as<int64_t>(), a->qe.as<int64_t>(), nq, a->off.as<uint64_t>(), a->out.as<uint8_t>());
  HIPCHK(hipEventRecord(ev[5], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  a->has_result = true;
  a->res_nq = nq;
  a->res_bytes = nbytes;
  *n_bytes = nbytes;
  if (n_overlaps) *n_overlaps = tot[0];
  if (timing) {
    (void)hipEventElapsedTime(&timing->upload_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&timing->count_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&timing->scan_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&timing->fill_ms, ev[4], ev[5]);
    (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[5]);
    timing->out_bytes = nbytes;
    timing->walk_steps = tot[1];
  }
  return HAWK_OK;
}

int hawk_annot_download(hawk_annot* a, uint8_t* blob, uint64_t* off, float* download_ms) {
  if (!a || !off || !a->has_result || (a->res_bytes && !blob)) return HAWK_E_INVALID;
  hawk_ctx* ctx = a->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (a->res_bytes) HIPCHK(hipMemcpyAsync(blob, a->out.p, a->res_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(off, a->off.p, (a->res_nq + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipStreamSynchronize(st));
  if (download_ms) (void)hipEventElapsedTime(download_ms, ctx->ev[0], ctx->ev[1]);
  // the batch's workspace goes back to the caching allocator: a handle lives as long as its file, a C4 column is tens of GB
  a->has_result = false;
  a->out.release(); a->qs.release(); a->qe.release(); a->off.release();
  return HAWK_OK;
}

}  // extern "C"
