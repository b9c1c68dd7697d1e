// hawk_api_gnomad.hip - C ABI: gnomAD sites records -> population-genotype lines (hawk_gnomad.hip) behind one handle per batch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "hawk_host.h"

struct hawk_gnomad {
  hawk_ctx* ctx;
  uint64_t n = 0, text_len = 0;
  uint32_t n_keys = 0, keep = 0;
  DevBuf text, lo, keys, koff, mask, flags, fo, qs, as;  // the batch and what k_gn_scan wrote
  DevBuf kidx, off, out, partial, pool, poff;            // the text passes
  bool has_text = false;
  uint64_t n_kept = 0, n_bytes = 0;
};

static GnDev gn_dev(const hawk_gnomad* g) {
  GnDev d;
  d.text = g->text.as<uint8_t>(); d.line_off = g->lo.as<uint64_t>(); d.n = g->n;
  d.keys = g->keys.as<uint8_t>(); d.key_off = g->koff.as<uint32_t>(); d.n_keys = g->n_keys; d.keep = g->keep;
  d.mask = g->mask.as<uint32_t>(); d.flags = g->flags.as<uint8_t>(); d.field_off = g->fo.as<uint32_t>();
  d.qual_span = g->qs.as<uint32_t>(); d.af_span = g->as.as<uint32_t>();
  return d;
}

static void gn_release(hawk_gnomad* g) {
  for (DevBuf* b : {&g->text, &g->lo, &g->keys, &g->koff, &g->mask, &g->flags, &g->fo, &g->qs, &g->as, &g->kidx, &g->off, &g->out, &g->partial,
                    &g->pool, &g->poff})
    b->release();
  delete g;
}

extern "C" {

int hawk_gnomad_scan(hawk_ctx* ctx, const uint8_t* text, uint64_t text_len, const uint64_t* line_off, uint64_t n_lines,
                     const uint8_t* key_blob, const uint64_t* key_off, uint32_t n_keys, int keep, hawk_gnomad** out,
                     hawk_gnomad_timing* timing) {
  if (!ctx || !out || n_lines > 0x7fffffffull) return HAWK_E_INVALID;
  if (!gn_args_ok(text, text_len, line_off, n_lines, key_blob, key_off, n_keys)) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hawk_gnomad* g = new (std::nothrow) hawk_gnomad();
  if (!g) return HAWK_E_INVALID;
  g->ctx = ctx; g->n = n_lines; g->text_len = text_len; g->n_keys = n_keys; g->keep = keep ? 1u : 0u;
  if (timing) memset(timing, 0, sizeof(*timing));
  if (n_lines) {
    const uint64_t n = n_lines, kbytes = key_off[n_keys];
    uint32_t koff32[GN_MAX_KEYS + 1];
    for (uint32_t k = 0; k <= n_keys; ++k) koff32[k] = (uint32_t)key_off[k];
    int rc;
    if ((rc = g->text.reserve(text_len)) || (rc = g->lo.reserve((n + 1) * 8)) || (rc = g->keys.reserve(std::max<uint64_t>(kbytes, 1))) ||
        (rc = g->koff.reserve((n_keys + 1) * 4)) || (rc = g->mask.reserve(n * 4)) || (rc = g->flags.reserve(n)) || (rc = g->fo.reserve(n * 32)) ||
        (rc = g->qs.reserve(n * 8)) || (rc = g->as.reserve(n * 8))) {
      gn_release(g);
      return rc;
    }
    hipStream_t st = ctx->stream;
    hipEvent_t* ev = ctx->ev;
    hipError_t e = hipEventRecord(ev[0], st);
    if (e == hipSuccess) e = hipMemcpyAsync(g->text.p, text, text_len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(g->lo.p, line_off, (n + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && kbytes) e = hipMemcpyAsync(g->keys.p, key_blob, kbytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(g->koff.p, koff32, (n_keys + 1) * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) {
      hawk_launch_gn_scan(st, gn_dev(g));
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[2], st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // koff32 and the caller's arrays may go once this returns
    if (e != hipSuccess) {
      snprintf(hawk_hip_err_buf(), 256, "hawk_gnomad_scan: %s", hipGetErrorString(e));
      gn_release(g);
      return HAWK_E_HIP;
    }
    if (timing) {
      (void)hipEventElapsedTime(&timing->upload_ms, ev[0], ev[1]);
      (void)hipEventElapsedTime(&timing->scan_ms, ev[1], ev[2]);
      (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[2]);
    }
  }
  if (timing) timing->n_records = n_lines;
  *out = g;
  return HAWK_OK;
}

int hawk_gnomad_records(hawk_gnomad* g, uint32_t* mask, uint8_t* flags, uint32_t* field_off, uint32_t* qual_span, uint32_t* af_span) {
  if (!g) return HAWK_E_INVALID;
  if (!g->n) return HAWK_OK;
  HIPCHK(hipSetDevice(g->ctx->device));
  hipStream_t st = g->ctx->stream;
  if (mask) HIPCHK(hipMemcpyAsync(mask, g->mask.p, g->n * 4, hipMemcpyDeviceToHost, st));
  if (flags) HIPCHK(hipMemcpyAsync(flags, g->flags.p, g->n, hipMemcpyDeviceToHost, st));
  if (field_off) HIPCHK(hipMemcpyAsync(field_off, g->fo.p, g->n * 32, hipMemcpyDeviceToHost, st));
  if (qual_span) HIPCHK(hipMemcpyAsync(qual_span, g->qs.p, g->n * 8, hipMemcpyDeviceToHost, st));
  if (af_span) HIPCHK(hipMemcpyAsync(af_span, g->as.p, g->n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}

int hawk_gnomad_text(hawk_gnomad* g, const uint8_t* pool_blob, const uint64_t* pool_off, uint64_t* n_bytes, uint64_t* n_kept,
                     hawk_gnomad_timing* timing) {
  if (!g || !n_bytes || !n_kept) return HAWK_E_INVALID;
  hawk_ctx* ctx = g->ctx;
  const uint64_t n = g->n;
  g->has_text = false;
  if (timing) { memset(timing, 0, sizeof(*timing)); timing->n_records = n; }
  if (!n) {
    *n_bytes = 0; *n_kept = 0;
    g->has_text = pool_off != nullptr;
    g->n_kept = 0; g->n_bytes = 0;
    return HAWK_OK;
  }
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  int rc;
  if ((rc = g->kidx.reserve((n + 1) * 8)) || (rc = g->off.reserve((n + 1) * 8)) || (rc = g->partial.reserve(std::max<uint64_t>(hawk_ann_scan_blocks(n), 1) * 8)))
    return rc;
  const GnDev d = gn_dev(g);
  // number the kept records: the pool is laid out by that number
  hawk_launch_gn_kept(st, d, g->kidx.as<uint64_t>());
  hawk_launch_ann_offsets(st, g->kidx.as<uint64_t>(), n, g->partial.as<uint64_t>());
  HIPCHK(hipGetLastError());
  uint64_t kept = 0;
  HIPCHK(hipMemcpyAsync(&kept, g->kidx.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *n_kept = kept;
  *n_bytes = 0;
  g->n_kept = kept;
  if (timing) timing->n_kept = kept;
  if (!pool_off) return HAWK_OK;
  // the pool as the kernels will index it: 2 * kept + 1 offsets that only grow, inside the blob
  if (pool_off[0] != 0) return HAWK_E_INVALID;
  for (uint64_t j = 0; j < 2 * kept; ++j)
    if (pool_off[j + 1] < pool_off[j]) return HAWK_E_INVALID;
  const uint64_t pbytes = pool_off[2 * kept];
  if (pbytes && !pool_blob) return HAWK_E_INVALID;
  if ((rc = g->pool.reserve(std::max<uint64_t>(pbytes, 1))) || (rc = g->poff.reserve((2 * kept + 1) * 8))) return rc;
  HIPCHK(hipEventRecord(ev[0], st));
  if (pbytes) HIPCHK(hipMemcpyAsync(g->pool.p, pool_blob, pbytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(g->poff.p, pool_off, (2 * kept + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev[1], st));
  hawk_launch_gn_text_len(st, d, g->kidx.as<uint64_t>(), g->pool.as<uint8_t>(), g->poff.as<uint64_t>(), kept, g->off.as<uint64_t>());
  HIPCHK(hipEventRecord(ev[2], st));
  hawk_launch_ann_offsets(st, g->off.as<uint64_t>(), n, g->partial.as<uint64_t>());
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  uint64_t nbytes = 0;
  HIPCHK(hipMemcpyAsync(&nbytes, g->off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the blob's size decides its allocation
  if ((rc = g->out.reserve(std::max<uint64_t>(nbytes, 1)))) return rc;
  HIPCHK(hipEventRecord(ev[4], st));
  hawk_launch_gn_text_fill(st, d, g->kidx.as<uint64_t>(), g->pool.as<uint8_t>(), g->poff.as<uint64_t>(), kept, g->off.as<uint64_t>(), g->out.as<uint8_t>());
  HIPCHK(hipEventRecord(ev[5], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  g->has_text = true;
  g->n_bytes = nbytes;
  *n_bytes = nbytes;
  if (timing) {
    (void)hipEventElapsedTime(&timing->upload_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&timing->len_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&timing->prefix_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&timing->fill_ms, ev[4], ev[5]);
    (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[5]);
    timing->out_bytes = nbytes;
  }
  return HAWK_OK;
}

int hawk_gnomad_text_download(hawk_gnomad* g, uint8_t* blob, uint64_t* off) {
  if (!g || !g->has_text) return HAWK_E_INVALID;
  if (!g->n) {
    if (off) off[0] = 0;
    return HAWK_OK;
  }
  HIPCHK(hipSetDevice(g->ctx->device));
  hipStream_t st = g->ctx->stream;
  if (blob && g->n_bytes) HIPCHK(hipMemcpyAsync(blob, g->out.p, g->n_bytes, hipMemcpyDeviceToHost, st));
  if (off) HIPCHK(hipMemcpyAsync(off, g->off.p, (g->n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}

void hawk_gnomad_destroy(hawk_gnomad* g) {
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->ctx->stream);
  gn_release(g);
}

}  // extern "C"
