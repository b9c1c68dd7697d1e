// hawk_api_uwin.hip - C ABI: the indel-window rows of an unphased VCF built on the device (include/hawk.h; kernels: hawk_uwin.hip;
// the rules: hawk_uwin.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "hawk_host.h"

// The kernels of a call are timed by the device's wall clock (hawk_launch_stamp), not by event packets: a stamp block of the call's
// own, cleared, stamped at the stage boundaries and read back with the results.
struct UwStamps {
  unsigned long long* d = nullptr;
  unsigned long long h[4] = {0, 0, 0, 0};
  int init(PoolScope& tmp, hipStream_t st) {
    if (int rc = tmp.alloc(reinterpret_cast<void**>(&d), sizeof(h))) return rc;
    return hipMemsetAsync(d, 0, sizeof(h), st) == hipSuccess ? HAWK_OK : HAWK_E_HIP;
  }
  void mark(hipStream_t st, int k) { hawk_launch_stamp(st, d + k); }
  hipError_t fetch(hipStream_t st) { return hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st); }
  float ms(const hawk_ctx* ctx, int a, int b) const { return hawk_stamp_ms(ctx, h[a], h[b]); }
};

static int uw_declined(hawk_ubuild_decline* decline, unsigned long long dec) {
  if (decline) { decline->reason = (int32_t)(dec & 0xffu); decline->var = (int64_t)(dec >> 8); }
  return HAWK_E_UNSUPPORTED;
}

extern "C" {

void hawk_uwin_free(hawk_uwin* w) {
  if (!w) return;
  (void)hipSetDevice(w->ctx->device);
  (void)hipStreamSynchronize(w->ctx->stream);
  for (DevBuf* b : {&w->line, &w->allele, &w->off, &w->ref_len, &w->alt_len, &w->pool_off, &w->pool, &w->rank_sample, &w->ref, &w->inst_off,
                    &w->inst_indel, &w->inst_sample, &w->inst_lo, &w->inst_hi})
    b->release();
  delete w;
}

int hawk_uwin_instances(hawk_gt* g, hawk_ubuild* u, const hawk_uwin_input* in, uint64_t* inst_off, hawk_uwin** out,
                        hawk_ubuild_decline* decline, float* kernel_ms) {
  if (out) *out = nullptr;
  if (kernel_ms) *kernel_ms = 0.f;
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->var = -1; }
  if (!g || !u || !in || !inst_off || !out || u->ctx != g->ctx || u->n_samples != g->n_samples) return HAWK_E_INVALID;
  const uint32_t ni = in->n_indel, ns = g->n_samples, L = in->region_len;
  if (!ns || !L || !in->ref || !in->rank_sample || (u->n_var && u->max_off >= L)) return HAWK_E_INVALID;
  if (ni && (!in->line || !in->allele || !in->off || !in->ref_len || !in->alt_len || !in->pool_off || !in->pool)) return HAWK_E_INVALID;
  // everything the kernels index with is checked here
  for (uint32_t k = 0; k < ni; ++k)
    if (in->line[k] >= g->n_lines || in->allele[k] == 0 || in->allele[k] == 255 ||
        (uint64_t)in->pool_off[k] + in->ref_len[k] + in->alt_len[k] > in->pool_len)
      return HAWK_E_INVALID;
  {
    std::vector<uint8_t> seen(ns, 0);
    for (uint32_t r = 0; r < ns; ++r) {
      if (in->rank_sample[r] >= ns || seen[in->rank_sample[r]]) return HAWK_E_INVALID;
      seen[in->rank_sample[r]] = 1;
    }
  }
  hawk_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hawk_uwin* w = new (std::nothrow) hawk_uwin();
  if (!w) return HAWK_E_INVALID;
  w->ctx = ctx; w->u = u; w->n_indel = ni; w->n_samples = ns; w->L = L;
  w->h_off.assign(in->off, in->off + ni); w->h_ref_len.assign(in->ref_len, in->ref_len + ni); w->h_alt_len.assign(in->alt_len, in->alt_len + ni);
  w->h_inst_off.assign((size_t)ni + 1, 0);
  struct Guard { hawk_uwin* w; ~Guard() { if (w) hawk_uwin_free(w); } } guard{w};
  int rc;
  const size_t n1 = std::max<size_t>(ni, 1);
  if ((rc = w->line.reserve(n1 * 4)) || (rc = w->allele.reserve(n1)) || (rc = w->off.reserve(n1 * 4)) || (rc = w->ref_len.reserve(n1 * 4)) ||
      (rc = w->alt_len.reserve(n1 * 4)) || (rc = w->pool_off.reserve(n1 * 4)) || (rc = w->pool.reserve(std::max<size_t>(in->pool_len, 1))) ||
      (rc = w->rank_sample.reserve((size_t)ns * 4)) || (rc = w->ref.reserve(L)) || (rc = w->inst_off.reserve(((size_t)ni + 1) * 8)))
    return rc;
  if (ni) {
    HIPCHK(hipMemcpyAsync(w->line.p, in->line, (size_t)ni * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->allele.p, in->allele, ni, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->off.p, in->off, (size_t)ni * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->ref_len.p, in->ref_len, (size_t)ni * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->alt_len.p, in->alt_len, (size_t)ni * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->pool_off.p, in->pool_off, (size_t)ni * 4, hipMemcpyHostToDevice, st));
    if (in->pool_len) HIPCHK(hipMemcpyAsync(w->pool.p, in->pool, in->pool_len, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(w->rank_sample.p, in->rank_sample, (size_t)ns * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(w->ref.p, in->ref, L, hipMemcpyHostToDevice, st));
  if (ni) {
    const uint32_t n_chunk = (ns + 63u) / 64u;
    uint32_t* d_cnt = nullptr;
    unsigned long long *d_bal = nullptr, *d_dec = nullptr;
    PoolScope tmp;
    TEMPCHK(tmp, &d_cnt, (size_t)ni * 4); TEMPCHK(tmp, &d_bal, (size_t)ni * n_chunk * 8); TEMPCHK(tmp, &d_dec, 8);
    HIPCHK(hipMemsetAsync(d_dec, 0xff, 8, st));
    UwStamps ts;
    if ((rc = ts.init(tmp, st))) return rc;
    ts.mark(st, 0);
    hawk_launch_uw_count(st, g->d_codes, w->view(), d_bal, d_cnt, d_dec);
    ts.mark(st, 1);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> cnt(ni);
    unsigned long long dec = ~0ull;
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)ni * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&dec, d_dec, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (dec != ~0ull) return uw_declined(decline, dec);
    for (uint32_t k = 0; k < ni; ++k) w->h_inst_off[k + 1] = w->h_inst_off[k] + cnt[k];  // n_indel values: a host prefix sum
    w->n_inst = w->h_inst_off[ni];
    if (w->n_inst >= 0xffffffffull) return HAWK_E_CAPACITY;
    const size_t m1 = std::max<size_t>(w->n_inst, 1);
    if ((rc = w->inst_indel.reserve(m1 * 4)) || (rc = w->inst_sample.reserve(m1 * 4)) || (rc = w->inst_lo.reserve(m1 * 8)) ||
        (rc = w->inst_hi.reserve(m1 * 8)))
      return rc;
    HIPCHK(hipMemcpyAsync(w->inst_off.p, w->h_inst_off.data(), ((size_t)ni + 1) * 8, hipMemcpyHostToDevice, st));
    ts.mark(st, 2);
    hawk_launch_uw_instances(st, w->view(), u->view(), d_bal);
    ts.mark(st, 3);
    HIPCHK(hipGetLastError());
    HIPCHK(ts.fetch(st));
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms) *kernel_ms = ts.ms(ctx, 0, 1) + ts.ms(ctx, 2, 3);
  } else {
    HIPCHK(hipMemsetAsync(w->inst_off.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  memcpy(inst_off, w->h_inst_off.data(), ((size_t)ni + 1) * 8);
  guard.w = nullptr;
  *out = w;
  return HAWK_OK;
}

int hawk_uwin_download(hawk_uwin* w, uint32_t* inst_sample, uint64_t* inst_lo, uint64_t* inst_hi) {
  if (!w || (w->n_inst && (!inst_sample || !inst_lo || !inst_hi))) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(w->ctx->device));
  hipStream_t st = w->ctx->stream;
  if (w->n_inst) {
    HIPCHK(hipMemcpyAsync(inst_sample, w->inst_sample.p, w->n_inst * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(inst_lo, w->inst_lo.p, w->n_inst * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(inst_hi, w->inst_hi.p, w->n_inst * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}

int hawk_uwin_signatures(hawk_uwin* w, uint64_t* sig, hawk_ubuild_decline* decline, float* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.f;
  if (decline) { decline->reason = 0; decline->reserved = 0; decline->var = -1; }
  if (!w || (w->n_inst && !sig)) return HAWK_E_INVALID;
  if (!w->n_inst) return HAWK_OK;
  hawk_ctx* ctx = w->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  unsigned long long *d_sig = nullptr, *d_dec = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_sig, (size_t)w->n_inst * 16); TEMPCHK(tmp, &d_dec, 8);
  HIPCHK(hipMemsetAsync(d_dec, 0xff, 8, ctx->stream));
  UwStamps ts;
  if (int rc = ts.init(tmp, ctx->stream)) return rc;
  ts.mark(ctx->stream, 0);
  hawk_launch_uw_sig(ctx->stream, w->view(), w->u->view(), d_sig, d_dec);
  ts.mark(ctx->stream, 1);
  HIPCHK(hipGetLastError());
  unsigned long long dec = ~0ull;
  HIPCHK(hipMemcpyAsync(sig, d_sig, (size_t)w->n_inst * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&dec, d_dec, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ts.fetch(ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kernel_ms) *kernel_ms = ts.ms(ctx, 0, 1);
  if (dec != ~0ull) return uw_declined(decline, dec);
  return HAWK_OK;
}

int hawk_uwin_group(hawk_uwin* w, const uint64_t* sig, uint32_t* head, float* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.f;
  if (!w || (w->n_inst && (!sig || !head))) return HAWK_E_INVALID;
  if (!w->n_inst) return HAWK_OK;
  hawk_ctx* ctx = w->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  unsigned long long* d_sig = nullptr;
  uint32_t* d_head = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_sig, (size_t)w->n_inst * 16); TEMPCHK(tmp, &d_head, (size_t)w->n_inst * 4);
  HIPCHK(hipMemcpyAsync(d_sig, sig, (size_t)w->n_inst * 16, hipMemcpyHostToDevice, ctx->stream));
  UwStamps ts;
  if (int rc = ts.init(tmp, ctx->stream)) return rc;
  ts.mark(ctx->stream, 0);
  hawk_launch_uw_group(ctx->stream, w->view(), w->u->view(), d_sig, d_head);
  ts.mark(ctx->stream, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(head, d_head, (size_t)w->n_inst * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ts.fetch(ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kernel_ms) *kernel_ms = ts.ms(ctx, 0, 1);
  return HAWK_OK;
}

int hawk_uwin_fill(hawk_uwin* w, hawk_hapset* hs, uint32_t ref_row, uint32_t first_row, uint32_t n_rows, const uint32_t* row_inst,
                   float* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.f;
  if (!w || !hs || hs->vplan || hs->ctx != w->ctx || (n_rows && !row_inst)) return HAWK_E_INVALID;
  // every row the kernel writes lies in the set and is as long as its instance's window row, REF is not among them and holds the
  // whole region, every instance exists
  if (ref_row >= hs->n_hap || first_row > hs->n_hap || n_rows > hs->n_hap - first_row) return HAWK_E_INVALID;
  if (ref_row >= first_row && ref_row - first_row < n_rows) return HAWK_E_INVALID;
  if (hs->hap_len[ref_row] != w->L) return HAWK_E_INVALID;
  if (hs->S % 4u) return HAWK_E_UNSUPPORTED;
  uint32_t longest = 0;
  for (uint32_t r = 0; r < n_rows; ++r) {
    if (row_inst[r] >= w->n_inst) return HAWK_E_INVALID;
    const uint32_t k = (uint32_t)(std::upper_bound(w->h_inst_off.begin(), w->h_inst_off.end(), (uint64_t)row_inst[r]) - w->h_inst_off.begin()) - 1u;
    UwGeom g;
    if (k >= w->n_indel || uw_geometry(w->h_off[k], w->h_ref_len[k], w->h_alt_len[k], w->L, &g)) return HAWK_E_INVALID;
    if (hs->hap_len[first_row + r] != g.rowlen || (uint64_t)g.rowlen > 32ull * hs->S) return HAWK_E_INVALID;
    longest = std::max(longest, g.rowlen);
  }
  if (!n_rows) return HAWK_OK;
  hawk_ctx* ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hs->refbits_valid = false;
  uint32_t* d_ri = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_ri, (size_t)n_rows * 4);
  HIPCHK(hipMemcpyAsync(d_ri, row_inst, (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
  UwStamps ts;
  if (int rc = ts.init(tmp, ctx->stream)) return rc;
  ts.mark(ctx->stream, 0);
  for (int pl = 0; pl < HAWK_PLANES; ++pl)  // the dead words of the rows, once: the kernel writes the live quads alone
    HIPCHK(hipMemsetAsync(hs->plane[pl] + (size_t)first_row * hs->S, 0, (size_t)n_rows * hs->S * 4, ctx->stream));
  hawk_launch_uw_fill(ctx->stream, hs->plane, hs->S, ref_row, first_row, n_rows, (longest + 127u) / 128u, d_ri, w->view(), w->u->view());
  ts.mark(ctx->stream, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(ts.fetch(ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kernel_ms) *kernel_ms = ts.ms(ctx, 0, 1);  // the clearing of the rows and the fill kernel
  return HAWK_OK;
}

}  // extern "C"
