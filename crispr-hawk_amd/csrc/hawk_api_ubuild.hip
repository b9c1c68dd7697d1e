// hawk_api_ubuild.hip - C ABI: the whole-region rows of an unphased VCF built on the device (include/hawk.h; kernels:
// hawk_ubuild.hip; hawk_gt_parse_unphased itself sits beside hawk_gt_parse in hawk_api_vcf.hip)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "hawk_host.h"

extern "C" {

void hawk_ubuild_free(hawk_ubuild* u) {
  if (!u) return;
  (void)hipSetDevice(u->ctx->device);
  (void)hipStreamSynchronize(u->ctx->stream);
  for (DevBuf* b : {&u->off, &u->idx, &u->var_off, &u->var_mask, &u->var_ref}) b->release();
  delete u;
}

int hawk_ubuild_lists(hawk_gt* g, const uint32_t* var_line, const uint8_t* var_allele, const uint32_t* var_off, const uint8_t* var_mask,
                      const uint8_t* var_ref, uint32_t n_var, uint64_t* sample_off, hawk_ubuild** out, float* kernel_ms) {
  if (out) *out = nullptr;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!g || !sample_off || !out || (n_var && (!var_line || !var_allele || !var_off || !var_mask || !var_ref))) return HAWK_E_INVALID;
  // everything the kernels index with or shift by is checked here
  for (uint32_t j = 0; j < n_var; ++j)
    if (var_line[j] >= g->n_lines || var_allele[j] == 0 || var_allele[j] == 255 || var_ref[j] > 3 || var_mask[j] > 15 ||
        (j && var_off[j] < var_off[j - 1]))
      return HAWK_E_INVALID;
  hawk_ctx* ctx = g->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t ns = g->n_samples, n_chunk = (n_var + 63u) / 64u;
  if ((n_chunk + 15u) / 16u > 65535u) return HAWK_E_UNSUPPORTED;  // k_ub_count's grid: 16 chunks of 64 variants per block row
  hawk_ubuild* u = new (std::nothrow) hawk_ubuild();
  if (!u) return HAWK_E_INVALID;
  u->ctx = ctx; u->n_samples = ns; u->n_var = n_var; u->max_off = n_var ? var_off[n_var - 1] : 0;
  u->h_off.assign((size_t)ns + 1, 0);
  struct Guard { hawk_ubuild* u; ~Guard() { if (u) hawk_ubuild_free(u); } } guard{u};
  int rc;
  if ((rc = u->off.reserve(((size_t)ns + 1) * 8)) || (rc = u->var_off.reserve(std::max<size_t>(n_var, 1) * 4)) ||
      (rc = u->var_mask.reserve(std::max<size_t>(n_var, 1))) || (rc = u->var_ref.reserve(std::max<size_t>(n_var, 1))))
    return rc;
  if (n_var) {
    uint32_t *d_vl = nullptr, *d_cnt = nullptr; uint8_t* d_va = nullptr;
    unsigned long long* d_bal = nullptr;
    PoolScope tmp;
    TEMPCHK(tmp, &d_vl, (size_t)n_var * 4); TEMPCHK(tmp, &d_va, n_var); TEMPCHK(tmp, &d_cnt, (size_t)ns * 4);
    TEMPCHK(tmp, &d_bal, (size_t)ns * n_chunk * 8);
    HIPCHK(hipMemcpyAsync(d_vl, var_line, (size_t)n_var * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_va, var_allele, n_var, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(u->var_off.p, var_off, (size_t)n_var * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(u->var_mask.p, var_mask, n_var, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(u->var_ref.p, var_ref, n_var, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    hawk_launch_ub_count(st, g->d_codes, ns, d_vl, d_va, n_var, d_bal, d_cnt);
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> cnt(ns);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)ns * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t s = 0; s < ns; ++s) u->h_off[s + 1] = u->h_off[s] + cnt[s];  // n_samples values: a host prefix sum
    u->n_entries = u->h_off[ns];
    if (u->n_entries > UB_MAX_ENTRIES) return HAWK_E_CAPACITY;
    if ((rc = u->idx.reserve(std::max<size_t>(u->n_entries, 1) * 4))) return rc;
    HIPCHK(hipMemcpyAsync(u->off.p, u->h_off.data(), ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    hawk_launch_ub_fill(st, ns, n_var, d_bal, u->off.as<uint64_t>(), u->idx.as<uint32_t>());
    HIPCHK(hipEventRecord(ctx->ev[3], st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms) {
      float a = 0.f, b = 0.f;
      (void)hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]); (void)hipEventElapsedTime(&b, ctx->ev[2], ctx->ev[3]);
      *kernel_ms = a + b;
    }
  } else {
    if ((rc = u->idx.reserve(4))) return rc;
    HIPCHK(hipMemsetAsync(u->off.p, 0, ((size_t)ns + 1) * 8, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  memcpy(sample_off, u->h_off.data(), ((size_t)ns + 1) * 8);
  guard.u = nullptr;
  *out = u;
  return HAWK_OK;
}

int hawk_ubuild_lists_download(hawk_ubuild* u, uint32_t* idx) {
  if (!u || (u->n_entries && !idx)) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(u->ctx->device));
  if (u->n_entries) HIPCHK(hipMemcpyAsync(idx, u->idx.p, u->n_entries * 4, hipMemcpyDeviceToHost, u->ctx->stream));
  HIPCHK(hipStreamSynchronize(u->ctx->stream));
  return HAWK_OK;
}

int hawk_ubuild_signatures(hawk_ubuild* u, uint64_t* sig, int64_t* decline_var, float* kernel_ms) {
  if (decline_var) *decline_var = -1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!u || !sig) return HAWK_E_INVALID;
  hawk_ctx* ctx = u->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  unsigned long long *d_sig = nullptr, *d_dec = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_sig, (size_t)u->n_samples * 16); TEMPCHK(tmp, &d_dec, 8);
  HIPCHK(hipMemsetAsync(d_dec, 0xff, 8, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  hawk_launch_ub_sig(ctx->stream, u->view(), d_sig, d_dec);
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipGetLastError());
  unsigned long long dec = ~0ull;
  HIPCHK(hipMemcpyAsync(sig, d_sig, (size_t)u->n_samples * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&dec, d_dec, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, ctx->ev[0], ctx->ev[1]);
  if (dec != ~0ull) {
    if (decline_var) *decline_var = (int64_t)dec;
    return HAWK_E_UNSUPPORTED;
  }
  return HAWK_OK;
}

int hawk_ubuild_fill(hawk_ubuild* u, hawk_hapset* hs, uint32_t ref_row, uint32_t first_row, uint32_t n_rows, const uint32_t* row_sample,
                     int64_t* decline_var, float* kernel_ms) {
  if (decline_var) *decline_var = -1;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!u || !hs || hs->vplan || hs->ctx != u->ctx || (n_rows && !row_sample)) return HAWK_E_INVALID;
  // every row the kernel writes lies in the set and is as long as REF, REF is not among them, every list expanded exists and no
  // site lies past REF's end
  if (ref_row >= hs->n_hap || first_row > hs->n_hap || n_rows > hs->n_hap - first_row) return HAWK_E_INVALID;
  if (ref_row >= first_row && ref_row - first_row < n_rows) return HAWK_E_INVALID;
  const uint32_t len = hs->hap_len[ref_row];
  for (uint32_t r = 0; r < n_rows; ++r)
    if (hs->hap_len[first_row + r] != len || row_sample[r] >= u->n_samples) return HAWK_E_INVALID;
  if (u->n_var && u->max_off >= len) return HAWK_E_INVALID;
  if (hs->S % 4u || (uint64_t)n_rows * (hs->S / 4u) / 256u >= 0x7fffffffull) return HAWK_E_UNSUPPORTED;
  if (!n_rows) return HAWK_OK;
  hawk_ctx* ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hs->refbits_valid = false;
  uint32_t* d_rs = nullptr;
  unsigned long long* d_dec = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_rs, (size_t)n_rows * 4); TEMPCHK(tmp, &d_dec, 8);
  HIPCHK(hipMemcpyAsync(d_rs, row_sample, (size_t)n_rows * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(d_dec, 0xff, 8, ctx->stream));
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  hawk_launch_ub_rows(ctx->stream, hs->plane, hs->S, ref_row, first_row, n_rows, d_rs, u->view(), d_dec);
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipGetLastError());
  unsigned long long dec = ~0ull;
  HIPCHK(hipMemcpyAsync(&dec, d_dec, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, ctx->ev[0], ctx->ev[1]);
  if (dec != ~0ull) {
    if (decline_var) *decline_var = (int64_t)dec;
    return HAWK_E_UNSUPPORTED;
  }
  return HAWK_OK;
}

int hawk_hapset_pack_ascii_rows(hawk_hapset* hs, uint32_t first_row, uint32_t n_rows, const char* seqs, const uint64_t* seq_off,
                                uint64_t* bad_index) {
  if (!hs || hs->vplan || (n_rows && (!seqs || !seq_off))) return HAWK_E_INVALID;
  if (first_row > hs->n_hap || n_rows > hs->n_hap - first_row) return HAWK_E_INVALID;
  if (!n_rows) return HAWK_OK;
  for (uint32_t i = 0; i < n_rows; ++i)
    if (seq_off[i + 1] < seq_off[i] || seq_off[i + 1] - seq_off[i] != hs->hap_len[first_row + i]) return HAWK_E_INVALID;
  hs->refbits_valid = false;
  hawk_ctx* ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  // k_pack indexes the offsets by the row's number in the set: the range's offsets sit at theirs, the rest is never read
  std::vector<uint64_t> off((size_t)hs->n_hap + 1, 0);
  for (uint32_t i = 0; i <= n_rows; ++i) off[first_row + i] = seq_off[i];
  uint64_t* d_off = nullptr;
  unsigned long long* d_bad = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_off, off.size() * 8);
  TEMPCHK(tmp, &d_bad, 8);
  HIPCHK(hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, 8, ctx->stream));
  const uint64_t kStage = 256ull << 20;  // whole rows per batch, as hawk_hapset_pack_ascii stages them
  uint64_t maxlen = 0, total = seq_off[n_rows] - seq_off[0];
  for (uint32_t i = 0; i < n_rows; ++i) maxlen = std::max<uint64_t>(maxlen, hs->hap_len[first_row + i]);
  const uint64_t stage_bytes = std::max(kStage, maxlen);
  uint8_t* d_stage = nullptr;
  TEMPCHK(tmp, &d_stage, std::min<uint64_t>(stage_bytes, std::max<uint64_t>(total, 1)));
  uint32_t i0 = 0;
  while (i0 < n_rows) {
    uint32_t i1 = i0;
    uint64_t bytes = 0;
    while (i1 < n_rows && (i1 == i0 || bytes + hs->hap_len[first_row + i1] <= stage_bytes)) { bytes += hs->hap_len[first_row + i1]; ++i1; }
    if (bytes) HIPCHK(hipMemcpyAsync(d_stage, seqs + seq_off[i0], bytes, hipMemcpyHostToDevice, ctx->stream));
    hawk_launch_pack(ctx->stream, d_stage, d_off, first_row + i0, i1 - i0, seq_off[i0], hs->d_hap_len, hs->S, hs->plane, d_bad);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));  // the staging buffer is reused by the next batch
    i0 = i1;
  }
  unsigned long long bad = ~0ull;
  HIPCHK(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
  if (bad != ~0ull) {
    if (bad_index) *bad_index = bad;
    return HAWK_E_IUPAC;
  }
  return HAWK_OK;
}

}  // extern "C"
