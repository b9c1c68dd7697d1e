// hawk_api_plm.hip - C ABI: PLM-CRISPR (hawk_plm_create / _protein / _score / _timing / _free; kernels in hawk_plm.hip)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "hawk_host.h"
#include "hawk_plm.h"

static_assert(PLM_NPARAMS == HAWK_PLM_NPARAMS, "include/hawk.h documents the packed block");

struct hawk_plm {
  hawk_ctx* ctx;
  uint32_t L;
  DevBuf params, aux, prot;  // the packed block, the unit-innermost copies of the small weights, out_protein[256]
  bool timed = false;
  float ms[4] = {0.f, 0.f, 0.f, 0.f};  // front, lin1, lin3, tail of the last timed hawk_plm_score
};

static void plm_release(hawk_plm* p) {
  p->params.release(); p->aux.release(); p->prot.release();
  delete p;
}

extern "C" {

int hawk_plm_create(hawk_ctx* ctx, const float* params, const float* protein, uint32_t L, hawk_plm** out) {
  if (!ctx || !params || !protein || !out || L < PLM_MIN_L) return HAWK_E_INVALID;
  *out = nullptr;
  HIPCHK(hipSetDevice(ctx->device));
  // the small weights once more with the output unit innermost
  std::vector<float> aux(PLM_NAUX);
  auto unit_inner = [&](size_t dst, size_t src, int units, int per_unit) {
    for (int u = 0; u < units; ++u)
      for (int k = 0; k < per_unit; ++k) aux[dst + (size_t)k * units + u] = params[src + (size_t)u * per_unit + k];
  };
  unit_inner(PLM_X_C1, PLM_O_C1W, PLM_CH, PLM_SYM * PLM_KW);
  unit_inner(PLM_X_C4, PLM_O_C4W, PLM_CH, PLM_SYM * PLM_KW);
  unit_inner(PLM_X_C2, PLM_O_C2W, PLM_CH, PLM_CH * PLM_KW);
  unit_inner(PLM_X_C3, PLM_O_C3W, PLM_CH, PLM_CH * PLM_KW);
  unit_inner(PLM_X_W0, PLM_O_W0W, PLM_H5, 2 * PLM_H3);
  unit_inner(PLM_X_L5, PLM_O_L5W, PLM_H5, PLM_H3);
  hawk_plm* p = new (std::nothrow) hawk_plm();
  if (!p) return HAWK_E_INVALID;
  p->ctx = ctx;
  p->L = L;
  struct Guard { hawk_plm* p; ~Guard() { if (p) plm_release(p); } } guard{p};
  int rc;
  if ((rc = p->params.reserve((size_t)PLM_NPARAMS * 4)) || (rc = p->aux.reserve((size_t)PLM_NAUX * 4)) || (rc = p->prot.reserve(PLM_H3 * 4)))
    return rc;
  float* d_emb = nullptr; uint32_t* d_pool = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_emb, (size_t)L * PLM_EMB * 4); TEMPCHK(tmp, &d_pool, PLM_PFEAT * 4);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(p->params.p, params, (size_t)PLM_NPARAMS * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(p->aux.p, aux.data(), (size_t)PLM_NAUX * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_emb, protein, (size_t)L * PLM_EMB * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_pool, 0, PLM_PFEAT * 4, st));
  hawk_launch_plm_protein(st, p->params.as<float>(), d_emb, L, d_pool, p->prot.as<float>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  guard.p = nullptr;
  *out = p;
  return HAWK_OK;
}

int hawk_plm_protein(hawk_plm* p, float* out256) {
  if (!p || !out256) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(p->ctx->device));
  HIPCHK(hipMemcpyAsync(out256, p->prot.p, PLM_H3 * 4, hipMemcpyDeviceToHost, p->ctx->stream));
  HIPCHK(hipStreamSynchronize(p->ctx->stream));
  return HAWK_OK;
}

int hawk_plm_timing(hawk_plm* p, int enable, float* ms4) {
  if (!p) return HAWK_E_INVALID;
  if (ms4) std::copy(p->ms, p->ms + 4, ms4);
  p->timed = enable != 0;
  return HAWK_OK;
}

int hawk_plm_score(hawk_plm* p, const char* seqs, uint32_t len, uint64_t n, uint32_t batch, float* out) {
  if (!p || len != PLM_GUIDE || (n && (!seqs || !out))) return HAWK_E_INVALID;
  if (!n) return HAWK_OK;
  hawk_ctx* ctx = p->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t B = std::min<uint64_t>(std::min<uint32_t>(batch ? batch : PLM_DEFAULT_BATCH, HAWK_PLM_MAX_BATCH), n);
  char* d_s = nullptr; float *d_o = nullptr, *d_feat = nullptr, *d_h1 = nullptr, *d_h3 = nullptr; int* d_status = nullptr;
  PoolScope tmp;
  TEMPCHK(tmp, &d_s, n * PLM_GUIDE); TEMPCHK(tmp, &d_o, n * 4); TEMPCHK(tmp, &d_status, 4);
  TEMPCHK(tmp, &d_feat, B * PLM_FEAT * 4); TEMPCHK(tmp, &d_h1, B * PLM_H1 * 4); TEMPCHK(tmp, &d_h3, B * PLM_H3 * 4);
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(d_s, seqs, n * PLM_GUIDE, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_status, 0, 4, st));
  const float* w = p->params.as<float>();
  const float* aux = p->aux.as<float>();
  if (p->timed) std::fill(p->ms, p->ms + 4, 0.f);
  for (uint64_t g0 = 0; g0 < n; g0 += B) {
    const uint64_t nb = std::min(B, n - g0);
    if (p->timed) HIPCHK(hipEventRecord(ctx->ev[0], st));
    hawk_launch_plm_front(st, d_s + g0 * PLM_GUIDE, nb, w, aux, d_feat, d_status);
    if (p->timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
    hawk_launch_plm_lin(st, d_feat, nb, PLM_FEAT, w + PLM_O_L1W, w + PLM_O_L1B, PLM_H1, true, d_h1);
    if (p->timed) HIPCHK(hipEventRecord(ctx->ev[2], st));
    hawk_launch_plm_lin(st, d_h1, nb, PLM_H1, w + PLM_O_L3W, w + PLM_O_L3B, PLM_H3, false, d_h3);
    if (p->timed) HIPCHK(hipEventRecord(ctx->ev[3], st));
    hawk_launch_plm_tail(st, d_h3, nb, p->prot.as<float>(), w, aux, d_o + g0);
    HIPCHK(hipGetLastError());
    if (p->timed) {  // the timed mode waits for every batch: its events are this call's scratch (hawk_host.h)
      HIPCHK(hipEventRecord(ctx->ev[4], st));
      HIPCHK(hipEventSynchronize(ctx->ev[4]));
      for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev[k], ctx->ev[k + 1]));
        p->ms[k] += ms;
      }
    }
  }
  int status = 0;
  HIPCHK(hipMemcpyAsync(out, d_o, n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return status;
}

void hawk_plm_free(hawk_plm* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);  // nothing queued may still read the blocks
  plm_release(p);
}

}  // extern "C"
