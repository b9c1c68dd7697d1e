// hawk_api_effects.hip - C ABI: variant effects on the report groups of a collapsed table (hawk_effects.hip) behind an opaque
// handle: hawk_effects_create / _create_columns run the score-independent passes once, hawk_effects_rank runs once per score
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "hawk_host.h"

struct hawk_effects {
  hawk_ctx* ctx;
  uint64_t G = 0;
  uint32_t guidelen = 0, pamlen = 0, right = 0, n_sample_ids = 0;
  bool has_cfdon = false, ranked = false;
  uint32_t n_chosen = 0, K = 0;
  uint64_t n_alts = 0;
  DevBuf start, strand, is_ref, rank, cfdon;                                     // the handle's own copies of what a rank call reads
  DevBuf head, type, dup, nsamp, counts;                                         // written once, by create
  DevBuf score, rs, delta, adelta, pref, pworst, pnv, pfr;                       // written by every rank call
  DevBuf cand_s, cand_t, chosen, part, alt_off, alt_group;
};

static void fx_release(hawk_effects* f) {
  for (DevBuf* b : {&f->start, &f->strand, &f->is_ref, &f->rank, &f->cfdon, &f->head, &f->type, &f->dup, &f->nsamp, &f->counts, &f->score, &f->rs,
                    &f->delta, &f->adelta, &f->pref, &f->pworst, &f->pnv, &f->pfr, &f->cand_s, &f->cand_t, &f->chosen, &f->part,
                    &f->alt_off, &f->alt_group})
    b->release();
  delete f;
}

static FxDev fx_dev(const hawk_effects* f) {
  FxDev F;
  memset(&F, 0, sizeof(F));
  F.c.n_groups = f->G;
  F.c.start = f->start.as<int64_t>(); F.c.strand = f->strand.as<uint8_t>(); F.c.is_ref = f->is_ref.as<uint8_t>(); F.c.rank = f->rank.as<uint32_t>();
  F.c.guidelen = f->guidelen; F.c.pamlen = f->pamlen; F.c.right = f->right; F.c.n_sample_ids = f->n_sample_ids;
  F.head = f->head.as<uint32_t>(); F.type = f->type.as<uint8_t>(); F.dup = f->dup.as<uint8_t>(); F.n_samples = f->nsamp.as<uint32_t>();
  F.counts = f->counts.as<unsigned long long>();
  F.rs = f->rs.as<double>(); F.delta = f->delta.as<double>(); F.abs_delta = f->adelta.as<double>();
  F.pos_ref = f->pref.as<uint32_t>(); F.pos_worst = f->pworst.as<double>(); F.pos_nvalid = f->pnv.as<uint32_t>(); F.pos_first_rank = f->pfr.as<uint32_t>();
  F.cand_start = f->cand_s.as<int64_t>(); F.cand_strand = f->cand_t.as<uint8_t>();
  F.chosen = f->chosen.as<uint32_t>(); F.part = f->part.as<FxEntry>();
  F.alt_off = f->alt_off.as<uint64_t>(); F.alt_group = f->alt_group.as<uint32_t>();
  return F;
}

// The score-independent passes.  `src` holds DEVICE pointers of everything create reads and the handle does not keep: stop, win,
// the member lists, the haplotype rows' origin and sample lists.  f->start / strand / rank are filled already.  d_hap_is_ref NULL:
// f->is_ref is filled already as well (hawk_effects_create_ugroups: the groups carry their origin).
static int fx_build(hawk_effects* f, const FxCols& src, const uint8_t* d_hap_is_ref, hawk_effects_timing* timing, hipEvent_t ev_begin) {
  hawk_ctx* ctx = f->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t G = f->G;
  int rc;
  if ((rc = f->is_ref.reserve(G + 1)) || (rc = f->head.reserve(G * 4 + 4)) || (rc = f->type.reserve(G + 1)) || (rc = f->dup.reserve(G + 1)) ||
      (rc = f->nsamp.reserve(G * 4 + 4)) || (rc = f->counts.reserve(64)))
    return rc;
  PoolScope tmp;
  uint32_t* d_long;
  TEMPCHK(tmp, &d_long, G * 4 + 4);
  HIPCHK(hipMemsetAsync(f->counts.p, 0, 64, st));
  if (d_hap_is_ref) hawk_launch_fx_isref_gather(st, d_hap_is_ref, src.member_hap, src.member_off, G, f->is_ref.as<uint8_t>());
  FxDev F = fx_dev(f);
  F.c = src;
  F.c.n_groups = G;
  F.c.start = f->start.as<int64_t>(); F.c.strand = f->strand.as<uint8_t>(); F.c.is_ref = f->is_ref.as<uint8_t>(); F.c.rank = f->rank.as<uint32_t>();
  F.long_list = d_long;
  HIPCHK(hipEventRecord(ctx->ev[1], st));
  hawk_launch_fx_groups(st, F);
  HIPCHK(hipEventRecord(ctx->ev[2], st));
  hawk_launch_fx_samples(st, F);
  HIPCHK(hipEventRecord(ctx->ev[3], st));
  HIPCHK(hipGetLastError());
  unsigned long long counts[8];
  HIPCHK(hipMemcpyAsync(counts, f->counts.p, 64, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the caller's arrays and the table's workspace may go once this returns
  if (timing) {
    memset(timing, 0, sizeof(*timing));
    (void)hipEventElapsedTime(&timing->upload_ms, ev_begin, ctx->ev[1]);
    (void)hipEventElapsedTime(&timing->groups_ms, ctx->ev[1], ctx->ev[2]);
    (void)hipEventElapsedTime(&timing->samples_ms, ctx->ev[2], ctx->ev[3]);
    (void)hipEventElapsedTime(&timing->total_ms, ev_begin, ctx->ev[3]);
    timing->n_groups = G; timing->n_positions = counts[5]; timing->n_long = counts[6];
  }
  return HAWK_OK;
}

extern "C" {

int hawk_effects_create_columns(hawk_ctx* ctx, const hawk_effects_columns* cols, hawk_effects** out, hawk_effects_timing* timing) {
  if (!ctx || !cols || !out) return HAWK_E_INVALID;
  FxCols c;
  memset(&c, 0, sizeof(c));
  c.n_groups = cols->n_groups; c.win_stride = cols->win_stride; c.start = cols->start; c.stop = cols->stop; c.strand = cols->strand; c.win = cols->win;
  c.member_off = cols->member_off; c.member_hap = cols->member_hap; c.hap_off = cols->hap_off; c.sample_id = cols->sample_id; c.rank = cols->rank;
  c.n_hap = cols->n_hap; c.n_sample_ids = cols->n_sample_ids; c.guidelen = cols->guidelen; c.pamlen = cols->pamlen; c.right = cols->right;
  const int bad = fx_check_cols(c);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  const uint64_t G = c.n_groups;
  if (G && !cols->hap_is_ref) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hawk_effects* f = new (std::nothrow) hawk_effects();
  if (!f) return HAWK_E_INVALID;
  f->ctx = ctx; f->G = G; f->guidelen = c.guidelen; f->pamlen = c.pamlen; f->right = c.right; f->n_sample_ids = c.n_sample_ids;
  f->has_cfdon = cols->cfdon != nullptr;
  hipStream_t st = ctx->stream;
  const uint64_t N = G ? c.member_off[G] : 0, NS = c.hap_off[c.n_hap];
  PoolScope tmp;
  int64_t* d_stop; uint64_t *d_win, *d_moff, *d_hoff; uint32_t *d_mhap, *d_sid; uint8_t* d_href;
  int rc = HAWK_OK;
  auto fail = [&](int code) { fx_release(f); return code; };
  if ((rc = f->start.reserve(G * 8 + 8)) || (rc = f->strand.reserve(G + 1)) || (rc = f->rank.reserve(G * 4 + 4)) || (rc = f->cfdon.reserve(G * 8 + 8)) ||
      (rc = tmp.alloc((void**)&d_stop, G * 8 + 8)) || (rc = tmp.alloc((void**)&d_win, G * 8 * FX_PLANES + 8)) || (rc = tmp.alloc((void**)&d_moff, (G + 1) * 8)) ||
      (rc = tmp.alloc((void**)&d_mhap, N * 4 + 4)) || (rc = tmp.alloc((void**)&d_hoff, ((uint64_t)c.n_hap + 1) * 8)) || (rc = tmp.alloc((void**)&d_sid, NS * 4 + 4)) ||
      (rc = tmp.alloc((void**)&d_href, (uint64_t)c.n_hap + 1)))
    return fail(rc);
  hipError_t e = hipEventRecord(ctx->ev[0], st);
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
  };
  up(f->start.p, c.start, G * 8); up(f->strand.p, c.strand, G); up(f->rank.p, c.rank, G * 4);
  if (cols->cfdon) up(f->cfdon.p, cols->cfdon, G * 8);
  up(d_stop, c.stop, G * 8);
  for (int p = 0; p < FX_PLANES; ++p) up(d_win + (uint64_t)p * G, c.win + (uint64_t)p * c.win_stride, G * 8);
  up(d_moff, c.member_off, G ? (G + 1) * 8 : 0); up(d_mhap, c.member_hap, N * 4);
  up(d_hoff, c.hap_off, ((uint64_t)c.n_hap + 1) * 8); up(d_sid, c.sample_id, NS * 4); up(d_href, cols->hap_is_ref, G ? c.n_hap : 0);
  if (e != hipSuccess) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_effects_create_columns: %s", hipGetErrorString(e));
    return fail(HAWK_E_HIP);
  }
  FxCols d = c;
  d.stop = d_stop; d.win = d_win; d.win_stride = G; d.member_off = d_moff; d.member_hap = d_mhap; d.hap_off = d_hoff; d.sample_id = d_sid;
  if ((rc = fx_build(f, d, d_href, timing, ctx->ev[0]))) return fail(rc);
  *out = f;
  return HAWK_OK;
}

int hawk_effects_create(hawk_table* t, const uint32_t* rank, const uint64_t* hap_off, const uint32_t* sample_id, uint32_t n_hap,
                        uint32_t n_sample_ids, hawk_effects** out, hawk_effects_timing* timing) {
  if (!out || !collapse_valid(t)) return HAWK_E_INVALID;
  hawk_hapset* hs = t->hs;
  hawk_ctx* ctx = hs->ctx;
  const uint64_t n = t->n_rows, G = n ? t->n_groups : 0;
  if (n_hap != hs->n_hap) return HAWK_E_INVALID;
  int bad = fx_check_sizes(G, n_sample_ids, t->guidelen, t->pamlen);
  if (!bad) bad = fx_check_samples(hap_off, sample_id, n_hap, n_sample_ids);
  if (!bad) bad = fx_check_rank(rank, G);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hawk_effects* f = new (std::nothrow) hawk_effects();
  if (!f) return HAWK_E_INVALID;
  f->ctx = ctx; f->G = G; f->guidelen = t->guidelen; f->pamlen = t->pamlen; f->right = t->right; f->n_sample_ids = n_sample_ids;
  f->has_cfdon = true;
  hipStream_t st = ctx->stream;
  auto fail = [&](int code) { fx_release(f); return code; };
  const uint64_t NS = hap_off[n_hap];
  PoolScope tmp;
  uint64_t* d_hoff; uint32_t* d_sid;
  int rc;
  GuideCols rep;
  memset(&rep, 0, sizeof(rep));
  if ((rc = f->start.reserve(G * 8 + 8)) || (rc = f->strand.reserve(G + 1)) || (rc = f->rank.reserve(G * 4 + 4)) || (rc = f->cfdon.reserve(G * 8 + 8)) ||
      (rc = tmp.alloc((void**)&d_hoff, ((uint64_t)n_hap + 1) * 8)) || (rc = tmp.alloc((void**)&d_sid, NS * 4 + 4)) ||
      (G && (rc = hawk_reserve_cols(hs->cws.rep, G, &rep))))
    return fail(rc);
  hipError_t e = hipEventRecord(ctx->ev[0], st);
  uint32_t* d_mem = hs->cws.members();  // the group export, as hawk_table_collapse_export runs it: representatives + members
  if (e == hipSuccess && G) {
    hawk_launch_collapse_export(st, t->cols, n, G, hs->cws.perm(n), hs->cws.group_off(), rep, d_mem);
    e = hipGetLastError();
  }
  auto cp = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, kind, st);
  };
  cp(f->start.p, rep.start, G * 8, hipMemcpyDeviceToDevice); cp(f->strand.p, rep.strand, G, hipMemcpyDeviceToDevice);
  cp(f->cfdon.p, rep.cfdon, G * 8, hipMemcpyDeviceToDevice); cp(f->rank.p, rank, G * 4, hipMemcpyHostToDevice);
  cp(d_hoff, hap_off, ((uint64_t)n_hap + 1) * 8, hipMemcpyHostToDevice); cp(d_sid, sample_id, NS * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_effects_create: %s", hipGetErrorString(e));
    return fail(HAWK_E_HIP);
  }
  FxCols d;
  memset(&d, 0, sizeof(d));
  d.n_groups = G; d.win_stride = rep.cap; d.stop = rep.stop; d.win = rep.win; d.member_off = hs->cws.group_off(); d.member_hap = d_mem;
  d.hap_off = d_hoff; d.sample_id = d_sid; d.n_hap = n_hap; d.n_sample_ids = n_sample_ids; d.guidelen = t->guidelen; d.pamlen = t->pamlen; d.right = t->right;
  if ((rc = fx_build(f, d, hs->d_is_ref, timing, ctx->ev[0]))) return fail(rc);
  *out = f;
  return HAWK_OK;
}

int hawk_effects_create_ugroups(hawk_ugroups* g, const uint32_t* rank, const uint64_t* hap_off, const uint32_t* sample_id, uint32_t n_hap,
                                uint32_t n_sample_ids, hawk_effects** out, hawk_effects_timing* timing) {
  if (out) *out = nullptr;
  if (!out || !g) return HAWK_E_INVALID;
  hawk_ctx* ctx = g->ctx;
  const uint64_t G = g->n_groups;
  if (n_hap != g->n_hap) return HAWK_E_INVALID;
  int bad = fx_check_sizes(G, n_sample_ids, g->guidelen, g->pamlen);
  if (!bad) bad = fx_check_samples(hap_off, sample_id, n_hap, n_sample_ids);
  if (!bad) bad = fx_check_rank(rank, G);
  if (bad) return bad == 2 ? HAWK_E_UNSUPPORTED : HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  hawk_effects* f = new (std::nothrow) hawk_effects();
  if (!f) return HAWK_E_INVALID;
  f->ctx = ctx; f->G = G; f->guidelen = g->guidelen; f->pamlen = g->pamlen; f->right = g->right; f->n_sample_ids = n_sample_ids;
  f->has_cfdon = g->has_cfd;
  hipStream_t st = ctx->stream;
  auto fail = [&](int code) { fx_release(f); return code; };
  const uint64_t NS = hap_off[n_hap];
  PoolScope tmp;
  uint64_t* d_hoff; uint32_t* d_sid;
  int rc;
  if ((rc = f->start.reserve(G * 8 + 8)) || (rc = f->strand.reserve(G + 1)) || (rc = f->rank.reserve(G * 4 + 4)) || (rc = f->cfdon.reserve(G * 8 + 8)) ||
      (rc = f->is_ref.reserve(G + 1)) || (rc = tmp.alloc((void**)&d_hoff, ((uint64_t)n_hap + 1) * 8)) || (rc = tmp.alloc((void**)&d_sid, NS * 4 + 4)))
    return fail(rc);
  hipError_t e = hipEventRecord(ctx->ev[0], st);
  auto cp = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(dst, src, bytes, kind, st);
  };
  // the handle's own copies (it outlives `g`); stop, the window planes and the member lists are read in place, by create alone
  cp(f->start.p, g->b[UG_B_START].p, G * 8, hipMemcpyDeviceToDevice); cp(f->strand.p, g->b[UG_B_STRAND].p, G, hipMemcpyDeviceToDevice);
  cp(f->cfdon.p, g->b[UG_B_CFDON].p, G * 8, hipMemcpyDeviceToDevice); cp(f->is_ref.p, g->b[UG_B_ISREF].p, G, hipMemcpyDeviceToDevice);
  cp(f->rank.p, rank, G * 4, hipMemcpyHostToDevice);
  cp(d_hoff, hap_off, ((uint64_t)n_hap + 1) * 8, hipMemcpyHostToDevice); cp(d_sid, sample_id, NS * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    snprintf(hawk_hip_err_buf(), 256, "hawk_effects_create_ugroups: %s", hipGetErrorString(e));
    (void)hipStreamSynchronize(st);
    return fail(HAWK_E_HIP);
  }
  FxCols d;
  memset(&d, 0, sizeof(d));
  d.n_groups = G; d.win_stride = G; d.stop = g->b[UG_B_STOP].as<int64_t>(); d.win = g->b[UG_B_WIN].as<uint64_t>();
  d.member_off = g->b[UG_B_MOFF].as<uint64_t>(); d.member_hap = g->b[UG_B_MHAP].as<uint32_t>();
  d.hap_off = d_hoff; d.sample_id = d_sid; d.n_hap = n_hap; d.n_sample_ids = n_sample_ids; d.guidelen = g->guidelen; d.pamlen = g->pamlen; d.right = g->right;
  if ((rc = fx_build(f, d, nullptr, timing, ctx->ev[0]))) {
    (void)hipStreamSynchronize(st);
    return fail(rc);
  }
  *out = f;
  return HAWK_OK;
}

void hawk_effects_free(hawk_effects* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  fx_release(f);
}

int hawk_effects_rank(hawk_effects* f, int family, const double* score, const int64_t* cand_start, const uint8_t* cand_strand,
                      uint32_t n_cand, uint32_t K, uint32_t* n_chosen, uint64_t* n_alts, hawk_effects_timing* timing) {
  if (!f || !n_chosen || !n_alts) return HAWK_E_INVALID;
  *n_chosen = 0; *n_alts = 0;
  f->ranked = false;
  if ((family != FX_SIGNED && family != FX_ABSOLUTE) || K < 1 || K > FX_MAX_K || n_cand > K || (n_cand && (!cand_start || !cand_strand)))
    return HAWK_E_INVALID;
  for (uint32_t k = 0; k < n_cand; ++k)
    if (cand_strand[k] > 1) return HAWK_E_INVALID;
  const uint64_t G = f->G;
  if (G && !score && !f->has_cfdon) return HAWK_E_INVALID;
  hawk_ctx* ctx = f->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  hipEvent_t* ev = ctx->ev;
  const uint32_t blocks = hawk_fx_topk_blocks(G);
  int rc;
  if ((rc = f->rs.reserve(G * 8 + 8)) || (rc = f->delta.reserve(G * 8 + 8)) || (rc = f->adelta.reserve(G * 8 + 8)) || (rc = f->pref.reserve(G * 4 + 4)) ||
      (rc = f->pworst.reserve(G * 8 + 8)) || (rc = f->pnv.reserve(G * 4 + 4)) || (rc = f->pfr.reserve(G * 4 + 4)) || (rc = f->cand_s.reserve(FX_MAX_K * 8)) ||
      (rc = f->cand_t.reserve(FX_MAX_K)) || (rc = f->chosen.reserve((2 * FX_MAX_K + 1) * 4)) ||
      (rc = f->part.reserve((uint64_t)blocks * FX_MAX_K * sizeof(FxEntry))) || (rc = f->alt_off.reserve((FX_MAX_K + 1) * 8)) ||
      (score && (rc = f->score.reserve(G * 8 + 8))))
    return rc;
  HIPCHK(hipEventRecord(ev[0], st));
  if (score && G) HIPCHK(hipMemcpyAsync(f->score.p, score, G * 8, hipMemcpyHostToDevice, st));
  if (n_cand) {
    HIPCHK(hipMemcpyAsync(f->cand_s.p, cand_start, (size_t)n_cand * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(f->cand_t.p, cand_strand, n_cand, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemsetAsync(f->chosen.p, 0xff, FX_MAX_K * 4, st));
  HIPCHK(hipMemsetAsync(f->chosen.as<uint32_t>() + FX_MAX_K, 0, (FX_MAX_K + 1) * 4, st));
  HIPCHK(hipMemsetAsync(f->alt_off.p, 0, (FX_MAX_K + 1) * 8, st));
  FxDev F = fx_dev(f);
  F.score = score ? f->score.as<double>() : f->cfdon.as<double>();
  F.n_cand = n_cand; F.K = K;
  HIPCHK(hipEventRecord(ev[1], st));
  hawk_launch_fx_positions(st, F, family);
  HIPCHK(hipEventRecord(ev[2], st));
  hawk_launch_fx_topk(st, F, family);
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  uint32_t back[2 * FX_MAX_K + 1];
  HIPCHK(hipMemcpyAsync(back, f->chosen.p, sizeof(back), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // which positions were chosen decides how many alternatives are listed: one 516-byte read-back
  const uint32_t nc = back[2 * FX_MAX_K];
  const uint32_t* nv = back + FX_MAX_K;
  if (nc > K) return HAWK_E_INVALID;
  uint64_t total = 0;
  for (uint32_t i = 0; i < nc; ++i) total += nv[i];
  if ((rc = f->alt_group.reserve(total * 4 + 4))) return rc;
  F.alt_group = f->alt_group.as<uint32_t>();
  HIPCHK(hipEventRecord(ev[4], st));
  hawk_launch_fx_alts(st, F, family, nc);
  HIPCHK(hipEventRecord(ev[5], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  f->ranked = true; f->n_chosen = nc; f->n_alts = total; f->K = K;
  *n_chosen = nc; *n_alts = total;
  if (timing) {
    memset(timing, 0, sizeof(*timing));
    (void)hipEventElapsedTime(&timing->upload_ms, ev[0], ev[1]);
    (void)hipEventElapsedTime(&timing->positions_ms, ev[1], ev[2]);
    (void)hipEventElapsedTime(&timing->topk_ms, ev[2], ev[3]);
    (void)hipEventElapsedTime(&timing->alts_ms, ev[4], ev[5]);
    (void)hipEventElapsedTime(&timing->total_ms, ev[0], ev[5]);
    timing->n_groups = G;
  }
  return HAWK_OK;
}

int hawk_effects_download(hawk_effects* f, const hawk_effects_out* out) {
  if (!f || !out) return HAWK_E_INVALID;
  const bool per_score = out->score || out->delta || out->abs_delta || out->pos_ref || out->pos_worst || out->pos_nvalid || out->pos_first_rank ||
                         out->chosen || out->alt_off || out->alt_group;
  if (per_score && !f->ranked) return HAWK_E_INVALID;
  hawk_ctx* ctx = f->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t G = f->G;
  auto dl = [&](void* dst, const DevBuf& src, size_t bytes) {
    return (dst && bytes) ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  HIPCHK(dl(out->score, f->rs, G * 8)); HIPCHK(dl(out->delta, f->delta, G * 8)); HIPCHK(dl(out->abs_delta, f->adelta, G * 8));
  HIPCHK(dl(out->n_samples, f->nsamp, G * 4)); HIPCHK(dl(out->type, f->type, G)); HIPCHK(dl(out->dup, f->dup, G));
  HIPCHK(dl(out->position, f->head, G * 4)); HIPCHK(dl(out->pos_ref, f->pref, G * 4)); HIPCHK(dl(out->pos_worst, f->pworst, G * 8));
  HIPCHK(dl(out->pos_nvalid, f->pnv, G * 4)); HIPCHK(dl(out->pos_first_rank, f->pfr, G * 4));
  HIPCHK(dl(out->chosen, f->chosen, (size_t)f->n_chosen * 4)); HIPCHK(dl(out->alt_off, f->alt_off, ((size_t)f->n_chosen + 1) * 8));
  HIPCHK(dl(out->alt_group, f->alt_group, f->n_alts * 4)); HIPCHK(dl(out->counts, f->counts, 64));
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}

}  // extern "C"
