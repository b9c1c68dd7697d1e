// hawk_api_cldict.hip - C ABI: the cluster dictionary of an expansion plan - its build (behind hawk_xplan_view and
// hawk_xplan_cluster_rebuild) and what it reports.  The kernels: hawk_cldict.hip; the sizes, views and status bits: hawk_cl.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "hawk_host.h"

static_assert(CL_MAX_ROWS == HAWK_ROW_MAX_HAP, "cl_build_sizes declines the rows the packed layout cannot hold");

// The zero block of a build - one allocation, one memset - seen through the layout of cl_build_sizes.
struct ClZero {
  char* base;
  const ClBuildSizes* z;
  template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
  uint32_t* status() const { return at<uint32_t>(z->z_status); }
  uint32_t* counters() const { return at<uint32_t>(z->z_counters); }
  ClResults* results() const { return at<ClResults>(z->z_results); }
  uint32_t* cnt() const { return at<uint32_t>(z->z_cnt); }
  uint32_t* lcnt() const { return at<uint32_t>(z->z_lcnt); }
  uint32_t* claim() const { return at<uint32_t>(z->z_claim); }
  unsigned long long* vdesc() const { return at<unsigned long long>(z->z_vdesc); }
  uint32_t* span2() const { return at<uint32_t>(z->z_span2); }  // of the first attempt, like the table
  ClSlot* tab() const { return at<ClSlot>(z->z_tab); }
};

// The zero block, the chunk index and the list - temporaries of the call - and the instance arrays, which the dictionary keeps (the
// instances stay in the order they are built in: (row, position)); all of it as the view the passes take.
static int dict_reserve(hawk_xplan* x, const ClBuildSizes& sz, PoolScope& tmp, ClZero* zero, ClBuild* b) {
  ClusterDictionary& cl = x->cl;
  const uint32_t n = x->n_hap;
  zero->z = &sz;
  TEMPCHK(tmp, &zero->base, sz.z_end);
  ClChunks& ch = b->ch;
  TEMPCHK(tmp, &ch.ch_off, (size_t)(n + 1) * 4);
  TEMPCHK(tmp, &ch.ch_row, (size_t)sz.ch_bound * 4);
  TEMPCHK(tmp, &ch.inst_base, (size_t)(sz.ch_bound + 1) * 4);
  TEMPCHK(tmp, &ch.list_base, (size_t)(sz.ch_bound + 1) * 4);
  TEMPCHK(tmp, &b->list.list, (size_t)sz.inst_bound * sizeof(ClListed));
  TEMPCHK(tmp, &b->list.state, (size_t)sz.inst_bound * 4);
  for (DevBuf* buf : {&cl.inst_uid, &cl.inst_o, &cl.inst_row, &cl.inst_pa, &cl.inst_rb})
    if (int rc = buf->reserve((size_t)sz.inst_bound * 4)) return rc;
  ch.ch_bound = sz.ch_bound; ch.cnt = zero->cnt(); ch.lcnt = zero->lcnt();
  b->list.bound = sz.inst_bound;
  ClPlan& p = b->plan;
  p.heads = x->heads.p; p.hv_off = x->off.as<uint64_t>(); p.hap_len = x->hlen.as<uint32_t>();
  p.ss = x->m_ss.as<int32_t>(); p.se = x->m_se.as<int32_t>(); p.is_ref = x->m_is_ref.as<uint8_t>();
  p.seg_off = x->m_seg_off.as<uint32_t>(); p.seg_rel = x->m_seg_rel.as<uint32_t>();
  p.n_rows = n; p.n_var = x->n_var;
  b->var.desc = zero->vdesc(); b->var.claim = zero->claim();
  ClInst& ci = b->inst;
  ci.o = cl.inst_o.as<int32_t>(); ci.row = cl.inst_row.as<uint32_t>(); ci.pa = cl.inst_pa.as<int32_t>(); ci.rb = cl.inst_rb.as<int32_t>();
  ci.uid = cl.inst_uid.as<uint32_t>();
  b->tally.counters = zero->counters(); b->tally.results = zero->results(); b->tally.status = zero->status();
  return HAWK_OK;
}

// chunks per row -> their offsets and rows, then the instances every chunk opens and how many of them go on the list of the
// clusters that are more than their variant - and, from a large job's first chunks, the variants they describe (the number of
// chunks is only known on the device - rows that scan nothing have none: the count pass and its scan run over the bound; chunks
// beyond the last one open nothing).  Queued once: a repeated attempt starts from these counts.
static void dict_cut(hipStream_t st, const ClBuild& b) {
  const ClChunks& ch = b.ch;
  hawk_launch_cl_chunks(st, b);
  hawk_launch_cl_count(st, b);
  if (hawk_cl_head_chunks(ch.ch_bound))  // (beside the scan, in its launch: the bitmap of the variants the first chunks described)
    hawk_launch_scan2_u32(st, ch.cnt, ch.lcnt, ch.ch_bound, ch.inst_base, ch.list_base, b.var.desc, b.var.claim, b.plan.n_var);
  else
    hawk_launch_scan2_u32(st, ch.cnt, ch.lcnt, ch.ch_bound, ch.inst_base, ch.list_base);
}

// One attempt = cut the rows (a one-record shareable instance is its variant; the rest goes on the list), the listed instances through
// the table, the distinct clusters' descriptions, the listed instances that share a cluster - queued without a read-back in
// between.  The host reads the result block once, at the end, into page-locked memory.
static int dict_attempt(hawk_xplan* x, const ClBuild& b, const ClTable& t, uint32_t* span2, ClResults* res) {
  ClusterDictionary& cl = x->cl;
  hawk_ctx* ctx = x->ctx;
  hipStream_t st = ctx->stream;
  for (DevBuf* buf : {&cl.u_rec, &cl.u_n, &cl.u_row, &cl.u_o, &cl.u_seg})
    if (int rc = buf->reserve((size_t)t.u_cap * 4)) return rc;
  ClUniq cu;
  cu.rec = cl.u_rec.as<uint32_t>(); cu.n = cl.u_n.as<uint32_t>(); cu.row = cl.u_row.as<uint32_t>(); cu.o = cl.u_o.as<int32_t>();
  cu.seg = cl.u_seg.as<uint32_t>(); cu.span2 = span2;
  hawk_launch_cl_fill(st, b);
  hawk_launch_cl_finish(st, b, t, cu);
  HIPCHK(hipMemcpyAsync(res, b.tally.results, sizeof(ClResults), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return HAWK_OK;
}

// What the dictionary keeps of the last attempt's results, and whether a search should use it: worth it when clusters are shared
// (the template rows are extra traffic otherwise) and the templates fit a sane budget (HAWK_CLUSTER_MAX_SLOTS template rows, default
// 2^27 = 10 GB; HAWK_CLUSTER_MIN_SHARE instances per distinct cluster, default 3: read per call so that tests can send small panels
// down this path)
static void dict_decide(ClusterDictionary& cl, const ClResults& res, uint32_t n_var, uint32_t u_bound) {
  cl.n_inst = (uint32_t)res.instances;
  cl.n_uniq = std::min<uint32_t>(n_var + (uint32_t)res.table_clusters, u_bound);  // the range of the numbers
  cl.n_real = (uint32_t)(res.table_clusters + res.variant_clusters);
  cl.last_uniq = (uint32_t)res.table_clusters;
  cl.slots = cl.n_uniq ? res.template_rows : 0;
  cl.status = (uint32_t)res.status;
  const char* e1 = getenv("HAWK_CLUSTER_MAX_SLOTS");
  const char* e2 = getenv("HAWK_CLUSTER_MIN_SHARE");
  const uint64_t max_slots = e1 ? strtoull(e1, nullptr, 10) : (1ull << 27);
  const double min_share = e2 ? atof(e2) : 3.0;
  if (!cl.status && (cl.slots > max_slots || (double)cl.n_inst < min_share * (double)std::max<uint32_t>(cl.n_real, 1))) cl.status = CL_ST_DECLINED;
  cl.usable = cl.status == 0;
}

// The cluster dictionary of a plan: which rows carry which distinct variant cluster.  Built once per plan, from the records and the
// rows' scan bounds; a search of a view then does the per-window work once per distinct cluster.  Not usable (the per-word search of
// hawk_vsearch.hip takes the plan instead) when a chain of variants is longer than the builder accepts, when two different clusters
// share a hash, or when sharing is too thin to pay for the template rows.
int xplan_build_dict(hawk_xplan* x) {
  ClusterDictionary& cl = x->cl;
  if (cl.built) return HAWK_OK;
  cl.built = true; cl.usable = false; cl.status = 0; cl.n_inst = cl.n_uniq = cl.n_real = 0; cl.slots = 0; cl.build_ms = 0.f;
  hawk_ctx* ctx = x->ctx;
  hipStream_t st = ctx->stream;
  const ClBuildSizes sz = cl_build_sizes(x->ncar, x->n_hap, x->n_var, cl.last_uniq);
  if (sz.declined) { cl.status = CL_ST_DECLINED; return HAWK_OK; }
  PoolScope tmp;
  ClZero zero;
  ClBuild b = {};
  int rc;
  if ((rc = dict_reserve(x, sz, tmp, &zero, &b))) return rc;
  HIPCHK(hipMemsetAsync(zero.base, 0, sz.z_end, st));
  dict_cut(st, b);
  ClResults* const res = &static_cast<PinnedBlock*>(ctx->pinned)->dict;
  *res = ClResults{};
  ClTable t;
  t.tab = zero.tab(); t.mask = sz.tsmall - 1; t.max_probe = sz.max_probe; t.fail_bit = sz.fail_bit; t.u_cap = sz.u_bound;
  if ((rc = dict_attempt(x, b, t, zero.span2(), res))) return rc;
  // build_ms: from where k_cl_chunks began to where k_cl_results ended, by the device's wall clock (the result block carries both
  // stamps) - the build's kernels, without the memset in front of them and the copy behind.  No event is recorded.  A repeated
  // attempt clears the block on the device and does not cut the rows again: the first attempt's begin is kept here.
  const unsigned long long build_begin = res->begin;
  if (res->status & CL_ST_FIRST_TABLE) {  // the small table filled up: once more with two slots per instance
    // The repeat: its own, larger table and bounds, the counters cleared again.  The variants' bitmap and describers stay: the counting
    // pass and the scan, which are not repeated, left the first rows' there, and who describes a variant does not depend on the table
    const uint32_t status = (uint32_t)res->status & ~(uint32_t)CL_ST_FIRST_TABLE;
    HIPCHK(hipMemcpyAsync(zero.status(), &status, 4, hipMemcpyHostToDevice, st));
    uint32_t* d_span2;
    t.mask = sz.tsize - 1; t.max_probe = 0xffffffffu; t.fail_bit = CL_ST_COLLISION; t.u_cap = sz.u_bound_repeat;
    TEMPCHK(tmp, &d_span2, (size_t)t.u_cap * 4);
    TEMPCHK(tmp, &t.tab, (size_t)sz.tsize * sizeof(ClSlot));
    HIPCHK(hipMemsetAsync(t.tab, 0, (size_t)sz.tsize * sizeof(ClSlot), st));
    HIPCHK(hipMemsetAsync(d_span2, 0, (size_t)t.u_cap * 4, st));
    HIPCHK(hipMemsetAsync(zero.counters(), 0, sz.z_cnt - sz.z_counters, st));  // counters, results
    if ((rc = dict_attempt(x, b, t, d_span2, res))) return rc;
  }
  if (res->instances == 0) { cl.status = CL_ST_DECLINED; return HAWK_OK; }
  if ((uint32_t)res->instances > sz.inst_bound) { snprintf(hawk_hip_err_buf(), 256, "hawk_xplan_view: instance count beyond its bound"); return HAWK_E_HIP; }
  cl.build_ms = hawk_stamp_ms(ctx, build_begin, res->end);
  dict_decide(cl, *res, x->n_var, t.u_cap);
  return HAWK_OK;
}

extern "C" {

int hawk_xplan_cluster_stats(const hawk_xplan* x, uint32_t* usable, uint32_t* n_instances, uint32_t* n_distinct, uint64_t* template_slots,
                             float* build_ms, uint32_t* status) {
  if (!x) return HAWK_E_INVALID;
  if (usable) *usable = x->cl.built && x->cl.usable ? 1u : 0u;
  if (n_instances) *n_instances = x->cl.n_inst;
  if (n_distinct) *n_distinct = x->cl.n_real;
  if (template_slots) *template_slots = x->cl.slots;
  if (build_ms) *build_ms = x->cl.build_ms;
  if (status) *status = x->cl.built ? x->cl.status : 0xffffffffu;
  return HAWK_OK;
}

int hawk_xplan_cluster_rebuild(hawk_xplan* x) {
  if (!x || !x->has_meta || x->ref_index != 0) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(x->ctx->device));
  x->cl.built = false;
  return xplan_build_dict(x);
}

}  // extern "C"
