// hawk_api_collapse.hip - C ABI: which rows the guide report merges (hawk_table_collapse*) and the group export
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hawk_host.h"

extern "C" {

// HAWK_COLLAPSE_EXACT=1 groups on the full keys from the start, HAWK_COLLAPSE_MODE=sort / hash overrides the choice between the
// sort and the hash table; read once per call.
struct CollapsePolicy {
  bool exact, force_hash, force_sort;
  bool verify, weak;  // the product library can neither skip the verification nor weaken the hash
  static CollapsePolicy read() {
    const char *ex = getenv("HAWK_COLLAPSE_EXACT"), *md = getenv("HAWK_COLLAPSE_MODE");
    CollapsePolicy p = {ex && ex[0] == '1', md && md[0] == 'h', md && md[0] == 's', true, false};
#ifdef HAWK_TEST_HOOKS  // libhawk_hip_hooks.so only (tests/hooks_collapse_check.py): a 4-bit hash so that the verify pass HAS collisions
    const char* vf = getenv("HAWK_COLLAPSE_VERIFY");  // to catch, and a way to look at the grouping without it
    const char* wk = getenv("HAWK_COLLAPSE_WEAK_HASH");
    p.verify = !(vf && vf[0] == '0');
    p.weak = wk && wk[0] == '1';
#endif
    return p;
  }
};

// one collapse of the rows of a table: what every path of it is handed
struct CollapseJob {
  hawk_table* t; CollapseKey key; CollapsePolicy pol;
  unsigned begin_bit, end_bit;  // the sort key's bits in use
  size_t temp_bytes;            // rocprim's temporary storage for the sort path
  uint64_t* n_groups; float* kernel_ms;
};
enum CollapseNext { COLLAPSE_DONE, COLLAPSE_TO_SORT, COLLAPSE_TO_EXACT };

static uint64_t seed_of(int attempt) { return 0x9e3779b97f4a7c15ull * (uint64_t)(attempt + 1); }

// the interval between events ev[first] and ev[first + 1], both recorded and waited for, onto *kernel_ms
static void add_interval(hawk_ctx* ctx, int first, float* kernel_ms) {
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev[first], ctx->ev[first + 1]);
  if (kernel_ms) *kernel_ms += ms;
}

// The end of every path: group_off's closing entry and the wait for it, then what the call leaves behind.  `refuted` (hash-table
// path): the verification's counter comes back in the same wait, and a grouping it refutes leaves nothing behind.
static int finish(hawk_table* t, uint64_t ng, uint64_t* n_groups, bool* refuted = nullptr) {
  hawk_hapset* hs = t->hs;
  hipStream_t st = hs->ctx->stream;
  const uint64_t n = t->n_rows;
  unsigned long long mismatches = 0;
  HIPCHK(hipMemcpyAsync(hs->cws.group_off() + ng, &n, 8, hipMemcpyHostToDevice, st));
  if (refuted) HIPCHK(hipMemcpyAsync(&mismatches, hs->cws.counters() + 3, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (refuted && (*refuted = mismatches != 0)) return HAWK_OK;
  hs->cws.gen = t->gen;
  hs->cws.last_groups = ng;
  if (hs->plan_groups) *hs->plan_groups = ng;
  t->n_groups = ng; t->collapsed = true;
  *n_groups = ng;
  return HAWK_OK;
}

// Slots of the hash table to group through, 0 for the sort: the table when groups are expected to be far fewer than rows - the
// sort then only orders (group number, row).
static uint64_t table_slots(const hawk_hapset* hs, uint64_t n, const CollapsePolicy& pol) {
  const uint64_t last = hs->cws.last_groups;
  const uint64_t g_est = last ? last + last / 4 : n / 16;
  uint64_t C = 1024;
  while (C < 2 * g_est) C <<= 1;  // at most half full (with the 25 % head room of g_est)
  const bool fits = C <= (1ull << 26) && hs->max_gen - hs->min_gen < 0xffffffffll;
  const bool want = !pol.weak && !pol.force_sort && fits && (pol.force_hash || (n >= (1u << 20) && (last == 0 || last * 8 <= n)));
  return want ? C : 0;
}

// Grouping through a hash table of C slots (hawk_collapse.hip).  A table that turns out too small, or an unlucky seed twice, falls
// through to the sort.
static int group_by_table(const CollapseJob& j, uint64_t C, CollapseNext* next) {
  hawk_hapset* hs = j.t->hs;
  hawk_ctx* ctx = hs->ctx;
  CollapseWs& ws = hs->cws;
  const uint64_t n = j.key.n;
  const size_t tb = hawk_collapse_hash_temp_bytes(n, (uint32_t)C);
  int rc;
  if ((rc = ws.reserve_table(C, std::max(tb, j.temp_bytes)))) return rc;
  CollapseHashView v = ws.hash_view(tb, n, C);
  *next = COLLAPSE_TO_SORT;
  for (int attempt = 0; attempt < 2; ++attempt) {
    unsigned long long hc[3] = {0, 0, 0};
    HIPCHK(hipMemsetAsync(ws.cnt.p, 0, 32, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (hawk_launch_collapse_hash1(ctx->stream, j.key, v, seed_of(attempt))) return HAWK_E_HIP;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hc, ws.cnt.p, 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (hc[1]) {  // no room: sort now, a larger table (or the sort) next time
      ws.last_groups = n;
      if (hs->plan_groups) *hs->plan_groups = n;
      return HAWK_OK;
    }
    if (hc[0]) continue;  // two identities under one key: another seed
    const uint64_t ng = hc[2];
    if (hawk_launch_collapse_hash2(ctx->stream, j.key, v, (uint32_t)ng, j.end_bit)) return HAWK_E_HIP;
    if (j.pol.verify) {
      if ((rc = ws.full.reserve(ng * 64 + 64))) return rc;
      v.full = ws.full.p;
      hawk_launch_collapse_verify_rows(ctx->stream, j.key, v, (uint32_t)ng);
    }
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipGetLastError());
    bool refuted = false;
    if ((rc = finish(j.t, ng, j.n_groups, &refuted))) return rc;
    add_interval(ctx, 0, j.kernel_ms);
    *next = refuted ? COLLAPSE_TO_EXACT : COLLAPSE_DONE;  // two different rows under one group: the exact path decides
    return HAWK_OK;
  }
  return HAWK_OK;
}

// Grouping by a sort of all rows on (start, strand, hash bits); `exact`: on all 31 hash bits, identities compared on the full keys.
static int group_by_sort(const CollapseJob& j, bool exact, CollapseNext* next) {
  hawk_hapset* hs = j.t->hs;
  hawk_ctx* ctx = hs->ctx;
  CollapseWs& ws = hs->cws;
  const uint64_t n = j.key.n;
  int rc;
  if (exact && (rc = ws.full.reserve(hawk_collapse_full_bytes(n)))) return rc;
  const CollapseSortView v = ws.sort_view(j.temp_bytes, n);
  unsigned long long cnt[3] = {0, 0, 0};
  // A new seed whenever two different rows of one (start, strand) collide: in the hash bits of the key (24 to 31) on the usual
  // path, which needs them apart to keep equal rows contiguous - thousands of different rows under one start (k of them collide
  // with probability ~ k^2 / 2^(bits + 1) per seed) can use up all four seeds, and the call goes to the exact path; there only in
  // all 63 hash bits, because its rows are sorted by identity below the key (hawk_launch_collapse).
  for (int attempt = 0; attempt < 4; ++attempt) {
    HIPCHK(hipMemsetAsync(ws.cnt.p, 0, 32, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (hawk_launch_collapse(ctx->stream, j.key, v, exact ? 0u : j.begin_bit, j.end_bit, seed_of(attempt), exact, j.pol.weak && !exact))
      return HAWK_E_HIP;
    if (j.pol.verify && !exact) hawk_launch_collapse_verify(ctx->stream, j.key, v);
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cnt, ws.cnt.p, 24, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    add_interval(ctx, 0, j.kernel_ms);
    if (cnt[0] == cnt[1]) break;
  }
  // every seed used up, or the verify pass found a group holding two different rows: once more, exactly
  if (cnt[0] != cnt[1] || cnt[2]) { *next = COLLAPSE_TO_EXACT; return exact ? HAWK_E_UNSUPPORTED : HAWK_OK; }
  *next = COLLAPSE_DONE;
  return finish(j.t, cnt[1], j.n_groups);
}

static int collapse_rows(hawk_table* t, uint32_t flank_up, uint32_t flank_down, uint64_t* n_groups, float* kernel_ms) {
  hawk_hapset* hs = t->hs;
  HIPCHK(hipSetDevice(hs->ctx->device));
  const uint64_t n = t->n_rows;
  t->collapsed = false;
  *n_groups = 0;
  if (kernel_ms) *kernel_ms = 0.f;
  if (n == 0) { hs->cws.gen = t->gen; t->n_groups = 0; t->collapsed = true; return HAWK_OK; }
  if (n > 0xffffffffull || hs->max_gen - hs->min_gen > 0xffffffffll) return HAWK_E_UNSUPPORTED;
  CollapseJob j = {t, {t->cols, hs->d_is_ref, n, (int)t->guidelen, (int)t->pamlen, (int)t->right, (int)flank_up, (int)flank_down, hs->min_gen},
                   CollapsePolicy::read(), 0, 32, 0, n_groups, kernel_ms};
  while (j.end_bit < 64 && ((uint64_t)(hs->max_gen - hs->min_gen) >> (j.end_bit - 32)) != 0) ++j.end_bit;
  // low hash bits the sort leaves out: start bits + strand + hash fill whole 8-bit passes, at least 24 hash bits stay
  const unsigned pos_bits = j.end_bit - 31;  // start - base, strand
  const unsigned hash_bits = std::min(31u, (pos_bits + 24 + 7) / 8 * 8 - pos_bits);
  j.begin_bit = 31 - hash_bits;
  j.temp_bytes = hawk_collapse_temp_bytes(n, j.begin_bit, j.end_bit);
  int rc;
  if ((rc = hs->cws.reserve_rows(n, j.temp_bytes))) return rc;
  // Rows are grouped on (start, strand, 63 hash bits of the rest) and the grouping is then VERIFIED: every member against
  // its group's first member on the full key (k_collapse_verify).  A mismatch - two different rows under one hash, never
  // seen - sends the call through the exact path (full 64-byte keys compared neighbour by neighbour), which
  // HAWK_COLLAPSE_EXACT=1 forces from the start.  The verification cannot be switched off in the product library.
  CollapseNext next = j.pol.exact ? COLLAPSE_TO_EXACT : COLLAPSE_TO_SORT;
  const uint64_t C = j.pol.exact ? 0 : table_slots(hs, n, j.pol);
  if (C && (rc = group_by_table(j, C, &next))) return rc;
  if (next == COLLAPSE_TO_SORT && (rc = group_by_sort(j, false, &next))) return rc;
  if (next == COLLAPSE_TO_EXACT && (rc = group_by_sort(j, true, &next))) return rc;
  return next == COLLAPSE_DONE ? HAWK_OK : HAWK_E_UNSUPPORTED;
}

// The collapse of a table the cluster search wrote.  Every non-REF row is a copy of one of the search's template rows in all the
// grouping compares (start, stop, strand, origin, windows), so the grouping - hashing, sorting, the exact verification - runs on
// REF's rows + the template rows (C3: 2.8 x 10^5 instead of 2.8 x 10^7; a C4 tile 10^6 instead of 10^8), and the table's rows
// only inherit their template row's group number before the one sort that orders them by (group, row).  Same groups, same
// order, same members as collapse_rows on the table itself (tests/test_gpu_vsearch.py, tools/stress_views.py).
static int collapse_by_templates(hawk_table* t, uint32_t flank_up, uint32_t flank_down, uint64_t* n_groups, float* kernel_ms) {
  hawk_hapset* hs = t->hs;
  hawk_ctx* ctx = hs->ctx;
  CollapseWs& ws = hs->cws;
  HIPCHK(hipSetDevice(ctx->device));
  const hawk_xplan* vx = hs->vplan;
  if (!vx || !vx->cl.usable) return HAWK_E_INVALID;
  const uint64_t n = t->n_rows;
  if (n > 0xffffffffull) return HAWK_E_UNSUPPORTED;
  t->collapsed = false;
  *n_groups = 0;
  if (kernel_ms) *kernel_ms = 0.f;
  // the template rows of the search: every distinct cluster's rows [tbase[u], tbase[u] + n0 + n1) of the template array (its
  // reservation may be longer: kept window starts that turned out to repeat REF); numbered densely here
  const uint32_t nu = vx->cl.n_uniq;
  PoolScope tmp;
  uint32_t* d_ucnt;
  uint64_t* d_moff;
  unsigned long long *d_partial, *d_shards;
  ScanTotals* d_tot;
  TEMPCHK(tmp, &d_ucnt, (size_t)std::max<uint32_t>(nu, 1) * 4);
  TEMPCHK(tmp, &d_moff, ((size_t)nu + 2) * 8);
  TEMPCHK(tmp, &d_partial, ((size_t)nu / 1024 + 2) * 8);
  TEMPCHK(tmp, &d_shards, 512 * 8);
  TEMPCHK(tmp, &d_tot, sizeof(ScanTotals));
  HIPCHK(hipMemsetAsync(d_shards, 0, 512 * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(d_tot, 0, sizeof(ScanTotals), ctx->stream));
  uint64_t r0 = 0;  // REF's rows come first: as many as the first cluster instance's offset says
  ScanTotals tot;
  memset(&tot, 0, sizeof(tot));
  if (nu) {
    hawk_launch_cc_ucnt(ctx->stream, hs->cs_res.p, nu, d_ucnt);
    hawk_launch_mscan(ctx->stream, d_ucnt, nu, d_partial, d_shards, d_moff, d_tot);
    HIPCHK(hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(&r0, hs->offsets.as<uint64_t>() + t->plane_tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipGetLastError());
  const uint64_t t_live = tot.n_keep;
  const uint64_t nm = r0 + t_live;
  if (r0 > n || nm == 0 || nm > 0xffffffffull) return HAWK_E_INVALID;
  int rc;
  GuideCols mini;
  if ((rc = hawk_reserve_cols(ws.mini, nm, &mini)) || (rc = ws.m_gid.reserve(nm * 4))) return rc;
  HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
  hawk_launch_cc_mini(ctx->stream, t->cols, r0, hs->cs_trows.p, t_live, d_moff, hs->cs_tbase.as<uint32_t>(), nu, hs->ref_startp, mini);
  HIPCHK(hipEventRecord(ctx->ev[9], ctx->stream));
  HIPCHK(hipGetLastError());
  // everything the rest of this call needs in the set's collapse workspace is reserved HERE, for the full table, before the
  // mini collapse fills it: a reservation after k_cc_gidm has been queued could hand the buffers it reads back to the pool.
  // (keys: the mini table's 64-bit sort keys, then the table's (group number, row) ping-pong; group_off: G <= nm groups)
  const size_t tb = hawk_collapse_expand_temp_bytes(n);
  if ((rc = ws.keys.reserve(std::max<size_t>(2 * nm * 8, 2 * n * 4))) || (rc = ws.vals.reserve(2 * n * 4)) || (rc = ws.goff.reserve((nm + 1) * 8)) ||
      (rc = ws.gc.reserve(2 * n)) || (rc = ws.temp.reserve(tb + 16)) || (rc = ws.flags.reserve(n * 4)))
    return rc;
  hawk_table tm;  // the mini table borrows the set's collapse workspace like any table of the set
  tm.hs = hs; tm.ctx = ctx; tm.n_rows = nm; tm.n_cand = tm.n_hits = 0; tm.cap = mini.cap; tm.cols = mini;
  tm.guidelen = t->guidelen; tm.pamlen = t->pamlen; tm.right = t->right; tm.n_groups = 0; tm.collapsed = false; tm.gen = t->gen;
  uint64_t G = 0;
  if ((rc = collapse_rows(&tm, flank_up, flank_down, &G, kernel_ms))) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  add_interval(ctx, 8, kernel_ms);
  // every mini row's group number, then every table row's; the table's rows sorted by (group, row)
  HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
  hawk_launch_cc_gidm(ctx->stream, ws.perm(nm), ws.group_off(), nm, G, ws.m_gid.as<uint32_t>());
  const ClDict cd = vx->cl.view();
  const CollapseKey key = {t->cols, hs->d_is_ref, n, (int)t->guidelen, (int)t->pamlen, (int)t->right, (int)flank_up, (int)flank_down, hs->min_gen};
  const CollapseHashView v = ws.hash_view(tb, n, 0);  // no table: the rows' group numbers come from their template rows
  hawk_launch_cs_gid(ctx->stream, cd, hs->cs_res.p, d_moff, hs->offsets.as<uint64_t>() + t->plane_tiles, r0, n, ws.m_gid.as<uint32_t>(), v.gid, v.vals);
  if (hawk_launch_collapse_expand(ctx->stream, key, v, G)) return HAWK_E_HIP;
  HIPCHK(hipEventRecord(ctx->ev[9], ctx->stream));
  HIPCHK(hipGetLastError());
  if ((rc = finish(t, G, n_groups))) return rc;
  add_interval(ctx, 8, kernel_ms);
  return HAWK_OK;
}

int hawk_table_collapse_ex(hawk_table* t, uint32_t flank_up, uint32_t flank_down, uint64_t* n_groups, float* kernel_ms) {
  if (!t || !n_groups || !t->hs || hawk_table_stale(t)) return HAWK_E_INVALID;
  if (flank_up > HAWK_PAD || flank_down > HAWK_PAD) return HAWK_E_UNSUPPORTED;
  // A table the cluster search wrote is grouped on its template rows
  if (t->by_cluster && t->n_rows) return collapse_by_templates(t, flank_up, flank_down, n_groups, kernel_ms);
  return collapse_rows(t, flank_up, flank_down, n_groups, kernel_ms);
}
int hawk_table_collapse(hawk_table* t, uint64_t* n_groups, float* kernel_ms) {
  return hawk_table_collapse_ex(t, 0, 0, n_groups, kernel_ms);
}

int hawk_table_collapse_download(hawk_table* t, uint32_t* perm, uint64_t* group_off, uint8_t* gc_num, uint8_t* gc_den) {
  if (!collapse_valid(t)) return HAWK_E_INVALID;
  const CollapseWs& ws = t->hs->cws;
  hawk_ctx* ctx = t->hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t n = t->n_rows, ng = t->n_groups;
  if (n == 0) { if (group_off) group_off[0] = 0; return HAWK_OK; }
  if (perm) HIPCHK(hipMemcpyAsync(perm, ws.perm(n), n * 4, hipMemcpyDefault, ctx->stream));
  if (group_off) HIPCHK(hipMemcpyAsync(group_off, ws.group_off(), (ng + 1) * 8, hipMemcpyDefault, ctx->stream));
  if (gc_num) HIPCHK(hipMemcpyAsync(gc_num, ws.gc_num(), ng, hipMemcpyDefault, ctx->stream));
  if (gc_den) HIPCHK(hipMemcpyAsync(gc_den, ws.gc_den(n), ng, hipMemcpyDefault, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return HAWK_OK;
}

int hawk_table_collapse_export(hawk_table* t, uint32_t* rep_row, uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* stop,
                               uint8_t* flags, double* cfdon, uint64_t* win, uint32_t* member_hap, float* kernel_ms) {
  if (!collapse_valid(t)) return HAWK_E_INVALID;
  hawk_hapset* hs = t->hs;
  hawk_ctx* ctx = hs->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t n = t->n_rows, ng = t->n_groups;
  if (kernel_ms) *kernel_ms = 0.f;
  if (n == 0) return HAWK_OK;
  GuideCols rep;
  int rc = hawk_reserve_cols(hs->cws.rep, ng, &rep);
  if (rc) return rc;
  uint32_t* d_mem = hs->cws.members();
  HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
  hawk_launch_collapse_export(ctx->stream, t->cols, n, ng, hs->cws.perm(n), hs->cws.group_off(), rep, d_mem);
  HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
  HIPCHK(hipGetLastError());
  hipStream_t st = ctx->stream;
  if (rep_row) HIPCHK(hipMemcpyAsync(rep_row, rep.hap, ng * 4, hipMemcpyDefault, st));
  if (pos) HIPCHK(hipMemcpyAsync(pos, rep.pos, ng * 4, hipMemcpyDefault, st));
  if (strand) HIPCHK(hipMemcpyAsync(strand, rep.strand, ng, hipMemcpyDefault, st));
  if (start) HIPCHK(hipMemcpyAsync(start, rep.start, ng * 8, hipMemcpyDefault, st));
  if (stop) HIPCHK(hipMemcpyAsync(stop, rep.stop, ng * 8, hipMemcpyDefault, st));
  if (flags) HIPCHK(hipMemcpyAsync(flags, rep.flags, ng, hipMemcpyDefault, st));
  if (cfdon) HIPCHK(hipMemcpyAsync(cfdon, rep.cfdon, ng * 8, hipMemcpyDefault, st));
  if (win)
    for (int p = 0; p < HAWK_PLANES; ++p)
      HIPCHK(hipMemcpyAsync(win + (size_t)p * ng, rep.win + (size_t)p * rep.cap, ng * 8, hipMemcpyDefault, st));
  if (member_hap) HIPCHK(hipMemcpyAsync(member_hap, d_mem, n * 4, hipMemcpyDefault, st));
  HIPCHK(hipStreamSynchronize(st));
  add_interval(ctx, 0, kernel_ms);
  return HAWK_OK;
}

}  // extern "C"
