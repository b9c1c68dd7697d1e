// hawk_host.h — host-side objects behind the opaque handles of include/hawk.h, shared by the C-ABI
// translation units (hawk_api.hip, hawk_comm.hip).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/hawk.h"
#include "hawk_device.h"

#define HAWK_MAX_DEVICES 16
char* hawk_hip_err_buf();  // thread-local text of the last HIP failure (hawk_last_hip_error)

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      snprintf(hawk_hip_err_buf(), 256, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return HAWK_E_HIP;                                                                     \
    }                                                                                        \
  } while (0)

#define HAWK_EV_TIMED 10  // slots [0, HAWK_EV_TIMED) of hawk_ctx::ev carry timestamps; the slots behind them only order two streams
                          // (hawk_search, which times itself by stamps: hawk_stamp_ms below)
struct hawk_ctx {
  int device;
  hipStream_t stream;
  // A cluster search runs REF's plane passes here, beside the cluster passes on `stream` (hawk_api_search.hip).  Whatever a call
  // queues on it is joined into `stream` - or waited for - before the call returns: to every other call the context has one stream.
  hipStream_t side = nullptr;
  // Scratch of the call that is running: every C-ABI call records the events it times with and reads them before it returns.
  // No call may read an event another call recorded (two calls use the same slots for different intervals).
  hipEvent_t ev[14];
  void* pinned = nullptr;  // page-locked host memory: a PinnedBlock (below)
  int wall_clock_khz = 0;  // rate of the device's wall clock (hipDeviceAttributeWallClockRate): what a stamp counts in
};
// Milliseconds between two stamps (hawk_stamp, hawk_device.h).  A stamp nobody wrote is still the 0 its block was cleared to, and
// an interval with such an end - or with its ends out of order - is 0, never a huge or a negative number.
inline float hawk_stamp_ms(const hawk_ctx* ctx, unsigned long long begin, unsigned long long end) {
  if (!begin || !end || end < begin || ctx->wall_clock_khz <= 0) return 0.f;
  return (float)((double)(end - begin) / (double)ctx->wall_clock_khz);
}

// What hs->misc holds while hawk_search runs.  The host and the kernels' launchers share the status block; the host reads it back
// whole, with the stamp block behind it (192 bytes, one copy into hawk_ctx::pinned).  The offsets are what the device side has always
// been handed.
struct SearchStatusBlock {
  int status;                        // the FIRST status a kernel raised (0: none)
  int pad0;
  unsigned long long template_rows;  // template rows a cluster search handed out (hawk_csearch.hip)
  uint32_t big_count;                // entries of the emit pass's work list
  uint32_t pad1[3];
  ScanTotals totals;
};
#define HAWK_SEARCH_STAMPS 16  // slots of the stamp block (SearchStamp, hawk_api_search.hip): the wall clock at the stage boundaries
struct SearchMisc {
  unsigned long long shards[256][2];  // candidate / hit partial sums
  SearchStatusBlock blk;
  unsigned long long stamps[HAWK_SEARCH_STAMPS];  // cleared with the rest, written by hawk_stamp, read back behind the status block
};
static_assert(sizeof(SearchStatusBlock) == 64 && sizeof(SearchMisc) == 4096 + 64 + 8 * HAWK_SEARCH_STAMPS, "status block layout");
static_assert(offsetof(SearchMisc, shards) == 0 && offsetof(SearchMisc, blk) == 4096 && offsetof(SearchMisc, stamps) == 4096 + 64, "status block layout");
static_assert(offsetof(SearchStatusBlock, status) == 0 && offsetof(SearchStatusBlock, template_rows) == 8 &&
              offsetof(SearchStatusBlock, big_count) == 16 && offsetof(SearchStatusBlock, totals) == 32, "status block layout");
// hawk_ctx::pinned: what the two read-backs that go through page-locked memory land in (a copy into pageable memory is staged)
struct PinnedBlock {
  SearchStatusBlock search;                       // [0, 64) hawk_search ...
  unsigned long long stamps[HAWK_SEARCH_STAMPS];  // [64, 192) ... and its stamps: the same copy (SearchMisc::blk, ::stamps)
  char gap0[64];
  ClResults dict;                                 // [256, 320) the build of the cluster dictionary
  char gap1[64];
};
static_assert(offsetof(PinnedBlock, search) == 0 && offsetof(PinnedBlock, stamps) == sizeof(SearchStatusBlock) && offsetof(PinnedBlock, dict) == 256 &&
              sizeof(PinnedBlock) == 384, "page-locked block layout");
static_assert(offsetof(PinnedBlock, stamps) - offsetof(PinnedBlock, search) == offsetof(SearchMisc, stamps) - offsetof(SearchMisc, blk),
              "the status block and the stamps cross in one copy");

// Caching device allocator, one per device: a freed block goes to a free list and is handed to the next request of a
// similar size, so a per-tile loop (expand -> search -> collapse, tile after tile) allocates its planes, columns and
// workspaces once.  Everything in this library runs on one stream per context, so stream order makes the reuse safe.
int hawk_pool_alloc(void** p, size_t bytes);   // HAWK_OK / HAWK_E_HIP (after releasing the cache and retrying once)
void hawk_pool_free(void* p);
void hawk_pool_trim();                          // hipFree every cached block of the current device
#define POOLCHK(ptr, bytes)                                                      \
  do {                                                                           \
    int rc_ = hawk_pool_alloc(reinterpret_cast<void**>(ptr), (bytes));           \
    if (rc_) return rc_;                                                         \
  } while (0)

// Temporaries of one C-ABI call: whatever TEMPCHK allocated goes back to the pool when the call returns, on the error paths
// too (the frees used to sit at the end of the success path only).  Blocks return to the pool, not to hipFree: work still
// queued on the context's stream keeps them valid, and the next user is on the same stream.
struct PoolScope {
  std::vector<void*> held;
  ~PoolScope() { for (void* q : held) hawk_pool_free(q); }
  int alloc(void** out, size_t bytes) {
    int rc = hawk_pool_alloc(out, bytes);
    if (!rc) held.push_back(*out);
    return rc;
  }
};
#define TEMPCHK(scope, ptr, bytes)                                               \
  do {                                                                           \
    int rc_ = (scope).alloc(reinterpret_cast<void**>(ptr), (bytes));             \
    if (rc_) return rc_;                                                         \
  } while (0)

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t need) {
    if (need <= bytes) return HAWK_OK;
    if (p) { hawk_pool_free(p); p = nullptr; bytes = 0; }
    size_t want = need + need / 8 + 256;
    int rc = hawk_pool_alloc(&p, want);
    if (rc) return rc;
    bytes = want;
    return HAWK_OK;
  }
  void release() { if (p) hawk_pool_free(p); p = nullptr; bytes = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The collapse workspace of a set (hawk_api_collapse.hip): the buffers, and in the accessors the roles they take in turn - every
// `+ n` and every shared storage of the stage is stated here.  The results stay valid for the table that was collapsed last.
struct CollapseWs {
  DevBuf keys, vals, flags, gidx, temp, goff, gc, cnt, full;  // the sort path and the result
  DevBuf table, occ, dense, gkey, gslot;                       // the hash-table path
  DevBuf mini[8], m_gid;  // a cluster-searched table: REF's rows + the template rows as a table of their own, their group numbers
  DevBuf rep[8];          // hawk_table_collapse_export: one representative row per group
  uint64_t gen = 0;          // generation of the table whose results sit here
  uint64_t last_groups = 0;  // groups of the last collapse on this set (sizes the hash table of the next one)
  void release() {
    for (DevBuf* b : {&keys, &vals, &flags, &gidx, &temp, &goff, &gc, &cnt, &full, &table, &occ, &dense, &gkey, &gslot, &m_gid}) b->release();
    for (auto& b : mini) b.release();
    for (auto& b : rep) b.release();
  }
  // ---- the result of a collapse of n rows
  uint32_t* perm(uint64_t n) const { return vals.as<uint32_t>() + n; }  // the half of the row-id ping-pong every path's last sort writes
  uint64_t* group_off() const { return goff.as<uint64_t>(); }
  uint8_t* gc_num() const { return gc.as<uint8_t>(); }
  uint8_t* gc_den(uint64_t n) const { return gc.as<uint8_t>() + n; }  // one byte per group behind the n bytes gc_num may take
  // the export's member list: `flags` (head flags / slot_of_row), dead once the groups stand
  uint32_t* members() const { return flags.as<uint32_t>(); }
  unsigned long long* counters() const { return cnt.as<unsigned long long>(); }
  // ---- reservations; `temp_bytes` as the hawk_collapse_*temp_bytes functions give them
  static int reserve_each(std::initializer_list<std::pair<DevBuf*, size_t>> needs) {
    for (const auto& need : needs)
      if (int rc = need.first->reserve(need.second)) return rc;
    return HAWK_OK;
  }
  int reserve_rows(uint64_t n, size_t temp_bytes) {
    return reserve_each({{&keys, 2 * n * 8}, {&vals, 2 * n * 4}, {&flags, n * 4}, {&gidx, n * 4}, {&temp, temp_bytes + 16}, {&goff, (n + 1) * 8},
                         {&gc, 2 * n}, {&cnt, 32}});
  }
  int reserve_table(uint64_t C, size_t temp_bytes) {
    return reserve_each({{&table, C * 16}, {&occ, C * 4}, {&dense, C * 4}, {&gkey, 2 * C * 8}, {&gslot, 2 * C * 4}, {&temp, temp_bytes + 16}, {&cnt, 32}});
  }
  // ---- the views the launchers take (hawk_device.h)
  void fill(CollapseView* v, size_t temp_bytes, uint64_t n) const {
    v->temp = temp.p; v->temp_bytes = temp_bytes; v->vals = vals.as<uint32_t>(); v->full = full.p; v->counters = counters();
    v->group_off = group_off(); v->gc_num = gc_num(); v->gc_den = gc_den(n);
  }
  CollapseSortView sort_view(size_t temp_bytes, uint64_t n) const {
    CollapseSortView v = {};
    fill(&v, temp_bytes, n);
    v.keys = keys.as<uint64_t>(); v.head_flags = flags.as<uint32_t>();
    // id2 is written by the key pass and last read by the head pass; the scan that writes group_index comes behind both
    v.group_index = v.id2 = gidx.as<uint32_t>();
    return v;
  }
  CollapseHashView hash_view(size_t temp_bytes, uint64_t n, uint64_t C) const {
    CollapseHashView v = {};
    fill(&v, temp_bytes, n);
    v.table = table.p; v.C = (uint32_t)C; v.dense = dense.as<uint32_t>(); v.gkey = gkey.as<uint64_t>(); v.gslot = gslot.as<uint32_t>();
    v.occ = v.slot_rank = occ.as<uint32_t>();  // the occupancy flags are dead once stage 1 has packed the occupied slots
    v.slot_of_row = flags.as<uint32_t>();      // no head flags on this path
    v.gid = keys.as<uint32_t>();               // 2 n words in the 2 n 64-bit keys the sort path would hold
    return v;
  }
};

struct hawk_hapset {
  hawk_ctx* ctx;
  uint32_t n_hap, S;
  uint64_t total_len;
  std::vector<uint32_t> hap_len;
  std::vector<int32_t> scan_start, scan_stop;
  uint32_t* plane[HAWK_PLANES];
  uint32_t* d_hap_len;
  uint8_t* d_is_ref;
  int32_t *d_scan_start, *d_scan_stop;
  uint32_t *d_seg_off, *d_seg_rel;
  int64_t* d_seg_gen;
  int32_t ref_index;
  uint32_t n_ref_rows = 0;           // rows flagged REF (their tiles take one emit work-list entry per 512 survivors)
  bool has_meta;
  bool has_partner = false;          // hawk_hapset_set_ref_partner_range
  int32_t partner_start = 0, partner_stop = 0;
  uint32_t bph;            // workgroups (tiles of 1024 words) per haplotype row
  TileMeta* d_tile_meta;   // [n_hap * bph] per-tile record (haplotype scalars + first position-map segment)
  int64_t ref_startp;
  int64_t min_gen, max_gen;  // range of genomic positions the position maps reach (collapse sort key)
  uint64_t cols_cap = 0;      // rows the guide-table columns currently hold (0: never reserved)
  uint64_t cols_gen = 0;      // bumped by every hawk_search: a hawk_table of an older generation is stale
  std::vector<double> cfd_host;  // the CFD tables resident in `cfd`
  // workspace reused across searches
  DevBuf keepF, keepR, counts, offsets, totals, misc, cfd, partial, sites, hits, guides, lists;
  CollapseWs cws;             // hawk_table_collapse*
  std::shared_ptr<uint64_t> plan_groups;  // cws.last_groups shared with the expansion plan the set came from: the next run of the plan starts from it
  DevBuf otoff, otcode, otid, othit;  // hawk_offtarget_scan: bucketed guides, gathered hit sites
  DevBuf otsum;                       // hawk_offtarget_summary: counters, per-guide sums, CFD tables - sized by the guides, not the hits
  // a variant-enriched genome (hawk_genome_variants, hawk_api_otvar.hip): the four allele planes (REF one-hot | ALT) in the rows'
  // geometry, and the workspace of hawk_offtarget_variant_scan - its site records, its rows, its stamps
  bool finalized = false;     // hawk_genome_finalize has made the planes one-hot
  bool has_variants = false;
  DevBuf ovplane[4], ovsites, ovhits, ovstamp;
  DevBuf big;                 // tiles whose rows exceed the hand-over list (k_search_emit's work list)
  DevBuf refbits;             // REF's candidate-window bitmaps, one per strand (k_ref_bits)
  bool refbits_valid = false;
  uint64_t refbits_key[6] = {0, 0, 0, 0, 0, 0};
  // a VIEW of an expansion plan (hawk_xplan_view): rows and metadata of the plan's haplotypes without their planes -
  // plane[] points at the plan's REF planes (row 0 only) and hawk_search runs from the plan's records (hawk_vsearch.hip)
  const struct hawk_xplan* vplan = nullptr;
  DevBuf vcnt0;               // per tile: rows of strand 0 (k_vsearch<0> -> k_vsearch<1>)
  DevBuf refhp;               // REF's PAM hits + prefix counts per strand (k_ref_hits), keyed like refbits
  uint64_t cs_tcap = 0;       // template rows a search of this view may need (raised to the plan's bound after an overflow)
  DevBuf cs_res, cs_tbase, cs_trows, cs_inst;  // per distinct cluster 32 B {rows per strand, hits, candidates} {first template row, REF hits before / behind}, first template row; template rows; per instance 16 B {rows, first template row, haplotype row shifted, position} (k_cs_count -> k_cs_emit_rows)
  DevBuf colsA[8];
  DevBuf rowsA;               // packed rows of a cluster-searched table (colsA then stages REF's rows only)
  uint64_t rows_cap = 0;
};

// The cluster dictionary of an expansion plan, as the host keeps it (kernels: hawk_cldict.hip; build: hawk_api_cldict.hip).
struct ClusterDictionary {
  bool built = false, usable = false;
  uint32_t n_inst = 0, n_uniq = 0;  // n_uniq: the RANGE of the distinct clusters' numbers (variants first - with holes - then the table's)
  uint32_t n_real = 0;              // how many distinct clusters there are
  uint32_t last_uniq = 0;  // distinct clusters of the previous build (sizes the first hash table of the next)
  uint64_t slots = 0;     // bound on the template rows of a search: window starts x 2 strands over all distinct clusters
  uint32_t status = 0;    // why it is not usable: ClStatus bits (hawk_cl.h)
  float build_ms = 0.f;
  DevBuf inst_uid, inst_o, inst_row, inst_pa, inst_rb, u_rec, u_n, u_row, u_o, u_seg;
  void release() {
    for (DevBuf* b : {&inst_uid, &inst_o, &inst_row, &inst_pa, &inst_rb, &u_rec, &u_n, &u_row, &u_o, &u_seg}) b->release();
  }
  ClDict view() const {  // what the kernels of a search read (hawk_device.h)
    ClDict cd;
    cd.n_inst = n_inst; cd.n_uniq = n_uniq;
    cd.inst_uid = inst_uid.as<uint32_t>(); cd.inst_o = inst_o.as<int32_t>(); cd.inst_row = inst_row.as<uint32_t>();
    cd.inst_pa = inst_pa.as<int32_t>(); cd.inst_rb = inst_rb.as<int32_t>();
    cd.u_rec = u_rec.as<uint32_t>(); cd.u_n = u_n.as<uint32_t>(); cd.u_row = u_row.as<uint32_t>(); cd.u_o = u_o.as<int32_t>();
    cd.u_seg = u_seg.as<uint32_t>();
    return cd;
  }
};

// An expansion plan keeps everything an expansion needs in HBM - the variant table, the carried-variant lists, the
// per-workgroup variant ranges and (after hawk_xplan_finish_meta) the metadata of the rows it produces - so that running
// it is device work only: the per-tile loop of a whole-contig search re-expands its tiles without touching the host.
struct hawk_xplan {
  hawk_ctx* ctx;
  uint32_t n_var, n_hap, ref_len;
  uint64_t ncar;
  std::vector<uint32_t> hap_len;
  uint32_t* ref_plane[4];  // the REF region's code planes, copied: the plan does not depend on the life of ref_set
  uint32_t ref_S;
  DevBuf ref5[HAWK_PLANES];  // the same planes (+ an all-zero V plane) at the ROWS' stride S: row 0 of a view (hawk_xplan_view)
  DevBuf recs, tiles, codes, off, hlen, hash;  // 32 B per carried variant, 16 B per (row, tile): hawk_expand.hip
  DevBuf heads;                               // the records' first 16 bytes {o, rs, alt_len, alt_off} once more: what the dictionary passes stream
  // metadata of the produced rows: segments from hawk_xplan_create_gt, scan ranges and tile records from hawk_xplan_finish_meta
  bool has_meta;
  std::vector<int32_t> scan_start, scan_stop;
  DevBuf m_is_ref, m_ss, m_se, m_seg_off, m_seg_rel, m_seg_gen, m_tile;
  uint32_t nseg, bph, S;
  int32_t ref_index;
  int64_t ref_startp, min_gen, max_gen;
  bool has_partner = false;
  int32_t partner_start = 0, partner_stop = 0;
  uint32_t n_ref_rows = 0;
  std::vector<int64_t> rev0, rev1;  // hawk_xplan_create_gt: posmap_rev of every row at the two positions asked for
  std::shared_ptr<uint64_t> groups = std::make_shared<uint64_t>(0);  // groups the last collapse of a set of this plan found
  ClusterDictionary cl;  // built by the first hawk_xplan_view after the metadata is set (hawk_api_cldict.hip)
};
int xplan_build_dict(hawk_xplan* x);  // hawk_api_cldict.hip: builds x->cl unless it stands; HAWK_OK also when the result is not usable

// genotypes of a VCF block in HBM and, after hawk_gt_lists, the carried-variant lists of every chromosome copy
struct hawk_gt {
  hawk_ctx* ctx;
  uint64_t n_lines;
  uint32_t n_samples, n_var;
  uint8_t* d_codes;   // [n_lines][2 * n_samples]
  uint8_t* d_flags;   // [n_lines]
  uint64_t n_entries; // carried-variant entries over all columns (valid after hawk_gt_lists)
  uint64_t* d_col_off; uint32_t* d_idx; int32_t* d_o; int64_t* d_delta;
  uint64_t n_indel = 0;          // entries whose variant changes the length (var_chain != 0)
  uint32_t* d_indel = nullptr;   // their entry indices, ascending
  uint64_t* d_ioff = nullptr;    // [2 * n_samples + 1] where each column's carried indels start in d_indel
  std::vector<uint64_t> h_off, h_ioff;  // host copies of d_col_off / d_ioff (after hawk_gt_lists)
  std::vector<int64_t> h_delta;         // per column: sum of the length changes of its carried variants
};

// the per-sample carried SNV lists of an unphased block and the variant table they index, in HBM (hawk_api_ubuild.hip)
struct hawk_ubuild {
  hawk_ctx* ctx;
  uint32_t n_samples = 0, n_var = 0;
  uint64_t n_entries = 0;
  uint32_t max_off = 0;                 // the largest var_off: a row the lists are expanded into is longer than that
  DevBuf off, idx, var_off, var_mask, var_ref;
  std::vector<uint64_t> h_off;          // [n_samples + 1]
  UbLists view() const {
    UbLists l;
    l.n_samples = n_samples; l.n_var = n_var; l.off = off.as<uint64_t>(); l.idx = idx.as<uint32_t>();
    l.var_off = var_off.as<uint32_t>(); l.var_mask = var_mask.as<uint8_t>(); l.var_ref = var_ref.as<uint8_t>();
    return l;
  }
};

// the indel table of an unphased block and its (indel, carrier) instances, in HBM (hawk_api_uwin.hip)
struct hawk_uwin {
  hawk_ctx* ctx;
  hawk_ubuild* u = nullptr;             // the SNV lists the instances index: the caller's, it outlives this object
  uint32_t n_indel = 0, n_samples = 0, L = 0;
  uint64_t n_inst = 0;
  DevBuf line, allele, off, ref_len, alt_len, pool_off, pool, rank_sample, ref, inst_off, inst_indel, inst_sample, inst_lo, inst_hi;
  std::vector<uint32_t> h_off, h_ref_len, h_alt_len;  // [n_indel]
  std::vector<uint64_t> h_inst_off;                  // [n_indel + 1]
  UwDev view() const {
    UwDev d;
    d.n_indel = n_indel; d.n_samples = n_samples; d.L = L; d.n_inst = n_inst;
    d.line = line.as<uint32_t>(); d.allele = allele.as<uint8_t>(); d.off = off.as<uint32_t>(); d.ref_len = ref_len.as<uint32_t>();
    d.alt_len = alt_len.as<uint32_t>(); d.pool_off = pool_off.as<uint32_t>(); d.pool = pool.as<uint8_t>();
    d.rank_sample = rank_sample.as<uint32_t>(); d.ref = ref.as<uint8_t>(); d.inst_off = inst_off.as<uint64_t>();
    d.inst_indel = inst_indel.as<uint32_t>(); d.inst_sample = inst_sample.as<uint32_t>(); d.inst_lo = inst_lo.as<uint64_t>();
    d.inst_hi = inst_hi.as<uint64_t>();
    return d;
  }
};

struct hawk_table {
  hawk_hapset* hs;  // nullptr for a merged table (hawk_table_gather): it owns its columns
  hawk_ctx* ctx;
  uint64_t n_rows, n_cand, n_hits, cap;
  GuideCols cols;  // points into hs->colsA, or into own[] for a merged table
  uint32_t guidelen, pamlen, right;
  uint64_t n_groups;  // valid after hawk_table_collapse
  bool collapsed;
  uint64_t gen;     // hs->cols_gen when the table was written
  DevBuf own[8];
  // written by the cluster search of a plan view (hawk_csearch.hip): rows [0, offsets[plane_tiles]) are REF's, every other row is
  // a copy of one of t_rows template rows - which lets the collapse group the template rows instead of the table
  bool by_cluster = false;
  uint32_t plane_tiles = 0;
  uint64_t t_rows = 0;
};
// HAWK_E_INVALID when a later hawk_search on the same set has overwritten the table's columns
inline bool hawk_table_stale(const hawk_table* t) { return t->hs && t->gen != t->hs->cols_gen; }
// the collapse results live in the set's workspace: valid for the table that was collapsed last, until the next search
inline bool collapse_valid(const hawk_table* t) { return t && t->collapsed && t->hs && !hawk_table_stale(t) && t->hs->cws.gen == t->gen; }

// hawk_table_resolve_unphased's handle (hawk_api_resolve.hip); hawk_resolve_groups (hawk_api_ugroups.hip) reads it as well
struct hawk_resolve {
  hawk_ctx* ctx;
  hawk_hapset* hs;        // whose columns the table's rows lie in ...
  uint64_t gen = 0;       // ... as long as no later search has overwritten them
  GuideCols cols;
  UrGeom g;
  uint64_t n_rows = 0, n_kept = 0, n_resolved = 0, bcap = 0, n_keys = 0;
  DevBuf key, aoff, ref, rkeys, rvals, res, kept, off;  // the allele table, REF's sorted keys, per-row counts and offsets
  std::vector<uint64_t> h_off;                           // [n_rows + 1]
  std::vector<uint32_t> h_cnt;                           // row_resolved[n_rows], row_kept[n_rows]
  hawk_resolve_timing tm;
  bool downloaded = false;  // the fill pass has run: by hawk_resolve_download, or by hawk_resolve_groups in its place
};
inline UrDev ur_dev(const hawk_resolve* r) {
  UrDev d = {};
  d.c = r->cols; d.n = r->n_rows; d.hap_len = r->hs->d_hap_len; d.is_ref = r->hs->d_is_ref; d.n_hap = r->hs->n_hap; d.g = r->g;
  d.al.key = r->key.as<uint64_t>(); d.al.off = r->aoff.as<uint32_t>(); d.al.ref = r->ref.as<uint8_t>(); d.al.n_keys = r->n_keys;
  d.ref_key = r->rkeys.as<uint64_t>() + r->n_rows; d.ref_row = r->rvals.as<uint32_t>() + r->n_rows;
  return d;
}

// hawk_resolve_groups' result (hawk_api_ugroups.hip); hawk_effects_create_ugroups (hawk_api_effects.hip) reads it where it lies
#define UG_NBUF 13
enum { UG_B_STRAND = 3, UG_B_START = 4, UG_B_STOP = 5, UG_B_ISREF = 6, UG_B_CFDON = 7, UG_B_WIN = 8, UG_B_MOFF = 11, UG_B_MHAP = 12 };
struct hawk_ugroups {
  hawk_ctx* ctx;
  uint64_t n_groups = 0, n_members = 0;
  uint32_t n_hap = 0, guidelen = 0, pamlen = 0, right = 0;  // of the set and the table the groups were made from
  bool has_cfd = false;                                      // CFD tables were given: cfdon holds scores, not NaN alone
  DevBuf b[UG_NBUF];  // rep_src_row, hap, pos, strand, start, stop, is_ref, cfdon, win, gc_num, gc_den, member_off, member_hap
  hawk_ugroups_timing tm;
};

int hawk_reserve_cols(DevBuf (&b)[8], uint64_t cap, GuideCols* c);

// shared by the C-ABI translation units (hawk_api_*.hip)
void hawk_ottext_forget(hawk_ctx* ctx);  // hawk_api_offtarget.hip: the context's undelivered hawk_offtarget_text result goes back to the pool
int hapset_create_impl(hawk_ctx* ctx, uint32_t n_hap, const uint32_t* hap_len, bool zero_planes, hawk_hapset** out, bool alloc_planes = true);
HapSetDev make_dev(const hawk_hapset* hs);
int make_scan_params(const hawk_hapset* hs, uint64_t pam_fwd, uint64_t pam_rev, uint32_t pamlen, uint32_t guidelen,
                            uint32_t right, bool need_v, ScanParams* sp);
int meta_build(uint32_t n, const std::vector<uint32_t>& hap_len, uint32_t bph, const uint8_t* is_ref, const int32_t* scan_start,
                      const int32_t* scan_stop, const uint32_t* seg_off, const uint32_t* seg_rel, const int64_t* seg_gen,
                      int32_t ref_index, std::vector<TileMeta>* t0, int64_t* min_gen, int64_t* max_gen);
