// hawk_api_search.hip - C ABI: the fused search (hawk_search) and the guide table it leaves in HBM
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "hawk_host.h"

// The columnar layout of a guide table: eight separate allocations (see GuideCols in hawk_device.h for the packed layout).
int hawk_reserve_cols(DevBuf (&b)[8], uint64_t cap, GuideCols* c) {
  int rc;
  const size_t sz[8] = {cap * 4, cap * 4, cap, cap * 8, cap * 8, cap, cap * 8, cap * 8 * HAWK_PLANES};
  for (int i = 0; i < 8; ++i) if ((rc = b[i].reserve(std::max<size_t>(sz[i], 16)))) return rc;
  c->hap = b[0].as<uint32_t>(); c->pos = b[1].as<uint32_t>(); c->strand = b[2].as<uint8_t>();
  c->start = b[3].as<int64_t>(); c->stop = b[4].as<int64_t>(); c->flags = b[5].as<uint8_t>();
  c->cfdon = b[6].as<double>(); c->win = b[7].as<uint64_t>(); c->cap = cap;
  c->rows = nullptr; c->startp = 0;
  return HAWK_OK;
}

#define HAWK_RETRY_TEMPLATES (-100)  // private to this file: the template rows of a cluster search outgrew their reservation

// A search records no timed event.  A recorded event is a packet of its own between two kernels of its stream (5-6 us on the main
// stream of a C3 search, profiles/ref_overlap.md), and two kernels with nothing between them follow each other in 0.2 us: the
// stage boundaries are STAMPS instead - the kernel that opens the next interval stores the device's wall clock into its slot of
// SearchMisc::stamps (hawk_stamp, hawk_device.h), the memset of the search clears the slots and the status copy brings them back.
// Where an interval ends and no kernel of ours follows on that stream (the end of the emit; the offsets when no emit is queued
// behind them) a one-thread launch stamps it (hawk_launch_stamp).  An interval that begins where another one ends shares its stamp.
// The events left are the four that order the two streams of a cluster search (created without timing): the main stream records a
// fork where the side stream may begin, the side stream a join where its work is done.
enum SearchEvent { EV_COUNT_FORK = HAWK_EV_TIMED, EV_COUNT_JOIN, EV_EMIT_FORK, EV_EMIT_JOIN, EV_SLOTS };
static_assert(EV_SLOTS == sizeof(hawk_ctx::ev) / sizeof(hipEvent_t), "hawk_ctx::ev ends with the search's ordering events");
enum SearchStamp {
  ST_COUNT_BEGIN,       // the main stream's first count-side kernel: k_search_count, or k_cs_templates of a cluster search
  ST_VIEW_COUNT_BEGIN,  // pass 0 of the per-word search (a cluster search: ST_COUNT_BEGIN)
  ST_CS_COUNT,          // k_cs_count: the templates are done
  ST_SCAN_BEGIN,        // the first scan kernel: the count side is done
  ST_OFFSETS_DONE,      // the offsets are done: the first kernel of a speculative emit (which it opens as well), else a stamp launch
  ST_EMIT_BEGIN,        // the first kernel of an emit that is not queued straight behind the scan
  ST_LIST_BEGIN,        // k_emit_list where it is not the emit's first kernel (a cluster search: on the side stream)
  ST_LIST_END,          // k_search_emit
  ST_VIEW_EMIT_BEGIN,   // pass 1 of the per-word search; k_rows_pack of a cluster search
  ST_EMIT_END,          // a stamp launch in front of the status copy
  ST_SLOTS
};
static_assert(ST_SLOTS <= HAWK_SEARCH_STAMPS, "SearchMisc::stamps holds every slot");

// One attempt of hawk_search: what its stages share.  search_classify .. search_view_args fill it, the stages behind them read it.
struct SearchRun {
  hawk_hapset* hs; hawk_ctx* ctx; hipStream_t st;
  hipStream_t side;               // where REF's plane passes of a cluster search run, beside the cluster passes on st
  const hawk_xplan* vx;           // the plan a view is searched from (nullptr: a set with planes, every row through the plane kernels)
  bool by_cluster;                // ... per distinct cluster (hawk_csearch.hip); false: per dirty word (hawk_vsearch.hip)
  HapSetDev d; ScanParams sp; GuideParams gp; RefInfo ri; VcArgs va; ClDict cd;
  uint64_t ntile, nscan;          // tiles of all rows; entries of the offset scan
  uint32_t plane_tiles, v_tiles;  // tiles the plane kernels take; tiles left to the per-word search
  uint64_t tcap, t_rows_used;     // cluster search: template rows reserved, and produced
  uint64_t stage_cap;             // ... rows of REF staged as columns: at most every window start of both strands
  unsigned long long* shards;     // hs->misc on the device (SearchMisc): the shard sums ...
  SearchStatusBlock* blk;         // ... and the status block every launcher is handed its fields of
  SearchStatusBlock* h;           // the status block as last read back (hawk_ctx::pinned)
  unsigned long long* stamps;     // SearchMisc::stamps on the device, [ST_SLOTS]
  const unsigned long long* h_stamps;  // ... and as last read back
  uint64_t* table_cap;            // rows the set's table holds: hs->rows_cap for a cluster search, else hs->cols_cap
  SearchStamp emit_begin;         // what opened the last emit: ST_OFFSETS_DONE straight behind the scan (a speculative emit), else ST_EMIT_BEGIN
};

// Parameter checks, and which path runs.  A view of an expansion plan (hawk_xplan_view) holds no planes: its REF row runs through the
// plane kernels on the plan's REF planes (hand-over lists included); every other row per distinct cluster when the plan's dictionary
// is usable (hawk_csearch.hip: the scan then runs over REF's tiles + one count per cluster instance), else - or with
// HAWK_VIEW_SEARCH=words, read per call - per dirty word (hawk_vsearch.hip).
static int search_classify(hawk_hapset* hs, const hawk_search_params* p, SearchRun* r) {
  if (!hs || !p || !hs->has_meta || p->score_cfdon > 2) return HAWK_E_INVALID;
  if (p->score_cfdon && (p->right || !p->cfd_mm || !p->cfd_pam || p->pamlen < 2)) return HAWK_E_INVALID;
  r->hs = hs; r->ctx = hs->ctx; r->st = hs->ctx->stream; r->side = hs->ctx->side; r->vx = hs->vplan;
  HIPCHK(hipSetDevice(r->ctx->device));
  const int rc = make_scan_params(hs, p->pam_fwd, p->pam_rev, p->pamlen, p->guidelen, p->right, true, &r->sp);
  if (rc) return rc;
  r->d = make_dev(hs);
  ++hs->cols_gen;  // the columns are about to be rewritten: earlier tables of this set become stale
  const hawk_xplan* vx = r->vx;
  if (vx && (hs->ref_index != 0 || hs->n_ref_rows != 1)) return HAWK_E_INVALID;  // a plan's rows: REF first, once
  r->by_cluster = vx && vx->cl.built && vx->cl.usable;
  if (r->by_cluster) { const char* e = getenv("HAWK_VIEW_SEARCH"); if (e && e[0] == 'w') r->by_cluster = false; }
  r->ntile = (uint64_t)hs->n_hap * r->sp.bph;
  // what the offset scan runs over: the plane kernels' tiles, then - for a cluster search - one entry per 64 consecutive cluster
  // instances (a wave of the count / emit kernels: its rows are one contiguous stretch of the table), else the view's tiles
  r->nscan = r->by_cluster ? (uint64_t)r->sp.bph + ((uint64_t)vx->cl.n_inst + 63) / 64 : r->ntile;
  r->plane_tiles = vx ? r->sp.bph : (uint32_t)r->ntile;
  r->v_tiles = (uint32_t)r->ntile - r->plane_tiles;
  r->stage_cap = r->by_cluster ? 2ull * hs->hap_len[hs->ref_index] + 64 : 0;
  r->table_cap = r->by_cluster ? &hs->rows_cap : &hs->cols_cap;
  r->tcap = r->t_rows_used = 0;
  r->emit_begin = ST_EMIT_BEGIN;
  return HAWK_OK;
}
// The workspaces every path needs, and what points into them.  Hand-over lists (2 KB per tile): the count pass leaves each small
// tile's valid survivors for the emit pass.  A REF tile takes one work-list entry per 512 survivors (<= 128 per tile), any other big tile one.
static int search_reserve(SearchRun* r, const hawk_search_params* p) {
  hawk_hapset* hs = r->hs;
  const ScanParams& sp = r->sp;
  const uint64_t n_ref_tiles = (uint64_t)sp.bph * hs->n_ref_rows;
  int rc;
  if ((rc = hs->counts.reserve(r->nscan * 4)) || (rc = hs->offsets.reserve((r->nscan + 1) * 8)) || (rc = hs->misc.reserve(sizeof(SearchMisc))) ||
      (rc = hs->cfd.reserve(336 * 8)) || (rc = hs->partial.reserve((r->nscan / 1024 + 2) * 8)) ||
      (rc = hs->lists.reserve((size_t)r->plane_tiles * HAWK_LIST_CAP * 4 + 16)) || (rc = hs->big.reserve(((size_t)r->plane_tiles + 128 * n_ref_tiles) * 8 + 16)))
    return rc;
  r->shards = &hs->misc.as<SearchMisc>()->shards[0][0];
  r->blk = &hs->misc.as<SearchMisc>()->blk;
  r->h = &static_cast<PinnedBlock*>(r->ctx->pinned)->search;
  r->stamps = hs->misc.as<SearchMisc>()->stamps;
  r->h_stamps = static_cast<PinnedBlock*>(r->ctx->pinned)->stamps;
  GuideParams& gp = r->gp;
  gp.pamlen = sp.pamlen; gp.guidelen = sp.guidelen; gp.right = sp.right; gp.L = sp.L;
  gp.score_cfdon = (int32_t)p->score_cfdon;  // 1: a non-ACGT base under a lookup is HAWK_E_CFD; 2: it scores NaN ("NA")
  gp.cfd_mm = hs->cfd.as<double>(); gp.cfd_pam = hs->cfd.as<double>() + 320; gp.bph = sp.bph;
  return HAWK_OK;
}
// The CFD tables go up once; later searches with the same tables find them in HBM.
static int search_upload_cfd(SearchRun* r, const hawk_search_params* p) {
  hawk_hapset* hs = r->hs;
  if (!p->score_cfdon) return HAWK_OK;
  if (hs->cfd_host.size() == 336 && memcmp(hs->cfd_host.data(), p->cfd_mm, 320 * 8) == 0 && memcmp(hs->cfd_host.data() + 320, p->cfd_pam, 16 * 8) == 0) return HAWK_OK;
  hs->cfd_host.assign(336, 0.0);
  memcpy(hs->cfd_host.data(), p->cfd_mm, 320 * 8);
  memcpy(hs->cfd_host.data() + 320, p->cfd_pam, 16 * 8);
  HIPCHK(hipMemcpyAsync(hs->cfd.p, hs->cfd_host.data(), 336 * 8, hipMemcpyHostToDevice, r->st));
  HIPCHK(hipStreamSynchronize(r->st));
  return HAWK_OK;
}
// Where REF has guides a haplotype row can be grouped with (RefInfo) and, cached on the set, REF's candidate windows as bitmaps
// (k_ref_bits) + for a view REF's PAM hits and prefix counts (k_ref_hits: what the clean stretches of a plan's rows are counted
// from).  Both are rebuilt only when the PAM / guide geometry or REF's range changed.
static int search_ref(SearchRun* r, const hawk_search_params* p) {
  hawk_hapset* hs = r->hs;
  const ScanParams& sp = r->sp;
  RefInfo& ri = r->ri;
  ri.index = hs->ref_index; ri.startp = hs->ref_startp;
  ri.bits[0] = ri.bits[1] = nullptr; ri.n_bits = 0;
  for (int s = 0; s < 2; ++s) {
    ri.lo[s] = 0; ri.hi[s] = 0;
    if (hs->ref_index < 0) continue;
    // same arithmetic as the kernel's phase A, for the REF haplotype
    const bool pamfirst = (sp.right != 0) != (s != 0);
    const int po = pamfirst ? 0 : sp.guidelen;
    const int haplen = (int)hs->hap_len[hs->ref_index];
    // REF's own scan range, or - for a tile of a larger region - the region's scan range as far as this tile's REF string
    // reaches (hawk_hapset_set_ref_partner_range)
    const int rs = hs->has_partner ? hs->partner_start : hs->scan_start[hs->ref_index];
    const int re = hs->has_partner ? hs->partner_stop : hs->scan_stop[hs->ref_index];
    ri.lo[s] = std::max(rs - po, HAWK_PAD);
    ri.hi[s] = std::min(re - po, haplen - sp.L - HAWK_PAD + 1);
  }
  if (hs->ref_index < 0) return HAWK_OK;
  const uint64_t key[6] = {p->pam_fwd, p->pam_rev, ((uint64_t)p->pamlen << 32) | p->guidelen, (uint64_t)(p->right ? 1 : 0),
                           ((uint64_t)(uint32_t)ri.lo[0] << 32) | (uint32_t)ri.hi[0], ((uint64_t)(uint32_t)ri.lo[1] << 32) | (uint32_t)ri.hi[1]};
  int rc;
  if ((rc = hs->refbits.reserve((size_t)hs->S * 4 * 2))) return rc;
  ri.bits[0] = hs->refbits.as<uint32_t>(); ri.bits[1] = hs->refbits.as<uint32_t>() + hs->S;
  ri.n_bits = hs->S * 32u;
  if (r->vx && ((rc = hs->refhp.reserve(((size_t)hs->S + 1) * 8 * 2)) || (rc = hs->vcnt0.reserve(r->by_cluster ? 16 : r->ntile * 4)))) return rc;
  if (hs->refbits_valid && memcmp(hs->refbits_key, key, sizeof(key)) == 0) return HAWK_OK;
  hawk_launch_ref_bits(r->st, r->d, sp, ri, hs->refbits.as<uint32_t>(), hs->refbits.as<uint32_t>() + hs->S);
  if (r->vx) hawk_launch_ref_hits(r->st, r->d, sp, hs->ref_index, hs->refhp.p);
  HIPCHK(hipGetLastError());
  memcpy(hs->refbits_key, key, sizeof(key));
  hs->refbits_valid = true;
  return HAWK_OK;
}
// What a view's kernels read beside the rows' metadata: the plan's records (VcArgs) and, for a cluster search, the dictionary
// (ClDict) with the room for this search's template rows.
static int search_view_args(SearchRun* r) {
  hawk_hapset* hs = r->hs;
  const hawk_xplan* vx = r->vx;
  VcArgs& va = r->va; ClDict& cd = r->cd;
  memset(&va, 0, sizeof(va)); memset(&cd, 0, sizeof(cd));
  if (!vx) return HAWK_OK;
  for (int pl = 0; pl < 4; ++pl) va.ref[pl] = vx->ref5[pl].as<uint32_t>();
  va.ref_S = hs->S; va.hp = hs->refhp.as<uint4>();
  va.recs_ = vx->recs.p; va.alt_codes = vx->codes.as<uint8_t>(); va.hv_off = vx->off.as<uint64_t>(); va.tiles_ = vx->tiles.p;
  if (!r->by_cluster) return HAWK_OK;
  const ClusterDictionary& cl = vx->cl;
  cd = cl.view();
  // template rows: packed as the search produces them.  Their number is bounded by the window starts of the distinct clusters
  // (cl.slots: 2 strands x every start), but a PAM keeps a few per cent of those: reserve 16 rows per distinct cluster, and
  // if a search needs more it produces no table (k_cs_count sees the counter), says so and is rerun with the bound reserved
  const char* e0 = getenv("HAWK_CLUSTER_ROWS0");  // tests: a first reservation small enough to overflow (read per call)
  const uint64_t first = e0 ? strtoull(e0, nullptr, 10) : 16ull * cl.n_uniq + 65536;
  r->tcap = std::max<uint64_t>(std::min<uint64_t>(cl.slots, std::max<uint64_t>(hs->cs_tcap, first)), 1);
  // (cs_res, 32 bytes per distinct cluster: {rows per strand, hits, candidates} {first template row, REF's hits before / behind it})
  const size_t n_uniq = std::max<uint32_t>(cl.n_uniq, 1), n_inst = std::max<uint32_t>(cl.n_inst, 1);
  int rc;
  if ((rc = hs->cs_res.reserve(n_uniq * 32)) || (rc = hs->cs_tbase.reserve(n_uniq * 4)) || (rc = hs->cs_trows.reserve((size_t)r->tcap * hawk_cs_row_bytes())) ||
      (rc = hs->cs_inst.reserve(n_inst * 16)))
    return rc;
  return HAWK_OK;
}
// The side stream's work behind a fork is done -> the main stream goes on.  Nothing between a fork and its join returns: if the join
// cannot be queued the host waits for the side stream instead, so no caller ever meets REF's kernels still in flight.
// (The wait costs the main stream about 6 us although REF's passes ended long before.  Joining on the HOST instead - it waits for
// the side stream, then queues what follows - removes both wait packets from a C3 trace and 0.005-0.012 ms of device time, but the step's
// wall time did not follow beyond its run-to-run spread at C3, an eighth of it, or C4: profiles/search_stamps.md.  Not built in.)
static hipError_t search_join(SearchRun* r, SearchEvent done) {
  hipError_t e = hipEventRecord(r->ctx->ev[done], r->side);
  if (e == hipSuccess) e = hipStreamWaitEvent(r->st, r->ctx->ev[done], 0);
  if (e != hipSuccess) (void)hipStreamSynchronize(r->side);
  return e;
}

// The count side: the plane kernels' tiles, then the view's share - templates + a count per cluster instance, or pass 0 of the
// per-word search - then the offset scan, which leaves the totals in the status block.  A cluster search forks: REF's tiles are
// counted on the side stream (counts[0, plane_tiles), the hand-over lists, the work list) while the main stream makes the templates
// and counts the instances (counts[plane_tiles, ..)); the shard sums and the status take atomics from both.  The scan reads both
// halves: the join stands right in front of it.  The stamps: every kernel named below stamps its own begin, so the cluster passes'
// brackets hold nothing but their kernels; `emit_follows`: a speculative emit is queued straight behind the scan and its first
// kernel stamps the offsets done, else a stamp launch does.
static int search_count(SearchRun* r, bool emit_follows) {
  hawk_hapset* hs = r->hs; hipStream_t st = r->st; hipEvent_t* ev = r->ctx->ev;
  SearchStatusBlock* blk = r->blk; uint32_t* counts = hs->counts.as<uint32_t>();
  unsigned long long* stamps = r->stamps;
  const bool fork = r->by_cluster;
  if (fork) {
    // the fork stands at the head, where the device is waiting for the host anyway: behind the memset, in front of the templates
    HIPCHK(hipEventRecord(ev[EV_COUNT_FORK], st));
    hawk_launch_cs_templates(st, r->d, r->va, r->cd, r->sp, r->gp, r->ri, hs->cs_res.p, hs->cs_tbase.as<uint32_t>(), hs->cs_trows.p, &blk->template_rows,
                             r->tcap, &blk->status, stamps + ST_COUNT_BEGIN);
    hawk_launch_cs_count(st, r->d, r->va, r->cd, r->sp, hs->cs_res.p, &blk->template_rows, r->tcap, counts + r->plane_tiles, hs->cs_inst.p,
                         r->shards, stamps + ST_CS_COUNT);
    // the main stream's kernels are queued first
    HIPCHK(hipStreamWaitEvent(r->side, ev[EV_COUNT_FORK], 0));  // (nothing is queued on the side stream yet)
    hawk_launch_search(r->side, 0, r->d, r->sp, r->gp, r->ri, hs->d_tile_meta, counts, r->shards, nullptr, GuideCols{}, &blk->status, hs->lists.as<uint32_t>(),
                       &blk->big_count, hs->big.as<unsigned long long>(), r->plane_tiles);
    HIPCHK(search_join(r, EV_COUNT_JOIN));
  } else {
    hawk_launch_search(st, 0, r->d, r->sp, r->gp, r->ri, hs->d_tile_meta, counts, r->shards, nullptr, GuideCols{}, &blk->status, hs->lists.as<uint32_t>(),
                       &blk->big_count, hs->big.as<unsigned long long>(), r->plane_tiles, stamps + ST_COUNT_BEGIN);
    if (r->vx)
      hawk_launch_vsearch(st, 0, r->d, r->va, r->sp, r->gp, r->ri, hs->d_tile_meta, counts, hs->vcnt0.as<uint32_t>(), r->shards, nullptr, GuideCols{}, &blk->status,
                          r->plane_tiles, r->v_tiles, stamps + ST_VIEW_COUNT_BEGIN);
  }
  hawk_launch_mscan(st, counts, r->nscan, hs->partial.as<unsigned long long>(), r->shards, hs->offsets.as<uint64_t>(), &blk->totals, stamps + ST_SCAN_BEGIN);
  if (!emit_follows) hawk_launch_stamp(st, stamps + ST_OFFSETS_DONE);
  HIPCHK(hipGetLastError());
  return HAWK_OK;
}
// Reserve for `cap` rows: `cols` is what the column emitters write, `table` what the finished table is
static int search_reserve_table(SearchRun* r, uint64_t cap, GuideCols* cols, GuideCols* table) {
  hawk_hapset* hs = r->hs;
  int rc;
  if ((rc = hawk_reserve_cols(hs->colsA, r->by_cluster ? r->stage_cap : cap, cols))) return rc;
  *table = *cols;
  if (!r->by_cluster) return HAWK_OK;
  if ((rc = hs->rowsA.reserve(cap * 64))) return rc;  // colsA then stages REF's rows only
  memset(table, 0, sizeof(*table));
  table->rows = hs->rowsA.as<uint4>(); table->cap = cap; table->startp = r->ri.startp;
  return HAWK_OK;
}
// The emit side, between its two stamps (`launch` false: a table of no rows - two stamp launches); `behind_scan`: nothing has been
// queued since the offset scan, and the stamp that opens the emit closes the offsets as well.  Plane kernels (all rows of a set with planes; REF's
// rows of a view) and the per-word search of a view write columns; the cluster search writes packed rows (k_cs_emit_rows), and REF's
// rows - staged as columns - are packed in front of them.  The kernels take their offsets from HBM and refuse to write past the capacity.
// A cluster search forks here too: REF's emit chain and its packing run on the side stream and write the table's rows
// [0, offsets[plane_tiles]) (through the staging columns, which nothing else touches); k_cs_emit_rows, the only kernel on the main stream,
// writes every row behind them.  The join stands in front of the end stamp, and so in front of whatever reads the status block or the
// table.  The fork is the one event left between two kernels of the main stream: REF's chain needs the offsets.
static int search_emit(SearchRun* r, const GuideCols& cols, const GuideCols& packed, bool launch, bool behind_scan) {
  hawk_hapset* hs = r->hs; hipStream_t st = r->st; hipEvent_t* ev = r->ctx->ev;
  SearchStatusBlock* blk = r->blk; const uint64_t* offsets = hs->offsets.as<uint64_t>();
  unsigned long long* stamps = r->stamps;
  r->emit_begin = behind_scan ? ST_OFFSETS_DONE : ST_EMIT_BEGIN;
  unsigned long long* begin = stamps + r->emit_begin;
  if (launch) {
    const hipStream_t ref_st = r->by_cluster ? r->side : st;
    if (r->by_cluster) {  // the main stream's kernel first, then the fork (nothing is queued on the side stream yet)
      HIPCHK(hipEventRecord(ev[EV_EMIT_FORK], st));
      hawk_launch_cs_emit_rows(st, r->cd.n_inst, hs->cs_inst.p, hs->cs_trows.p, offsets + r->plane_tiles, &blk->template_rows,
                               r->tcap, packed.rows, packed.cap, &blk->status, begin);
      HIPCHK(hipStreamWaitEvent(r->side, ev[EV_EMIT_FORK], 0));
    }
    // k_emit_list opens the emit where it is the first kernel; k_search_emit begins where it ends
    hawk_launch_search(ref_st, 1, r->d, r->sp, r->gp, r->ri, hs->d_tile_meta, hs->counts.as<uint32_t>(), r->shards, offsets, cols, &blk->status, hs->lists.as<uint32_t>(),
                       &blk->big_count, hs->big.as<unsigned long long>(), r->plane_tiles, r->by_cluster ? stamps + ST_LIST_BEGIN : begin, stamps + ST_LIST_END);
    if (r->by_cluster) {
      hawk_launch_rows_pack(ref_st, cols, offsets + r->plane_tiles, 0, std::min<uint64_t>(r->stage_cap, packed.cap), packed.rows, packed.startp, &blk->status,
                            stamps + ST_VIEW_EMIT_BEGIN);
      HIPCHK(search_join(r, EV_EMIT_JOIN));
    } else if (r->vx) {
      hawk_launch_vsearch(st, 1, r->d, r->va, r->sp, r->gp, r->ri, hs->d_tile_meta, hs->counts.as<uint32_t>(), hs->vcnt0.as<uint32_t>(), r->shards, offsets, cols,
                          &blk->status, r->plane_tiles, r->v_tiles, stamps + ST_VIEW_EMIT_BEGIN);
    }
  } else {
    hawk_launch_stamp(st, begin);
  }
  hawk_launch_stamp(st, stamps + ST_EMIT_END);
  HIPCHK(hipGetLastError());
  return HAWK_OK;
}
// The status block after the count side (and a speculative emit): totals, status, and the template rows a cluster search used.
// If those outgrew their reservation the rerun reserves what this search asked for (+ 1/8), at most the plan's bound.
static int search_read_block(SearchRun* r) {
  HIPCHK(hipMemcpyAsync(r->h, r->blk, sizeof(SearchStatusBlock) + sizeof(SearchMisc::stamps), hipMemcpyDeviceToHost, r->st));
  HIPCHK(hipStreamSynchronize(r->st));
  if (!r->by_cluster) return HAWK_OK;
  const uint64_t tcu = r->h->template_rows;
  if (tcu > r->tcap) { r->hs->cs_tcap = std::min<uint64_t>(r->vx->cl.slots, tcu + tcu / 8 + 64); return HAWK_RETRY_TEMPLATES; }
  r->t_rows_used = tcu;
  return HAWK_OK;
}

// The intervals, from the stamps as last read back.  The device's clock begins an interval with the kernel that opens it: the time the
// device stood idle in front of a stage's first kernel belongs to no interval.
static void search_timing(const SearchRun* r, uint64_t nrows, hawk_timing* timing) {
  const hawk_hapset* hs = r->hs; const unsigned long long* t = r->h_stamps;
  const auto ms = [&](int a, int b) { return hawk_stamp_ms(r->ctx, t[a], t[b]); };
  const SearchStamp emit_begin = r->emit_begin;
  memset(timing, 0, sizeof(*timing));
  timing->count_ms = ms(ST_COUNT_BEGIN, ST_SCAN_BEGIN);
  timing->offsets_ms = ms(ST_SCAN_BEGIN, ST_OFFSETS_DONE);
  timing->emit_ms = ms(emit_begin, ST_EMIT_END);
  if (nrows) timing->emit_list_ms = ms(r->by_cluster ? ST_LIST_BEGIN : emit_begin, ST_LIST_END);
  timing->total_ms = ms(ST_COUNT_BEGIN, ST_EMIT_END);
  if (r->vx) {
    // a cluster search: the main stream holds the cluster passes alone, their brackets open with the stage's
    const SearchStamp v_count_begin = r->by_cluster ? ST_COUNT_BEGIN : ST_VIEW_COUNT_BEGIN;
    timing->v_count_ms = ms(v_count_begin, ST_SCAN_BEGIN);
    if (nrows) timing->v_emit_ms = ms(ST_VIEW_EMIT_BEGIN, ST_EMIT_END);
    timing->v_path = r->by_cluster ? 2u : 1u;
    if (r->by_cluster) timing->v_templates_ms = ms(v_count_begin, ST_CS_COUNT);
    if (r->by_cluster && nrows) timing->v_emit_rows_ms = ms(emit_begin, ST_EMIT_END);
  }
  uint64_t pos = 0;
  for (uint32_t h = 0; h < hs->n_hap; ++h) pos += (uint64_t)std::max(0, hs->scan_stop[h] - hs->scan_start[h]);
  timing->scanned_positions = pos;
}

static int search_make_table(const SearchRun* r, const hawk_search_params* p, const GuideCols& tc, hawk_table** out) {
  hawk_table* t = new (std::nothrow) hawk_table();
  if (!t) return HAWK_E_INVALID;
  const ScanTotals& tot = r->h->totals;
  t->hs = r->hs; t->ctx = r->ctx; t->gen = r->hs->cols_gen;
  t->n_rows = tot.n_keep; t->n_cand = tot.n_cand; t->n_hits = tot.n_hits; t->cols = tc; t->cap = tc.cap;
  t->guidelen = p->guidelen; t->pamlen = p->pamlen; t->right = p->right ? 1 : 0; t->n_groups = 0; t->collapsed = false;
  t->by_cluster = r->by_cluster; t->plane_tiles = r->plane_tiles; t->t_rows = r->by_cluster ? r->t_rows_used : 0;
  *out = t;
  return HAWK_OK;
}

// One attempt: the count side, then the table.  Its recovery rule, in one place:
//  * a table an earlier search on this set reserved takes a SPECULATIVE emit straight behind the offset scan, instead of waiting for
//    the row count to cross PCIe.  The status block then decides: template rows beyond their reservation - no table,
//    HAWK_RETRY_TEMPLATES (hawk_search reruns the attempt with more reserved); the rows fit the speculative emit - finished; else
//    reserve for the rows and emit (again);
//  * only the capacity refusal of a speculative emit is answered by emitting again.  Any other status was raised by the count side
//    (a strict-mode CFD error, an unsupported coordinate range) and stands - the kernels keep the FIRST status they raise;
//  * a cluster search runs REF's plane passes on the context's side stream (search_count, search_emit): each fork is joined into the
//    main stream before the stage returns, on its error paths too, so every return below leaves nothing in flight beside the main stream.
static int hawk_search_once(hawk_hapset* hs, const hawk_search_params* p, hawk_table** out, hawk_timing* timing) {
  if (!out) return HAWK_E_INVALID;
  SearchRun r;
  int rc;
  if ((rc = search_classify(hs, p, &r)) || (rc = search_reserve(&r, p)) || (rc = search_upload_cfd(&r, p))) return rc;
  HIPCHK(hipMemsetAsync(r.hs->misc.p, 0, sizeof(SearchMisc), r.st));
  if ((rc = search_ref(&r, p)) || (rc = search_view_args(&r))) return rc;
  uint64_t& table_cap = *r.table_cap;
  const bool speculative = table_cap != 0;
  if ((rc = search_count(&r, speculative))) return rc;
  GuideCols cols, table;
  if (speculative && ((rc = search_reserve_table(&r, table_cap, &cols, &table)) || (rc = search_emit(&r, cols, table, true, true)))) return rc;
  if ((rc = search_read_block(&r))) return rc;
  const uint64_t nrows = r.h->totals.n_keep;
  if (!speculative || nrows > table_cap) {
    const int status = r.h->status;
    if (status && !(speculative && status == HAWK_E_CAPACITY)) return status;
    if (speculative) HIPCHK(hipMemsetAsync(&r.blk->status, 0, sizeof(int), r.st));
    if ((rc = search_reserve_table(&r, std::max<uint64_t>(std::max<uint64_t>(nrows, 1), table_cap), &cols, &table))) return rc;
    table_cap = table.cap;
    if ((rc = search_emit(&r, cols, table, nrows != 0, false))) return rc;
    // (the status, and the stamps of this emit; nothing else in the block has changed)
    HIPCHK(hipMemcpyAsync(r.h, r.blk, sizeof(SearchStatusBlock) + sizeof(SearchMisc::stamps), hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
  }
  if (timing) search_timing(&r, nrows, timing);
  if (r.h->status) return r.h->status;
  return search_make_table(&r, p, table, out);
}

extern "C" {

int hawk_search(hawk_hapset* hs, const hawk_search_params* p, hawk_table** out, hawk_timing* timing) {
  int rc = hawk_search_once(hs, p, out, timing);
  if (rc == HAWK_RETRY_TEMPLATES) rc = hawk_search_once(hs, p, out, timing);  // now reserved for the bound: cannot recur
  return rc == HAWK_RETRY_TEMPLATES ? HAWK_E_CAPACITY : rc;
}

void hawk_table_destroy(hawk_table* t) {  // columns live in the hapset's workspace, or in own[] for a merged table
  if (!t) return;
  if (!t->hs) {
    (void)hipSetDevice(t->ctx->device);
    (void)hipStreamSynchronize(t->ctx->stream);
    for (auto& b : t->own) b.release();
  }
  delete t;
}

int hawk_table_counts(const hawk_table* t, uint64_t* n_rows, uint64_t* n_candidates, uint64_t* n_hits) {
  if (!t) return HAWK_E_INVALID;
  if (n_rows) *n_rows = t->n_rows;
  if (n_candidates) *n_candidates = t->n_cand;
  if (n_hits) *n_hits = t->n_hits;
  return HAWK_OK;
}

int hawk_table_download(hawk_table* t, uint32_t* hap, uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* stop,
                        uint8_t* flags, double* cfdon, uint64_t* win) {
  if (!t || hawk_table_stale(t)) return HAWK_E_INVALID;
  hawk_ctx* ctx = t->ctx;
  HIPCHK(hipSetDevice(ctx->device));
  const uint64_t n = t->n_rows;
  if (!n) return HAWK_OK;
  GuideCols c = t->cols;
  PoolScope tmp;
  if (c.rows) {  // packed rows: the asked-for columns are cut out on the device first
    GuideCols u;
    memset(&u, 0, sizeof(u));
    u.cap = n;
    if (hap) TEMPCHK(tmp, &u.hap, n * 4);
    if (pos) TEMPCHK(tmp, &u.pos, n * 4);
    if (strand) TEMPCHK(tmp, &u.strand, n);
    if (start) TEMPCHK(tmp, &u.start, n * 8);
    if (stop) TEMPCHK(tmp, &u.stop, n * 8);
    if (flags) TEMPCHK(tmp, &u.flags, n);
    if (cfdon) TEMPCHK(tmp, &u.cfdon, n * 8);
    if (win) TEMPCHK(tmp, &u.win, n * 8 * HAWK_PLANES);
    hawk_launch_rows_unpack(ctx->stream, c.rows, n, c.startp, u);
    HIPCHK(hipGetLastError());
    c = u;
  }
  if (hap) HIPCHK(hipMemcpyAsync(hap, c.hap, n * 4, hipMemcpyDefault, ctx->stream));
  if (pos) HIPCHK(hipMemcpyAsync(pos, c.pos, n * 4, hipMemcpyDefault, ctx->stream));
  if (strand) HIPCHK(hipMemcpyAsync(strand, c.strand, n, hipMemcpyDefault, ctx->stream));
  if (start) HIPCHK(hipMemcpyAsync(start, c.start, n * 8, hipMemcpyDefault, ctx->stream));
  if (stop) HIPCHK(hipMemcpyAsync(stop, c.stop, n * 8, hipMemcpyDefault, ctx->stream));
  if (flags) HIPCHK(hipMemcpyAsync(flags, c.flags, n, hipMemcpyDefault, ctx->stream));
  if (cfdon) HIPCHK(hipMemcpyAsync(cfdon, c.cfdon, n * 8, hipMemcpyDefault, ctx->stream));
  if (win)
    for (int p = 0; p < HAWK_PLANES; ++p)
      HIPCHK(hipMemcpyAsync(win + (size_t)p * n, c.win + (size_t)p * c.cap, n * 8, hipMemcpyDefault, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return HAWK_OK;
}

int hawk_table_layout(const hawk_table* t, uint32_t* layout, int64_t* startp) {
  if (!t || !layout) return HAWK_E_INVALID;
  *layout = t->cols.rows ? HAWK_LAYOUT_ROWS : HAWK_LAYOUT_COLUMNS;
  if (startp) *startp = t->cols.rows ? t->cols.startp : 0;
  return HAWK_OK;
}

int hawk_table_download_rows(hawk_table* t, void* rows64) {
  if (!t || hawk_table_stale(t) || !rows64) return HAWK_E_INVALID;
  if (!t->cols.rows) return HAWK_E_UNSUPPORTED;
  HIPCHK(hipSetDevice(t->ctx->device));
  if (t->n_rows) HIPCHK(hipMemcpyAsync(rows64, t->cols.rows, t->n_rows * 64, hipMemcpyDefault, t->ctx->stream));
  HIPCHK(hipStreamSynchronize(t->ctx->stream));
  return HAWK_OK;
}

int hawk_table_device_rows(hawk_table* t, void** rows64, int64_t* startp) {
  if (!t || hawk_table_stale(t) || !rows64) return HAWK_E_INVALID;
  if (!t->cols.rows) return HAWK_E_UNSUPPORTED;
  *rows64 = t->cols.rows;
  if (startp) *startp = t->cols.startp;
  return HAWK_OK;
}

int hawk_table_device_columns(hawk_table* t, void** hap, void** pos, void** strand, void** start, void** stop,
                              void** flags, void** cfdon, void** win, uint64_t* win_plane_stride) {
  if (!t || hawk_table_stale(t)) return HAWK_E_INVALID;
  const GuideCols& c = t->cols;
  if (c.rows) return HAWK_E_UNSUPPORTED;  // packed rows: hawk_table_device_rows
  if (hap) *hap = c.hap;
  if (pos) *pos = c.pos;
  if (strand) *strand = c.strand;
  if (start) *start = c.start;
  if (stop) *stop = c.stop;
  if (flags) *flags = c.flags;
  if (cfdon) *cfdon = c.cfdon;
  if (win) *win = c.win;
  if (win_plane_stride) *win_plane_stride = c.cap;  // plane p of the window slices starts at win + p * stride
  return HAWK_OK;
}

}  // extern "C"
