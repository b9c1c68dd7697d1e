// hawk_cl.h — the cluster dictionary of an expansion plan: what its kernels (hawk_cldict.hip), its host side (hawk_api_cldict.hip)
// and the cluster search (hawk_csearch.hip) share - the instance constants, the records and views the launchers take, the status
// bits, the result block, and the sizes of a build.  Plain C++17: no HIP call, no HIP header (tests/test_cldict_sizes.py compiles
// cl_build_sizes with the host compiler alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define CL_LINK 64           // two variants interact only if fewer positions separate their alleles (hawk_csearch.hip)
#define CL_NONE 0xffffffffu  // an instance without a distinct cluster
#define CL_FAR (1 << 29)     // "position" of a row's closing instance: the clean run in front of it reaches the row's end
#define CL_ROW_U 4           // records per thread in the two passes over the records: their loads are in flight together
#define CL_CHUNK (256 * CL_ROW_U)
#define CL_MAX_ROWS (1u << 23)  // = HAWK_ROW_MAX_HAP (hawk_device.h; asserted in hawk_api_cldict.hip): the packed rows of a cluster search hold no higher haplotype row

// Why a dictionary is not usable (hawk_xplan_cluster_stats reports the word; 0: usable)
enum ClStatus : uint32_t {
  CL_ST_CHAIN = 1,        // a chain of more than CL_MAXWALK records (k_cl_fill)
  CL_ST_COLLISION = 2,    // two different clusters share a hash (k_cl_uid), or the full-size table failed (k_cl_enter)
  CL_ST_DECLINED = 4,     // too large, too little sharing, or nothing to share
  CL_ST_FIRST_TABLE = 8,  // the first, small table gave up (k_cl_enter): the host repeats the attempt with the full size
};

struct ClInst {  // per instance (k_cl_fill)
  int32_t* o;      // row position of the cluster's first allele (closing instance: CL_FAR)
  uint32_t* row;
  int32_t* pa;     // where the clean run in front of the instance starts: end of the previous record's allele, 0 at the row's start
  int32_t* rb;     // REF shift of that run
  uint32_t* uid;   // its distinct cluster (CL_NONE: none)
};
struct ClUniq {  // per distinct cluster: first record, records, row and row position of the instance that describes it; k_cl_describe adds the rest
  uint32_t* rec; uint32_t* n; uint32_t* row; int32_t* o; uint32_t* seg; uint32_t* span2;
};
// a slot of the table of the listed instances' clusters, and a list entry (hawk_cldict.hip says what the passes make of them)
struct __attribute__((aligned(32))) ClSlot { unsigned long long key; unsigned long long pad; uint32_t up1, ncls, refp, var; };
static_assert(sizeof(ClSlot) == 32, "table slot layout");
struct __attribute__((aligned(32))) ClListed {  // a listed instance: all the table passes need of it
  uint32_t inst, key_lo, key_hi, rec, ncls, refp; int32_t o_first; uint32_t var;
};
static_assert(sizeof(ClListed) == 32, "list entry layout");

// What k_cl_results writes and the host reads of a finished attempt, in one copy - and the device's wall clock (hawk_stamp) where
// the build's first kernel began (k_cl_chunks; a repeated attempt clears the block, the host keeps the first attempt's) and where
// k_cl_results ended.
struct ClResults {
  unsigned long long instances, table_clusters, variant_clusters, template_rows, status, begin, end, pad;
};
static_assert(sizeof(ClResults) == 64 && offsetof(ClResults, begin) == 40 && offsetof(ClResults, end) == 48, "result block layout");

// ---- what the launchers of a build take (hawk_device.h) ----------------------------------------------
struct ClPlan {  // what every pass reads of the plan
  const void* heads;        // {o, rs, alt_len, variant} per record (hawk_launch_hx_heads)
  const uint64_t* hv_off;   // [n_rows + 1] record range of every row
  const uint32_t* hap_len;
  const int32_t* ss;        // the rows' scan bounds
  const int32_t* se;
  const uint8_t* is_ref;
  const uint32_t* seg_off;  // the rows' position-map segments
  const uint32_t* seg_rel;
  uint32_t n_rows, n_var;
};
struct ClChunks {  // the rows' records in chunks of CL_CHUNK
  uint32_t* ch_off;     // [n_rows + 1] chunks in front of every row
  uint32_t* ch_row;     // [ch_bound] every chunk's row
  uint32_t ch_bound;    // the chunks' number is on the device only: grids and arrays run over this bound
  uint32_t* cnt;        // [ch_bound] instances a chunk opens (zeroed)
  uint32_t* lcnt;       // [ch_bound] ... and how many of them go on the list (zeroed; 16-byte aligned)
  uint32_t* inst_base;  // [ch_bound + 1] the scans of the two; the last entries are the totals
  uint32_t* list_base;
};
struct ClVariants {
  unsigned long long* desc;  // 8 B per variant, zeroed: {record, row} of an instance that is the variant
  uint32_t* claim;           // n_var bits: whom the first chunks described (hawk_launch_scan2_u32)
};
struct ClList {  // the instances that go through the table
  ClListed* list;
  uint32_t* state;   // per entry: CL_NONE (it opened its cluster, or failed) or the slot it waits for
  uint32_t bound;    // room on the list = the launches' bound
};
struct ClTally {
  uint32_t* counters;  // 8, zeroed: [0] the table's distinct clusters, [1] the variants that are clusters, [4..5] template rows at most
  ClResults* results;  // device copy of the result block
  uint32_t* status;    // ClStatus bits
};
struct ClBuild { ClPlan plan; ClChunks ch; ClVariants var; ClInst inst; ClList list; ClTally tally; };
struct ClTable {  // the table of one attempt
  ClSlot* tab;         // mask + 1 slots, zeroed
  uint32_t mask;
  uint32_t max_probe;  // slots an instance tries before it gives up ...
  uint32_t fail_bit;   // ... and the status bit it raises then
  uint32_t u_cap;      // range of the cluster numbers: the variants, then what the table can hold
};

// rows -> chunks: ch_row and the chunks' counts have room for n_records / CL_CHUNK + n_rows entries
inline uint32_t hawk_cl_chunk_bound(uint64_t n_records, uint32_t n_rows) { return (uint32_t)(n_records / CL_CHUNK) + n_rows; }

// ---- the sizes of a build ----------------------------------------------------------------------------
// Nothing in a build waits for a count from the device.  An instance starts at a record or closes a row, so records + rows bounds
// their number: the instance arrays, the list and the grids of the passes are sized by the bound, the passes read the true counts
// on the device, and the host learns them together with the number of distinct clusters, once, at the end.
struct ClBuildSizes {
  bool declined;  // nothing to share, or a size the cluster path cannot hold: the per-word search takes the plan (CL_ST_DECLINED)
  uint32_t ch_bound, inst_bound;
  uint32_t bm_words;  // the variants' bitmap
  // The table of the clusters that are more than their variant: at least two slots per listed instance would always do, but the
  // distinct clusters are a small fraction of the instances and clearing 32 bytes x 2^25 slots costs more than every kernel of a
  // build - so the first attempt takes two slots per distinct cluster EXPECTED (the last build's count, else an eighth of the
  // instances) and gives up after 64 probes (CL_ST_FIRST_TABLE); the attempt is then repeated with the full size.  A first
  // table that is the full one (tsmall == tsize) never gives up.
  uint32_t tsize, tsmall;
  uint32_t max_probe, fail_bit;     // of the first attempt
  uint32_t u_bound, u_bound_repeat; // cluster numbers of the first attempt and of the repeat: the variants, then what the table can hold
  // Everything that starts from zero, in ONE block cleared by ONE memset: status, counters, the device's result block, the chunks'
  // counts, the variants' bitmap and describers, the clusters' template-row bounds, the first attempt's table.  Every offset is a
  // multiple of 256 - but z_lcnt, which follows the chunks' counts rounded up to four: 16-byte aligned, because k_scan2_u32
  // loads four counts at a time.
  size_t z_status, z_counters, z_results, z_cnt, z_lcnt, z_claim, z_vdesc, z_span2, z_tab, z_end;
};
inline ClBuildSizes cl_build_sizes(uint64_t ncar, uint32_t n_rows, uint32_t n_var, uint32_t last_uniq) {
  ClBuildSizes s = {};
  // (records + rows beyond 32 bits would wrap the instance bound; rows the packed layout cannot hold would come out as other rows)
  s.declined = ncar == 0 || n_rows < 2 || ncar + n_rows >= (1ull << 32) || n_rows >= CL_MAX_ROWS;
  if (s.declined) return s;
  s.ch_bound = hawk_cl_chunk_bound(ncar, n_rows);
  s.inst_bound = (uint32_t)(ncar + n_rows);
  s.bm_words = n_var / 32 + 1;
  s.tsize = 1024;
  while (s.tsize < 2ull * s.inst_bound && s.tsize < (1u << 30)) s.tsize <<= 1;
  s.tsmall = s.tsize < (1u << 16) ? s.tsize : (1u << 16);
  const uint64_t expect = last_uniq ? (uint64_t)last_uniq * 2 : (uint64_t)s.inst_bound / 8;
  while (s.tsmall < expect && s.tsmall < s.tsize) s.tsmall <<= 1;
  const bool small = s.tsmall < s.tsize;
  s.max_probe = small ? 64u : 0xffffffffu;
  s.fail_bit = small ? CL_ST_FIRST_TABLE : CL_ST_COLLISION;
  s.u_bound = n_var + (s.tsmall < s.inst_bound ? s.tsmall : s.inst_bound);
  s.u_bound_repeat = n_var + (s.tsize < s.inst_bound ? s.tsize : s.inst_bound);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  s.z_status = 0; s.z_counters = 256; s.z_results = 512; s.z_cnt = 768;
  s.z_lcnt = s.z_cnt + (((size_t)s.ch_bound + 3) & ~(size_t)3) * 4;
  s.z_claim = s.z_cnt + up(((size_t)s.ch_bound + 4) * 8);
  s.z_vdesc = s.z_claim + up((size_t)s.bm_words * 4);
  s.z_span2 = s.z_vdesc + up((size_t)(n_var ? n_var : 1) * 8);
  s.z_tab = s.z_span2 + up((size_t)s.u_bound * 4);
  s.z_end = s.z_tab + (size_t)s.tsmall * sizeof(ClSlot);
  return s;
}
