// hawk_device.h — device-side data model shared by the kernels (hawk_kernels.hip) and the
// C-ABI host layer (hawk_api.hip).  gfx950 only: 64-wide wavefronts are assumed throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hawk_cl.h"

#define HAWK_PLANES 5   // A, C, G, T (the IUPAC nibble's bits, encoder.py:18-34) and V (lower case)
#define HAWK_PAD 10     // GUIDESEQPAD, guide.py:21
#define HAWK_BLOCK 256  // threads per workgroup = 4 wavefronts
#define HAWK_WPT 4      // 32-base words per thread (one 16-byte load per plane)

// A haplotype set resident in HBM.  Plane p of haplotype h is plane[p] + h*S words; bit j of
// word w is base 32*w + j.  Rows are zero past hap_len and S >= words(hap_len) + 2, S % 4 == 0,
// so a 64-bit look-ahead never leaves the row and never sees another haplotype.
struct HapSetDev {
  uint32_t n_hap;
  uint32_t S;
  const uint32_t* plane[HAWK_PLANES];
  const uint32_t* hap_len;
  const uint8_t* is_ref;
  const int32_t* scan_start;
  const int32_t* scan_stop;
  const uint32_t* seg_off;
  const uint32_t* seg_rel;
  const int64_t* seg_gen;
  int32_t ref_index;
};

// Everything a search workgroup needs to know about its tile, in one 32-byte record so that a single scalar
// load (instead of a chain of dependent ones) stands between the kernel arguments and the plane loads.
struct TileMeta {
  uint32_t h, blk;       // haplotype row, tile index within the row
  uint32_t hap_len;
  int32_t scan_start, scan_stop;
  uint32_t is_ref;
  uint32_t seg0, seg_end;  // first position-map segment the tile needs; end of the haplotype's segments
};

struct ScanParams {
  uint64_t pam_fwd, pam_rev;  // PAM.bits / PAM.bitsrc: first PAM base in the most significant nibble
  int32_t pamlen, guidelen, right;
  int32_t L;                  // guidelen + pamlen
  uint32_t bph;               // workgroups per haplotype row
  uint32_t need;              // bit p set: plane p is read by this PAM (bit 4: V plane)
  int32_t poF, poR;           // raw scan: PAM offset inside the window per strand (0 = index by PAM position)
};

// Totals written by k_offsets.
struct ScanTotals {
  uint64_t n_keep;     // bits set in the keep planes (fwd + rev)
  uint64_t n_keep_fwd; // raw mode: forward total (reverse hits start here in the scan order)
  uint64_t n_cand;     // PAM hits passing is_pamhit_in_range
  uint64_t n_hits;     // PAM hits inside the scan range
};

// The guide table.  Two layouts:
//  * columns (SoA) - what the plane kernels and the per-word search of a view write: hap, pos, strand, start, stop, flags, cfdon,
//    win[5][cap]; `rows` is null;
//  * packed rows (`rows` != null; the column pointers are null) - what the cluster search of a view writes (hawk_csearch.hip):
//    ONE array of 64-byte rows, a single linear write stream.  Row i = 16 words:
//      [0] pos   [1] strand | flags << 1 | haplotype row << 9   [2] start - startp   [3] stop - start   [4,5] cfdon
//      [6 + 2 p, 7 + 2 p] window slice of plane p
//    (`startp` = genomic position of REF's base 0; haplotype rows < 2^23 and both differences within int32 are checked where the
//    rows are made).
struct GuideCols {
  uint32_t* hap;
  uint32_t* pos;
  uint8_t* strand;
  int64_t* start;
  int64_t* stop;
  uint8_t* flags;
  double* cfdon;
  uint64_t* win;  // [5][cap]
  uint64_t cap;
  uint4* rows;    // packed layout
  int64_t startp;
};
#define HAWK_ROW_HAP_SHIFT 9
#define HAWK_ROW_MAX_HAP (1u << 23)
// A stage boundary is timed by the kernel that opens the next interval: thread 0 of workgroup 0 stores the device's wall clock
// (a constant-rate counter, hipDeviceAttributeWallClockRate) into its slot of a stamp block the host reads back with the results.
// A null slot stamps nothing.  Where no kernel follows on the stream, hawk_launch_stamp queues a one-thread kernel that does it.
void hawk_launch_stamp(hipStream_t st, unsigned long long* slot);
#ifdef __HIPCC__
__device__ __forceinline__ void hawk_stamp(unsigned long long* slot) {
  if (slot && blockIdx.x == 0 && threadIdx.x == 0) *slot = wall_clock64();
}
// field access for either layout (the branch is uniform over a launch)
__device__ __forceinline__ const uint32_t* gc_roww(const GuideCols& c, uint64_t i) { return reinterpret_cast<const uint32_t*>(c.rows) + i * 16; }
__device__ __forceinline__ uint32_t gc_hap(const GuideCols& c, uint64_t i) { return c.rows ? gc_roww(c, i)[1] >> HAWK_ROW_HAP_SHIFT : c.hap[i]; }
__device__ __forceinline__ uint32_t gc_pos(const GuideCols& c, uint64_t i) { return c.rows ? gc_roww(c, i)[0] : c.pos[i]; }
__device__ __forceinline__ uint32_t gc_strand(const GuideCols& c, uint64_t i) { return c.rows ? (gc_roww(c, i)[1] & 1u) : (uint32_t)c.strand[i]; }
__device__ __forceinline__ uint32_t gc_flags(const GuideCols& c, uint64_t i) { return c.rows ? ((gc_roww(c, i)[1] >> 1) & 0xffu) : (uint32_t)c.flags[i]; }
__device__ __forceinline__ int64_t gc_start(const GuideCols& c, uint64_t i) { return c.rows ? c.startp + (int64_t)(int32_t)gc_roww(c, i)[2] : c.start[i]; }
__device__ __forceinline__ int64_t gc_stop(const GuideCols& c, uint64_t i) {
  if (!c.rows) return c.stop[i];
  const uint32_t* w = gc_roww(c, i);
  return c.startp + (int64_t)(int32_t)w[2] + (int64_t)(int32_t)w[3];
}
__device__ __forceinline__ double gc_cfdon(const GuideCols& c, uint64_t i) {
  if (!c.rows) return c.cfdon[i];
  const uint32_t* w = gc_roww(c, i);
  return __longlong_as_double((long long)((uint64_t)w[4] | ((uint64_t)w[5] << 32)));
}
__device__ __forceinline__ uint64_t gc_win(const GuideCols& c, int pl, uint64_t i) {
  if (!c.rows) return c.win[(size_t)pl * c.cap + i];
  const uint32_t* w = gc_roww(c, i);
  return (uint64_t)w[6 + 2 * pl] | ((uint64_t)w[7 + 2 * pl] << 32);
}
#endif
// columns [0, n) -> packed rows [0, n) (n read on the device: *n_dev, or n_host when n_dev is null) and back (null destination
// columns are skipped).  Packing reports HAWK_E_UNSUPPORTED through *status for a row the layout cannot hold.
void hawk_launch_rows_pack(hipStream_t st, const GuideCols& src, const uint64_t* n_dev, uint64_t n_host, uint64_t max_rows, uint4* rows, int64_t startp,
                           int* status, unsigned long long* stamp = nullptr);
void hawk_launch_rows_unpack(hipStream_t st, const uint4* rows, uint64_t n, int64_t startp, const GuideCols& dst);

struct GuideParams {
  int32_t pamlen, guidelen, right, L;
  int32_t score_cfdon;
  const double* cfd_mm;   // device, [20][4][4]
  const double* cfd_pam;  // device, [16]
  uint32_t bph;
};

// Where the REF haplotype has candidate windows, per strand (scan range and in-range test of
// REF expressed on the window start q), and the genomic position of its base 0.
struct RefInfo {
  int32_t index;
  int32_t lo[2], hi[2];
  int64_t startp;
  const uint32_t* bits[2];  // per strand: bit q set <=> REF has a candidate window starting at q (k_ref_bits); n_bits valid bits
  uint32_t n_bits;
};
// The search straight from an expansion plan (hawk_vsearch.hip): what it reads beside the rows' metadata.
struct VcArgs {
  const uint32_t* ref[4];   // REF planes A, C, G, T (ref_S words each, zero past the last base)
  uint32_t ref_S;
  const void* recs_;        // HxVar[]: one record per carried variant of every row (hawk_hx.h)
  const uint8_t* alt_codes;
  const uint64_t* hv_off;   // [n_hap + 1] record range of every row
  const void* tiles_;       // HxTile[n_hap * tiles per row]
  const uint4* hp;          // REF's PAM hits: {hit bits of word w on strand 0, hits in the words before, the same for strand 1}, w <= ref_S
};
void hawk_launch_vsearch(hipStream_t st, int pass, const HapSetDev& hs, const VcArgs& va, const ScanParams& p, const struct GuideParams& gp,
                         const struct RefInfo& ri, const TileMeta* tmeta, uint32_t* counts, uint32_t* counts0, unsigned long long* shards,
                         const uint64_t* offsets, struct GuideCols out, int* status, uint32_t tile0, uint32_t n_tiles,
                         unsigned long long* stamp = nullptr);
void hawk_launch_ref_hits(hipStream_t st, const HapSetDev& hs, const ScanParams& p, int32_t ref_index, void* hp);
// The cluster dictionary of an expansion plan (hawk_cldict.hip): every row's records cut into clusters (variants whose
// alleles lie within 64 positions of each other), identical clusters of different rows numbered once.
struct ClDict {
  uint32_t n_inst, n_uniq;
  const uint32_t* inst_uid;  // per instance, in (row, position) order: its distinct cluster, 0xffffffff for none
  const int32_t* inst_o;     // row position of the cluster's first allele
  const uint32_t* inst_row;
  const int32_t* inst_pa;    // start of the clean run in front of the instance and the REF shift in force there
  const int32_t* inst_rb;
  const uint32_t* u_rec;     // per distinct cluster: first record of the representative instance, its records, its row,
  const uint32_t* u_n;       // the row position of its first allele
  const uint32_t* u_row;
  const int32_t* u_o;
  const uint32_t* u_seg;     // a position-map segment of that row in force in front of every position a search of the cluster maps
};
size_t hawk_cs_row_bytes();
void hawk_launch_scan2_u32(hipStream_t st, const uint32_t* cnt_a, const uint32_t* cnt_b, uint32_t n, uint32_t* off_a, uint32_t* off_b,
                           const void* desc = nullptr, uint32_t* desc_bits = nullptr, uint32_t n_desc = 0);  // two arrays, one launch; beside it, if asked for:
                           // which of n_desc 64-bit words are not 0, as a bitmap of n_desc / 32 + 1 words
// hawk_cldict.hip: a build of the dictionary, pass by pass, over the views of hawk_cl.h
void hawk_launch_hx_heads(hipStream_t st, const void* recs, const uint32_t* hv_idx, uint64_t n, void* heads);  // {o, rs, alt_len, variant} per record
void hawk_launch_cl_chunks(hipStream_t st, const ClBuild& b);  // rows -> chunks: ch_off, ch_row
uint32_t hawk_cl_head_chunks(uint32_t ch_bound);  // the first chunks, whose variants the counting pass describes (0: a small job, none)
void hawk_launch_cl_count(hipStream_t st, const ClBuild& b);  // per chunk: the instances it opens (cnt), and how many of them go on the list
                          // (lcnt); the first hawk_cl_head_chunks() chunks also describe the variants they carry
void hawk_launch_cl_fill(hipStream_t st, const ClBuild& b);   // behind the scan of the counts: the instances, the list, the variants' describers
void hawk_launch_cl_finish(hipStream_t st, const ClBuild& b, const ClTable& t, const ClUniq& cu);  // the list through the table, the clusters' descriptions, the result block
void hawk_launch_cs_templates(hipStream_t st, const HapSetDev& hs, const VcArgs& va, const ClDict& cd, const ScanParams& p, const struct GuideParams& gp,
                              const struct RefInfo& ri, void* res /* 32 B per distinct cluster */, uint32_t* tbase, void* trows,
                              unsigned long long* t_count, uint64_t t_cap, int* status, unsigned long long* stamp = nullptr);
void hawk_launch_cs_count(hipStream_t st, const HapSetDev& hs, const VcArgs& va, const ClDict& cd, const ScanParams& p, const void* res,
                          const unsigned long long* t_count, uint64_t t_cap, uint32_t* group_counts, void* inst /* 16 B per instance */,
                          unsigned long long* shards, unsigned long long* stamp = nullptr);
void hawk_launch_cs_emit_rows(hipStream_t st, uint32_t n_inst, const void* inst, const void* trows, const uint64_t* offsets,
                              const unsigned long long* t_count, uint64_t t_cap, void* rows, uint64_t cap, int* status,
                              unsigned long long* stamp = nullptr);
void hawk_cs_emit_geometry(uint32_t* inst_per_wave, uint32_t* rows_per_chunk);  // of the instantiation hawk_launch_cs_emit_rows launches
// hawk_meta.hip: the rows' metadata of an expansion plan, built on the device
void hawk_launch_list_check(hipStream_t st, const uint64_t* row_off, uint32_t n_rows, const uint32_t* hv_idx, const int32_t* hv_o,
                            const int32_t* v_r0, const int32_t* v_span, const int32_t* v_chain, uint32_t n_var, uint32_t ref_len,
                            int check_clamp, uint32_t* status);
void hawk_launch_segments(hipStream_t st, const uint64_t* ioff, const uint32_t* indel, const uint32_t* hv_idx, const int32_t* hv_o,
                          const int32_t* v_r0, const int32_t* v_chain, const uint32_t* hap_len, uint32_t n_rows, int64_t startp,
                          uint32_t* seg_cnt, uint32_t* seg_off, uint32_t* seg_rel /* null: count + offsets only */, int64_t* seg_gen);
void hawk_launch_rev_lookup(hipStream_t st, const uint32_t* seg_off, const uint32_t* seg_rel, const int64_t* seg_gen, const uint32_t* hap_len,
                            uint32_t n_rows, int64_t g0, int64_t g1, int64_t* out0, int64_t* out1);
void hawk_launch_tile_meta(hipStream_t st, const uint32_t* seg_off, const uint32_t* seg_rel, const uint32_t* hap_len, const uint8_t* is_ref,
                           const int32_t* scan_start, const int32_t* scan_stop, uint32_t n_rows, uint32_t bph, TileMeta* tm);
void hawk_launch_ref_bits(hipStream_t st, const HapSetDev& hs, const ScanParams& p, const RefInfo& ri, uint32_t* bitsF, uint32_t* bitsR);

// K7 records
struct OtSite {   // one PAM-bearing genome window in guide orientation
  uint64_t code;  // base i of the window at bits 2i,2i+1 (A0 C1 G2 T3)
  uint32_t nmask; // bit i: base i is ambiguous (N / IUPAC)
  uint32_t q;     // window start inside the row | strand << 31
  uint32_t row;
  uint32_t pad;
};
struct OtHit { uint64_t site; uint32_t guide; uint32_t mm; };
// Seeds of the pigeonhole filter: the spacer is cut into max_mm + 1 blocks, so a pair within max_mm mismatches agrees
// exactly in at least one block.  Per block: its first base, the bases used as the bucket key (<= 6), where its
// bucket offsets start in `goff`, and the folded-XOR bits (even positions) of the key bases.
#define OT_MAX_BLOCKS 8
struct OtSeeds {
  int32_t nb;
  int32_t start[OT_MAX_BLOCKS], klen[OT_MAX_BLOCKS];
  uint32_t off_base[OT_MAX_BLOCKS];
  uint64_t pmask2[OT_MAX_BLOCKS];
};

// Pair seeds: the spacer cut into max_mm + 2 blocks, so a pair within max_mm mismatches agrees exactly in at least TWO of them;
// the guides are bucketed per PAIR of blocks (i < j) by the key bases of both (<= 4 each: tables of <= 4^8 buckets), which
// leaves ~4^-8 of the site x guide pairs as candidates per table instead of ~4^-4.  off_base[p]: where pair p's bucket offsets
// start in `goff`; its codes / guide ids are rows p of gcode / gid ([n_pairs][n_guides]).
#define OT_MAX_PAIRS (OT_MAX_BLOCKS * (OT_MAX_BLOCKS - 1) / 2)
struct OtPairSeeds {
  int32_t nb, n_pairs;
  int32_t start[OT_MAX_BLOCKS], klen[OT_MAX_BLOCKS];
  uint64_t pmask2[OT_MAX_BLOCKS];
  uint8_t pi[OT_MAX_PAIRS], pj[OT_MAX_PAIRS];
  uint32_t off_base[OT_MAX_PAIRS];
};
// Which match kernel a call runs and what it reads (chosen by ot_front, hawk_api_offtarget.hip): all pairs (k_ot_match: `guides`),
// single-block seeds (k_ot_match_seeded: sd + the bucketed tables goff / gcode / gid) or pair seeds (k_ot_match_pairs: ps + the
// tables).  The bulge kernels read the same sites and guides; their guidelen is the GUIDE's, this one the window scan's spacer.
enum OtMatchKind { OT_MATCH_ALL, OT_MATCH_SEEDED, OT_MATCH_PAIRS };
struct OtMatchPlan {
  OtMatchKind kind;
  OtSeeds sd;
  OtPairSeeds ps;
  const OtSite* sites;
  uint64_t n_sites;
  const uint64_t* guides;
  uint32_t n_guides;
  const uint32_t* goff;
  const uint64_t* gcode;
  const uint32_t* gid;
  int guidelen, sp0, max_mm;
};
// What the summaries' sinks share (OtSumSink, hawk_offtarget.hip; OtbSumSink, hawk_otbulge.hip): where a hit goes instead of hits[].
struct OtSumOut {
  const double* tab;             // CFD tables mm[20][4][4] + pam[16]; nullptr: counts only
  uint32_t* hist;                // [n_guides][stride], zeroed
  unsigned long long* cfd_e4;    // [n_guides], zeroed: per-guide sum of round(CFD, 4) in units of 1e-4 (two's complement)
  unsigned long long* counters;  // [0] hits, [1] hits with an ambiguous base under a CFD lookup; zeroed
  uint32_t stride;               // max_mm + 1
  OtSumOut() {}  // user-provided for the layout alone: the ABI then starts a derived struct's fields right behind `stride`
};
struct OtSumSites { const OtSite* sites; };
struct OtSummary : OtSumSites, OtSumOut {  // sites, then OtSumOut's fields
  int32_t sp0, pam2, ncmp;                 // window positions of spacer base 0 and of PAM[-2]; min(guidelen, 20)
};
struct OtBulgeSummary : OtSumOut {
  int32_t pamlen, right;
};
static_assert(sizeof(OtSummary) == 56 && sizeof(OtBulgeSummary) == 48, "kernel arguments: the layouts the sinks were compiled for");
// Bulged sites (hawk_otbulge.hip: k_ot_bulge).  `sites`: the records of a scan whose window is Gs + pamlen bases, Gs = guidelen +
// bsize (dna) or guidelen - bsize (RNA bulge); one launch per (type, size).  A row per (site, guide) whose best placement of the
// bsize gaps has <= max_mm mismatches; gaps: bit i = position i (of the site spacer for DNA bulges, of the guide for RNA bulges)
// faces nothing.  *n_hits (zeroed) counts past cap.
struct OtBulgeHit { uint64_t site; uint32_t guide, mm, gaps, pad; };

// launch wrappers
void hawk_launch_ot_onehot(hipStream_t st, uint32_t* const* plane, uint64_t nwords);
void hawk_launch_ot_sites(hipStream_t st, const HapSetDev& hs, const ScanParams& p, const uint32_t* keepF, const uint32_t* keepR,
                          const uint64_t* offsets, OtSite* sites);
// the plan's match kernel with the list sink (hits[] behind a counter that keeps counting past cap) / the summary's sink
void hawk_launch_ot_match(hipStream_t st, const OtMatchPlan& m, OtHit* hits, uint64_t cap, unsigned long long* n_hits);
void hawk_launch_ot_match_sum(hipStream_t st, const OtMatchPlan& m, const OtSummary& sm);
// the sites of the hits as a compact array; Hit = OtHit or OtBulgeHit (both begin with the site's index)
template <class Hit>
void hawk_launch_ot_gather(hipStream_t st, const OtSite* sites, const Hit* hits, uint64_t n_hits, OtSite* out);
void hawk_launch_ot_bulge(hipStream_t st, const OtSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, int guidelen,
                          int sp0, int max_mm, int dna, int bsize, OtBulgeHit* hits, uint64_t cap, unsigned long long* n_hits);
void hawk_launch_ot_bulge_sum(hipStream_t st, const OtSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, int guidelen,
                              int sp0, int max_mm, int dna, int bsize, const OtBulgeSummary& sm);
// ---- the scan over a variant-enriched genome (hawk_otvar.hip; the rule that resolves a window: hawk_otvar.h)
#include "hawk_otvar.h"
struct OvPlanes { uint32_t* p[4]; };  // the allele planes of an index: REF one-hot | ALT, the rows' geometry
struct OvSite {      // one PAM-bearing window that holds an ALT allele, in guide orientation
  uint64_t code;     // REF's bases, base i at bits 2i,2i+1 (A0 C1 G2 T3)
  uint32_t nmask;    // bit i: REF's base i is ambiguous
  uint32_t am[4];    // bit i of am[b]: base b is in the allele set of position i
  uint32_t q;        // window start inside the row | strand << 31
  uint32_t row;
  uint32_t pad;
};
struct OvHit { uint64_t code; uint32_t nmask, alt, q, row, guide, mm; };  // a variant row: the RESOLVED window, nothing to look up
static_assert(sizeof(OvSite) == 40 && sizeof(OvHit) == 32, "record layouts");
void hawk_launch_ov_fill(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const uint32_t* row, const uint32_t* q, const uint8_t* ref,
                         const uint8_t* alt, uint64_t n, uint8_t* status);
void hawk_launch_ov_filter(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const ScanParams& p, uint32_t* keepF, uint32_t* keepR,
                           uint32_t* counts);
void hawk_launch_ov_sites(hipStream_t st, const HapSetDev& hs, const OvPlanes& al, const ScanParams& p, const uint32_t* keepF,
                          const uint32_t* keepR, const uint64_t* offsets, OvSite* sites);
void hawk_launch_ov_match(hipStream_t st, const OvSite* sites, uint64_t n_sites, const uint64_t* guides, uint32_t n_guides, const OvGeom& g,
                          int max_mm, OvHit* hits, uint64_t cap, unsigned long long* n_hits);
void hawk_launch_pack(hipStream_t st, const uint8_t* ascii, const uint64_t* seq_off, uint32_t hap0, uint32_t n_hap_batch,
                      uint64_t batch_base, const uint32_t* hap_len, uint32_t S, uint32_t* const* plane,
                      unsigned long long* bad_index);
void hawk_launch_scan_raw(hipStream_t st, const HapSetDev& hs, const ScanParams& p, uint32_t* keepF, uint32_t* keepR,
                          uint32_t* counts);
void hawk_launch_emit_hits(hipStream_t st, const HapSetDev& hs, uint32_t bph, const uint32_t* keepF, const uint32_t* keepR,
                           const uint64_t* offsets, uint64_t n_fwd_total, uint32_t* hits_fwd, uint32_t* hits_rev);
void hawk_launch_search(hipStream_t st, int pass, const HapSetDev& hs, const ScanParams& p, const GuideParams& gp,
                        const RefInfo& ri, const TileMeta* tmeta, uint32_t* counts, unsigned long long* shards,
                        const uint64_t* offsets, GuideCols out, int* status, uint32_t* lists, uint32_t* big_count,
                        unsigned long long* big_list, uint32_t n_tiles = 0xffffffffu, unsigned long long* stamp = nullptr,
                        unsigned long long* stamp_mid = nullptr);  // stamp: the pass's first kernel; stamp_mid: k_search_emit (pass 1)
// ---- the collapse (hawk_collapse.hip).  These structs are host-side: the kernels keep their plain parameter lists.
struct CollapseKey {  // the rows of one table and what two of them are compared on
  GuideCols c; const uint8_t* is_ref; uint64_t n;
  int guidelen, pamlen, right, flank_up, flank_down;
  int64_t base;  // the set's smallest genomic position: the sort key holds start - base
};
// Plain device-pointer views of the set's collapse workspace (CollapseWs in hawk_host.h, which says who shares storage with whom),
// one per path.  What both hold: rocprim's scratch, the row ids, the counters and the result.
struct CollapseView {
  void* temp; size_t temp_bytes;
  uint32_t* vals;  // [2][n] sort ping-pong; the half every path's last sort writes is the result's permutation
  void* full;      // 64-byte full-key records: one per row on the exact sort path, one per group on the hash path
  // [4], zeroed by the caller.  Sort path: heads by key, heads by identity, verify mismatches.  Hash path: identity collisions,
  // rows that found no slot, groups, verify mismatches.
  unsigned long long* counters;
  uint64_t* group_off;  // n + 1 entries: the number of groups is only known afterwards
  uint8_t *gc_num, *gc_den;
};
struct CollapseSortView : CollapseView {
  uint64_t* keys;         // [2][n] sort ping-pong
  uint32_t* head_flags;   // [n]
  uint32_t* group_index;  // [n] exclusive scan of the head flags
  uint32_t* id2;          // [n] 32 further hash bits per row, read by the head pass: group_index's storage
};
struct CollapseHashView : CollapseView {
  void* table; uint32_t C;  // C slots of 16 B, a power of two
  uint32_t* occ;          // [C] stage 1: occupied slots
  uint32_t* slot_rank;    // [C] stage 2: slot -> group number, in occ's storage
  uint32_t* dense;        // [C]
  uint64_t* gkey; uint32_t* gslot;  // [2][C] each: the (key, slot) sort's ping-pong
  uint32_t* slot_of_row;  // [n]
  uint32_t* gid;          // [2][n] every row's group number: with vals the (group number, row) sort's ping-pong
};
size_t hawk_collapse_temp_bytes(uint64_t n, unsigned begin_bit, unsigned end_bit);
size_t hawk_collapse_full_bytes(uint64_t n);
size_t hawk_collapse_hash_temp_bytes(uint64_t n, uint32_t C);
size_t hawk_collapse_expand_temp_bytes(uint64_t n);
int hawk_launch_collapse(hipStream_t st, const CollapseKey& k, const CollapseSortView& v, unsigned begin_bit, unsigned end_bit, uint64_t seed,
                         bool exact /* identity by full key, not by hash */, bool weak_hash = false);
void hawk_launch_collapse_verify(hipStream_t st, const CollapseKey& k, const CollapseSortView& v);
int hawk_launch_collapse_hash1(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint64_t seed);
int hawk_launch_collapse_hash2(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint32_t G, unsigned key_end_bit);
void hawk_launch_collapse_verify_rows(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint32_t G);
int hawk_launch_collapse_expand(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint64_t G);  // reads temp, gid, vals; writes the result
void hawk_launch_rows_equal(hipStream_t st, const HapSetDev& hs, uint32_t n_pairs, const uint32_t* ra, const uint32_t* rb, uint8_t* equal);
void hawk_launch_cc_ucnt(hipStream_t st, const void* res, uint32_t nu, uint32_t* cnt);
void hawk_launch_cc_mini(hipStream_t st, const GuideCols& c, uint64_t r0, const void* trows, uint64_t t_rows, const uint64_t* moff, const uint32_t* tbase,
                         uint32_t nu, int64_t startp, GuideCols m);
void hawk_launch_cc_gidm(hipStream_t st, const uint32_t* perm, const uint64_t* goff, uint64_t nm, uint64_t G, uint32_t* gidm);
void hawk_launch_cs_gid(hipStream_t st, const ClDict& cd, const void* res, const uint64_t* moff, const uint64_t* offsets, uint64_t r0, uint64_t n,
                        const uint32_t* gidm, uint32_t* gid, uint32_t* vals);
void hawk_launch_collapse_export(hipStream_t st, const GuideCols& c, uint64_t n, uint64_t ng, const uint32_t* perm,
                                 const uint64_t* group_off, const GuideCols& rep, uint32_t* member_hap);
void hawk_launch_gt_parse(hipStream_t st, const uint8_t* text, const uint64_t* line_off, const uint64_t* gt_off, uint64_t n_lines,
                          uint32_t n_samples, uint8_t* codes, uint8_t* flags);
void hawk_launch_gt_count(hipStream_t st, const uint8_t* codes, uint32_t n_cols, const uint32_t* var_line, const uint8_t* var_allele,
                          const int32_t* var_chain, uint32_t n_var, unsigned long long* ballots, uint32_t* col_count /* [2 * n_cols] */);
void hawk_launch_gt_fill(hipStream_t st, uint32_t n_cols, const int32_t* var_r0, const int32_t* var_chain, uint32_t n_var,
                         const unsigned long long* ballots, const uint64_t* col_off, uint32_t* hv_idx, int32_t* hv_o, int64_t* col_delta,
                         const uint64_t* indel_off, uint32_t* indel_entry);
#define HAWK_LIST_CAP 512  // entries per tile in the count pass -> emit pass hand-over list (hawk_search.hip LIST_CAP)
enum { HAWK_MSCAN_ONE = 0, HAWK_MSCAN_M1_M23 = 1, HAWK_MSCAN_WIDE = 2, HAWK_MSCAN_M1_M2_M3 = 3 };  // k_mscan_one / k_mscan1 + k_mscan23 / k_mscan1w + k_mscan23w / k_mscan1, 2, 3
int hawk_mscan_route(uint64_t n, bool shards, bool aligned);
void hawk_launch_mscan(hipStream_t st, const uint32_t* counts, uint64_t n, unsigned long long* partial,
                       const unsigned long long* shards, uint64_t* offsets, ScanTotals* totals, unsigned long long* stamp = nullptr);
void hawk_launch_cfd(hipStream_t st, const char* wt, const char* sg, uint32_t len, const char* pam2, uint64_t n,
                     const double* mm, const double* pamtab, double* out, int* status);
void hawk_launch_deepcpf1(hipStream_t st, const char* seqs, uint64_t n, const float* w, float* out, int* status);
void hawk_launch_tm_nn(hipStream_t st, const char* seqs, uint32_t len, uint64_t n, double* out, int* status);
void hawk_launch_azimuth(hipStream_t st, const char* seqs, uint64_t n, uint32_t n_trees, const int32_t* tree_off,
                         const int32_t* feature, const int32_t* left, const int32_t* right, const double* threshold,
                         const double* value, double init, double lr, double* out, double* feats_out, int* status);
void hawk_launch_gbt(hipStream_t st, const double* feats, uint64_t n, uint32_t nf, uint32_t n_trees, const int32_t* tree_off,
                     const int32_t* feature, const int32_t* left, const int32_t* right, const double* threshold, const double* value,
                     double init, double lr, int cast_f32, double* out);
uint32_t hawk_hx_tiles_per_row(uint32_t S);
size_t hawk_hx_record_bytes();
size_t hawk_hx_tile_bytes();
void hawk_launch_hx_prepare(hipStream_t st, const uint64_t* hv_off, const uint32_t* hv_idx, const int32_t* hv_o, uint64_t ncar,
                            const uint32_t* v_r0, const uint32_t* v_span, const uint32_t* v_alt_off, const uint32_t* v_alt_len,
                            const void* v_am /* uint4 per variant */, const uint32_t* hap_len, uint32_t n_hap, uint32_t S, void* recs,
                            void* tiles);
void hawk_launch_hx_build(hipStream_t st, const uint32_t* const* ref, uint32_t ref_S, const void* recs, const uint8_t* alt_codes,
                          const uint64_t* hv_off, const uint32_t* hap_len, uint32_t n_hap, uint32_t S, uint32_t* const* plane,
                          const void* tiles);
void hawk_launch_hx_hash(hipStream_t st, uint32_t* const* plane, uint32_t n_hap, uint32_t S, unsigned long long* hash);
// hawk_haptext.hip: the listed rows of a plan as cased IUPAC text, row i at out + dst_off[i] (device memory, any alignment)
void hawk_launch_hx_text(hipStream_t st, const uint32_t* const* ref, uint32_t ref_S, const void* recs, const uint8_t* alt_codes,
                         const uint64_t* hv_off, const uint32_t* hap_len, uint32_t S, const void* tiles, uint32_t n_rows, const uint32_t* rows,
                         const uint64_t* dst_off, uint8_t* out);

// ---- BED annotation join (hawk_annot.hip): the features of one (file, contig, label kind), sorted by start, resident in HBM
struct AnnDev {
  const int64_t *start, *end;  // [n] 0-based half-open
  const int64_t* rmax;         // [n] max(end[0..i])
  const int64_t* bmax;         // [ceil(n / 64)] max(end) per block of 64 features
  const uint64_t* loff;        // [n + 1] label i = blob[loff[i], loff[i + 1])
  const uint8_t* blob;
  uint64_t n;
};
uint64_t hawk_ann_scan_blocks(uint64_t n);  // entries of the `partial` workspace a scan over n elements needs
void hawk_launch_ann_index(hipStream_t st, const int64_t* end, uint64_t n, int64_t* partial, int64_t* rmax, int64_t* bmax);
// off[q] <- bytes of row q; totals[0] += overlaps, totals[1] += walk steps
void hawk_launch_ann_count(hipStream_t st, const AnnDev& A, const int64_t* qs, const int64_t* qe, uint64_t nq, uint64_t* off,
                           unsigned long long* totals);
// off[nq + 1] <- exclusive 64-bit sums of off[0..nq), in place
void hawk_launch_ann_offsets(hipStream_t st, uint64_t* off, uint64_t nq, uint64_t* partial);
void hawk_launch_ann_fill(hipStream_t st, const AnnDev& A, const int64_t* qs, const int64_t* qe, uint64_t nq, const uint64_t* off, uint8_t* out);

// ---- the off-targets table as text (hawk_ottext.hip; the row itself: ot_text_row, hawk_ottext.h)
#include "hawk_ottext.h"
struct OtTextDev {
  // the hit columns, n records (device)
  const uint32_t *guide, *row, *q, *nmask;
  const uint64_t *code, *gaps;
  const uint8_t *strand, *mm, *kind, *size;
  const uint64_t* order;       // output row i = record order[i]; NULL: input order
  const uint64_t* guides2;     // the guides' 2-bit codes
  const uint32_t* row_contig;  // per genome row: contig id ...
  const uint64_t* row_off;     // ... and offset on it
  const uint8_t* names;        // contig c = names[name_off[c], name_off[c + 1])
  const uint64_t* name_off;
  const double* tab;           // mm[20][4][4] + pam[16], or NULL
  OtTextFmt fmt;
  uint64_t n;
};
// len[i] <- bytes of output row i, cfd_e4[i] <- its CFD in 1e-4 units (-1: NA or unscorable), *n_unscorable += the unscorable rows
void hawk_launch_ot_text_len(hipStream_t st, const OtTextDev& A, uint64_t* len, int64_t* cfd_e4, unsigned long long* n_unscorable);
// row i at out[off[i], off[i + 1]) (off: the exclusive sums of len, off[n] = bytes of the blob)
void hawk_launch_ot_text_fill(hipStream_t st, const OtTextDev& A, const uint64_t* off, uint8_t* out);

// ---- gnomAD sites records -> population-genotype lines (hawk_gnomad.hip; the rules themselves: hawk_gnomad.h)
#include "hawk_gnomad.h"
struct GnDev {
  const uint8_t* text;       // the batch's data lines
  const uint64_t* line_off;  // [n + 1]
  uint64_t n;
  const uint8_t* keys;       // key k = keys[key_off[k], key_off[k + 1])
  const uint32_t* key_off;   // [n_keys + 1]
  uint32_t n_keys, keep;
  // per record: what k_gn_scan writes and the text kernels read
  uint32_t* mask;
  uint8_t* flags;
  uint32_t* field_off;  // [n][8]
  uint32_t* qual_span;  // [n][2]
  uint32_t* af_span;    // [n][2]
};
void hawk_launch_gn_scan(hipStream_t st, const GnDev& G);
// kept[i] <- 1 for a record without flags, else 0 (the input of the scan that numbers the kept records)
void hawk_launch_gn_kept(hipStream_t st, const GnDev& G, uint64_t* kept);
// len[i] <- bytes of record i's output line (0 for a record with flags); kidx: the exclusive sums of kept; pool entry j =
// pool[pool_off[j], pool_off[j + 1]), QUAL of kept record k at k, its AF at n_kept + k
void hawk_launch_gn_text_len(hipStream_t st, const GnDev& G, const uint64_t* kidx, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_kept,
                             uint64_t* len);
void hawk_launch_gn_text_fill(hipStream_t st, const GnDev& G, const uint64_t* kidx, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_kept,
                              const uint64_t* off, uint8_t* out);

// ---- BGZF members -> text, one wavefront per member (hawk_inflate.hip; the rules themselves: hawk_inflate.h)
struct BzDev {
  const uint8_t* in;      // the members' bytes from c_off[0] on
  const uint64_t* c_off;  // [n + 1] as the caller gave them: member k = in[c_off[k] - c_off[0], c_off[k + 1] - c_off[0])
  const uint64_t* u_off;  // [n + 1] likewise: its text = out[u_off[k] - u_off[0], u_off[k + 1] - u_off[0])
  uint32_t n;
  uint8_t* out;
  uint8_t* status;        // [n] HAWK_BZ_*
};
void hawk_launch_bz_inflate(hipStream_t st, const BzDev& B, unsigned long long* stamp);

// ---- variant effects on the report groups (hawk_effects.hip; the rules themselves: hawk_effects.h)
#include "hawk_effects.h"
struct FxDev {
  FxCols c;  // device pointers
  // score-independent, per group (hawk_launch_fx_groups / _samples)
  uint32_t* head;
  uint8_t* type;
  uint8_t* dup;
  uint32_t* n_samples;
  uint32_t* long_list;         // groups whose sample list takes a wave; their number is counts[6]
  unsigned long long* counts;  // [8]
  // per score (hawk_launch_fx_positions)
  const double* score;
  double *rs, *delta, *abs_delta;
  uint32_t *pos_ref, *pos_nvalid, *pos_first_rank;
  double* pos_worst;
  // the selection
  const int64_t* cand_start;
  const uint8_t* cand_strand;
  uint32_t n_cand, K;
  uint32_t* chosen;     // [2 * FX_MAX_K + 1]: the candidates' heads, then the K - n_cand best others; at FX_MAX_K their valid-alternative counts; last their number
  FxEntry* part;        // [blocks][FX_MAX_K] per-workgroup candidates of the selection
  uint64_t* alt_off;    // [K + 1]
  uint32_t* alt_group;
};
// ---- unphased IUPAC windows resolved on the table (hawk_resolve.hip; the rules themselves: hawk_resolve.h)
#include "hawk_resolve.h"
struct UrDev {
  GuideCols c;              // either layout
  uint64_t n;               // rows
  const uint32_t* hap_len;  // [n_hap]
  const uint8_t* is_ref;    // [n_hap]
  uint32_t n_hap;
  UrGeom g;
  UrAlleles al;             // device pointers
  const uint64_t* ref_key;  // [n] sorted start * 2 + strand of REF's rows, UR_SAT behind them
  const uint32_t* ref_row;  // [n] the row of each key
};
size_t hawk_ur_temp_bytes(uint64_t n);
int hawk_launch_ur_refsort(hipStream_t st, const UrDev& d, void* temp, size_t temp_bytes, uint64_t* keys /* [2][n] */, uint32_t* vals /* [2][n] */);
void hawk_launch_ur_count(hipStream_t st, const UrDev& d, uint32_t* n_resolved, uint32_t* n_kept, unsigned long long* decline /* ~0 */,
                          unsigned long long* totals /* [2], zeroed */);
int hawk_launch_ur_offsets(hipStream_t st, const uint32_t* n_kept /* [n + 1], last 0 */, uint64_t n, void* temp, size_t temp_bytes, uint64_t* offsets);
void hawk_launch_ur_fill(hipStream_t st, const UrDev& d, const uint32_t* n_resolved, const uint32_t* n_kept, const uint64_t* offsets, uint64_t r0,
                         uint64_t r1, uint64_t o0, uint64_t n_out, uint32_t* out_src, uint64_t* out_win, uint64_t out_stride);

// ---- report groups of the kept guides (hawk_ugroups.hip; the rules themselves: hawk_ugroups.h)
#include "hawk_ugroups.h"
struct UgDev {
  GuideCols c;               // the table, either layout
  const uint8_t* is_ref;     // [n_hap]
  uint32_t n_hap;
  uint64_t n_rows;
  const uint64_t* ref_key;   // [n_rows] sorted start * 2 + strand of REF's rows, UR_SAT behind them
  const uint32_t* ref_row;   // [n_rows] the row of each key
  const uint32_t* row_kept;  // [n_rows] kept guides per table row
  const uint64_t* row_off;   // [n_rows + 1] first kept guide of a row
  uint64_t n;                // kept guides
  const uint32_t* src_row;   // [n]
  const uint64_t* win;       // [5][n]
  const double* cfd;         // [UG_CFD_MM + UG_CFD_PAM], or null: every CFDon is NaN
  UgGeom g;
};
struct UgWork {          // per kept guide, [n] each
  uint64_t* keyw;        // [UG_KEY_WORDS][n]
  uint64_t* hp;          // hap << 32 | pos
  double* cfdon;
  uint16_t* gc;          // num | den << 8
};
struct UgOut {           // the groups, in HBM
  uint32_t *rep_src_row, *hap, *pos;
  uint8_t *strand, *is_ref, *gc_num, *gc_den;
  int64_t *start, *stop;
  double* cfdon;
  uint64_t *win, *member_off;  // [5][n_groups], [n_groups + 1]
  uint32_t* member_hap;
  uint64_t n_groups, n_members;
};
size_t hawk_ug_temp_bytes(uint64_t n);
void hawk_launch_ug_keys(hipStream_t st, const UgDev& u, const UgWork& w, uint32_t* idx /* [n]: 0 .. n - 1 */, int* status);
// the LSD passes: (hap << 32 | pos) first, then the key words from the least significant; returns the sorted order (vals_a or vals_b), null on failure
const uint32_t* hawk_launch_ug_sort(hipStream_t st, const UgDev& u, const UgWork& w, void* temp, size_t temp_bytes, uint64_t* keys_a, uint64_t* keys_b,
                                    uint32_t* vals_a /* 0 .. n - 1 */, uint32_t* vals_b);
void hawk_launch_ug_heads(hipStream_t st, const UgWork& w, uint64_t n, const uint32_t* order, uint32_t* gflag /* [n + 1], last 0 */,
                          uint32_t* mflag /* [n + 1], last 0 */);
void hawk_launch_ug_emit(hipStream_t st, const UgDev& u, const UgWork& w, const uint32_t* order, const uint32_t* gflag, const uint32_t* mflag,
                         const uint64_t* gidx /* [n + 1] */, const uint64_t* midx /* [n + 1] */, const UgOut& o);

// ---- the whole-region rows of an unphased VCF (hawk_ubuild.hip; the rules themselves: hawk_ubuild.h)
#include "hawk_ubuild.h"
struct UbLists {             // device pointers
  uint32_t n_samples, n_var;
  const uint64_t* off;       // [n_samples + 1] CSR of the per-sample carried lists
  const uint32_t* idx;       // ascending variant indices
  const uint32_t* var_off;   // [n_var] offset in the region, ascending
  const uint8_t* var_mask;   // [n_var] the alt's 4-bit mask
  const uint8_t* var_ref;    // [n_var] the ref base 0-3
};
void hawk_launch_gt_parse_unphased(hipStream_t st, const uint8_t* text, const uint64_t* line_off, const uint64_t* gt_off, uint64_t n_lines,
                                   uint32_t n_samples, uint8_t* codes, uint8_t* flags);
void hawk_launch_ub_count(hipStream_t st, const uint8_t* codes, uint32_t n_samples, const uint32_t* var_line, const uint8_t* var_allele,
                          uint32_t n_var, unsigned long long* ballots, uint32_t* count /* [n_samples] */);
void hawk_launch_ub_fill(hipStream_t st, uint32_t n_samples, uint32_t n_var, const unsigned long long* ballots, const uint64_t* off, uint32_t* idx);
void hawk_launch_ub_sig(hipStream_t st, const UbLists& l, unsigned long long* sig /* [n_samples][2] */, unsigned long long* decline /* ~0 */);
void hawk_launch_ub_rows(hipStream_t st, uint32_t* const* plane, uint32_t S, uint32_t ref_row, uint32_t first_row, uint32_t n_rows,
                         const uint32_t* row_sample, const UbLists& l, unsigned long long* decline /* ~0 */);

// ---- the indel-window rows of an unphased VCF (hawk_uwin.hip; the rules themselves: hawk_uwin.h)
#include "hawk_uwin.h"
struct UwDev {                  // device pointers
  uint32_t n_indel, n_samples, L;
  uint64_t n_inst;
  const uint32_t* line;         // [n_indel] the record of each indel allele, in (record, allele) order
  const uint8_t* allele;        // [n_indel] its allele number
  const uint32_t* off;          // [n_indel] its normalised offset in the region
  const uint32_t *ref_len, *alt_len;
  const uint32_t* pool_off;     // [n_indel] where its ref bases, then its alt bases, start in `pool`
  const uint8_t* pool;          // ub_base_index of every base
  const uint32_t* rank_sample;  // [n_samples] the sample columns in the order of their sorted names
  const uint8_t* ref;           // [L] REF's bytes
  const uint64_t* inst_off;     // [n_indel + 1] CSR of the instances
  uint32_t *inst_indel, *inst_sample;
  uint64_t *inst_lo, *inst_hi;  // the carrier's list entries inside the window
};
void hawk_launch_uw_count(hipStream_t st, const uint8_t* codes, const UwDev& d, unsigned long long* ballots, uint32_t* count /* [n_indel] */,
                          unsigned long long* decline /* ~0; indel << 8 | reason */);
void hawk_launch_uw_instances(hipStream_t st, const UwDev& d, const UbLists& l, const unsigned long long* ballots);
void hawk_launch_uw_sig(hipStream_t st, const UwDev& d, const UbLists& l, unsigned long long* sig /* [n_inst][2] */, unsigned long long* decline);
void hawk_launch_uw_group(hipStream_t st, const UwDev& d, const UbLists& l, const unsigned long long* sig, uint32_t* head /* [n_inst] */);
void hawk_launch_uw_fill(hipStream_t st, uint32_t* const* plane, uint32_t S, uint32_t ref_row, uint32_t first_row, uint32_t n_rows,
                         uint32_t qpr /* threads per row */, const uint32_t* row_inst, const UwDev& d, const UbLists& l);

#define FX_TOPK_MAX_BLOCKS 1024u
void hawk_launch_fx_isref_gather(hipStream_t st, const uint8_t* hap_is_ref, const uint32_t* member_hap, const uint64_t* member_off, uint64_t n_groups, uint8_t* out);
void hawk_launch_fx_groups(hipStream_t st, const FxDev& F);
void hawk_launch_fx_samples(hipStream_t st, const FxDev& F);
void hawk_launch_fx_positions(hipStream_t st, const FxDev& F, int family);
uint32_t hawk_fx_topk_blocks(uint64_t n_groups);
void hawk_launch_fx_topk(hipStream_t st, const FxDev& F, int family);
void hawk_launch_fx_alts(hipStream_t st, const FxDev& F, int family, uint32_t n_chosen);
