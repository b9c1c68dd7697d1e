/*
 * hawk.h — C ABI of libhawk_hip.so: the MI355X (gfx950) implementation of CRISPR-HAWK's
 * variant-aware guide search hot path.
 *
 * The reference (pinellolab/CRISPR-HAWK) has no FFI layer: its hot path is a chain of plain
 * Python call sites in crisprhawk_search() (crisprhawk.py:121-138).  Each entry point below
 * names the reference call it replaces; INTEGRATION.md shows the ctypes binding a maintainer
 * would add on the reference side.  Conventions: plain pointers and sizes, no C++/torch types;
 * every function returns HAWK_OK (0) or a negative hawk_status and never throws; outputs are
 * caller-allocated with an explicit capacity, or stay resident in HBM behind an opaque handle
 * until downloaded; one hawk_ctx per process per device; not fork-safe (a HIP context does
 * not survive fork — the reference's ProcessPoolExecutor scorers, scoring.py:129, must call
 * from the parent).
 *
 * Data layout in HBM: a haplotype set is five bit-planes
 * A, C, G, T (the four bits of the reference's IUPAC nibble, encoder.py:18-34) and V
 * ("this base came from a variant" = lower case in the reference's haplotype strings),
 * one bit per base, 32 bases per little-endian 32-bit word, rows padded to a common
 * 16-byte-aligned stride.
 */
#ifndef HAWK_H
#define HAWK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HAWK_OK = 0,
  HAWK_E_INVALID = -1,    /* bad argument */
  HAWK_E_HIP = -2,        /* HIP runtime failure (hawk_last_hip_error() has the text) */
  HAWK_E_CAPACITY = -3,   /* caller buffer too small; required size is reported */
  HAWK_E_IUPAC = -4,      /* non-IUPAC character: CrisprHawkIupacTableError (encoder.py:37-45) */
  HAWK_E_CFD = -5,        /* non-ACGT base under a CFD lookup: CrisprHawkCfdScoreError (cfdscore.py:93-94) */
  HAWK_E_NODEVICE = -6,   /* no gfx950 device visible */
  HAWK_E_UNSUPPORTED = -7, /* parameter outside the kernel's range (e.g. guidelen+pamlen > 44) */
  HAWK_E_COMM = -8,        /* RCCL failure or librccl.so missing (hawk_comm_last_error() has the text) */
  HAWK_E_OVERLAP = -9,     /* a chromosome copy carries overlapping variants (haplotype.py:214-252 raises on them) */
  HAWK_E_CLAMP = -10,      /* an indel reaches past the region's original length (the reference's clamp, haplotype.py:199-201) */
  HAWK_E_OOM = -11         /* device memory the allocator cannot give (hawk_resolve_groups) */
} hawk_status;

typedef struct hawk_ctx hawk_ctx;
typedef struct hawk_hapset hawk_hapset;
typedef struct hawk_table hawk_table;

#define HAWK_GUIDESEQPAD 10 /* guide.py:21 */
#define HAWK_MAX_CORE 44    /* guidelen + pamlen limit: the 20-nt padded window must fit 64 bits */

/* ---- context -----------------------------------------------------------------------
 * One context = one HIP stream per device and process.  hawk_init for a device that already has a context returns that
 * same context (reference-counted; the last hawk_destroy releases it): the library serves device memory from a caching
 * allocator whose reuse of freed blocks is ordered by that single stream. */
int hawk_device_count(int* n);
int hawk_init(int device, hawk_ctx** out);
void hawk_destroy(hawk_ctx* ctx);
const char* hawk_strerror(int status);
const char* hawk_last_hip_error(void);
/* the hipStream_t all of this context's work is enqueued on (for external event timing) */
void* hawk_stream(hawk_ctx* ctx);
int hawk_sync(hawk_ctx* ctx);
/* Device memory is served by a caching allocator (freed planes / columns / workspaces are reused by the next
 * haplotype set of the same shape, e.g. the next tile of a whole-contig search); this returns the cache to HIP. */
int hawk_release_cached_memory(hawk_ctx* ctx);
/* Page-locked host memory for buffers a download writes into (hawk_table_download, hawk_table_collapse_export ...): the copy
 * then runs at link speed.  Plain host memory is accepted everywhere; this is an optimisation for large results. */
int hawk_host_alloc(hawk_ctx* ctx, uint64_t bytes, void** out);
void hawk_host_free(void* p);

/* ---- haplotype set: replaces encode() per haplotype (crisprhawk.py:64-81, encoder.py:48-57)
 * plus the Haplotype fields the search reads (haplotype.py:395-491) ---------------------- */

/* Allocate planes for n_hap haplotypes of the given lengths (bases). */
int hawk_hapset_create(hawk_ctx* ctx, uint32_t n_hap, const uint32_t* hap_len, hawk_hapset** out);
void hawk_hapset_destroy(hawk_hapset* hs);

/* K1: pack cased ASCII haplotypes (host memory, concatenated, seq_off[n_hap+1] byte offsets)
 * into the planes.  Upper/lower case is data: lower case sets the V plane.  On a non-IUPAC
 * character returns HAWK_E_IUPAC and *bad_index = its offset in `seqs` (encoder.py:37-45). */
int hawk_hapset_pack_ascii(hawk_hapset* hs, const char* seqs, const uint64_t* seq_off, uint64_t* bad_index);

/* Per-haplotype metadata the search needs:
 *   is_ref[h]      1 iff haplotype.samples == "REF" (search_guides.py:468-471)
 *   scan_start/stop  compute_scan_start_stop() (search_guides.py:49-84), relative positions
 *   seg_off[n_hap+1], seg_rel[], seg_gen[]  the haplotype position map (haplotype.py:90-159)
 *     as unit-slope segments: posmap[rel] = seg_gen[k] + (rel - seg_rel[k]) for the last k in
 *     [seg_off[h], seg_off[h+1]) with seg_rel[k] <= rel.
 *   ref_index      index of the REF haplotype, or -1 */
int hawk_hapset_set_meta(hawk_hapset* hs, const uint8_t* is_ref, const int32_t* scan_start, const int32_t* scan_stop,
                         const uint32_t* seg_off, const uint32_t* seg_rel, const int64_t* seg_gen, int32_t ref_index);

/* Tiles of a larger region (region-tiled whole-contig search): a haplotype row is grouped with the REF guide at its
 * (start, strand) (remove_redundant_guides, search_guides.py:340-369; CFDon's wild type, scoring.py:368-381) wherever in
 * the REGION that guide's PAM lies, while this set's REF row only scans the tile it owns.  [start, stop) is the
 * region's scan range (compute_scan_start_stop) in the REF row's relative positions, clipped to the row; default =
 * REF's own scan range.  Call after hawk_hapset_set_meta. */
int hawk_hapset_set_ref_partner_range(hawk_hapset* hs, int32_t start, int32_t stop);

/* Row stride in 32-bit words, and a copy of one plane (0..4 = A,C,G,T,V) to host
 * (n_hap * stride words) — for tests and for decoding windows on the host. */
int hawk_hapset_stride(const hawk_hapset* hs, uint32_t* stride_words);
int hawk_hapset_download_plane(hawk_hapset* hs, int plane, uint32_t* out_words);
/* equal[i] = 1 iff rows rows_a[i] and rows_b[i] hold the same bases, case included (all five planes compared): what makes
 * collapsing haplotypes on their 128-bit content hash (hawk_xplan_run's hash_out; haplotypes.py:274-294 compares the
 * strings) exact - the caller checks every row it is about to alias onto another. */
int hawk_hapset_rows_equal(hawk_hapset* hs, uint32_t n_pairs, const uint32_t* rows_a, const uint32_t* rows_b, uint8_t* equal);
/* Upload planes computed elsewhere (5 * n_hap * stride words, plane-major). */
int hawk_hapset_upload_planes(hawk_hapset* hs, const uint32_t* planes);

/* ---- haplotype expansion on the device, replacing Haplotype.add_variants_phased
 * (haplotype.py:214-252) per chromosome copy, as a reusable plan whose inputs stay in HBM.  ref_set: a one-row hapset
 * holding the REF region (the plan copies its planes, so ref_set may be destroyed).  Variant table (sorted by position):
 * v_r0 = position in the region, v_span = REF bases replaced (SNV 1, deletion len(ref), insertion 1), alt allele =
 * v_alt_len IUPAC codes (encoder.py nibbles, one per byte) at alt_codes + v_alt_off, v_chain[i] = alt_len - span.  Alt
 * bases are written with the V plane set, exactly as the reference lower-cases them.
 * Plan creation straight from the genotype inversion: `g` is a hawk_gt after hawk_gt_lists, whose carried-variant lists
 * are still in HBM - they are used in place (rows = REF + every chromosome copy with a non-empty list, in column order),
 * nothing is downloaded, and what the host used to do over every list entry runs as kernels: the ascending /
 * non-overlapping check (HAWK_E_OVERLAP), the reference's end-of-region clamp for indels when check_clamp != 0
 * (HAWK_E_CLAMP), the position-map segments of every row (haplotype.py:90-159) and posmap_rev at the two genomic positions
 * rev_g0 / rev_g1 the scan bounds start from (search_guides.py:49-84).  hawk_xplan_rows returns the rows' lengths and
 * the two look-ups (-1: the position is deleted from that row); the caller turns them into scan ranges (rows collapsed
 * onto another get an empty one) and hawk_xplan_finish_meta builds the per-tile records.
 * hawk_xplan_segments downloads the segments (for labels / reports); hawk_xplan_install_meta gives a set hawk_xplan_run
 * wrote BEFORE the metadata existed (the run whose hashes decide which rows collapse) the finished metadata.
 * hawk_xplan_set_ref_partner_range: hawk_hapset_set_ref_partner_range for every set the plan installs its metadata into.
 * hawk_xplan_run writes a fresh haplotype set from the plan with device work only: what the region-tiling loop of a
 * whole-contig search (search_guides.py:510-548 over one 50 Mb region; here one tile at a time inside a fixed HBM
 * budget) runs per tile.  hash_out (optional, 2 words per row): content hash for collapse_haplotypes
 * (haplotypes.py:274-294).  hash_out / kernel_ms may be NULL (then the run is asynchronous on the context's stream). */
typedef struct hawk_xplan hawk_xplan;
typedef struct hawk_gt hawk_gt;
int hawk_xplan_create_gt(hawk_hapset* ref_set, hawk_gt* g, uint32_t n_var, const uint32_t* v_r0, const uint32_t* v_span,
                         const uint32_t* v_alt_off, const uint32_t* v_alt_len, const int32_t* v_chain, const uint8_t* alt_codes,
                         uint32_t alt_codes_len, int64_t startp, int check_clamp, int64_t rev_g0, int64_t rev_g1, uint32_t* n_hap_out,
                         hawk_xplan** out);
int hawk_xplan_rows(hawk_xplan* x, uint32_t* hap_len, int64_t* rev0, int64_t* rev1);
int hawk_xplan_finish_meta(hawk_xplan* x, const int32_t* scan_start, const int32_t* scan_stop);
int hawk_xplan_segments(hawk_xplan* x, uint32_t* seg_off, uint32_t* seg_rel, int64_t* seg_gen, uint64_t cap, uint64_t* n_seg);
int hawk_xplan_install_meta(hawk_xplan* x, hawk_hapset* hs);
int hawk_xplan_set_ref_partner_range(hawk_xplan* x, int32_t start, int32_t stop);
int hawk_xplan_run(hawk_xplan* x, hawk_hapset** out, uint64_t* hash_out, float* kernel_ms);
void hawk_xplan_destroy(hawk_xplan* x);
/* The rows of a plan as text: the `haplotype` column of the reference's haplotypes_table (haplotypes.py:818-859, written by
 * `search --haplotype-table`) - the cased IUPAC string of a haplotype, alt bases in lower case - without planes in HBM and
 * without a decode on the host (crispr-hawk_amd/csrc/hawk_haptext.hip: the words the expansion would write, turned into
 * letters).  rows: n_rows row indices of the plan, in any order, repeats allowed.  Row i of the call is written to
 * out[out_off[i] .. out_off[i + 1]) (host memory; page-locked memory copies fastest; no alignment is asked of the offsets) and
 * is exactly as long as hawk_xplan_rows reports for it; no other byte of `out` is written.  HAWK_E_INVALID, with nothing
 * written, when a row index is >= the plan's rows, when out_off[i + 1] - out_off[i] is not that row's length, or when out_off
 * is not ascending.  n_rows == 0 is HAWK_OK.  The device image of the call's rows (out_off[n_rows] - out_off[0] bytes) comes
 * from the library's caching allocator: callers with many long rows call in batches of whole rows.  The plan is only read: a
 * search of its view gives the same table before and after.  kernel_ms may be NULL. */
int hawk_xplan_text(hawk_xplan* x, uint32_t n_rows, const uint32_t* rows, const uint64_t* out_off, char* out, float* kernel_ms);
/* A VIEW of the plan's rows: a haplotype set with the plan's metadata (hawk_xplan_finish_meta must have been called, REF =
 * row 0) but WITHOUT planes.  hawk_search on a view computes the same table, totals and row order as on the set hawk_xplan_run
 * writes - encode (encoder.py:48-57 over every haplotype) and search (search_guides.py:510-548) in one step, straight from
 * REF + the rows' variant records: windows without a variant base are dropped by the reference (search_guides.py:468-471),
 * so only the words around a row's variants are assembled (in registers) and matched; the PAM hits of the verbatim REF
 * stretches in between, which only the totals count, come from prefix counts over REF's own hits.  Everything that reads
 * planes (hawk_pam_scan, hawk_hapset_download_plane, hawk_offtarget_scan ...) returns HAWK_E_INVALID on a view; tables,
 * collapse, export and gather work as on any set.  The plan must outlive the view. */
int hawk_xplan_view(hawk_xplan* x, hawk_hapset** out);
/* The cluster dictionary hawk_xplan_view builds for a plan (crispr-hawk_amd/csrc/hawk_cldict.hip): a row's carried variants
 * fall into clusters (alleles within 64 positions of each other - the reach of one padded guide window); a cluster carried by
 * many chromosome copies is searched ONCE per hawk_search and its rows copied to every carrier.  usable = 0: the plan is
 * searched per row instead (status 1: a chain of more than 4096 variants, 2: two different clusters with one hash, 4: too
 * little sharing - fewer than HAWK_CLUSTER_MIN_SHARE (3) instances per distinct cluster - or more than
 * HAWK_CLUSTER_MAX_SLOTS (2^27) template rows).  Same table either way, up to the order of a haplotype's rows.
 * No reference counterpart: the reference searches every haplotype string on its own (search_guides.py:510-548). */
int hawk_xplan_cluster_stats(const hawk_xplan* x, uint32_t* usable, uint32_t* n_instances, uint32_t* n_distinct, uint64_t* template_slots,
                             float* build_ms, uint32_t* status);
/* Builds the dictionary again from the plan's records (same result; buffers reused).  What bench.py calls inside its timed
 * step so that `value` carries the dictionary's cost: the product builds one per plan and searches it once (pipeline.search_files). */
int hawk_xplan_cluster_rebuild(hawk_xplan* x);

/* ---- K2: pam_search() (search_guides.py:102-131) ---------------------------------------
 * Raw PAM hits of every haplotype inside its [scan_start, scan_stop): ascending relative
 * positions per haplotype, forward-PAM hits in hits_fwd and reverse-complement-PAM hits in
 * hits_rev, haplotype h occupying [off_fwd[h], off_fwd[h+1]) (off arrays have n_hap+1
 * entries).  pam_fwd/pam_rev are PAM.bits / PAM.bitsrc (pam.py:127-141). */
int hawk_pam_scan(hawk_hapset* hs, uint64_t pam_fwd, uint64_t pam_rev, uint32_t pamlen, uint32_t* hits_fwd,
                  uint32_t* hits_rev, uint64_t cap_fwd, uint64_t cap_rev, uint64_t* off_fwd, uint64_t* off_rev);

/* Average duration (HIP events on the context stream) of the K2 PAM-scan kernel alone over `reps`
 * back-to-back launches on this set: plane codes in, one forward and one reverse hit bit per position
 * out - the kernel SURVEY.md §8(d) prices at 0.75 B per scanned position. */
int hawk_pam_scan_time(hawk_hapset* hs, uint64_t pam_fwd, uint64_t pam_rev, uint32_t pamlen, uint32_t reps, float* avg_ms,
                       uint64_t* scanned_positions);

/* ---- fused search: search() (search_guides.py:510-548) + the CFDon slice of
 * scoring_guides() (scoring.py:352-387, after annotation.reverse_guides) ------------------- */
typedef struct {
  uint64_t pam_fwd, pam_rev; /* PAM.bits, PAM.bitsrc */
  uint32_t pamlen, guidelen;
  uint32_t right;            /* --right: guide downstream of the PAM (Cpf1-like) */
  uint32_t score_cfdon;      /* 1: compute CFDon for every kept guide (needs right == 0); a non-ACGT base under a
                                table lookup is HAWK_E_CFD, as the reference's KeyError (cfdscore.py:93-94).
                                2: the same, but such a guide scores NaN ("NA") - the opt-in for regions with N runs */
  const double* cfd_mm;      /* [20][4][4]: position, wildtype RNA base A,C,G,U, sgRNA base A,C,G,T */
  const double* cfd_pam;     /* [16]: PAM[-2:] dinucleotide, 4*b0+b1 over A,C,G,T */
} hawk_search_params;

typedef struct {          /* kernel times of the last hawk_search (HIP events on the ctx stream), ms.  A cluster search of a plan view
                             (v_path 2) runs the REF row's plane kernels on a second stream beside the cluster kernels: the intervals
                             below are the main stream's, and the waits for REF's kernels fall into offsets_ms and emit_ms */
  float count_ms;   /* k_search_count: scan + filters + redundancy classification -> tile counts + hand-over lists */
  float offsets_ms; /* k_mscan1-3: tile counts -> row offsets */
  float emit_ms;    /* k_emit_list + k_search_emit: finished rows (coordinates, windows, CFDon) */
  float total_ms;   /* first kernel start to last kernel end, including the host round trip for the row count */
  uint64_t scanned_positions; /* sum over haplotypes of (scan_stop - scan_start) */
  float emit_list_ms; /* k_emit_list alone (0 when the hand-over lists are switched off) */
  float v_count_ms;   /* a plan view (hawk_xplan_view): its count side alone (v_path 1: k_vsearch<0>; 2: k_cs_templates + k_cs_count) -
                         count_ms also holds the REF row's plane kernel (v_path 1; v_path 2 runs it beside them: the same interval) */
  float v_emit_ms;    /* ... its emit side alone (k_vsearch<1> / k_rows_pack + k_cs_emit_rows) */
  float v_templates_ms; /* the cluster path of a view: k_cs_templates alone (v_count_ms: templates + k_cs_count) */
  uint32_t v_path;    /* 0: planes, 1: a view searched per dirty word (k_vsearch), 2: a view searched per distinct cluster (hawk_csearch.hip) */
  float v_emit_rows_ms; /* the cluster path: k_cs_emit_rows, the main stream's one emit kernel (= emit_ms; v_emit_ms begins on the second
                           stream, where k_rows_pack packs REF's staged rows) */
  float reserved;
} hawk_timing;

/* Runs the whole device pipeline; the guide table stays in HBM. `timing` may be NULL. */
int hawk_search(hawk_hapset* hs, const hawk_search_params* p, hawk_table** out, hawk_timing* timing);
void hawk_table_destroy(hawk_table* t);
/* n_rows: guides after remove_redundant_guides; n_candidates: PAM hits passing
 * is_pamhit_in_range (the bench metric's unit); n_hits: all PAM hits in scan range. */
int hawk_table_counts(const hawk_table* t, uint64_t* n_rows, uint64_t* n_candidates, uint64_t* n_hits);
/* Column download (each array n_rows long; any pointer may be NULL; destinations may be host or
 * device memory - the copy kind is inferred, so a table can be exported into buffers a
 * collective library owns without a host bounce).  Rows are haplotype-major; within a haplotype they are ordered by
 * (32 768-position tile, strand, position) - the plane kernels emit tile by tile - or, for a plan view searched per
 * distinct variant cluster (hawk_timing.v_path == 2), by (cluster along the row, strand, position);
 * sorting by (haplotype, strand, position) gives the reference's pre-dedup emission order either way.
 * Lifetime: the columns live in the haplotype set's workspace.  The next hawk_search (or hawk_hapset_set_meta) on
 * the same set overwrites them; from then on every call below on the older table returns HAWK_E_INVALID.
 *   pos: relative PAM position (what retrieve_guides iterates), start/stop: genomic
 *   (search_guides.py:260-280), strand 0/1, flags bit0 = a REF guide shares (start,strand),
 *   cfdon: NaN when no REF guide shares the key, win[5][n_rows]: bits [pos_window) of planes
 *   A,C,G,T,V for the guidelen+pamlen+20-nt window, bit 0 = leftmost base. */
int hawk_table_download(hawk_table* t, uint32_t* hap, uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* stop,
                        uint8_t* flags, double* cfdon, uint64_t* win);
/* Layout of a table in HBM.  The plane kernels and the per-word search of a view write COLUMNS (the arrays above); the cluster
 * search of a plan view (hawk_timing.v_path == 2) writes PACKED ROWS: one array of 64-byte rows, a single linear write stream,
 *   word 0 pos | 1 strand + (flags << 1) + (haplotype row << 9) | 2 start - startp | 3 stop - start | 4-5 cfdon | 6 + 2p, 7 + 2p
 *   window slice of plane p (little-endian 32-bit words; startp = genomic position of the region string's base 0).
 * hawk_table_download hands out columns whichever layout the table has (a packed table is cut into the asked-for columns on the
 * device first); hawk_table_download_rows / hawk_table_device_rows give the packed rows as they lie (HAWK_E_UNSUPPORTED on a
 * columnar table), hawk_table_device_columns the column pointers (HAWK_E_UNSUPPORTED on a packed table). */
#define HAWK_LAYOUT_COLUMNS 0u
#define HAWK_LAYOUT_ROWS 1u
int hawk_table_layout(const hawk_table* t, uint32_t* layout, int64_t* startp);
int hawk_table_download_rows(hawk_table* t, void* rows64 /* n_rows x 64 bytes, host or device */);
int hawk_table_device_rows(hawk_table* t, void** rows64, int64_t* startp);
/* Device pointers of the same columns (valid until the next hawk_search on the same set);
 * plane p of the window slices starts at win + p * win_plane_stride (in uint64 elements). */
int hawk_table_device_columns(hawk_table* t, void** hap, void** pos, void** strand, void** start, void** stop,
                              void** flags, void** cfdon, void** win, uint64_t* win_plane_stride);

/* ---- f2: which rows the guide report merges.  Replaces the pandas groupby of
 * `_collapse_report_entries` (reports.py:958-1008; group columns chr, start, stop, sgRNA_sequence, pam,
 * strand, scores, gc_content, origin): two rows merge iff they agree in start, stop, strand, origin
 * (REF haplotype or not) and in the case-preserving spacer+PAM; scores and GC are functions of those.
 * hawk_table_collapse sorts and groups in HBM (results stay in the set's workspace until the next
 * search or collapse); hawk_table_collapse_download copies them out (host or device destinations,
 * any pointer may be NULL):
 *   perm[n_rows]         row indices ordered by (start, strand, group); rows of one group are contiguous
 *                        and keep table order (haplotype ascending)
 *   group_off[n_groups+1] CSR offsets into perm
 *   gc_num, gc_den[n_groups]  G/C/S and A/C/G/T/S/W base counts of the group's spacer: gc_content =
 *                        gc_num / gc_den (annotation.py:513-541 -> Biopython gc_fraction, ambiguous bases dropped)
 * Rows of one (start, strand) are told apart by 63 bits of a hash of everything compared (a false merge needs a 63-bit
 * collision inside one (start, strand): ~1e-12 over a whole-chromosome run); with HAWK_COLLAPSE_EXACT=1 in the
 * environment (read per call) the full keys are compared instead; that path's cost is unmeasured.
 * Any number of different rows may share one (start, strand): when they collide in the key's hash bits under every seed the
 * usual path tries (thousands of different rows under one start), the call answers through the exact path, which orders the
 * rows of one key by identity and needs no collision-free key.  HAWK_E_UNSUPPORTED is left for more than 2^32 - 1 rows, for a
 * position-map range max - min above 0xffffffff, and for a flank above the 10 stored bases. */
int hawk_table_collapse(hawk_table* t, uint64_t* n_groups, float* kernel_ms);
int hawk_table_collapse_download(hawk_table* t, uint32_t* perm, uint64_t* group_off, uint8_t* gc_num, uint8_t* gc_den);
/* The same grouping with the compared sequence widened by flank_up bases 5' and flank_down bases 3' of the guide (as it
 * reads after annotation.reverse_guides): 4 / 3 is the k-mer the model scorers see (scoring.py:50-67), so with Azimuth
 * or DeepCpf1 switched on rows that differ only in those flanks - and may score differently - stay separate, as the
 * reference's groupby over the score columns keeps them (reports.py:978-1003). */
int hawk_table_collapse_ex(hawk_table* t, uint32_t flank_up, uint32_t flank_down, uint64_t* n_groups, float* kernel_ms);
/* Group-level export after a collapse: per group its first member in table order (rep_row = that row's index, and the
 * row's columns: pos, strand, start, stop, flags, cfdon, win[5][n_groups]) and, for every row in group order (CSR by
 * group_off), the haplotype it came from (member_hap[n_rows]) - what the report needs (74 B per report row + 4 B per
 * guide row) without downloading the table. */
int hawk_table_collapse_export(hawk_table* t, uint32_t* rep_row, uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* stop,
                               uint8_t* flags, double* cfdon, uint64_t* win, uint32_t* member_hap, float* kernel_ms);

/* Host-side helper of the report assembly: which of its haplotype's variants a guide SHOWS - annotation.polish_guide_variants
 * (annotation.py:185-284) - for many rows at once (the rows with an indel among their candidate variants; all-SNV rows are answered
 * in bulk by the caller).  Row k: cores[k] = the + strand spacer + PAM (L cased bytes), hap[k] its haplotype row whose position map
 * is segments [seg_start[h], seg_start[h + 1]) of (seg_rel, seg_gen), pivot[k] the guide's first position in the row, stop[k] its
 * genomic stop, cand_var[cand_off[k] .. cand_off[k + 1]) the candidate variants (ascending indices, no duplicates).  Variant v:
 * adjusted position t_pos[v], alleles in the ref / alt pools, name_rank[v] = rank of its id in string order.  out_var (capacity
 * cand_off[n]) receives per row the variants shown, in id order, out_off their CSR offsets; need_python[k] = 1 where the
 * reference's own assertion (annotation.py:185-189) would fire - the caller's Python mirror then raises as the reference does. */
int hawk_host_polish_rows(uint64_t n, uint32_t L, const uint8_t* cores, const uint32_t* hap, const int64_t* pivot, const int64_t* stop,
                          const uint64_t* cand_off, const uint32_t* cand_var, const uint64_t* seg_start, const uint32_t* seg_rel,
                          const int64_t* seg_gen, uint64_t n_haps, const int64_t* t_pos, const uint8_t* ref_pool, const uint64_t* ref_off,
                          const uint8_t* alt_pool, const uint64_t* alt_off, uint32_t n_var, const uint32_t* name_rank, uint64_t* out_off,
                          uint32_t* out_var, uint8_t* need_python);

/* The same for EVERY alt row of a report, candidates found here as well (annotation.py:246-284: the variants of the guide's haplotype
 * whose adjusted position lies in [start, max(stop, start + L)]).  Haplotype row h lists its variants - indices into the variant
 * table - at var_idx[var_off[h] .. var_off[h + 1]), ascending by position.  hawk_host_variant_window: per row k the window
 * [first[k], first[k] + count[k]) of its haplotype's list with p_lo[k] <= position <= p_hi[k]  (HAWK_E_UNSUPPORTED when a list is not in
 * position order: the caller keeps its own route).  hawk_host_polish_windows: hawk_host_polish_rows with row k's candidates read from
 * var_idx[first[k] ..), cand_off[k + 1] - cand_off[k] of them (sorted and made unique here); out_var has capacity cand_off[n]. */
int hawk_host_variant_window(uint64_t n, const uint32_t* hap, const int64_t* p_lo, const int64_t* p_hi, const uint64_t* var_off,
                             const int64_t* var_idx, const int64_t* t_pos, uint64_t n_haps, uint32_t n_var, uint64_t* first, uint32_t* count);
int hawk_host_polish_windows(uint64_t n, uint32_t L, const uint8_t* cores, const uint32_t* hap, const int64_t* pivot, const int64_t* stop,
                             const uint64_t* first, const uint64_t* cand_off, const int64_t* var_idx, uint64_t n_idx, const uint64_t* seg_start,
                             const uint32_t* seg_rel, const int64_t* seg_gen, uint64_t n_haps, const int64_t* t_pos, const uint8_t* ref_pool,
                             const uint64_t* ref_off, const uint8_t* alt_pool, const uint64_t* alt_off, uint32_t n_var, const uint32_t* name_rank,
                             uint64_t* out_off, uint32_t* out_var, uint8_t* need_python);

/* The line index of a VCF text held in (mapped) memory - replaces the streaming index pass of readers.VCF (variant.py:622-708: the
 * reference opens the file through pysam / tabix): per line its start, POS (-1 header or empty line, -2 malformed record), where
 * the sample columns begin (0: fewer than nine tabs) and the length of its CHROM field; line_start has n_lines + 1 entries.  The
 * text must end with a newline.  HAWK_E_CAPACITY (only *n_lines written) when cap < lines.  Multi-threaded, no device work. */
int hawk_host_vcf_index(const uint8_t* text, uint64_t len, uint64_t cap, uint64_t* line_start, int64_t* pos, uint64_t* gt_off,
                        uint32_t* chrom_len, uint64_t* n_lines, uint32_t* multi_contig);

/* The guide report written as TSV text straight to its file (what _store_report does with DataFrame.to_csv(sep="\t", index=False),
 * reports.py:739) from COLUMNS as the assembly keeps them, so that no row string and no text column ever exists in Python - a C3
 * report is 0.64 GB of text.  Output row i is source row order[i] (order == NULL: i), fields separated by tabs, rows ended by a
 * newline; `header` (with its newline) goes first.  The caller guarantees that no field holds a tab, quote or line break (csv's
 * minimal quoting would then apply; reports.write_report_tsv checks the vocabularies and falls back to pandas).  Column kinds:
 *   HAWK_TSV_CONST   data = the text (width bytes), the same in every row
 *   HAWK_TSV_FIXED   data = [n_rows][width] bytes
 *   HAWK_TSV_RAGGED  data = bytes, off = [n_rows + 1] offsets into them
 *   HAWK_TSV_INT64   data = int64[n_rows], written in decimal
 *   HAWK_TSV_VOCAB   data = uint32[n_rows] indices into n_vocab strings: pool = their bytes, off = [n_vocab + 1] offsets
 * Multi-threaded, two passes (row lengths, then bytes) into a shared mapping of the file (plain writes where mapping fails). */
#define HAWK_TSV_CONST 0u
#define HAWK_TSV_FIXED 1u
#define HAWK_TSV_RAGGED 2u
#define HAWK_TSV_INT64 3u
#define HAWK_TSV_VOCAB 4u
typedef struct {
  uint32_t kind, width;
  const void* data;
  const uint64_t* off;
  const void* pool;
  uint64_t n_vocab;
} hawk_tsv_col;
int hawk_host_tsv_write(const char* path, const char* header, uint64_t header_len, uint64_t n_rows, const uint64_t* order, uint32_t n_cols,
                        const hawk_tsv_col* cols, uint64_t* bytes_out);

/* Host-side helper of the report assembly (no device work): the report's `samples` / `haplotype_id` columns list every
 * carrier of every report row (reports.py:767-857) - a ragged join of label strings.  Items item_label[group_off[g] ..
 * group_off[g+1]) of group g name byte strings pool[pool_off[l] .. pool_off[l+1]); the group's text is those strings
 * joined by `sep`.  out_off[n_groups+1] always receives the groups' byte offsets; with out == NULL only sizes are
 * computed; HAWK_E_CAPACITY when out_cap is too small (required size in out_off[n_groups]). */
int hawk_host_ragged_join(const uint32_t* item_label, const uint64_t* group_off, uint64_t n_groups, const uint8_t* pool,
                          const uint64_t* pool_off, uint64_t n_labels, uint8_t sep, uint8_t* out, uint64_t out_cap,
                          uint64_t* out_off);

/* The same for a group's SET of items: haplotype h carries the items hap_item[hap_item_off[h] .. hap_item_off[h+1]) (indices
 * into a label pool held in sort order); per group the sorted unique items of its members member_hap[member_off[g] ..
 * member_off[g+1]) are joined - collapse_haplotype_ids (reports.py:845-857) and the unphased collapse_samples. */
int hawk_host_group_join(const uint64_t* member_off, const uint32_t* member_hap, uint64_t n_groups, const uint64_t* hap_item_off,
                         const uint32_t* hap_item, uint64_t n_haps, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_labels,
                         uint8_t sep, uint8_t* out, uint64_t out_cap, uint64_t* out_off);
/* The phased `samples` column (reports.py:767-810): per group one `name:a|b` per sample (samples numbered in the order of
 * their first entry in the sorted entry list) with the per-copy maxima over the members' entries.  ent_ok[e] = 0 marks an
 * entry that is not `name:int|int`; group_flags[g] bit 0: the group holds a well-formed entry, bit 1: it holds one that is
 * not; a group with none well-formed gets its sorted unique entries joined as they are (strings in ent_pool), one mixing
 * both kinds is left empty for the caller to resolve. */
int hawk_host_group_samples(const uint64_t* member_off, const uint32_t* member_hap, uint64_t n_groups, const uint64_t* hap_ent_off,
                            const uint32_t* hap_ent, uint64_t n_haps, const uint32_t* ent_sample, const uint16_t* ent_a1,
                            const uint16_t* ent_a2, const uint8_t* ent_ok, uint64_t n_entries, const uint8_t* name_pool,
                            const uint64_t* name_off, uint64_t n_samples, const uint8_t* ent_pool, const uint64_t* ent_pool_off,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* group_flags);

/* ---- the one exchange of a multi-GPU job.  One process per GPU, haplotypes block-partitioned with REF
 * on every rank (search_guides.py:111-131, 530-547 loop over independent haplotypes), no collective on the search
 * path; afterwards every rank's guide table goes to one rank over RCCL / xGMI.  The caller moves the 128-byte id from
 * rank 0 to the others (crisprhawk_hip/parallel.py does it over TCP).  hawk_table_gather: all-gather of the row
 * counts, then grouped ncclSend / ncclRecv of the columns straight from the tables' device memory; on `dst` *merged
 * is a table that owns its columns (download / device_columns / destroy), haplotype indices moved by each rank's
 * hap_offset (local row 0 = REF stays 0).  hawk_comm_gatherv: variable-length byte gather of host or device buffers
 * (recv_off[world + 1] byte offsets, needed on dst only). */
typedef struct hawk_comm hawk_comm;
int hawk_comm_unique_id(uint8_t* id128);
int hawk_comm_init(hawk_ctx* ctx, int world, int rank, const uint8_t* id128, hawk_comm** out);
void hawk_comm_destroy(hawk_comm* c);
const char* hawk_comm_last_error(void);
int hawk_comm_allgather_u64(hawk_comm* c, const uint64_t* mine, uint32_t k, uint64_t* all);
int hawk_comm_gatherv(hawk_comm* c, const void* send, uint64_t send_bytes, int send_on_device, void* recv,
                      const uint64_t* recv_off, int recv_on_device, int dst);
int hawk_table_gather(hawk_comm* c, hawk_table* t, uint32_t hap_offset, int dst, hawk_table** merged, float* ms);
/* The arithmetic of hawk_table_gather as a host function, free of device and RCCL calls (it runs without a GPU): from the
 * directory all ranks contributed - dir4[4 r .. 4 r + 3] = {rows, haplotype offset, candidates, hits} of rank r - the row
 * offset of every rank's slice in the merged table (row_off[world + 1]), the totals {rows, candidates, hits} and this
 * rank's transfers.  Columns are numbered hap pos strand start stop flags cfdon win[0..4] (HAWK_GATHER_COLS).  A sender gets
 * one op per column {col, dst, 0, bytes}; the destination one per column and rank {col, rank, byte offset into the merged
 * column, bytes}, its own slice included (a local copy).  ops == NULL only counts. */
#define HAWK_GATHER_COLS 12
typedef struct { uint32_t col, peer; uint64_t offset, bytes; } hawk_gather_op;
int hawk_host_gather_plan(int world, int rank, int dst, const uint64_t* dir4, uint64_t* row_off, uint64_t* totals3,
                          hawk_gather_op* ops, uint32_t cap, uint32_t* n_ops);

/* ---- f3: VCF sample columns -> allele codes -> carried-variant lists.  Replaces the per-sample Python work of
 * VariantRecord.read_vcf_line -> _genotypes_to_samples (variant.py:286-311, 558-619) and the inversion into
 * per-sample variant lists of compute_haplotypes_phased (haplotypes.py:132-159).
 * hawk_gt_parse: text = the raw bytes of n_lines VCF records ('\n'-terminated), record i =
 *   text[line_off[i], line_off[i+1]), its first sample column starts at gt_off[i] (host arrays).  The device
 *   keeps codes[n_lines][2*n_samples]: allele carried by copy 0 / copy 1 of each sample (0 REF, k = k-th ALT,
 *   255 missing or absent; an allele number >= 254 reads 254), and a flag byte per record, OR-ed over its first
 *   n_samples sample columns.  With g = a column up to its first ':':
 *     1 = g is not exactly two '|'-separated parts: unphased separator, haploid, three or more parts, empty column (the
 *         arity refusal of _parse_genotype_phased, variant.py:514-520, which comes before any look at the alleles);
 *     2 = the record does not have n_samples columns (columns beyond n_samples are not read, absent ones stay 255);
 *     4 = one of the first two parts of g - split at '|' if g holds one, else at '/' - is neither '.' nor all ASCII
 *         digits (no sign, no blank); its code stays 255.  "|1", "0|" , "0|1/2" and "0/1|2" are two '|'-parts of which
 *         one is no number: 4 alone, where the reference fails in int().  Next to 1 it is additional information.
 *   A record with any bit set is rejected by the callers (workload.expand_from_vcf: 2, then 1, then 4 decide the
 *   message).  A section that is empty (gt_off at the record's end or at its line terminator) has no column at all.
 *   hawk_gt_codes downloads both arrays (NULL skips).
 * hawk_gt_lists: variants j = (record var_line[j], allele var_allele[j] in 1..254); "ascending" below means ascending
 *   j - the caller's variant order (by position) - and var_line need not be monotone (multi-allelic records are
 *   re-positioned allele by allele).  Allele 254 matches code 254, i.e. every allele number the parser clamped.
 *   var_r0[j] = offset of
 *   the variant in the reference region, var_chain[j] = alt length - replaced length.  Per chromosome copy
 *   (column c = 2*sample + copy) the ascending list of carried variants is built on the device; col_off[2*n_samples+1]
 *   (host) receives the CSR offsets, col_delta (host, may be NULL) the summed length change per column.
 *   hawk_gt_lists_download copies hv_idx and hv_o = var_r0 + exclusive running sum of var_chain within the
 *   column (host or device destinations): the lists hawk_xplan_create_gt expands in place, for the rows "columns
 *   with a non-empty list, in column order". */
int hawk_gt_parse(hawk_ctx* ctx, const uint8_t* text, uint64_t text_len, const uint64_t* line_off, const uint64_t* gt_off,
                  uint64_t n_lines, uint32_t n_samples, hawk_gt** out, float* kernel_ms);
/* The same object from an allele-code matrix the caller already holds (codes[n_lines][2*n_samples], host): genotypes that
 * never were VCF text (an in-memory panel) enter the device inversion (hawk_gt_lists) without a host-side nonzero scan. */
int hawk_gt_from_codes(hawk_ctx* ctx, const uint8_t* codes, uint64_t n_lines, uint32_t n_samples, hawk_gt** out);
void hawk_gt_destroy(hawk_gt* g);
int hawk_gt_codes(hawk_gt* g, uint8_t* codes, uint8_t* line_flags);
int hawk_gt_lists(hawk_gt* g, const uint32_t* var_line, const uint8_t* var_allele, const int32_t* var_r0, const int32_t* var_chain,
                  uint32_t n_var, uint64_t* col_off, int64_t* col_delta, float* kernel_ms);
int hawk_gt_lists_download(hawk_gt* g, uint32_t* hv_idx, int32_t* hv_o);
/* The entries of those lists whose variant changes the haplotype's length (var_chain != 0), as ascending entry indices:
 * what the position-map segments are built from (haplotype.py:90-159) without a pass over all entries on the host.
 * *n_indel is always set; up to cap indices are copied (cap = 0 / NULL: ask for the number first). */
int hawk_gt_lists_indels(hawk_gt* g, uint32_t* entry_idx, uint64_t cap, uint64_t* n_indel);

/* ---- K7: off-target enumeration, replacing the external `crispritz.py search ... -mm M -bDNA 0
 * -bRNA 0` of offtargets.py:222-293 (CRISPRitz 2.6.6 is a third-party binary the reference shells
 * out to; semantics restated from the call site and the consumed fields, offtarget.py:77-101).
 * The genome is a hawk_hapset whose rows are equal-sized contig pieces (made on the host, each
 * piece overlapping the next by guidelen+pamlen-1 bases; scan_start/scan_stop of a row = the
 * window starts it owns).  hawk_genome_finalize() turns the planes one-hot once after packing.
 * guides2: one 64-bit word per guide, spacer base i (5'->3') at bits 2i,2i+1 with A0 C1 G2 T3.
 * A hit = window whose PAM positions hold unambiguous bases inside the PAM's IUPAC sets and whose
 * spacer has <= max_mm mismatches (ambiguous genome bases count as mismatches), either strand.
 * Outputs (cap entries each, any may be NULL): guide index, row, window start in the row, strand,
 * mismatches, the window in guide orientation as a 2-bit code, its ambiguity mask.  Unordered.
 * If more than cap hits exist returns HAWK_E_CAPACITY with *n_out = required. */
typedef struct { uint64_t pam_fwd, pam_rev; uint32_t pamlen, guidelen, right, max_mm; } hawk_ot_params;
typedef struct { float scan_ms, sites_ms, match_ms, total_ms; uint64_t n_sites, scanned_positions; } hawk_ot_timing;
int hawk_genome_finalize(hawk_hapset* rows);
int hawk_offtarget_scan(hawk_hapset* rows, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                        uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand, uint8_t* out_mm,
                        uint64_t* out_code, uint32_t* out_nmask, uint64_t cap, uint64_t* n_out, hawk_ot_timing* timing);
/* Bulged sites (-bDNA / -bRNA of the CRISPRitz call), one call per (type, size), selected on the device (k_ot_bulge).
 * p->guidelen is the GUIDE's length G; bulge_type 1 = DNA bulge (the site's spacer has Gs = G + bulge_size bases, bulge_size of
 * its interior positions 1 .. Gs - 2 face no guide base), 2 = RNA bulge (Gs = G - bulge_size, bulge_size interior guide positions
 * 1 .. G - 2 face no site base); bulge_size 1..2.  The rows' scan ranges (hawk_hapset_set_meta) must be those of windows of
 * Gs + pamlen bases.  At most one row per (guide, site, strand): the placement with the fewest mismatches among the paired
 * bases, ties to the lexicographically smallest tuple of bulge positions in guide orientation, reported when that minimum is
 * <= max_mm.  An aligned ambiguous site base counts as a mismatch; an ambiguous site base is never bulged out.
 * Output columns as hawk_offtarget_scan (code / nmask: the window of Gs + pamlen bases) plus out_gaps: bit i = position i is
 * bulged (of the site spacer for DNA bulges, of the guide for RNA bulges).  Rows are unordered.  cap / *n_out / HAWK_E_CAPACITY
 * as hawk_offtarget_scan.  HAWK_E_INVALID: type or size out of range, scan ranges that let a window of Gs + pamlen bases reach
 * past its row; HAWK_E_UNSUPPORTED: G - bulge_size < 3, G > 32, Gs + pamlen > 32.  Device memory is sized by n_guides and cap,
 * never by the placements. */
int hawk_offtarget_bulges(hawk_hapset* rows, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                          uint32_t bulge_type, uint32_t bulge_size, uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q,
                          uint8_t* out_strand, uint8_t* out_mm, uint64_t* out_code, uint32_t* out_nmask, uint64_t* out_gaps,
                          uint64_t cap, uint64_t* n_out, hawk_ot_timing* timing);
/* The same scan with every hit consumed inside the match kernel instead of listed: per-guide aggregates, mismatch-only, and no
 * memory on host or device that grows with the number of hits (no capacity, no retry).
 *   out_hist[g][m]  (row stride max_mm + 1) hits of guide g with m mismatches - the on-target site included
 *   out_cfd_e4[g]   sum over guide g's hits of round(CFD(guide, site), 4) in units of 1e-4, with the CFD formed as hawk_cfd forms
 *                   it (wildtype = the guide, sg = the site's spacer, the site's PAM[-2:]; same tables) and rounded as Python's
 *                   round(x, 4): correctly rounded on the binary value, exact ties to even.  The reference's global CFD is
 *                   100 / (100 + out_cfd_e4[g] / 1e4) (offtargets.py:561-627).  Integer sums: independent of the order of the
 *                   device's atomics and exactly additive over genome shards.
 * cfd_mm / cfd_pam both NULL: counts only (out_cfd_e4, if given, is zeroed).  A hit whose site has a non-ACGT base under a CFD
 * lookup (among the first min(guidelen, 20) spacer bases or in PAM[-2:]) - hawk_cfd's HAWK_E_CFD - is counted in *n_unscorable,
 * still counts in out_hist and adds nothing to out_cfd_e4.  *n_hits = all hits.  Argument checks as hawk_offtarget_scan;
 * HAWK_E_UNSUPPORTED also for max_mm > 32 and for CFD tables with pamlen < 2.  Duplicate guides get equal rows. */
int hawk_offtarget_summary(hawk_hapset* rows, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                           const double* cfd_mm, const double* cfd_pam, uint32_t* out_hist, int64_t* out_cfd_e4,
                           uint64_t* n_hits, uint64_t* n_unscorable, hawk_ot_timing* timing);
/* The summary of the bulged sites of one (type, size): hawk_offtarget_bulges' rows consumed inside k_ot_bulge instead of listed - no
 * hit list, no cap, no retry; device memory is sized by n_guides and max_mm alone.  All pairs, as hawk_offtarget_bulges.
 *   out_hist[g][m]  (row stride max_mm + 1) rows of guide g whose selected placement has m mismatches
 *   out_cfd_e4[g]   sum over guide g's rows of the CFD the off-targets table prints for the row, in units of 1e-4: the value
 *                   hawk_offtarget_text computes for the record (site window, guide, mm, gaps, kind, size) - the alignment column as
 *                   the table's position index, columns beside a '-' skipped, the last two characters of the spacer field as the
 *                   PAM key - through the same function (csrc/hawk_ottext.h: ot_text_row; csrc/hawk_otbulge.h: otb_pair)
 * p->guidelen is the GUIDE's length; bulge_type / bulge_size, the scan ranges and their refusals as hawk_offtarget_bulges (type or
 * size out of range, a plan view, scan ranges set for a shorter window: HAWK_E_INVALID; G - bulge_size < 3, G > 32, Gs + pamlen >
 * 32: HAWK_E_UNSUPPORTED); cfd_mm / cfd_pam, *n_hits, *n_unscorable and the remaining rules as hawk_offtarget_summary (both tables
 * or neither; HAWK_E_UNSUPPORTED for tables with pamlen < 2 and for max_mm > 32).  An unscorable row counts in out_hist and in
 * *n_unscorable and adds nothing.  Nothing is written to the outputs of a refused call. */
int hawk_offtarget_bulge_summary(hawk_hapset* rows, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                                 uint32_t bulge_type, uint32_t bulge_size, const double* cfd_mm, const double* cfd_pam,
                                 uint32_t* out_hist, int64_t* out_cfd_e4, uint64_t* n_hits, uint64_t* n_unscorable,
                                 hawk_ot_timing* timing);
/* The same sums on the host, no device: the site windows are given - code[i] / nmask[i] of the Gs + pamlen bases of site i in guide
 * orientation, as hawk_offtarget_bulges returns them (every one is taken to bear the PAM; p->pam_fwd / pam_rev are not read) - and
 * every (site, guide) pair goes through the function the kernel's summing sink runs, in a plain loop.  Same parameters, tables,
 * outputs and argument refusals. */
int hawk_host_offtarget_bulge_summary(const uint64_t* code, const uint32_t* nmask, uint64_t n_sites, const uint64_t* guides2,
                                      uint32_t n_guides, const hawk_ot_params* p, uint32_t bulge_type, uint32_t bulge_size,
                                      const double* cfd_mm, const double* cfd_pam, uint32_t* out_hist, int64_t* out_cfd_e4,
                                      uint64_t* n_hits, uint64_t* n_unscorable);

/* ---- K7 over a variant-enriched genome: the sites only an ALT allele makes.  (The reference defers this to CRISPRitz over an
 * enriched index and to CRISPRme; the semantics are this project's own, PARITY UNPINNED.)
 * hawk_genome_variants, after hawk_genome_finalize: n SNV entries (row, position q inside the row, REF base, ALT base; bases
 *   A0 C1 G2 T3) are added to the index.  The first call allocates four ALLELE planes in the rows' geometry - REF's one-hot planes
 *   with the ALT bases OR-ed in, 4/5 of the genome planes' bytes; ALT alone is allele & ~REF - and later calls add to the set.  A
 *   variant in the overlap of two rows is entered in both by the caller.  An entry is dropped, never refused, when the index
 *   holds a non-ACGT base at its position (HAWK_OV_REF_N = 1), when its REF base is not the index's (HAWK_OV_REF_MISMATCH = 2) or
 *   when its ALT is its REF (HAWK_OV_ALT_IS_REF = 3): status[i] (may be NULL) says which, 0 = applied; *n_applied / *n_dropped
 *   count the entries.  HAWK_E_INVALID, with nothing written: a row or position outside the index, a base above 3, a set that was
 *   not finalized, a plan view.  hawk_hapset_destroy frees the planes.  The plain scans never read them.
 * The allele set of a position = {REF base} + {its ALT bases}; an N position keeps the empty set and stays ambiguous.  Genotypes
 *   and phasing are not consulted: each allele is taken to exist in somebody and every combination inside a window on one
 *   chromosome (the enriched-genome semantics of CRISPRitz add-variants): an UPPER BOUND on what a population carries.
 * A window of guidelen + pamlen bases, either strand, in guide orientation, is resolved against one guide position by position
 *   (csrc/hawk_otvar.h: ov_resolve, the one statement kernel and host share):
 *     PAM position     satisfied iff its allele set meets the PAM's IUPAC set (a PAM 'N': any position, an ambiguous one
 *                      included, as in hawk_offtarget_scan); resolved base = REF's if REF is in the PAM's set, else the lowest
 *                      allele (A < C < G < T in guide orientation) of the intersection
 *     spacer position  resolved base = the guide's if it is in the allele set, else REF's, a mismatch; ambiguous = mismatch
 *   mm = mismatches of the resolved spacer, alt = bit i set where the resolved base (window position i) differs from REF's.
 * hawk_offtarget_variant_scan lists a row per (window, strand, guide) with every PAM position satisfied, mm <= max_mm and
 *   alt != 0.  Rows with alt == 0 are exactly hawk_offtarget_scan's and are not listed; a window may so have a REF row there and
 *   an ALT row here for one guide - two alleles of one locus.  Mismatch-only, all pairs.  Columns, cap / *n_out / HAWK_E_CAPACITY
 *   as hawk_offtarget_scan; out_code / out_nmask are the RESOLVED window (it feeds hawk_offtarget_text as it is), out_alt the alt
 *   mask.  Unordered.  The timing block is filled from the device's wall clock stamped at the stage boundaries (scan_ms: the PAM
 *   scan over the allele planes, the ALT-window filter and the offset scan; n_sites: PAM-bearing windows that hold an ALT allele).
 *   HAWK_E_INVALID: no hawk_genome_variants call on the set, scan ranges that let a window reach past its row, what
 *   hawk_offtarget_scan refuses. */
int hawk_genome_variants(hawk_hapset* rows, const uint32_t* row, const uint32_t* q, const uint8_t* ref, const uint8_t* alt, uint64_t n,
                         uint8_t* status, uint64_t* n_applied, uint64_t* n_dropped);
int hawk_offtarget_variant_scan(hawk_hapset* rows, const hawk_ot_params* p, const uint64_t* guides2, uint32_t n_guides,
                                uint32_t* out_guide, uint32_t* out_row, uint32_t* out_q, uint8_t* out_strand, uint8_t* out_mm,
                                uint64_t* out_code, uint32_t* out_nmask, uint32_t* out_alt, uint64_t cap, uint64_t* n_out,
                                hawk_ot_timing* timing);
/* The same rows on the host, no device: the rows' text (row h = seqs[seq_off[h], seq_off[h + 1]), any case, non-ACGT = ambiguous),
 * the window starts each row owns [scan_start[h], scan_stop[h]), the variant entries as hawk_genome_variants takes them (v_status
 * as its status, may be NULL) and the guides go through ov_resolve in plain loops.  Rows in (row, q, strand, guide) order; more
 * than cap: HAWK_E_CAPACITY with *n_out = required.  p->pam_rev is not read. */
int hawk_host_offtarget_variant_scan(const char* seqs, const uint64_t* seq_off, uint32_t n_rows, const int32_t* scan_start,
                                     const int32_t* scan_stop, const uint32_t* v_row, const uint32_t* v_q, const uint8_t* v_ref,
                                     const uint8_t* v_alt, uint64_t n_var, uint8_t* v_status, const hawk_ot_params* p,
                                     const uint64_t* guides2, uint32_t n_guides, uint32_t* out_guide, uint32_t* out_row,
                                     uint32_t* out_q, uint8_t* out_strand, uint8_t* out_mm, uint64_t* out_code, uint32_t* out_nmask,
                                     uint32_t* out_alt, uint64_t cap, uint64_t* n_out);

/* The hits of hawk_offtarget_scan / hawk_offtarget_bulges as the rows of offtargets_{contig}_{start}_{stop}.tsv (offtargets.py:
 * 41-53, 530-544), written on the device: per row the eleven fields chrom, position, strand, grna, spacer, pam, mm, bulge_size,
 * bulg_type, cfd, elevation joined by tabs, no newline - byte for byte what the package's host chain prints for the hit
 * (GenomeIndex._bulge_hit / hits_from_arrays -> crispritz_bulge_line / crispritz_report_line -> Offtarget.report_line -> the
 * float columns of offtargets_table).  One statement of the row serves device and host (csrc/hawk_ottext.h).
 *   records     n entries per column (host arrays): guide, row, q, strand, mm, code, nmask as the scans return them, gaps (0 for
 *               un-bulged hits), kind 0 = X / 1 = DNA / 2 = RNA, size 0 / 1..2.  The window (code / nmask) has Gs + pamlen bases,
 *               Gs = guidelen + size (DNA), guidelen - size (RNA) or guidelen; p->guidelen is the GUIDE's length.
 *   guides2     the guides' 2-bit codes (n_guides); p: pamlen, guidelen, right (pam_fwd / pam_rev / max_mm are not read)
 *   row table   row_contig[r] / row_off[r]: contig id and 64-bit offset of genome row r (n_table_rows); position = row_off + q
 *   contigs     contig c's name is name_blob[name_off[c], name_off[c + 1]) (n_contigs)
 *   pam_text    the NOMINAL PAM, pamlen bytes: the pam field, and the PAM of the grna field (in front when p->right)
 *   order       optional: output row i is record order[i] (any order, repeats allowed); NULL keeps input order
 *   cfd_mm / cfd_pam   mm[20][4][4] + pam[16] as hawk_cfd takes them, or both NULL: the cfd field is NA
 * cfd: compute_cfd as hawk_cfd forms it on the row's own strings - a left-to-right fp64 product over the first min(columns, 20)
 * ALIGNMENT columns, those with equal bases or a '-' on either side skipped, the table's position being the alignment column (a
 * DNA bulge moves every later mismatch by one), times the entry of the spacer field's last two characters - rounded as Python's
 * round(x, 4) and printed as repr() prints the rounded value (0.0, 1.0, 0.0312, 12.3456).  A row with an ambiguous base under a
 * lookup (hawk_cfd's HAWK_E_CFD) prints NA and is counted in *n_unscorable.  elevation is NA.
 * The rows stay in HBM: *n_bytes = bytes of their blob.  hawk_offtarget_text_download copies them into the caller's buffers -
 * blob[n_bytes], off = uint64[n + 1] (row i = blob[off[i], off[i + 1])), cfd_e4 = int64[n], the rows' CFD in units of 1e-4
 * (-1: NA or unscorable) - and returns the workspace to the caching allocator; once per hawk_offtarget_text of the context.
 * n = 0 is HAWK_OK (an empty blob, off[0] = 0).  All offsets are 64 bits.  HAWK_E_INVALID, with nothing written and the context
 * usable as before: kind or size out of range (or a bulge without size / a size without bulge), gaps with a bit outside the
 * interior positions 1 .. span - 2 (span = Gs for DNA, guidelen for RNA bulges) or a popcount that is not size, a window beyond 32
 * bases, a guide index >= n_guides, a row index >= n_table_rows, a contig id >= n_contigs, an order entry >= n.
 * HAWK_E_UNSUPPORTED: guidelen + pamlen > 32, CFD tables with pamlen < 2. */
typedef struct {
  float upload_ms, len_ms, scan_ms, fill_ms, reserved, total_ms; /* HIP events around the stages of one call */
  uint64_t out_bytes, n_rows;
} hawk_ot_text_timing;
int hawk_offtarget_text(hawk_ctx* ctx, uint64_t n, const uint32_t* guide, const uint32_t* row, const uint32_t* q, const uint8_t* strand,
                        const uint8_t* mm, const uint64_t* code, const uint32_t* nmask, const uint64_t* gaps, const uint8_t* kind,
                        const uint8_t* size, const uint64_t* guides2, uint32_t n_guides, const hawk_ot_params* p,
                        const uint32_t* row_contig, const uint64_t* row_off, uint32_t n_table_rows, const uint8_t* name_blob,
                        const uint64_t* name_off, uint32_t n_contigs, const char* pam_text, const uint64_t* order, const double* cfd_mm,
                        const double* cfd_pam, uint64_t* n_bytes, uint64_t* n_unscorable, hawk_ot_text_timing* timing);
int hawk_offtarget_text_download(hawk_ctx* ctx, uint8_t* blob, uint64_t* off, int64_t* cfd_e4, float* download_ms);
/* The same rows made on the host by the same function, single-threaded, no device (the CPU tests hold the statement to the
 * fixtures with it).  Same arguments, checks and statuses; off[n + 1], cfd_e4[n], *n_bytes and *n_unscorable are always written,
 * the bytes when `blob` is non-NULL and blob_cap suffices - else HAWK_E_CAPACITY with the required size in *n_bytes. */
int hawk_host_offtarget_text(uint64_t n, const uint32_t* guide, const uint32_t* row, const uint32_t* q, const uint8_t* strand,
                             const uint8_t* mm, const uint64_t* code, const uint32_t* nmask, const uint64_t* gaps, const uint8_t* kind,
                             const uint8_t* size, const uint64_t* guides2, uint32_t n_guides, const hawk_ot_params* p,
                             const uint32_t* row_contig, const uint64_t* row_off, uint32_t n_table_rows, const uint8_t* name_blob,
                             const uint64_t* name_off, uint32_t n_contigs, const char* pam_text, const uint64_t* order,
                             const double* cfd_mm, const double* cfd_pam, uint8_t* blob, uint64_t blob_cap, uint64_t* off, int64_t* cfd_e4,
                             uint64_t* n_bytes, uint64_t* n_unscorable);

/* ---- K4 stand-alone: compute_cfd() (scores/cfdscore/cfdscore.py:53-95) on n triples --------
 * wt / sg: n spacers of `len` characters each (host, contiguous, any case, T or U); pam2: n
 * two-character strings (the caller passes guide.pam[-2:], crisprhawk_scores.py:84-86).
 * out[i] = prod over i<min(len,20), wt!=sg of mm[i][wt][sg] times pam[pam2], fp64, left to
 * right.  Any non-ACGT base under a lookup -> HAWK_E_CFD (the reference's KeyError). */
int hawk_cfd(hawk_ctx* ctx, const char* wt, const char* sg, uint32_t len, const char* pam2, uint64_t n,
             const double* cfd_mm, const double* cfd_pam, double* out);

/* ---- K6: Seq-DeepCpf1 (scores/deepCpf1/seqdeepcpf1.py:22-92; wrapper scores/crisprhawk_scores.py:
 * 90-107): n 34-mers (host, contiguous, ACGT any case) -> n fp32 scores.  `weights` is one packed
 * fp32 block in the torch layout of SeqDeepCpf1: conv.weight[80][4][5], conv.bias[80],
 * fc1.weight[80][1200], fc1.bias[80], fc2.weight[40][80], fc2.bias[40], fc3.weight[40][40],
 * fc3.bias[40], output.weight[1][40], output.bias[1].  A non-ACGT base -> HAWK_E_IUPAC (the
 * reference's KeyError, seqdeepcpf1.py:91). */
#define HAWK_DEEPCPF1_NPARAMS (1600 + 80 + 96000 + 80 + 3200 + 40 + 1600 + 40 + 40 + 1)
int hawk_deepcpf1(hawk_ctx* ctx, const char* seqs34, uint64_t n, const float* weights, float* out);

/* ---- K5: Azimuth / Rule Set 2 (scoring.py:87-193 -> scores/azimuth/model_comparison.py:507-585):
 * n 30-mers (4 nt + 20-nt guide + NGG + 3 nt) -> fp64 predictions of a gradient-boosted regression
 * tree ensemble over the 627 features of features/featurization.py (order-1/2 position-dependent
 * and -independent nucleotide features, GC features, NGGX, four nearest-neighbour melting
 * temperatures).  The model is the flattened form of the sklearn GradientBoostingRegressor the
 * reference unpickles: per tree a node range [tree_off[t], tree_off[t+1]); node k is a leaf iff
 * feature[k] < 0, else x[feature[k]] (as float32) <= threshold[k] goes to left[k] else right[k]
 * (indices relative to the tree); prediction = init + learning_rate * sum of leaf values.
 * feats_out (optional, n*627 doubles) receives the feature matrix.  Non-ACGT -> HAWK_E_IUPAC. */
typedef struct {
  uint32_t n_trees, n_nodes;
  const int32_t* tree_off; /* n_trees + 1 */
  const int32_t* feature;  /* n_nodes */
  const int32_t* left;
  const int32_t* right;
  const double* threshold;
  const double* value;
  double init, learning_rate;
} hawk_gbt_model;
/* The melting temperature behind Azimuth's four Tm features on its own - Biopython's MeltingTemp.Tm_NN with its defaults
 * (featurization.py:358-397 calls it on the 30-mer and three of its slices) - for n sequences of `len` <= 32 bases each,
 * A/C/G/T only (HAWK_E_IUPAC otherwise).  The same device function k_azimuth uses; tests hold it to the value Biopython documents. */
int hawk_tm_nn(hawk_ctx* ctx, const char* seqs, uint32_t len, uint64_t n, double* out);
int hawk_azimuth(hawk_ctx* ctx, const char* seqs30, uint64_t n, const hawk_gbt_model* model, double* out, double* feats_out);

/* The same tree evaluator over a feature matrix the caller supplies (feats[n][n_features], host, row-major doubles):
 * the device half of RS3 (scoring.py:196-300 -> rs3.seq.predict_seq, scores/crisprhawk_scores.py:47-62: a LightGBM
 * model over sglearn features; the third-party featuriser stays on the caller's side, the exported LightGBM text
 * model is flattened into hawk_gbt_model by crisprhawk_hip/scoring.py).  cast_f32 = 1 compares float32(x) as sklearn
 * does, 0 the double itself as LightGBM does. */
int hawk_gbt_predict(hawk_ctx* ctx, const double* feats, uint64_t n, uint32_t n_features, const hawk_gbt_model* model, int cast_f32,
                     double* out);

/* ---- BED annotation join: BedAnnotation.fetch_features + the label join per guide / off-target row (bedfile.py:406-425,
 * annotation.py:373-462, offtargets.py:407-483) for a whole batch of rows ----------------------------------------------------
 * One handle per (annotation file, contig, label kind), resident in HBM.  `start` / `end`: the contig's n features in FILE order,
 * 0-based half-open, sorted by start (what tabix requires of a BED file) with end >= start - HAWK_E_INVALID otherwise; feature
 * i's label is label_blob[label_off[i], label_off[i + 1]) (label_off[0] = 0).  All arrays are host memory and are copied.
 * n = 0 is a valid table (a contig the file does not have): every row of every query is "NA".  *index_ms (may be NULL): device
 * time of the two index kernels (running maximum of end, maximum per block of 64 features).
 *
 * hawk_annot_query: feature [fs, fe) and query [qs, qe) overlap iff fs < qe && fe > qs (tabix's half-open rule; parity
 * unpinned: pysam absent).  Row q of the result is the labels of query q's overlapping features joined by ',' in file order
 * (an empty label is an empty field: one overlap with an empty label gives the empty row, as the reference's join does), or
 * the two bytes "NA" when nothing overlaps.  The rows are left in HBM; *n_bytes = bytes of their blob, *n_overlaps (may be
 * NULL) = (feature, query) pairs found.  Offsets and coordinates are 64 bits.  Queries may come in any order; callers'
 * queries are sorted by position, which is what makes neighbouring lanes read the same lines.
 * hawk_annot_download copies the rows of the last query into the caller's buffers - blob[n_bytes], off = uint64[nq + 1], row
 * q = blob[off[q], off[q + 1]); page-locked buffers (hawk_host_alloc) take the copy at link speed - and returns the batch's
 * device workspace to the caching allocator.  Once per query; HAWK_E_INVALID without a query before it. */
typedef struct hawk_annot hawk_annot;
typedef struct {
  float upload_ms, count_ms, scan_ms, fill_ms, reserved, total_ms; /* HIP events around the stages of one query call */
  uint64_t out_bytes;  /* bytes of the blob */
  uint64_t walk_steps; /* features and skipped blocks the count pass stepped over, all queries */
} hawk_annot_timing;
int hawk_annot_create(hawk_ctx* ctx, const int64_t* start, const int64_t* end, const uint8_t* label_blob, const uint64_t* label_off,
                      uint64_t n, hawk_annot** out, float* index_ms);
int hawk_annot_query(hawk_annot* annot, const int64_t* qstart, const int64_t* qstop, uint64_t nq, uint64_t* n_bytes,
                     uint64_t* n_overlaps, hawk_annot_timing* timing);
int hawk_annot_download(hawk_annot* annot, uint8_t* blob, uint64_t* off, float* download_ms);
void hawk_annot_free(hawk_annot* annot);

/* ---- gnomAD sites VCF -> population-genotype VCF (converter.py:129-265 of the reference: _asses_genotype, _format_vrecord and
 * the keep rule of _convert, per data line) ------------------------------------------------------------------------------------
 * `text` holds whole data lines of a sites VCF (no '#' lines), record i = text[line_off[i], line_off[i + 1]) ending in '\n'
 * (a '\r' before it is dropped).  Key k (a population's allele-count key, e.g. AC_afr) is key_blob[key_off[k], key_off[k + 1]);
 * at most 31 keys of at most 255 bytes and 2048 bytes in all, none empty or holding ';', '=' or a tab.  The rules are stated once, in
 * csrc/hawk_gnomad.h, for the kernels and for hawk_host_gnomad_lines.
 *
 * hawk_gnomad_scan uploads the text once and runs k_gn_scan; hawk_gnomad_records downloads, per record (a NULL argument skips
 * that array):
 *   mask       uint32     bit k: key k's value holds a count > 0 (read left to right up to the first such count)
 *   flags      uint8      HAWK_GN_DROPPED (keep == 0 and FILTER has no token PASS; nothing else of the record is examined),
 *                         HAWK_GN_KEY_ABSENT, HAWK_GN_BAD_VALUE ('.' before a positive count, an empty value, the key without '=',
 *                         an entry that is no optionally signed run of 1..10 digits), HAWK_GN_FEW_FIELDS (fewer than eight),
 *                         HAWK_GN_ALT_MISSING (ALT is "."), HAWK_GN_BAD_POS (POS empty or not all digits)
 *   field_off  uint32[8]  where the first eight fields start, relative to the record (the record's length for a field it lacks)
 *   qual_span  uint32[2]  offset and length of QUAL
 *   af_span    uint32[2]  offset and length of the value of the INFO entry whose key is exactly AF; when there is none the
 *                         length is 0xffffffff and the first word holds the number of ALT alleles (commas in ALT plus one)
 * hawk_gnomad_text writes the output line of every record whose flags are 0 ("CHROM POS ID REF ALT QUAL FILTER AF=<af> GT" and
 * one 0/1 or 0/0 per key, tab-joined, ended by '\n'; FILTER "." becomes the empty string) and leaves the lines in HBM.  QUAL
 * and AF are printed from the caller's pool, entry j = pool_blob[pool_off[j], pool_off[j + 1]): entry k is the QUAL text of
 * the k-th kept record, entry n_kept + k its AF text (ignored when the record has no AF entry: "0.0" per ALT allele is
 * printed).  pool_off has 2 * n_kept + 1 entries; *n_kept and *n_bytes are written in any case, so a call with pool_off == NULL
 * reports n_kept and does nothing else.  hawk_gnomad_text_download copies the lines: blob[n_bytes], off = uint64[n_lines + 1]
 * (line i = blob[off[i], off[i + 1]), empty for a record with flags); either may be NULL.
 * HAWK_E_INVALID with nothing written: n_keys > 31, a malformed key, a text that does not end in '\n', offsets that are not
 * whole lines inside the text, a record longer than 2^32 - 1 bytes.  n_lines = 0 is HAWK_OK with an empty blob.  All offsets
 * are 64 bits. */
#define HAWK_GN_DROPPED 1
#define HAWK_GN_KEY_ABSENT 2
#define HAWK_GN_BAD_VALUE 4
#define HAWK_GN_FEW_FIELDS 8
#define HAWK_GN_ALT_MISSING 16
#define HAWK_GN_BAD_POS 32
typedef struct hawk_gnomad hawk_gnomad;
typedef struct {
  float upload_ms, scan_ms, len_ms, prefix_ms, fill_ms, total_ms; /* HIP events around the stages of one call */
  uint64_t n_records, n_kept, out_bytes;
} hawk_gnomad_timing;
int hawk_gnomad_scan(hawk_ctx* ctx, const uint8_t* text, uint64_t text_len, const uint64_t* line_off, uint64_t n_lines,
                     const uint8_t* key_blob, const uint64_t* key_off, uint32_t n_keys, int keep, hawk_gnomad** out,
                     hawk_gnomad_timing* timing);
int hawk_gnomad_records(hawk_gnomad* g, uint32_t* mask, uint8_t* flags, uint32_t* field_off, uint32_t* qual_span, uint32_t* af_span);
int hawk_gnomad_text(hawk_gnomad* g, const uint8_t* pool_blob, const uint64_t* pool_off, uint64_t* n_bytes, uint64_t* n_kept,
                     hawk_gnomad_timing* timing);
int hawk_gnomad_text_download(hawk_gnomad* g, uint8_t* blob, uint64_t* off);
void hawk_gnomad_destroy(hawk_gnomad* g);
/* The same on the host by the same header, single-threaded, no device.  The per-record arrays (those that are not NULL) and
 * *n_kept are always written; with pool_off == NULL the call ends there (*n_bytes = 0).  Otherwise off[n_lines + 1] (if not
 * NULL) and *n_bytes are written, the lines when `blob` is non-NULL and blob_cap suffices - else HAWK_E_CAPACITY with the
 * required size in *n_bytes. */
int hawk_host_gnomad_lines(const uint8_t* text, uint64_t text_len, const uint64_t* line_off, uint64_t n_lines, const uint8_t* key_blob,
                           const uint64_t* key_off, uint32_t n_keys, int keep, uint32_t* mask, uint8_t* flags, uint32_t* field_off,
                           uint32_t* qual_span, uint32_t* af_span, const uint8_t* pool_blob, const uint64_t* pool_off, uint8_t* blob,
                           uint64_t blob_cap, uint64_t* off, uint64_t* n_bytes, uint64_t* n_kept);
/* What pysam hands Python for a Float field, printed as Python prints it: string i = text[start[i], start[i] + len[i]) is a
 * comma list; every entry is read with strtod, narrowed to float32, widened again and printed as str() prints that double
 * (shortest digits that round-trip; fixed notation while the decimal exponent is in -4 .. 15, ".0" appended to integers, else
 * d.ddde-05 with at least two exponent digits).  An entry that is exactly "." prints as `missing`.  len[i] == 0xffffffff
 * gives the empty string.  status[i] = 1 when an entry is empty, is no decimal number in full, or is not finite as a float32
 * (its output is then empty).  out_off[n + 1] is always written; the bytes when `out` is non-NULL and out_cap suffices, else
 * HAWK_E_CAPACITY with the required size in out_off[n].  `threads` host threads (0: one per core, at most 32). */
int hawk_host_f32_repr(const uint8_t* text, const uint64_t* start, const uint32_t* len, uint64_t n, const char* missing, uint8_t* out,
                       uint64_t out_cap, uint64_t* out_off, uint8_t* status, uint32_t threads);

/* ---- variant effects: the data stage behind the reference's --graphical-reports (graphical_reports.py: _compute_delta_table,
 * _count_guide_type) on the report GROUPS of a collapsed table, which stay in HBM.  The rules are stated once, in
 * csrc/hawk_effects.h, for the kernels (k_fx_*) and for hawk_host_effects: the score as the report prints it (round(x, 4)), the
 * delta against the REF group of the same (start, strand), the valid alternatives, the worst delta per position, the ranking
 * and the guide types.  ONE order is this project's own: inside a run of equal worst deltas, where pandas' unstable sort leaves
 * the reference's order undefined, positions rank by their first appearance in report order.
 *
 * Groups come in collapse order (start, strand, group) - hawk_table_collapse_download documents it - so the groups of one
 * position are contiguous; a POSITION is named by the index of its first group (its head), and per-position results sit at the
 * head's index of arrays of n_groups entries (other entries hold HAWK_FX_NONE / 0).  `rank[g]` is the report rank of group g (the
 * inverse of the row order the report is written in): it orders the alternatives, breaks ties and decides which of two groups
 * showing the same guide counts.  Haplotype rows name their samples through a CSR (hap_off[n_hap + 1], sample_id[], REF rows
 * empty); ids lie in [0, n_sample_ids) and n_sample_ids may be at most HAWK_FX_SAMPLE_CAP (one bit per sample in 8 KiB of LDS):
 * more is HAWK_E_UNSUPPORTED, never a wrong count.  guidelen + pamlen + 20 may be at most 64, as for every table.
 *
 * hawk_effects_create runs the group export of a collapsed table on the device and then the score-independent passes
 * (k_fx_groups: position heads, guide type, the duplicate rule, the four type counts; k_fx_samples_*: distinct samples per group);
 * nothing of the table is downloaded, and the handle keeps its own copies, so it outlives the table and later searches.
 * hawk_effects_create_columns does the same from host arrays (tests; callers whose groups were merged on the host).
 * hawk_effects_create_ugroups keeps hawk_effects_create's contract with the report groups of an unphased resolution (a
 * hawk_ugroups result, declared below with hawk_resolve_groups) in place of a collapsed table's: rank, hap_off and sample_id come
 * from the host, every group column is read where it lies in HBM - the groups ascend by (start, strand, ...), so a position's
 * groups are contiguous - and the origin of a group is the result's is_ref (what k_fx_isref_gather makes of the set's flags and
 * the first members).  n_hap must be the set's the groups were made from (HAWK_E_INVALID otherwise).  A valid empty result gives
 * a valid handle of zero groups.  Groups made without CFD tables hold NaN alone in cfdon: hawk_effects_rank(score = NULL) on such
 * a handle is HAWK_E_INVALID, as after _create_columns without cfdon.  The handle keeps its own copies of start, strand, origin,
 * rank and CFDon: it outlives the hawk_ugroups result, the hawk_resolve handle, the table and the set.
 * All three: on every status but HAWK_OK *out stays NULL (create_ugroups writes it so; the other two leave it untouched) and
 * nothing stays allocated; timing->upload_ms covers the host arrays and the device-to-device copies.
 * hawk_effects_rank, once per score on the same handle: `family` HAWK_FX_SIGNED (score_cfdon) or HAWK_FX_ABSOLUTE (azimuth, rs3,
 * deepcpf1); `score` = double[n_groups], or NULL for the table's CFDon; candidates are positions (start, strand), they come
 * first in the order given, then the best K - n_cand other positions that have a REF group.  1 <= K <= HAWK_FX_MAX_K and
 * n_cand <= K, else HAWK_E_INVALID.  A candidate whose position is absent or has no REF group is reported as HAWK_FX_NONE in
 * `chosen` (the caller raises).  *n_chosen and *n_alts size the download.
 * hawk_effects_download copies what is not NULL in `out`:
 *   per group     score (rounded), delta, abs_delta (double), n_samples (uint32; REF 0), type (uint8: 0 ref, 1 spacer+PAM,
 *                 2 spacer, 3 PAM, HAWK_FX_TYPE_UNKNOWN neither), dup (uint8: an earlier group in report order shows the same guide), position
 *                 (uint32: the head)
 *   per position  pos_ref (uint32 group or HAWK_FX_NONE), pos_worst (double), pos_nvalid, pos_first_rank (uint32)
 *   chosen        uint32[n_chosen] heads in rank order; alt_off uint64[n_chosen + 1], alt_group uint32[n_alts]: the valid
 *                 alternatives of every chosen position in report order
 *   counts        uint64[8]: groups of type 0..3 and of type HAWK_FX_TYPE_UNKNOWN that are no duplicates, positions, groups whose sample
 *                 list went to the wave path, 0 */
#define HAWK_FX_SIGNED 0
#define HAWK_FX_ABSOLUTE 1
#define HAWK_FX_MAX_K 64
#define HAWK_FX_SAMPLE_CAP 65536
#define HAWK_FX_NONE 0xffffffffu       /* "no group" / "no position" in pos_ref, chosen, pos_first_rank */
#define HAWK_FX_TYPE_UNKNOWN 255        /* an alternative without a lower-case base in spacer or PAM */
typedef struct hawk_effects hawk_effects;
struct hawk_ugroups; /* hawk_resolve_groups' result: typedef'd below */
typedef struct {
  uint64_t n_groups, win_stride;
  const int64_t* start;
  const int64_t* stop;
  const uint8_t* strand;
  const uint64_t* win;        /* [5][win_stride] window slices */
  const double* cfdon;        /* may be NULL when every rank call brings its scores */
  const uint64_t* member_off; /* [n_groups + 1] */
  const uint32_t* member_hap;
  const uint8_t* hap_is_ref;  /* [n_hap] */
  const uint64_t* hap_off;    /* [n_hap + 1] */
  const uint32_t* sample_id;
  const uint32_t* rank;
  uint32_t n_hap, n_sample_ids, guidelen, pamlen, right, reserved;
} hawk_effects_columns;
typedef struct {
  double* score;
  double* delta;
  double* abs_delta;
  uint32_t* n_samples;
  uint8_t* type;
  uint8_t* dup;
  uint32_t* position;
  uint32_t* pos_ref;
  double* pos_worst;
  uint32_t* pos_nvalid;
  uint32_t* pos_first_rank;
  uint32_t* chosen;
  uint64_t* alt_off;
  uint32_t* alt_group;
  uint64_t* counts;
} hawk_effects_out;
typedef struct {
  float upload_ms, groups_ms, samples_ms, positions_ms, topk_ms, alts_ms, total_ms; /* HIP events around the stages of one call */
  float reserved;
  uint64_t n_groups, n_positions, n_long;
} hawk_effects_timing;
int hawk_effects_create(hawk_table* t, const uint32_t* rank, const uint64_t* hap_off, const uint32_t* sample_id, uint32_t n_hap,
                        uint32_t n_sample_ids, hawk_effects** out, hawk_effects_timing* timing);
int hawk_effects_create_columns(hawk_ctx* ctx, const hawk_effects_columns* cols, hawk_effects** out, hawk_effects_timing* timing);
int hawk_effects_create_ugroups(struct hawk_ugroups* g, const uint32_t* rank, const uint64_t* hap_off, const uint32_t* sample_id,
                                uint32_t n_hap, uint32_t n_sample_ids, hawk_effects** out, hawk_effects_timing* timing);
int hawk_effects_rank(hawk_effects* fx, int family, const double* score, const int64_t* cand_start, const uint8_t* cand_strand,
                      uint32_t n_cand, uint32_t K, uint32_t* n_chosen, uint64_t* n_alts, hawk_effects_timing* timing);
int hawk_effects_download(hawk_effects* fx, const hawk_effects_out* out);
void hawk_effects_free(hawk_effects* fx);
/* The same on the host by the same header, single-threaded, no device: every array of `out` that is not NULL is written
 * (alt_group holds up to alt_cap entries, else HAWK_E_CAPACITY with the need in *n_alts).  Same refusals. */
int hawk_host_effects(const hawk_effects_columns* cols, int family, const double* score, const int64_t* cand_start,
                      const uint8_t* cand_strand, uint32_t n_cand, uint32_t K, const hawk_effects_out* out, uint64_t alt_cap,
                      uint32_t* n_chosen, uint64_t* n_alts);
/* round(x, 4) as Python computes it (csrc/hawk_effects.h: fx_round4), element by element */
int hawk_host_round4(const double* x, uint64_t n, double* out);

/* ---- unphased IUPAC windows resolved on the table: retrieve_guides' unphased branch and remove_redundant_guides
 * (search_guides.py:163-257, 340-369, 463-480) on the rows in HBM.  The rules are stated once, in csrc/hawk_resolve.h, for the
 * kernels (k_ur_count, k_ur_fill) and for hawk_host_resolve_unphased: a row's validity (is_pamhit_valid, strict on the right), the
 * options of a window position (its set bases in A, C, G, T order, once per allele entry of (haplotype, position), upper case where
 * the base is the entry's ref), the PAM re-check on the resolved PAM slice, itertools.product order (leftmost position slowest),
 * and the redundancy rule: a combination of a non-REF row is dropped when a REF guide shares its (start, strand) and its upper-cased
 * core (window offsets [10, W - 10)) is REF's.  W = guidelen + pamlen + 20 <= 64.
 *
 * The allele table: `key` = sorted (haplotype row << 32 | position in the haplotype) of every position with entries, `off` the CSR
 * offsets of its entries, `ref` one byte per entry (the entry's ref base 0-3 for A C G T, 255 when its ref is not one base).
 *
 * hawk_table_resolve_unphased runs on a table whose set carries its metadata (hawk_hapset_set_meta), before hawk_table_download;
 * the table stays as it is.  It uploads the allele table, lists REF's rows by (start, strand), counts (k_ur_count), scans and reads
 * the offsets back: *n_kept says how much room the result needs.  hawk_resolve_download then runs the fill pass (k_ur_fill) in
 * batches of whole rows of at most HAWK_RESOLVE_BATCH_BYTES (environment, read by hawk_table_resolve_unphased, default 256 MiB; 44
 * bytes per kept guide) of device memory and copies every batch straight into what is not NULL of src_row[n_kept] and
 * win[5][n_kept] (plane stride n_kept; host - page-locked for copies at link speed - or device); row_resolved / row_kept[n_rows]:
 * per table row the combinations after the PAM re-check and after the redundancy rule.  Kept guides come in table-row order,
 * inside a row in enumeration order.  The handle reads the set's row buffers: it must be downloaded before the next search on the
 * set (HAWK_E_INVALID afterwards) and freed before the set is destroyed.  `timing`: the first call fills all but fill_ms and
 * n_batches, the download returns the same with them (total_ms: both calls' device intervals).
 *
 * A call DECLINES - nothing is computed, *out stays NULL, `decline` (optional) names the reason and the first offending row - with
 *   HAWK_E_UNSUPPORTED  HAWK_RESOLVE_NO_ENTRY   an ambiguous position without allele entries (the reference's KeyError)
 *                       HAWK_RESOLVE_MULTI_REF  more than one haplotype flagged REF (row = -1)
 *                       HAWK_RESOLVE_REF_AMBIG  a REF row with more than one combination
 *   HAWK_E_CAPACITY     HAWK_RESOLVE_ROW_SIZE   a row of more than 2^32 - 1 combinations (counts are 64-bit and saturate)
 *                       HAWK_RESOLVE_BATCH      a row whose kept guides do not fit the batch budget
 * HAWK_E_INVALID: a stale or merged table, a malformed allele table (unsorted keys, offsets that do not ascend, a ref byte that is
 * neither 0-3 nor 255).  hawk_host_resolve_unphased: the same from host arrays by the same header, single-threaded, no device;
 * src_row[out_cap] and win[5][out_cap] (plane stride out_cap) are written when either is not NULL: HAWK_E_CAPACITY with
 * decline->reason == 0 and the need in *n_out when out_cap is too small (the per-row counts are written); with both NULL the call
 * only counts.  batch_bytes: the budget a row's kept guides must fit (0: none). */
#define HAWK_RESOLVE_NO_ENTRY 1
#define HAWK_RESOLVE_MULTI_REF 2
#define HAWK_RESOLVE_REF_AMBIG 3
#define HAWK_RESOLVE_ROW_SIZE 4
#define HAWK_RESOLVE_BATCH 5
typedef struct hawk_resolve hawk_resolve;
typedef struct {
  uint64_t n_keys;
  const uint64_t* key;
  const uint32_t* off;  /* [n_keys + 1] */
  const uint8_t* ref;   /* [off[n_keys]] */
} hawk_resolve_alleles;
typedef struct {
  uint64_t n_rows, win_stride;
  const uint32_t* hap;
  const uint32_t* pos;
  const uint8_t* strand;
  const int64_t* start;
  const uint8_t* flags;
  const uint64_t* win;        /* [5][win_stride] */
  const uint32_t* hap_len;    /* [n_hap] */
  const uint8_t* hap_is_ref;  /* [n_hap] */
  uint64_t pam_fwd, pam_rev;
  uint32_t n_hap, guidelen, pamlen, right;
} hawk_resolve_columns;
typedef struct {
  int32_t reason;  /* HAWK_RESOLVE_*, 0: none */
  int32_t reserved;
  int64_t row;     /* table row, -1: none */
} hawk_resolve_decline;
typedef struct {
  float upload_ms, refsort_ms, count_ms, scan_ms, fill_ms, total_ms; /* HIP events; fill_ms: kernels and copies of all batches (hawk_resolve_download) */
  uint32_t n_batches, reserved;
  uint64_t n_rows, n_resolved, n_kept;
} hawk_resolve_timing;
int hawk_table_resolve_unphased(hawk_table* t, const hawk_resolve_alleles* alleles, uint64_t pam_fwd, uint64_t pam_rev, hawk_resolve** out,
                                uint64_t* n_kept, uint64_t* n_resolved, hawk_resolve_decline* decline, hawk_resolve_timing* timing);
int hawk_resolve_download(hawk_resolve* r, uint32_t* src_row, uint64_t* win, uint32_t* row_resolved, uint32_t* row_kept,
                          hawk_resolve_timing* timing);
void hawk_resolve_free(hawk_resolve* r);
int hawk_host_resolve_unphased(const hawk_resolve_columns* cols, const hawk_resolve_alleles* alleles, uint64_t batch_bytes,
                               uint32_t* row_resolved, uint32_t* row_kept, uint32_t* src_row, uint64_t* win, uint64_t out_cap,
                               uint64_t* n_out, uint64_t* n_resolved, hawk_resolve_decline* decline);

/* ---- report groups of an unphased resolution: the kept guides of a hawk_resolve handle grouped as the guide report merges them
 * (reports.report_from_guides), with CFDon against the REF guide at the same (start, strand) (scoring.cfdon_score), in HBM.  The
 * rules are stated once, in csrc/hawk_ugroups.h, for the kernels (k_ug_keys, k_ug_heads, k_ug_emit) and for
 * hawk_host_unphased_groups.
 *
 * The key of a kept guide, compared in this order: start, strand, origin (its row's haplotype is REF), stop, then the five
 * planes (A, C, G, T, case) of its core at window offsets [10 - up, W - 10 + down), flank_up / flank_down (<= 10) in guide
 * orientation as hawk_table_collapse_ex takes them ((0, 0): the plain report, (4, 3): the scorers' k-mer).  Two guides share a
 * group iff their keys are equal (decided on the words, by an LSD sequence of radix sorts - no hash); groups come out ascending
 * by the key.  Inside a group the guides are ordered by (haplotype row, pos, kept index): the first is the representative, whose
 * src_row, hap, pos, strand, start, stop, is_ref, cfdon, win[5] and G/C counts (of its spacer, as hawk_table_collapse counts) are
 * the group's; member_hap[member_off[g] .. member_off[g + 1]) holds each haplotype row of the group once, ascending.
 * CFDon: the guide's REF partner is the one kept guide of a REF row at the same (start, strand) - a REF row that is invalid or
 * whose PAM fails the re-check kept nothing and is no partner; without a partner, or with cfd_mm NULL, the value is NaN; else the
 * left-to-right fp64 product of hawk_search's CFDon (cfd_mm[20][4][4], cfd_pam[16]); a base under a lookup that is not one of
 * A C G T is HAWK_E_CFD.
 *
 * hawk_resolve_groups is called on the handle IN PLACE OF hawk_resolve_download, before the next search on the set; it runs the
 * fill pass into device memory (44 bytes per kept guide, batched under HAWK_RESOLVE_BATCH_BYTES as the download) and after it
 * the handle counts as downloaded.  *out is a valid, empty result for zero kept guides.  HAWK_E_INVALID: a handle that was
 * already downloaded or grouped, or whose table a later search has overwritten; cfd_mm without cfd_pam.  HAWK_E_UNSUPPORTED: a
 * flank above 10, more than 2^32 - 1 kept guides.  HAWK_E_OOM: device memory the allocator cannot give.  On every status but
 * HAWK_OK *out stays NULL and nothing is left allocated.  hawk_ugroups_download copies what is not NULL (host or device
 * destinations; win[5][n_groups], member_off[n_groups + 1]).  The result owns its memory: it outlives the handle and the set, not
 * the context.  hawk_host_unphased_groups: the same from host arrays (the table's columns + `stop`, and src_row[n_kept] /
 * win[5][win_stride] of the kept guides, src_row ascending as hawk_resolve_download gives it) by the same header,
 * single-threaded, no device; outputs of group_cap / member_cap entries (win[5][group_cap]) are written when the counts fit,
 * else HAWK_E_CAPACITY with the need in *n_groups / *n_members (every output pointer may be NULL; all NULL: the call counts). */
typedef struct hawk_ugroups hawk_ugroups;
typedef struct {
  float fill_ms, keys_ms, sort_ms, heads_ms, emit_ms, total_ms; /* HIP events; heads_ms: the head flags and both scans */
  uint32_t n_batches, reserved;                                  /* batches of the fill pass */
  uint64_t n_kept, n_groups, n_members;
} hawk_ugroups_timing;
int hawk_resolve_groups(hawk_resolve* r, const double* cfd_mm, const double* cfd_pam, uint32_t flank_up, uint32_t flank_down,
                        hawk_ugroups** out, uint64_t* n_groups, uint64_t* n_members, hawk_ugroups_timing* timing);
int hawk_ugroups_download(hawk_ugroups* g, uint32_t* rep_src_row, uint32_t* hap, uint32_t* pos, uint8_t* strand, int64_t* start,
                          int64_t* stop, uint8_t* is_ref, double* cfdon, uint64_t* win, uint8_t* gc_num, uint8_t* gc_den,
                          uint64_t* member_off, uint32_t* member_hap);
void hawk_ugroups_free(hawk_ugroups* g);
int hawk_host_unphased_groups(const hawk_resolve_columns* cols, const int64_t* stop, const uint32_t* src_row, const uint64_t* win,
                              uint64_t n_kept, uint64_t win_stride, const double* cfd_mm, const double* cfd_pam, uint32_t flank_up,
                              uint32_t flank_down, uint64_t group_cap, uint64_t member_cap, uint32_t* rep_src_row, uint32_t* hap,
                              uint32_t* pos, uint8_t* strand, int64_t* start, int64_t* out_stop, uint8_t* is_ref, double* cfdon,
                              uint64_t* out_win, uint8_t* gc_num, uint8_t* gc_den, uint64_t* member_off, uint32_t* member_hap,
                              uint64_t* n_groups, uint64_t* n_members);

/* ---- the whole-region IUPAC rows of an unphased VCF, built on the device from the genotype text: what
 * add_variants_unphased (haplotypes.py:370-712) does for the SNV alleles - one region-long row per carrier, equal rows merged -
 * without a string on the host.  The rules are stated once, in csrc/hawk_ubuild.h, for the kernels (k_gt_parse_unphased, k_ub_sig,
 * k_ub_rows) and for hawk_host_unphased_rows.
 *
 * hawk_gt_parse_unphased: hawk_gt_parse's arguments and object (codes[n_lines][2*n_samples], hawk_gt_codes downloads them) under the
 *   unphased genotype rule.  With g = a column up to its first ':': part 0 of g split at '/' -> column 2s, part 1 -> column 2s + 1
 *   (0 REF, k = k-th ALT, 255 for '.', clamp at 254).  Flags per record, OR-ed over its first n_samples columns:
 *     1 = g is not exactly two '/'-separated parts, or holds a '|' (haploid, three or more parts, empty, phased);
 *     2 = the record does not have n_samples columns;
 *     4 = one of the first two '/'-parts is neither '.' nor all ASCII digits; its code stays 255 ("0|1" is one part that is no
 *         number: 1 and 4).
 * hawk_ubuild_lists: variants j = (record var_line[j], allele var_allele[j] in 1..254, offset var_off[j] in the region, the alt's
 *   4-bit mask var_mask[j] (A 1, C 2, G 4, T 8), ref base var_ref[j] 0-3), var_off ascending (HAWK_E_INVALID otherwise): the SNV
 *   alleles of the block in the caller's order.  Sample s carries j iff codes[var_line[j]][2s] or [2s + 1] equals var_allele[j]
 *   (_genotypes_to_samples(phased=False), slot 0).  One ascending list per SAMPLE is built on the device and stays there with the
 *   variant table; sample_off[n_samples + 1] (host) receives the CSR offsets, hawk_ubuild_lists_download the indices.  More than
 *   2^32 - 1 entries: HAWK_E_CAPACITY; more than 65535 x 1024 variants (the count kernel's grid): HAWK_E_UNSUPPORTED; nothing left
 *   allocated either way.
 * hawk_ubuild_signatures: sig[n_samples][2], 128 bits over each sample's merged sites (offset, REF's bit | the carried alts' bits),
 *   computed from the lists before any plane is written; a sample without entries gives (0, 0).  Equal rows have equal signatures;
 *   the caller compares the lists of samples that share one before it merges them.  A sample that carries an alt twice at one
 *   position (a duplicated record, or alt == ref behind another allele): HAWK_E_UNSUPPORTED with the first such variant in
 *   *decline_var - the host builder's sequential IUPAC encoding fails there, so the caller hands the interval to it.
 * hawk_ubuild_fill: rows [first_row, first_row + n_rows) of an ordinary set - each as long as row ref_row, which is packed already
 *   and not among them - become REF with the sites of sample row_sample[r]: at a carried position the A/C/G/T bits are REF's OR-ed
 *   with every carried alt's and the V bit is set; everything else, padding included, is REF's.  One pass, each word written
 *   once.  A site where REF does not hold exactly the variant's ref base in upper case: HAWK_E_UNSUPPORTED with the first such
 *   variant in *decline_var - nothing faults, the caller discards the set.  HAWK_E_INVALID, with nothing written: rows outside the
 *   set or of another length, a sample or a var_off the lists / REF do not have, a plan view, another context's set.
 * hawk_hapset_pack_ascii_rows: hawk_hapset_pack_ascii for rows [first_row, first_row + n_rows) alone (seq_off[n_rows + 1] into
 *   `seqs`): REF and the host-built window rows of such a set.  The other rows are not touched.
 * hawk_host_unphased_rows: the same rows from host arrays by the same header, single-threaded, no device: codes + variant table +
 *   REF bytes -> the distinct rows as cased ASCII (seqs[row_cap][ref_len]), their members (first carrier first, samples ascending),
 *   the per-sample lists and signatures, and the allele table of the rows (hawk_resolve_alleles' layout: key = (row_base + row)
 *   << 32 | offset, one entry per carried allele of the FIRST member, ref byte 0-3).  Counts are always written; an output that is
 *   not NULL needs its capacity (row_cap rows; entry_cap list entries / allele entries), else HAWK_E_CAPACITY.  Declines
 *   (HAWK_E_UNSUPPORTED, reason and variant in *decline): HAWK_UBUILD_OUTSIDE, HAWK_UBUILD_REF (checked for every CARRIED
 *   variant, whichever sample carries it), HAWK_UBUILD_REPEAT; HAWK_UBUILD_ENTRIES is HAWK_E_CAPACITY.  The remaining reasons are the caller's: it reads the flags and the fixed columns. */
#define HAWK_UBUILD_GENOTYPE 1 /* a record flag of the unphased parse */
#define HAWK_UBUILD_MNV 2      /* an equal-length allele longer than one base */
#define HAWK_UBUILD_BASE 3     /* an alt or ref base outside A/C/G/T */
#define HAWK_UBUILD_REF 4      /* REF does not hold exactly the record's ref base at a site */
#define HAWK_UBUILD_OUTSIDE 5  /* an SNV outside the region */
#define HAWK_UBUILD_ENTRIES 6  /* more than 2^32 - 1 list entries */
#define HAWK_UBUILD_REPEAT 7   /* a sample carries an alt twice at one position */
typedef struct hawk_ubuild hawk_ubuild;
typedef struct {
  const uint8_t* codes; /* [n_lines][2 * n_samples] */
  uint64_t n_lines;
  uint32_t n_samples, n_var;
  const uint32_t* var_line;
  const uint8_t* var_allele;
  const uint32_t* var_off;
  const uint8_t* var_mask;
  const uint8_t* var_ref;
  const char* ref; /* REF's bytes */
  uint32_t ref_len, row_base;
} hawk_ubuild_input;
typedef struct {
  uint64_t row_cap, entry_cap;
  char* seqs;              /* [row_cap][ref_len] */
  uint32_t* member_off;    /* [row_cap + 1] */
  uint32_t* member_sample; /* [n_samples] */
  uint64_t* sample_off;    /* [n_samples + 1] */
  uint32_t* list_idx;      /* [entry_cap] */
  uint64_t* sig;           /* [n_samples][2] */
  uint64_t* al_key;        /* [entry_cap] */
  uint32_t* al_off;        /* [entry_cap + 1] */
  uint8_t* al_ref;         /* [entry_cap] */
  uint64_t n_rows, n_members, n_entries, n_keys;
} hawk_ubuild_rows;
typedef struct {
  int32_t reason, reserved; /* HAWK_UBUILD_*, 0: none */
  int64_t var;              /* the first offending variant, or -1 */
} hawk_ubuild_decline;
int hawk_gt_parse_unphased(hawk_ctx* ctx, const uint8_t* text, uint64_t text_len, const uint64_t* line_off, const uint64_t* gt_off,
                           uint64_t n_lines, uint32_t n_samples, hawk_gt** out, float* kernel_ms);
int hawk_ubuild_lists(hawk_gt* g, const uint32_t* var_line, const uint8_t* var_allele, const uint32_t* var_off, const uint8_t* var_mask,
                      const uint8_t* var_ref, uint32_t n_var, uint64_t* sample_off, hawk_ubuild** out, float* kernel_ms);
int hawk_ubuild_lists_download(hawk_ubuild* u, uint32_t* idx);
int hawk_ubuild_signatures(hawk_ubuild* u, uint64_t* sig, int64_t* decline_var, float* kernel_ms);
int hawk_ubuild_fill(hawk_ubuild* u, hawk_hapset* hs, uint32_t ref_row, uint32_t first_row, uint32_t n_rows, const uint32_t* row_sample,
                     int64_t* decline_var, float* kernel_ms);
void hawk_ubuild_free(hawk_ubuild* u);
int hawk_hapset_pack_ascii_rows(hawk_hapset* hs, uint32_t first_row, uint32_t n_rows, const char* seqs, const uint64_t* seq_off,
                                uint64_t* bad_index);
int hawk_host_unphased_rows(const hawk_ubuild_input* in, hawk_ubuild_rows* out, hawk_ubuild_decline* decline);

/* ---- the indel-window rows of an unphased VCF on the device: what haplotypes.unphased_indel_windows builds per indel allele
 * inside the region and per carrier - the region cut to 100 nt either side of the indel, the indel and the carrier's SNVs inside
 * that window applied, equal rows of one indel merged - from the genotype codes (hawk_gt_parse_unphased) and the per-sample SNV
 * lists (hawk_ubuild_lists), without a record object or a row string.  The rules are stated once, in csrc/hawk_uwin.h (geometry,
 * which sites are applied and which survive, the ref check, the signature), for the kernels (hawk_uwin.hip) and for
 * hawk_host_unphased_windows.
 *
 * hawk_uwin_input: the indel alleles in (record, allele) order - the caller leaves out those outside the interval as given
 *   (indel_in_region) - each with its record line[k], allele number allele[k], NORMALISED offset off[k] in the region
 *   (adjust_multiallelic), ref_len[k] / alt_len[k], and pool_off[k]: where ub_base_index of its ref bases, then of its alt bases,
 *   starts in pool[pool_len] (255: outside A/C/G/T).  rank_sample[n_samples]: the sample columns in the order of their sorted
 *   names (a permutation); ref[region_len]: REF's bytes.
 * hawk_uwin_instances: an instance is one (indel, carrier).  Instances are ordered by (indel, rank of the carrier's name);
 *   inst_off[n_indel + 1] (host) receives their CSR offsets, hawk_uwin_download the carrier (its column) and the [lo, hi) range
 *   of the carrier's list entries (indices into the entries of hawk_ubuild_lists_download) with an offset inside the window.
 *   `u` stays the caller's and must outlive *out.  An indel nobody carries is never looked at.  Declines (HAWK_E_UNSUPPORTED,
 *   reason and indel in *decline; nothing left allocated): HAWK_UBUILD_WINDOW, HAWK_UBUILD_INDEL_BASE, and HAWK_UBUILD_REF for an
 *   alt of a deletion or a ref of an insertion longer than one base.  HAWK_E_INVALID: a line, allele number, pool range or rank the
 *   inputs do not have, `u` of another genotype block.
 * hawk_uwin_signatures: sig[n_inst][2], ub_sig_add over each instance's SURVIVING sites (an instance without one gives (0, 0)),
 *   and the ref check of every instance: HAWK_UBUILD_REF where the row does not hold the indel's ref (REF's base exactly, or a
 *   letter of the carrier's site there).
 * hawk_uwin_group: head[k] = the first instance of k's indel whose surviving sites equal k's one by one, k itself if there is
 *   none: the instances with head[k] == k, in order, are the distinct rows in first-seen order.  `sig` (host, [n_inst][2]) only
 *   proposes: whatever values the caller passes - all equal, say - the heads are the same.
 * hawk_uwin_fill: rows [first_row, first_row + n_rows) of an ordinary set become the window rows of instances row_inst[r]: source
 *   before the anchor | the alt with the V bit on every base | source behind the span, the surviving sites OR-ed in (ACGT bits
 *   REF's | the carried alts', V set); words past a row's length are zero, as hawk_hapset_pack_ascii leaves them.  Row ref_row
 *   holds REF, packed already.  HAWK_E_INVALID, nothing written: rows outside the set, REF among them, a row whose length is not
 *   the instance's, a REF row shorter than the region.
 * hawk_host_unphased_windows: the same instances, signatures, heads and rows from host arrays by the same header,
 *   single-threaded, no device.  The SNV lists are passed as hawk_host_unphased_rows (or the device) gave them.  Counts are
 *   always written; an output that is not NULL needs its capacity, else HAWK_E_CAPACITY.  out->forged_sig, if not NULL, replaces
 *   the signatures the grouping step reads (out->sig still receives the true ones). */
#define HAWK_UBUILD_WINDOW 8     /* an indel that does not fit the window the host builder cuts around it */
#define HAWK_UBUILD_INDEL_BASE 9 /* a base of an indel's ref or alt outside A/C/G/T */
typedef struct hawk_uwin hawk_uwin;
typedef struct {
  uint32_t n_indel, region_len;
  const uint32_t* line;
  const uint8_t* allele;
  const uint32_t* off;
  const uint32_t* ref_len;
  const uint32_t* alt_len;
  const uint32_t* pool_off;
  const uint8_t* pool;
  uint64_t pool_len;
  const uint32_t* rank_sample; /* [n_samples] */
  const char* ref;             /* [region_len] */
} hawk_uwin_input;
typedef struct {
  const uint8_t* codes; /* [n_lines][2 * n_samples] */
  uint64_t n_lines;
  uint32_t n_samples, n_var;
  const uint64_t* sample_off; /* [n_samples + 1] */
  const uint32_t* list_idx;
  const uint32_t* var_off;
  const uint8_t* var_mask;
  const uint8_t* var_ref;
} hawk_uwin_lists;
typedef struct {
  uint64_t inst_cap, row_cap, seq_cap;
  uint64_t* inst_off;    /* [n_indel + 1] */
  uint32_t* inst_sample; /* [inst_cap] */
  uint64_t* inst_lo;     /* [inst_cap] */
  uint64_t* inst_hi;     /* [inst_cap] */
  uint64_t* sig;         /* [inst_cap][2] */
  uint32_t* head;        /* [inst_cap] */
  const uint64_t* forged_sig; /* [n_inst][2] or NULL */
  char* seqs;            /* [seq_cap]: the distinct rows as cased ASCII, back to back */
  uint64_t* seq_off;     /* [row_cap + 1] */
  uint64_t n_inst, n_rows, n_seq;
} hawk_uwin_rows;
int hawk_uwin_instances(hawk_gt* g, hawk_ubuild* u, const hawk_uwin_input* in, uint64_t* inst_off, hawk_uwin** out,
                        hawk_ubuild_decline* decline, float* kernel_ms);
int hawk_uwin_download(hawk_uwin* w, uint32_t* inst_sample, uint64_t* inst_lo, uint64_t* inst_hi);
int hawk_uwin_signatures(hawk_uwin* w, uint64_t* sig, hawk_ubuild_decline* decline, float* kernel_ms);
int hawk_uwin_group(hawk_uwin* w, const uint64_t* sig, uint32_t* head, float* kernel_ms);
int hawk_uwin_fill(hawk_uwin* w, hawk_hapset* hs, uint32_t ref_row, uint32_t first_row, uint32_t n_rows, const uint32_t* row_inst,
                   float* kernel_ms);
void hawk_uwin_free(hawk_uwin* w);
int hawk_host_unphased_windows(const hawk_uwin_input* in, const hawk_uwin_lists* lists, hawk_uwin_rows* out, hawk_ubuild_decline* decline);

/* ---- PLM-CRISPR (scores/plm_crispr/train_general.py, class sgrna_net, forward with train=False; wrapper
 * scores/plm_crispr/plm_crispr.py:136-258): n guide+PAM 23-mers -> n fp32 scores, all arithmetic in fp32 (lin1 and lin3 on the
 * f32-input MFMA).  The 83 MB of parameters and the protein branch's result live in HBM behind a handle.
 *
 * hawk_plm_create: `params` is ONE packed fp32 block (host) in the order of sgrna_net().state_dict(), every tensor row-major in
 * its torch shape:
 *   conv1.weight[64][5][5] conv1.bias[64]  conv2.weight[64][64][5] conv2.bias[64]  conv3.weight[64][64][5] conv3.bias[64]
 *   conv4.weight[64][5][5] conv4.bias[64]
 *   text_cnn.convs.0.weight[128][1280][5] .bias[128]  text_cnn.convs.1.weight[128][1280][9] .bias[128]
 *   text_cnn.convs.2.weight[128][1280][13] .bias[128]
 *   lin1.weight[2048][7552] lin1.bias[2048]  lin3.weight[256][2048] lin3.bias[256]  lin4.weight[256][384] lin4.bias[256]
 *   lin5.weight[128][256] lin5.bias[128]  lin6.weight[1][128] lin6.bias[1]
 *   weight_net.0.weight[128][512] weight_net.0.bias[128]  weight_net.2.weight[2][128] weight_net.2.bias[2]
 * (HAWK_PLM_NPARAMS floats; offsets in crispr-hawk_amd/csrc/hawk_plm.h).  `protein` is the per-residue ESM embedding, L x 1280
 * fp32 (host); it is rounded through fp16 HERE (round to nearest even, as the reference's .to(torch.float16), plm_crispr.py:133),
 * so a caller that has rounded already loses nothing.  L < 13 (the widest text_cnn kernel) -> HAWK_E_INVALID.  The call runs the
 * protein branch once - text_cnn, lin4, relu, sigmoid - and keeps its 256 values; hawk_plm_protein copies them out.
 *
 * hawk_plm_score: `seqs` = n x len bytes (host, contiguous; A C G T N in either case), len must be 23 (HAWK_E_INVALID otherwise:
 * the reference's ValueError); the 36-nt scaffold is appended on the device.  Any other character -> HAWK_E_IUPAC (the
 * reference's KeyError), first writer wins, `out` is then unspecified.  Guides are processed `batch` at a time (0: 8192; at most
 * HAWK_PLM_MAX_BATCH) with a workspace of batch x (7552 + 2048 + 256) floats from the caching allocator; a guide's score does
 * not depend on batch, n or its place in `seqs`, bit for bit.  n = 0 is HAWK_OK.
 * hawk_plm_timing: ms4 (may be NULL) receives the device times {front, lin1, lin3, tail} summed over the batches of the last
 * hawk_plm_score that ran with timing enabled; `enable` switches it for the following calls (a timed call waits per batch). */
#define HAWK_PLM_NPARAMS (2 * (1600 + 64) + 2 * (20480 + 64) + 128 * 1280 * (5 + 9 + 13) + 3 * 128 + 2048 * 7552 + 2048 + \
                          256 * 2048 + 256 + 256 * 384 + 256 + 128 * 256 + 128 + 128 + 1 + 128 * 512 + 128 + 2 * 128 + 2)
#define HAWK_PLM_MAX_BATCH 65536u
typedef struct hawk_plm hawk_plm;
int hawk_plm_create(hawk_ctx* ctx, const float* params, const float* protein, uint32_t L, hawk_plm** out);
int hawk_plm_protein(hawk_plm* p, float out256[256]);
int hawk_plm_score(hawk_plm* p, const char* seqs, uint32_t len, uint64_t n, uint32_t batch, float* out);
int hawk_plm_timing(hawk_plm* p, int enable, float ms4[4]);
void hawk_plm_free(hawk_plm* p);

/* ---- BGZF members -> text (what readers._TextSource does with zlib, one member at a time): every member of a bgzipped VCF or BED
 * is an independent gzip member of at most 64 KiB of text, so a batch of them inflates in one call, one wavefront per member
 * (k_bz_inflate).  The rules - which headers, blocks and code sets are accepted (zlib's inflate decides), and that no member, however
 * malformed, is read or written outside its ranges - are stated once, in csrc/hawk_inflate.h, for the kernel and for
 * hawk_host_bgzf_inflate.  The CRC32 of the trailer is not checked (the zlib route never read it).
 *
 * Member k is in[c_off[k], c_off[k + 1]) - the whole gzip member, header and trailer - and its text goes to
 * out[u_off[k], u_off[k + 1]); both offset arrays have n_members + 1 entries and are relative to `in` / `out`, which are host
 * buffers (page-locked ones from hawk_host_alloc copy at link speed).  The device call uploads in[c_off[0], c_off[n_members]),
 * inflates into device memory of the caching allocator, downloads out[u_off[0], u_off[n_members]) and status[n_members] and
 * returns its workspace, all on the context's stream.  HAWK_OK when every member is HAWK_BZ_OK; HAWK_E_INVALID when any member
 * failed - status[] says which and why, the bytes of a failed member's range are unspecified, no byte outside it is touched.
 * HAWK_E_INVALID also, with nothing launched or written, for offsets that do not ascend, a member range outside in_bytes, or a
 * missing array.  n_members == 0 is HAWK_OK.  `timing` (may be NULL): the laps by the device's wall clock.
 * hawk_host_bgzf_inflate: the same header over the members on `threads` host threads (0: one per core, at most 32), no device. */
enum hawk_bz_status {
  HAWK_BZ_OK = 0,
  HAWK_BZ_HEADER = 1,      /* no gzip magic, or a compression method other than deflate */
  HAWK_BZ_UNSUPPORTED = 2, /* FLG is not exactly FEXTRA: not a member bgzip writes */
  HAWK_BZ_INPUT = 3,       /* the member ends before its stream does */
  HAWK_BZ_SIZE = 4,        /* ISIZE is not the range given for the text or exceeds 65536; the stream gives more or fewer bytes */
  HAWK_BZ_BLOCK = 5,       /* block type 3, or a stored block whose LEN and ~LEN disagree */
  HAWK_BZ_CODE = 6,        /* a code set zlib refuses, or a code an incomplete set does not hold */
  HAWK_BZ_SYMBOL = 7,      /* length symbol 286 / 287, distance symbol 30 / 31 */
  HAWK_BZ_DISTANCE = 8     /* a distance that reaches back past the member's first byte */
};
typedef struct {
  float upload_ms, inflate_ms, download_ms, total_ms;
  uint64_t in_bytes, out_bytes;
  uint32_t n_members, n_failed;
} hawk_bgzf_timing;
int hawk_bgzf_inflate(hawk_ctx* ctx, const uint8_t* in, uint64_t in_bytes, const uint64_t* c_off, const uint64_t* u_off,
                      uint32_t n_members, uint8_t* out, uint8_t* status, hawk_bgzf_timing* timing);
int hawk_host_bgzf_inflate(const uint8_t* in, uint64_t in_bytes, const uint64_t* c_off, const uint64_t* u_off, uint32_t n_members,
                           uint8_t* out, uint8_t* status, uint32_t threads);

#ifdef __cplusplus
}
#endif
#endif /* HAWK_H */
