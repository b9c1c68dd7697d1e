// hawk_collapse.hip — f2: which guide rows the report merges (reports.py:958-1008
// `_collapse_report_entries`: a pandas groupby over chr, start, stop, sgRNA_sequence, pam, strand,
// scores, gc_content, origin).  Scores and GC are functions of the sequence and of the REF guide at
// the same (start, strand), so two rows merge iff they agree in start, stop, strand, origin (REF
// haplotype or not) and in the case-preserving spacer+PAM — on the device: the five L-bit core
// slices of the window planes (the V plane is the case).  Equality of the stored (+ strand) cores is
// equality of the reverse-complemented guides the report prints.
//
//   k_collapse_keys   row -> 64-bit sort key  (start - base) << 32 | strand << 31 | hash31(core, stop, origin), and 32
//                     further bits of the same 64-bit hash of the row's identity (id2, table order)
//   rocprim::radix_sort_pairs (key, row id) over the bits in use - the low hash bits are dropped (zero in the key) so
//                     that start + strand + hash fill a whole number of 8-bit passes with >= 24 hash bits (a 4 Mb tile:
//                     48 bits, 6 passes instead of 7); stable, so equal keys keep table order (haplotype ascending)
//                     exact path: all 31 hash bits, and a stable sort by id2 in front, so that the rows of one key lie
//                     ordered by (id2, table order) - any number of different rows may share a (start, strand)
//   k_collapse_heads  neighbours in sorted order open a group when their keys differ or, with equal keys, their id2
//                     (two 4-byte gathers); counts heads by key and heads by identity - if they differ, two different
//                     rows of one (start, strand) collided in the 31 key bits and may interleave: the host layer
//                     re-runs with another seed.  Two different rows are merged only if they agree in start, strand
//                     and 63 hash bits (~10^-12 for a whole C4 contig); HAWK_COLLAPSE_EXACT=1 compares the FULL row
//                     keys instead (64-byte records written by k_collapse_keys, two 64-byte gathers per row: 8.5 of
//                     the 18 ms a 1.1 x 10^8-row tile took) - the tests run both
//   rocprim::exclusive_scan of the flags, k_collapse_groups: CSR offsets + GC counts of each group's guide
//                     (annotation.py:513-541: gc_fraction(guide.guide); Biopython's default drops ambiguous bases)
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "hawk_device.h"

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

struct RowKey {
  int64_t start, stop;
  uint64_t core[HAWK_PLANES];
  uint32_t sr;  // strand | origin << 1
};
// The compared slice is the spacer+PAM core widened by `up` bases on the guide's 5' side and `down` on its 3' side
// (0/0: the report without model scores; 4/3: the k-mer the model scorers read, scoring.py:50-67, so that rows whose
// flanks differ - and whose Azimuth / DeepCpf1 scores may therefore differ - stay separate, reports.py:978-1003).
// Rows are stored on the + strand: a strand-1 guide's 5' side is the window's right side.
__device__ __forceinline__ RowKey row_key(const GuideCols& c, const uint8_t* __restrict__ is_ref, uint64_t i, int L, int up, int down) {
  RowKey k;
  k.start = gc_start(c, i);
  k.stop = gc_stop(c, i);
  const uint32_t strand = gc_strand(c, i);
  k.sr = strand | ((uint32_t)(is_ref[gc_hap(c, i)] != 0) << 1);
  const int fl = strand ? down : up, fr = strand ? up : down;
  const int width = L + fl + fr;
  const uint64_t mask = width >= 64 ? ~0ull : ((1ull << width) - 1ull);
#pragma unroll
  for (int pl = 0; pl < HAWK_PLANES; ++pl) k.core[pl] = (gc_win(c, pl, i) >> (HAWK_PAD - fl)) & mask;
  return k;
}
__device__ __forceinline__ bool same_row(const RowKey& a, const RowKey& b) {
  bool s = a.start == b.start && a.stop == b.stop && a.sr == b.sr;
#pragma unroll
  for (int pl = 0; pl < HAWK_PLANES; ++pl) s = s && a.core[pl] == b.core[pl];
  return s;
}
// The 64-bit hash of a row's identity below (start, strand).  Its top 31 bits fill the sort key behind start - base and the strand
// (`hash_mask` drops the low ones the sort leaves out; the hash table keys on all 31), its low 32 are the rows' second word id2.
__device__ __forceinline__ uint64_t row_hash(const RowKey& k, uint64_t seed) {
  uint64_t h = seed;
#pragma unroll
  for (int pl = 0; pl < HAWK_PLANES; ++pl) h = mix64(h ^ k.core[pl]);
  return mix64(h ^ (uint64_t)k.stop ^ ((uint64_t)(k.sr >> 1) << 63));
}
__device__ __forceinline__ uint64_t sort_key(const RowKey& k, int64_t base, uint64_t h, uint32_t hash_mask) {
  return ((uint64_t)(k.start - base) << 32) | ((uint64_t)(k.sr & 1u) << 31) | ((h >> 33) & hash_mask);
}
// The full key as one 64-byte record: a pass that compares rows scattered over the table reads one line per row instead of nine
// (one per column).
struct KeyRecord { ulonglong4 a, b; };
__device__ __forceinline__ KeyRecord key_record(const RowKey& k) {
  return {make_ulonglong4((unsigned long long)k.start, (unsigned long long)k.stop, (unsigned long long)k.sr, k.core[0]),
          make_ulonglong4(k.core[1], k.core[2], k.core[3], k.core[4])};
}
__device__ __forceinline__ bool same4(const ulonglong4& a, const ulonglong4& b) {
  return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}
__device__ __forceinline__ bool same_record(const KeyRecord& x, const KeyRecord& y) { return same4(x.a, y.a) && same4(x.b, y.b); }
// (G/C bases, unambiguous bases) of row r's spacer inside the stored (+ strand) core: behind the PAM when the PAM comes first
// (right ^ strand)
__device__ __forceinline__ uchar2 spacer_gc(const GuideCols& c, uint64_t r, int guidelen, int pamlen, int right) {
  const bool pamfirst = (right != 0) != (gc_strand(c, r) != 0);
  const int sh = HAWK_PAD + (pamfirst ? pamlen : 0);
  const uint64_t m = guidelen >= 64 ? ~0ull : ((1ull << guidelen) - 1ull);
  const uint64_t A = (gc_win(c, 0, r) >> sh) & m, C = (gc_win(c, 1, r) >> sh) & m, G = (gc_win(c, 2, r) >> sh) & m,
                 T = (gc_win(c, 3, r) >> sh) & m;
  const uint64_t gc = (C | G) & ~(A | T);  // C, G, S
  const uint64_t at = (A | T) & ~(C | G);  // A, T, W
  return make_uchar2((uint8_t)__popcll(gc), (uint8_t)__popcll(gc | at));
}

__global__ __launch_bounds__(256) void k_collapse_keys(GuideCols c, const uint8_t* __restrict__ is_ref, uint64_t n, int L, int up, int down,
                                                       int64_t base, uint64_t seed, uint32_t hash_mask, uint32_t id_mask,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ id2,
                                                       ulonglong4* __restrict__ full /* exact mode, else null */) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const RowKey k = row_key(c, is_ref, i, L, up, down);
  if (full) reinterpret_cast<KeyRecord*>(full)[i] = key_record(k);  // the head pass compares neighbours of the SORTED order
  const uint64_t h = row_hash(k, seed);
  keys[i] = sort_key(k, base, h, hash_mask);
  vals[i] = (uint32_t)i;
  id2[i] = (uint32_t)h & id_mask;  // id_mask / hash_mask = 0: the test that forces hash collisions (HAWK_COLLAPSE_WEAK_HASH)
}

// exact path: the keys in the order of a stable sort of the rows by identity, so that the stable sort by key that follows leaves
// the rows of one key ordered by (identity, table order) - equal rows contiguous however many different rows share the key
__global__ __launch_bounds__(256) void k_collapse_by_id(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, uint64_t n,
                                                        uint64_t* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = keys[order[j]];
}

__global__ __launch_bounds__(256) void k_collapse_heads(const ulonglong4* __restrict__ full, const uint32_t* __restrict__ id2, uint64_t n,
                                                        const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        uint32_t* __restrict__ flags, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t hk = 0, hf = 0;
  if (j < n) {
    if (j == 0) {
      hk = hf = 1;
    } else {
      hk = keys[j] != keys[j - 1];
      if (!hk) {
        const uint64_t a = vals[j], b = vals[j - 1];
        if (full) {  // exact: rows of one key lie sorted by identity (k_collapse_by_id), so the identity counts as key here
          hk = id2[a] != id2[b];
          const KeyRecord* rec = reinterpret_cast<const KeyRecord*>(full);
          hf = hk || !same_record(rec[a], rec[b]);
        } else {
          hf = id2[a] != id2[b];
        }
      } else {
        hf = 1;
      }
    }
    flags[j] = hf;
  }
  const unsigned long long bk = __ballot(hk), bf = __ballot(hf);
  if ((threadIdx.x & 63) == 0) { atomicAdd(&s_cnt[0], (uint32_t)__popcll(bk)); atomicAdd(&s_cnt[1], (uint32_t)__popcll(bf)); }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// flags (0/1) and their exclusive scan gidx: a head at sorted position j opens group gidx[j]
__global__ __launch_bounds__(256) void k_collapse_groups(GuideCols c, uint64_t n, const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ flags, const uint32_t* __restrict__ gidx,
                                                         int guidelen, int pamlen, int right, uint64_t* __restrict__ group_off,
                                                         uint8_t* __restrict__ gc_num, uint8_t* __restrict__ gc_den) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n || !flags[j]) return;
  const uint32_t g = gidx[j];
  group_off[g] = j;
  const uchar2 gc = spacer_gc(c, vals[j], guidelen, pamlen, right);
  gc_num[g] = gc.x;
  gc_den[g] = gc.y;
}

// Every member of a group against the group's first member on the FULL key (start, stop, strand, origin, the five core
// slices): grouping by hash - 63 bits in either path above - is thereby checked, not trusted; one mismatch sends the call
// to the exact path.  `grp_a[j] + (grp_b ? grp_b[j] - 1 : 0)` = the group of sorted position j (sort path: exclusive scan of
// the head flags + the flag - 1; hash path: the sorted group numbers).  The head's key is shared by the group's members
// (L2), the member's own key is the one scattered read per row.
__global__ __launch_bounds__(256) void k_collapse_verify(GuideCols c, const uint8_t* __restrict__ is_ref, uint64_t n, int L, int up, int down,
                                                         const uint32_t* __restrict__ perm, const uint32_t* __restrict__ grp_a,
                                                         const uint32_t* __restrict__ grp_b, const uint64_t* __restrict__ group_off,
                                                         unsigned long long* __restrict__ mismatches) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (j < n) {
    const uint32_t g = grp_b ? grp_a[j] + grp_b[j] - 1u : grp_a[j];
    const uint64_t hj = group_off[g];
    if (hj != j) bad = !same_row(row_key(c, is_ref, perm[j], L, up, down), row_key(c, is_ref, perm[hj], L, up, down));
  }
  const unsigned long long b = __ballot(bad);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(mismatches, (unsigned long long)__popcll(b));
}
// The same check in TABLE order, for the hash-table path, which knows every row's group (slot -> group number): first the
// full key of every group's first member as one 64-byte record per group (k_collapse_head_keys: a few 10^5 records that
// stay in L2), then every row reads its own key where it lies (coalesced) and its group's record - three gathers per row
// instead of two scattered keys of nine columns each.
__global__ __launch_bounds__(256) void k_collapse_head_keys(GuideCols c, const uint8_t* __restrict__ is_ref, uint32_t G, int L, int up, int down,
                                                            const uint32_t* __restrict__ perm, const uint64_t* __restrict__ group_off,
                                                            ulonglong4* __restrict__ full) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  reinterpret_cast<KeyRecord*>(full)[g] = key_record(row_key(c, is_ref, perm[group_off[g]], L, up, down));
}
__global__ __launch_bounds__(256) void k_collapse_verify_rows(GuideCols c, const uint8_t* __restrict__ is_ref, uint64_t n, int L, int up, int down,
                                                              const uint32_t* __restrict__ slot_of_row, const uint32_t* __restrict__ slot2rank,
                                                              const ulonglong4* __restrict__ full, unsigned long long* __restrict__ mismatches) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const RowKey k = row_key(c, is_ref, i, L, up, down);
    const KeyRecord head = reinterpret_cast<const KeyRecord*>(full)[slot2rank[slot_of_row[i]]];  // both halves loaded before the compare
    bad = !same_record(head, key_record(k));
  }
  const unsigned long long bl = __ballot(bad);
  if (bl && (threadIdx.x & 63) == 0) atomicAdd(mismatches, (unsigned long long)__popcll(bl));
}
void hawk_launch_collapse_verify_rows(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint32_t G) {
  if (!k.n || !G) return;
  const int L = k.guidelen + k.pamlen;
  hipLaunchKernelGGL(k_collapse_head_keys, dim3((G + 255) / 256), dim3(256), 0, st, k.c, k.is_ref, G, L, k.flank_up, k.flank_down, v.vals + k.n,
                     v.group_off, (ulonglong4*)v.full);
  hipLaunchKernelGGL(k_collapse_verify_rows, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, st, k.c, k.is_ref, k.n, L, k.flank_up, k.flank_down,
                     v.slot_of_row, v.slot_rank, (const ulonglong4*)v.full, v.counters + 3);
}
// group of sorted position j: exclusive scan of the head flags + its own flag - 1
void hawk_launch_collapse_verify(hipStream_t st, const CollapseKey& k, const CollapseSortView& v) {
  if (!k.n) return;
  hipLaunchKernelGGL(k_collapse_verify, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, st, k.c, k.is_ref, k.n, k.guidelen + k.pamlen, k.flank_up,
                     k.flank_down, v.vals + k.n, v.group_index, v.head_flags, v.group_off, v.counters + 2);
}

// whole rows of a set against each other, all five planes: the check behind collapsing haplotypes on their content hash
__global__ __launch_bounds__(256) void k_rows_equal(HapSetDev hs, const uint32_t* __restrict__ ra, const uint32_t* __restrict__ rb,
                                                    uint8_t* __restrict__ equal) {
  __shared__ uint32_t s_diff;
  if (threadIdx.x == 0) s_diff = 0;
  __syncthreads();
  const size_t a = (size_t)ra[blockIdx.x] * hs.S, b = (size_t)rb[blockIdx.x] * hs.S;
  uint32_t d = 0;
  for (uint32_t w = threadIdx.x; w < hs.S; w += 256)
#pragma unroll
    for (int pl = 0; pl < HAWK_PLANES; ++pl) d |= hs.plane[pl][a + w] ^ hs.plane[pl][b + w];
  if (d) atomicOr(&s_diff, 1u);
  __syncthreads();
  if (threadIdx.x == 0) equal[blockIdx.x] = s_diff ? 0 : 1;
}
void hawk_launch_rows_equal(hipStream_t st, const HapSetDev& hs, uint32_t n_pairs, const uint32_t* ra, const uint32_t* rb, uint8_t* equal) {
  if (n_pairs) hipLaunchKernelGGL(k_rows_equal, dim3(n_pairs), dim3(256), 0, st, hs, ra, rb, equal);
}

// bytes of the full-key records (64 per row)
size_t hawk_collapse_full_bytes(uint64_t n) { return (size_t)n * 64; }

size_t hawk_collapse_temp_bytes(uint64_t n, unsigned begin_bit, unsigned end_bit) {
  size_t a = 0, b = 0, d = 0, e = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, begin_bit,
                                  end_bit, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), (hipStream_t)0);
  // the exact path: every hash bit in the key, and the sort by identity in front of it
  (void)rocprim::radix_sort_pairs(nullptr, d, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, end_bit,
                                  (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, e, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32,
                                  (hipStream_t)0);
  return std::max(std::max(a, b), std::max(d, e));
}

int hawk_launch_collapse(hipStream_t st, const CollapseKey& k, const CollapseSortView& v, unsigned begin_bit, unsigned end_bit, uint64_t seed,
                         bool exact, bool weak_hash) {
  const uint64_t n = k.n;
  const int L = k.guidelen + k.pamlen;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  void* const full = exact ? v.full : nullptr;
  hipLaunchKernelGGL(k_collapse_keys, grid, block, 0, st, k.c, k.is_ref, n, L, k.flank_up, k.flank_down, k.base, seed,
                     weak_hash ? 0u : (~((1u << begin_bit) - 1u) & 0x7fffffffu), weak_hash ? 0u : 0xffffffffu, v.keys, v.vals, v.id2, (ulonglong4*)full);
  size_t tb = v.temp_bytes;
  if (exact) {
    // Exact path (begin_bit = 0 here): rows by identity first (`head_flags` takes the sorted identities, free until the head pass),
    // then by key.  The head pass then needs no collision-free key: it opens a group where key, identity or full record change,
    // and counts a changed record under one key + identity (63 equal hash bits, never seen) for the host to answer with a seed.
    if (rocprim::radix_sort_pairs(v.temp, tb, v.id2, v.head_flags, v.vals, v.vals + n, n, 0, 32, st) != hipSuccess) return -2;
    hipLaunchKernelGGL(k_collapse_by_id, grid, block, 0, st, v.keys, v.vals + n, n, v.keys + n);
    tb = v.temp_bytes;
    if (rocprim::radix_sort_pairs(v.temp, tb, v.keys + n, v.keys, v.vals + n, v.vals, n, begin_bit, end_bit, st) != hipSuccess) return -2;
    if (hipMemcpyAsync(v.keys + n, v.keys, n * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(v.vals + n, v.vals, n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
      return -2;
  } else if (rocprim::radix_sort_pairs(v.temp, tb, v.keys, v.keys + n, v.vals, v.vals + n, n, begin_bit, end_bit, st) != hipSuccess) {
    return -2;
  }
  hipLaunchKernelGGL(k_collapse_heads, grid, block, 0, st, (const ulonglong4*)full, v.id2, n, v.keys + n, v.vals + n, v.head_flags, v.counters);
  tb = v.temp_bytes;
  if (rocprim::exclusive_scan(v.temp, tb, v.head_flags, v.group_index, 0u, n, rocprim::plus<uint32_t>(), st) != hipSuccess) return -2;
  hipLaunchKernelGGL(k_collapse_groups, grid, block, 0, st, k.c, n, v.vals + n, v.head_flags, v.group_index, k.guidelen, k.pamlen, k.right, v.group_off,
                     v.gc_num, v.gc_den);
  return 0;
}

// ---- group export: one representative row per group + every row's haplotype in group order, so that the host
// downloads group-level columns (74 B per report row) and 4 B per guide row instead of the whole table
__global__ __launch_bounds__(256) void k_collapse_export(GuideCols c, uint64_t n, uint64_t ng, const uint32_t* __restrict__ perm,
                                                         const uint64_t* __restrict__ group_off, GuideCols rep,
                                                         uint32_t* __restrict__ member_hap) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) member_hap[j] = gc_hap(c, perm[j]);
  if (j < ng) {
    const uint64_t r = perm[group_off[j]];  // the group's first member in table order
    rep.hap[j] = (uint32_t)r;               // the representative's row index in the full table
    rep.pos[j] = gc_pos(c, r);
    rep.strand[j] = (uint8_t)gc_strand(c, r);
    rep.start[j] = gc_start(c, r);
    rep.stop[j] = gc_stop(c, r);
    rep.flags[j] = (uint8_t)gc_flags(c, r);
    rep.cfdon[j] = gc_cfdon(c, r);
#pragma unroll
    for (int pl = 0; pl < HAWK_PLANES; ++pl) rep.win[(size_t)pl * rep.cap + j] = gc_win(c, pl, r);
  }
}
void hawk_launch_collapse_export(hipStream_t st, const GuideCols& c, uint64_t n, uint64_t ng, const uint32_t* perm,
                                 const uint64_t* group_off, const GuideCols& rep, uint32_t* member_hap) {
  const uint64_t m = n > ng ? n : ng;
  hipLaunchKernelGGL(k_collapse_export, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, c, n, ng, perm, group_off, rep, member_hap);
}

// ---------------------------------------------------------------------------------------------------------------
// Grouping through a hash table instead of a sort of all rows: when groups are far fewer than rows (a C4 tile: 1.1 x 10^8
// rows in 8.9 x 10^5 groups) the table (16 B per slot, a few MB) lives in the memory-side cache, every row finds its
// group with one or two probes, and what is sorted afterwards is (group number, row) on ~20 bits instead of the 48-bit
// row keys.  Same key, same identity test (63 hash bits; a 31-bit collision inside one (start, strand) is counted and
// answered with another seed) and the SAME output as the sort path: groups in key order, members in table order.
//   k_cg_insert  row -> key, identity; claim / find the key's slot (CAS), keep the smallest (identity, row) per slot
//   k_cg_occ + rocprim::exclusive_scan + k_cg_pack   occupied slots -> dense (key, slot) pairs, their number
//   rocprim::radix_sort_pairs (key, slot); k_cg_rank: slot -> position of its key = group number
//   k_cg_rowgid  row -> group number;  rocprim::radix_sort_pairs (group number, row);  k_cg_groups: CSR offsets + GC
struct CgSlot { unsigned long long key, idrow; };
#define CG_EMPTY 0xffffffffffffffffull
#define CG_MAXPROBE 64

__global__ __launch_bounds__(256) void k_cg_insert(GuideCols c, const uint8_t* __restrict__ is_ref, uint64_t n, int L, int up, int down,
                                                   int64_t base, uint64_t seed, CgSlot* __restrict__ T, uint32_t mask,
                                                   uint32_t* __restrict__ slot_of_row, unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // the table has turned out too small (far more groups than expected): the call is going to the sort path anyway
  if (__hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 4096ull) return;
  const RowKey k = row_key(c, is_ref, i, L, up, down);
  const uint64_t h = row_hash(k, seed);
  const unsigned long long key = sort_key(k, base, h, 0x7fffffffu);
  const unsigned long long idr = ((unsigned long long)(uint32_t)h << 32) | (uint32_t)i;
  uint32_t s = (uint32_t)mix64(key) & mask;
  for (int probe = 0; probe < CG_MAXPROBE; ++probe, s = (s + 1) & mask) {
    // One 16-byte read of the slot: the usual row finds its key and a smaller row of its identity there and is done.  A
    // plain load - what it returns may be stale, and every decision taken on it is either confirmed by an atomic (an
    // empty slot is claimed by CAS, a larger minimum replaced by atomicMin, both of which answer with the truth) or
    // stays right when the slot has moved on (keys never change; the minimum only falls; any earlier minimum is a row of
    // the same key to compare identities with).
    const ulonglong2 sl = *reinterpret_cast<const ulonglong2*>(&T[s]);
    unsigned long long cur = sl.x, old = sl.y;
    if (cur == CG_EMPTY) {
      const unsigned long long prev = atomicCAS(&T[s].key, CG_EMPTY, key);
      cur = prev == CG_EMPTY ? key : prev;
    }
    if (cur != key) continue;
    // the slot's (identity, row) minimum: rows arrive roughly in table order, so most leave without an atomic
    if (old == CG_EMPTY || old > idr) old = atomicMin(&T[s].idrow, idr);
    if (old != CG_EMPTY && (uint32_t)(old >> 32) != (uint32_t)(idr >> 32)) atomicAdd(&counters[0], 1ull);  // two identities, one key
    slot_of_row[i] = s;
    return;
  }
  atomicAdd(&counters[1], 1ull);  // table too full: the caller falls back to the sort
  slot_of_row[i] = 0;
}

__global__ __launch_bounds__(256) void k_cg_occ(const CgSlot* __restrict__ T, uint32_t C, uint32_t* __restrict__ flags) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s < C) flags[s] = T[s].key != CG_EMPTY ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_cg_pack(const CgSlot* __restrict__ T, uint32_t C, const uint32_t* __restrict__ flags,
                                                 const uint32_t* __restrict__ dense, uint64_t* __restrict__ gkey,
                                                 uint32_t* __restrict__ gslot, unsigned long long* __restrict__ counters) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= C) return;
  if (flags[s]) { gkey[dense[s]] = T[s].key; gslot[dense[s]] = s; }
  if (s == C - 1) counters[2] = (unsigned long long)dense[s] + flags[s];
}
__global__ __launch_bounds__(256) void k_cg_rank(const uint32_t* __restrict__ gslot_sorted, uint32_t G, uint32_t* __restrict__ slot2rank) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p < G) slot2rank[gslot_sorted[p]] = p;
}
__global__ __launch_bounds__(256) void k_cg_rowgid(const uint32_t* __restrict__ slot_of_row, const uint32_t* __restrict__ slot2rank, uint64_t n,
                                                   uint32_t* __restrict__ gid, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { gid[i] = slot2rank[slot_of_row[i]]; vals[i] = (uint32_t)i; }
}
__global__ __launch_bounds__(256) void k_cg_groups(GuideCols c, uint64_t n, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ gid,
                                                   int guidelen, int pamlen, int right, uint64_t* __restrict__ group_off,
                                                   uint8_t* __restrict__ gc_num, uint8_t* __restrict__ gc_den) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t g = gid[j];
  if (j && gid[j - 1] == g) return;
  group_off[g] = j;
  const uchar2 gc = spacer_gc(c, vals[j], guidelen, pamlen, right);  // of the group's first member in table order
  gc_num[g] = gc.x;
  gc_den[g] = gc.y;
}

size_t hawk_collapse_hash_temp_bytes(uint64_t n, uint32_t C) {
  size_t a = 0, b = 0, d = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)C, rocprim::plus<uint32_t>(), (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)C, 0, 64,
                                  (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, d, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 32,
                                  (hipStream_t)0);
  return std::max(a, std::max(b, d));
}

// stage 1: rows into the table, occupied slots packed; the host reads the counters before stage 2
int hawk_launch_collapse_hash1(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint64_t seed) {
  const uint32_t C = v.C;
  if (hipMemsetAsync(v.table, 0xff, (size_t)C * sizeof(CgSlot), st) != hipSuccess) return -2;
  hipLaunchKernelGGL(k_cg_insert, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, st, k.c, k.is_ref, k.n, k.guidelen + k.pamlen, k.flank_up,
                     k.flank_down, k.base, seed, (CgSlot*)v.table, C - 1, v.slot_of_row, v.counters);
  const dim3 cg((C + 255) / 256);
  hipLaunchKernelGGL(k_cg_occ, cg, dim3(256), 0, st, (const CgSlot*)v.table, C, v.occ);
  size_t tb = v.temp_bytes;
  if (rocprim::exclusive_scan(v.temp, tb, v.occ, v.dense, 0u, (size_t)C, rocprim::plus<uint32_t>(), st) != hipSuccess) return -2;
  hipLaunchKernelGGL(k_cg_pack, cg, dim3(256), 0, st, (const CgSlot*)v.table, C, v.occ, v.dense, v.gkey, v.gslot, v.counters);
  return 0;
}

// stage 2: groups in key order, every row's group number, then the tail below
int hawk_launch_collapse_hash2(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint32_t G, unsigned key_end_bit) {
  size_t tb = v.temp_bytes;
  if (rocprim::radix_sort_pairs(v.temp, tb, v.gkey, v.gkey + v.C, v.gslot, v.gslot + v.C, (size_t)G, 0, key_end_bit, st) != hipSuccess) return -2;
  hipLaunchKernelGGL(k_cg_rank, dim3((G + 255) / 256), dim3(256), 0, st, v.gslot + v.C, G, v.slot_rank);
  hipLaunchKernelGGL(k_cg_rowgid, dim3((unsigned)((k.n + 255) / 256)), dim3(256), 0, st, v.slot_of_row, v.slot_rank, k.n, v.gid, v.vals);
  return hawk_launch_collapse_expand(st, k, v, G);
}

// The tail of the grouping for rows that know their group number (stage 2 above; a cluster-searched table, whose rows inherit
// their template row's): rows sorted by (group, row) on the bits G groups need, CSR offsets and G/C counts from each group's first member.
size_t hawk_collapse_expand_temp_bytes(uint64_t n) {
  size_t d = 0;
  (void)rocprim::radix_sort_pairs(nullptr, d, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0, 32,
                                  (hipStream_t)0);
  return d;
}
static unsigned group_bits(uint64_t G) {
  unsigned gbits = 1;
  while (gbits < 32 && (G >> gbits) != 0) ++gbits;
  return gbits;
}
int hawk_launch_collapse_expand(hipStream_t st, const CollapseKey& k, const CollapseHashView& v, uint64_t G) {
  const uint64_t n = k.n;
  size_t tb = v.temp_bytes;
  if (rocprim::radix_sort_pairs(v.temp, tb, v.gid, v.gid + n, v.vals, v.vals + n, (size_t)n, 0, group_bits(G), st) != hipSuccess) return -2;
  hipLaunchKernelGGL(k_cg_groups, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, k.c, n, v.vals + n, v.gid + n, k.guidelen, k.pamlen, k.right,
                     v.group_off, v.gc_num, v.gc_den);
  return 0;
}
