// hawk_cldict.hip — the cluster dictionary of an expansion plan: the record heads and the kernels that cut every row's records into
// cluster instances and number the distinct clusters (k_cl_*), with their launchers.  hawk_csearch.hip has the overview and the
// searches that run from the dictionary; hawk_api_cldict.hip queues a build; hawk_cl.h holds what the three share.
#include <cstdlib>

#include "hawk_hx.h"

#define CL_MAXWALK 4096      // records per cluster the dictionary accepts (longer chains: the per-word search takes the plan)

__device__ __forceinline__ uint64_t cl_mix(uint64_t h, uint64_t v) {
  h = (h ^ v) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
// What the dictionary passes read of a record: {o, rs, alt_len} and WHICH variant it is (its index in the plan's variant table, from
// which hawk_expand.hip took rs, alt_len and the alt bases - so two records of one variant are the same allele at the same place in
// REF, by construction).  The plan keeps these 16 bytes as an array of their own (hawk_launch_hx_heads, at plan creation): the
// passes over every record are HBM-bound, and a 32-byte record fetched for half its bytes is twice the traffic.
struct __attribute__((aligned(16))) HxHead { int32_t o; uint32_t rs; uint32_t alt_len; uint32_t var; };
static_assert(sizeof(HxHead) == 16, "record head layout");
__global__ __launch_bounds__(256) void k_hx_heads(const HxVar* __restrict__ recs, const uint32_t* __restrict__ hv_idx, uint64_t n, uint4* __restrict__ heads) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint4 r = *reinterpret_cast<const uint4*>(recs + j);
  heads[j] = make_uint4(r.x, r.y, r.z, hv_idx[j]);
}
void hawk_launch_hx_heads(hipStream_t st, const void* recs, const uint32_t* hv_idx, uint64_t n, void* heads) {
  if (n) hipLaunchKernelGGL(k_hx_heads, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const HxVar*>(recs), hv_idx, n,
                            static_cast<uint4*>(heads));
}
__device__ __forceinline__ bool cl_starts(const HxHead* __restrict__ recs, uint64_t j, uint64_t lo) {
  if (j == lo) return true;
  const int32_t prev_end = recs[j - 1].o + (int32_t)recs[j - 1].alt_len;
  return recs[j].o - prev_end > CL_LINK;
}

// ---- dictionary -----------------------------------------------------------------------------------
// The rows' records are walked in CHUNKS of CL_CHUNK consecutive records of one row (a row of C3 has two): one workgroup per chunk
// in the two passes over the records, so that the grid is ten thousand equal pieces of work and not five thousand loops.
// Instances per row: its clusters + one closing instance (the clean run behind the last cluster); REF and rows that scan nothing
// (collapsed onto another row) have none - and no chunk.  (CL_ROW_U, CL_CHUNK: hawk_cl.h - the sizes of a build need them.)
// rows -> chunks, one workgroup: chunks per row, their offsets (ch_off[n_rows + 1]) and every chunk's row
__global__ __launch_bounds__(1024) void k_cl_chunks(const uint64_t* __restrict__ hv_off, const uint8_t* __restrict__ is_ref, const int32_t* __restrict__ ss,
                                                    const int32_t* __restrict__ se, uint32_t n_rows, uint32_t* __restrict__ ch_off,
                                                    uint32_t* __restrict__ ch_row, unsigned long long* stamp) {
  __shared__ uint32_t s_w[1024 / WAVE];
  hawk_stamp(stamp);  // a build begins here (ClResults::begin)
  uint32_t carry = 0;
  for (uint32_t r0 = 0; r0 < n_rows; r0 += 1024) {
    const uint32_t row = r0 + threadIdx.x;
    uint32_t nch = 0;
    if (row < n_rows) {
      const uint64_t len = hv_off[row + 1] - hv_off[row];
      const bool dead = is_ref[row] || se[row] <= ss[row];
      nch = dead ? 0u : (len ? (uint32_t)((len + CL_CHUNK - 1) / CL_CHUNK) : 1u);
    }
    uint32_t tot;
    const uint32_t ex = carry + block_excl_scan<1024 / WAVE>(nch, s_w, &tot);
    if (row < n_rows) {
      ch_off[row] = ex;
      for (uint32_t c = 0; c < nch; ++c) ch_row[ex + c] = row;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) ch_off[n_rows] = carry;
}
// (ClInst, ClUniq - per instance, per distinct cluster - and the table's ClSlot and the list's ClListed: hawk_cl.h)
#define CL_PENDING 0x80000000u
// Nine clusters in ten are ONE record of a shareable instance: such a cluster IS its variant, and its number is the variant's
// index - no table, no comparison.  Which instance describes it does not matter: every such instance whose variant the first rows
// have not described yet writes {its record, its row} - ONE aligned 64-bit store, so whichever write lands last is whole.
// Every other instance with a cluster - several records, or windows that could meet a bound of its row - is put on a LIST by the
// cutting pass (its place known without an atomic: the counting pass counts those too) and goes through a hash table of 32-byte
// slots in passes of their own over that list: {hash key (0: free), -} for the pass that enters them, {cluster number + 1 (0: not yet
// numbered), records | class << 16 of the instance that opened the slot, REF position of its first allele, its first variant} -
// ONE 16-byte piece, one request - for the pass that compares; these are numbered behind the variants, in the order they are met
// (the order carries no meaning: every table a search writes is in instance order).
// Why this shape: the passes are bound by the NUMBER of requests to L2 (a 4-byte gather costs what a 64-byte line costs: ~1.3 x 10^11
// requests/s at best) and by same-address atomics (~10 ns each, whoever waits for them) - not by bytes and not by arithmetic.

// One cluster start: the walk over its records and what follows from it.  r0 / rp: the record at j and the one before it; nx1 / nx2:
// the records of lanes + 1, + 2 (a cluster's second and third record are the records of the lanes above - nine clusters in ten are
// one record, ninety-nine in a hundred at most three: no dependent load until a cluster is longer or crosses the wave's end).
struct ClCut { int32_t o_first, o_end, pa, rb; uint32_t n, cls; unsigned long long key; bool run_inside, too_long; };
#ifdef HAWK_TEST_HOOKS  // libhawk_hip_hooks.so only (tests/hooks_cluster_check.py): HAWK_CLUSTER_WEAK_HASH=1 keys a cluster by its FIRST
// record alone, so that clusters which share it collide in the table and k_cl_uid's record-by-record compare has something to catch
__device__ uint32_t cl_weak_hash;
#endif
__device__ __forceinline__ ClCut cl_cut(const HxHead* __restrict__ recs, uint64_t lo, uint64_t hi, uint64_t j, const uint4& r0, const uint4& rp,
                                         const uint4& nx1, const uint4& nx2, uint32_t lane, int32_t ss, int32_t se, int32_t hl, uint32_t row) {
  ClCut c;
  // A cluster's identity is WHERE in REF its first allele starts and, record by record, which variant it is (and so which allele,
  // where it lies and where REF resumes behind it) and where it lies relative to the first - hashed here, compared record by
  // record before two instances share a cluster (k_cl_uid).
  c.o_first = (int32_t)r0.x; c.pa = 0; c.rb = 0; c.too_long = false;
  if (j > lo) { c.pa = (int32_t)rp.x + (int32_t)rp.z; c.rb = (int32_t)rp.y - c.pa; }
  uint64_t e = j + 1, h = cl_mix(0x243F6A8885A308D3ull, (uint64_t)(uint32_t)(c.o_first + c.rb));
  h = cl_mix(h, (uint64_t)r0.w | ((uint64_t)r0.z << 32));
  h = cl_mix(h, (uint64_t)r0.y);
#ifdef HAWK_TEST_HOOKS
  const uint64_t h_first = h;
#endif
  c.n = 1;
  c.o_end = (int32_t)r0.x + (int32_t)r0.z;  // end of the cluster's last allele so far
  bool open = e < hi;                        // the record at e may still belong to the cluster
  while (open) {
    const uint32_t ahead = (uint32_t)(e - j);
    uint4 r;
    if (ahead == 1 && lane + 1 < WAVE) r = nx1;
    else if (ahead == 2 && lane + 2 < WAVE) r = nx2;
    else r = *reinterpret_cast<const uint4*>(recs + e);
    if ((int32_t)r.x - c.o_end > CL_LINK) break;      // it starts the next cluster
    if (c.n >= CL_MAXWALK) { c.too_long = true; break; }  // a chain too long for this path
    h = cl_mix(h, (uint64_t)r.w | ((uint64_t)r.z << 32));
    h = cl_mix(h, (uint64_t)r.y | ((uint64_t)(uint32_t)((int32_t)r.x - c.o_first) << 32));
    c.o_end = (int32_t)r.x + (int32_t)r.z;
    ++c.n; ++e;
    open = e < hi;
  }
#ifdef HAWK_TEST_HOOKS
  if (cl_weak_hash) h = h_first;
#endif
  // window starts the cluster can touch: [o_first - (L - 1), o_end), L <= 44; the ranges they are tested against
  // (search_guides.py:49-84, 395-420) are [ss - po, se - po) and [PAD, len - L - PAD], po in {0, guidelen}
  const bool outside = c.o_end <= ss - 44 || c.o_first - 43 >= se;
  const bool interior = c.o_first - 43 >= (ss > HAWK_PAD ? ss : HAWK_PAD) && c.o_first >= 64 && c.o_end <= se - 44 &&
                        c.o_end <= hl - 44 - HAWK_PAD + 1 && c.o_end + 128 <= hl;
  c.key = h; c.cls = 1;
  if (outside) { c.cls = 0; c.key = 0; }
  else if (!interior) { c.cls = 2; c.key = cl_mix(h ^ 0xA4093822299F31D0ull, (uint64_t)row + 1u); }
  if (c.cls && c.key == 0) c.key = 1;
  // the clean run in front, [pa, o_first - (L - 1)), lies inside every range of both strands for every geometry: its count
  // then needs neither the row nor its bounds (bit 31 of the instance's pa)
  c.run_inside = c.pa >= (ss > HAWK_PAD ? ss : HAWK_PAD) && c.o_first <= se - 44 && c.o_first <= hl - 44 - HAWK_PAD + 1;
  return c;
}
__device__ __forceinline__ uint4 shfl_down4(const uint4& v, int d) {
  return make_uint4((uint32_t)__shfl_down((int)v.x, d), (uint32_t)__shfl_down((int)v.y, d), (uint32_t)__shfl_down((int)v.z, d),
                    (uint32_t)__shfl_down((int)v.w, d));
}

// chunk b: the instances it opens (its cluster starts + the closing instance in a row's last chunk) and how many of them go on the list
__global__ __launch_bounds__(256) void k_cl_count(const HxHead* __restrict__ recs, const uint64_t* __restrict__ hv_off, const uint32_t* __restrict__ hap_len,
                                                  const int32_t* __restrict__ ss_, const int32_t* __restrict__ se_, const uint32_t* __restrict__ ch_off,
                                                  const uint32_t* __restrict__ ch_row, uint32_t n_rows, uint32_t n_var, uint32_t* __restrict__ cnt,
                                                  uint32_t* __restrict__ lcnt, unsigned long long* __restrict__ var_desc, uint32_t n_head) {
  __shared__ uint32_t s_w[256 / WAVE];
  const uint32_t b = blockIdx.x;
  if (b >= ch_off[n_rows]) return;  // (launched over the bound on the chunks: their number is only known on the device; workgroup-uniform)
  const uint32_t row = ch_row[b];
  const uint64_t lo = hv_off[row], hi = hv_off[row + 1];
  const uint64_t b0 = lo + (uint64_t)(b - ch_off[row]) * CL_CHUNK;
  const int32_t ss = ss_[row], se = se_[row], hl = (int32_t)hap_len[row];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  uint32_t c = 0;  // starts | listed << 16
  if (hi > lo) {
    uint4 r0[CL_ROW_U], rp[CL_ROW_U];
#pragma unroll
    for (int u = 0; u < CL_ROW_U; ++u) {
      const uint64_t j = b0 + u * 256 + threadIdx.x;
      const uint64_t jc = j < hi ? j : hi - 1;
      r0[u] = *reinterpret_cast<const uint4*>(recs + jc);
      rp[u] = *reinterpret_cast<const uint4*>(recs + (jc > lo ? jc - 1 : jc));
    }
    auto one = [&](const int u) __attribute__((always_inline)) {
      const uint4 nx1 = shfl_down4(r0[u], 1), nx2 = shfl_down4(r0[u], 2);  // (every lane takes part in the exchange)
      const uint64_t j = b0 + u * 256 + threadIdx.x;
      if (!(j < hi && (j == lo || (int32_t)r0[u].x - ((int32_t)rp[u].x + (int32_t)rp[u].z) > CL_LINK))) return;
      const ClCut k = cl_cut(recs, lo, hi, j, r0[u], rp[u], nx1, nx2, lane, ss, se, hl, row);
      const uint32_t v = r0[u].w;
      const bool simple = k.n == 1 && k.cls == 1 && v < n_var;
      c += 1u + ((k.cls != 0 && !simple) ? 0x10000u : 0u);
      // the first rows describe what they carry, before the cutting pass and its crowd: one aligned 64-bit store, whichever lands last
      // is whole (row >= 1: never 0).  Which variants are described goes into the bitmap beside the scan (hawk_launch_scan2_u32): an
      // atomic OR per instance here, as the head launch of the cutting pass once did it, cost this pass 13 us on C3
      if (simple && b < n_head) var_desc[v] = (unsigned long long)(uint32_t)j | ((unsigned long long)row << 32);
    };
    static_assert(CL_ROW_U == 4, "one call per slice");
    one(0); one(1); one(2); one(3);
  }
  uint32_t tot;
  (void)block_excl_scan<256 / WAVE>(c, s_w, &tot);
  if (threadIdx.x == 0) { cnt[b] = (tot & 0xffffu) + (b + 1 == ch_off[row + 1] ? 1u : 0u); lcnt[b] = tot >> 16; }
}

// Cuts the rows' chunks into instances.  A one-record shareable instance IS its variant (uid = the variant's index);
// any other instance with a cluster goes on the list for k_cl_enter / k_cl_uid.  No atomic that anybody waits for:
// places in the instance arrays and on the list come from the counting pass; the variants the FIRST rows described there (k_cl_count)
// have their bit set (k_scan2_u32), and this pass reads those bits through LDS (a chunk's records are consecutive variants-in-a-row, ascending: one window of
// the bitmap, C3: all 4 KB of it, loaded once per workgroup) and describes what they left.
#define CL_BM_WORDS 4096  // the window's LDS words (16 KB); a chunk that spans more variants asks the bitmap in HBM directly
__global__ __launch_bounds__(256) void k_cl_fill(const HxHead* __restrict__ recs, const uint64_t* __restrict__ hv_off,
                                                 const uint32_t* __restrict__ hap_len, const int32_t* __restrict__ ss_,
                                                 const int32_t* __restrict__ se_, const uint32_t* __restrict__ ch_off,
                                                 const uint32_t* __restrict__ ch_row, const uint32_t* __restrict__ inst_base,
                                                 const uint32_t* __restrict__ list_base, ClInst ci, unsigned long long* __restrict__ var_desc,
                                                 const uint32_t* __restrict__ claim_bits, uint32_t n_var, ClListed* __restrict__ cx_list, uint32_t* __restrict__ status,
                                                 uint32_t n_rows) {
  __shared__ uint32_t s_c[256 / WAVE][CL_ROW_U];  // cluster starts per wave and record slice
  __shared__ uint32_t s_l[256 / WAVE][CL_ROW_U];  // ... and how many of them are listed
  __shared__ uint32_t s_bm[CL_BM_WORDS];
  const uint32_t b = blockIdx.x;
  if (b >= ch_off[n_rows]) return;  // (launched over the bound on the chunks; workgroup-uniform)
  const uint32_t row = ch_row[b];
  const uint64_t lo = hv_off[row], hi = hv_off[row + 1];
  const uint64_t b0 = lo + (uint64_t)(b - ch_off[row]) * CL_CHUNK;
  const int32_t ss = ss_[row], se = se_[row], hl = (int32_t)hap_len[row];
  const uint32_t lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const uint32_t at = inst_base[b], lat = list_base[b];
  uint32_t round_tot = 0;
  if (hi > lo) {
    // the chunk's window of the variants' bitmap (the first chunks' variants, described by the counting pass; nothing here writes it)
    const uint64_t b1 = b0 + CL_CHUNK < hi ? b0 + CL_CHUNK : hi;
    const uint32_t v_lo = recs[b0].var, v_hi = recs[b1 - 1].var;
    const uint32_t w_lo = v_lo >> 5, n_w = v_hi >= v_lo && v_hi < n_var ? (v_hi >> 5) - w_lo + 1u : 0u;
    const bool bm_lds = n_w != 0u && n_w <= CL_BM_WORDS;  // workgroup-uniform
    if (bm_lds) for (uint32_t w = threadIdx.x; w < n_w; w += 256) s_bm[w] = claim_bits[w_lo + w];
    // CL_ROW_U slices of 256 consecutive records: every thread's record and the one before it, asked for at once
    uint4 r0[CL_ROW_U], rp[CL_ROW_U];
    bool st[CL_ROW_U];
    unsigned long long bal[CL_ROW_U];
#pragma unroll
    for (int u = 0; u < CL_ROW_U; ++u) {
      const uint64_t j = b0 + u * 256 + threadIdx.x;
      const uint64_t jc = j < hi ? j : hi - 1;
      r0[u] = *reinterpret_cast<const uint4*>(recs + jc);                        // {o, rs, alt_len, variant}
      rp[u] = *reinterpret_cast<const uint4*>(recs + (jc > lo ? jc - 1 : jc));
    }
#pragma unroll
    for (int u = 0; u < CL_ROW_U; ++u) {
      const uint64_t j = b0 + u * 256 + threadIdx.x;
      st[u] = j < hi && (j == lo || (int32_t)r0[u].x - ((int32_t)rp[u].x + (int32_t)rp[u].z) > CL_LINK);
      bal[u] = __ballot(st[u]);
      if (lane == 0) s_c[wv][u] = (uint32_t)__popcll(bal[u]);
    }
    __syncthreads();  // (also publishes the bitmap window)
    uint32_t pre[CL_ROW_U];  // starts of the slices / waves in front of this wave's part of slice u (slice-major = record order)
#pragma unroll
    for (int u = 0; u < CL_ROW_U; ++u) {
      pre[u] = round_tot;
#pragma unroll
      for (int w = 0; w < 256 / WAVE; ++w) {
        const uint32_t x = s_c[w][u];
        if (w < (int)wv) pre[u] += x;
        round_tot += x;
      }
    }
    uint4 ea[CL_ROW_U], eb[CL_ROW_U];  // the list entries of this thread's starts, if they are listed
    bool listed[CL_ROW_U];
    unsigned long long lbal[CL_ROW_U];
    auto cut = [&](const int u) __attribute__((always_inline)) {  // (called once per slice with a constant: the slices' registers stay registers)
      const uint4 nx1 = shfl_down4(r0[u], 1), nx2 = shfl_down4(r0[u], 2);  // (every lane takes part in the exchange)
      listed[u] = false;
      ea[u] = make_uint4(0u, 0u, 0u, 0u); eb[u] = ea[u];
      if (st[u]) {
        const uint64_t j = b0 + u * 256 + threadIdx.x;
        const uint32_t i = at + pre[u] + (uint32_t)__popcll(bal[u] & ((1ull << lane) - 1ull));
        const ClCut k = cl_cut(recs, lo, hi, j, r0[u], rp[u], nx1, nx2, lane, ss, se, hl, row);
        if (k.too_long) atomicOr(status, 1u);
        ci.o[i] = k.o_first; ci.row[i] = row; ci.pa[i] = k.pa | (k.run_inside ? (int32_t)0x80000000 : 0); ci.rb[i] = k.rb;
        const uint32_t v = r0[u].w;
        const bool simple = k.n == 1 && k.cls == 1 && v < n_var;  // the cluster is its variant
        if (!k.cls) ci.uid[i] = CL_NONE;
        if (simple) {
          ci.uid[i] = v;
          const uint32_t bit = 1u << (v & 31u);
          if (!((bm_lds ? s_bm[(v >> 5) - w_lo] : claim_bits[v >> 5]) & bit))  // nobody among the first rows carries it as a cluster of its own
            var_desc[v] = (unsigned long long)(uint32_t)j | ((unsigned long long)row << 32);  // (row >= 1: never 0; whichever lands last is whole: one aligned 64-bit store)
        }
        listed[u] = k.cls != 0 && !simple;
        ea[u] = make_uint4(i, (uint32_t)k.key, (uint32_t)(k.key >> 32), (uint32_t)j);
        eb[u] = make_uint4(k.n | (k.cls << 16), (uint32_t)(k.o_first + k.rb), (uint32_t)k.o_first, v);
      }
      lbal[u] = __ballot(listed[u]);
      if (lane == 0) s_l[wv][u] = (uint32_t)__popcll(lbal[u]);
    };
    static_assert(CL_ROW_U == 4, "one call per slice");
    cut(0); cut(1); cut(2); cut(3);
    __syncthreads();
    uint32_t lpre = lat;  // places on the list: slice-major, like the instances
#pragma unroll
    for (int u = 0; u < CL_ROW_U; ++u) {
      uint32_t mine = lpre;
#pragma unroll
      for (int w = 0; w < 256 / WAVE; ++w) {
        const uint32_t x = s_l[w][u];
        if (w < (int)wv) mine += x;
        lpre += x;
      }
      if (listed[u]) {
        uint4* dst = reinterpret_cast<uint4*>(cx_list + mine + (uint32_t)__popcll(lbal[u] & ((1ull << lane) - 1ull)));
        dst[0] = ea[u]; dst[1] = eb[u];
      }
    }
  }
  if (threadIdx.x == 0 && b + 1 == ch_off[row + 1]) {  // the row's last chunk: the closing instance
    const uint32_t i = at + round_tot;
    int32_t pa = 0, rb = 0;
    if (hi > lo) { pa = recs[hi - 1].o + (int32_t)recs[hi - 1].alt_len; rb = (int32_t)recs[hi - 1].rs - pa; }
    ci.o[i] = CL_FAR; ci.row[i] = row; ci.pa[i] = pa; ci.rb[i] = rb; ci.uid[i] = CL_NONE;
  }
}

// The listed instances into the table, CL_UID_U per thread (their looks in flight together; an ordinary cached load first: a stale
// answer only sends the instance on to the atomic, which tells the truth).  The instance that takes a free slot opens a new distinct
// cluster: it draws the next number behind the variants (one atomic per WORKGROUP), describes the cluster and fills in the slot; one
// that finds its key there notes CL_PENDING | slot for k_cl_uid.
#define CL_UID_U 4
__global__ __launch_bounds__(256) void k_cl_enter(const ClListed* __restrict__ cx_list, const uint32_t* __restrict__ n_list_dev, uint32_t t_first,
                                                  uint32_t t_end, ClSlot* tab, uint32_t mask, uint32_t max_probe, uint32_t fail_bit,
                                                  uint32_t* __restrict__ inst_uid, const uint32_t* __restrict__ inst_row, uint32_t* __restrict__ cx_state,
                                                  ClUniq cu, uint32_t* n_table, uint32_t n_var, uint32_t u_cap, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_n[256 / WAVE][CL_UID_U];
  __shared__ uint32_t s_base;
  const uint32_t n_list = *n_list_dev < t_end ? *n_list_dev : t_end;  // (launched over the bound on the list)
  const uint32_t t0 = t_first + blockIdx.x * (256 * CL_UID_U) + threadIdx.x;
  if (t_first + blockIdx.x * (256 * CL_UID_U) >= n_list) return;  // workgroup-uniform
  const uint32_t lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  uint4 ent[CL_UID_U], lk[CL_UID_U];
  uint32_t sl[CL_UID_U];
  bool on[CL_UID_U], won[CL_UID_U];
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    const uint32_t t = t0 + u * 256;
    on[u] = t < n_list;
    ent[u] = *reinterpret_cast<const uint4*>(cx_list + (on[u] ? t : t_first));  // {instance, key, first record}
  }
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    const unsigned long long k = (unsigned long long)ent[u].y | ((unsigned long long)ent[u].z << 32);
    sl[u] = (uint32_t)(k >> 17) & mask;
    lk[u] = *reinterpret_cast<const uint4*>(tab + sl[u]);
  }
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    won[u] = false;
    if (!on[u]) continue;
    const unsigned long long k = (unsigned long long)ent[u].y | ((unsigned long long)ent[u].z << 32);
    uint4 e0 = lk[u];
    uint32_t s = sl[u];
    bool placed = false;
    // (the full-size table has >= 2 slots per instance: a free slot is met long before the bound; a first attempt with a table sized
    // for the distinct clusters expected gives up after max_probe slots and the host repeats the passes with the full size)
    for (uint32_t probe = 0; probe <= mask && probe < max_probe; ++probe) {
      if (probe) e0 = *reinterpret_cast<const uint4*>(tab + s);
      unsigned long long c = (unsigned long long)e0.x | ((unsigned long long)e0.y << 32);
      if (c == 0ull) {  // (a slot never changes hands once taken: any other value seen is final)
        c = atomicCAS(&tab[s].key, 0ull, k);
        won[u] = c == 0ull;
      }
      if (c == 0ull || c == k) { placed = true; break; }
      s = (s + 1u) & mask;
    }
    sl[u] = s;
    const uint32_t t = t0 + u * 256;
    if (!placed) { won[u] = false; cx_state[t] = CL_NONE; inst_uid[ent[u].x] = CL_NONE; atomicOr(status, fail_bit); continue; }  // full-size table: cannot happen
    cx_state[t] = won[u] ? CL_NONE : (CL_PENDING | s);
  }
  // the new distinct clusters of this workgroup draw their numbers with one atomic
  unsigned long long wb[CL_UID_U];
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) { wb[u] = __ballot(won[u]); if (lane == 0) s_n[wv][u] = (uint32_t)__popcll(wb[u]); }
  __syncthreads();
  uint32_t tot = 0, mine[CL_UID_U];
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    mine[u] = tot;
#pragma unroll
    for (int w = 0; w < 256 / WAVE; ++w) { const uint32_t x = s_n[w][u]; if (w < (int)wv) mine[u] += x; tot += x; }
  }
  if (!tot) return;  // workgroup-uniform
  if (threadIdx.x == 0) s_base = atomicAdd(n_table, tot);
  __syncthreads();
  const uint32_t base = n_var + s_base;
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    if (!won[u]) continue;
    const uint32_t un = base + mine[u] + (uint32_t)__popcll(wb[u] & ((1ull << lane) - 1ull));
    const uint32_t i = ent[u].x;
    if (un >= u_cap) { inst_uid[i] = CL_NONE; atomicOr(status, fail_bit); continue; }  // (more distinct clusters than slots: cannot happen)
    const uint4 e1 = reinterpret_cast<const uint4*>(cx_list + (t0 + u * 256))[1];  // {records | class, REF position, row position, first variant}
    *reinterpret_cast<uint4*>(&tab[sl[u]].up1) = make_uint4(un + 1u, e1.x, e1.y, e1.w);
    inst_uid[i] = un;
    cu.rec[un] = ent[u].w; cu.n[un] = e1.x & 0xffffu; cu.row[un] = inst_row[i]; cu.o[un] = (int32_t)e1.z;
  }
}

// what a search needs of every distinct cluster: for a variant's cluster the description unpacked from the one word its describer
// left (a variant that is nowhere a cluster of its own stays a hole: u_n = 0); for all of them the template rows they can have and
// the position-map segment their searches start from
__global__ __launch_bounds__(256) void k_cl_describe(const uint32_t* __restrict__ n_table_dev, uint32_t n_var, uint32_t u_cap,
                                                     const unsigned long long* __restrict__ var_desc, ClUniq cu, const HxHead* __restrict__ recs,
                                                     const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_rel,
                                                     uint32_t* __restrict__ n_variant_clusters, unsigned long long* __restrict__ slots_total) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  uint32_t span_u = 0;
  const uint32_t nu = n_var + *n_table_dev < u_cap ? n_var + *n_table_dev : u_cap;  // (launched over the bound on the distinct clusters)
  bool variant_cluster = false;
  if (u < nu) {
    uint32_t n, r, row;
    int32_t o_first;
    if (u < n_var) {
      const unsigned long long d = var_desc[u];
      variant_cluster = d != 0ull;
      r = (uint32_t)d; row = (uint32_t)(d >> 32); n = variant_cluster ? 1u : 0u;
      o_first = variant_cluster ? recs[r].o : 0;
      cu.rec[u] = r; cu.n[u] = n; cu.row[u] = row; cu.o[u] = o_first;
    } else {
      n = cu.n[u]; r = cu.rec[u]; row = cu.row[u]; o_first = cu.o[u];
    }
    if (n == 0) { cu.span2[u] = 0; cu.seg[u] = 0; }
    else {
      const int32_t o_end = recs[r + n - 1].o + (int32_t)recs[r + n - 1].alt_len;
      span_u = 2u * ((uint32_t)(o_end - o_first) + CL_LINK);  // rows the cluster can have: window starts [o_first - L + 1, o_end) x 2 strands
      cu.span2[u] = span_u;
      // the position-map segment in force CL_LINK + PAD positions in front of the cluster: every position a search asks for lies behind it
      const uint32_t rel = o_first > CL_LINK + HAWK_PAD ? (uint32_t)(o_first - CL_LINK - HAWK_PAD) : 0u;
      uint32_t lo = seg_off[row], hi = seg_off[row + 1];
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_rel[mid] <= rel) lo = mid; else hi = mid;
      }
      cu.seg[u] = lo;
    }
  }
  // how many variants are clusters of their own (statistics), and the template rows a search may need at most - the sum of the
  // clusters' bounds: one atomic each per WORKGROUP (same-address atomics are served one after the other, ~10 ns each)
  __shared__ uint32_t s_red[256 / WAVE][2];
  const unsigned long long vb = __ballot(variant_cluster);
  const uint32_t ssum = wave_sum(span_u);
  if ((threadIdx.x & (WAVE - 1)) == 0) { s_red[threadIdx.x / WAVE][0] = (uint32_t)__popcll(vb); s_red[threadIdx.x / WAVE][1] = ssum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int w = 0; w < 256 / WAVE; ++w) { a += s_red[w][0]; b += s_red[w][1]; }
    if (a) atomicAdd(n_variant_clusters, a);
    if (b) atomicAdd(slots_total, (unsigned long long)b);
  }
}
// what the host wants to know of a finished build, as one block (one copy instead of four)
__global__ void k_cl_results(const uint32_t* __restrict__ n_inst, const uint32_t* __restrict__ counters, const unsigned long long* __restrict__ slots_total,
                             const uint32_t* __restrict__ status, unsigned long long* __restrict__ out) {
  out[0] = *n_inst; out[1] = counters[0]; out[2] = counters[1]; out[3] = *slots_total; out[4] = *status;
  out[6] = wall_clock64();  // ClResults::end: the attempt's kernels are done
}
// The listed instances that found their hash in the table: number from the slot, identity compared record by record with the instance
// that opened the cluster (exactness: same hash is not same cluster until then).  Loads level by level.
__global__ __launch_bounds__(256) void k_cl_uid(const ClListed* __restrict__ cx_list, const uint32_t* __restrict__ n_list_dev, uint32_t t_end,
                                                const uint32_t* __restrict__ cx_state, const ClSlot* __restrict__ tab, uint32_t* __restrict__ inst_uid,
                                                ClUniq cu, const HxHead* __restrict__ recs, uint32_t* __restrict__ status) {
  const uint32_t n_list = *n_list_dev < t_end ? *n_list_dev : t_end;  // (launched over the bound on the list)
  if (blockIdx.x * (256 * CL_UID_U) >= n_list) return;
  const uint32_t t0 = blockIdx.x * (256 * CL_UID_U) + threadIdx.x;
  uint32_t v[CL_UID_U];
  bool pend[CL_UID_U];
  bool any = false;
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    const uint32_t t = t0 + u * 256;
    v[u] = t < n_list ? cx_state[t] : CL_NONE;
    pend[u] = v[u] != CL_NONE && (v[u] & CL_PENDING);
    any = any || pend[u];
  }
  if (!__any(any)) return;
  uint4 e1[CL_UID_U], la[CL_UID_U], lb[CL_UID_U];
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    e1[u] = reinterpret_cast<const uint4*>(tab + (pend[u] ? (v[u] & ~CL_PENDING) : 0u))[1];  // {number + 1, records | class, REF position, first variant}
    const uint4* l = reinterpret_cast<const uint4*>(cx_list + (pend[u] ? t0 + u * 256 : 0u));
    la[u] = l[0]; lb[u] = l[1];  // {instance, key, first record} {records | class, REF position, row position, first variant}
  }
  uint32_t rrec[CL_UID_U];
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) rrec[u] = (pend[u] && e1[u].x != 0u && (lb[u].x & 0xffffu) > 1u) ? cu.rec[e1[u].x - 1u] : 0u;
  bool bad = false;
#pragma unroll
  for (int u = 0; u < CL_UID_U; ++u) {
    if (!pend[u]) continue;
    const uint32_t i = la[u].x, ncls = lb[u].x;
    if (e1[u].x == 0u) { inst_uid[i] = CL_NONE; bad = true; continue; }  // (a taken slot without a number: cannot happen)
    inst_uid[i] = e1[u].x - 1u;
    // both shareable, as many records, the same REF position of the first allele and the same first variant (its allele, place and
    // REF resume follow), then record by record
    bool b = ncls != e1[u].y || (ncls >> 16) != 1 || lb[u].y != e1[u].z || lb[u].w != e1[u].w;
    const uint32_t n = ncls & 0xffffu;
    if (!b && n > 1) {
      const HxHead* pa = recs + la[u].w;
      const HxHead* pb = recs + rrec[u];
      const int32_t oa = (int32_t)lb[u].z, ob = pb[0].o;
      for (uint32_t k = 1; k < n; ++k) {
        const uint4 xa = *reinterpret_cast<const uint4*>(pa + k), xb = *reinterpret_cast<const uint4*>(pb + k);
        b = b || xa.w != xb.w || xa.z != xb.z || xa.y != xb.y || (int32_t)xa.x - oa != (int32_t)xb.x - ob;
      }
    }
    bad = bad || b;
  }
  if (bad) atomicOr(status, 2u);
}

// ---- launchers: the views of hawk_cl.h unpacked into the kernels' parameter lists ----------------------
// rows -> chunks: ch_off[n_rows + 1] (chunks in front of every row) and the chunks' rows (room: hawk_cl_chunk_bound)
void hawk_launch_cl_chunks(hipStream_t st, const ClBuild& b) {
  hipLaunchKernelGGL(k_cl_chunks, dim3(1), dim3(1024), 0, st, b.plan.hv_off, b.plan.is_ref, b.plan.ss, b.plan.se, b.plan.n_rows, b.ch.ch_off, b.ch.ch_row,
                     &b.tally.results->begin);
}
// The first CL_HEAD_CHUNKS chunks (a few dozen rows) describe the variants they carry in the COUNTING pass, which cuts them anyway;
// the launch of the scan turns the describers into the bitmap, and the cutting pass - one launch - describes what they left.  A
// common variant has thousands of instances, half of which are in flight at once: without the bitmap they would all describe it.
// Likewise the table passes run the head of the list as a launch of its own, then the rest: in a single launch the instances of a
// common cluster all find their slot empty and all go to the atomic - thousands of device-scope atomics queued at one address
// (60-90 us, whatever the panel's size).
// A small job - a stretch of a region on one of several GPUs - has no crowd to keep away from one address: no bitmap, no head.
// The launches run over BOUNDS (the numbers of chunks and of listed instances are on the device only; surplus workgroups leave at once).
#define CL_HEAD_CHUNKS 96
#define CL_HEAD_LISTED 16384
uint32_t hawk_cl_head_chunks(uint32_t ch_bound) { return ch_bound < 16 * CL_HEAD_CHUNKS ? 0u : CL_HEAD_CHUNKS; }
void hawk_launch_cl_count(hipStream_t st, const ClBuild& b) {
  const ClPlan& p = b.plan;
  if (b.ch.ch_bound)
    hipLaunchKernelGGL(k_cl_count, dim3(b.ch.ch_bound), dim3(256), 0, st, static_cast<const HxHead*>(p.heads), p.hv_off, p.hap_len, p.ss, p.se, b.ch.ch_off,
                       b.ch.ch_row, p.n_rows, p.n_var, b.ch.cnt, b.ch.lcnt, b.var.desc, hawk_cl_head_chunks(b.ch.ch_bound));
}
void hawk_launch_cl_fill(hipStream_t st, const ClBuild& b) {
  const ClPlan& p = b.plan;
#ifdef HAWK_TEST_HOOKS
  {
    const char* wk = getenv("HAWK_CLUSTER_WEAK_HASH");
    const uint32_t weak = wk && wk[0] == '1' ? 1u : 0u;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(cl_weak_hash), &weak, sizeof(weak));
  }
#endif
  if (b.ch.ch_bound)
    hipLaunchKernelGGL(k_cl_fill, dim3(b.ch.ch_bound), dim3(256), 0, st, static_cast<const HxHead*>(p.heads), p.hv_off, p.hap_len, p.ss, p.se, b.ch.ch_off,
                       b.ch.ch_row, b.ch.inst_base, b.ch.list_base, b.inst, b.var.desc, b.var.claim, p.n_var, b.list.list, b.tally.status, p.n_rows);
}
// after the cutting pass: the listed instances through the table of this attempt, the distinct clusters' descriptions, then the
// listed instances that share a cluster, and the result block for the host
void hawk_launch_cl_finish(hipStream_t st, const ClBuild& b, const ClTable& t, const ClUniq& cu) {
  const ClPlan& p = b.plan;
  const HxHead* recs = static_cast<const HxHead*>(p.heads);
  const uint32_t* n_inst_dev = b.ch.inst_base + b.ch.ch_bound;  // the scans' totals
  const uint32_t* n_list_dev = b.ch.list_base + b.ch.ch_bound;
  uint32_t* counters = b.tally.counters;
  uint32_t* status = b.tally.status;
  const uint32_t list_bound = b.list.bound;
  const uint32_t per = 256 * CL_UID_U;
  const uint32_t head = list_bound < 16 * CL_HEAD_LISTED ? 0u : CL_HEAD_LISTED;
  if (head)
    hipLaunchKernelGGL(k_cl_enter, dim3((head + per - 1) / per), dim3(256), 0, st, b.list.list, n_list_dev, 0u, head, t.tab, t.mask, t.max_probe,
                       t.fail_bit, b.inst.uid, b.inst.row, b.list.state, cu, counters, p.n_var, t.u_cap, status);
  if (list_bound > head)
    hipLaunchKernelGGL(k_cl_enter, dim3((list_bound - head + per - 1) / per), dim3(256), 0, st, b.list.list, n_list_dev, head, list_bound, t.tab,
                       t.mask, t.max_probe, t.fail_bit, b.inst.uid, b.inst.row, b.list.state, cu, counters, p.n_var, t.u_cap, status);
  hipLaunchKernelGGL(k_cl_describe, dim3((t.u_cap + 255) / 256), dim3(256), 0, st, counters, p.n_var, t.u_cap, b.var.desc, cu, recs, p.seg_off, p.seg_rel,
                     counters + 1, reinterpret_cast<unsigned long long*>(counters + 4));
  if (list_bound)
    hipLaunchKernelGGL(k_cl_uid, dim3((list_bound + per - 1) / per), dim3(256), 0, st, b.list.list, n_list_dev, list_bound, b.list.state, t.tab, b.inst.uid, cu,
                       recs, status);
  hipLaunchKernelGGL(k_cl_results, dim3(1), dim3(1), 0, st, n_inst_dev, counters, reinterpret_cast<const unsigned long long*>(counters + 4), status,
                     &b.tally.results->instances);
}
