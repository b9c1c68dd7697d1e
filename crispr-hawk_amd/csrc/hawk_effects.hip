// hawk_effects.hip - variant effects on the report groups of a collapsed table: k_fx_groups, k_fx_samples_*, k_fx_positions,
// k_fx_cands / k_fx_topk_*, k_fx_alts.  Every rule is a function of hawk_effects.h, which hawk_host_effects applies on the host.
//
// Shapes.  The groups of one position lie next to each other and are few (REF plus the alternatives a 23-base window sees: one
// or two nearly always, a few dozen at most), so the per-position work is a walk over the position by whichever thread needs it
// - a position may straddle any wave or workgroup boundary without any thread noticing.  The walks meet the alternatives in
// collapse order; everything that depends on report order is stated through the groups' report ranks (FxWorst, fx_is_dup), so
// no pass sorts.  The one pass whose work is per table ROW is the distinct-sample count: a group whose member rows list at most
// FX_SHORT_LIST sample entries is counted by its own thread of k_fx_samples_short (pairwise, no memory), a longer one is queued
// and gets a wave of k_fx_samples_long and a bitmap of one bit per sample id in LDS.
#include <hip/hip_runtime.h>

#include "hawk_device.h"

#define FX_BLOCK 256

__global__ __launch_bounds__(FX_BLOCK) void k_fx_isref_gather(const uint8_t* __restrict__ hap_is_ref, const uint32_t* __restrict__ member_hap,
                                                              const uint64_t* __restrict__ member_off, uint64_t n_groups, uint8_t* __restrict__ out) {
  const uint64_t g = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
  if (g < n_groups) out[g] = hap_is_ref[member_hap[member_off[g]]];
}
void hawk_launch_fx_isref_gather(hipStream_t st, const uint8_t* hap_is_ref, const uint32_t* member_hap, const uint64_t* member_off, uint64_t n_groups,
                                 uint8_t* out) {
  if (n_groups) hipLaunchKernelGGL(k_fx_isref_gather, dim3((unsigned)((n_groups + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, st, hap_is_ref, member_hap, member_off, n_groups, out);
}

// ---- per group: its position's head, its type, whether an earlier group of the report shows the same guide; the type counts
__global__ __launch_bounds__(FX_BLOCK) void k_fx_groups(FxDev F) {
  __shared__ unsigned int cnt[8];
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
  if (g < F.c.n_groups) {
    const uint64_t h = fx_head(F.c, g);
    const uint8_t type = fx_guide_type(fx_is_ref(F.c, g), fx_case_bits(F.c, g));
    const bool dup = fx_is_dup(F.c, g, h);
    F.head[g] = (uint32_t)h;
    F.type[g] = type;
    F.dup[g] = dup ? 1 : 0;
    if (!dup) atomicAdd(&cnt[type == FX_TYPE_UNKNOWN ? 4 : type], 1u);
    if (h == g) atomicAdd(&cnt[5], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 6 && cnt[threadIdx.x]) atomicAdd(&F.counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}
void hawk_launch_fx_groups(hipStream_t st, const FxDev& F) {
  if (F.c.n_groups) hipLaunchKernelGGL(k_fx_groups, dim3((unsigned)((F.c.n_groups + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, st, F);
}

// ---- distinct samples per group.  Short lists: entry after entry, counted when no earlier entry names the same sample.
__global__ __launch_bounds__(FX_BLOCK) void k_fx_samples_short(FxDev F) {
  const uint64_t g = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
  if (g >= F.c.n_groups) return;
  if (fx_is_ref(F.c, g)) { F.n_samples[g] = 0; return; }
  const uint64_t m0 = F.c.member_off[g], m1 = F.c.member_off[g + 1];
  uint64_t entries = 0;
  bool is_long = m1 - m0 > FX_SHORT_LIST;
  for (uint64_t m = m0; m < m1 && !is_long; ++m) {
    const uint32_t hp = F.c.member_hap[m];
    entries += F.c.hap_off[hp + 1] - F.c.hap_off[hp];
    is_long = entries > FX_SHORT_LIST;
  }
  if (is_long) {
    const unsigned long long slot = atomicAdd(&F.counts[6], 1ull);
    F.long_list[slot] = (uint32_t)g;  // at most one slot per group: the list holds n_groups entries
    return;
  }
  uint32_t ns = 0;
  for (uint64_t m = m0; m < m1; ++m) {
    const uint32_t hp = F.c.member_hap[m];
    for (uint64_t e = F.c.hap_off[hp]; e < F.c.hap_off[hp + 1]; ++e) {
      const uint32_t id = F.c.sample_id[e];
      bool seen = false;
      for (uint64_t m2 = m0; m2 <= m && !seen; ++m2) {
        const uint32_t hp2 = F.c.member_hap[m2];
        const uint64_t e1 = m2 == m ? e : F.c.hap_off[hp2 + 1];
        for (uint64_t e2 = F.c.hap_off[hp2]; e2 < e1 && !seen; ++e2) seen = F.c.sample_id[e2] == id;
      }
      ns += seen ? 0u : 1u;
    }
  }
  F.n_samples[g] = ns;
}
// Long lists: one wave per queued group, the member rows strided over its lanes, one bit per sample id in LDS (ids < n_sample_ids
// <= FX_SAMPLE_CAP, checked where the lists were uploaded); the bitmap is as long as the ids need, not as the cap allows.
__global__ __launch_bounds__(64) void k_fx_samples_long(FxDev F, uint32_t words) {
  extern __shared__ unsigned int bm[];
  const unsigned long long n_long = F.counts[6];
  for (unsigned long long q = blockIdx.x; q < n_long; q += gridDim.x) {
    const uint32_t g = F.long_list[q];
    for (uint32_t w = threadIdx.x; w < words; w += 64) bm[w] = 0;
    __syncthreads();
    for (uint64_t m = F.c.member_off[g] + threadIdx.x; m < F.c.member_off[g + 1]; m += 64) {
      const uint32_t hp = F.c.member_hap[m];
      for (uint64_t e = F.c.hap_off[hp]; e < F.c.hap_off[hp + 1]; ++e) {
        const uint32_t id = F.c.sample_id[e];
        if ((id >> 5) < words) atomicOr(&bm[id >> 5], 1u << (id & 31));
      }
    }
    __syncthreads();
    uint32_t ns = 0;
    for (uint32_t w = threadIdx.x; w < words; w += 64) ns += __popc(bm[w]);
    for (int o = 32; o > 0; o >>= 1) ns += __shfl_down(ns, o, 64);
    if (threadIdx.x == 0) F.n_samples[g] = ns;
    __syncthreads();
  }
}
void hawk_launch_fx_samples(hipStream_t st, const FxDev& F) {
  const uint64_t G = F.c.n_groups;
  if (!G) return;
  hipLaunchKernelGGL(k_fx_samples_short, dim3((unsigned)((G + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, st, F);
  const uint32_t words = (F.c.n_sample_ids + 31) / 32 ? (F.c.n_sample_ids + 31) / 32 : 1;
  const unsigned grid = (unsigned)(G < 4096 ? G : 4096);  // the queue's length is known on the device only: the waves stride over it
  hipLaunchKernelGGL(k_fx_samples_long, dim3(grid), dim3(64), words * 4, st, F, words);
}

// ---- per group its rounded score and its deltas; per position (at its head) the REF group, the valid alternatives, the worst delta
__global__ __launch_bounds__(FX_BLOCK) void k_fx_positions(FxDev F, int family) {
  const uint64_t g = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
  if (g >= F.c.n_groups) return;
  const uint64_t h = F.head[g];
  const double s = fx_round4(F.score[g]);
  F.rs[g] = s;
  if (h == g) {
    const FxPosition p = fx_position(F.c, F.score, family, h, fx_end(F.c, h));
    F.pos_ref[g] = p.ref; F.pos_worst[g] = p.worst; F.pos_nvalid[g] = p.n_valid; F.pos_first_rank[g] = p.first_rank;
    const double d = p.ref == FX_NONE ? 0.0 : fx_delta(s, p.ref_score);
    F.delta[g] = d; F.abs_delta[g] = fabs(d);
  } else {
    const uint32_t ref = fx_find_ref(F.c, h, fx_end(F.c, h));
    const double d = ref == FX_NONE ? 0.0 : fx_delta(s, fx_round4(F.score[ref]));
    F.delta[g] = d; F.abs_delta[g] = fabs(d);
    F.pos_ref[g] = FX_NONE; F.pos_worst[g] = 0.0; F.pos_nvalid[g] = 0; F.pos_first_rank[g] = FX_NONE;
  }
}
void hawk_launch_fx_positions(hipStream_t st, const FxDev& F, int family) {
  if (F.c.n_groups) hipLaunchKernelGGL(k_fx_positions, dim3((unsigned)((F.c.n_groups + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, st, F, family);
}

// ---- the selection.  Candidates first: chosen[k] <- the head of candidate k's position if it has a REF group (else it stays FX_NONE)
__global__ __launch_bounds__(FX_BLOCK) void k_fx_cands(FxDev F) {
  const uint64_t g = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
  if (g >= F.c.n_groups || F.head[g] != g || F.pos_ref[g] == FX_NONE) return;
  for (uint32_t k = 0; k < F.n_cand; ++k)
    if (F.cand_start[k] == F.c.start[g] && F.cand_strand[k] == F.c.strand[g]) F.chosen[k] = (uint32_t)g;
}

// The K best of a stream of entries under fx_before, kept sorted in L (LDS).  A tile's entries that beat the current K-th are
// collected, joined with L and ranked by counting: the order is total (report ranks differ), so every entry's count is its
// place.  After the first tiles hardly any entry beats the K-th and a tile costs one compare per thread.
struct FxTopK {
  FxEntry L[FX_MAX_K];
  FxEntry buf[FX_BLOCK + FX_MAX_K];
  uint32_t nL, nbuf;
};
__device__ __forceinline__ void fx_topk_tile(FxTopK& S, const FxEntry e, uint32_t K) {
  if (threadIdx.x == 0) S.nbuf = 0;
  __syncthreads();
  const uint32_t nL = S.nL;
  if (e.head != FX_NONE && (nL < K || fx_before(e, S.L[K - 1]))) S.buf[atomicAdd(&S.nbuf, 1u)] = e;
  __syncthreads();
  const uint32_t m = S.nbuf;
  if (m == 0) return;  // (uniform: read behind the barrier)
  if (threadIdx.x < nL) S.buf[m + threadIdx.x] = S.L[threadIdx.x];
  __syncthreads();
  const uint32_t total = m + nL;
  for (uint32_t j = threadIdx.x; j < total; j += FX_BLOCK) {
    const FxEntry x = S.buf[j];
    uint32_t r = 0;
    for (uint32_t k = 0; k < total; ++k) r += fx_before(S.buf[k], x) ? 1u : 0u;
    if (r < K) S.L[r] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) S.nL = total < K ? total : K;
  __syncthreads();
}
__device__ __forceinline__ bool fx_is_candidate(const FxDev& F, uint64_t g) {
  for (uint32_t k = 0; k < F.n_cand; ++k)
    if (F.cand_start[k] == F.c.start[g] && F.cand_strand[k] == F.c.strand[g]) return true;
  return false;
}
// per workgroup: the K - n_cand best ranked positions of its share of the groups -> part[block][FX_MAX_K] (FX_NONE-filled)
__global__ __launch_bounds__(FX_BLOCK) void k_fx_topk_part(FxDev F, int family, uint32_t take) {
  __shared__ FxTopK S;
  if (threadIdx.x == 0) S.nL = 0;
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * FX_BLOCK; base < F.c.n_groups; base += (uint64_t)gridDim.x * FX_BLOCK) {
    const uint64_t g = base + threadIdx.x;
    FxEntry e;
    e.key = 0; e.rank = 0; e.head = FX_NONE;
    if (take && g < F.c.n_groups && F.head[g] == g && F.pos_ref[g] != FX_NONE && !fx_is_candidate(F, g)) {
      e.key = fx_key(family, F.pos_worst[g]); e.rank = F.pos_first_rank[g]; e.head = (uint32_t)g;
    }
    fx_topk_tile(S, e, take ? take : 1);
  }
  if (threadIdx.x < FX_MAX_K) {
    FxEntry e;
    e.key = 0; e.rank = 0; e.head = FX_NONE;
    F.part[(uint64_t)blockIdx.x * FX_MAX_K + threadIdx.x] = threadIdx.x < S.nL ? S.L[threadIdx.x] : e;
  }
}
// one workgroup: the best of the workgroups' candidates, behind the candidate positions
__global__ __launch_bounds__(FX_BLOCK) void k_fx_topk_merge(FxDev F, uint32_t blocks, uint32_t take) {
  __shared__ FxTopK S;
  if (threadIdx.x == 0) S.nL = 0;
  __syncthreads();
  const uint32_t n = blocks * FX_MAX_K;
  for (uint32_t base = 0; base < n; base += FX_BLOCK) {
    FxEntry e;
    e.key = 0; e.rank = 0; e.head = FX_NONE;
    if (take && base + threadIdx.x < n) e = F.part[base + threadIdx.x];
    fx_topk_tile(S, e, take ? take : 1);
  }
  if (threadIdx.x < S.nL) F.chosen[F.n_cand + threadIdx.x] = S.L[threadIdx.x].head;
  __syncthreads();
  // what the host reads back in one copy: the chosen heads, behind them how many valid alternatives each has, then their number
  const uint32_t nc = F.n_cand + S.nL;
  if (threadIdx.x < nc) {
    const uint32_t h = F.chosen[threadIdx.x];
    F.chosen[FX_MAX_K + threadIdx.x] = h == FX_NONE ? 0u : F.pos_nvalid[h];
  }
  if (threadIdx.x == 0) F.chosen[2 * FX_MAX_K] = nc;
}
uint32_t hawk_fx_topk_blocks(uint64_t n_groups) {
  const uint64_t b = (n_groups + FX_BLOCK - 1) / FX_BLOCK;
  return (uint32_t)(b < 1 ? 1 : b > FX_TOPK_MAX_BLOCKS ? FX_TOPK_MAX_BLOCKS : b);
}
void hawk_launch_fx_topk(hipStream_t st, const FxDev& F, int family) {
  const uint64_t G = F.c.n_groups;
  const uint32_t blocks = hawk_fx_topk_blocks(G), take = F.K - F.n_cand;
  if (G && F.n_cand) hipLaunchKernelGGL(k_fx_cands, dim3((unsigned)((G + FX_BLOCK - 1) / FX_BLOCK)), dim3(FX_BLOCK), 0, st, F);
  hipLaunchKernelGGL(k_fx_topk_part, dim3(blocks), dim3(FX_BLOCK), 0, st, F, family, take);
  hipLaunchKernelGGL(k_fx_topk_merge, dim3(1), dim3(FX_BLOCK), 0, st, F, blocks, take);
}

// ---- the valid alternatives of every chosen position, in report order: one wave per position, a group's place = the valid
// alternatives of its position that come before it in the report
__global__ __launch_bounds__(64) void k_fx_alts(FxDev F, int family, uint32_t n_chosen) {
  const uint32_t i = blockIdx.x;
  uint64_t off = 0;
  for (uint32_t k = 0; k < i; ++k) off += F.chosen[k] == FX_NONE ? 0 : F.pos_nvalid[F.chosen[k]];
  const uint32_t h = F.chosen[i];
  const uint32_t mine = h == FX_NONE ? 0 : F.pos_nvalid[h];
  if (threadIdx.x == 0) {
    F.alt_off[i] = off;
    if (i + 1 == n_chosen) F.alt_off[n_chosen] = off + mine;
  }
  if (h == FX_NONE || mine == 0) return;
  const uint64_t e = fx_end(F.c, h);
  const double ref_score = F.rs[F.pos_ref[h]];
  for (uint64_t j = (uint64_t)h + threadIdx.x; j < e; j += 64) {
    if (fx_is_ref(F.c, j) || !fx_valid_alt(family, F.rs[j], ref_score)) continue;
    uint32_t r = 0;
    for (uint64_t k = h; k < e; ++k)
      r += (!fx_is_ref(F.c, k) && fx_valid_alt(family, F.rs[k], ref_score) && F.c.rank[k] < F.c.rank[j]) ? 1u : 0u;
    if (r < mine) F.alt_group[off + r] = (uint32_t)j;
  }
}
void hawk_launch_fx_alts(hipStream_t st, const FxDev& F, int family, uint32_t n_chosen) {
  if (n_chosen) hipLaunchKernelGGL(k_fx_alts, dim3(n_chosen), dim3(64), 0, st, F, family, n_chosen);
}
