// hawk_csearch.hip — the guide search from an expansion plan, once per DISTINCT variant cluster instead of once per row.
//
// A non-REF haplotype row contributes guide rows only where a window touches an alt allele (search_guides.py:468-471), and
// what those rows look like - PAM hits, coordinates, the REF partner, the padded window, CFDon - depends on nothing but
// the carried variants within reach of the window: two variants interact only if fewer than CL_LINK = 64 positions
// separate their alleles (a window's padded slice spans guidelen + pamlen + 2 x 10 <= 64 positions).  So a row's records
// fall into CLUSTERS (maximal runs with gaps <= CL_LINK), and a cluster carried by many chromosome copies - a common SNV
// with no neighbour - yields the same rows in every one of them, shifted by the copies' upstream indels.  On the C3 panel
// 8.8 x 10^6 cluster instances are 7.3 x 10^4 distinct clusters.
//
//   dictionary (once per plan; hawk_xplan_view; its kernels: hawk_cldict.hip, its host side: hawk_api_cldict.hip, what it shares
//       with this file - CL_LINK, CL_NONE: hawk_cl.h):  k_cl_chunks / k_cl_count / k_cl_fill cut every row's records into cluster instances.
//       An instance of ONE record whose windows can meet no bound of its row IS its variant: its distinct cluster is the variant's
//       index in the plan's table - nothing to look up, nothing to compare (the counting pass describes the variants of the
//       first rows, the cutting pass - one launch - what they left).  Every other instance with a cluster goes on a list and
//       through a hash table of the variant identities (k_cl_enter), and is compared record by record with the instance that
//       opened its cluster (k_cl_uid: exactly - same hash is not same cluster until then); those clusters are numbered behind the
//       variants.  An instance whose windows could meet a row-specific bound (scan range, row ends) is a cluster of its own; one
//       wholly outside the scan range carries no cluster at all.
//   per search:  k_cs_templates builds each distinct cluster's rows ONCE, on its representative row, with the string
//       builder, PAM match and filters of hawk_vsearch.hip and the row rules of hawk_rows.h (64-byte template rows, CsRow there;
//       strand 0 / strand 1 regions in position order); k_cs_count gives every instance its row count and adds up the job's totals
//       (candidates, hits: the cluster's own + REF's hits under the shift of the clean stretch in front of it) and adds a wave's
//       rows up (the offset scan runs over one entry per 64 instances); k_cs_emit_rows then copies template rows into the guide
//       table - packed 64-byte rows, one linear write stream - a wave per 256 consecutive instances, patching haplotype row
//       and position.
// The table holds the same rows as hawk_search on the materialised planes; their order within a haplotype is (cluster,
// strand, position) instead of (tile, strand, position) - GuideTable.emission_order() sorts either into the reference's.
// The REF row goes through the plane kernels as before.
#include "hawk_vc.h"

#define CS_G 8              // lanes per distinct cluster in k_cs_templates: one 32-window word each per round

size_t hawk_cs_row_bytes() { return sizeof(CsRow); }

// ---- per search ------------------------------------------------------------------------------------
__device__ __forceinline__ VcRanges cs_ranges(const HapSetDev& hs, const ScanParams& p, uint32_t h) {
  VcRanges rg;
  const int ss = hs.scan_start[h], se = hs.scan_stop[h], haplen = (int)hs.hap_len[h];
  const int poF = p.right ? 0 : p.guidelen, poR = p.right ? p.guidelen : 0;
  const int qmin = HAWK_PAD, qmax = haplen - p.L - HAWK_PAD + 1;
  rg.slo[0] = ss - poF; rg.shi[0] = se - poF; rg.slo[1] = ss - poR; rg.shi[1] = se - poR;
  rg.lo[0] = rg.slo[0] > qmin ? rg.slo[0] : qmin; rg.hi[0] = rg.shi[0] < qmax ? rg.shi[0] : qmax;
  rg.lo[1] = rg.slo[1] > qmin ? rg.slo[1] : qmin; rg.hi[1] = rg.shi[1] < qmax ? rg.shi[1] : qmax;
  return rg;
}
// inclusive sum over the CS_G lanes of a group
__device__ __forceinline__ uint32_t group_incl_scan(uint32_t v, uint32_t gl) {
#pragma unroll
  for (int d = 1; d < CS_G; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, d, CS_G);
    if (gl >= (uint32_t)d) v += t;
  }
  return v;
}

// position map (haplotype.py:90-159) from a hint: k0 = a segment of row h starting at or before every position the cluster asks for
__device__ __forceinline__ int64_t posmap_hint(const HapSetDev& hs, uint32_t k0, uint32_t kend, uint32_t rel) {
  uint32_t k = k0;
  while (k + 1 < kend && hs.seg_rel[k + 1] <= rel) ++k;
  return hs.seg_gen[k] + (int64_t)(rel - hs.seg_rel[k]);
}

// Every distinct cluster's rows, once: a group of CS_G lanes per cluster, each lane one word of 32 window starts per round.
// res[2u] = {rows of strand 0, rows of strand 1, PAM hits, candidates} of the cluster's own window starts, res[2u + 1] = {first template
// row, REF's hits before the cluster, REF's hits behind it, -} (32 bytes: one request to L2 from k_cs_count); its template rows sit
// at tbase[u] (strand 0 in position order, then strand 1), packed: a workgroup adds up its clusters' rows and takes its
// stretch of the template array with one atomic.
__global__ __launch_bounds__(256) void k_cs_templates(HapSetDev hs, VcArgs va, ClDict cd, ScanParams p, GuideParams gp, RefInfo ri,
                                                      uint4* __restrict__ res, uint32_t* __restrict__ tbase, CsRow* __restrict__ trows, unsigned long long* __restrict__ t_count, uint64_t t_cap, int* status,
                                                      unsigned long long* stamp) {
  __shared__ double s_cfd[336];
  __shared__ uint32_t s_w[256 / WAVE];
  __shared__ unsigned long long s_base;
  __shared__ uint32_t s_X[15][256];  // a short cluster's strings, one column per lane: [plane * 3 + word][lane]
  __shared__ uint32_t s_k[2][256];   // ... the window starts its filters keep, per strand
  __shared__ uint32_t s_e[256];      // ... and how many the group's lanes before it keep (strand 0 | strand 1 << 16)
  const uint32_t tid = threadIdx.x;
  hawk_stamp(stamp);
  if (gp.score_cfdon) for (uint32_t i = tid; i < 336; i += 256) s_cfd[i] = gp.cfd_mm[i];
  __syncthreads();
  const uint32_t gl = tid & (CS_G - 1);
  const uint32_t u = (blockIdx.x * 256 + tid) / CS_G;
  // the numbers of the distinct clusters have holes (a variant that is nowhere a cluster of its own: u_n = 0); their groups and the
  // surplus groups of the last workgroup go through the motions on record 0 of row 0 with no window start, and write nothing
  const uint32_t nc_u = u < cd.n_uniq ? cd.u_n[u] : 0u;
  const bool live = nc_u != 0u;
  const bool hole = u < cd.n_uniq && !live;
  const HxVar* __restrict__ recs = static_cast<const HxVar*>(va.recs_);
  const uint32_t h = live ? cd.u_row[u] : 0u, r0 = live ? cd.u_rec[u] : 0u, nc = live ? nc_u : 1u;
  const uint32_t seg0 = live ? cd.u_seg[u] : hs.seg_off[0], seg_end = hs.seg_off[h + 1];
  const uint32_t back = (uint64_t)r0 > va.hv_off[h] ? 1u : 0u;  // the record in front of the cluster sets the REF shift it starts from
  const HxVar* __restrict__ sv = recs + r0 - back;
  const int nrec = (int)(nc + back);
  const RowGeom geom = row_geom(p, gp);
  const int L = geom.L;
  const int32_t haplen = (int32_t)hs.hap_len[h];
  const int32_t o_first = live ? cd.u_o[u] : 0;
  const int32_t o_end = live ? recs[r0 + nc - 1].o + (int32_t)recs[r0 + nc - 1].alt_len : 0;
  const int32_t qa = o_first - (L - 1) > 0 ? o_first - (L - 1) : 0;
  const int32_t qb = o_end < haplen ? o_end : haplen;
  const int nwords = qb > qa ? (qb - qa + 31) / 32 : 0;
  const VcRanges rg = cs_ranges(hs, p, h);
  // REF's PAM hits (both strands) in front of where the cluster's own window starts begin, and in front of where REF resumes behind
  // its last allele: the clean run between two clusters of a row then has  before(this cluster) - behind(the one in front)  hits,
  // whichever row carries the two (k_cs_count) - REF coordinates, so part of the cluster's identity
  auto hits_before = [&](int64_t x) -> uint32_t {
    const int64_t xm = (int64_t)va.ref_S * 32;
    const uint32_t xc = (uint32_t)(x < 0 ? 0 : (x > xm ? xm : x));
    const uint4 e = va.hp[xc >> 5];
    const uint32_t m = (1u << (xc & 31u)) - 1u;
    return e.y + (uint32_t)__popc(e.x & m) + e.w + (uint32_t)__popc(e.z & m);
  };
  const int32_t rb_front = back ? (int32_t)sv[0].rs - (sv[0].o + (int32_t)sv[0].alt_len) : 0;
  const uint32_t h_front = hits_before((int64_t)o_first + rb_front - (L - 1)), h_behind = hits_before((int64_t)recs[r0 + nc - 1].rs);
  const int poF = p.right ? 0 : p.guidelen, poR = p.right ? p.guidelen : 0;
  auto ref32 = [&](int pl, uint32_t r) -> uint32_t {
    const uint32_t w = (r >> 5) < va.ref_S - 2 ? (r >> 5) : va.ref_S - 2;
    return ext32_glb(va.ref[pl], (w << 5) | (r & 31u));
  };
  // one word: the five 96-bit strings around window starts [q0, q0 + 32), PAM hits, candidates, the starts kept by the filters
  auto word = [&](int32_t q0, uint32_t (&X)[5][3], uint32_t& kF, uint32_t& kR, uint32_t& hits, uint32_t& cand) {
    const int32_t p0 = q0 - HAWK_PAD;
    const int32_t p0c = p0 < 0 ? 0 : p0;
    int32_t shift_run = 0;
    if (!vc_string_fast(va, sv, nrec, p0c, haplen, q0 + 32, X, shift_run))
      hx_words_t<false, 3>(va.alt_codes, sv, sv, nrec, nrec, false, p0c, haplen, ref32, X[0], X[1], X[2], X[3], X[4]);
    if (p0 < 0) {  // the string starts at the row's first base: bit i is position q0 - PAD + i all the same
      const uint32_t sh = (uint32_t)(-p0);
#pragma unroll
      for (int pl = 0; pl < 5; ++pl) {
        X[pl][2] = fsh(X[pl][1], X[pl][2], 32u - sh);
        X[pl][1] = fsh(X[pl][0], X[pl][1], 32u - sh);
        X[pl][0] = X[pl][0] << sh;
      }
    }
    uint32_t v0 = X[4][0], v1 = X[4][1], v2 = X[4][2];  // E: window starts whose spacer + PAM holds a variant base
    int r = 1;
    while (2 * r <= L && r < 32) {
      v0 |= fsh(v0, v1, (uint32_t)r); v1 |= fsh(v1, v2, (uint32_t)r); v2 |= v2 >> r;
      r *= 2;
    }
    const int rem = L - r;
    if (rem > 0) {
      if (rem < 32) { v0 |= fsh(v0, v1, (uint32_t)rem); v1 |= fsh(v1, v2, (uint32_t)rem); v2 |= v2 >> rem; }
      else { v0 |= v1; v1 |= v2; }
    }
    const uint32_t E = fsh(v0, v1, HAWK_PAD);
    const uint32_t own = range_mask(q0, qa, qb);
    uint32_t f = pam_match96(X, p.pam_fwd, p.pamlen, HAWK_PAD + poF) & own;
    uint32_t rv = pam_match96(X, p.pam_rev, p.pamlen, HAWK_PAD + poR) & own;
    f &= range_mask(q0, rg.slo[0], rg.shi[0]);
    rv &= range_mask(q0, rg.slo[1], rg.shi[1]);
    hits += __popc(f) + __popc(rv);
    f &= range_mask(q0, rg.lo[0], rg.hi[0]);
    rv &= range_mask(q0, rg.lo[1], rg.hi[1]);
    cand += __popc(f) + __popc(rv);
    kF = f & E;
    kR = rv & E;
  };
  // which kept starts are rows: not the REF guide at the same (start, strand) again (remove_redundant_guides).  REF's core is
  // asked for only where REF has a guide: a second round trip, but for few of a long cluster's many starts
  auto classify = [&](int32_t q0, const uint32_t (&X)[5][3], uint32_t kF, uint32_t kR, uint32_t& vF, uint32_t& vR) {
    vF = 0; vR = 0;
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      uint32_t m = s ? kR : kF;
      while (m) {
        const uint32_t bpos = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        RefProbe pr = ref_probe_bit(ri, posmap_hint(hs, seg0, seg_end, (uint32_t)q0 + bpos), (uint32_t)s);
        bool same = false;
        if (probe_has_ref(pr)) {
          W2 win[5], core[4], rcore[4];
          bool has_ref;
          ref_probe_cores(pr, va.ref);
          row_slices([&](int pl, int k) { return X[pl][k]; }, bpos, geom, win, core);
          same = ref_verdict(pr, core, geom, rcore, has_ref);
        }
        if (!same) { if (s) vR |= 1u << bpos; else vF |= 1u << bpos; }
      }
    }
  };
  // one row per start classify kept: slices -> probe -> verdict -> store (pass 2 of a short cluster does the same from LDS)
  auto write = [&](int32_t q0, const uint32_t (&X)[5][3], uint32_t vF, uint32_t vR, uint64_t at0, uint64_t at1) {
#pragma unroll 1
    for (int s = 0; s < 2; ++s) {
      uint32_t m = s ? vR : vF;
      while (m) {
        const uint32_t bpos = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const uint32_t q = (uint32_t)q0 + bpos;
        const int64_t start = posmap_hint(hs, seg0, seg_end, q), stop = posmap_hint(hs, seg0, seg_end, q + (uint32_t)L);
        const RefProbe pr = ref_probe(ri, va.ref, start, (uint32_t)s);
        W2 win[5], core[4], rcore[4];
        bool has_ref;
        row_slices([&](int pl, int k) { return X[pl][k]; }, bpos, geom, win, core);
        ref_verdict(pr, core, geom, rcore, has_ref);  // (classify kept only starts that are rows)
        const double score = row_cfdon(gp, has_ref, core, rcore, (uint32_t)s, geom, s_cfd, status);
        template_row_store(trows, s ? at1++ : at0++, t_cap, q, o_first, (uint32_t)s, start, stop, ri.startp, has_ref, win, score, p, status);
      }
    }
  };

  // ---- pass 1.  A cluster of up to CS_G words (nearly all of them) leaves its strings and kept starts in LDS: its survivors
  // are then dealt to the group's lanes one each per round, so that the position-map and REF look-ups of a cluster run side by
  // side instead of one after the other in the lane that owns the word (the kernel is a chain of dependent loads: with one
  // lane walking its word's survivors a wave lived 40 us).  Longer clusters count, then write, word by word.
  const bool one_round = nwords <= CS_G;  // uniform within a group
  const uint32_t g0 = tid & ~(uint32_t)(CS_G - 1);
  uint32_t X[5][3];
#pragma unroll
  for (int pl = 0; pl < 5; ++pl) X[pl][0] = X[pl][1] = X[pl][2] = 0;
  uint32_t vF = 0, vR = 0, n0 = 0, n1 = 0, hits = 0, cand = 0, TF = 0, TR = 0;
  if (one_round) {
    uint32_t kF = 0, kR = 0;
    if ((int)gl < nwords) word(qa + 32 * (int32_t)gl, X, kF, kR, hits, cand);
    const uint32_t c = (uint32_t)__popc(kF) | ((uint32_t)__popc(kR) << 16);
    const uint32_t inc = group_incl_scan(c, gl);
    const uint32_t tot = (uint32_t)__shfl((int)inc, CS_G - 1, CS_G);
    TF = tot & 0xffffu; TR = tot >> 16;
#pragma unroll
    for (int pl = 0; pl < 5; ++pl) { s_X[pl * 3 + 0][tid] = X[pl][0]; s_X[pl * 3 + 1][tid] = X[pl][1]; s_X[pl * 3 + 2][tid] = X[pl][2]; }
    s_k[0][tid] = kF; s_k[1][tid] = kR; s_e[tid] = inc - c;
  } else {
#pragma unroll 1
    for (int w0 = 0; w0 < nwords; w0 += CS_G) {
      const int w = w0 + (int)gl;
      uint32_t kF = 0, kR = 0;
      vF = 0; vR = 0;
      if (w < nwords) {
        word(qa + 32 * w, X, kF, kR, hits, cand);
        classify(qa + 32 * w, X, kF, kR, vF, vR);
      }
      const uint32_t c = (uint32_t)__popc(vF) | ((uint32_t)__popc(vR) << 16);
      const uint32_t tot = (uint32_t)__shfl((int)group_incl_scan(c, gl), CS_G - 1, CS_G);
      n0 += tot & 0xffffu; n1 += tot >> 16;
    }
  }
  hits = group_incl_scan(hits, gl); cand = group_incl_scan(cand, gl);  // the group's totals in its last lane
  // ---- the workgroup's stretch of the template array: rows of the long clusters, kept starts (>= rows) of the others
  const bool leader = live && gl == CS_G - 1;
  if (hole && gl == CS_G - 1) { res[2 * u] = make_uint4(0u, 0u, 0u, 0u); res[2 * u + 1] = make_uint4(0u, 0u, 0u, 0u); tbase[u] = 0u; }
  const uint32_t want = one_round ? TF + TR : n0 + n1;
  uint32_t btot;
  const uint32_t bex = block_excl_scan<256 / WAVE>(leader ? want : 0u, s_w, &btot);  // its barriers publish the groups' LDS entries
  if (tid == 0) s_base = btot ? atomicAdd(t_count, (unsigned long long)btot) : 0ull;
  __syncthreads();
  const uint32_t gex = (uint32_t)__shfl((int)bex, CS_G - 1, CS_G);  // the leader's exclusive offset = rows of the groups before
  const uint64_t tb = s_base + gex;
  if (tb + want > 0xffffffffull) atomicExch(status, -7 /* HAWK_E_UNSUPPORTED: template rows beyond 32-bit indices */);
  if (!one_round) {
    if (leader) { res[2 * u] = make_uint4(n0, n1, hits, cand); res[2 * u + 1] = make_uint4((uint32_t)tb, h_front, h_behind, 0u); tbase[u] = (uint32_t)tb; }
    if (!live || n0 + n1 == 0) return;  // no barrier below
    uint32_t b0 = 0, b1 = 0, h2 = 0, c2 = 0;
#pragma unroll 1
    for (int w0 = 0; w0 < nwords; w0 += CS_G) {
      const int w = w0 + (int)gl;
      uint32_t kF = 0, kR = 0;
      vF = 0; vR = 0;
      if (w < nwords) {
        word(qa + 32 * w, X, kF, kR, h2, c2);
        classify(qa + 32 * w, X, kF, kR, vF, vR);
      }
      const uint32_t c = (uint32_t)__popc(vF) | ((uint32_t)__popc(vR) << 16);
      const uint32_t inc = group_incl_scan(c, gl);
      const uint32_t tot = (uint32_t)__shfl((int)inc, CS_G - 1, CS_G);
      const uint32_t ex = inc - c;
      if (w < nwords) write(qa + 32 * w, X, vF, vR, tb + b0 + (ex & 0xffffu), tb + n0 + b1 + (ex >> 16));
      b0 += tot & 0xffffu; b1 += tot >> 16;
    }
    return;
  }
  // ---- pass 2 of a short cluster: survivor j of a strand -> lane j mod CS_G
  uint32_t done = 0;  // rows written so far (strand 0 first)
#pragma unroll 1
  for (int sd = 0; sd < 2; ++sd) {
    const uint32_t T = sd ? TR : TF, sh16 = sd ? 16u : 0u;
    uint32_t ns = 0;
#pragma unroll 1
    for (uint32_t j0 = 0; j0 < T; j0 += CS_G) {  // uniform within a group
      const uint32_t j = j0 + gl;
      const bool act = j < T;
      const uint32_t jj = act ? j : 0u;
      uint32_t l = 0;
#pragma unroll
      for (uint32_t step = CS_G / 2; step; step >>= 1) l += (((s_e[g0 + l + step] >> sh16) & 0xffffu) <= jj) ? step : 0u;
      const uint32_t src = g0 + l;
      const uint32_t bpos = select_bit(s_k[sd][src], jj - ((s_e[src] >> sh16) & 0xffffu));
      const uint32_t q = (uint32_t)(qa + 32 * (int32_t)l) + bpos;
      W2 win[5], core[4], rcore[4];
      row_slices([&](int pl, int k) { return s_X[pl * 3 + k][src]; }, bpos, geom, win, core);
      const int64_t start = posmap_hint(hs, seg0, seg_end, q), stop = posmap_hint(hs, seg0, seg_end, q + (uint32_t)L);
      const RefProbe pr = ref_probe(ri, va.ref, start, (uint32_t)sd);  // REF's core whether or not REF has a guide there: one round trip
      bool has_ref;
      const bool valid = act && !ref_verdict(pr, core, geom, rcore, has_ref);
      const uint32_t vinc = group_incl_scan(valid ? 1u : 0u, gl);
      const uint32_t vtot = (uint32_t)__shfl((int)vinc, CS_G - 1, CS_G);
      if (valid && live) {
        const double score = row_cfdon(gp, has_ref, core, rcore, (uint32_t)sd, geom, s_cfd, status);
        template_row_store(trows, tb + done + ns + (vinc - 1u), t_cap, q, o_first, (uint32_t)sd, start, stop, ri.startp, has_ref, win, score, p, status);
      }
      ns += vtot;
    }
    if (sd == 0) n0 = ns; else n1 = ns;
    done += ns;
  }
  if (leader) { res[2 * u] = make_uint4(n0, n1, hits, cand); res[2 * u + 1] = make_uint4((uint32_t)tb, h_front, h_behind, 0u); tbase[u] = (uint32_t)tb; }
}

// 16 bytes to a 16-byte-aligned address, past the caches' allocation (`nt`): the table is written once and read by a later kernel.
// The four dword stores to consecutive addresses are merged into one global_store_dwordx4 ... nt by the compiler.
__device__ __forceinline__ void nt_store4(uint32_t* q, const uint4& v) {
  __builtin_nontemporal_store(v.x, q); __builtin_nontemporal_store(v.y, q + 1);
  __builtin_nontemporal_store(v.z, q + 2); __builtin_nontemporal_store(v.w, q + 3);
}
// an instance's hand-over record, k_cs_count -> k_cs_emit_rows: a plain store (the next kernel but one reads it: written `nt` the
// emit pass took 0.397 ms for 0.375 on C3, profiles/emit_cold.md), read once: one global_load_dwordx4 ... nt
__device__ __forceinline__ void cs_inst_store(uint4* q, const uint4& v) { *q = v; }
__device__ __forceinline__ uint4 cs_inst_load(const uint4* q) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(q));
  return make_uint4(v.x, v.y, v.z, v.w);
}
// every instance: rows = those of its cluster; the job's totals get the cluster's own hits and those of the clean run in front of it -
// REF's hits before this cluster minus REF's hits behind the cluster in front (second half of the two entries, the neighbour's through the lane
// below): two 16-byte gathers per instance.  CS_CNT_U instances per thread, loads issued level by level: the instance's four dictionary
// words (cluster, run in front, haplotype row, position) are read-once streams and go out together, the gathers follow.
// What the emit pass needs of an instance leaves here as ONE 16-byte record {rows, first template row, haplotype row <<
// HAWK_ROW_HAP_SHIFT, position}: the emit pass then reads one stream this kernel has just written and nothing of the dictionary,
// whose arrays k_cl_fill wrote several hundred MB of traffic earlier in a step that rebuilds it (profiles/emit_cold.md).
#define CS_CNT_U 4
__global__ __launch_bounds__(256) void k_cs_count(HapSetDev hs, VcArgs va, ClDict cd, ScanParams p, const uint4* __restrict__ res,
                                                  const unsigned long long* __restrict__ t_count, uint64_t t_cap,
                                                  uint32_t* __restrict__ group_counts, uint4* __restrict__ inst, unsigned long long* __restrict__ shards,
                                                  unsigned long long* stamp) {
  __shared__ uint32_t s_red[256 / WAVE][2];
  hawk_stamp(stamp);
  const uint32_t i0 = blockIdx.x * (256 * CS_CNT_U) + threadIdx.x;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const bool ovf = *t_count > t_cap;  // the template rows outgrew their reservation: no table (the host reruns the search)
  uint32_t uid[CS_CNT_U], below[CS_CNT_U], row[CS_CNT_U];
  int32_t paf[CS_CNT_U], o[CS_CNT_U];
  bool in[CS_CNT_U];
#pragma unroll
  for (int u = 0; u < CS_CNT_U; ++u) {
    const uint32_t i = i0 + u * 256;
    in[u] = i < cd.n_inst;
    const uint32_t ic = in[u] ? i : 0u;
    uid[u] = __builtin_nontemporal_load(cd.inst_uid + ic); paf[u] = __builtin_nontemporal_load(cd.inst_pa + ic);
    row[u] = __builtin_nontemporal_load(cd.inst_row + ic); o[u] = __builtin_nontemporal_load(cd.inst_o + ic);
    below[u] = CL_NONE;
    if (lane == 0 && in[u] && i > 0) below[u] = cd.inst_uid[i - 1];  // (the other lanes' neighbour is the lane below)
  }
  uint4 r[CS_CNT_U], r2[CS_CNT_U];
  uint32_t behind0[CS_CNT_U];
#pragma unroll
  for (int u = 0; u < CS_CNT_U; ++u) {
    const bool has = in[u] && uid[u] != CL_NONE;
    r[u] = make_uint4(0u, 0u, 0u, 0u); r2[u] = r[u]; behind0[u] = 0u;
    if (cd.n_uniq) {
      const uint32_t us = has ? uid[u] : 0u;
      r[u] = res[2 * us]; r2[u] = res[2 * us + 1];
      if (lane == 0 && below[u] != CL_NONE) behind0[u] = res[2 * below[u] + 1].z;
    }
    if (!has) { r[u] = make_uint4(0u, 0u, 0u, 0u); r2[u] = r[u]; }
  }
  uint32_t cand = 0, hits = 0;
#pragma unroll
  for (int u = 0; u < CS_CNT_U; ++u) {
    const uint32_t i = i0 + u * 256;
    uint32_t behind = (uint32_t)__shfl_up((int)r2[u].z, 1);
    if (lane == 0) behind = behind0[u];
    uint32_t rows_i = 0;
    if (in[u]) {
      if (paf[u] < 0) {  // the run in front lies inside every range (k_cl_fill): it has a cluster at either end, and those know
        const uint32_t hc = r2[u].y - behind;
        hits += hc; cand += hc;
      } else {
        const int32_t pa = paf[u], pb = o[u] - (p.L - 1);
        if (pb > pa) {
          const VcRanges rg = cs_ranges(hs, p, row[u]);
          vc_count_run(va, rg, pa, pb, cd.inst_rb[i], cand, hits);
        }
      }
      hits += r[u].z; cand += r[u].w;
      rows_i = ovf ? 0u : r[u].x + r[u].y;
      // the hand-over record (r2.x: the instance's first template row, so the emit pass does not go through the cluster number)
      cs_inst_store(inst + i, make_uint4(rows_i, r2[u].x, row[u] << HAWK_ROW_HAP_SHIFT, (uint32_t)o[u]));
    }
    // what the offset scan runs over: the rows of 64 consecutive instances (one wave here, one wave's contiguous stretch of the table in
    // the emit pass) - 1.4 x 10^5 entries on C3 instead of 8.8 x 10^6
    const uint32_t gsum = wave_sum(rows_i);
    const uint32_t iw = blockIdx.x * (256 * CS_CNT_U) + u * 256 + (threadIdx.x & ~(uint32_t)(WAVE - 1));
    if (lane == 0 && iw < cd.n_inst) group_counts[iw / WAVE] = gsum;
  }
  const uint32_t a = wave_sum(cand), b = wave_sum(hits);
  if (lane == 0) { s_red[threadIdx.x / WAVE][0] = a; s_red[threadIdx.x / WAVE][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t0 = 0, t1 = 0;
#pragma unroll
    for (int wv = 0; wv < 256 / WAVE; ++wv) { t0 += s_red[wv][0]; t1 += s_red[wv][1]; }
    if (t0 | t1) {
      atomicAdd(&shards[(blockIdx.x & 255u) * 2 + 0], (unsigned long long)t0);
      atomicAdd(&shards[(blockIdx.x & 255u) * 2 + 1], (unsigned long long)t1);
    }
  }
}

// ---- packed rows (round 4): the guide table of a cluster search as ONE array of 64-byte rows -----------------------------
// A template row (CsRow, hawk_rows.h: the field order is written down there) with two words patched: pos and the haplotype row.  A wave's rows are contiguous, four lanes move one row (16 bytes each), so every store
// instruction writes 1 KB of consecutive addresses and the whole table is a single linear write stream - twelve column
// streams whose relative placement decided the speed before (profiles/r03_csearch_ablation.txt).
// NI x 64 consecutive instances per wave, their rows one contiguous stretch of the table.  What bounds the pass is not bytes but
// how long a wave's loads take while 1.8 GB of stores are queued at the memory controllers (the same kernel runs 0.36 ms with its
// 160 MB read set cache-resident and 0.53 with it in HBM): so a wave asks for all its instance data at once, up front, and
// keeps the template loads of the next 128 rows in flight while it stores the current 128.
template <int NI, int CE_CH>
__global__ __launch_bounds__(256) void k_cs_emit_rows(uint32_t n_inst, const uint4* __restrict__ inst,
                                                      const CsRow* __restrict__ trows, const uint64_t* __restrict__ offsets,
                                                      const unsigned long long* __restrict__ t_count, uint64_t t_cap, uint4* __restrict__ rows,
                                                      uint64_t cap, int* status, unsigned long long* stamp) {
  // everything below is private to a wave (its own LDS slices, no workgroup barrier): the four waves of a workgroup drift apart freely
  constexpr int NE = NI * WAVE;
  constexpr int CE_SUB = CE_CH / 16;  // 16-byte loads per lane and chunk
  __shared__ uint32_t s_ex[4][NE + 1];
  __shared__ uint32_t s_tb[4][NE], s_h[4][NE];
  __shared__ int32_t s_dq[4][NE];
  __shared__ uint32_t s_src[4][2][CE_CH], s_rh[4][2][CE_CH];
  __shared__ int32_t s_rdq[4][2][CE_CH];
  hawk_stamp(stamp);
  if (*t_count > t_cap) return;  // the template rows outgrew their reservation (k_cs_count left no counts): the host reruns the search
  const uint32_t wv = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const uint32_t i0 = (blockIdx.x * 4 + wv) * NE;  // the wave's first instance
  if (i0 >= n_inst) return;
  // per instance: ONE 16-byte streaming load of the record k_cs_count has just left {rows, first template row, haplotype row
  // shifted, position} - nothing here waits for a gather through the cluster number or reads the dictionary's arrays; lane l takes
  // instances i0 + 64 c + l (lanes past the last instance are clamped onto it and count no rows)
  uint32_t cnt[NI], tb[NI], h[NI];
  int32_t dq[NI];
#pragma unroll
  for (int c = 0; c < NI; ++c) {
    const uint32_t i = i0 + c * WAVE + lane;
    const bool in = i < n_inst;
    const uint4 rec = cs_inst_load(inst + (in ? i : n_inst - 1));
    cnt[c] = in ? rec.x : 0u; tb[c] = rec.y; h[c] = rec.z; dq[c] = (int32_t)rec.w;
  }
  // the wave's first row
  const uint64_t o0 = offsets[i0 / WAVE];  // one offset per 64 instances (k_cs_count's groups); wave-uniform: a scalar load
  uint32_t Wt = 0;
#pragma unroll
  for (int c = 0; c < NI; ++c) {
    const uint32_t inc = wave_incl_scan(cnt[c]);
    s_ex[wv][c * WAVE + lane] = Wt + inc - cnt[c];
    s_tb[wv][c * WAVE + lane] = tb[c]; s_h[wv][c * WAVE + lane] = h[c]; s_dq[wv][c * WAVE + lane] = dq[c];
    Wt += (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
  }
  if (Wt == 0) return;  // wave-uniform
  if (o0 + Wt > cap) { if (lane == 0) atomicCAS(status, 0, -3 /* HAWK_E_CAPACITY */); return; }
  __builtin_amdgcn_wave_barrier();
  const uint32_t qd = lane & 3u, rq = lane >> 2;
  uint4* __restrict__ const dst = rows + o0 * 4 + qd;
  // which template row each of a chunk's rows copies, its haplotype row and position shift (rows past the wave's last are
  // clamped onto it: every lane then loads a valid template row and the loads need no branch)
  auto meta = [&](uint32_t c0, uint32_t buf) {
#pragma unroll
    for (uint32_t sub = 0; sub < (CE_CH + WAVE - 1) / WAVE; ++sub) {
      const uint32_t r = sub * WAVE + lane;
      if (CE_CH < WAVE && r >= CE_CH) break;
      const uint32_t t = c0 + r < Wt ? c0 + r : Wt - 1;
      uint32_t l = 0;
#pragma unroll
      for (uint32_t step = NE / 2; step; step >>= 1) l += (s_ex[wv][l + step] <= t) ? step : 0u;  // l + step <= NE - 1
      s_src[wv][buf][r] = s_tb[wv][l] + (t - s_ex[wv][l]);
      s_rh[wv][buf][r] = s_h[wv][l];
      s_rdq[wv][buf][r] = s_dq[wv][l];
    }
    __builtin_amdgcn_wave_barrier();
  };
  // four lanes per row, 16 bytes each
  auto fetch = [&](uint4 (&v)[CE_SUB], uint32_t buf) {
#pragma unroll
    for (uint32_t j = 0; j < CE_SUB; ++j) v[j] = reinterpret_cast<const uint4*>(trows + s_src[wv][buf][j * 16 + rq])[qd];
  };
  auto store = [&](const uint4 (&v)[CE_SUB], uint32_t c0, uint32_t buf) {
#pragma unroll
    for (uint32_t j = 0; j < CE_SUB; ++j) {
      const uint32_t r = j * 16 + rq;
      uint4 w = v[j];
      if (qd == 0) {
        w.x = (uint32_t)((int32_t)w.x + s_rdq[wv][buf][r]);
        w.y |= s_rh[wv][buf][r];
      }
      if (c0 + r < Wt) nt_store4(reinterpret_cast<uint32_t*>(dst + (size_t)(c0 + r) * 4), w);
    }
  };
  uint4 va[CE_SUB], vb[CE_SUB];
  meta(0, 0);
  fetch(va, 0);
#pragma unroll 1
  for (uint32_t c0 = 0; c0 < Wt; c0 += 2 * CE_CH) {
    const bool more1 = c0 + CE_CH < Wt, more2 = c0 + 2 * CE_CH < Wt;  // wave-uniform
    if (more1) { meta(c0 + CE_CH, 1); fetch(vb, 1); }
    store(va, c0, 0);
    __builtin_amdgcn_wave_barrier();
    if (more1) {
      if (more2) { meta(c0 + 2 * CE_CH, 0); fetch(va, 0); }
      store(vb, c0 + CE_CH, 1);
      __builtin_amdgcn_wave_barrier();
    }
  }
}
// the ONE instantiation of the emit pass: 64-instance groups per wave, rows per chunk (the sweeps are below)
constexpr int CS_EMIT_NI = 4, CS_EMIT_CH = 256;
void hawk_cs_emit_geometry(uint32_t* inst_per_wave, uint32_t* rows_per_chunk) { *inst_per_wave = CS_EMIT_NI * WAVE; *rows_per_chunk = CS_EMIT_CH; }
void hawk_launch_cs_emit_rows(hipStream_t st, uint32_t n_inst, const void* inst, const void* trows, const uint64_t* offsets,
                              const unsigned long long* t_count, uint64_t t_cap, void* rows, uint64_t cap, int* status,
                              unsigned long long* stamp) {
  if (!n_inst) { if (stamp) hawk_launch_stamp(st, stamp); return; }
  // 256 instances per wave, 256 rows in flight per wave (184 VGPRs: two waves per SIMD).  Measured on C3 (profiles/r04_emit_rows.md):
  // 64 / 128 / 256 rows in flight at 8 / 4 / 2 waves per SIMD: 0.53 / 0.47 / 0.45 ms before the offset scan went to one entry per
  // 64 instances, 0.39 (128 rows, 128 instances) / 0.38 after - few waves with long contiguous bursts write best.
  // Those figures are searches of a resident dictionary.  Behind a dictionary build (every step of bench.py) the pass took 0.45 - 0.48
  // while it read inst_row / inst_o / counts / inst_tb itself, and 0.37 - 0.38 in either regime since it reads k_cs_count's records.
  // Swept again behind the build, on the records (profiles/emit_cold.md; instances per wave x rows per chunk: VGPRs, waves per SIMD,
  // ms rebuilt / resident): 128 x 128: 103, 4, 0.377 / 0.374; 128 x 256: 184, 2, 0.378 / 0.367; 256 x 128: 104, 4, 0.376 / 0.373;
  // 256 x 256: 185, 2, 0.374 - 0.380 / 0.371 - 0.374; 512 x 128: 105, 3 (LDS), 0.382 / 0.377; 512 x 256: 186, 2, 0.378 / 0.371 -
  // all inside one another's spread (0.01), so the instantiation stays.  On the four arrays 512 instances per wave gained 0.03
  // behind the build (0.434 for 0.467) and the records made that gain moot.
  constexpr int NI = CS_EMIT_NI, CH = CS_EMIT_CH;
  hipLaunchKernelGGL((k_cs_emit_rows<NI, CH>), dim3((n_inst + 256 * NI - 1) / (256 * NI)), dim3(256), 0, st, n_inst, static_cast<const uint4*>(inst),
                     static_cast<const CsRow*>(trows), offsets, t_count, t_cap, static_cast<uint4*>(rows), cap, status, stamp);
}

void hawk_launch_cs_templates(hipStream_t st, const HapSetDev& hs, const VcArgs& va, const ClDict& cd, const ScanParams& p, const GuideParams& gp,
                              const RefInfo& ri, void* res, uint32_t* tbase, void* trows, unsigned long long* t_count, uint64_t t_cap, int* status,
                              unsigned long long* stamp) {
  if (!cd.n_uniq) { if (stamp) hawk_launch_stamp(st, stamp); return; }
  const uint32_t nb = (uint32_t)(((uint64_t)cd.n_uniq * CS_G + 255) / 256);
  hipLaunchKernelGGL(k_cs_templates, dim3(nb), dim3(256), 0, st, hs, va, cd, p, gp, ri, static_cast<uint4*>(res), tbase, static_cast<CsRow*>(trows),
                     t_count, t_cap, status, stamp);
}
void hawk_launch_cs_count(hipStream_t st, const HapSetDev& hs, const VcArgs& va, const ClDict& cd, const ScanParams& p, const void* res,
                          const unsigned long long* t_count, uint64_t t_cap, uint32_t* group_counts, void* inst, unsigned long long* shards,
                          unsigned long long* stamp) {
  if (!cd.n_inst) { if (stamp) hawk_launch_stamp(st, stamp); return; }
  hipLaunchKernelGGL(k_cs_count, dim3((cd.n_inst + 256 * CS_CNT_U - 1) / (256 * CS_CNT_U)), dim3(256), 0, st, hs, va, cd, p, static_cast<const uint4*>(res), t_count, t_cap,
                     group_counts, static_cast<uint4*>(inst), shards, stamp);
}

// columns -> packed rows (REF's rows, which the plane kernels write as columns; a columnar table before an exchange) and back:
// the field order of CsRow (hawk_rows.h).  `max_rows`: what `rows` holds.  The row count comes from the device, and a speculative
// emit packs into a table an earlier search reserved: REF alone can have more rows than that table (a one-base PAM behind NGG on a
// panel of few variants).  Like every other writer of a table the kernel then refuses instead of writing past the end - the launch is
// rounded up to 256 threads, and those between max_rows and the next multiple used to write up to 255 rows behind the allocation.
__global__ __launch_bounds__(256) void k_rows_pack(GuideCols c, const uint64_t* __restrict__ n_dev, uint64_t n_host, uint64_t max_rows, uint4* __restrict__ rows,
                                                   int64_t startp, int* status, unsigned long long* stamp) {
  hawk_stamp(stamp);
  const uint64_t n = n_dev ? *n_dev : n_host;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (n > max_rows) { if (i == 0) atomicCAS(status, 0, -3 /* HAWK_E_CAPACITY */); return; }
  if (i >= n) return;
  const int64_t start = c.start[i], ds = start - startp, de = c.stop[i] - start;
  const uint32_t h = c.hap[i];
  if (ds < INT32_MIN || ds > INT32_MAX || de < INT32_MIN || de > INT32_MAX || h >= HAWK_ROW_MAX_HAP) atomicCAS(status, 0, -7 /* HAWK_E_UNSUPPORTED */);
  const uint64_t sc = (uint64_t)__double_as_longlong(c.cfdon[i]);
  uint64_t w[HAWK_PLANES];
#pragma unroll
  for (int pl = 0; pl < HAWK_PLANES; ++pl) w[pl] = c.win[(size_t)pl * c.cap + i];
  uint4* __restrict__ r = rows + i * 4;
  r[0] = make_uint4(c.pos[i], (uint32_t)(c.strand[i] & 1u) | ((uint32_t)c.flags[i] << 1) | (h << HAWK_ROW_HAP_SHIFT), (uint32_t)(int32_t)ds, (uint32_t)(int32_t)de);
  r[1] = make_uint4((uint32_t)sc, (uint32_t)(sc >> 32), (uint32_t)w[0], (uint32_t)(w[0] >> 32));
  r[2] = make_uint4((uint32_t)w[1], (uint32_t)(w[1] >> 32), (uint32_t)w[2], (uint32_t)(w[2] >> 32));
  r[3] = make_uint4((uint32_t)w[3], (uint32_t)(w[3] >> 32), (uint32_t)w[4], (uint32_t)(w[4] >> 32));
}
__global__ __launch_bounds__(256) void k_rows_unpack(const uint4* __restrict__ rows, uint64_t n, int64_t startp, GuideCols d) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4* __restrict__ r = rows + i * 4;
  const uint4 a = r[0], b = r[1], cc = r[2], e = r[3];
  const int64_t start = startp + (int64_t)(int32_t)a.z;
  if (d.hap) d.hap[i] = a.y >> HAWK_ROW_HAP_SHIFT;
  if (d.pos) d.pos[i] = a.x;
  if (d.strand) d.strand[i] = (uint8_t)(a.y & 1u);
  if (d.flags) d.flags[i] = (uint8_t)((a.y >> 1) & 0xffu);
  if (d.start) d.start[i] = start;
  if (d.stop) d.stop[i] = start + (int64_t)(int32_t)a.w;
  if (d.cfdon) d.cfdon[i] = __longlong_as_double((long long)((uint64_t)b.x | ((uint64_t)b.y << 32)));
  if (d.win) {
    d.win[i] = (uint64_t)b.z | ((uint64_t)b.w << 32);
    d.win[d.cap + i] = (uint64_t)cc.x | ((uint64_t)cc.y << 32);
    d.win[2 * d.cap + i] = (uint64_t)cc.z | ((uint64_t)cc.w << 32);
    d.win[3 * d.cap + i] = (uint64_t)e.x | ((uint64_t)e.y << 32);
    d.win[4 * d.cap + i] = (uint64_t)e.z | ((uint64_t)e.w << 32);
  }
}
void hawk_launch_rows_pack(hipStream_t st, const GuideCols& src, const uint64_t* n_dev, uint64_t n_host, uint64_t max_rows, uint4* rows, int64_t startp,
                           int* status, unsigned long long* stamp) {
  if (!max_rows) { if (stamp) hawk_launch_stamp(st, stamp); return; }
  hipLaunchKernelGGL(k_rows_pack, dim3((unsigned)((max_rows + 255) / 256)), dim3(256), 0, st, src, n_dev, n_host, max_rows, rows, startp, status, stamp);
}
void hawk_launch_rows_unpack(hipStream_t st, const uint4* rows, uint64_t n, int64_t startp, const GuideCols& dst) {
  if (!n) return;
  hipLaunchKernelGGL(k_rows_unpack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, n, startp, dst);
}

// ---- the collapse of a cluster-searched table (hawk_api.hip: collapse_by_templates) ---------------------------------------
// REF's rows + the template rows as a table of their own: the grouping compares nothing that differs between a template row and
// its copies (start, stop, strand, REF-or-not, the windows)
__global__ __launch_bounds__(256) void k_cc_ucnt(const uint4* __restrict__ res, uint32_t nu, uint32_t* __restrict__ cnt) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u < nu) { const uint4 r = res[2 * u]; cnt[u] = r.x + r.y; }
}
// mini row r0 + moff[u] + k is row k of distinct cluster u: template row tbase[u] + k (CsRow, hawk_rows.h)
__global__ __launch_bounds__(256) void k_cc_mini(GuideCols c, uint64_t r0, const CsRow* __restrict__ trows, uint64_t t_rows,
                                                 const uint64_t* __restrict__ moff, const uint32_t* __restrict__ tbase, uint32_t nu, int64_t startp,
                                                 GuideCols m) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= r0 + t_rows) return;
  if (i < r0) {
    m.hap[i] = gc_hap(c, i); m.pos[i] = gc_pos(c, i); m.strand[i] = (uint8_t)gc_strand(c, i); m.start[i] = gc_start(c, i); m.stop[i] = gc_stop(c, i);
    m.flags[i] = (uint8_t)gc_flags(c, i); m.cfdon[i] = gc_cfdon(c, i);
#pragma unroll
    for (int pl = 0; pl < HAWK_PLANES; ++pl) m.win[(size_t)pl * m.cap + i] = gc_win(c, pl, i);
    return;
  }
  uint32_t lo = 0, hi = nu;  // last u with moff[u] <= i - r0
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (moff[mid] <= i - r0) lo = mid; else hi = mid;
  }
  const uint4* __restrict__ tp = reinterpret_cast<const uint4*>(trows + (tbase[lo] + (i - r0 - moff[lo])));
  const uint4 a = tp[0], b = tp[1], cc = tp[2], d = tp[3];
  const int64_t start = startp + (int64_t)(int32_t)a.z;
  m.hap[i] = 1u;  // any row but REF's: the grouping asks for the origin only
  m.pos[i] = a.x; m.strand[i] = (uint8_t)(a.y & 1u); m.flags[i] = (uint8_t)((a.y >> 1) & 0xffu);
  m.start[i] = start; m.stop[i] = start + (int64_t)(int32_t)a.w;
  m.cfdon[i] = __longlong_as_double((long long)((uint64_t)b.x | ((uint64_t)b.y << 32)));
  m.win[0 * m.cap + i] = (uint64_t)b.z | ((uint64_t)b.w << 32);
  m.win[1 * m.cap + i] = (uint64_t)cc.x | ((uint64_t)cc.y << 32);
  m.win[2 * m.cap + i] = (uint64_t)cc.z | ((uint64_t)cc.w << 32);
  m.win[3 * m.cap + i] = (uint64_t)d.x | ((uint64_t)d.y << 32);
  m.win[4 * m.cap + i] = (uint64_t)d.z | ((uint64_t)d.w << 32);
}
// group number of every mini row from the mini collapse's (permutation, CSR offsets)
__global__ __launch_bounds__(256) void k_cc_gidm(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ goff, uint64_t nm, uint64_t G,
                                                 uint32_t* __restrict__ gidm) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nm) return;
  uint64_t lo = 0, hi = G;  // last g with goff[g] <= j
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (goff[mid] <= j) lo = mid; else hi = mid;
  }
  gidm[perm[j]] = (uint32_t)lo;
}
// every table row's group number = its template row's (REF's rows: their own), next to its index: the pairs the sort orders
__global__ __launch_bounds__(256) void k_cs_gid(ClDict cd, const uint4* __restrict__ res, const uint64_t* __restrict__ moff,
                                                const uint64_t* __restrict__ offsets, uint64_t r0, uint64_t n, const uint32_t* __restrict__ gidm,
                                                uint32_t* __restrict__ gid, uint32_t* __restrict__ vals) {
  __shared__ uint32_t s_ex[4][WAVE + 1];
  __shared__ uint32_t s_tb[4][WAVE];
  const uint32_t wv = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint32_t cnt = 0, tb = 0;
  if (i < cd.n_inst) {
    const uint32_t u = cd.inst_uid[i];
    if (u != CL_NONE) { const uint4 r = res[2 * u]; cnt = r.x + r.y; tb = (uint32_t)moff[u]; }
  }
  const uint32_t inc = wave_incl_scan(cnt);
  const uint32_t Wt = (uint32_t)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
  const uint32_t i0 = blockIdx.x * 256 + wv * WAVE;
  const uint64_t o0 = i0 < cd.n_inst ? offsets[i0 / WAVE] : 0;  // one offset per 64 instances (k_cs_count's groups)
  s_ex[wv][lane] = inc - cnt;
  s_tb[wv][lane] = tb;
  __syncthreads();
  if (o0 + Wt > n) return;  // cannot happen for the table these offsets were scanned for
  for (uint32_t t = lane; t < Wt; t += WAVE) {
    uint32_t l = 0;
#pragma unroll
    for (uint32_t step = WAVE / 2; step; step >>= 1) l += (s_ex[wv][l + step] <= t) ? step : 0u;
    const uint64_t o = o0 + t;
    gid[o] = gidm[r0 + s_tb[wv][l] + (t - s_ex[wv][l])];
    vals[o] = (uint32_t)o;
  }
}
__global__ __launch_bounds__(256) void k_cc_refgid(uint64_t r0, const uint32_t* __restrict__ gidm, uint32_t* __restrict__ gid, uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < r0) { gid[i] = gidm[i]; vals[i] = (uint32_t)i; }
}
void hawk_launch_cc_ucnt(hipStream_t st, const void* res, uint32_t nu, uint32_t* cnt) {
  hipLaunchKernelGGL(k_cc_ucnt, dim3((nu + 255) / 256), dim3(256), 0, st, static_cast<const uint4*>(res), nu, cnt);
}
void hawk_launch_cc_mini(hipStream_t st, const GuideCols& c, uint64_t r0, const void* trows, uint64_t t_rows, const uint64_t* moff, const uint32_t* tbase,
                         uint32_t nu, int64_t startp, GuideCols m) {
  const uint64_t nm = r0 + t_rows;
  hipLaunchKernelGGL(k_cc_mini, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, c, r0, static_cast<const CsRow*>(trows), t_rows, moff, tbase, nu,
                     startp, m);
}
void hawk_launch_cc_gidm(hipStream_t st, const uint32_t* perm, const uint64_t* goff, uint64_t nm, uint64_t G, uint32_t* gidm) {
  hipLaunchKernelGGL(k_cc_gidm, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, perm, goff, nm, G, gidm);
}
void hawk_launch_cs_gid(hipStream_t st, const ClDict& cd, const void* res, const uint64_t* moff, const uint64_t* offsets, uint64_t r0, uint64_t n,
                        const uint32_t* gidm, uint32_t* gid, uint32_t* vals) {
  if (r0) hipLaunchKernelGGL(k_cc_refgid, dim3((unsigned)((r0 + 255) / 256)), dim3(256), 0, st, r0, gidm, gid, vals);
  if (cd.n_inst) hipLaunchKernelGGL(k_cs_gid, dim3((cd.n_inst + 255) / 256), dim3(256), 0, st, cd, static_cast<const uint4*>(res), moff, offsets, r0, n,
                                    gidm, gid, vals);
}
