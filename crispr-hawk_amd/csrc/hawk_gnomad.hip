// hawk_gnomad.hip - gnomAD sites VCF records -> the lines of the population-genotype VCF, on the device: what the reference's
// converter (converter.py:148-214, 246-250) does with one pysam object, ten INFO look-ups and one join per record.  The raw
// text of a batch of data lines goes to HBM once; every rule is a function of hawk_gnomad.h, which the host twin
// (hawk_host_gnomad_lines) runs too.
//
//   k_gn_scan       one 256-thread workgroup per record, the record swept in 4096-byte pieces of 16-byte chunks as k_gt_parse
//                   (hawk_vcf.hip) sweeps one: tabs counted per chunk, a workgroup scan gives every chunk the index of the field
//                   its first byte belongs to.  The thread that owns a field start records it (first eight fields); the thread
//                   that owns an entry start inside INFO compares the bytes behind it with the key table (<= 31 keys, data in
//                   LDS, plus "AF" in slot 31) and keeps the LOWEST position per key with an LDS atomicMin: the first
//                   occurrence wins, whichever sweep or thread finds it.  Commas inside ALT are counted on the way.  After the
//                   sweep one thread per key reads its value (gn_value), one thread composes the flags (gn_record_flags).
//                   ~53 bytes written per record against kilobytes read.
//   k_gn_kept       1 per record without flags; k_ann_scan1-3 (hawk_annot.hip) number the kept records
//   k_gn_text_len   one thread per record: gn_line into a counting sink; k_ann_scan1-3 place the lines
//   k_gn_text_fill  a wave owns 64 consecutive records, whose lines are ONE contiguous range of the blob: each lane composes
//                   its line in the wave's LDS slot at the range's phase on the destination's 16-byte grid, then the wave copies
//                   the range out in aligned dwordx4 pieces, consecutive lanes consecutive pieces (the rule of k_ot_text_fill).
//                   A range beyond the slot (kilobase ALT alleles) is written by its lanes straight to global memory.
//
// Byte compares and integer work only; the scan is bound by reading the text.
#include <hip/hip_runtime.h>

#include "hawk_bits.h"

#define GN_CHUNK 16
#define GN_BLOCK 256
#define GN_KEY_LDS GN_MAX_KEY_BYTES  // bytes of LDS for the keys' text: gn_args_ok
#define GN_SLOT 8192     // bytes of LDS per wave in the fill pass: 64 lines of ~110 bytes

namespace {

__global__ __launch_bounds__(GN_BLOCK) void k_gn_scan(GnDev G) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_pos[32];    // lowest entry start per key (slot 31: AF), relative to the record
  __shared__ uint32_t s_field[8];
  __shared__ uint32_t s_koff[33];
  __shared__ uint32_t s_first[8];   // bitmap of the keys' first bytes
  __shared__ uint32_t s_misc[3];    // commas in ALT, keys absent, values in error
  __shared__ uint32_t s_mask;
  __shared__ uint8_t s_key[GN_KEY_LDS + 2];
  const uint32_t tid = threadIdx.x;
  const uint64_t rec = blockIdx.x;
  const uint8_t* __restrict__ text = G.text;
  const uint64_t lo = G.line_off[rec];
  uint64_t hi = G.line_off[rec + 1];  // one past the '\n'
  while (hi > lo && (text[hi - 1] == '\n' || text[hi - 1] == '\r')) --hi;  // workgroup-uniform
  const uint32_t len = (uint32_t)(hi - lo);
  const uint32_t nk = G.n_keys, kbytes = G.key_off[nk];
  if (tid < 32) s_pos[tid] = GN_ABSENT;
  if (tid < 8) { s_field[tid] = len; s_first[tid] = 0; }
  if (tid < 3) s_misc[tid] = 0;
  if (tid == 0) s_mask = 0;
  if (tid <= nk) s_koff[tid] = G.key_off[tid];
  for (uint32_t k = tid; k < kbytes; k += GN_BLOCK) s_key[k] = G.keys[k];
  if (tid == 0) { s_key[kbytes] = 'A'; s_key[kbytes + 1] = 'F'; }
  __syncthreads();
  if (tid < nk) { const uint8_t c = s_key[s_koff[tid]]; atomicOr(&s_first[c >> 5], 1u << (c & 31u)); }
  if (tid == 0) atomicOr(&s_first['A' >> 5], 1u << ('A' & 31u));
  __syncthreads();
  uint32_t field_base = 0, commas = 0;
  for (uint64_t base = lo; base < hi; base += (uint64_t)GN_BLOCK * GN_CHUNK) {  // workgroup-uniform trip count
    const uint64_t a = base + (uint64_t)tid * GN_CHUNK;
    uint8_t c[GN_CHUNK];
    uint32_t ntab = 0;
#pragma unroll
    for (int k = 0; k < GN_CHUNK; ++k) {
      c[k] = a + k < hi ? text[a + k] : 0;
      ntab += c[k] == '\t';
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan<4>(ntab, s_w, &tot);
    uint32_t f = field_base + ex;  // index of the field the chunk's first byte belongs to
    uint8_t prev = a == lo ? (uint8_t)'\t' : (a < hi ? text[a - 1] : 0);
#pragma unroll 1
    for (int k = 0; k < GN_CHUNK; ++k) {
      if (a + k >= hi) break;
      const uint64_t p = a + k;
      if (prev == '\t' && f < 8) s_field[f] = (uint32_t)(p - lo);  // a field starts here; f counts the tabs before it
      if (f == 4) commas += c[k] == ',';
      if (f == 7 && gn_entry_start(prev) && ((s_first[c[k] >> 5] >> (c[k] & 31u)) & 1u)) {
        for (uint32_t j = 0; j < nk; ++j)
          if (gn_key_at(text, p, hi, s_key + s_koff[j], s_koff[j + 1] - s_koff[j])) atomicMin(&s_pos[j], (uint32_t)(p - lo));
        if (gn_key_at(text, p, hi, s_key + kbytes, 2)) atomicMin(&s_pos[31], (uint32_t)(p - lo));
      }
      prev = c[k];
      f += c[k] == '\t';
    }
    field_base += tot;
  }
  if (commas) atomicAdd(&s_misc[0], commas);
  __syncthreads();
  // fields = tabs + 1
  const bool full = field_base >= 7;
  if (full && tid < nk) {
    const uint32_t p = s_pos[tid];
    if (p == GN_ABSENT) atomicOr(&s_misc[1], 1u);
    else {
      const uint32_t kl = s_koff[tid + 1] - s_koff[tid];
      const int v = gn_key_at(text, lo + p, hi, s_key + s_koff[tid], kl) == 1 ? gn_value(text, lo + p + kl + 1, hi) : 2;
      if (v == 1) atomicOr(&s_mask, 1u << tid);
      if (v == 2) atomicOr(&s_misc[2], 1u);
    }
  }
  __syncthreads();
  if (tid < 8) G.field_off[rec * 8 + tid] = s_field[tid];
  if (tid == 32) {
    uint32_t fl = GN_FEW_FIELDS;
    if (full) fl = gn_record_flags(text + lo, s_field, G.keep, s_misc[1] != 0, s_misc[2] != 0);
    G.flags[rec] = (uint8_t)fl;
    G.mask[rec] = fl ? 0u : s_mask;
  }
  if (tid == 33) gn_spans(text + lo, s_field, len, full, s_pos[31], s_misc[0], G.qual_span + rec * 2, G.af_span + rec * 2);
}

__global__ __launch_bounds__(GN_BLOCK) void k_gn_kept(const uint8_t* __restrict__ flags, uint64_t n, uint64_t* __restrict__ kept) {
  const uint64_t i = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i < n) kept[i] = flags[i] == 0;
}

// what gn_line needs of record i (flags 0)
struct GnLineArgs {
  const uint8_t *rec, *qual, *af;
  uint32_t fo[8];
  uint64_t qual_len, af_len;
  uint32_t mask, n_alt;
  bool af_present;
};
__device__ __forceinline__ GnLineArgs gn_load(const GnDev& G, uint64_t i, const uint64_t* __restrict__ kidx, const uint8_t* pool,
                                              const uint64_t* __restrict__ pool_off, uint64_t n_kept) {
  GnLineArgs L;
  L.rec = G.text + G.line_off[i];
#pragma unroll
  for (int k = 0; k < 8; ++k) L.fo[k] = G.field_off[i * 8 + k];
  L.mask = G.mask[i];
  const uint64_t k = kidx[i];
  const uint64_t q0 = pool_off[k], q1 = pool_off[k + 1], a0 = pool_off[n_kept + k], a1 = pool_off[n_kept + k + 1];
  L.qual = pool + q0; L.qual_len = q1 - q0;
  L.af = pool + a0; L.af_len = a1 - a0;
  L.af_present = G.af_span[i * 2 + 1] != GN_ABSENT;
  L.n_alt = G.af_span[i * 2];
  return L;
}

__global__ __launch_bounds__(GN_BLOCK) void k_gn_text_len(GnDev G, const uint64_t* __restrict__ kidx, const uint8_t* __restrict__ pool,
                                                           const uint64_t* __restrict__ pool_off, uint64_t n_kept, uint64_t* __restrict__ len) {
  const uint64_t i = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= G.n) return;
  uint64_t n = 0;
  if (G.flags[i] == 0) {
    const GnLineArgs L = gn_load(G, i, kidx, pool, pool_off, n_kept);
    GnCount s;
    gn_line(L.rec, L.fo, L.mask, G.n_keys, L.qual, L.qual_len, L.af, L.af_len, L.af_present, L.n_alt, s);
    n = s.n;
  }
  len[i] = n;
}

__global__ __launch_bounds__(GN_BLOCK) void k_gn_text_fill(GnDev G, const uint64_t* __restrict__ kidx, const uint8_t* __restrict__ pool,
                                                            const uint64_t* __restrict__ pool_off, uint64_t n_kept,
                                                            const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_buf[GN_BLOCK / 64][GN_SLOT];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t r0 = ((uint64_t)blockIdx.x * (GN_BLOCK / 64) + w) * 64;  // the wave's first record (wave-uniform)
  const bool wave_on = r0 < G.n;
  const uint64_t r1 = wave_on ? (r0 + 64 < G.n ? r0 + 64 : G.n) : r0;
  const uint64_t b0 = wave_on ? off[r0] : 0, total = wave_on ? off[r1] - b0 : 0;  // the wave's range of the blob
  uint8_t* const dst = out + b0;
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const bool staged = a + total <= GN_SLOT;  // wave-uniform
  const uint64_t i = r0 + lane;
  if (i < r1 && G.flags[i] == 0) {
    const GnLineArgs L = gn_load(G, i, kidx, pool, pool_off, n_kept);
    const uint64_t rel = off[i] - b0;
    GnBytes s;
    s.w = staged ? &s_buf[w][a + rel] : dst + rel;
    gn_line(L.rec, L.fo, L.mask, G.n_keys, L.qual, L.qual_len, L.af, L.af_len, L.af_present, L.n_alt, s);
  }
  __syncthreads();  // the lines of every staged wave are in LDS (no thread left before this point)
  if (!staged || !total) return;
  const uint32_t nbytes = (uint32_t)total, npiece = (a + nbytes + 15u) >> 4;  // <= GN_SLOT / 16
  const uint8_t* const src = &s_buf[w][0];
  for (uint32_t c = lane; c < npiece; c += 64) {
    const int32_t p = (int32_t)(16 * c) - (int32_t)a;  // the piece's first byte, relative to the range
    if (p >= 0 && (uint32_t)p + 16 <= nbytes) {
      *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(src + 16 * c);  // both multiples of 16
    } else {  // across the range's first or last byte: only the bytes of the range, one by one
      for (int32_t j = 0; j < 16; ++j) {
        const int32_t q = p + j;
        if (q >= 0 && (uint32_t)q < nbytes) dst[q] = src[16 * c + j];
      }
    }
  }
}

}  // namespace

void hawk_launch_gn_scan(hipStream_t st, const GnDev& G) {
  if (G.n) hipLaunchKernelGGL(k_gn_scan, dim3((unsigned)G.n), dim3(GN_BLOCK), 0, st, G);
}
void hawk_launch_gn_kept(hipStream_t st, const GnDev& G, uint64_t* kept) {
  if (G.n) hipLaunchKernelGGL(k_gn_kept, dim3((unsigned)((G.n + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, st, G.flags, G.n, kept);
}
void hawk_launch_gn_text_len(hipStream_t st, const GnDev& G, const uint64_t* kidx, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_kept,
                             uint64_t* len) {
  if (G.n) hipLaunchKernelGGL(k_gn_text_len, dim3((unsigned)((G.n + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, st, G, kidx, pool, pool_off, n_kept, len);
}
void hawk_launch_gn_text_fill(hipStream_t st, const GnDev& G, const uint64_t* kidx, const uint8_t* pool, const uint64_t* pool_off, uint64_t n_kept,
                              const uint64_t* off, uint8_t* out) {
  if (G.n)
    hipLaunchKernelGGL(k_gn_text_fill, dim3((unsigned)((G.n + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, st, G, kidx, pool, pool_off, n_kept, off, out);
}
