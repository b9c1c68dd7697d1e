// hawk_ottext.hip - the rows of offtargets_{contig}_{start}_{stop}.tsv from hit records, on the device: what
// offtargets.report_offtargets made one Python object, one CRISPRitz line, one parse and one join per site of
// (offtargets.py:296-363, 486-558 of the reference).  The row's every byte is ot_text_row (hawk_ottext.h), the function the
// host twin (hawk_host_offtarget_text) runs too.  count -> scan -> fill, no atomics for places:
//
//   k_ot_text_len    one thread per OUTPUT row i (= record order[i]): ot_text_row into a counting sink -> the row's bytes and its
//                    CFD in 1e-4 units (-1: NA or unscorable); the unscorable rows of a workgroup are counted with one atomic.
//   k_ann_scan1-3    (hawk_annot.hip, hawk_launch_ann_offsets) the exclusive 64-bit sums of the lengths
//   k_ot_text_fill   a wave owns 64 consecutive output rows, whose bytes are ONE contiguous range of the blob.  Each lane composes
//                    its row in the wave's LDS slot, at the row's offset inside the range shifted by the phase of the range's first
//                    byte on the destination's 16-byte grid - LDS and destination then share that grid -, and the wave copies the
//                    range out: aligned 16-byte pieces as one dwordx4 store per lane, consecutive lanes consecutive pieces; the
//                    pieces across the range's first and last byte go byte by byte, only the bytes of the range (the rule of
//                    k_hx_text).  A range that does not fit the slot (contig names of hundreds of bytes) is written by its lanes
//                    straight to global memory.  Either way a wave writes its own rows' bytes and no others.
//
// Integer / bitwise work and fp64 table products; nothing here has an MFMA shape.  The job is small next to the scan that feeds
// it (4.4x10^5 rows are ~35 MB): what it buys is the per-row Python it replaces, so nothing is tuned beyond coalesced stores.
//
// Resources (-O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_ot_text_len 36 VGPRs, 256 B LDS, occupancy 8 waves / SIMD;
// k_ot_text_fill 46 VGPRs, 32768 B LDS (four slots), occupancy 5, LDS-limited; no scratch in either.
#include <hip/hip_runtime.h>

#include "hawk_device.h"

#define OTT_BLOCK 256
#define OTT_SLOT 8192  // bytes of LDS per wave: 64 rows of up to ~127 bytes each (a row with a 17-byte contig name has ~105)

namespace {

struct OtTextRow {
  OtTextRec rec;
  uint64_t gcode, pos, name_len;
  const uint8_t* name;
};

__device__ __forceinline__ OtTextRow ott_load(const OtTextDev& A, uint64_t i) {
  const uint64_t j = A.order ? A.order[i] : i;
  OtTextRow r;
  r.rec.guide = A.guide[j]; r.rec.row = A.row[j]; r.rec.q = A.q[j]; r.rec.nmask = A.nmask[j];
  r.rec.code = A.code[j]; r.rec.gaps = A.gaps[j];
  r.rec.strand = A.strand[j]; r.rec.mm = A.mm[j]; r.rec.kind = A.kind[j]; r.rec.size = A.size[j];
  r.gcode = A.guides2[r.rec.guide];
  const uint32_t c = A.row_contig[r.rec.row];
  r.pos = A.row_off[r.rec.row] + r.rec.q;
  const uint64_t a = A.name_off[c];
  r.name = A.names + a;
  r.name_len = A.name_off[c + 1] - a;
  return r;
}

__global__ __launch_bounds__(OTT_BLOCK) void k_ot_text_len(OtTextDev A, uint64_t* __restrict__ len, int64_t* __restrict__ cfd_e4,
                                                            unsigned long long* __restrict__ n_unscorable) {
  const uint64_t i = (uint64_t)blockIdx.x * OTT_BLOCK + threadIdx.x;
  int uns = 0;
  if (i < A.n) {
    const OtTextRow r = ott_load(A, i);
    OtTextCount s;
    const long long u = ot_text_row(r.rec, r.gcode, r.name, r.name_len, r.pos, A.fmt, A.tab, s);
    len[i] = s.n;
    cfd_e4[i] = u < 0 ? -1 : u;
    uns = u == OT_TEXT_UNSCORABLE;
  }
  const int c = __syncthreads_count(uns);  // every thread of the workgroup is here
  if (threadIdx.x == 0 && c) atomicAdd(n_unscorable, (unsigned long long)c);
}

__global__ __launch_bounds__(OTT_BLOCK) void k_ot_text_fill(OtTextDev A, const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t s_buf[OTT_BLOCK / 64][OTT_SLOT];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint64_t r0 = ((uint64_t)blockIdx.x * (OTT_BLOCK / 64) + w) * 64;  // the wave's first output row (wave-uniform)
  const bool wave_on = r0 < A.n;
  const uint64_t r1 = wave_on ? (r0 + 64 < A.n ? r0 + 64 : A.n) : r0;
  const uint64_t b0 = wave_on ? off[r0] : 0, total = wave_on ? off[r1] - b0 : 0;  // the wave's range of the blob
  uint8_t* const dst = out + b0;
  const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const bool staged = a + total <= OTT_SLOT;  // wave-uniform
  const uint64_t i = r0 + lane;
  if (i < r1) {
    const OtTextRow r = ott_load(A, i);
    const uint64_t rel = off[i] - b0;
    OtTextBytes s;
    s.w = staged ? &s_buf[w][a + rel] : dst + rel;
    (void)ot_text_row(r.rec, r.gcode, r.name, r.name_len, r.pos, A.fmt, A.tab, s);
  }
  __syncthreads();  // the rows of every staged wave are in LDS (no thread left before this point)
  if (!staged || !total) return;
  const uint32_t nbytes = (uint32_t)total, npiece = (a + nbytes + 15u) >> 4;  // <= OTT_SLOT / 16
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

void hawk_launch_ot_text_len(hipStream_t st, const OtTextDev& A, uint64_t* len, int64_t* cfd_e4, unsigned long long* n_unscorable) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_ot_text_len, dim3((unsigned)((A.n + OTT_BLOCK - 1) / OTT_BLOCK)), dim3(OTT_BLOCK), 0, st, A, len, cfd_e4, n_unscorable);
}

void hawk_launch_ot_text_fill(hipStream_t st, const OtTextDev& A, const uint64_t* off, uint8_t* out) {
  if (!A.n) return;
  hipLaunchKernelGGL(k_ot_text_fill, dim3((unsigned)((A.n + OTT_BLOCK - 1) / OTT_BLOCK)), dim3(OTT_BLOCK), 0, st, A, off, out);
}
