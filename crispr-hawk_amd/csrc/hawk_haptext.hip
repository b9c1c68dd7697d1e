// hawk_haptext.hip - the rows of an expansion plan as text: what haplotypes_table (haplotypes.py:818-859) writes into the
// `haplotype` column of haplotypes_table_{contig}_{start}_{stop}.tsv - the cased IUPAC string of every haplotype, alt
// bases in lower case (haplotype.py:120).
//
//   k_hx_text  one workgroup per (listed row, tile of 32768 output positions).  The first half IS k_hx_build's: the tile's
//              HxTile entry, its records and its image in REF's planes staged in LDS, four words per thread from hx_words_t
//              with every slow branch (hx_tile_quad, hawk_hx.h) - there is no second statement of the expansion, so the
//              text cannot drift from the planes a search sees.  The words then go to LDS as the tile's five planes (the
//              staged REF image is dead by then: the same memory), and the workgroup turns round: a thread no longer owns
//              128 consecutive bases but one 16-byte piece of the DESTINATION at a time, consecutive lanes consecutive
//              pieces.  It funnel-shifts the piece's 16 bases out of each plane (two LDS words per plane; a pair of lanes
//              shares a word, the lanes of a wave read consecutive words: no bank conflict), spreads every four bases'
//              bits into the bytes of a dword (x 0x00204081), looks the nibbles up in the 16 letters - the inverse of
//              encoder.py's table, "ACMGRSVTWYHKDBN" for 1 .. 15, held in four registers and indexed by v_perm_b32 - sets
//              0x20 where the V bit is, and writes one aligned 16-byte vector store.
//
// Destination: row i of a call lands at byte dst_off[i] of a compact device image of the call's rows and is hap_len[row] bytes
// long; the rows' lengths are arbitrary, so a tile's first byte has any of the 16 alignment phases.  The unaligned head and
// tail are handled HERE (not by rows at an aligned pitch and a strided copy): the pieces are cut on the destination's
// 16-byte grid, not on the tile's, which costs nothing - the bit offset of the funnel shift absorbs the phase - and the at
// most two pieces per tile that straddle the tile's (or the row's) ends are written byte by byte, only the bytes that belong
// to the tile.  Neighbouring tiles and rows therefore never write each other's bytes, nothing outside a row's range is
// touched, and the image reaches the host in ONE copy per call instead of one per row (4097 short rows would be 4097 copies).
//
// The plan is read only: records, tile index, REF planes and lengths are const here.
//
// Resources (-O3, gfx950): 69 VGPRs, no scratch, LDS 23632 B (96 records + five planes of 1028 words) -> six workgroups =
// 24 waves per CU (6 per SIMD), LDS-limited; the registers would allow 7 per SIMD.
#include "hawk_hx.h"

#define HT_PW (HX_TW + 4)  // words per plane in LDS: the tile's 1024 and a zero quad behind them (a piece's funnel shift reads word + 1)
static_assert(5 * HT_PW >= 4 * HX_RW, "the tile's planes reuse the staged REF window");

// "?ACMGRSVTWYHKDBN" as the four source registers of two v_perm_b32 (nibble 0 - no base - never occurs inside a row)
constexpr uint32_t ht4(char a, char b, char c, char d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24; }
constexpr uint32_t HT_L0 = ht4('?', 'A', 'C', 'M'), HT_L1 = ht4('G', 'R', 'S', 'V'), HT_H0 = ht4('T', 'W', 'Y', 'H'), HT_H1 = ht4('K', 'D', 'B', 'N');

// four bases (the low four bits of each plane's argument) -> their four letters, first base in the low byte
__device__ __forceinline__ uint32_t ht_letters4(uint32_t a, uint32_t c, uint32_t g, uint32_t t, uint32_t v) {
  const uint32_t M = 0x00204081u;  // bit k of a nibble -> bit 0 of byte k (the shifted copies do not overlap: no carries)
  const uint32_t lo3 = ((a & 15u) * M & 0x01010101u) | ((c & 15u) * (M << 1) & 0x02020202u) | ((g & 15u) * (M << 2) & 0x04040404u);
  const uint32_t st = (t & 15u) * M & 0x01010101u, sv = (v & 15u) * M & 0x01010101u;
  const uint32_t tm = (st << 8) - st;  // 0xff in the bytes whose T bit is set: the upper half of the table
  const uint32_t lo = __builtin_amdgcn_perm(HT_L1, HT_L0, lo3), hi = __builtin_amdgcn_perm(HT_H1, HT_H0, lo3);
  return ((hi & tm) | (lo & ~tm)) | (sv << 5);
}

__global__ __launch_bounds__(HAWK_BLOCK) void k_hx_text(HxArgs g, const uint64_t* __restrict__ hv_off, const uint32_t* __restrict__ hap_len,
                                                         uint32_t wpr /*tiles per row*/, const HxTile* __restrict__ tiles,
                                                         const uint32_t* __restrict__ rows, const uint64_t* __restrict__ dst_off,
                                                         uint8_t* __restrict__ out) {
  __shared__ HxVar s_v[HX_MAXV];
  __shared__ __attribute__((aligned(16))) uint32_t s_buf[5 * HT_PW];
  const uint32_t i = blockIdx.x / wpr, wb = blockIdx.x % wpr;
  const uint32_t h = rows[i];
  const int32_t len = (int32_t)hap_len[h];
  const int64_t left = (int64_t)len - (int64_t)wb * (HX_TW * 32);
  if (left <= 0) return;  // the row ends before this tile (the whole workgroup leaves)
  const int32_t nbytes = left < HX_TW * 32 ? (int32_t)left : HX_TW * 32;
  const uint32_t w0 = wb * HX_TW + threadIdx.x * 4u;
  uint32_t o[5][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  hx_tile_quad(g, hv_off, h, tiles[(size_t)h * wpr + wb] /* k_hx_index */, len, w0, s_v, reinterpret_cast<uint32_t(*)[HX_RW]>(s_buf),
               o[0], o[1], o[2], o[3], o[4]);
  __syncthreads();  // every thread is done with the staged REF image: its memory takes the tile's planes
#pragma unroll
  for (int pl = 0; pl < 5; ++pl) {
    *reinterpret_cast<uint4*>(s_buf + pl * HT_PW + 4 * threadIdx.x) = make_uint4(o[pl][0], o[pl][1], o[pl][2], o[pl][3]);
    if (threadIdx.x == 0) *reinterpret_cast<uint4*>(s_buf + pl * HT_PW + HX_TW) = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  uint8_t* const dst = out + dst_off[i] + (uint64_t)wb * (HX_TW * 32);  // the tile's first byte
  const int32_t a = (int32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const int32_t npiece = (a + nbytes + 15) >> 4;  // <= 2049
  for (int32_t c = (int32_t)threadIdx.x; c < npiece; c += HAWK_BLOCK) {
    const int32_t p = 16 * c - a;  // the piece's first base, relative to the tile
    if (p >= 0 && p + 16 <= nbytes) {
      const uint32_t w = (uint32_t)p >> 5, sh = (uint32_t)p & 31u;
      uint32_t b[5];
#pragma unroll
      for (int pl = 0; pl < 5; ++pl) b[pl] = fsh(s_buf[pl * HT_PW + w], s_buf[pl * HT_PW + w + 1], sh);
      uint4 q;
      q.x = ht_letters4(b[0], b[1], b[2], b[3], b[4]);
      q.y = ht_letters4(b[0] >> 4, b[1] >> 4, b[2] >> 4, b[3] >> 4, b[4] >> 4);
      q.z = ht_letters4(b[0] >> 8, b[1] >> 8, b[2] >> 8, b[3] >> 8, b[4] >> 8);
      q.w = ht_letters4(b[0] >> 12, b[1] >> 12, b[2] >> 12, b[3] >> 12, b[4] >> 12);
      *reinterpret_cast<uint4*>(dst + p) = q;  // dst + p is a multiple of 16
    } else {  // a piece across the tile's first or last byte: only the bytes of the tile, one by one
      for (int32_t j = 0; j < 16; ++j) {
        const int32_t q = p + j;
        if (q < 0 || q >= nbytes) continue;
        const uint32_t w = (uint32_t)q >> 5, bit = (uint32_t)q & 31u;
        dst[q] = (uint8_t)ht_letters4(s_buf[w] >> bit, s_buf[HT_PW + w] >> bit, s_buf[2 * HT_PW + w] >> bit, s_buf[3 * HT_PW + w] >> bit,
                                      s_buf[4 * HT_PW + w] >> bit);
      }
    }
  }
}

// n_rows listed rows of a plan -> text at out + dst_off[i] (device pointers; hawk_xplan_text).  The grid is cut so that no launch
// exceeds 2^30 workgroups.
void hawk_launch_hx_text(hipStream_t st, const uint32_t* const* ref, uint32_t ref_S, const void* recs, const uint8_t* alt_codes,
                         const uint64_t* hv_off, const uint32_t* hap_len, uint32_t S, const void* tiles, uint32_t n_rows, const uint32_t* rows,
                         const uint64_t* dst_off, uint8_t* out) {
  const uint32_t wpr = hawk_hx_tiles_per_row(S);
  HxArgs g;
  for (int p = 0; p < 4; ++p) g.ref[p] = ref[p];
  g.ref_S = ref_S; g.recs = (const HxVar*)recs; g.alt_codes = alt_codes;
  const uint32_t step = (1u << 30) / wpr ? (1u << 30) / wpr : 1u;
  for (uint32_t r = 0; r < n_rows; r += step) {
    const uint32_t n = n_rows - r < step ? n_rows - r : step;
    hipLaunchKernelGGL(k_hx_text, dim3(n * wpr), dim3(HAWK_BLOCK), 0, st, g, hv_off, hap_len, wpr, (const HxTile*)tiles, rows + r, dst_off + r, out);
  }
}
