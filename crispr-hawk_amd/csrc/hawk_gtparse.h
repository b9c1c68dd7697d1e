// hawk_gtparse.h - one record of VCF sample columns -> two allele codes per sample and the record's flag byte: the body of
// k_gt_parse (hawk_vcf.hip, "a|b") and k_gt_parse_unphased (hawk_ubuild.hip, "a/b"), which differ in the separator of a plain
// field and in the function every other field goes through.  One workgroup of 256 threads per record: tabs are counted per
// 16-byte chunk, a workgroup scan gives every chunk the index of its first field, and the thread that owns a field start parses
// it.  Device code; include after hawk_bits.h.
#pragma once
#include "hawk_bits.h"

#define GT_CHUNK 16

// SEP: the separator of a plain field.  Classify: a functor (text, field start, record end) -> flags | code0 << 8 | code1 << 16 for
// a field that is not a plain "a SEP b" ended by a tab, a ':' or the record.
template <uint8_t SEP, class Classify>
__device__ __forceinline__ void gt_parse_record(const uint8_t* __restrict__ text, const uint64_t* __restrict__ line_off,
                                                const uint64_t* __restrict__ gt_off, uint32_t n_samples, uint8_t* __restrict__ codes,
                                                uint8_t* __restrict__ flags, Classify classify) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_flag;
  const uint32_t tid = threadIdx.x;
  const uint64_t rec = blockIdx.x;
  const uint64_t lo = gt_off[rec];
  uint64_t hi = line_off[rec + 1];  // one past the '\n'
  while (hi > lo && (text[hi - 1] == '\n' || text[hi - 1] == '\r')) --hi;  // workgroup-uniform
  if (tid == 0) s_flag = 0;
  __syncthreads();
  uint8_t* out = codes + rec * 2ull * n_samples;
  uint32_t field_base = 0, myflag = 0;
  for (uint64_t base = lo; base < hi; base += 256ull * GT_CHUNK) {  // workgroup-uniform trip count
    const uint64_t a = base + (uint64_t)tid * GT_CHUNK;
    uint8_t c[GT_CHUNK];
    uint32_t ntab = 0;
#pragma unroll
    for (int k = 0; k < GT_CHUNK; ++k) {
      c[k] = a + k < hi ? text[a + k] : 0;
      ntab += c[k] == '\t';
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan<4>(ntab, s_w, &tot);
    uint32_t f = field_base + ex;  // index of the field the chunk's first byte belongs to
    uint8_t prev = a == lo ? (uint8_t)'\t' : (a < hi ? text[a - 1] : 0);
#pragma unroll 1
    for (int k = 0; k < GT_CHUNK; ++k) {
      if (a + k >= hi) break;
      if (prev == '\t') {  // a field starts here; f counts the tabs before it
        if (f < n_samples) {
          uint64_t p = a + k;
          uint32_t v[2] = {255u, 255u};
          bool plain = true;  // "a SEP b" ended by a tab, a ':' or the record: every field of a well-formed file
          for (int nal = 0; nal < 2; ++nal) {
            uint8_t ch = p < hi ? text[p] : (uint8_t)'\t';
            if (ch == '.') { v[nal] = 255u; ++p; }
            else if (ch >= '0' && ch <= '9') {
              uint32_t x = 0;
              while (p < hi && (ch = text[p]) >= '0' && ch <= '9') { x = x * 10u + (ch - '0'); if (x > 254u) x = 254u; ++p; }
              v[nal] = x;
            } else { plain = false; break; }
            if (nal == 0) {
              if (p < hi && text[p] == SEP) ++p;
              else { plain = false; break; }
            }
          }
          if (plain) {
            const uint8_t endc = p < hi ? text[p] : (uint8_t)'\t';
            plain = endc == '\t' || endc == ':';
          }
          if (!plain) {
            const uint32_t r = classify(text, a + k, hi);
            myflag |= r & 0xffu;
            v[0] = (r >> 8) & 0xffu;
            v[1] = (r >> 16) & 0xffu;
          }
          out[2ull * f] = (uint8_t)v[0];
          out[2ull * f + 1] = (uint8_t)v[1];
        }
      }
      prev = c[k];
      f += c[k] == '\t';
    }
    field_base += tot;
  }
  // fields = tabs + 1 (an empty section has no field at all)
  const uint32_t nfields = hi > lo ? field_base + 1 : 0;
  if (nfields != n_samples) myflag |= 2u;
  // a tab as the section's last byte: the last field is empty and starts at hi, where no chunk owns it - the empty genotype's
  // flags (one part, no number) are set here, its codes stay 255
  if (tid == 0 && hi > lo && text[hi - 1] == '\t' && field_base < n_samples) myflag |= 5u;
  if (myflag) atomicOr(&s_flag, myflag);
  __syncthreads();
  if (tid == 0) flags[rec] = (uint8_t)s_flag;
}
