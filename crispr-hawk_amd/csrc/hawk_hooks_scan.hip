// hawk_hooks_scan.hip — entry points of libhawk_hip_hooks.so ONLY (the Makefile links this file into the hooks library and not
// into the product library; include/hawk.h does not know them): the offset scans on buffers of the test's making, so that
// tests/hooks_scan_check.py can run hawk_launch_mscan and hawk_launch_scan2_u32 at sizes, alignments and counts no product call
// of test size reaches.  Every output buffer is filled with a sentinel first, guard words behind its last element included.
#include <cstring>

#include "hawk_host.h"

#define HOOK_SENTINEL_BYTE 0xA5  // every byte of an unwritten word: 0xA5A5A5A5(A5A5A5A5)
#define HOOK_GUARD 16            // guard words behind the last element

static inline char* hook_align16(void* p) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15); }

// counts[n] -> offsets_out[n], guard_out[16] (the words behind offsets[n - 1]), totals_out[4] (n_keep, n_keep_fwd, n_cand, n_hits),
// *route_out (HAWK_MSCAN_*).  shards: 512 values (256 pairs) or null.  shift_counts / shift_offsets in {0, 1}: the device pointer
// moved by one element off its 16-byte boundary.  The partials are sized as every caller sizes them.  n == 0 is refused: no caller
// passes it (see hawk_launch_mscan) and without shard sums it would be a launch of 0 workgroups.
extern "C" __attribute__((visibility("default"))) int hawk_hook_mscan(hawk_ctx* ctx, const uint32_t* counts, uint64_t n,
                                                                      const unsigned long long* shards, int shift_counts,
                                                                      int shift_offsets, uint64_t* offsets_out, uint64_t* guard_out,
                                                                      uint64_t* totals_out, int* route_out) {
  if (!ctx || !counts || !n || !offsets_out || !guard_out || !totals_out || !route_out) return HAWK_E_INVALID;
  if ((shift_counts | shift_offsets) & ~1) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  PoolScope tmp;
  char *b_counts, *b_offsets;
  unsigned long long *d_partial, *d_shards = nullptr;
  ScanTotals* d_tot;
  const size_t off_words = (size_t)n + HOOK_GUARD + 1;  // + the element the shift skips
  TEMPCHK(tmp, &b_counts, ((size_t)n + 1) * 4 + 16);
  TEMPCHK(tmp, &b_offsets, off_words * 8 + 16);
  TEMPCHK(tmp, &d_partial, ((size_t)n / 1024 + 2) * 8);
  TEMPCHK(tmp, &d_tot, sizeof(ScanTotals));
  if (shards) TEMPCHK(tmp, &d_shards, 512 * 8);
  uint32_t* const d_counts = reinterpret_cast<uint32_t*>(hook_align16(b_counts)) + shift_counts;
  char* const a_offsets = hook_align16(b_offsets);
  uint64_t* const d_offsets = reinterpret_cast<uint64_t*>(a_offsets) + shift_offsets;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(d_counts, counts, (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (shards) HIPCHK(hipMemcpyAsync(d_shards, shards, 512 * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(a_offsets, HOOK_SENTINEL_BYTE, off_words * 8, st));
  HIPCHK(hipMemsetAsync(d_tot, HOOK_SENTINEL_BYTE, sizeof(ScanTotals), st));
  const bool aligned = (reinterpret_cast<uintptr_t>(d_counts) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_offsets) & 15) == 0;
  *route_out = hawk_mscan_route(n, shards != nullptr, aligned);
  hawk_launch_mscan(st, d_counts, n, d_partial, d_shards, d_offsets, d_tot);
  HIPCHK(hipGetLastError());
  ScanTotals tot;
  HIPCHK(hipMemcpyAsync(offsets_out, d_offsets, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(guard_out, d_offsets + n, HOOK_GUARD * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  totals_out[0] = tot.n_keep; totals_out[1] = tot.n_keep_fwd; totals_out[2] = tot.n_cand; totals_out[3] = tot.n_hits;
  return HAWK_OK;
}

// cnt_a[n], cnt_b[n] -> off_a_out / off_b_out [n + 1 + 16]: the n + 1 offsets and the 16 guard words behind them.
// desc: n_desc 64-bit words or null -> bits_out[n_desc / 32 + 2]: the bitmap's n_desc / 32 + 1 words and one guard word.
extern "C" __attribute__((visibility("default"))) int hawk_hook_scan2_u32(hawk_ctx* ctx, const uint32_t* cnt_a, const uint32_t* cnt_b,
                                                                          uint32_t n, const unsigned long long* desc, uint32_t n_desc,
                                                                          uint32_t* off_a_out, uint32_t* off_b_out, uint32_t* bits_out) {
  if (!ctx || !cnt_a || !cnt_b || !n || !off_a_out || !off_b_out || (desc && (!n_desc || !bits_out))) return HAWK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->device));
  PoolScope tmp;
  char *b_a, *b_b, *b_oa, *b_ob, *b_desc = nullptr, *b_bits = nullptr;
  const size_t off_words = (size_t)n + 1 + HOOK_GUARD, bit_words = (size_t)n_desc / 32 + 2;
  TEMPCHK(tmp, &b_a, (size_t)n * 4 + 16);
  TEMPCHK(tmp, &b_b, (size_t)n * 4 + 16);
  TEMPCHK(tmp, &b_oa, off_words * 4 + 16);
  TEMPCHK(tmp, &b_ob, off_words * 4 + 16);
  if (desc) {
    TEMPCHK(tmp, &b_desc, (size_t)n_desc * 8 + 16);
    TEMPCHK(tmp, &b_bits, bit_words * 4 + 16);
  }
  uint32_t* const d_a = reinterpret_cast<uint32_t*>(hook_align16(b_a));
  uint32_t* const d_b = reinterpret_cast<uint32_t*>(hook_align16(b_b));
  uint32_t* const d_oa = reinterpret_cast<uint32_t*>(hook_align16(b_oa));
  uint32_t* const d_ob = reinterpret_cast<uint32_t*>(hook_align16(b_ob));
  unsigned long long* const d_desc = desc ? reinterpret_cast<unsigned long long*>(hook_align16(b_desc)) : nullptr;
  uint32_t* const d_bits = desc ? reinterpret_cast<uint32_t*>(hook_align16(b_bits)) : nullptr;
  hipStream_t st = ctx->stream;
  HIPCHK(hipMemcpyAsync(d_a, cnt_a, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_b, cnt_b, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_oa, HOOK_SENTINEL_BYTE, off_words * 4, st));
  HIPCHK(hipMemsetAsync(d_ob, HOOK_SENTINEL_BYTE, off_words * 4, st));
  if (desc) {
    HIPCHK(hipMemcpyAsync(d_desc, desc, (size_t)n_desc * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_bits, HOOK_SENTINEL_BYTE, bit_words * 4, st));
  }
  hawk_launch_scan2_u32(st, d_a, d_b, n, d_oa, d_ob, d_desc, d_bits, n_desc);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(off_a_out, d_oa, off_words * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(off_b_out, d_ob, off_words * 4, hipMemcpyDeviceToHost, st));
  if (desc) HIPCHK(hipMemcpyAsync(bits_out, d_bits, bit_words * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}
