// hawk_hooks_emit.hip — entry points of libhawk_hip_hooks.so ONLY (the Makefile links this file into the hooks library and not
// into the product library; include/hawk.h does not know them): the emit pass of the cluster search, k_cs_emit_rows, on instance
// records and template rows of the test's making, so that tests/hooks_emit_check.py can put a wave's row total on either side of
// a chunk, an empty wave between two full ones and an instance count on either side of a wave - which no search of test size pins.
// The table and 16 guard rows behind it are filled with a sentinel byte first.
#include <cstring>
#include <vector>

#include "hawk_host.h"

#define HOOK_SENTINEL_BYTE 0xA5  // every byte of an unwritten row
#define HOOK_GUARD_ROWS 16       // guard rows behind the table's capacity
#define HOOK_ROW_BYTES 64
#define HOOK_WAVE 64  // instances per offset: one wave of k_cs_count

// what hawk_launch_cs_emit_rows launches: instances per wave, rows per chunk; and where a packed row keeps its haplotype row
extern "C" __attribute__((visibility("default"))) int hawk_hook_cs_emit_geometry(uint32_t* inst_per_wave, uint32_t* rows_per_chunk,
                                                                                 uint32_t* hap_shift, uint32_t* max_hap) {
  if (!inst_per_wave || !rows_per_chunk || !hap_shift || !max_hap) return HAWK_E_INVALID;
  hawk_cs_emit_geometry(inst_per_wave, rows_per_chunk);
  *hap_shift = HAWK_ROW_HAP_SHIFT; *max_hap = HAWK_ROW_MAX_HAP;
  return HAWK_OK;
}

// inst[n_inst][4] {rows, first template row, haplotype row << HAWK_ROW_HAP_SHIFT, position} (what k_cs_count leaves),
// trows[n_trows][16] -> table_out[cap][16], guard_out[16][16], *status_out.  The offsets are made as the search makes them: one
// count per 64 instances (the wave sums of k_cs_count), scanned by hawk_launch_mscan.  t_count / t_cap: the template counter and
// its reservation (t_count > t_cap: the search that overflowed, no row may be written).  Every instance's template rows must lie
// inside trows (checked here: the kernel trusts its records).
extern "C" __attribute__((visibility("default"))) int hawk_hook_cs_emit(hawk_ctx* ctx, const uint32_t* inst, uint32_t n_inst, const uint32_t* trows,
                                                                        uint64_t n_trows, uint64_t t_count, uint64_t t_cap, uint64_t cap,
                                                                        uint32_t* table_out, uint32_t* guard_out, int* status_out) {
  if (!ctx || !inst || !n_inst || !trows || !n_trows || !guard_out || !status_out || (cap && !table_out)) return HAWK_E_INVALID;
  if (hawk_cs_row_bytes() != HOOK_ROW_BYTES) return HAWK_E_INVALID;
  const uint64_t ng = ((uint64_t)n_inst + HOOK_WAVE - 1) / HOOK_WAVE;
  std::vector<uint32_t> gsum(ng, 0u);
  for (uint32_t i = 0; i < n_inst; ++i) {
    const uint64_t rows = inst[4 * (size_t)i], tb = inst[4 * (size_t)i + 1];
    if (rows && tb + rows > n_trows) return HAWK_E_INVALID;
    if (!rows && tb >= n_trows) return HAWK_E_INVALID;  // (a chunk's clamp never reads an instance of no rows, but keep every record valid)
    if ((uint64_t)gsum[i / HOOK_WAVE] + rows > 0xffffffffull) return HAWK_E_INVALID;
    gsum[i / HOOK_WAVE] += (uint32_t)rows;
  }
  HIPCHK(hipSetDevice(ctx->device));
  PoolScope tmp;
  char *d_inst, *d_trows, *d_rows;
  uint32_t* d_gsum;
  uint64_t* d_offsets;
  unsigned long long *d_partial, *d_tcount;
  ScanTotals* d_tot;
  int* d_status;
  const size_t table_bytes = ((size_t)cap + HOOK_GUARD_ROWS) * HOOK_ROW_BYTES;
  TEMPCHK(tmp, &d_inst, (size_t)n_inst * 16);
  TEMPCHK(tmp, &d_trows, (size_t)n_trows * HOOK_ROW_BYTES);
  TEMPCHK(tmp, &d_rows, table_bytes);
  TEMPCHK(tmp, &d_gsum, (size_t)ng * 4);
  TEMPCHK(tmp, &d_offsets, (size_t)ng * 8);
  TEMPCHK(tmp, &d_partial, ((size_t)ng / 1024 + 2) * 8);
  TEMPCHK(tmp, &d_tot, sizeof(ScanTotals));
  TEMPCHK(tmp, &d_tcount, 8);
  TEMPCHK(tmp, &d_status, 4);
  hipStream_t st = ctx->stream;
  const unsigned long long tc = t_count;
  HIPCHK(hipMemcpyAsync(d_inst, inst, (size_t)n_inst * 16, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_trows, trows, (size_t)n_trows * HOOK_ROW_BYTES, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_gsum, gsum.data(), (size_t)ng * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_tcount, &tc, 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_rows, HOOK_SENTINEL_BYTE, table_bytes, st));
  HIPCHK(hipMemsetAsync(d_status, 0, 4, st));
  hawk_launch_mscan(st, d_gsum, ng, d_partial, nullptr, d_offsets, d_tot);
  hawk_launch_cs_emit_rows(st, n_inst, d_inst, d_trows, d_offsets, d_tcount, t_cap, d_rows, cap, d_status);
  HIPCHK(hipGetLastError());
  if (cap) HIPCHK(hipMemcpyAsync(table_out, d_rows, (size_t)cap * HOOK_ROW_BYTES, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(guard_out, d_rows + (size_t)cap * HOOK_ROW_BYTES, (size_t)HOOK_GUARD_ROWS * HOOK_ROW_BYTES, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(status_out, d_status, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return HAWK_OK;
}
