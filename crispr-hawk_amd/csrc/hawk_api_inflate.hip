// hawk_api_inflate.hip - C ABI: BGZF members -> text on the device (include/hawk.h; kernel: hawk_inflate.hip; the rules: hawk_inflate.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "hawk_host.h"
#include "hawk_inflate.h"

extern "C" {

int hawk_bgzf_inflate(hawk_ctx* ctx, const uint8_t* in, uint64_t in_bytes, const uint64_t* c_off, const uint64_t* u_off,
                      uint32_t n_members, uint8_t* out, uint8_t* status, hawk_bgzf_timing* timing) {
  if (timing) memset(timing, 0, sizeof(*timing));
  if (!ctx || !bz_args_ok(in, in_bytes, c_off, u_off, n_members, out, status)) return HAWK_E_INVALID;
  if (!n_members) return HAWK_OK;
  const uint64_t n = n_members, cbytes = c_off[n] - c_off[0], ubytes = u_off[n] - u_off[0];
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PoolScope tmp;
  BzDev B = {};
  uint8_t* d_in = nullptr;
  uint64_t *d_coff = nullptr, *d_uoff = nullptr;
  // the call's laps by the device's wall clock: begin, kernel begins (its own first stamp), kernel done, downloads done
  unsigned long long *d_stamps = nullptr, h_stamps[4] = {0, 0, 0, 0};
  TEMPCHK(tmp, &d_in, std::max<uint64_t>(cbytes, 1));
  TEMPCHK(tmp, &d_coff, (n + 1) * 8);
  TEMPCHK(tmp, &d_uoff, (n + 1) * 8);
  TEMPCHK(tmp, &B.out, std::max<uint64_t>(ubytes, 1));
  TEMPCHK(tmp, &B.status, n);
  TEMPCHK(tmp, &d_stamps, sizeof(h_stamps));
  B.in = d_in; B.c_off = d_coff; B.u_off = d_uoff; B.n = n_members;
  HIPCHK(hipMemsetAsync(d_stamps, 0, sizeof(h_stamps), st));
  hawk_launch_stamp(st, d_stamps + 0);
  if (cbytes) HIPCHK(hipMemcpyAsync(d_in, in + c_off[0], cbytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_coff, c_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_uoff, u_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
  hawk_launch_bz_inflate(st, B, d_stamps + 1);
  hawk_launch_stamp(st, d_stamps + 2);
  HIPCHK(hipGetLastError());
  if (ubytes) HIPCHK(hipMemcpyAsync(out + u_off[0], B.out, ubytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(status, B.status, n, hipMemcpyDeviceToHost, st));
  hawk_launch_stamp(st, d_stamps + 3);
  HIPCHK(hipMemcpyAsync(h_stamps, d_stamps, sizeof(h_stamps), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the caller's arrays may go once this returns
  uint32_t failed = 0;
  for (uint64_t k = 0; k < n; ++k) failed += status[k] != HAWK_BZ_OK;
  if (timing) {
    timing->upload_ms = hawk_stamp_ms(ctx, h_stamps[0], h_stamps[1]);
    timing->inflate_ms = hawk_stamp_ms(ctx, h_stamps[1], h_stamps[2]);
    timing->download_ms = hawk_stamp_ms(ctx, h_stamps[2], h_stamps[3]);
    timing->total_ms = hawk_stamp_ms(ctx, h_stamps[0], h_stamps[3]);
    timing->in_bytes = cbytes; timing->out_bytes = ubytes; timing->n_members = n_members; timing->n_failed = failed;
  }
  return failed ? HAWK_E_INVALID : HAWK_OK;
}

}  // extern "C"
