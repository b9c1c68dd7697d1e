// hawk_inflate.hip - k_bz_inflate: BGZF members -> text, one wavefront per member (the decoder itself: hawk_inflate.h)
//
// A member is serial - a symbol's first bit is known only when the one before it is decoded - and members are independent, so a
// wave takes a member: its 64 lanes run the decoder of hawk_inflate.h in step, the bit reader's state equal in all of them (the
// bytes they read and the table entries they look up go through readfirstlane, so the state lives in scalar registers and every
// branch is a scalar one), and split only what the header splits: building the code tables (a ballot per code length counts and
// ranks 64 symbols at a time), clearing them, writing a batch's literals, copying a match or a stored block.  Tables and token
// batch are the wave's own 2944 bytes of LDS; four waves make a workgroup, which share nothing and never meet at a barrier: a
// wave whose member is the 28-byte end marker ends while its neighbour is still in a 64 KiB block.
#include <hip/hip_runtime.h>

#include "hawk_device.h"
#include "hawk_inflate.h"

#define BZ_WAVES 4  // per workgroup

struct BzWave {
  static constexpr uint32_t lanes = 64;
  __device__ static uint32_t lane() { return threadIdx.x & 63u; }
  __device__ static uint64_t ballot(bool p) { return __ballot(p); }
  __device__ static uint64_t lt_mask() { return (1ull << (threadIdx.x & 63u)) - 1ull; }
  // The lanes of a wave issue their LDS and global accesses in program order; what has to be kept is the compiler's order.
  __device__ static void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __device__ static uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

__global__ __launch_bounds__(64 * BZ_WAVES) void k_bz_inflate(BzDev B, unsigned long long* stamp) {
  hawk_stamp(stamp);
  __shared__ BzTables tables[BZ_WAVES];
  const uint32_t wave = BzWave::uni(threadIdx.x >> 6);
  const uint64_t k = (uint64_t)blockIdx.x * BZ_WAVES + wave;
  if (k >= B.n) return;
  const uint64_t c0 = B.c_off[k], c1 = B.c_off[k + 1], u0 = B.u_off[k], u1 = B.u_off[k + 1];
  const uint32_t st = bz_inflate_member<BzWave>(B.in + (c0 - B.c_off[0]), c1 - c0, B.out + (u0 - B.u_off[0]), u1 - u0, &tables[wave]);
  if ((threadIdx.x & 63u) == 0) B.status[k] = (uint8_t)st;
}

void hawk_launch_bz_inflate(hipStream_t st, const BzDev& B, unsigned long long* stamp) {
  if (!B.n) return;
  hipLaunchKernelGGL(k_bz_inflate, dim3((B.n + BZ_WAVES - 1) / BZ_WAVES), dim3(64 * BZ_WAVES), 0, st, B, stamp);
}
