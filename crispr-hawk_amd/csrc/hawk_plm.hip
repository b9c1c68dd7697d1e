// hawk_plm.hip - PLM-CRISPR forward pass (scores/plm_crispr/train_general.py:53-131, inference: train=False), fp32 throughout.
//   k_plm_protein (+ head)  once per model: text_cnn over the ESM embedding, lin4, relu, sigmoid -> out_protein[256]
//   k_plm_front             per guide: encode, the .view(-1, 5, 59) quirk, conv4 | conv1-3 with sigmoids -> 7552 features
//   k_plm_lin1              [n x K] x [N x K]^T + bias (sigmoid optional) on the f32-input MFMA: lin1, and lin3 as its second use
//   k_plm_tail              per guide: weight_net, softmax, mix, lin5, lin6
// Every row's arithmetic order is fixed by the tiling alone: a guide's score does not depend on its place in the call.
#include "hawk_plm.h"

#include <hip/hip_fp16.h>

#include "../../include/hawk.h"

static_assert(PLM_O_L1W % 4 == 0 && PLM_O_L3W % 4 == 0, "k_plm_lin1 reads its weights as float4");
static_assert(PLM_FEAT % (PLM_TK * PLM_FLUSH) == 0 && PLM_H1 % (PLM_TK * PLM_FLUSH) == 0, "K is whole flush periods");
static_assert(PLM_H1 % PLM_TN == 0 && PLM_H3 % PLM_TN == 0, "N is whole tiles");

__device__ __forceinline__ float plm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------- protein branch
// One block: 128 output channels (one per thread) x PLM_PROT_P positions of one text_cnn convolution.  The embedding rows the
// block needs are staged 32 channels at a time, rounded through fp16 as the reference's loader does (plm_crispr.py:133); a
// stage's products form one fma chain of 32 x KS and are then added to the position's total, which keeps the chains short.
// relu'd values are >= +0, so their bit patterns order like unsigned integers: the global max is an atomicMax on them.
template <int KS>
__global__ __launch_bounds__(PLM_PC) void k_plm_protein(const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ emb, uint32_t L, uint32_t* __restrict__ pooled) {
  const uint32_t P = L - KS + 1, p0 = blockIdx.x * PLM_PROT_P;
  if (p0 >= P) return;
  constexpr int ROWS = PLM_PROT_P + KS - 1;
  __shared__ float E[ROWS][33];
  const int o = threadIdx.x;
  float tot[PLM_PROT_P];
#pragma unroll
  for (int j = 0; j < PLM_PROT_P; ++j) tot[j] = 0.f;
  for (int c0 = 0; c0 < PLM_EMB; c0 += 32) {
    __syncthreads();
    for (int i = threadIdx.x; i < ROWS * 32; i += PLM_PC) {
      const uint32_t r = i >> 5, cc = i & 31, row = p0 + r;
      E[r][cc] = row < L ? __half2float(__float2half_rn(emb[(size_t)row * PLM_EMB + c0 + cc])) : 0.f;
    }
    __syncthreads();
    float part[PLM_PROT_P];
#pragma unroll
    for (int j = 0; j < PLM_PROT_P; ++j) part[j] = 0.f;
    const float* wo = w + ((size_t)o * PLM_EMB + c0) * KS;
    for (int cc = 0; cc < 32; ++cc) {
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const float wv = wo[cc * KS + t];
#pragma unroll
        for (int j = 0; j < PLM_PROT_P; ++j) part[j] = fmaf(wv, E[j + t][cc], part[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < PLM_PROT_P; ++j) tot[j] += part[j];
  }
  float best = 0.f;
#pragma unroll
  for (int j = 0; j < PLM_PROT_P; ++j) {
    const float v = tot[j] + b[o];
    if (p0 + j < P && v > best) best = v;
  }
  atomicMax(&pooled[o], __float_as_uint(best));
}

__global__ __launch_bounds__(PLM_H3) void k_plm_protein_head(const float* __restrict__ w4, const float* __restrict__ b4,
                                                             const uint32_t* __restrict__ pooled, float* __restrict__ out) {
  __shared__ float f[PLM_PFEAT];
  for (int i = threadIdx.x; i < PLM_PFEAT; i += PLM_H3) f[i] = __uint_as_float(pooled[i]);
  __syncthreads();
  const int u = threadIdx.x;
  float acc = 0.f;
  for (int k = 0; k < PLM_PFEAT; ++k) acc = fmaf(w4[u * PLM_PFEAT + k], f[k], acc);
  acc += b4[u];
  out[u] = plm_sigmoid(acc > 0.f ? acc : 0.f);
}

// `pooled` (384 words) must be zero: the running maxima start at +0
void hawk_launch_plm_protein(hipStream_t st, const float* params, const float* emb, uint32_t L, uint32_t* pooled, float* out256) {
  const uint32_t tiles = (L - 5 + 1 + PLM_PROT_P - 1) / PLM_PROT_P;  // the narrowest kernel has the most positions
  hipLaunchKernelGGL(k_plm_protein<5>, dim3(tiles), dim3(PLM_PC), 0, st, params + PLM_O_T0W, params + PLM_O_T0B, emb, L, pooled);
  hipLaunchKernelGGL(k_plm_protein<9>, dim3(tiles), dim3(PLM_PC), 0, st, params + PLM_O_T1W, params + PLM_O_T1B, emb, L, pooled + PLM_PC);
  hipLaunchKernelGGL(k_plm_protein<13>, dim3(tiles), dim3(PLM_PC), 0, st, params + PLM_O_T2W, params + PLM_O_T2B, emb, L,
                     pooled + 2 * PLM_PC);
  hipLaunchKernelGGL(k_plm_protein_head, dim3(1), dim3(PLM_H3), 0, st, params + PLM_O_L4W, params + PLM_O_L4B, pooled, out256);
}

// ---------------------------------------------------------------------------------------------------------------- sgRNA front
// One block per guide, 256 threads: thread (o = tid & 63, pg = tid >> 6) owns output channel o at positions [15 pg, 15 pg + 15).
// Activations live in LDS as x[channel][2 + position] with two zero columns on either side (the convolutions' padding).
#define PLM_XS 65       // row stride of an activation plane: lanes of a wave differ in the channel, so an odd stride
#define PLM_PG 15       // positions per thread
__device__ const char k_plm_scaffold[PLM_SCAF + 1] = "GTTTCAGAGCTATGCTGGAAACAGCATAGCAAGTTG";

__device__ __forceinline__ void plm_conv64(const float* __restrict__ wt, const float* __restrict__ bias, const float* xin, float* xout,
                                           int o, int p0) {
  float acc[PLM_PG];
  const float b = bias[o];
#pragma unroll
  for (int j = 0; j < PLM_PG; ++j) acc[j] = b;
  for (int c = 0; c < PLM_CH; ++c) {
    float x[PLM_PG + PLM_KW - 1];
#pragma unroll
    for (int i = 0; i < PLM_PG + PLM_KW - 1; ++i) x[i] = xin[c * PLM_XS + p0 + i];  // p0 + i <= 45 + 18 < PLM_XS
#pragma unroll
    for (int t = 0; t < PLM_KW; ++t) {
      const float w = wt[(c * PLM_KW + t) * PLM_CH + o];
#pragma unroll
      for (int j = 0; j < PLM_PG; ++j) acc[j] = fmaf(w, x[j + t], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < PLM_PG; ++j)
    if (p0 + j < PLM_SEQ) xout[o * PLM_XS + 2 + p0 + j] = plm_sigmoid(acc[j]);
}

__global__ __launch_bounds__(256) void k_plm_front(const char* __restrict__ seqs, uint64_t n, const float* __restrict__ params,
                                                   const float* __restrict__ aux, float* __restrict__ feat, int* status) {
  __shared__ float xa[PLM_CH * PLM_XS], xb[PLM_CH * PLM_XS];
  __shared__ unsigned char code[64];
  __shared__ unsigned char hot[PLM_SYM * 64];  // hot[c][2 + p]: the conv input after the reshape quirk, zero-padded
  const uint64_t g = blockIdx.x;
  if (g >= n) return;
  const int tid = threadIdx.x;
  for (int i = tid; i < PLM_SYM * 64; i += 256) hot[i] = 0;
  for (int i = tid; i < PLM_CH * PLM_XS; i += 256) { xa[i] = 0.f; xb[i] = 0.f; }
  if (tid < PLM_SEQ) {
    char ch = tid < PLM_GUIDE ? seqs[g * PLM_GUIDE + tid] : k_plm_scaffold[tid - PLM_GUIDE];
    if (ch >= 'a' && ch <= 'z') ch -= 32;
    int cd = 4;
    switch (ch) {
      case 'A': cd = 0; break;
      case 'T': cd = 1; break;
      case 'C': cd = 2; break;
      case 'G': cd = 3; break;
      case 'N': cd = 4; break;
      default: atomicCAS(status, 0, HAWK_E_IUPAC); break;  // the reference's KeyError (plm_crispr.py:199); first writer wins
    }
    code[tid] = (unsigned char)cd;
  }
  __syncthreads();
  // one_hot(59, 5).view(5, 59): flat element f = 5 i + code[i] of the row-major one-hot is channel f / 59, position f % 59
  if (tid < PLM_SEQ) {
    const int f = tid * PLM_SYM + code[tid];
    hot[(f / PLM_SEQ) * 64 + 2 + f % PLM_SEQ] = 1;
  }
  __syncthreads();
  const int o = tid & 63, p0 = (tid >> 6) * PLM_PG;
  {  // conv1 (-> sigmoid -> xa) and conv4 (-> xb, no activation): the input is 0 / 1, so the weights are gathered, not multiplied
    float a1[PLM_PG], a4[PLM_PG];
    const float b1 = params[PLM_O_C1B + o], b4 = params[PLM_O_C4B + o];
#pragma unroll
    for (int j = 0; j < PLM_PG; ++j) { a1[j] = b1; a4[j] = b4; }
    for (int c = 0; c < PLM_SYM; ++c) {
#pragma unroll
      for (int t = 0; t < PLM_KW; ++t) {
        const float w1 = aux[PLM_X_C1 + (c * PLM_KW + t) * PLM_CH + o], w4 = aux[PLM_X_C4 + (c * PLM_KW + t) * PLM_CH + o];
#pragma unroll
        for (int j = 0; j < PLM_PG; ++j)
          if (hot[c * 64 + p0 + j + t]) { a1[j] += w1; a4[j] += w4; }  // p0 + j + t <= 45 + 14 + 4 < 64
      }
    }
#pragma unroll
    for (int j = 0; j < PLM_PG; ++j)
      if (p0 + j < PLM_SEQ) {
        xa[o * PLM_XS + 2 + p0 + j] = plm_sigmoid(a1[j]);
        xb[o * PLM_XS + 2 + p0 + j] = a4[j];
      }
  }
  __syncthreads();
  float* row = feat + g * PLM_FEAT;
  for (int i = tid; i < PLM_BR; i += 256) row[PLM_BR + i] = xb[(i / PLM_SEQ) * PLM_XS + 2 + i % PLM_SEQ];  // be, channel-major
  __syncthreads();
  plm_conv64(aux + PLM_X_C2, params + PLM_O_C2B, xa, xb, o, p0);
  __syncthreads();
  plm_conv64(aux + PLM_X_C3, params + PLM_O_C3B, xb, xa, o, p0);
  __syncthreads();
  for (int i = tid; i < PLM_BR; i += 256) row[i] = xa[(i / PLM_SEQ) * PLM_XS + 2 + i % PLM_SEQ];
}

void hawk_launch_plm_front(hipStream_t st, const char* seqs, uint64_t n, const float* params, const float* aux, float* feat, int* status) {
  hipLaunchKernelGGL(k_plm_front, dim3((uint32_t)n), dim3(256), 0, st, seqs, n, params, aux, feat, status);
}

// ---------------------------------------------------------------------------------------------------------------- lin1 / lin3
// out[m][j] = f(bias[j] + sum_k a[m][k] w[j][k]) on v_mfma_f32_32x32x2_f32.  Block tile 128 x 128, four waves, each a 2 x 2 grid of
// 32 x 32 tiles: four independent accumulators per wave cover the instruction's 64-cycle dependent latency.  Both operands are
// K-contiguous in memory; a stage stores them K-major in LDS ([k][row], stride 132) so that a lane's operand - A[row = lane & 31]
// [k = lane >> 5], B[k = lane >> 5][unit = lane & 31] - is one conflict-free word read.  The next stage's global loads are issued
// before the current stage's MFMAs.  An accumulator is a k-ordered fp32 fma chain; after PLM_FLUSH stages (128 products) it is added
// to the element's total and cleared, so no chain is longer than 128 and the totals add 59 (lin1) or 16 (lin3) partial sums.
// Rows at or past n are loaded as zeros and never stored; a row's sums never see another row.
typedef float plm_f32x16 __attribute__((ext_vector_type(16)));
#define PLM_LD (PLM_TM + 4)

template <bool SIGMOID>
__global__ __launch_bounds__(256, 2) void k_plm_lin1(const float* __restrict__ a, uint64_t n, uint32_t K, const float* __restrict__ w,
                                                  const float* __restrict__ bias, uint32_t N, float* __restrict__ out) {
  __shared__ float As[PLM_TK * PLM_LD], Ws[PLM_TK * PLM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const uint64_t m0 = (uint64_t)blockIdx.y * PLM_TM;
  const uint32_t n0 = blockIdx.x * PLM_TN;
  const int lr = tid >> 3, lq = (tid & 7) * 4;  // this thread stages rows lr + 32 i, k = lq .. lq + 3 of both tiles
  float4 ra[4], rw[4];
  auto fetch = [&](uint32_t k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t m = m0 + lr + 32 * i;
      ra[i] = m < n ? *reinterpret_cast<const float4*>(a + m * K + k0 + lq) : make_float4(0.f, 0.f, 0.f, 0.f);
      rw[i] = *reinterpret_cast<const float4*>(w + (size_t)(n0 + lr + 32 * i) * K + k0 + lq);
    }
  };
  plm_f32x16 acc[4], tot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; tot[i][r] = 0.f; }
  const uint32_t KT = K / PLM_TK;
  fetch(0);
  for (uint32_t kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = lr + 32 * i;
      As[(lq + 0) * PLM_LD + r] = ra[i].x; As[(lq + 1) * PLM_LD + r] = ra[i].y;
      As[(lq + 2) * PLM_LD + r] = ra[i].z; As[(lq + 3) * PLM_LD + r] = ra[i].w;
      Ws[(lq + 0) * PLM_LD + r] = rw[i].x; Ws[(lq + 1) * PLM_LD + r] = rw[i].y;
      Ws[(lq + 2) * PLM_LD + r] = rw[i].z; Ws[(lq + 3) * PLM_LD + r] = rw[i].w;
    }
    __syncthreads();
    if (kt + 1 < KT) fetch((kt + 1) * PLM_TK);
    const float* ap = As + (lane >> 5) * PLM_LD + wm * 64 + (lane & 31);
    const float* wp = Ws + (lane >> 5) * PLM_LD + wn * 64 + (lane & 31);
#pragma unroll
    for (int ks = 0; ks < PLM_TK / 2; ++ks) {
      const float a0 = ap[2 * ks * PLM_LD], a1 = ap[2 * ks * PLM_LD + 32];
      const float b0 = wp[2 * ks * PLM_LD], b1 = wp[2 * ks * PLM_LD + 32];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[3], 0, 0, 0);
    }
    if ((kt + 1) % PLM_FLUSH == 0 || kt + 1 == KT) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { tot[i][r] += acc[i][r]; acc[i][r] = 0.f; }
    }
    __syncthreads();
  }
  // C/D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t j = n0 + wn * 64 + (i & 1) * 32 + (lane & 31);
    const float bj = bias[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint64_t m = m0 + wm * 64 + (i >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (m < n) {
        const float v = tot[i][r] + bj;
        out[m * N + j] = SIGMOID ? plm_sigmoid(v) : v;
      }
    }
  }
}

void hawk_launch_plm_lin(hipStream_t st, const float* a, uint64_t n, uint32_t K, const float* w, const float* bias, uint32_t N,
                         bool sigmoid, float* out) {
  const dim3 grid(N / PLM_TN, (uint32_t)((n + PLM_TM - 1) / PLM_TM));
  if (sigmoid) hipLaunchKernelGGL(k_plm_lin1<true>, grid, dim3(256), 0, st, a, n, K, w, bias, N, out);
  else hipLaunchKernelGGL(k_plm_lin1<false>, grid, dim3(256), 0, st, a, n, K, w, bias, N, out);
}

// ---------------------------------------------------------------------------------------------------------------- head
// PLM_TAIL_G guides per block, one thread per hidden unit: a weight is read once per block and used for every guide of it.
__global__ __launch_bounds__(PLM_H5) void k_plm_tail(const float* __restrict__ sg, uint64_t n, const float* __restrict__ prot,
                                                     const float* __restrict__ params, const float* __restrict__ aux,
                                                     float* __restrict__ out) {
  __shared__ float v[PLM_TAIL_G][2 * PLM_H3];  // [out_sgrna | out_protein], then the mix in the first half
  __shared__ float h[PLM_TAIL_G][PLM_H5];
  __shared__ float lg[PLM_TAIL_G][2];
  const int u = threadIdx.x;
  const uint64_t g0 = (uint64_t)blockIdx.x * PLM_TAIL_G;
  for (int i = u; i < PLM_TAIL_G * PLM_H3; i += PLM_H5) {
    const int g = i / PLM_H3, k = i % PLM_H3;
    v[g][k] = g0 + g < n ? sg[(g0 + g) * PLM_H3 + k] : 0.f;
    v[g][PLM_H3 + k] = prot[k];
  }
  __syncthreads();
  float acc[PLM_TAIL_G];
  {
    const float b = params[PLM_O_W0B + u];
#pragma unroll
    for (int g = 0; g < PLM_TAIL_G; ++g) acc[g] = b;
    for (int k = 0; k < 2 * PLM_H3; ++k) {
      const float wv = aux[PLM_X_W0 + k * PLM_H5 + u];
#pragma unroll
      for (int g = 0; g < PLM_TAIL_G; ++g) acc[g] = fmaf(wv, v[g][k], acc[g]);
    }
#pragma unroll
    for (int g = 0; g < PLM_TAIL_G; ++g) h[g][u] = acc[g] > 0.f ? acc[g] : 0.f;
  }
  __syncthreads();
  if (u < 2 * PLM_TAIL_G) {
    const int g = u >> 1, j = u & 1;
    float l = params[PLM_O_W2B + j];
    for (int k = 0; k < PLM_H5; ++k) l = fmaf(params[PLM_O_W2W + j * PLM_H5 + k], h[g][k], l);
    lg[g][j] = l;
  }
  __syncthreads();
  float w0[PLM_TAIL_G], w1[PLM_TAIL_G];
#pragma unroll
  for (int g = 0; g < PLM_TAIL_G; ++g) {  // softmax over the two logits, as torch: exp(x - max) / sum
    const float m = fmaxf(lg[g][0], lg[g][1]);
    const float e0 = expf(lg[g][0] - m), e1 = expf(lg[g][1] - m);
    w0[g] = e0 / (e0 + e1);
    w1[g] = e1 / (e0 + e1);
  }
#pragma unroll
  for (int g = 0; g < PLM_TAIL_G; ++g)
    for (int k = u; k < PLM_H3; k += PLM_H5)  // the reference rounds both products, then adds
      v[g][k] = __fadd_rn(__fmul_rn(w0[g], v[g][k]), __fmul_rn(w1[g], v[g][PLM_H3 + k]));
  __syncthreads();
  {
    const float b = params[PLM_O_L5B + u];
#pragma unroll
    for (int g = 0; g < PLM_TAIL_G; ++g) acc[g] = b;
    for (int k = 0; k < PLM_H3; ++k) {
      const float wv = aux[PLM_X_L5 + k * PLM_H5 + u];
#pragma unroll
      for (int g = 0; g < PLM_TAIL_G; ++g) acc[g] = fmaf(wv, v[g][k], acc[g]);
    }
#pragma unroll
    for (int g = 0; g < PLM_TAIL_G; ++g) h[g][u] = plm_sigmoid(acc[g]);  // h was last read before the barrier behind lg
  }
  __syncthreads();
  if (u < PLM_TAIL_G && g0 + u < n) {
    float z = params[PLM_O_L6B];
    for (int k = 0; k < PLM_H5; ++k) z = fmaf(params[PLM_O_L6W + k], h[u][k], z);
    out[g0 + u] = plm_sigmoid(z);
  }
}

void hawk_launch_plm_tail(hipStream_t st, const float* sg, uint64_t n, const float* prot, const float* params, const float* aux,
                          float* out) {
  hipLaunchKernelGGL(k_plm_tail, dim3((uint32_t)((n + PLM_TAIL_G - 1) / PLM_TAIL_G)), dim3(PLM_H5), 0, st, sg, n, prot, params, aux, out);
}
