// hawk_plm.h - PLM-CRISPR (scores/plm_crispr/train_general.py, class sgrna_net): layer shapes, the offsets of every tensor in the
// packed parameter block of hawk_plm_create (torch state_dict order, fp32), and the launchers of hawk_plm.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#define PLM_GUIDE 23    // spacer + PAM
#define PLM_SCAF 36     // the fixed scaffold the wrapper appends (plm_crispr.py:29-32)
#define PLM_SEQ 59      // symbols per guide
#define PLM_SYM 5       // A T C G N
#define PLM_CH 64       // channels of conv1..conv4
#define PLM_KW 5        // their kernel width (padding 2)
#define PLM_BR (PLM_CH * PLM_SEQ)  // 3776: one branch, flattened [channel][position]
#define PLM_FEAT (2 * PLM_BR)      // 7552: [conv1-3 branch | conv4 branch]
#define PLM_H1 2048     // lin1
#define PLM_H3 256      // lin3 = out_sgrna; lin4 = out_protein
#define PLM_EMB 1280    // ESM embedding width
#define PLM_PC 128      // channels per text_cnn convolution
#define PLM_PFEAT 384   // 3 x PLM_PC
#define PLM_H5 128      // lin5, weight_net.0
#define PLM_MIN_L 13    // the widest text_cnn kernel: a shorter protein leaves it no position

// offsets (in floats) into the packed block; the order is sgrna_net().state_dict()
enum : size_t {
  PLM_O_C1W = 0,                                        // conv1.weight [64][5][5]
  PLM_O_C1B = PLM_O_C1W + PLM_CH * PLM_SYM * PLM_KW,    // conv1.bias [64]
  PLM_O_C2W = PLM_O_C1B + PLM_CH,                       // conv2.weight [64][64][5]
  PLM_O_C2B = PLM_O_C2W + PLM_CH * PLM_CH * PLM_KW,
  PLM_O_C3W = PLM_O_C2B + PLM_CH,                       // conv3.weight [64][64][5]
  PLM_O_C3B = PLM_O_C3W + PLM_CH * PLM_CH * PLM_KW,
  PLM_O_C4W = PLM_O_C3B + PLM_CH,                       // conv4.weight [64][5][5]
  PLM_O_C4B = PLM_O_C4W + PLM_CH * PLM_SYM * PLM_KW,
  PLM_O_T0W = PLM_O_C4B + PLM_CH,                       // text_cnn.convs.0.weight [128][1280][5]
  PLM_O_T0B = PLM_O_T0W + (size_t)PLM_PC * PLM_EMB * 5,
  PLM_O_T1W = PLM_O_T0B + PLM_PC,                       // text_cnn.convs.1.weight [128][1280][9]
  PLM_O_T1B = PLM_O_T1W + (size_t)PLM_PC * PLM_EMB * 9,
  PLM_O_T2W = PLM_O_T1B + PLM_PC,                       // text_cnn.convs.2.weight [128][1280][13]
  PLM_O_T2B = PLM_O_T2W + (size_t)PLM_PC * PLM_EMB * 13,
  PLM_O_L1W = PLM_O_T2B + PLM_PC,                       // lin1.weight [2048][7552]
  PLM_O_L1B = PLM_O_L1W + (size_t)PLM_H1 * PLM_FEAT,
  PLM_O_L3W = PLM_O_L1B + PLM_H1,                       // lin3.weight [256][2048]
  PLM_O_L3B = PLM_O_L3W + (size_t)PLM_H3 * PLM_H1,
  PLM_O_L4W = PLM_O_L3B + PLM_H3,                       // lin4.weight [256][384]
  PLM_O_L4B = PLM_O_L4W + (size_t)PLM_H3 * PLM_PFEAT,
  PLM_O_L5W = PLM_O_L4B + PLM_H3,                       // lin5.weight [128][256]
  PLM_O_L5B = PLM_O_L5W + (size_t)PLM_H5 * PLM_H3,
  PLM_O_L6W = PLM_O_L5B + PLM_H5,                       // lin6.weight [1][128]
  PLM_O_L6B = PLM_O_L6W + PLM_H5,                       // lin6.bias [1]
  PLM_O_W0W = PLM_O_L6B + 1,                            // weight_net.0.weight [128][512]
  PLM_O_W0B = PLM_O_W0W + (size_t)PLM_H5 * 2 * PLM_H3,
  PLM_O_W2W = PLM_O_W0B + PLM_H5,                       // weight_net.2.weight [2][128]
  PLM_O_W2B = PLM_O_W2W + 2 * PLM_H5,                   // weight_net.2.bias [2]
  PLM_NPARAMS = PLM_O_W2B + 2
};

// Copies of the small weights with the output unit innermost, made once by hawk_plm_create: a wave whose lanes are output units
// reads them coalesced.  Offsets in floats into hawk_plm::aux.
enum : size_t {
  PLM_X_C1 = 0,                                      // [5*5][64]   conv1.weight[o][c][t] at [(c*5+t)*64 + o]
  PLM_X_C4 = PLM_X_C1 + PLM_SYM * PLM_KW * PLM_CH,   // [5*5][64]
  PLM_X_C2 = PLM_X_C4 + PLM_SYM * PLM_KW * PLM_CH,   // [64*5][64]
  PLM_X_C3 = PLM_X_C2 + PLM_CH * PLM_KW * PLM_CH,    // [64*5][64]
  PLM_X_W0 = PLM_X_C3 + PLM_CH * PLM_KW * PLM_CH,    // [512][128]  weight_net.0.weight[u][k] at [k*128 + u]
  PLM_X_L5 = PLM_X_W0 + 2 * PLM_H3 * PLM_H5,         // [256][128]  lin5.weight[u][k] at [k*128 + u]
  PLM_NAUX = PLM_X_L5 + PLM_H3 * PLM_H5
};

// the GEMM's block tile: PLM_TM rows of the batch x PLM_TN output units, PLM_TK of K per LDS stage.  Every K and N it is used
// with (7552 / 2048 and 2048 / 256) is a multiple of PLM_TK x PLM_FLUSH and of PLM_TN.
#define PLM_TM 128
#define PLM_TN 128
#define PLM_TK 32
#define PLM_FLUSH 4      // LDS stages whose products one MFMA accumulator chains before it is added to the row's total
#define PLM_TAIL_G 8     // guides per block of k_plm_tail
#define PLM_PROT_P 16    // positions per block of k_plm_protein
#define PLM_DEFAULT_BATCH 8192u

void hawk_launch_plm_protein(hipStream_t st, const float* params, const float* emb, uint32_t L, uint32_t* pooled, float* out256);
void hawk_launch_plm_front(hipStream_t st, const char* seqs, uint64_t n, const float* params, const float* aux, float* feat, int* status);
void hawk_launch_plm_lin(hipStream_t st, const float* a, uint64_t n, uint32_t K, const float* w, const float* bias, uint32_t N,
                         bool sigmoid, float* out);
void hawk_launch_plm_tail(hipStream_t st, const float* sg, uint64_t n, const float* prot, const float* params, const float* aux,
                          float* out);
