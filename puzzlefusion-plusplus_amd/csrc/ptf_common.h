// What the eval unit (csrc/matching_tf.hip) and the training unit (csrc/matching_ptf_train.hip) of the matcher's point-transformer layer
// share: the sizes, the offsets into the two packed weight buffers, and the ONE recomputation of the 128-wide quantities (p_r, r and the
// normalised pre-activation) that the training forward and every backward pass call, so that a ReLU mask recomputed in the backward is
// the forward's mask bit for bit.  Both units are compiled without contraction; fused operations are written as fmaf.
#pragma once
#include "pfpp_common.h"

namespace {

constexpr int TF_C = 128;      // channels of the descriptors
constexpr int TF_K = 16;       // neighbours

// offsets into the eval-mode packed weights (floats; include/pfpp.h PFPP_PTF_WEIGHT_FLOATS)
constexpr int PW_P1W = 0;        // linear_p[0].weight [3][3]
constexpr int PW_P1S = 12;       // BatchNorm(3) folded behind it: scale [3]
constexpr int PW_P1T = 16;       //                                shift [3] (carries the bias of linear_p[0])
constexpr int PW_P2W = 20;       // linear_p[3].weight [128][3]
constexpr int PW_P2B = 404;      // linear_p[3].bias [128]
constexpr int PW_A1 = 532;       // linear_w[0] (BatchNorm(128)): scale [128]
constexpr int PW_C1 = 660;       //                               shift [128]
constexpr int PW_W3 = 788;       // linear_w[2].weight [16][128]
constexpr int PW_A2 = 2836;      // BatchNorm(16) folded behind it: scale [16]
constexpr int PW_C2 = 2852;      //                                 shift [16] (carries the bias of linear_w[2])
constexpr int PW_W4 = 2868;      // linear_w[5].weight [16][16]
constexpr int PW_B4 = 3124;      // linear_w[5].bias [16]
constexpr int PW_TOTAL = 3140;
static_assert(PW_TOTAL == PFPP_PTF_WEIGHT_FLOATS, "include/pfpp.h and the kernel disagree on the packed weights");

constexpr int AG_LDH = TF_C + 4;   // row stride of the relation tile: the four rows a wave reads at once start 4 banks apart

// offsets into the training pack (floats; include/pfpp.h PFPP_PTF_TRAIN_FLOATS): the raw linear weights, and per BatchNorm the vectors
// the finalise kernel derives from the batch sums: scale = gamma rstd, shift = beta - mean scale (z = fmaf(x, scale, shift)),
// rstd, nmr = -mean rstd (x hat = fmaf(x, rstd, nmr)); behind them the means of dz and dz x hat of the backward
constexpr int TW_W0 = 0;         // linear_p[0].weight [3][3]
constexpr int TW_B0 = 12;        // linear_p[0].bias [3]
constexpr int TW_S0 = 16;        // BatchNorm(3): scale, shift, rstd, nmr [3] each, 4 floats apart
constexpr int TW_T0 = 20;
constexpr int TW_R0 = 24;
constexpr int TW_N0 = 28;
constexpr int TW_W3 = 36;        // linear_p[3].weight [128][3]
constexpr int TW_B3 = 420;       // linear_p[3].bias [128]
constexpr int TW_S1 = 548;       // BatchNorm(128): scale, shift, rstd, nmr [128] each
constexpr int TW_T1 = 676;
constexpr int TW_R1 = 804;
constexpr int TW_N1 = 932;
constexpr int TW_W2 = 1060;      // linear_w[2].weight [16][128]
constexpr int TW_B2 = 3108;      // linear_w[2].bias [16]
constexpr int TW_S2 = 3124;      // BatchNorm(16): scale, shift, rstd, nmr [16] each
constexpr int TW_T2 = 3140;
constexpr int TW_R2 = 3156;
constexpr int TW_N2 = 3172;
constexpr int TW_W5 = 3188;      // linear_w[5].weight [16][16]
constexpr int TW_B5 = 3444;      // linear_w[5].bias [16]
constexpr int TW_M2 = 3460;      // backward of BatchNorm(16): mean of dz [16] | mean of dz x hat [16]
constexpr int TW_M1 = 3492;      // backward of BatchNorm(128): mean of dz [128] | mean of dz x hat [128]
constexpr int TW_TOTAL = 3748;
static_assert(TW_TOTAL == PFPP_PTF_TRAIN_FLOATS, "include/pfpp.h and the kernels disagree on the training pack");
static_assert(TW_W3 % 4 == 0 && TW_W2 % 4 == 0 && TW_W5 % 4 == 0, "the matrices of the training pack start 16-byte aligned");

// what a thread that owns channel c keeps of the training pack for every point it sees
struct PtfChan {
  float w0[9], b0[3], s0[3], t0[3];    // linear_p[0] and the BatchNorm(3) behind it
  float p2x, p2y, p2z, p2b;            // row c of linear_p[3]
  float s1, t1;                        // BatchNorm(128), channel c
};

__device__ __forceinline__ PtfChan ptf_chan_load(const float* __restrict__ tw, int c) {
  PtfChan w;
#pragma unroll
  for (int i = 0; i < 9; ++i) w.w0[i] = tw[TW_W0 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { w.b0[i] = tw[TW_B0 + i]; w.s0[i] = tw[TW_S0 + i]; w.t0[i] = tw[TW_T0 + i]; }
  w.p2x = tw[TW_W3 + 3 * c]; w.p2y = tw[TW_W3 + 3 * c + 1]; w.p2z = tw[TW_W3 + 3 * c + 2]; w.p2b = tw[TW_B3 + c];
  w.s1 = tw[TW_S1 + c]; w.t1 = tw[TW_T1 + c];
  return w;
}

// one (point, slot, channel) of the relation tile
struct PtfRel {
  float d[3];      // masked offset g_p (0 for a padded slot)
  float a[3];      // linear_p[0] of it, bias included: the input of BatchNorm(3)
  float z0[3];     // fmaf(a, scale, shift): what the first ReLU thresholds
  float pr;        // p_r, channel c
  float r;         // x_k[ik] - x_q + p_r, channel c: the input of BatchNorm(128)
  float z1;        // fmaf(r, scale, shift): what the second ReLU thresholds
};

// linear_p[0] (bias included) of the masked offset of slot ik of a point at (px, py, pz); an index outside [0, N) is the zero row
__device__ __forceinline__ void ptf_offset(const float* __restrict__ xyz, int64_t N, int ik, float px, float py, float pz,
                                           const float* w0, const float* b0, float d[3], float a[3]) {
  const bool ok = (unsigned)ik < (unsigned)N;
  const int64_t rk = ok ? ik : 0;
  d[0] = ok ? xyz[3 * rk] - px : 0.0f;
  d[1] = ok ? xyz[3 * rk + 1] - py : 0.0f;
  d[2] = ok ? xyz[3 * rk + 2] - pz : 0.0f;
#pragma unroll
  for (int m = 0; m < 3; ++m) a[m] = fmaf(w0[3 * m + 2], d[2], fmaf(w0[3 * m + 1], d[1], w0[3 * m] * d[0])) + b0[m];
}

// THE recomputation: kk = x_k[ik][c] (0 for a padded slot), q = x_q[n][c].  Before the statistics of a BatchNorm exist its scale and
// shift in w are whatever the pack holds and the fields behind it are not used.
__device__ __forceinline__ PtfRel ptf_relation(const PtfChan& w, const float* __restrict__ xyz, int64_t N, int ik, float px, float py,
                                               float pz, float kk, float q) {
  PtfRel o;
  ptf_offset(xyz, N, ik, px, py, pz, w.w0, w.b0, o.d, o.a);
#pragma unroll
  for (int m = 0; m < 3; ++m) o.z0[m] = fmaf(o.a[m], w.s0[m], w.t0[m]);
  const float g0 = fmaxf(o.z0[0], 0.0f), g1 = fmaxf(o.z0[1], 0.0f), g2 = fmaxf(o.z0[2], 0.0f);
  o.pr = fmaf(w.p2z, g2, fmaf(w.p2y, g1, fmaf(w.p2x, g0, w.p2b)));
  o.r = (kk - q) + o.pr;
  o.z1 = fmaf(o.r, w.s1, w.t1);
  return o;
}

// dh1[c] = sum_j du[j] W2[j][c] in j order (w2c = column c of linear_w[2]); du: 16 floats, 16-byte aligned (LDS or global)
__device__ __forceinline__ float ptf_dh1(const float* du, const float* w2c) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < TF_K / 4; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(du + 4 * i);
    s = fmaf(v.x, w2c[4 * i], s); s = fmaf(v.y, w2c[4 * i + 1], s); s = fmaf(v.z, w2c[4 * i + 2], s); s = fmaf(v.w, w2c[4 * i + 3], s);
  }
  return s;
}

// dr[c] from dh1: ReLU mask of the recomputed z1, then the train-mode BatchNorm backward with the global means m1 = mean(dz), m2 = mean(dz x hat)
__device__ __forceinline__ float ptf_dr(float dh1, float z1, float r, float s1, float r1, float n1, float m1, float m2) {
  const float dz = z1 > 0.0f ? dh1 : 0.0f;
  const float xh = fmaf(r, r1, n1);
  return s1 * ((dz - m1) - xh * m2);
}

}  // namespace
