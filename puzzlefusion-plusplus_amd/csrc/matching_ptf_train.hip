// Training of the matcher's point-transformer layer tf_self1 (Jigsaw_matching/model/jigsaw/attention_layer.py:159-225 in .train() under
// autograd) behind the projection GEMM and the two neighbour searches: the forward with BATCH statistics in its three BatchNorms
// (LayerNorm1d = BatchNorm1d over the channels of [N, 16, C]: the batch is all 16 N rows of the call, padded slots included), and the
// backward down to dq | dk | dv.  Nothing with N 16 128 elements is written: per point the passes keep u, w and du ([16, 16] each) and
// recompute everything 128 wide from q | k | v, xyz, the lists and the statistics with ptf_relation (csrc/ptf_common.h).
//
// Forward (a workgroup of 256 threads walks points; thread roles as in ptf_aggregate_kernel: (channel c, half hf) for the tile, (slot t,
// output j) for the 16 x 16 quantities):
//  * ptf_bn3_stats_kernel   — sums of a = linear_p[0](g_p) and a^2 over all (point, slot) rows.
//  * ptf_bn128_stats_kernel — sums of r = x_k[ik] - x_q + p_r and r^2 per channel.
//  * ptf_tile_kernel        — h1 = relu(bn(r)) in LDS, u = W2 h1 + b2 with the weight row in registers, u stored, sums of u and u^2.
//  * ptf_finish_kernel      — h2 = relu(bn(u)), the logits, the softmax over the 16 slots (w stored), out = sum_t (x_v[iv] + p_r) w.
// Backward:
//  * ptf_bwd_w_kernel       — dw = dout (x_v + p_r) summed over the 8 groups, softmax backward, dW5, db5, dz2 (stored), sums of dz2, dz2 x hat.
//  * ptf_bwd_u_kernel       — du from dz2 (in place), dW2 against the recomputed h1, sums of dz1, dz1 x hat per channel.
//  * ptf_bwd_r_kernel       — dr, dp_r = dout w + dr, dx_q = -sum_t dr, dW3, db3, dh0 and the 27 moments that make dgamma0, dbeta0, dW0 closed forms.
//  * ptf_bwd_gather_kernel  — dx_k[m] and dx_v[m] summed over the inverse lists of m in (point, slot) order, dr recomputed per element.
// Every per-channel sum is accumulated in fp64 per thread, leaves the workgroup as one fp64 partial and is folded by ptf_fold_kernel
// in a fixed order (8 slices of the workgroups per output, then the slices in order) on ceil(outputs / 32) workgroups.  No atomics:
// two runs agree bitwise.  ptf_bn_finalise_kernel turns the sums of a BatchNorm into scale / shift / rstd / -mean rstd in the training
// pack and updates the running buffers.  A launch that thresholds a pre-activation stores it to pre_dump when that is non-null (tests).
// This unit is compiled without contraction; fused operations are written as fmaf.
#include "pfpp_common.h"
#include "ptf_common.h"

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_WG = PFPP_PTF_TRAIN_MAX_WG;

// number of fp64 partials a workgroup of each pass leaves
constexpr int NP_BN3 = 6;                                    // sum a [3] | sum a^2 [3]
constexpr int NP_BN128 = 2 * TF_C;                           // sum r [128] | sum r^2 [128]
constexpr int NP_TILE = 2 * TF_K;                            // sum u [16] | sum u^2 [16]
constexpr int NP_BWD_W = TF_K * TF_K + 3 * TF_K;             // dW5 [16][16] | db5 [16] | sum dz2 [16] | sum dz2 x hat [16]
constexpr int NP_BWD_U = TF_K * TF_C + 2 * TF_C;             // dW2 [16][128] | sum dz1 [128] | sum dz1 x hat [128]
constexpr int NP_BWD_R = 3 * TF_C + TF_C + 27;               // dW3 [128][3] | db3 [128] | 27 moments of the BatchNorm(3) backward
static_assert(NP_BWD_W == PFPP_PTF_TRAIN_BWD_W_SUMS && NP_BWD_U == PFPP_PTF_TRAIN_BWD_U_SUMS && NP_BWD_R == PFPP_PTF_TRAIN_BWD_R_SUMS,
              "include/pfpp.h and the kernels disagree on the sums");
static_assert(NP_BWD_U <= PFPP_PTF_TRAIN_WS_DOUBLES / PFPP_PTF_TRAIN_MAX_WG, "the workspace holds the widest partial row of every workgroup");

__device__ __forceinline__ double wave_sum(double v) {       // butterfly: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ the fold
// part [G][K] fp64 -> out [K]: 32 outputs x 8 slices per workgroup; slice s adds the workgroups g = s, s + 8, ... in that order, slice 0
// adds the eight slices in slice order.  The outputs [mean_lo, mean_lo + mean_n) also go to mean_out as (float)(sum inv_rows).
constexpr int FO_OUT = 32, FO_SLICES = 8;

__global__ __launch_bounds__(FO_OUT * FO_SLICES) void ptf_fold_kernel(const double* __restrict__ part, int G, int K, double* __restrict__ out,
                                                                     int mean_lo, int mean_n, double inv_rows, float* __restrict__ mean_out) {
  __shared__ double s_sum[FO_SLICES][FO_OUT];
  const int o = threadIdx.x & (FO_OUT - 1), slice = threadIdx.x >> 5;
  const int k = blockIdx.x * FO_OUT + o;
  double acc = 0.0;
  if (k < K)
    for (int g = slice; g < G; g += FO_SLICES) acc += part[(int64_t)g * K + k];
  s_sum[slice][o] = acc;
  __syncthreads();
  if (slice == 0 && k < K) {
    double a = s_sum[0][o];
#pragma unroll
    for (int i = 1; i < FO_SLICES; ++i) a += s_sum[i][o];
    out[k] = a;
    if (mean_out && k >= mean_lo && k < mean_lo + mean_n) mean_out[k - mean_lo] = (float)(a * inv_rows);
  }
}

void fold(hipStream_t st, const double* part, int64_t G, int K, double* out, int mean_lo = 0, int mean_n = 0, double inv_rows = 0.0,
          float* mean_out = nullptr) {
  hipLaunchKernelGGL(ptf_fold_kernel, dim3((unsigned)((K + FO_OUT - 1) / FO_OUT)), dim3(FO_OUT * FO_SLICES), 0, st, part, (int)G, K, out, mean_lo,
                     mean_n, inv_rows, mean_out);
}

// ------------------------------------------------------------------------------------------------ BatchNorm: sums -> pack, running buffers
// sums [2 C] = sum x | sum x^2 over `rows` rows.  Biased variance for the normalisation, unbiased for the running buffer.
__global__ __launch_bounds__(128) void ptf_bn_finalise_kernel(const double* __restrict__ sums, int C, double rows, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, double eps, double momentum,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ rstd,
                                                              float* __restrict__ nmr) {
  const int c = threadIdx.x;
  if (c >= C) return;
  const double mean = sums[c] / rows;
  double var = sums[C + c] / rows - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const double rs = 1.0 / sqrt(var + eps);
  const double sc = (double)gamma[c] * rs;
  scale[c] = (float)sc;
  shift[c] = (float)((double)beta[c] - mean * sc);
  rstd[c] = (float)rs;
  nmr[c] = (float)(-mean * rs);
  running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
  running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * rows / (rows - 1.0)));
}

// ------------------------------------------------------------------------------------------------ forward 1: sums of BatchNorm(3)
__global__ __launch_bounds__(PT_THREADS) void ptf_bn3_stats_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                                  const float* __restrict__ tw, int64_t N, double* __restrict__ part) {
  __shared__ double s_red[4][NP_BN3];
  float w0[9], b0[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) w0[i] = tw[TW_W0 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) b0[i] = tw[TW_B0 + i];
  double acc[NP_BN3] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < N * TF_K; e += (int64_t)gridDim.x * PT_THREADS) {
    const int64_t n = e >> 4;
    float d[3], a[3];
    ptf_offset(xyz, N, idx_k[e], xyz[3 * n], xyz[3 * n + 1], xyz[3 * n + 2], w0, b0, d, a);
#pragma unroll
    for (int m = 0; m < 3; ++m) { acc[m] += (double)a[m]; acc[3 + m] += (double)a[m] * (double)a[m]; }
  }
#pragma unroll
  for (int k = 0; k < NP_BN3; ++k) {
    const double v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NP_BN3) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * NP_BN3 + k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
  }
}

// ------------------------------------------------------------------------------------------------ forward 2: sums of BatchNorm(128)
__global__ __launch_bounds__(PT_THREADS) void ptf_bn128_stats_kernel(const float* __restrict__ xq, const float* __restrict__ xk, int64_t ld,
                                                                    const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                                    const float* __restrict__ tw, int64_t N, double* __restrict__ part,
                                                                    float* __restrict__ pre_dump) {
  __shared__ double s_red[2][TF_C];
  const int tid = threadIdx.x, c = tid & (TF_C - 1), hf = tid >> 7;
  const PtfChan w = ptf_chan_load(tw, c);
  double sum = 0.0, sq = 0.0;
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float q = xq[pt * ld + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int ik = idx_k[pt * TF_K + tt];
      const bool ok = (unsigned)ik < (unsigned)N;
      const float kk = ok ? xk[(int64_t)(ok ? ik : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, ik, px, py, pz, kk, q);
      sum += (double)o.r;
      sq += (double)o.r * (double)o.r;
      if (pre_dump && c < 3) pre_dump[(pt * TF_K + tt) * 3 + c] = c == 0 ? o.z0[0] : c == 1 ? o.z0[1] : o.z0[2];
    }
  }
  // the two halves of a channel in half order
  s_red[hf][c] = sum;
  __syncthreads();
  if (hf == 0) part[(int64_t)blockIdx.x * NP_BN128 + c] = s_red[0][c] + s_red[1][c];
  __syncthreads();
  s_red[hf][c] = sq;
  __syncthreads();
  if (hf == 0) part[(int64_t)blockIdx.x * NP_BN128 + TF_C + c] = s_red[0][c] + s_red[1][c];
}

// ------------------------------------------------------------------------------------------------ forward 3: the tile pass
__global__ __launch_bounds__(PT_THREADS) void ptf_tile_kernel(const float* __restrict__ xq, const float* __restrict__ xk, int64_t ld,
                                                             const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                             const float* __restrict__ tw, int64_t N, float* __restrict__ u_out,
                                                             double* __restrict__ part, float* __restrict__ pre_dump) {
  __shared__ __attribute__((aligned(16))) float s_h[TF_K][AG_LDH];       // relu(bn(r)) of the point's 16 neighbours
  __shared__ double s_red[2][TF_K][TF_K];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;
  const int t = tid >> 4, j = tid & 15;
  float w2[TF_C];                                            // row j of linear_w[2]
#pragma unroll
  for (int i = 0; i < TF_C / 4; ++i) {
    const float4 v = reinterpret_cast<const float4*>(tw + TW_W2 + j * TF_C)[i];
    w2[4 * i] = v.x; w2[4 * i + 1] = v.y; w2[4 * i + 2] = v.z; w2[4 * i + 3] = v.w;
  }
  const float b2 = tw[TW_B2 + j];
  const PtfChan w = ptf_chan_load(tw, c);
  double sum = 0.0, sq = 0.0;
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float q = xq[pt * ld + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int ik = idx_k[pt * TF_K + tt];
      const bool ok = (unsigned)ik < (unsigned)N;
      const float kk = ok ? xk[(int64_t)(ok ? ik : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, ik, px, py, pz, kk, q);
      s_h[tt][c] = fmaxf(o.z1, 0.0f);
      if (pre_dump) pre_dump[(pt * TF_K + tt) * TF_C + c] = o.z1;
    }
    __syncthreads();
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;        // thread (t, j), four partial sums as in the eval kernel
#pragma unroll
    for (int i = 0; i < TF_C; i += 4) {
      const float4 h = *reinterpret_cast<const float4*>(&s_h[t][i]);
      s0 = fmaf(h.x, w2[i], s0); s1 = fmaf(h.y, w2[i + 1], s1); s2 = fmaf(h.z, w2[i + 2], s2); s3 = fmaf(h.w, w2[i + 3], s3);
    }
    const float uu = ((s0 + s1) + (s2 + s3)) + b2;
    u_out[pt * (TF_K * TF_K) + tid] = uu;
    sum += (double)uu;
    sq += (double)uu * (double)uu;
    __syncthreads();                                         // the tile has been read
  }
  s_red[0][t][j] = sum;
  s_red[1][t][j] = sq;
  __syncthreads();
  if (tid < 2 * TF_K) {                                      // the 16 slots of an output in slot order
    const int which = tid >> 4, jj = tid & 15;
    double a = s_red[which][0][jj];
#pragma unroll
    for (int i = 1; i < TF_K; ++i) a += s_red[which][i][jj];
    part[(int64_t)blockIdx.x * NP_TILE + tid] = a;
  }
}

// ------------------------------------------------------------------------------------------------ forward 4: the finish pass
__global__ __launch_bounds__(PT_THREADS) void ptf_finish_kernel(const float* __restrict__ xv, int64_t ld, const float* __restrict__ xyz,
                                                               const int32_t* __restrict__ idx_k, const int32_t* __restrict__ idx_v,
                                                               const float* __restrict__ tw, int64_t N, const float* __restrict__ u_in,
                                                               float* __restrict__ w_out, float* __restrict__ out, float* __restrict__ pre_dump) {
  __shared__ float s_u[TF_K][TF_K + 1];                      // relu(bn(u))
  __shared__ float s_w[TF_K][TF_K + 1];                      // logits, then exp(logit - max)
  __shared__ float s_p[TF_K][TF_K + 1];                      // the softmax weights
  __shared__ float s_part[2][TF_C];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;
  const int t = tid >> 4, j = tid & 15;
  float w5[TF_K];
#pragma unroll
  for (int i = 0; i < TF_K; ++i) w5[i] = tw[TW_W5 + j * TF_K + i];
  const float s2 = tw[TW_S2 + j], t2 = tw[TW_T2 + j], b5 = tw[TW_B5 + j];
  const PtfChan w = ptf_chan_load(tw, c);
  const int jc = c & (TF_K - 1);
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float z2 = fmaf(u_in[pt * (TF_K * TF_K) + tid], s2, t2);
    if (pre_dump) pre_dump[pt * (TF_K * TF_K) + tid] = z2;
    s_u[t][j] = fmaxf(z2, 0.0f);
    // the gather role meanwhile: p_r and x_v of this thread's channel and 8 slots
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    float val[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int iv = idx_v[pt * TF_K + tt];
      const bool ok_v = (unsigned)iv < (unsigned)N;
      const float vv = ok_v ? xv[(int64_t)(ok_v ? iv : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, idx_k[pt * TF_K + tt], px, py, pz, 0.0f, 0.0f);
      val[u] = vv + o.pr;
    }
    __syncthreads();
    float lg = b5;
#pragma unroll
    for (int i = 0; i < TF_K; ++i) lg = fmaf(s_u[t][i], w5[i], lg);
    s_w[t][j] = lg;
    __syncthreads();
    float mx = s_w[0][j];                                    // softmax over the neighbours (dim 1) per channel j
#pragma unroll
    for (int i = 1; i < TF_K; ++i) mx = fmaxf(mx, s_w[i][j]);
    __syncthreads();
    const float ex = expf(lg - mx);
    s_w[t][j] = ex;
    __syncthreads();
    float den = 0.0f;
#pragma unroll
    for (int i = 0; i < TF_K; ++i) den += s_w[i][j];
    const float wv = ex / den;
    w_out[pt * (TF_K * TF_K) + tid] = wv;
    s_p[t][j] = wv;
    __syncthreads();
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(val[u], s_p[hf * 8 + u][jc], acc);
    s_part[hf][c] = acc;
    __syncthreads();
    if (hf == 0) out[pt * TF_C + c] = s_part[0][c] + s_part[1][c];
  }
}

// ------------------------------------------------------------------------------------------------ backward 1: softmax and linear_w[5]
__global__ __launch_bounds__(PT_THREADS) void ptf_bwd_w_kernel(const float* __restrict__ dout, const float* __restrict__ w_in,
                                                              const float* __restrict__ u_in, const float* __restrict__ xv, int64_t ld,
                                                              const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                              const int32_t* __restrict__ idx_v, const float* __restrict__ tw, int64_t N,
                                                              float* __restrict__ dz2_out, double* __restrict__ part,
                                                              float* __restrict__ pre_dump) {
  __shared__ __attribute__((aligned(16))) float s_t[TF_K][AG_LDH];       // dout (x_v + p_r) per (slot, channel)
  __shared__ float s_a[TF_K][TF_K + 1];                      // w dw
  __shared__ float s_dlg[TF_K][TF_K + 1];
  __shared__ float s_h2[TF_K][TF_K + 1];
  __shared__ double s_red[2][TF_K][TF_K];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;
  const int t = tid >> 4, j = tid & 15;
  float w5c[TF_K];                                           // column j of linear_w[5]
#pragma unroll
  for (int i = 0; i < TF_K; ++i) w5c[i] = tw[TW_W5 + i * TF_K + j];
  const float s2 = tw[TW_S2 + j], t2 = tw[TW_T2 + j], r2 = tw[TW_R2 + j], n2 = tw[TW_N2 + j];
  const PtfChan w = ptf_chan_load(tw, c);
  double dw5 = 0.0, db5 = 0.0, sum1 = 0.0, sum2 = 0.0;       // dW5[t][j] (the thread's pair read as (output, input)), db5[t] in the threads j = 0
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float g = dout[pt * TF_C + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int iv = idx_v[pt * TF_K + tt];
      const bool ok_v = (unsigned)iv < (unsigned)N;
      const float vv = ok_v ? xv[(int64_t)(ok_v ? iv : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, idx_k[pt * TF_K + tt], px, py, pz, 0.0f, 0.0f);
      s_t[tt][c] = g * (vv + o.pr);
    }
    const float wv = w_in[pt * (TF_K * TF_K) + tid], uu = u_in[pt * (TF_K * TF_K) + tid];
    const float z2 = fmaf(uu, s2, t2), xh = fmaf(uu, r2, n2);
    if (pre_dump) pre_dump[pt * (TF_K * TF_K) + tid] = z2;
    __syncthreads();
    float dw = s_t[t][j];                                    // the 8 groups of channel j in group order
#pragma unroll
    for (int s = 1; s < TF_C / TF_K; ++s) dw += s_t[t][s * TF_K + j];
    s_a[t][j] = wv * dw;
    __syncthreads();
    float dot = s_a[0][j];
#pragma unroll
    for (int i = 1; i < TF_K; ++i) dot += s_a[i][j];
    const float dlg = wv * (dw - dot);
    s_dlg[t][j] = dlg;
    s_h2[t][j] = fmaxf(z2, 0.0f);
    __syncthreads();
    float dh2 = 0.0f;
#pragma unroll
    for (int i = 0; i < TF_K; ++i) dh2 = fmaf(s_dlg[t][i], w5c[i], dh2);
    const float dz2 = z2 > 0.0f ? dh2 : 0.0f;
    dz2_out[pt * (TF_K * TF_K) + tid] = dz2;
    sum1 += (double)dz2;
    sum2 += (double)dz2 * (double)xh;
    // dW5[a][b] with (a, b) = (t, j): over the slots in order
#pragma unroll
    for (int i = 0; i < TF_K; ++i) dw5 = fma((double)s_dlg[i][t], (double)s_h2[i][j], dw5);
    if (j == 0) {
#pragma unroll
      for (int i = 0; i < TF_K; ++i) db5 += (double)s_dlg[i][t];
    }
    __syncthreads();                                         // the tiles have been read
  }
  double* p = part + (int64_t)blockIdx.x * NP_BWD_W;
  p[tid] = dw5;
  if (j == 0) p[TF_K * TF_K + t] = db5;
  s_red[0][t][j] = sum1;
  s_red[1][t][j] = sum2;
  __syncthreads();
  if (tid < 2 * TF_K) {
    const int which = tid >> 4, jj = tid & 15;
    double a = s_red[which][0][jj];
#pragma unroll
    for (int i = 1; i < TF_K; ++i) a += s_red[which][i][jj];
    p[TF_K * TF_K + TF_K + tid] = a;
  }
}

// ------------------------------------------------------------------------------------------------ backward 2: BatchNorm(16) and linear_w[2]
__global__ __launch_bounds__(PT_THREADS) void ptf_bwd_u_kernel(const float* __restrict__ xq, const float* __restrict__ xk, int64_t ld,
                                                              const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                              const float* __restrict__ tw, int64_t N, const float* __restrict__ u_in,
                                                              float* __restrict__ du, double* __restrict__ part, float* __restrict__ pre_dump) {
  __shared__ __attribute__((aligned(16))) float s_h[TF_K][AG_LDH];
  __shared__ __attribute__((aligned(16))) float s_du[TF_K][TF_K];
  __shared__ double s_red[2][TF_C];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;
  const int t = tid >> 4, j = tid & 15;
  const float s2 = tw[TW_S2 + j], r2 = tw[TW_R2 + j], n2 = tw[TW_N2 + j], m1 = tw[TW_M2 + j], m2 = tw[TW_M2 + TF_K + j];
  float w2c[TF_K];                                           // column c of linear_w[2]
#pragma unroll
  for (int i = 0; i < TF_K; ++i) w2c[i] = tw[TW_W2 + i * TF_C + c];
  const float r1 = tw[TW_R1 + c], n1 = tw[TW_N1 + c];
  const PtfChan w = ptf_chan_load(tw, c);
  double dw2[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // dW2[8 hf + i][c]
  double sum1 = 0.0, sum2 = 0.0;
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    {                                                        // du of (t, j) from dz2, in place
      const int64_t e = pt * (TF_K * TF_K) + tid;
      const float xh = fmaf(u_in[e], r2, n2);
      const float d = s2 * ((du[e] - m1) - xh * m2);
      du[e] = d;
      s_du[t][j] = d;
    }
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float q = xq[pt * ld + c];
    float z1[8], rr[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int ik = idx_k[pt * TF_K + tt];
      const bool ok = (unsigned)ik < (unsigned)N;
      const float kk = ok ? xk[(int64_t)(ok ? ik : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, ik, px, py, pz, kk, q);
      z1[u] = o.z1;
      rr[u] = o.r;
      s_h[tt][c] = fmaxf(o.z1, 0.0f);
      if (pre_dump) pre_dump[(pt * TF_K + tt) * TF_C + c] = o.z1;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float dh1 = ptf_dh1(&s_du[hf * 8 + u][0], w2c);
      const float dz = z1[u] > 0.0f ? dh1 : 0.0f;
      sum1 += (double)dz;
      sum2 += (double)dz * (double)fmaf(rr[u], r1, n1);
    }
#pragma unroll 4
    for (int i = 0; i < TF_K; ++i) {
      const double h = (double)s_h[i][c];
#pragma unroll
      for (int k = 0; k < 8; ++k) dw2[k] = fma((double)s_du[i][hf * 8 + k], h, dw2[k]);
    }
    __syncthreads();                                         // the tiles have been read
  }
  double* p = part + (int64_t)blockIdx.x * NP_BWD_U;
#pragma unroll
  for (int k = 0; k < 8; ++k) p[(hf * 8 + k) * TF_C + c] = dw2[k];
  s_red[hf][c] = sum1;
  __syncthreads();
  if (hf == 0) p[TF_K * TF_C + c] = s_red[0][c] + s_red[1][c];
  __syncthreads();
  s_red[hf][c] = sum2;
  __syncthreads();
  if (hf == 0) p[TF_K * TF_C + TF_C + c] = s_red[0][c] + s_red[1][c];
}

// ------------------------------------------------------------------------------------------------ backward 3: BatchNorm(128), linear_p
// moments (fp64, over all (point, slot) rows), m and l in 0 .. 2: [0, 3) sum dz0_m; [3, 6) sum dz0_m xh0_m; [6, 15) sum dz0_m d_l;
// [15, 24) sum xh0_m d_l; [24, 27) sum d_l
__global__ __launch_bounds__(PT_THREADS) void ptf_bwd_r_kernel(const float* __restrict__ dout, const float* __restrict__ w_in,
                                                              const float* __restrict__ du, const float* __restrict__ xq,
                                                              const float* __restrict__ xk, int64_t ld, const float* __restrict__ xyz,
                                                              const int32_t* __restrict__ idx_k, const float* __restrict__ tw, int64_t N,
                                                              float* __restrict__ dqkv, int64_t ldg, double* __restrict__ part,
                                                              float* __restrict__ pre_dump) {
  __shared__ __attribute__((aligned(16))) float s_dp[TF_K][AG_LDH];      // dp_r per (slot, channel)
  __shared__ float s_w3[3][TF_C];                            // linear_p[3].weight, input-major
  __shared__ float s_z0[TF_K][3], s_x0[TF_K][3], s_d[TF_K][3], s_dz0[TF_K][3];
  __shared__ float s_part[2][TF_C];
  __shared__ double s_red[2][TF_C];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;
  const int jc = c & (TF_K - 1);
  float w2c[TF_K];
#pragma unroll
  for (int i = 0; i < TF_K; ++i) w2c[i] = tw[TW_W2 + i * TF_C + c];
  const float r1 = tw[TW_R1 + c], n1 = tw[TW_N1 + c], m1 = tw[TW_M1 + c], m2 = tw[TW_M1 + TF_C + c];
  const PtfChan w = ptf_chan_load(tw, c);
  float r0[3], n0[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) { r0[m] = tw[TW_R0 + m]; n0[m] = tw[TW_N0 + m]; }
  if (hf == 0) { s_w3[0][c] = w.p2x; s_w3[1][c] = w.p2y; s_w3[2][c] = w.p2z; }
  double dw3[3] = {0.0, 0.0, 0.0}, db3 = 0.0, mom = 0.0;
  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float q = xq[pt * ld + c];
    const float g = dout[pt * TF_C + c];
    float sdr = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int ik = idx_k[pt * TF_K + tt];
      const bool ok = (unsigned)ik < (unsigned)N;
      const float kk = ok ? xk[(int64_t)(ok ? ik : 0) * ld + c] : 0.0f;
      const PtfRel o = ptf_relation(w, xyz, N, ik, px, py, pz, kk, q);
      const float dh1 = ptf_dh1(du + (pt * TF_K + tt) * TF_K, w2c);
      const float dr = ptf_dr(dh1, o.z1, o.r, w.s1, r1, n1, m1, m2);
      const float dp = g * w_in[(pt * TF_K + tt) * TF_K + jc] + dr;
      sdr += dr;
      s_dp[tt][c] = dp;
      db3 += (double)dp;
#pragma unroll
      for (int m = 0; m < 3; ++m) dw3[m] = fma((double)dp, (double)fmaxf(o.z0[m], 0.0f), dw3[m]);
      if (c == 0) {
#pragma unroll
        for (int m = 0; m < 3; ++m) { s_z0[tt][m] = o.z0[m]; s_x0[tt][m] = fmaf(o.a[m], r0[m], n0[m]); s_d[tt][m] = o.d[m]; }
      }
      if (pre_dump && c < 3) pre_dump[(pt * TF_K + tt) * 3 + c] = c == 0 ? o.z0[0] : c == 1 ? o.z0[1] : o.z0[2];
    }
    s_part[hf][c] = sdr;
    __syncthreads();
    if (hf == 0) dqkv[pt * ldg + c] = -(s_part[0][c] + s_part[1][c]);          // dx_q = -sum_t dr
    if (tid < 3 * TF_K) {                                    // dh0[t][m] = sum_c dp[t][c] W3[c][m]: four running sums in fp64, channel order
      const int tt = tid / 3, m = tid - 3 * tt;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
      for (int i = 0; i < TF_C; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(&s_dp[tt][i]);
        a0 = fma((double)v.x, (double)s_w3[m][i], a0); a1 = fma((double)v.y, (double)s_w3[m][i + 1], a1);
        a2 = fma((double)v.z, (double)s_w3[m][i + 2], a2); a3 = fma((double)v.w, (double)s_w3[m][i + 3], a3);
      }
      const float dh0 = (float)((a0 + a1) + (a2 + a3));
      s_dz0[tt][m] = s_z0[tt][m] > 0.0f ? dh0 : 0.0f;
    }
    __syncthreads();
    if (tid < 27) {                                          // one moment per thread, over the slots in order
      const int k = tid;
      const int m = k < 6 ? k % 3 : k < 24 ? ((k - 6) % 9) / 3 : 0, l = k < 6 ? 0 : (k - 6) % 3;
#pragma unroll 1
      for (int i = 0; i < TF_K; ++i) {
        const double dz = (double)s_dz0[i][m], xh = (double)s_x0[i][m], dd = (double)s_d[i][l];
        mom += k < 3 ? dz : k < 6 ? dz * xh : k < 15 ? dz * dd : k < 24 ? xh * dd : dd;
      }
    }
    __syncthreads();                                         // the tiles have been read
  }
  double* p = part + (int64_t)blockIdx.x * NP_BWD_R;
#pragma unroll 1
  for (int m = 0; m < 4; ++m) {                              // dW3[c][0 .. 2], db3[c]: the two halves of a channel in half order
    s_red[hf][c] = m == 0 ? dw3[0] : m == 1 ? dw3[1] : m == 2 ? dw3[2] : db3;
    __syncthreads();
    if (hf == 0) p[m < 3 ? 3 * c + m : 3 * TF_C + c] = s_red[0][c] + s_red[1][c];
    __syncthreads();
  }
  if (tid < 27) p[4 * TF_C + tid] = mom;
}

// ------------------------------------------------------------------------------------------------ backward 4: dx_k | dx_v by inverse lists
// off [N + 1], ent: the (point 16 + slot) entries whose index is m, ascending.  Waves 0-1 sum the k list of row m, waves 2-3 the v list.
__global__ __launch_bounds__(PT_THREADS) void ptf_bwd_gather_kernel(const float* __restrict__ dout, const float* __restrict__ w_in,
                                                                   const float* __restrict__ du, const float* __restrict__ xq,
                                                                   const float* __restrict__ xk, int64_t ld, const float* __restrict__ xyz,
                                                                   const float* __restrict__ tw, int64_t N, const int64_t* __restrict__ off_k,
                                                                   const int32_t* __restrict__ ent_k, const int64_t* __restrict__ off_v,
                                                                   const int32_t* __restrict__ ent_v, float* __restrict__ dqkv, int64_t ldg) {
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), side = tid >> 7;
  const int jc = c & (TF_K - 1);
  if (side == 0) {
    float w2c[TF_K];
#pragma unroll
    for (int i = 0; i < TF_K; ++i) w2c[i] = tw[TW_W2 + i * TF_C + c];
    const float r1 = tw[TW_R1 + c], n1 = tw[TW_N1 + c], m1 = tw[TW_M1 + c], m2 = tw[TW_M1 + TF_C + c];
    const PtfChan w = ptf_chan_load(tw, c);
    for (int64_t m = blockIdx.x; m < N; m += gridDim.x) {
      const float kk = xk[m * ld + c];
      float acc = 0.0f;
      for (int64_t e = off_k[m]; e < off_k[m + 1]; ++e) {
        const int ent = ent_k[e];
        const int64_t n = ent >> 4;
        const PtfRel o = ptf_relation(w, xyz, N, (int)m, xyz[3 * n], xyz[3 * n + 1], xyz[3 * n + 2], kk, xq[n * ld + c]);
        const float dh1 = ptf_dh1(du + (int64_t)ent * TF_K, w2c);
        acc += ptf_dr(dh1, o.z1, o.r, w.s1, r1, n1, m1, m2);
      }
      dqkv[m * ldg + TF_C + c] = acc;
    }
  } else {
    for (int64_t m = blockIdx.x; m < N; m += gridDim.x) {
      float acc = 0.0f;
      for (int64_t e = off_v[m]; e < off_v[m + 1]; ++e) {
        const int ent = ent_v[e];
        acc += dout[(int64_t)(ent >> 4) * TF_C + c] * w_in[(int64_t)ent * TF_K + jc];
      }
      dqkv[m * ldg + 2 * TF_C + c] = acc;
    }
  }
}

inline int64_t point_grid(int64_t N) { return N < PT_MAX_WG ? N : PT_MAX_WG; }

}  // namespace

#define PTF_SIZES(name)                                                      \
  PFPP_REQUIRE(N >= 0, "bad sizes");                                         \
  PFPP_SUPPORTED(C == TF_C, "rows of 128 channels only");                    \
  PFPP_SUPPORTED(K == TF_K, "K must be 16");                                 \
  PFPP_SUPPORTED(N < (1ll << 31) / (TF_K * TF_K), "index range exceeds int32"); \
  if (N == 0) return PFPP_OK

extern "C" int pfpp_ptf_train_bn3_stats(const float* xyz, const int32_t* idx_k, const float* pack, int64_t N, int64_t K, double* workspace,
                                        double* sums, pfpp_stream_t stream) {
  const int64_t C = TF_C;
  PTF_SIZES();
  PFPP_REQUIRE(xyz && idx_k && pack && workspace && sums, "null pointer");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t rows = N * TF_K;
  const int64_t G = (rows + PT_THREADS - 1) / PT_THREADS < 256 ? (rows + PT_THREADS - 1) / PT_THREADS : 256;
  hipLaunchKernelGGL(ptf_bn3_stats_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, xyz, idx_k, pack, N, workspace);
  fold(st, workspace, G, NP_BN3, sums);
  return pfpp::check_launch("pfpp_ptf_train_bn3_stats");
}

extern "C" int pfpp_ptf_train_bn_finalise(const double* sums, int64_t which, int64_t rows, const float* gamma, const float* beta, float eps,
                                          float momentum, float* running_mean, float* running_var, float* pack, pfpp_stream_t stream) {
  PFPP_REQUIRE(which >= 0 && which <= 2 && rows >= 2 && eps >= 0.0f && momentum >= 0.0f && momentum <= 1.0f, "bad sizes");
  PFPP_REQUIRE(sums && gamma && beta && running_mean && running_var && pack, "null pointer");
  const int C = which == 0 ? 3 : which == 1 ? TF_C : TF_K;
  const int so = which == 0 ? TW_S0 : which == 1 ? TW_S1 : TW_S2, to = which == 0 ? TW_T0 : which == 1 ? TW_T1 : TW_T2;
  const int ro = which == 0 ? TW_R0 : which == 1 ? TW_R1 : TW_R2, no = which == 0 ? TW_N0 : which == 1 ? TW_N1 : TW_N2;
  hipLaunchKernelGGL(ptf_bn_finalise_kernel, dim3(1), dim3(128), 0, pfpp::as_stream(stream), sums, C, (double)rows, gamma, beta, (double)eps,
                     (double)momentum, running_mean, running_var, pack + so, pack + to, pack + ro, pack + no);
  return pfpp::check_launch("pfpp_ptf_train_bn_finalise");
}

extern "C" int pfpp_ptf_train_bn128_stats(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, const float* pack,
                                          int64_t N, int64_t C, int64_t K, double* workspace, double* sums, float* pre_dump,
                                          pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(q && k && xyz && idx_k && pack && workspace && sums, "null pointer");
  PFPP_REQUIRE(ld >= C, "ld >= C");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t G = point_grid(N);
  hipLaunchKernelGGL(ptf_bn128_stats_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, q, k, ld, xyz, idx_k, pack, N, workspace, pre_dump);
  fold(st, workspace, G, NP_BN128, sums);
  return pfpp::check_launch("pfpp_ptf_train_bn128_stats");
}

extern "C" int pfpp_ptf_train_tile(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, const float* pack,
                                   int64_t N, int64_t C, int64_t K, float* u, double* workspace, double* sums, float* pre_dump,
                                   pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(q && k && xyz && idx_k && pack && u && workspace && sums, "null pointer");
  PFPP_REQUIRE(ld >= C && pfpp::aligned16(pack), "ld >= C, pack 16-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t G = point_grid(N);
  hipLaunchKernelGGL(ptf_tile_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, q, k, ld, xyz, idx_k, pack, N, u, workspace, pre_dump);
  fold(st, workspace, G, NP_TILE, sums);
  return pfpp::check_launch("pfpp_ptf_train_tile");
}

extern "C" int pfpp_ptf_train_finish(const float* v, int64_t ld, const float* xyz, const int32_t* idx_k, const int32_t* idx_v, const float* pack,
                                     int64_t N, int64_t C, int64_t K, const float* u, float* w, float* out, float* pre_dump,
                                     pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(v && xyz && idx_k && idx_v && pack && u && w && out, "null pointer");
  PFPP_REQUIRE(ld >= C, "ld >= C");
  hipLaunchKernelGGL(ptf_finish_kernel, dim3((unsigned)point_grid(N)), dim3(PT_THREADS), 0, pfpp::as_stream(stream), v, ld, xyz, idx_k, idx_v,
                     pack, N, u, w, out, pre_dump);
  return pfpp::check_launch("pfpp_ptf_train_finish");
}

extern "C" int pfpp_ptf_train_bwd_w(const float* dout, const float* w, const float* u, const float* v, int64_t ld, const float* xyz,
                                    const int32_t* idx_k, const int32_t* idx_v, float* pack, int64_t N, int64_t C, int64_t K, float* dz2,
                                    double* workspace, double* sums, float* pre_dump, pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(dout && w && u && v && xyz && idx_k && idx_v && pack && dz2 && workspace && sums, "null pointer");
  PFPP_REQUIRE(ld >= C, "ld >= C");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t G = point_grid(N);
  hipLaunchKernelGGL(ptf_bwd_w_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, dout, w, u, v, ld, xyz, idx_k, idx_v, pack, N, dz2, workspace,
                     pre_dump);
  fold(st, workspace, G, NP_BWD_W, sums, TF_K * TF_K + TF_K, 2 * TF_K, 1.0 / (double)(N * TF_K), pack + TW_M2);
  return pfpp::check_launch("pfpp_ptf_train_bwd_w");
}

extern "C" int pfpp_ptf_train_bwd_u(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, float* pack, int64_t N,
                                    int64_t C, int64_t K, const float* u, float* du, double* workspace, double* sums, float* pre_dump,
                                    pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(q && k && xyz && idx_k && pack && u && du && workspace && sums, "null pointer");
  PFPP_REQUIRE(ld >= C, "ld >= C");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t G = point_grid(N);
  hipLaunchKernelGGL(ptf_bwd_u_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, q, k, ld, xyz, idx_k, pack, N, u, du, workspace, pre_dump);
  fold(st, workspace, G, NP_BWD_U, sums, TF_K * TF_C, 2 * TF_C, 1.0 / (double)(N * TF_K), pack + TW_M1);
  return pfpp::check_launch("pfpp_ptf_train_bwd_u");
}

extern "C" int pfpp_ptf_train_bwd_r(const float* dout, const float* w, const float* du, const float* q, const float* k, int64_t ld,
                                    const float* xyz, const int32_t* idx_k, const float* pack, int64_t N, int64_t C, int64_t K, float* dqkv,
                                    int64_t ldg, double* workspace, double* sums, float* pre_dump, pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(dout && w && du && q && k && xyz && idx_k && pack && dqkv && workspace && sums, "null pointer");
  PFPP_REQUIRE(ld >= C && ldg >= 3 * C && pfpp::aligned16(du), "ld >= C, ldg >= 3 C, du 16-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t G = point_grid(N);
  hipLaunchKernelGGL(ptf_bwd_r_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, st, dout, w, du, q, k, ld, xyz, idx_k, pack, N, dqkv, ldg,
                     workspace, pre_dump);
  fold(st, workspace, G, NP_BWD_R, sums);
  return pfpp::check_launch("pfpp_ptf_train_bwd_r");
}

extern "C" int pfpp_ptf_train_bwd_gather(const float* dout, const float* w, const float* du, const float* q, const float* k, int64_t ld,
                                         const float* xyz, const float* pack, int64_t N, int64_t C, int64_t K, const int64_t* off_k,
                                         const int32_t* ent_k, const int64_t* off_v, const int32_t* ent_v, float* dqkv, int64_t ldg,
                                         pfpp_stream_t stream) {
  PTF_SIZES();
  PFPP_REQUIRE(dout && w && du && q && k && xyz && pack && off_k && ent_k && off_v && ent_v && dqkv, "null pointer");
  PFPP_REQUIRE(ld >= C && ldg >= 3 * C && pfpp::aligned16(du), "ld >= C, ldg >= 3 C, du 16-byte aligned");
  const int64_t G = N < 4096 ? N : 4096;
  hipLaunchKernelGGL(ptf_bwd_gather_kernel, dim3((unsigned)G), dim3(PT_THREADS), 0, pfpp::as_stream(stream), dout, w, du, q, k, ld, xyz, pack, N,
                     off_k, ent_k, off_v, ent_v, dqkv, ldg);
  return pfpp::check_launch("pfpp_ptf_train_bwd_gather");
}
