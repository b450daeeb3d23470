// Training of the matcher's DGCNN encoder (Jigsaw_matching/model/modules/encoder/dgcnn.py:41-56, 130-213 in .train() under autograd),
// in the decomposed form of csrc/dgcnn.hip: uv = X [W_a ; W_b - W_a]^T is one product per level, z_ij = u[idx_ij] + v[i] (0 for a padded
// slot) is never stored.  The BatchNorm of a level normalises with the statistics of all R = 20 N slot rows, padded zeros included.
//
//  * dgt_stats_kernel<LPR> / dgt_finalise_kernel — one gather pass over u: a thread owns four channels of a point (the ownership of
//    dgcnn_edge_kernel, the 20 float4 of u in flight together) and produces e = max_j z (gamma >= 0) or min_j z (gamma < 0) by
//    comparisons in slot order (a later slot must be strictly better: the first slot wins a tie), the winning slot as one byte, and the
//    sums of z and z^2 over its slots in fp64.  A workgroup takes a contiguous share of the points, reduces its row phases in LDS in
//    phase order and writes ONE fp64 partial row; the finalise folds the workgroups in a fixed order (8 slices, then the slices in order),
//    writes coef = a | b | mean | rstd (biased variance) and moves the running buffers (unbiased variance, fp64, rounded once).
//  * dgt_apply_kernel — out = LeakyReLU(y a + b) with one multiply and one add, not fused (the arithmetic of dgcnn_edge_kernel).
//  * dgt_bwd_partial_kernel / dgt_bwd_finalise_kernel / dgt_bwd_dy_kernel — h = (g1 + g2) (y a + b > 0 ? 1 : slope) with the forward's
//    own operations, dbeta = sum h, dgamma = sum h (y - mean) rstd in fp64 partials, m1 = dbeta / count, m2 = dgamma / count; with dy
//    the plain BatchNorm backward dy = a ((h - m1) - x_hat m2) over the same rows (conv5: count = rows).
//  * dgt_dv_kernel<LPR> — walks the forward lists: dv[i] = a (h_i [w_i real] - n_i m1 - m2 rstd (sum_{j real} u[idx_ij] + n_i (v[i] - mean))).
//  * dgt_du_kernel<LPR> — walks inverse lists of any length: du[p] = a (sum_{(i,j): idx_ij = p} h_i [w_i = j] - c_p m1
//    - m2 rstd (c_p (u[p] - mean) + sum v[i])).  The dense terms are summed in fp64 in list order and rounded once.
// No atomics anywhere: two runs agree bitwise.  This unit is compiled without contraction.
#include "pfpp_common.h"

namespace {

constexpr int DG_K = 20;
constexpr int DT_THREADS = 256;
constexpr int DT_MAX_WG = PFPP_DGCNN_TRAIN_MAX_WG;           // partial rows of 2 C <= 512 doubles
constexpr int DT_MAX_C = 1024;
constexpr int FO_OUT = 32, FO_SLICES = 8;

inline unsigned fold_grid(int64_t C) { return (unsigned)((C + FO_OUT - 1) / FO_OUT); }

// part [G][stride] fp64: the columns k0 and k1 folded over the workgroups; slice s adds g = s, s + 8, ... in that order, then the eight
// slices in slice order.  The result is valid in the threads of slice 0.
__device__ __forceinline__ void fold_pair(const double* __restrict__ part, int G, int stride, int k0, int k1, bool live,
                                          double (*s_sum)[FO_SLICES][FO_OUT], double& r0, double& r1) {
  const int o = threadIdx.x & (FO_OUT - 1), slice = threadIdx.x >> 5;
  double a0 = 0.0, a1 = 0.0;
  if (live)
    for (int g = slice; g < G; g += FO_SLICES) {
      a0 += part[(int64_t)g * stride + k0];
      a1 += part[(int64_t)g * stride + k1];
    }
  s_sum[0][slice][o] = a0;
  s_sum[1][slice][o] = a1;
  __syncthreads();
  r0 = s_sum[0][0][o];
  r1 = s_sum[1][0][o];
#pragma unroll
  for (int i = 1; i < FO_SLICES; ++i) { r0 += s_sum[0][i][o]; r1 += s_sum[1][i][o]; }
}

// workgroups and rows per workgroup of a pass over `rows` rows, `per` rows per sweep of a workgroup
inline int64_t share_grid(int64_t rows, int64_t per, int64_t max_wg, int64_t* share) {
  int64_t G = (rows + 4 * per - 1) / (4 * per);              // at least four sweeps per workgroup before another one is started
  if (G > max_wg) G = max_wg;
  if (G < 1) G = 1;
  *share = (rows + G - 1) / G;
  if (*share < 1) *share = 1;
  if (rows < 1) return 1;
  return (rows + *share - 1) / *share;                       // no empty workgroup
}

// the reduction of the row phases of a workgroup: red [RP][2 C] -> part[blockIdx.x][2 C], phases in order
__device__ __forceinline__ void phases_to_partial(const double* red, int RP, int C, double* __restrict__ part) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += DT_THREADS) {
    double a = 0.0;
    for (int p = 0; p < RP; ++p) a += red[(size_t)p * 2 * C + i];
    part[(size_t)blockIdx.x * 2 * C + i] = a;
  }
}

// ------------------------------------------------------------------------------------------------ statistics + extremum
template <int LPR>
__global__ __launch_bounds__(DT_THREADS) void dgt_stats_kernel(const float* __restrict__ uv, int64_t ld, const int32_t* __restrict__ idx,
                                                               const float* __restrict__ gamma, int64_t N, int64_t share,
                                                               float* __restrict__ e_out, unsigned char* __restrict__ win_out,
                                                               double* __restrict__ part) {
  constexpr int CO = 4 * LPR, RP = DT_THREADS / LPR;
  __shared__ double red[RP * 2 * CO];                        // 16 KiB
  const int cl = threadIdx.x % LPR, rp = threadIdx.x / LPR;
  const int c = 4 * cl;
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < N ? r0 + share : N;
  const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
  const bool up[4] = {gm.x >= 0.0f, gm.y >= 0.0f, gm.z >= 0.0f, gm.w >= 0.0f};
  double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
  for (int64_t i = r0 + rp; i < r1; i += RP) {
    int nb[DG_K];
#pragma unroll
    for (int t = 0; t < DG_K / 4; ++t) {
      const int4 v = reinterpret_cast<const int4*>(idx + i * DG_K)[t];
      nb[4 * t] = v.x; nb[4 * t + 1] = v.y; nb[4 * t + 2] = v.z; nb[4 * t + 3] = v.w;
    }
    const float4 v = *reinterpret_cast<const float4*>(uv + i * ld + CO + c);
    float4 u[DG_K];
#pragma unroll
    for (int t = 0; t < DG_K; ++t) {                         // a slot that holds N (or anything outside [0, N)) reads nothing
      const bool ok = (unsigned)nb[t] < (unsigned)N;
      u[t] = ok ? *reinterpret_cast<const float4*>(uv + (int64_t)nb[t] * ld + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    float hi[4], lo[4];
    int ahi[4] = {0, 0, 0, 0}, alo[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < DG_K; ++t) {
      const bool ok = (unsigned)nb[t] < (unsigned)N;
      const float z[4] = {ok ? __fadd_rn(u[t].x, v.x) : 0.0f, ok ? __fadd_rn(u[t].y, v.y) : 0.0f, ok ? __fadd_rn(u[t].z, v.z) : 0.0f,
                          ok ? __fadd_rn(u[t].w, v.w) : 0.0f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double zd = (double)z[k];
        s[k] += zd;
        q[k] += zd * zd;
        if (t == 0) {
          hi[k] = z[k]; lo[k] = z[k];
        } else {
          if (z[k] > hi[k]) { hi[k] = z[k]; ahi[k] = t; }
          if (z[k] < lo[k]) { lo[k] = z[k]; alo[k] = t; }
        }
      }
    }
    *reinterpret_cast<float4*>(e_out + i * CO + c) = make_float4(up[0] ? hi[0] : lo[0], up[1] ? hi[1] : lo[1], up[2] ? hi[2] : lo[2],
                                                                 up[3] ? hi[3] : lo[3]);
    *reinterpret_cast<uchar4*>(win_out + i * CO + c) = make_uchar4((unsigned char)(up[0] ? ahi[0] : alo[0]), (unsigned char)(up[1] ? ahi[1] : alo[1]),
                                                                  (unsigned char)(up[2] ? ahi[2] : alo[2]), (unsigned char)(up[3] ? ahi[3] : alo[3]));
  }
  double* o = red + (size_t)rp * 2 * CO;
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[c + k] = s[k]; o[CO + c + k] = q[k]; }
  phases_to_partial(red, RP, CO, part);
}

// sums [2 C] (optional): the folded sums of z and z^2
__global__ __launch_bounds__(FO_OUT * FO_SLICES) void dgt_finalise_kernel(const double* __restrict__ part, int G, int C, double rows,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         double eps, double momentum, float* __restrict__ running_mean,
                                                                         float* __restrict__ running_var, float* __restrict__ coef,
                                                                         double* __restrict__ sums) {
  __shared__ double s_sum[2][FO_SLICES][FO_OUT];
  const int c = blockIdx.x * FO_OUT + (threadIdx.x & (FO_OUT - 1));
  const bool live = c < C;
  double s, q;
  fold_pair(part, G, 2 * C, live ? c : 0, live ? C + c : 0, live, s_sum, s, q);
  if ((threadIdx.x >> 5) != 0 || !live) return;
  if (sums) { sums[c] = s; sums[C + c] = q; }
  const double mean = s / rows;
  double var = q / rows - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const double rs = 1.0 / sqrt(var + eps);
  const float a = (float)((double)gamma[c] * rs);
  coef[c] = a;
  coef[C + c] = (float)((double)beta[c] - mean * (double)a);
  coef[2 * C + c] = (float)mean;
  coef[3 * C + c] = (float)rs;
  if (running_mean) {
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * rows / (rows - 1.0)));
  }
}

// ------------------------------------------------------------------------------------------------ apply + LeakyReLU
// what the forward writes and the backward thresholds: one multiply, then one add
__device__ __forceinline__ float dgt_pre(float y, float a, float b) { return __fadd_rn(__fmul_rn(y, a), b); }

__global__ __launch_bounds__(DT_THREADS) void dgt_apply_kernel(const float* __restrict__ y, int64_t rows, int C, int64_t ld,
                                                               const float* __restrict__ coef, float slope, float* __restrict__ out,
                                                               int64_t ldo) {
  const int CL = C / 4;
  const int64_t i = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (i >= rows * CL) return;
  const int64_t r = i / CL;
  const int c = (int)(i - r * CL) * 4;
  const float4 a = *reinterpret_cast<const float4*>(coef + c), b = *reinterpret_cast<const float4*>(coef + C + c);
  const float4 t = *reinterpret_cast<const float4*>(y + r * ld + c);
  float4 o = make_float4(dgt_pre(t.x, a.x, b.x), dgt_pre(t.y, a.y, b.y), dgt_pre(t.z, a.z, b.z), dgt_pre(t.w, a.w, b.w));
  o.x = o.x > 0.0f ? o.x : __fmul_rn(o.x, slope);
  o.y = o.y > 0.0f ? o.y : __fmul_rn(o.y, slope);
  o.z = o.z > 0.0f ? o.z : __fmul_rn(o.z, slope);
  o.w = o.w > 0.0f ? o.w : __fmul_rn(o.w, slope);
  *reinterpret_cast<float4*>(out + r * ldo + c) = o;
}

// ------------------------------------------------------------------------------------------------ BatchNorm + LeakyReLU backward
// block: CL = C / 4 column lanes x RP = 256 / CL row phases; h [rows, C] is written here
__global__ __launch_bounds__(DT_THREADS) void dgt_bwd_partial_kernel(const float* __restrict__ y, int64_t ld, const float* __restrict__ g1,
                                                                     int64_t ldg1, const float* __restrict__ g2, int64_t ldg2, int64_t rows,
                                                                     int C, int64_t share, const float* __restrict__ coef, float slope,
                                                                     float* __restrict__ h, double* __restrict__ part) {
  __shared__ double red[2 * DT_MAX_C];                       // [RP][2 C], RP C <= 1024
  const int CL = C / 4, RP = DT_THREADS / CL;
  const int cl = threadIdx.x % CL, rp = threadIdx.x / CL;
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < rows ? r0 + share : rows;
  if (rp < RP) {
    float a[4], b[4], m[4], rs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = cl * 4 + k;
      a[k] = coef[c]; b[k] = coef[C + c]; m[k] = coef[2 * C + c]; rs[k] = coef[3 * C + c];
    }
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    for (int64_t r = r0 + rp; r < r1; r += RP) {
      const float4 yv = *reinterpret_cast<const float4*>(y + r * ld + cl * 4);
      float4 gv = *reinterpret_cast<const float4*>(g1 + r * ldg1 + cl * 4);
      if (g2) {
        const float4 g = *reinterpret_cast<const float4*>(g2 + r * ldg2 + cl * 4);
        gv.x = __fadd_rn(gv.x, g.x); gv.y = __fadd_rn(gv.y, g.y); gv.z = __fadd_rn(gv.z, g.z); gv.w = __fadd_rn(gv.w, g.w);
      }
      const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
      float hh[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hh[k] = dgt_pre(yy[k], a[k], b[k]) > 0.0f ? gg[k] : __fmul_rn(gg[k], slope);
        s[k] += (double)hh[k];
        q[k] += (double)hh[k] * ((double)yy[k] - (double)m[k]) * (double)rs[k];
      }
      *reinterpret_cast<float4*>(h + r * (int64_t)C + cl * 4) = make_float4(hh[0], hh[1], hh[2], hh[3]);
    }
    double* o = red + (size_t)rp * 2 * C;
#pragma unroll
    for (int k = 0; k < 4; ++k) { o[cl * 4 + k] = s[k]; o[C + cl * 4 + k] = q[k]; }
  }
  phases_to_partial(red, RP, C, part);
}

__global__ __launch_bounds__(FO_OUT * FO_SLICES) void dgt_bwd_finalise_kernel(const double* __restrict__ part, int G, int C, double count,
                                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                             float* __restrict__ means) {
  __shared__ double s_sum[2][FO_SLICES][FO_OUT];
  const int c = blockIdx.x * FO_OUT + (threadIdx.x & (FO_OUT - 1));
  const bool live = c < C;
  double s, q;
  fold_pair(part, G, 2 * C, live ? c : 0, live ? C + c : 0, live, s_sum, s, q);
  if ((threadIdx.x >> 5) != 0 || !live) return;
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
  means[c] = (float)(s / count);
  means[C + c] = (float)(q / count);
}

// dy may alias h (the same element is read, then written)
__global__ __launch_bounds__(DT_THREADS) void dgt_bwd_dy_kernel(const float* __restrict__ y, int64_t ld, const float* h, int64_t rows, int C,
                                                                const float* __restrict__ coef, const float* __restrict__ means, float* dy) {
  const int CL = C / 4;
  const int64_t i = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (i >= rows * CL) return;
  const int64_t r = i / CL;
  const int c = (int)(i - r * CL) * 4;
  const float4 yv = *reinterpret_cast<const float4*>(y + r * ld + c);
  const float4 hv = *reinterpret_cast<const float4*>(h + r * (int64_t)C + c);
  const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, hh[4] = {hv.x, hv.y, hv.z, hv.w};
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float xh = (yy[k] - coef[2 * C + c + k]) * coef[3 * C + c + k];
    o[k] = coef[c + k] * ((hh[k] - means[c + k]) - xh * means[C + c + k]);
  }
  *reinterpret_cast<float4*>(dy + r * (int64_t)C + c) = make_float4(o[0], o[1], o[2], o[3]);
}

// ------------------------------------------------------------------------------------------------ the two backward gathers
// duv [N, 2 CO]: du in the columns [0, CO), dv in [CO, 2 CO)
template <int LPR>
__global__ __launch_bounds__(DT_THREADS) void dgt_dv_kernel(const float* __restrict__ uv, int64_t ld, const int32_t* __restrict__ idx,
                                                            const unsigned char* __restrict__ win, const float* __restrict__ h,
                                                            const float* __restrict__ coef, const float* __restrict__ means, int64_t N,
                                                            float* __restrict__ duv) {
  constexpr int CO = 4 * LPR;
  const int64_t t = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  const int64_t i = t / LPR;
  const int c = 4 * (int)(t % LPR);
  if (i >= N) return;
  int nb[DG_K];
#pragma unroll
  for (int s = 0; s < DG_K / 4; ++s) {
    const int4 v = reinterpret_cast<const int4*>(idx + i * DG_K)[s];
    nb[4 * s] = v.x; nb[4 * s + 1] = v.y; nb[4 * s + 2] = v.z; nb[4 * s + 3] = v.w;
  }
  float4 u[DG_K];
#pragma unroll
  for (int s = 0; s < DG_K; ++s) {
    const bool ok = (unsigned)nb[s] < (unsigned)N;
    u[s] = ok ? *reinterpret_cast<const float4*>(uv + (int64_t)nb[s] * ld + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const float4 v = *reinterpret_cast<const float4*>(uv + i * ld + CO + c);
  const float4 hv = *reinterpret_cast<const float4*>(h + i * CO + c);
  const uchar4 wv = *reinterpret_cast<const uchar4*>(win + i * CO + c);
  double su[4] = {0, 0, 0, 0};
  int n = 0;
#pragma unroll
  for (int s = 0; s < DG_K; ++s) {
    const bool ok = (unsigned)nb[s] < (unsigned)N;
    n += ok ? 1 : 0;
    su[0] += (double)u[s].x; su[1] += (double)u[s].y; su[2] += (double)u[s].z; su[3] += (double)u[s].w;   // a padded slot adds 0
  }
  const float vv[4] = {v.x, v.y, v.z, v.w}, hh[4] = {hv.x, hv.y, hv.z, hv.w};
  const int ww[4] = {wv.x, wv.y, wv.z, wv.w};
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = coef[c + k], mu = coef[2 * CO + c + k], rs = coef[3 * CO + c + k], m1 = means[c + k], m2 = means[CO + c + k];
    int wslot = 0;                                           // the index in the winning slot, without a dynamic register index
#pragma unroll
    for (int s = 0; s < DG_K; ++s) wslot = ww[k] == s ? nb[s] : wslot;
    const bool real = ww[k] < DG_K && (unsigned)wslot < (unsigned)N;
    const double dense = (double)n * m1 + m2 * rs * (su[k] + (double)n * ((double)vv[k] - mu));
    o[k] = (float)(a * ((real ? (double)hh[k] : 0.0) - dense));
  }
  *reinterpret_cast<float4*>(duv + i * (2 * CO) + CO + c) = make_float4(o[0], o[1], o[2], o[3]);
}

// the entries of point p's list are the flat positions e = i 20 + j with idx[e] = p, ascending; the list has any length
template <int LPR>
__global__ __launch_bounds__(DT_THREADS) void dgt_du_kernel(const float* __restrict__ uv, int64_t ld, const int64_t* __restrict__ off,
                                                            const int32_t* __restrict__ ent, int64_t n_ent,
                                                            const unsigned char* __restrict__ win, const float* __restrict__ h,
                                                            const float* __restrict__ coef, const float* __restrict__ means, int64_t N,
                                                            float* __restrict__ duv) {
  constexpr int CO = 4 * LPR;
  const int64_t t = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  const int64_t p = t / LPR;
  const int c = 4 * (int)(t % LPR);
  if (p >= N) return;
  int64_t e0 = off[p], e1 = off[p + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > n_ent ? n_ent : e1;                              // a malformed list reads nothing outside ent
  double sh[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
  int64_t cnt = 0;
  for (int64_t q = e0; q < e1; ++q) {
    const int e = ent[q];
    const int64_t i = e / DG_K;
    const int j = e - (int)i * DG_K;
    if ((uint64_t)i >= (uint64_t)N) continue;               // an entry outside the table reads nothing
    const float4 v = *reinterpret_cast<const float4*>(uv + i * ld + CO + c);
    const float4 hv = *reinterpret_cast<const float4*>(h + i * CO + c);
    const uchar4 wv = *reinterpret_cast<const uchar4*>(win + i * CO + c);
    ++cnt;
    sv[0] += (double)v.x; sv[1] += (double)v.y; sv[2] += (double)v.z; sv[3] += (double)v.w;
    sh[0] += wv.x == j ? (double)hv.x : 0.0;
    sh[1] += wv.y == j ? (double)hv.y : 0.0;
    sh[2] += wv.z == j ? (double)hv.z : 0.0;
    sh[3] += wv.w == j ? (double)hv.w : 0.0;
  }
  const float4 u = *reinterpret_cast<const float4*>(uv + p * ld + c);
  const float uu[4] = {u.x, u.y, u.z, u.w};
  float o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = coef[c + k], mu = coef[2 * CO + c + k], rs = coef[3 * CO + c + k], m1 = means[c + k], m2 = means[CO + c + k];
    const double dense = (double)cnt * m1 + m2 * rs * ((double)cnt * ((double)uu[k] - mu) + sv[k]);
    o[k] = (float)(a * (sh[k] - dense));
  }
  *reinterpret_cast<float4*>(duv + p * (2 * CO) + c) = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace

#define DGT_EDGE_SIZES()                                                                                             \
  PFPP_REQUIRE(N >= 0, "bad sizes");                                                                                 \
  PFPP_SUPPORTED(C_out == 64 || C_out == 128 || C_out == 256, "64, 128 or 256 output channels only");                \
  PFPP_SUPPORTED(K == DG_K, "K must be 20");                                                                         \
  PFPP_SUPPORTED(N < (1ll << 31) / DG_K, "index range exceeds int32")

extern "C" int pfpp_dgcnn_edge_stats(const float* uv, int64_t ld, const int32_t* idx, const float* gamma, const float* beta, double eps,
                                     double momentum, float* running_mean, float* running_var, int64_t N, int64_t C_out, int64_t K, float* e,
                                     unsigned char* winner, float* coef, double* workspace, pfpp_stream_t stream) {
  DGT_EDGE_SIZES();
  PFPP_REQUIRE(N >= 1, "no points");
  PFPP_REQUIRE(uv && idx && gamma && beta && e && winner && coef && workspace, "null pointer");
  PFPP_REQUIRE(ld >= 2 * C_out && ld % 4 == 0, "ld >= 2 C_out, a multiple of 4");
  PFPP_REQUIRE(!running_mean == !running_var, "running_mean and running_var go together");
  PFPP_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "bad eps / momentum");
  PFPP_REQUIRE(pfpp::aligned16(uv) && pfpp::aligned16(idx) && pfpp::aligned16(gamma) && pfpp::aligned16(e) && pfpp::aligned16(coef) &&
                   (reinterpret_cast<uintptr_t>(winner) & 3) == 0,
               "16-byte alignment (winner: 4-byte)");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t lpr = C_out / 4, per = DT_THREADS / lpr;
  int64_t share;
  const int64_t G = share_grid(N, per, DT_MAX_WG, &share);
  const dim3 grid((unsigned)G), block(DT_THREADS);
  if (C_out == 64) hipLaunchKernelGGL(dgt_stats_kernel<16>, grid, block, 0, st, uv, ld, idx, gamma, N, share, e, winner, workspace);
  else if (C_out == 128) hipLaunchKernelGGL(dgt_stats_kernel<32>, grid, block, 0, st, uv, ld, idx, gamma, N, share, e, winner, workspace);
  else hipLaunchKernelGGL(dgt_stats_kernel<64>, grid, block, 0, st, uv, ld, idx, gamma, N, share, e, winner, workspace);
  double* sums = workspace + (size_t)DT_MAX_WG * 512;       // behind the partial rows: sum z | sum z^2
  hipLaunchKernelGGL(dgt_finalise_kernel, dim3(fold_grid(C_out)), dim3(FO_OUT * FO_SLICES), 0, st, workspace, (int)G, (int)C_out,
                     (double)(N * DG_K), gamma, beta, eps, momentum, running_mean, running_var, coef, sums);
  return pfpp::check_launch("pfpp_dgcnn_edge_stats");
}

#define DGT_ROW_SIZES()                                                                      \
  PFPP_REQUIRE(rows >= 0 && C >= 4 && ld >= C && ld % 4 == 0, "bad sizes");                  \
  PFPP_SUPPORTED(C % 4 == 0 && C <= DT_MAX_C, "C must be a multiple of 4, at most 1024");    \
  PFPP_SUPPORTED(rows < (1ll << 31), "more than 2^31 rows")

extern "C" int pfpp_dgcnn_bn_leaky_apply(const float* y, int64_t rows, int64_t C, int64_t ld, const float* coef, float slope, float* out,
                                         int64_t ldo, pfpp_stream_t stream) {
  DGT_ROW_SIZES();
  PFPP_REQUIRE(ldo >= C && ldo % 4 == 0, "ldo >= C, a multiple of 4");
  if (rows == 0) return PFPP_OK;
  PFPP_REQUIRE(y && coef && out, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(y) && pfpp::aligned16(coef) && pfpp::aligned16(out), "16-byte alignment");
  const int64_t total = rows * (C / 4);
  hipLaunchKernelGGL(dgt_apply_kernel, dim3((unsigned)((total + DT_THREADS - 1) / DT_THREADS)), dim3(DT_THREADS), 0, pfpp::as_stream(stream), y,
                     rows, (int)C, ld, coef, slope, out, ldo);
  return pfpp::check_launch("pfpp_dgcnn_bn_leaky_apply");
}

extern "C" int pfpp_dgcnn_bn_leaky_bwd(const float* y, int64_t ld, const float* g1, int64_t ldg1, const float* g2, int64_t ldg2, int64_t rows,
                                       int64_t C, const float* coef, float slope, double count, float* h, float* dgamma, float* dbeta,
                                       float* means, float* dy, double* workspace, pfpp_stream_t stream) {
  DGT_ROW_SIZES();
  PFPP_REQUIRE(rows >= 1 && count >= 1.0, "no rows");
  PFPP_REQUIRE(y && g1 && coef && h && dgamma && dbeta && means && workspace, "null pointer");
  PFPP_REQUIRE(ldg1 >= C && ldg1 % 4 == 0 && (!g2 || (ldg2 >= C && ldg2 % 4 == 0)), "gradient rows: at least C floats, a multiple of 4");
  PFPP_REQUIRE(pfpp::aligned16(y) && pfpp::aligned16(g1) && pfpp::aligned16(g2) && pfpp::aligned16(h) && pfpp::aligned16(dy), "16-byte alignment");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t per = DT_THREADS / (C / 4) > 0 ? DT_THREADS / (C / 4) : 1;
  int64_t max_wg = (int64_t)DT_MAX_WG * 512 / (2 * C);       // the partial rows fit the workspace
  if (max_wg > DT_MAX_WG) max_wg = DT_MAX_WG;
  int64_t share;
  const int64_t G = share_grid(rows, per, max_wg, &share);
  hipLaunchKernelGGL(dgt_bwd_partial_kernel, dim3((unsigned)G), dim3(DT_THREADS), 0, st, y, ld, g1, ldg1, g2, ldg2, rows, (int)C, share, coef,
                     slope, h, workspace);
  hipLaunchKernelGGL(dgt_bwd_finalise_kernel, dim3(fold_grid(C)), dim3(FO_OUT * FO_SLICES), 0, st, workspace, (int)G, (int)C, count, dgamma,
                     dbeta, means);
  if (dy) {
    const int64_t total = rows * (C / 4);
    hipLaunchKernelGGL(dgt_bwd_dy_kernel, dim3((unsigned)((total + DT_THREADS - 1) / DT_THREADS)), dim3(DT_THREADS), 0, st, y, ld, h, rows, (int)C,
                       coef, means, dy);
  }
  return pfpp::check_launch("pfpp_dgcnn_bn_leaky_bwd");
}

extern "C" int pfpp_dgcnn_edge_bwd_dv(const float* uv, int64_t ld, const int32_t* idx, const unsigned char* winner, const float* h,
                                      const float* coef, const float* means, int64_t N, int64_t C_out, int64_t K, float* duv,
                                      pfpp_stream_t stream) {
  DGT_EDGE_SIZES();
  if (N == 0) return PFPP_OK;
  PFPP_REQUIRE(uv && idx && winner && h && coef && means && duv, "null pointer");
  PFPP_REQUIRE(ld >= 2 * C_out && ld % 4 == 0, "ld >= 2 C_out, a multiple of 4");
  PFPP_REQUIRE(pfpp::aligned16(uv) && pfpp::aligned16(idx) && pfpp::aligned16(h) && pfpp::aligned16(duv) &&
                   (reinterpret_cast<uintptr_t>(winner) & 3) == 0,
               "16-byte alignment (winner: 4-byte)");
  const int64_t lpr = C_out / 4;
  const dim3 grid((unsigned)((N * lpr + DT_THREADS - 1) / DT_THREADS)), block(DT_THREADS);
  hipStream_t s = pfpp::as_stream(stream);
  if (C_out == 64) hipLaunchKernelGGL(dgt_dv_kernel<16>, grid, block, 0, s, uv, ld, idx, winner, h, coef, means, N, duv);
  else if (C_out == 128) hipLaunchKernelGGL(dgt_dv_kernel<32>, grid, block, 0, s, uv, ld, idx, winner, h, coef, means, N, duv);
  else hipLaunchKernelGGL(dgt_dv_kernel<64>, grid, block, 0, s, uv, ld, idx, winner, h, coef, means, N, duv);
  return pfpp::check_launch("pfpp_dgcnn_edge_bwd_dv");
}

extern "C" int pfpp_dgcnn_edge_bwd_du(const float* uv, int64_t ld, const int64_t* off, const int32_t* ent, int64_t n_ent,
                                      const unsigned char* winner, const float* h, const float* coef, const float* means, int64_t N,
                                      int64_t C_out, int64_t K, float* duv, pfpp_stream_t stream) {
  DGT_EDGE_SIZES();
  PFPP_REQUIRE(n_ent >= 0 && n_ent <= N * DG_K, "more entries than slots");
  if (N == 0) return PFPP_OK;
  PFPP_REQUIRE(uv && off && winner && h && coef && means && duv && (ent || n_ent == 0), "null pointer");
  PFPP_REQUIRE(ld >= 2 * C_out && ld % 4 == 0, "ld >= 2 C_out, a multiple of 4");
  PFPP_REQUIRE(pfpp::aligned16(uv) && pfpp::aligned16(h) && pfpp::aligned16(duv) && (reinterpret_cast<uintptr_t>(winner) & 3) == 0,
               "16-byte alignment (winner: 4-byte)");
  const int64_t lpr = C_out / 4;
  const dim3 grid((unsigned)((N * lpr + DT_THREADS - 1) / DT_THREADS)), block(DT_THREADS);
  hipStream_t s = pfpp::as_stream(stream);
  if (C_out == 64) hipLaunchKernelGGL(dgt_du_kernel<16>, grid, block, 0, s, uv, ld, off, ent, n_ent, winner, h, coef, means, N, duv);
  else if (C_out == 128) hipLaunchKernelGGL(dgt_du_kernel<32>, grid, block, 0, s, uv, ld, off, ent, n_ent, winner, h, coef, means, N, duv);
  else hipLaunchKernelGGL(dgt_du_kernel<64>, grid, block, 0, s, uv, ld, off, ent, n_ent, winner, h, coef, means, N, duv);
  return pfpp::check_launch("pfpp_dgcnn_edge_bwd_du");
}
