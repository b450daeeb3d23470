// Training of the matcher's ragged PointNet++ encoder (Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/ in .train() under
// autograd) around the GEMMs: the BatchNorms of the 33 convolutions in front of conv1 on the statistics of all rows of the call, and the backward of the
// grouping and of the interpolation.  The MLP products (forward, dX, dW) are pfpp_gemm in its exact-fp32 mode; sampling, neighbour
// search, grouping and interpolation are csrc/pointnet_ragged.hip, unchanged.
//
//  * rbn_partial_kernel / rbn_finalise_kernel — per-channel sums of y and y^2 over the rows of [rows, ld], any C % 4 == 0, C <= 1024:
//    a workgroup takes one contiguous share of the rows, accumulates in fp64 per thread, reduces its row phases in LDS in phase order
//    and writes ONE fp64 partial row; the finalise folds the workgroups in a fixed order (8 slices of the workgroups per channel, then
//    the slices in order: the scheme of ptf_fold_kernel), writes coef = a | b | mean | rstd (biased variance) and moves the running
//    buffers like torch (unbiased variance, momentum, fp64, rounded once).
//  * rbn_apply_kernel — h = relu(y a + b), optionally the max over `pool` consecutive rows and the first row that attains it.
//  * rbn_pool_bwd_kernel — the max's backward: the pooled gradient goes to the winning row of each group.
//  * rbn_bwd_partial_kernel / rbn_bwd_finalise_kernel / rbn_bwd_apply_kernel — backward of h = relu(BN_train(y)): sums of dz and
//    dz x hat in fp64 (dbeta, dgamma), then dy = gamma rstd (dz - mean dz - x hat mean(dz x hat)).
//    Every kernel that thresholds goes through rbn_pre(): the forward's h > 0 and the backward's sign test are the same bits.
//  * ragged_group_bwd_kernel — dfeats[p] = sum of the grouped rows whose neighbour index is p, walking an inverse list in order.
//  * ragged_interp_bwd_kernel / rcol_partial_kernel — dpoints2[s] = sum w dout over the slots that read s, through an inverse list;
//    with one centroid in the call the column sum over all rows, in fp64 through per-workgroup partials.
// No atomics anywhere: two runs agree bitwise.  This unit is compiled without contraction; the one fused operation is written as fmaf.
#include "pfpp_common.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_WG = PFPP_RAGGED_TRAIN_MAX_WG;
constexpr int RT_MAX_C = 1024;
constexpr int RT_SHARE = 64;                                 // rows a workgroup takes at least before another workgroup is started
constexpr int FO_OUT = 32, FO_SLICES = 8;                    // the fold: 32 outputs x 8 slices per workgroup

// what every ReLU of this unit thresholds: the forward writes max(rbn_pre, 0), the backward tests rbn_pre > 0
__device__ __forceinline__ float rbn_pre(float y, float a, float b) { return fmaf(y, a, b); }

// number of workgroups and rows per workgroup of a pass over `rows` rows
inline int64_t share_grid(int64_t rows, int64_t* share) {
  int64_t G = (rows + RT_SHARE - 1) / RT_SHARE;
  if (G > RT_MAX_WG) G = RT_MAX_WG;
  if (G < 1) G = 1;
  *share = (rows + G - 1) / G;
  if (*share < 1) *share = 1;                                // no rows: one workgroup that finds none
  if (rows < 1) return 1;
  return (rows + *share - 1) / *share;                       // no empty workgroup
}

// part [G][stride] fp64: the columns k0 and k1 folded over the workgroups; slice s adds g = s, s + 8, ... in that order, then the eight
// slices in slice order.  Called by all 256 threads of a workgroup (o = tid & 31 the output, tid >> 5 the slice); the result is valid
// in the threads of slice 0.
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

// ------------------------------------------------------------------------------------------------ statistics
// block: CL = C / 4 column lanes x RP = 256 / CL row phases; workgroup g takes the rows [g share, (g + 1) share)
__global__ __launch_bounds__(RT_THREADS) void rbn_partial_kernel(const float* __restrict__ x, int64_t rows, int C, int64_t ld, int64_t share,
                                                                double* __restrict__ part) {
  __shared__ double red[2 * RT_MAX_C];                       // [RP][2][C], RP C <= 1024
  const int CL = C / 4, RP = RT_THREADS / CL;
  const int cl = threadIdx.x % CL, rp = threadIdx.x / CL;
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < rows ? r0 + share : rows;
  if (rp < RP) {
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    for (int64_t r = r0 + rp; r < r1; r += RP) {
      const float4 v = *reinterpret_cast<const float4*>(x + r * ld + cl * 4);
      const double a = v.x, b = v.y, c = v.z, d = v.w;
      s[0] += a; s[1] += b; s[2] += c; s[3] += d;
      q[0] += a * a; q[1] += b * b; q[2] += c * c; q[3] += d * d;
    }
    double* o = red + (size_t)rp * 2 * C;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[cl * 4 + e] = s[e]; o[C + cl * 4 + e] = q[e]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += RT_THREADS) {
    double a = 0.0;
    for (int p = 0; p < RP; ++p) a += red[(size_t)p * 2 * C + i];
    part[(size_t)blockIdx.x * 2 * C + i] = a;
  }
}

__global__ __launch_bounds__(FO_OUT * FO_SLICES) void rbn_finalise_kernel(const double* __restrict__ part, int G, int C, double rows,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         double eps, double momentum, float* __restrict__ running_mean,
                                                                         float* __restrict__ running_var, float* __restrict__ coef) {
  __shared__ double s_sum[2][FO_SLICES][FO_OUT];
  const int c = blockIdx.x * FO_OUT + (threadIdx.x & (FO_OUT - 1));
  const bool live = c < C;
  double s, q;
  fold_pair(part, G, 2 * C, live ? c : 0, live ? C + c : 0, live, s_sum, s, q);
  if ((threadIdx.x >> 5) != 0 || !live) return;
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

// ------------------------------------------------------------------------------------------------ apply + ReLU (+ max over a pool)
// thread = one float4 column group of one output row
__global__ __launch_bounds__(RT_THREADS) void rbn_apply_kernel(const float* __restrict__ y, int64_t out_rows, int C, int64_t ld,
                                                              const float* __restrict__ coef, float* __restrict__ out, int64_t ldo, int pool,
                                                              int32_t* __restrict__ winner) {
  const int CL = C / 4;
  const int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= out_rows * CL) return;
  const int64_t orow = i / CL;
  const int c = (int)(i - orow * CL) * 4;
  const float4 a = *reinterpret_cast<const float4*>(coef + c);
  const float4 b = *reinterpret_cast<const float4*>(coef + C + c);
  const int np = pool > 0 ? pool : 1;
  float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};                      // the ReLU's output is >= 0: 0 is the identity of the max
  int arg[4] = {-1, -1, -1, -1};                             // the first row that attains a positive max; -1: every row is <= 0
  for (int p = 0; p < np; ++p) {
    const float4 t = *reinterpret_cast<const float4*>(y + (orow * np + p) * ld + c);
    const float v[4] = {rbn_pre(t.x, a.x, b.x), rbn_pre(t.y, a.y, b.y), rbn_pre(t.z, a.z, b.z), rbn_pre(t.w, a.w, b.w)};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[e] > o[e]) { o[e] = v[e]; arg[e] = p; }
  }
  *reinterpret_cast<float4*>(out + orow * ldo + c) = make_float4(o[0], o[1], o[2], o[3]);
  if (winner) *reinterpret_cast<int4*>(winner + orow * C + c) = make_int4(arg[0], arg[1], arg[2], arg[3]);
}

// dh [groups pool, C]: dout[g, c] at the first row of group g that attains max_p relu(rbn_pre) when that max is > 0, else 0
__global__ __launch_bounds__(RT_THREADS) void rbn_pool_bwd_kernel(const float* __restrict__ y, int64_t groups, int pool, int C, int64_t ld,
                                                                 const float* __restrict__ coef, const float* __restrict__ dout, int64_t ldd,
                                                                 float* __restrict__ dh) {
  const int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= groups * C) return;
  const int64_t g = i / C;
  const int c = (int)(i - g * C);
  const float a = coef[c], b = coef[C + c];
  float best = 0.0f;
  int arg = -1;
  for (int p = 0; p < pool; ++p) {
    const float v = rbn_pre(y[(g * pool + p) * ld + c], a, b);
    if (v > best) { best = v; arg = p; }
  }
  const float d = dout[g * ldd + c];
  for (int p = 0; p < pool; ++p) dh[(g * pool + p) * (int64_t)C + c] = (p == arg) ? d : 0.0f;
}

// ------------------------------------------------------------------------------------------------ BatchNorm + ReLU backward
__global__ __launch_bounds__(RT_THREADS) void rbn_bwd_partial_kernel(const float* __restrict__ y, const float* __restrict__ dh, int64_t rows,
                                                                    int C, int64_t ld, int64_t share, const float* __restrict__ coef,
                                                                    double* __restrict__ part) {
  __shared__ double red[2 * RT_MAX_C];
  const int CL = C / 4, RP = RT_THREADS / CL;
  const int cl = threadIdx.x % CL, rp = threadIdx.x / CL;
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < rows ? r0 + share : rows;
  if (rp < RP) {
    float a[4], b[4], m[4], rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = cl * 4 + e;
      a[e] = coef[c]; b[e] = coef[C + c]; m[e] = coef[2 * C + c]; rs[e] = coef[3 * C + c];
    }
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    for (int64_t r = r0 + rp; r < r1; r += RP) {
      const float4 yv = *reinterpret_cast<const float4*>(y + r * ld + cl * 4);
      const float4 gv = *reinterpret_cast<const float4*>(dh + r * (int64_t)C + cl * 4);
      const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dz = rbn_pre(yy[e], a[e], b[e]) > 0.0f ? gg[e] : 0.0f;
        s[e] += (double)dz;
        q[e] += (double)dz * (double)((yy[e] - m[e]) * rs[e]);
      }
    }
    double* o = red + (size_t)rp * 2 * C;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[cl * 4 + e] = s[e]; o[C + cl * 4 + e] = q[e]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += RT_THREADS) {
    double acc = 0.0;
    for (int p = 0; p < RP; ++p) acc += red[(size_t)p * 2 * C + i];
    part[(size_t)blockIdx.x * 2 * C + i] = acc;
  }
}

// dbeta = sum dz, dgamma = sum dz x hat (OVERWRITTEN); means [2 C] = their means as fp32 for the second pass
__global__ __launch_bounds__(FO_OUT * FO_SLICES) void rbn_bwd_finalise_kernel(const double* __restrict__ part, int G, int C, double rows,
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
  means[c] = (float)(s / rows);
  means[C + c] = (float)(q / rows);
}

// dy may alias dh (the same element is read, then written)
__global__ __launch_bounds__(RT_THREADS) void rbn_bwd_apply_kernel(const float* __restrict__ y, const float* dh, int64_t rows, int C, int64_t ld,
                                                                  const float* __restrict__ coef, const float* __restrict__ gamma,
                                                                  const float* __restrict__ means, float* dy) {
  const int CL = C / 4;
  const int64_t total = rows * CL;
  for (int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RT_THREADS) {
    const int64_t r = i / CL;
    const int c = (int)(i - r * CL) * 4;
    const float4 yv = *reinterpret_cast<const float4*>(y + r * ld + c);
    const float4 gv = *reinterpret_cast<const float4*>(dh + r * (int64_t)C + c);
    const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float rs = coef[3 * C + c + e];
      const float dz = rbn_pre(yy[e], coef[c + e], coef[C + c + e]) > 0.0f ? gg[e] : 0.0f;
      const float xh = (yy[e] - coef[2 * C + c + e]) * rs;
      o[e] = (gamma[c + e] * rs) * ((dz - means[c + e]) - xh * means[C + c + e]);
    }
    *reinterpret_cast<float4*>(dy + r * (int64_t)C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------ grouping backward
// a wave per source point: the lanes walk the D feature columns, the entries of the point's list one after the other.  Entry e = s K + j
// names the grouped row s pool + j.
__global__ __launch_bounds__(RT_THREADS) void ragged_group_bwd_kernel(const float* __restrict__ dA, int64_t lda, int D,
                                                                     const int64_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                                     int64_t n_ent, int K, int pool, int64_t Np, float* __restrict__ dfeats,
                                                                     int64_t ldf, int accumulate) {
  const int lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < Np; p += (int64_t)gridDim.x * 4) {
    int64_t beg = off[p], end = off[p + 1];
    if (beg < 0) beg = 0;
    if (end > n_ent) end = n_ent;
    for (int c = lane; c < D; c += 64) {
      float acc = accumulate ? dfeats[p * ldf + c] : 0.0f;
      for (int64_t k = beg; k < end; ++k) {
        const int64_t e = ent[k];
        if ((uint64_t)e >= (uint64_t)n_ent) continue;
        acc += dA[((e / K) * pool + e % K) * lda + c];
      }
      dfeats[p * ldf + c] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------ interpolation backward
// a wave per centroid s: entry e = 3 i + j names slot j of point i, its weight w[e] and the row dout[i, D1 : D1 + D2]
__global__ __launch_bounds__(RT_THREADS) void ragged_interp_bwd_kernel(const float* __restrict__ dout, int64_t ldo, int D1, int D2,
                                                                      const float* __restrict__ w, const int64_t* __restrict__ off,
                                                                      const int32_t* __restrict__ ent, int64_t n_ent, int64_t S,
                                                                      float* __restrict__ dp2) {
  const int lane = threadIdx.x & 63;
  for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < S; s += (int64_t)gridDim.x * 4) {
    int64_t beg = off[s], end = off[s + 1];
    if (beg < 0) beg = 0;
    if (end > n_ent) end = n_ent;
    for (int c = lane; c < D2; c += 64) {
      float acc = 0.0f;
      for (int64_t k = beg; k < end; ++k) {
        const int64_t e = ent[k];
        if ((uint64_t)e >= (uint64_t)n_ent) continue;
        acc += w[e] * dout[(e / 3) * ldo + D1 + c];
      }
      dp2[s * (int64_t)D2 + c] = acc;
    }
  }
}

// one centroid in the whole call: every row reads it with weight 1.  Workgroup g sums its share of the rows per column in fp64.
__global__ __launch_bounds__(RT_THREADS) void rcol_partial_kernel(const float* __restrict__ x, int64_t rows, int cols, int64_t ld, int64_t share,
                                                                 double* __restrict__ part) {
  const int64_t r0 = (int64_t)blockIdx.x * share;
  const int64_t r1 = r0 + share < rows ? r0 + share : rows;
  for (int c = threadIdx.x; c < cols; c += RT_THREADS) {
    double acc = 0.0;
    for (int64_t r = r0; r < r1; ++r) acc += (double)x[r * ld + c];
    part[(size_t)blockIdx.x * cols + c] = acc;
  }
}

__global__ __launch_bounds__(FO_OUT * FO_SLICES) void rcol_fold_kernel(const double* __restrict__ part, int G, int cols, float* __restrict__ out) {
  __shared__ double s_sum[2][FO_SLICES][FO_OUT];
  const int c = blockIdx.x * FO_OUT + (threadIdx.x & (FO_OUT - 1));
  const bool live = c < cols;
  double s, unused;
  fold_pair(part, G, cols, live ? c : 0, live ? c : 0, live, s_sum, s, unused);
  if ((threadIdx.x >> 5) == 0 && live) out[c] = (float)s;
}

inline unsigned fold_grid(int64_t C) { return (unsigned)((C + FO_OUT - 1) / FO_OUT); }

}  // namespace

#define RBN_SIZES()                                                                          \
  PFPP_REQUIRE(rows >= 0 && C >= 4 && ld >= C && ld % 4 == 0, "bad sizes");                  \
  PFPP_SUPPORTED(C % 4 == 0 && C <= RT_MAX_C, "C must be a multiple of 4, at most 1024");    \
  PFPP_SUPPORTED(rows < (1ll << 31), "more than 2^31 rows")

extern "C" int pfpp_ragged_bn_stats(const float* y, int64_t rows, int64_t C, int64_t ld, const float* gamma, const float* beta, double eps,
                                    double momentum, float* running_mean, float* running_var, float* coef, double* workspace,
                                    pfpp_stream_t stream) {
  RBN_SIZES();
  PFPP_REQUIRE(rows >= 2, "a batch-statistics BatchNorm needs at least 2 rows");
  PFPP_REQUIRE(y && gamma && beta && coef && workspace, "null pointer");
  PFPP_REQUIRE(!running_mean == !running_var, "running_mean and running_var go together");
  PFPP_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "bad eps / momentum");
  PFPP_REQUIRE(pfpp::aligned16(y) && pfpp::aligned16(coef), "16-byte alignment");
  hipStream_t st = pfpp::as_stream(stream);
  int64_t share;
  const int64_t G = share_grid(rows, &share);
  hipLaunchKernelGGL(rbn_partial_kernel, dim3((unsigned)G), dim3(RT_THREADS), 0, st, y, rows, (int)C, ld, share, workspace);
  hipLaunchKernelGGL(rbn_finalise_kernel, dim3(fold_grid(C)), dim3(FO_OUT * FO_SLICES), 0, st, workspace, (int)G, (int)C, (double)rows, gamma,
                     beta, eps, momentum, running_mean, running_var, coef);
  return pfpp::check_launch("pfpp_ragged_bn_stats");
}

extern "C" int pfpp_ragged_bn_apply(const float* y, int64_t rows, int64_t C, int64_t ld, const float* coef, float* out, int64_t ldo,
                                    int64_t pool, int32_t* winner, pfpp_stream_t stream) {
  RBN_SIZES();
  PFPP_REQUIRE(ldo >= C && ldo % 4 == 0 && pool >= 0 && pool <= 1024 && (pool == 0 || rows % pool == 0), "bad sizes (rows % pool != 0?)");
  if (rows == 0) return PFPP_OK;
  PFPP_REQUIRE(y && coef && out, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(y) && pfpp::aligned16(coef) && pfpp::aligned16(out) && (!winner || pfpp::aligned16(winner)), "16-byte alignment");
  const int64_t out_rows = pool > 0 ? rows / pool : rows;
  const int64_t total = out_rows * (C / 4);
  hipLaunchKernelGGL(rbn_apply_kernel, dim3((unsigned)((total + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, pfpp::as_stream(stream), y,
                     out_rows, (int)C, ld, coef, out, ldo, (int)pool, winner);
  return pfpp::check_launch("pfpp_ragged_bn_apply");
}

extern "C" int pfpp_ragged_pool_bwd(const float* y, int64_t groups, int64_t pool, int64_t C, int64_t ld, const float* coef, const float* dout,
                                    int64_t ldd, float* dh, pfpp_stream_t stream) {
  const int64_t rows = groups * pool;
  RBN_SIZES();
  PFPP_REQUIRE(groups >= 0 && pool >= 1 && pool <= 1024 && ldd >= C, "bad sizes");
  if (rows == 0) return PFPP_OK;
  PFPP_REQUIRE(y && coef && dout && dh, "null pointer");
  const int64_t total = groups * C;
  hipLaunchKernelGGL(rbn_pool_bwd_kernel, dim3((unsigned)((total + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, pfpp::as_stream(stream),
                     y, groups, (int)pool, (int)C, ld, coef, dout, ldd, dh);
  return pfpp::check_launch("pfpp_ragged_pool_bwd");
}

extern "C" int pfpp_ragged_bn_relu_bwd(const float* y, const float* dh, int64_t rows, int64_t C, int64_t ld, const float* coef,
                                       const float* gamma, float* dgamma, float* dbeta, float* dy, double* workspace, pfpp_stream_t stream) {
  RBN_SIZES();
  PFPP_REQUIRE(rows >= 1, "no rows");
  PFPP_REQUIRE(y && dh && coef && gamma && dgamma && dbeta && dy && workspace, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(y) && pfpp::aligned16(dh) && pfpp::aligned16(dy), "16-byte alignment");
  hipStream_t st = pfpp::as_stream(stream);
  int64_t share;
  const int64_t G = share_grid(rows, &share);
  float* means = reinterpret_cast<float*>(workspace + (size_t)RT_MAX_WG * 2 * RT_MAX_C);      // behind the partial rows
  hipLaunchKernelGGL(rbn_bwd_partial_kernel, dim3((unsigned)G), dim3(RT_THREADS), 0, st, y, dh, rows, (int)C, ld, share, coef, workspace);
  hipLaunchKernelGGL(rbn_bwd_finalise_kernel, dim3(fold_grid(C)), dim3(FO_OUT * FO_SLICES), 0, st, workspace, (int)G, (int)C, (double)rows,
                     dgamma, dbeta, means);
  const int64_t total = rows * (C / 4);
  int64_t grid = (total + RT_THREADS - 1) / RT_THREADS;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(rbn_bwd_apply_kernel, dim3((unsigned)grid), dim3(RT_THREADS), 0, st, y, dh, rows, (int)C, ld, coef, gamma, means, dy);
  return pfpp::check_launch("pfpp_ragged_bn_relu_bwd");
}

extern "C" int pfpp_ragged_group_bwd(const float* dA, int64_t lda, int64_t D, const int64_t* off, const int32_t* ent, int64_t S, int64_t K,
                                     int64_t pool, int64_t Np, float* dfeats, int64_t ldf, int accumulate, pfpp_stream_t stream) {
  PFPP_REQUIRE(S >= 0 && Np >= 0 && D >= 1 && K >= 1 && pool >= K && lda >= D && ldf >= D, "bad sizes");
  PFPP_SUPPORTED(S * pool < (1ll << 31) && Np < (1ll << 31) && D < (1 << 20), "sizes exceed the kernel's index range");
  if (Np == 0) return PFPP_OK;
  PFPP_REQUIRE((dA || S == 0) && off && (ent || S == 0) && dfeats, "null pointer");
  int64_t grid = (Np + 3) / 4;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(ragged_group_bwd_kernel, dim3((unsigned)grid), dim3(RT_THREADS), 0, pfpp::as_stream(stream), dA, lda, (int)D, off, ent, S * K,
                     (int)K, (int)pool, Np, dfeats, ldf, accumulate);
  return pfpp::check_launch("pfpp_ragged_group_bwd");
}

extern "C" int pfpp_ragged_interp_bwd(const float* dout, int64_t ldo, int64_t D1, int64_t D2, const float* weights, const int64_t* off,
                                      const int32_t* ent, int64_t N, int64_t S, float* dpoints2, double* workspace, pfpp_stream_t stream) {
  PFPP_REQUIRE(N >= 0 && S >= 1 && D1 >= 0 && D2 >= 1 && ldo >= D1 + D2, "bad sizes");
  PFPP_SUPPORTED(N < (1ll << 31) / 3 && S < (1ll << 31) && D2 < (1 << 20), "sizes exceed the kernel's index range");
  PFPP_REQUIRE(dpoints2 && (dout || N == 0), "null pointer");
  hipStream_t st = pfpp::as_stream(stream);
  if (S == 1) {                                              // the reference's broadcast of the one centroid (:191-192)
    PFPP_SUPPORTED(D2 <= RT_MAX_C, "one centroid: at most 1024 channels");
    PFPP_REQUIRE(workspace, "null pointer");
    int64_t share;
    const int64_t G = share_grid(N, &share);
    hipLaunchKernelGGL(rcol_partial_kernel, dim3((unsigned)G), dim3(RT_THREADS), 0, st, dout + D1, N, (int)D2, ldo, share, workspace);
    hipLaunchKernelGGL(rcol_fold_kernel, dim3(fold_grid(D2)), dim3(FO_OUT * FO_SLICES), 0, st, workspace, (int)G, (int)D2, dpoints2);
    return pfpp::check_launch("pfpp_ragged_interp_bwd");
  }
  PFPP_REQUIRE(weights && off && ent, "null pointer");
  int64_t grid = (S + 3) / 4;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(ragged_interp_bwd_kernel, dim3((unsigned)grid), dim3(RT_THREADS), 0, st, dout, ldo, (int)D1, (int)D2, weights, off, ent,
                     3 * N, S, dpoints2);
  return pfpp::check_launch("pfpp_ragged_interp_bwd");
}
