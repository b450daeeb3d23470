// Stage-1 pre-training of the VQ-VAE (vqvae/model/fracture_ae.py, vq_vae.py, pn2.py, quantizer.py): the pieces of the
// training step that the encoder's forward kernels do not already provide.
//
//  * pfpp_chamfer_fwd / pfpp_chamfer_bwd / pfpp_chamfer_reduce — chamferdist.ChamferDistance(r, p, bidirectional=True)
//    (pn2.py:83-97, vq_vae.py:75-89) with its gradient.  The forward is nn_dist_kernel (metrics.hip) with the index of the
//    nearest point kept (strict <, ascending scan: the lowest index wins an exact tie) and the same (dx^2 + dy^2) + dz^2
//    arithmetic, so the distances equal pfpp_nn_dist's bit for bit.  The source cloud may be given as offset + centre
//    (pc_offset + xyz[:, :, None], `rep` offsets per centre).  The backward's reverse term is a scatter (every target
//    adds into its nearest source); it is written as a gather per source point over the target indices, no float atomics.
//  * pfpp_vq_train — the quantizer's loss, perplexity and gradients (quantizer.py:45-67) from the codes pfpp_vq_encode wrote.
//    The codebook gradient is a gather per code (no float atomics).
//  * pfpp_sa_pool_bwd / pfpp_bn_relu_bwd — backward of relu(BatchNorm_train(y)) (and of the max over the neighbourhood that
//    ends a set-abstraction level, pn2_utils.py:210-214) from the saved raw conv output y and the batch statistics.
//  * pfpp_group_gather_bwd — backward of the grouping (pfpp_group_gather): the feature columns of the grouped-row gradient
//    summed per source point, as a gather per point tile (no float atomics).
// Built with the default contraction like bn_train.hip: the BatchNorm affine below is bn_apply_kernel's expressions, so the
// recomputed h = relu(BN(y)) (ReLU masks, the row that attains a neighbourhood's max) is the forward's value bit for bit.  The
// Chamfer distance switches contraction off locally (metrics.hip is built with -ffp-contract=off).
#include "pfpp_common.h"

namespace {

constexpr int CH_TILE = 1024;

__device__ __forceinline__ void src_point(const float* off, const float* ctr, int64_t rep, int64_t b, int64_t n, int64_t i,
                                          float& x, float& y, float& z) {
  const float* o = off + (b * n + i) * 3;
  x = o[0]; y = o[1]; z = o[2];
  if (ctr) {
    const float* c = ctr + (b * (n / rep) + i / rep) * 3;
    x = x + c[0]; y = y + c[1]; z = z + c[2];
  }
}

// nearest neighbour of every point of cloud A in cloud B; A and B are either (source, target) or (target, source)
template <bool A_IS_SRC>
__global__ __launch_bounds__(256) void chamfer_nn_kernel(const float* __restrict__ off, const float* __restrict__ ctr, int64_t rep,
                                                         const float* __restrict__ tgt, int64_t n, int64_t m,
                                                         float* __restrict__ dist, int32_t* __restrict__ idx) {
#pragma clang fp contract(off)
  __shared__ float tx[CH_TILE], ty[CH_TILE], tz[CH_TILE];
  const int64_t b = blockIdx.y;
  const int64_t na = A_IS_SRC ? n : m, nb = A_IS_SRC ? m : n;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = i < na;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (ok) {
    if (A_IS_SRC) {
      src_point(off, ctr, rep, b, n, i, px, py, pz);
    } else {
      const float* t = tgt + (b * m + i) * 3;
      px = t[0]; py = t[1]; pz = t[2];
    }
  }
  float best = __builtin_huge_valf();
  int32_t arg = 0;
  for (int64_t j0 = 0; j0 < nb; j0 += CH_TILE) {
    const int cnt = (int)min((int64_t)CH_TILE, nb - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      if (A_IS_SRC) {
        const float* t = tgt + (b * m + j0 + j) * 3;
        tx[j] = t[0]; ty[j] = t[1]; tz[j] = t[2];
      } else {
        src_point(off, ctr, rep, b, n, j0 + j, tx[j], ty[j], tz[j]);
      }
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) {
      const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
      const float d = (dx * dx + dy * dy) + dz * dz;
      if (d < best) { best = d; arg = (int32_t)(j0 + j); }
    }
  }
  if (ok) {
    dist[b * na + i] = best;
    idx[b * na + i] = arg;
  }
}

// grad[b, i] = s * 2 * [(r_i - p_{nn(i)}) + sum_{j : nn'(j) = i} (r_i - p_j)],  s = scale (* *gscale)
__global__ __launch_bounds__(256) void chamfer_bwd_kernel(const float* __restrict__ off, const float* __restrict__ ctr, int64_t rep,
                                                          const float* __restrict__ tgt, const int32_t* __restrict__ i_src,
                                                          const int32_t* __restrict__ i_tgt, int64_t n, int64_t m, float scale,
                                                          const float* __restrict__ gscale, float* __restrict__ grad) {
  __shared__ float tx[CH_TILE], ty[CH_TILE], tz[CH_TILE];
  __shared__ int32_t ti[CH_TILE];
  const int64_t b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = i < n;
  float rx = 0.0f, ry = 0.0f, rz = 0.0f;
  if (ok) src_point(off, ctr, rep, b, n, i, rx, ry, rz);
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  if (ok) {
    const int64_t j = i_src[b * n + i];
    const float* t = tgt + (b * m + j) * 3;
    gx = rx - t[0]; gy = ry - t[1]; gz = rz - t[2];
  }
  for (int64_t j0 = 0; j0 < m; j0 += CH_TILE) {
    const int cnt = (int)min((int64_t)CH_TILE, m - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const float* t = tgt + (b * m + j0 + j) * 3;
      tx[j] = t[0]; ty[j] = t[1]; tz[j] = t[2];
      ti[j] = i_tgt[b * m + j0 + j];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      if (ti[j] == (int32_t)i) { gx += rx - tx[j]; gy += ry - ty[j]; gz += rz - tz[j]; }
    }
  }
  if (!ok) return;
  const float s = 2.0f * scale * (gscale ? gscale[0] : 1.0f);
  float* g = grad + (b * n + i) * 3;
  g[0] = s * gx; g[1] = s * gy; g[2] = s * gz;
}

// one workgroup: out[0] = scale * (sum a + sum b) with fp64 accumulation in a fixed order (deterministic)
__global__ __launch_bounds__(1024) void sum2_kernel(const float* __restrict__ a, int64_t na, const float* __restrict__ b, int64_t nb,
                                                    float scale, float* __restrict__ out) {
  __shared__ double red[1024];
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < na; k += 1024) s += (double)a[k];
  for (int64_t k = threadIdx.x; k < nb; k += 1024) s += (double)b[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] * (double)scale);
}

// ---------------------------------------------------------------------------------------------------- vector quantizer
// per element: dz = g * 2 (z - e) / n  (the commitment term's gradient reaches z only);  sq[row] = sum_d (e - z)^2
template <int D>
__global__ __launch_bounds__(256) void vq_rows_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                      const int32_t* __restrict__ codes, int64_t R, float inv_n,
                                                      const float* __restrict__ gscale, float* __restrict__ dz, float* __restrict__ sq) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const float* zr = z + r * D;
  const float* e = cb + (int64_t)codes[r] * D;
  const float g = 2.0f * inv_n * (gscale ? gscale[0] : 1.0f);
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float diff = zr[d] - e[d];
    s += diff * diff;
    if (dz) dz[r * D + d] = g * diff;
  }
  sq[r] = s;
}

// one workgroup per code k: dcb[k] = g * 2 beta / n * sum_{codes[r] = k} (e_k - z_r),  cnt[k] = #{r : codes[r] = k}
template <int D>
__global__ __launch_bounds__(256) void vq_code_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                      const int32_t* __restrict__ codes, int64_t R, float coef,
                                                      const float* __restrict__ gscale, float* __restrict__ dcb,
                                                      float* __restrict__ cnt) {
  __shared__ float red[256][D + 1];
  const int k = blockIdx.x;
  float e[D], acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { e[d] = cb[(int64_t)k * D + d]; acc[d] = 0.0f; }
  float c = 0.0f;
  for (int64_t r = threadIdx.x; r < R; r += 256) {
    if (codes[r] != k) continue;
    c += 1.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] += e[d] - z[r * D + d];
  }
#pragma unroll
  for (int d = 0; d < D; ++d) red[threadIdx.x][d] = acc[d];
  red[threadIdx.x][D] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int d = 0; d <= D; ++d) red[threadIdx.x][d] += red[threadIdx.x + h][d];
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < D) {
    if (dcb) dcb[(int64_t)k * D + threadIdx.x] = coef * (gscale ? gscale[0] : 1.0f) * red[0][threadIdx.x];
  } else if ((int)threadIdx.x == D) {
    cnt[k] = red[0][D];
  }
}

// one workgroup: out[0] = (1 + beta) * sum(sq) / n (embedding loss), out[1] = exp(-sum_k p_k log(p_k + 1e-10)), p_k = cnt[k] / R
__global__ __launch_bounds__(1024) void vq_finish_kernel(const float* __restrict__ sq, int64_t R, const float* __restrict__ cnt,
                                                         int64_t K, float beta, float inv_n, float* __restrict__ out) {
  __shared__ double red[2][1024];
  double s = 0.0, h = 0.0;
  for (int64_t r = threadIdx.x; r < R; r += 1024) s += (double)sq[r];
  for (int64_t k = threadIdx.x; k < K; k += 1024) {
    const float p = cnt[k] / (float)R;
    h += (double)(p * logf(p + 1e-10f));
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = h;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)((1.0 + (double)beta) * red[0][0] * (double)inv_n);
    out[1] = expf(-(float)red[1][0]);
  }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm + ReLU backward
// the affine of bn_apply_kernel (bn_train.hip), same expressions: h = relu(y * a + b)
__device__ __forceinline__ void bn_affine(const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                                          int c, float& a, float& b) {
  a = gamma[c] * (1.0f / sqrtf(var[c] + eps));
  b = beta[c] - mean[c] * a;
}

// dh [groups * pool, C]: dout[g, c] at the first row of group g that attains max_p relu(a y_p + b) when that max is > 0, else 0
__global__ __launch_bounds__(256) void sa_pool_bwd_kernel(const float* __restrict__ y, int64_t groups, int pool, int C, int64_t ld,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          const float* __restrict__ dout, float* __restrict__ dh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= groups * C) return;
  const int64_t g = i / C;
  const int c = (int)(i - g * C);
  float a, b;
  bn_affine(mean, var, gamma, beta, eps, c, a, b);
  float best = 0.0f;
  int arg = -1;
  for (int p = 0; p < pool; ++p) {
    const float v = y[(g * pool + p) * ld + c] * a + b;
    if (v > best) { best = v; arg = p; }
  }
  const float d = dout[g * C + c];
  for (int p = 0; p < pool; ++p) dh[(g * pool + p) * (int64_t)C + c] = (p == arg) ? d : 0.0f;
}

constexpr int BSLAB = 2048;

// per slab of rows: fp64 sums of dz and dz * xhat per channel, dz = dh * (relu(a y + b) > 0), xhat = (y - mean) / sqrt(var + eps)
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ y, const float* __restrict__ dh, int64_t rows,
                                                             int C, int64_t ld, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, double* __restrict__ part) {
  extern __shared__ double bwd_red[];      // [RP][2][C]
  const int CL = C / 4;
  const int RP = 256 / CL;
  const int cl = threadIdx.x % CL, rp = threadIdx.x / CL;
  const int64_t r0 = (int64_t)blockIdx.x * BSLAB;
  const int64_t r1 = min(rows, r0 + BSLAB);
  if (rp < RP) {
    float a[4], b[4], m[4], rs[4];
    for (int e = 0; e < 4; ++e) {
      const int c = cl * 4 + e;
      bn_affine(mean, var, gamma, beta, eps, c, a[e], b[e]);
      m[e] = mean[c];
      rs[e] = 1.0f / sqrtf(var[c] + eps);
    }
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    for (int64_t r = r0 + rp; r < r1; r += RP) {
      const float4 yv = *reinterpret_cast<const float4*>(y + r * ld + cl * 4);
      const float4 gv = *reinterpret_cast<const float4*>(dh + r * (int64_t)C + cl * 4);
      const float yy[4] = {yv.x, yv.y, yv.z, yv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dz = (yy[e] * a[e] + b[e] > 0.0f) ? gg[e] : 0.0f;
        s[e] += (double)dz;
        q[e] += (double)dz * (double)((yy[e] - m[e]) * rs[e]);
      }
    }
    double* o = bwd_red + (size_t)rp * 2 * C;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[cl * 4 + e] = s[e]; o[C + cl * 4 + e] = q[e]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    double acc = 0.0;
    for (int p = 0; p < RP; ++p) acc += bwd_red[(size_t)p * 2 * C + i];
    part[(size_t)blockIdx.x * 2 * C + i] = acc;
  }
}

// partials in slab order -> dbeta += sum dz, dgamma += sum dz xhat; coef = (mean dz, mean dz xhat) as fp32 for the second pass
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int n_part, int64_t rows, int C,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ coef, unsigned int* __restrict__ amax) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (amax && c == 0) *amax = 0u;          // cleared here: the apply pass behind this launch takes the max of |dy|
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int p = 0; p < n_part; ++p) {
    s += part[(size_t)p * 2 * C + c];
    q += part[(size_t)p * 2 * C + C + c];
  }
  if (dbeta) dbeta[c] += (float)s;
  if (dgamma) dgamma[c] += (float)q;
  coef[c] = (float)(s / (double)rows);
  coef[C + c] = (float)(q / (double)rows);
}

// dy = gamma / sqrt(var + eps) * (dz - mean dz - xhat * mean(dz xhat)); dy may alias dh (same element read, then written)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ y, const float* dh, int64_t rows, int C, int64_t ld,
                                                           const float* __restrict__ mean, const float* __restrict__ var,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ coef, float* dy, unsigned int* __restrict__ amax) {
  __shared__ unsigned int red[256];
  unsigned int bits = 0u;
  const int64_t total = rows * C;
  // grid-stride: a bounded number of workgroups, so the max below costs one atomic per workgroup, not one per 256 elements
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    float a, b;
    bn_affine(mean, var, gamma, beta, eps, c, a, b);
    const float rs = 1.0f / sqrtf(var[c] + eps);
    const float yv = y[r * ld + c];
    const float dz = (yv * a + b > 0.0f) ? dh[i] : 0.0f;
    const float xh = (yv - mean[c]) * rs;
    const float v = gamma[c] * rs * ((dz - coef[c]) - xh * coef[C + c]);
    dy[i] = v;
    bits = max(bits, __float_as_uint(fabsf(v)));      // non-negative floats order like their bit patterns (NaN above inf)
  }
  if (!amax) return;
  red[threadIdx.x] = bits;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(amax, red[0]);      // integer max of the bit patterns: order-independent, exact
}

// ---------------------------------------------------------------------------------------------------- grouping backward
constexpr int GB_PT = 16;      // source points per workgroup
constexpr int GB_CH = 256;     // slot indices staged per pass

// dfeats[f, p, c] = sum over slots s of fragment f with idx[f, s] = p of dA[f * S*ns + s, c]  (c < D; slot order: deterministic)
__global__ __launch_bounds__(256) void group_gather_bwd_kernel(const float* __restrict__ dA, int64_t lda, const int32_t* __restrict__ idx,
                                                               float* __restrict__ dfeats, int64_t N, int64_t slots, int D) {
  __shared__ int32_t sidx[GB_CH];
  const int64_t f = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * GB_PT;
  float acc[2][GB_PT];
#pragma unroll
  for (int k = 0; k < GB_PT; ++k) { acc[0][k] = 0.0f; acc[1][k] = 0.0f; }
  const int c0 = threadIdx.x, c1 = threadIdx.x + 256;
  const float* base = dA + f * slots * lda;
  for (int64_t s0 = 0; s0 < slots; s0 += GB_CH) {
    const int cnt = (int)min((int64_t)GB_CH, slots - s0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) sidx[threadIdx.x] = idx[f * slots + s0 + threadIdx.x];
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int64_t q = (int64_t)sidx[j] - p0;
      if (q < 0 || q >= GB_PT) continue;
      const float* row = base + (s0 + j) * lda;
      const float v0 = c0 < D ? row[c0] : 0.0f;
      const float v1 = c1 < D ? row[c1] : 0.0f;
#pragma unroll
      for (int k = 0; k < GB_PT; ++k) {
        if (k == (int)q) { acc[0][k] += v0; acc[1][k] += v1; }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < GB_PT; ++k) {
    const int64_t p = p0 + k;
    if (p >= N) break;
    if (c0 < D) dfeats[(f * N + p) * D + c0] = acc[0][k];
    if (c1 < D) dfeats[(f * N + p) * D + c1] = acc[1][k];
  }
}

}  // namespace

extern "C" int pfpp_chamfer_fwd(const float* off, const float* ctr, int64_t rep, const float* tgt, float* d_src, int32_t* i_src,
                                float* d_tgt, int32_t* i_tgt, int64_t batch, int64_t n, int64_t m, pfpp_stream_t stream) {
  PFPP_REQUIRE(off && tgt && d_src && i_src && d_tgt && i_tgt, "null pointer");
  PFPP_REQUIRE(batch >= 0 && n >= 1 && m >= 1, "bad sizes (both clouds must be non-empty)");
  PFPP_REQUIRE(!ctr || (rep >= 1 && n % rep == 0), "n must be a multiple of rep");
  PFPP_SUPPORTED(batch <= 65535 && n < (1ll << 31) && m < (1ll << 31), "more than 65535 clouds or 2^31 points per launch");
  if (batch == 0) return PFPP_OK;
  hipStream_t st = pfpp::as_stream(stream);
  hipLaunchKernelGGL(chamfer_nn_kernel<true>, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, off, ctr, rep,
                     tgt, n, m, d_src, i_src);
  hipLaunchKernelGGL(chamfer_nn_kernel<false>, dim3((unsigned)((m + 255) / 256), (unsigned)batch), dim3(256), 0, st, off, ctr, rep,
                     tgt, n, m, d_tgt, i_tgt);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_chamfer_bwd(const float* off, const float* ctr, int64_t rep, const float* tgt, const int32_t* i_src,
                                const int32_t* i_tgt, float* grad, int64_t batch, int64_t n, int64_t m, float scale,
                                const float* gscale, pfpp_stream_t stream) {
  PFPP_REQUIRE(off && tgt && i_src && i_tgt && grad, "null pointer");
  PFPP_REQUIRE(batch >= 0 && n >= 1 && m >= 1, "bad sizes");
  PFPP_REQUIRE(!ctr || (rep >= 1 && n % rep == 0), "n must be a multiple of rep");
  PFPP_SUPPORTED(batch <= 65535 && n < (1ll << 31) && m < (1ll << 31), "more than 65535 clouds or 2^31 points per launch");
  if (batch == 0) return PFPP_OK;
  hipLaunchKernelGGL(chamfer_bwd_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, pfpp::as_stream(stream),
                     off, ctr, rep, tgt, i_src, i_tgt, n, m, scale, gscale, grad);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_chamfer_reduce(const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, float scale, float* loss,
                                   pfpp_stream_t stream) {
  PFPP_REQUIRE(loss && (d_src || n_src == 0) && (d_tgt || n_tgt == 0), "null pointer");
  PFPP_REQUIRE(n_src >= 0 && n_tgt >= 0, "bad sizes");
  hipLaunchKernelGGL(sum2_kernel, dim3(1), dim3(1024), 0, pfpp::as_stream(stream), d_src, n_src, d_tgt, n_tgt, scale, loss);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_vq_train(const float* z, const float* codebook, const int32_t* codes, int64_t R, int64_t K, int64_t D, float beta,
                             const float* g_emb, float* dz, float* dcodebook, float* out, void* workspace, pfpp_stream_t stream) {
  PFPP_REQUIRE(z && codebook && codes && out && workspace, "null pointer");
  PFPP_REQUIRE(R >= 1 && K >= 1, "bad sizes");
  PFPP_SUPPORTED(D == 16, "code width != 16 (quantizer.py: embedding_dim 16)");
  PFPP_SUPPORTED(K <= 65535, "more than 65535 codes");
  hipStream_t st = pfpp::as_stream(stream);
  float* sq = reinterpret_cast<float*>(workspace);
  float* cnt = sq + R;
  const float inv_n = (float)(1.0 / ((double)R * (double)D));
  hipLaunchKernelGGL(vq_rows_kernel<16>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, z, codebook, codes, R, inv_n, g_emb, dz, sq);
  hipLaunchKernelGGL(vq_code_kernel<16>, dim3((unsigned)K), dim3(256), 0, st, z, codebook, codes, R, 2.0f * beta * inv_n, g_emb,
                     dcodebook, cnt);
  hipLaunchKernelGGL(vq_finish_kernel, dim3(1), dim3(1024), 0, st, sq, R, cnt, K, beta, inv_n, out);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_vq_train_workspace(int64_t R, int64_t K) { return (R + K) * (int64_t)sizeof(float); }

extern "C" int pfpp_sa_pool_bwd(const float* y, int64_t groups, int64_t pool, int64_t C, int64_t ld, const float* mean, const float* var,
                                const float* gamma, const float* beta, float eps, const float* dout, float* dh, pfpp_stream_t stream) {
  PFPP_REQUIRE(y && mean && var && gamma && beta && dout && dh, "null pointer");
  PFPP_REQUIRE(groups >= 0 && pool >= 1 && C >= 1 && ld >= C, "bad sizes");
  const int64_t total = groups * C;
  if (total == 0) return PFPP_OK;
  hipLaunchKernelGGL(sa_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pfpp::as_stream(stream), y, groups,
                     (int)pool, (int)C, ld, mean, var, gamma, beta, eps, dout, dh);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_bn_relu_bwd_workspace(int64_t rows, int64_t C) {
  const int64_t n_part = (rows + BSLAB - 1) / BSLAB;
  return n_part * 2 * C * (int64_t)sizeof(double) + 2 * C * (int64_t)sizeof(float);
}

extern "C" int pfpp_bn_relu_bwd(const float* y, const float* dh, int64_t rows, int64_t C, int64_t ld, const float* mean, const float* var,
                                const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, float* dy, float* amax,
                                void* workspace, pfpp_stream_t stream) {
  PFPP_REQUIRE(y && dh && mean && var && gamma && beta && dy && workspace, "null pointer");
  PFPP_REQUIRE(rows >= 1 && ld >= C && ld % 4 == 0 && pfpp::aligned16(y) && pfpp::aligned16(dh), "bad sizes / alignment");
  PFPP_SUPPORTED(C == 64 || C == 128 || C == 256 || C == 512 || C == 1024, "C not in {64,128,256,512,1024}");
  hipStream_t st = pfpp::as_stream(stream);
  const int n_part = (int)((rows + BSLAB - 1) / BSLAB);
  double* part = reinterpret_cast<double*>(workspace);
  float* coef = reinterpret_cast<float*>(part + (size_t)n_part * 2 * C);
  const int RP = 256 / (int)(C / 4);
  const size_t smem = (size_t)RP * 2 * C * sizeof(double);
  hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)n_part), dim3(256), smem, st, y, dh, rows, (int)C, ld, mean, var, gamma, beta,
                     eps, part);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, (const double*)part, n_part, rows,
                     (int)C, dgamma, dbeta, coef, reinterpret_cast<unsigned int*>(amax));
  const int64_t total = rows * C;
  const int64_t apply_blocks = min((total + 255) / 256, (int64_t)4096);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)apply_blocks), dim3(256), 0, st, y, dh, rows, (int)C, ld, mean, var,
                     gamma, beta, eps, (const float*)coef, dy, reinterpret_cast<unsigned int*>(amax));
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_group_gather_bwd(const float* dA, int64_t lda, const int32_t* idx, float* dfeats, int64_t F, int64_t N, int64_t S,
                                     int64_t ns, int64_t D, pfpp_stream_t stream) {
  PFPP_REQUIRE(dA && idx && dfeats, "null pointer");
  PFPP_REQUIRE(F >= 0 && N >= 1 && S >= 1 && ns >= 1 && D >= 1 && lda >= D, "bad sizes");
  PFPP_SUPPORTED(D <= 512 && F <= 65535, "D > 512 or more than 65535 fragments");
  if (F == 0) return PFPP_OK;
  hipLaunchKernelGGL(group_gather_bwd_kernel, dim3((unsigned)((N + GB_PT - 1) / GB_PT), (unsigned)F), dim3(256), 0,
                     pfpp::as_stream(stream), dA, lda, idx, dfeats, N, S * ns, (int)D);
  return pfpp::check_launch(__func__);
}
