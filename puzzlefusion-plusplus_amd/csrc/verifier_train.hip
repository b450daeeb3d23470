// Training step of the VerifierTransformer (verifier/model/verifier.py:20-69, verifier_transformer.py:8-58 in train mode):
// the kernels the denoiser's training path does not already provide.
//   * masked multi-head attention with dropout on the attention probabilities (nn.MultiheadAttention(dropout=0.1) inside
//     nn.TransformerEncoderLayer), forward with lse and a single-launch backward (dq, dk, dv);
//   * mlp_out + the weighted BCE of Verifier._loss fused, with its backward and the confusion counts;
//   * GELU + dropout of the feed-forward (TransformerEncoderLayer.linear1 -> gelu -> dropout), forward and backward.
// Dropout masks come from the counter-based generator of pfpp_dropout (pfpp_rng_u32) and are regenerated in the backward.
#include <math.h>

#include "pfpp_common.h"

namespace {

constexpr int VA_DH = 32;          // head width (d_model 256 / 8 heads)
constexpr int VA_MAXE = 256;       // tokens per sequence held in LDS
constexpr int VA_THREADS = 256;

__device__ __forceinline__ float dot32(const float* __restrict__ a, const float* __restrict__ b) {
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < VA_DH; c += 4) {
    const float4 x = *reinterpret_cast<const float4*>(a + c);
    const float4 y = *reinterpret_cast<const float4*>(b + c);
    s = fmaf(x.x, y.x, s);
    s = fmaf(x.y, y.y, s);
    s = fmaf(x.z, y.z, s);
    s = fmaf(x.w, y.w, s);
  }
  return s;
}

// keep bit of attention probability (b, h, q, k): counter ((b*H + h)*E + q)*E + k — the layout of the exported [B, H, E, E] mask
__device__ __forceinline__ bool va_keep(uint64_t seed, uint32_t site, uint32_t thresh, int64_t bh, int E, int q, int k) {
  if (thresh == 0u) return true;
  return pfpp_rng_u32(seed, site, ((uint64_t)bh * E + q) * E + k) >= thresh;
}

// copy one head's [E, 32] slice of a [rows, ld] tensor into LDS (float4 per thread)
__device__ __forceinline__ void va_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int E) {
  for (int i = threadIdx.x; i < E * (VA_DH / 4); i += VA_THREADS) {
    const int r = i / (VA_DH / 4), c = (i % (VA_DH / 4)) * 4;
    *reinterpret_cast<float4*>(dst + r * VA_DH + c) = *reinterpret_cast<const float4*>(src + (int64_t)r * ld + c);
  }
}

// One workgroup per (sequence, head); thread q owns query row q.  Online softmax over the valid keys in exact fp32; the dropout
// mask multiplies the probability's contribution to the output only (the normaliser is that of the undropped softmax, as
// F.dropout(softmax(s)) @ v).  A query whose sequence has no valid key writes zeros and lse = +inf (the backward then sees P = 0).
__global__ __launch_bounds__(VA_THREADS) void vattn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                               float* __restrict__ lse, const uint8_t* __restrict__ key_valid,
                                                               int E, int H, float scale, uint32_t thresh, float inv_keep,
                                                               uint64_t seed, uint32_t site) {
  __shared__ __attribute__((aligned(16))) float Ks[VA_MAXE * VA_DH];
  __shared__ __attribute__((aligned(16))) float Vs[VA_MAXE * VA_DH];
  __shared__ uint8_t kv[VA_MAXE];
  const int64_t bh = blockIdx.x;
  const int64_t b = bh / H;
  const int h = (int)(bh % H);
  const int C = H * VA_DH;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + b * E * ld + h * VA_DH;
  va_stage(Ks, base + C, ld, E);
  va_stage(Vs, base + 2 * C, ld, E);
  for (int i = threadIdx.x; i < E; i += VA_THREADS) kv[i] = key_valid[b * E + i];
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= E) return;
  __attribute__((aligned(16))) float qr[VA_DH];
  __attribute__((aligned(16))) float acc[VA_DH];
#pragma unroll
  for (int c = 0; c < VA_DH; c += 4) {
    *reinterpret_cast<float4*>(qr + c) = *reinterpret_cast<const float4*>(base + q * ld + c);
    acc[c] = acc[c + 1] = acc[c + 2] = acc[c + 3] = 0.0f;
  }
  float m = -INFINITY, l = 0.0f;
  for (int k = 0; k < E; ++k) {
    if (!kv[k]) continue;                       // the same k for every lane: no divergence
    const float s = dot32(qr, Ks + k * VA_DH) * scale;
    if (s > m) {
      const float corr = expf(m - s);           // m = -inf on the first valid key: corr = 0
      l *= corr;
#pragma unroll
      for (int c = 0; c < VA_DH; ++c) acc[c] *= corr;
      m = s;
    }
    const float e = expf(s - m);
    l += e;
    if (va_keep(seed, site, thresh, bh, E, q, k)) {
      const float* v = Vs + k * VA_DH;
#pragma unroll
      for (int c = 0; c < VA_DH; ++c) acc[c] = fmaf(e, v[c], acc[c]);
    }
  }
  float* o = out + (b * E + q) * (int64_t)C + h * VA_DH;
  const float f = l > 0.0f ? inv_keep / l : 0.0f;
#pragma unroll
  for (int c = 0; c < VA_DH; c += 4)
    *reinterpret_cast<float4*>(o + c) = make_float4(acc[c] * f, acc[c + 1] * f, acc[c + 2] * f, acc[c + 3] * f);
  lse[(b * E + q) * H + h] = l > 0.0f ? m + logf(l) : INFINITY;
}

// Single-launch backward, one workgroup per (sequence, head) with q, k, v and dO of the head in LDS (4 x E x 32 x 4 B).
// With P = softmax(s), Pd = P * keep / (1 - p), O = Pd v:
//   dv_j = sum_i Pd_ij dO_i ;  dPd_ij = dO_i . v_j ;  dP_ij = dPd_ij keep / (1 - p) ;  dS_ij = P_ij (dP_ij - D_i)
//   D_i = sum_j P_ij dP_ij = sum_j Pd_ij dPd_ij = dO_i . O_i ;  dq_i = scale sum_j dS_ij k_j ;  dk_j = scale sum_i dS_ij q_i
// Thread t computes dq of query t (loop over keys) and then dk, dv of key t (loop over queries): no atomics, no second pass.
__global__ __launch_bounds__(VA_THREADS) void vattn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                               const float* __restrict__ dout, const float* __restrict__ lse,
                                                               float* __restrict__ dqkv, const uint8_t* __restrict__ key_valid,
                                                               int E, int H, float scale, uint32_t thresh, float inv_keep,
                                                               uint64_t seed, uint32_t site) {
  extern __shared__ __attribute__((aligned(16))) float va_smem[];
  float* Qs = va_smem;
  float* Ks = Qs + E * VA_DH;
  float* Vs = Ks + E * VA_DH;
  float* Gs = Vs + E * VA_DH;                  // dO
  float* Ls = Gs + E * VA_DH;                  // lse
  float* Ds = Ls + E;                          // D = rowsum(dO * O)
  uint8_t* kv = reinterpret_cast<uint8_t*>(Ds + E);
  const int64_t bh = blockIdx.x;
  const int64_t b = bh / H;
  const int h = (int)(bh % H);
  const int C = H * VA_DH;
  const int64_t ld = 3 * (int64_t)C;
  const float* base = qkv + b * E * ld + h * VA_DH;
  va_stage(Qs, base, ld, E);
  va_stage(Ks, base + C, ld, E);
  va_stage(Vs, base + 2 * C, ld, E);
  va_stage(Gs, dout + b * E * C + h * VA_DH, C, E);
  for (int i = threadIdx.x; i < E; i += VA_THREADS) {
    kv[i] = key_valid[b * E + i];
    Ls[i] = lse[(b * E + i) * H + h];
    const float* o = out + (b * E + i) * (int64_t)C + h * VA_DH;
    const float* g = dout + (b * E + i) * (int64_t)C + h * VA_DH;
    Ds[i] = dot32(o, g);
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= E) return;
  float* dst = dqkv + (b * E + t) * ld + h * VA_DH;
  __attribute__((aligned(16))) float x[VA_DH];
  __attribute__((aligned(16))) float y[VA_DH];
  __attribute__((aligned(16))) float a0[VA_DH];
  __attribute__((aligned(16))) float a1[VA_DH];

  // ---- dq of query t
  {
    const float lse_t = Ls[t], d_t = Ds[t];
#pragma unroll
    for (int c = 0; c < VA_DH; ++c) {
      x[c] = Qs[t * VA_DH + c];
      y[c] = Gs[t * VA_DH + c];
      a0[c] = 0.0f;
    }
    for (int k = 0; k < E; ++k) {
      if (!kv[k]) continue;
      const float P = expf(dot32(x, Ks + k * VA_DH) * scale - lse_t);
      const float dP = va_keep(seed, site, thresh, bh, E, t, k) ? dot32(y, Vs + k * VA_DH) * inv_keep : 0.0f;
      const float dS = P * (dP - d_t);
      const float* kr = Ks + k * VA_DH;
#pragma unroll
      for (int c = 0; c < VA_DH; ++c) a0[c] = fmaf(dS, kr[c], a0[c]);
    }
#pragma unroll
    for (int c = 0; c < VA_DH; c += 4)
      *reinterpret_cast<float4*>(dst + c) = make_float4(a0[c] * scale, a0[c + 1] * scale, a0[c + 2] * scale, a0[c + 3] * scale);
  }
  // ---- dk, dv of key t (zero for a masked key)
#pragma unroll
  for (int c = 0; c < VA_DH; ++c) {
    x[c] = Ks[t * VA_DH + c];
    y[c] = Vs[t * VA_DH + c];
    a0[c] = 0.0f;
    a1[c] = 0.0f;
  }
  if (kv[t]) {
    for (int q = 0; q < E; ++q) {
      const float P = expf(dot32(Qs + q * VA_DH, x) * scale - Ls[q]);
      const float* g = Gs + q * VA_DH;
      float dP = 0.0f;
      if (va_keep(seed, site, thresh, bh, E, q, t)) {
        const float Pd = P * inv_keep;
#pragma unroll
        for (int c = 0; c < VA_DH; ++c) a1[c] = fmaf(Pd, g[c], a1[c]);
        dP = dot32(g, y) * inv_keep;
      }
      const float dS = P * (dP - Ds[q]);
      const float* qr = Qs + q * VA_DH;
#pragma unroll
      for (int c = 0; c < VA_DH; ++c) a0[c] = fmaf(dS, qr[c], a0[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < VA_DH; c += 4) {
    *reinterpret_cast<float4*>(dst + C + c) = make_float4(a0[c] * scale, a0[c + 1] * scale, a0[c + 2] * scale, a0[c + 3] * scale);
    *reinterpret_cast<float4*>(dst + 2 * C + c) = make_float4(a1[c], a1[c + 1], a1[c + 2], a1[c + 3]);
  }
}

__global__ void vattn_mask_kernel(uint8_t* __restrict__ keep, int64_t n, uint32_t thresh, uint64_t seed, uint32_t site) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keep[i] = (thresh == 0u || pfpp_rng_u32(seed, site, (uint64_t)i) >= thresh) ? 1 : 0;
}

// ---- head + weighted BCE ---------------------------------------------------------------------------------------------------
constexpr int VH_C = 256;          // d_model: one float4 per lane covers a row
constexpr int VH_WAVES = 4;
constexpr int VH_WS = 4 + VH_C + 1;   // doubles of the workspace (see pfpp.h)
__device__ __forceinline__ bool target_mode(const float* y, const float* dlogit_in) { return y != nullptr && dlogit_in == nullptr; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One pass over h6: logit, loss term, dlogit, dh6 row, dw_out / db_out partials, confusion counts.  N (valid rows) is counted by
// every workgroup from the flags (M bytes), so no second launch is needed; the last workgroup to finish turns the fp64 workspace
// into loss / amax / counts / gradient sums and clears it again (the workspace is zero between calls).
__global__ __launch_bounds__(VH_WAVES * 64) void vhead_bce_kernel(const float* __restrict__ h6, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, const float* __restrict__ y,
                                                                  const uint8_t* __restrict__ valid, const float* __restrict__ dlogit_in,
                                                                  int64_t M, float neg_weight,
                                                                  float* __restrict__ logits, float* __restrict__ dlogit,
                                                                  float* __restrict__ dh, float* __restrict__ dw, float* __restrict__ db,
                                                                  float* __restrict__ loss, int32_t* __restrict__ stats,
                                                                  float* __restrict__ amax, double* __restrict__ ws) {
  __shared__ int s_cnt[VH_WAVES];
  __shared__ double s_loss[VH_WAVES];
  __shared__ double s_db[VH_WAVES];
  __shared__ int s_st[VH_WAVES][4];
  __shared__ float s_amax[VH_WAVES];
  __shared__ __attribute__((aligned(16))) float s_dw[VH_WAVES][VH_C];
  __shared__ bool s_last;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // N = number of valid rows
  const bool bce = target_mode(y, dlogit_in);
  int cnt = 0;
  if (bce)
    for (int64_t i = threadIdx.x; i < M; i += blockDim.x) cnt += valid[i] != 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) s_cnt[wv] = cnt;
  __syncthreads();
  int N = 0;
#pragma unroll
  for (int i = 0; i < VH_WAVES; ++i) N += s_cnt[i];
  const float invN = N > 0 ? 1.0f / (float)N : 0.0f;
  const float4 wr = *reinterpret_cast<const float4*>(w + lane * 4);
  const float b0 = bias[0];
  float4 dwp = make_float4(0.f, 0.f, 0.f, 0.f);
  double lsum = 0.0, dbsum = 0.0;
  int tp = 0, fp = 0, tn = 0, fn = 0;
  float am = 0.0f;
  for (int64_t r = (int64_t)blockIdx.x * VH_WAVES + wv; r < M; r += (int64_t)gridDim.x * VH_WAVES) {
    const float4 x = *reinterpret_cast<const float4*>(h6 + r * VH_C + lane * 4);
    float s = x.x * wr.x;
    s = fmaf(x.y, wr.y, s);
    s = fmaf(x.z, wr.z, s);
    s = fmaf(x.w, wr.w, s);
    const float z = wave_sum(s) + b0;
    float d = 0.0f;
    if (dlogit_in) {
      d = dlogit_in[r];
      if (lane == 0) {
        dbsum += (double)d;
        am = fmaxf(am, fabsf(d));
      }
      dwp.x = fmaf(d, x.x, dwp.x);
      dwp.y = fmaf(d, x.y, dwp.y);
      dwp.z = fmaf(d, x.z, dwp.z);
      dwp.w = fmaf(d, x.w, dwp.w);
    } else if (bce && valid[r]) {
      const float t = y[r];
      const float wt = t == 0.0f ? neg_weight : 1.0f;
      const float sig = 1.0f / (1.0f + expf(-z));           // torch.sigmoid's fp32 formula
      const bool pred = sig > 0.5f, pos = t > 0.5f;
      d = wt * (sig - t) * invN;
      if (lane == 0) {
        lsum += (double)(wt * (fmaxf(z, 0.0f) - z * t + log1pf(expf(-fabsf(z)))));
        dbsum += (double)d;
        tp += pred && pos;
        fp += pred && !pos;
        tn += !pred && !pos;
        fn += !pred && pos;
        am = fmaxf(am, fabsf(d));
      }
      dwp.x = fmaf(d, x.x, dwp.x);
      dwp.y = fmaf(d, x.y, dwp.y);
      dwp.z = fmaf(d, x.z, dwp.z);
      dwp.w = fmaf(d, x.w, dwp.w);
    }
    if (lane == 0) {
      logits[r] = z;
      if (dlogit) dlogit[r] = d;
    }
    if (dh) *reinterpret_cast<float4*>(dh + r * VH_C + lane * 4) = make_float4(d * wr.x, d * wr.y, d * wr.z, d * wr.w);
  }
  *reinterpret_cast<float4*>(&s_dw[wv][lane * 4]) = dwp;
  if (lane == 0) {
    s_loss[wv] = lsum;
    s_db[wv] = dbsum;
    s_st[wv][0] = tp; s_st[wv][1] = fp; s_st[wv][2] = tn; s_st[wv][3] = fn;
    s_amax[wv] = am;
  }
  __syncthreads();
  uint32_t* wsu = reinterpret_cast<uint32_t*>(ws);
  int32_t* wsi = reinterpret_cast<int32_t*>(ws);
  if (threadIdx.x < VH_C) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < VH_WAVES; ++i) v += (double)s_dw[i][threadIdx.x];
    if (v != 0.0) atomicAdd(ws + 4 + threadIdx.x, v);
  }
  if (threadIdx.x == 0) {
    double lv = 0.0, dv = 0.0;
    int st[4] = {0, 0, 0, 0};
    float a = 0.0f;
    for (int i = 0; i < VH_WAVES; ++i) {
      lv += s_loss[i];
      dv += s_db[i];
      for (int j = 0; j < 4; ++j) st[j] += s_st[i][j];
      a = fmaxf(a, s_amax[i]);
    }
    if (lv != 0.0) atomicAdd(ws + 0, lv);
    if (dv != 0.0) atomicAdd(ws + 4 + VH_C, dv);
    for (int j = 0; j < 4; ++j)
      if (st[j]) atomicAdd(wsi + 4 + j, st[j]);              // ws[2], ws[3]: four int32 counts
    atomicMax(wsu + 3, __float_as_uint(a));                  // non-negative floats order like their bit patterns
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(wsu + 2, 1u) == gridDim.x - 1;   // ws[1].lo: arrival counter
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  volatile double* vws = ws;
  volatile int32_t* vwsi = wsi;
  if (threadIdx.x < VH_C) {
    dw[threadIdx.x] += (float)vws[4 + threadIdx.x];
    vws[4 + threadIdx.x] = 0.0;
  }
  if (threadIdx.x == 0) {
    loss[0] = N > 0 ? (float)(vws[0] / (double)N) : 0.0f;
    db[0] += (float)vws[4 + VH_C];
    for (int j = 0; j < 4; ++j) stats[j] = vwsi[4 + j];
    if (amax) amax[0] = __uint_as_float(((volatile uint32_t*)wsu)[3]);
    vws[0] = 0.0;
    vws[1] = 0.0;
    vws[2] = 0.0;
    vws[3] = 0.0;
    vws[4 + VH_C] = 0.0;
  }
}

// ---- GELU (exact erf form, TransformerEncoderLayer activation='gelu') + dropout ------------------------------------------------
__device__ __forceinline__ float gelu_erf(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_erf_grad(float z) {
  return 0.5f * (1.0f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
}

template <bool BWD>
__global__ void vgelu_drop_kernel(const float* __restrict__ z, const float* __restrict__ du, float* __restrict__ out, int64_t n4,
                                  uint32_t thresh, float inv_keep, uint64_t seed, uint32_t site) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 zv = reinterpret_cast<const float4*>(z)[i];
    float4 g = BWD ? reinterpret_cast<const float4*>(du)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
    float r[4] = {zv.x, zv.y, zv.z, zv.w};
    const float gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool keep = thresh == 0u || pfpp_rng_u32(seed, site, (uint64_t)(4 * i + j)) >= thresh;
      r[j] = keep ? (BWD ? gelu_erf_grad(r[j]) * gg[j] : gelu_erf(r[j])) * inv_keep : 0.0f;
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(r[0], r[1], r[2], r[3]);
  }
}

int grid_for(int64_t n, int per_block) {
  int64_t g = (n + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

size_t vattn_bwd_lds(int64_t E) { return (size_t)E * (4 * VA_DH + 2) * sizeof(float) + (size_t)E; }

}  // namespace

extern "C" int pfpp_verifier_attn_fwd(const float* qkv, float* out, float* lse, const uint8_t* key_valid, int64_t B, int64_t E,
                                      int64_t H, int64_t dh, float scale, float p, uint64_t seed, uint32_t site,
                                      pfpp_stream_t stream) {
  PFPP_REQUIRE(qkv && out && lse && key_valid, "null pointer");
  PFPP_REQUIRE(p >= 0.0f && p < 1.0f, "p outside [0, 1)");
  PFPP_REQUIRE(pfpp::aligned16(qkv) && pfpp::aligned16(out), "16-byte alignment");
  PFPP_SUPPORTED(dh == VA_DH && H >= 1 && H <= 64, "head width 32");
  PFPP_SUPPORTED(E >= 1 && E <= VA_MAXE, "1 <= E <= 256 tokens per sequence");
  if (B == 0) return PFPP_OK;
  hipLaunchKernelGGL(vattn_fwd_kernel, dim3((unsigned)(B * H)), dim3(VA_THREADS), 0, pfpp::as_stream(stream), qkv, out, lse,
                     key_valid, (int)E, (int)H, scale, pfpp_drop_thresh(p), 1.0f / (1.0f - p), seed, site);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_verifier_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                      const uint8_t* key_valid, int64_t B, int64_t E, int64_t H, int64_t dh, float scale, float p,
                                      uint64_t seed, uint32_t site, pfpp_stream_t stream) {
  PFPP_REQUIRE(qkv && out && dout && lse && dqkv && key_valid, "null pointer");
  PFPP_REQUIRE(p >= 0.0f && p < 1.0f, "p outside [0, 1)");
  PFPP_REQUIRE(pfpp::aligned16(qkv) && pfpp::aligned16(out) && pfpp::aligned16(dout) && pfpp::aligned16(dqkv), "16-byte alignment");
  PFPP_SUPPORTED(dh == VA_DH && H >= 1 && H <= 64, "head width 32");
  PFPP_SUPPORTED(E >= 1 && E <= VA_MAXE, "1 <= E <= 256 tokens per sequence");
  if (B == 0) return PFPP_OK;
  const size_t lds = vattn_bwd_lds(E);
  if (pfpp_allow_dyn_lds<vattn_bwd_kernel>((int)vattn_bwd_lds(VA_MAXE)) != hipSuccess) {
    pfpp::set_error("%s: hipFuncSetAttribute failed", __func__);
    return PFPP_EHIP;
  }
  hipLaunchKernelGGL(vattn_bwd_kernel, dim3((unsigned)(B * H)), dim3(VA_THREADS), lds, pfpp::as_stream(stream), qkv, out, dout, lse,
                     dqkv, key_valid, (int)E, (int)H, scale, pfpp_drop_thresh(p), 1.0f / (1.0f - p), seed, site);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_verifier_attn_dropout_mask(uint8_t* keep, int64_t B, int64_t H, int64_t E, float p, uint64_t seed, uint32_t site,
                                               pfpp_stream_t stream) {
  PFPP_REQUIRE(keep, "null pointer");
  PFPP_REQUIRE(p >= 0.0f && p < 1.0f, "p outside [0, 1)");
  PFPP_SUPPORTED(E >= 1 && E <= VA_MAXE, "1 <= E <= 256 tokens per sequence");
  const int64_t n = B * H * E * E;
  if (n == 0) return PFPP_OK;
  hipLaunchKernelGGL(vattn_mask_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, pfpp::as_stream(stream), keep, n,
                     pfpp_drop_thresh(p), seed, site);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_verifier_head_bce(const float* h6, const float* w, const float* b, const float* target, const uint8_t* valid,
                                      const float* dlogit_in, int64_t M, int64_t C, float neg_weight, float* logits, float* dlogit,
                                      float* dh6, float* dw, float* db, float* loss, int32_t* stats, float* amax, double* workspace,
                                      pfpp_stream_t stream) {
  PFPP_REQUIRE(h6 && w && b && logits && dw && db && loss && stats && workspace, "null pointer");
  PFPP_REQUIRE(!target || dlogit_in || valid, "target needs valid flags");
  PFPP_REQUIRE(pfpp::aligned16(h6) && pfpp::aligned16(w) && pfpp::aligned16(dh6) && pfpp::aligned16(workspace), "16-byte alignment");
  PFPP_SUPPORTED(C == VH_C, "d_model 256");
  PFPP_REQUIRE(M >= 0, "M < 0");
  int g = (int)((M + 8 * VH_WAVES - 1) / (8 * VH_WAVES));
  g = g < 1 ? 1 : (g > 160 ? 160 : g);
  hipLaunchKernelGGL(vhead_bce_kernel, dim3(g), dim3(VH_WAVES * 64), 0, pfpp::as_stream(stream), h6, w, b, target, valid, dlogit_in, M, neg_weight,
                     logits, dlogit, dh6, dw, db, loss, stats, amax, workspace);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_verifier_head_bce_workspace(void) { return VH_WS; }

extern "C" int pfpp_verifier_gelu_dropout(const float* z, float* u, int64_t n, float p, uint64_t seed, uint32_t site,
                                          pfpp_stream_t stream) {
  PFPP_REQUIRE(z && u, "null pointer");
  PFPP_REQUIRE(p >= 0.0f && p < 1.0f, "p outside [0, 1)");
  PFPP_REQUIRE(n % 4 == 0 && pfpp::aligned16(z) && pfpp::aligned16(u), "n % 4 != 0 or alignment");
  if (n == 0) return PFPP_OK;
  hipLaunchKernelGGL(vgelu_drop_kernel<false>, dim3(grid_for(n / 4, 256)), dim3(256), 0, pfpp::as_stream(stream), z, nullptr, u, n / 4,
                     pfpp_drop_thresh(p), 1.0f / (1.0f - p), seed, site);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_verifier_gelu_dropout_bwd(const float* z, const float* du, float* dz, int64_t n, float p, uint64_t seed,
                                              uint32_t site, pfpp_stream_t stream) {
  PFPP_REQUIRE(z && du && dz, "null pointer");
  PFPP_REQUIRE(p >= 0.0f && p < 1.0f, "p outside [0, 1)");
  PFPP_REQUIRE(n % 4 == 0 && pfpp::aligned16(z) && pfpp::aligned16(du) && pfpp::aligned16(dz), "n % 4 != 0 or alignment");
  if (n == 0) return PFPP_OK;
  hipLaunchKernelGGL(vgelu_drop_kernel<true>, dim3(grid_for(n / 4, 256)), dim3(256), 0, pfpp::as_stream(stream), z, du, dz, n / 4,
                     pfpp_drop_thresh(p), 1.0f / (1.0f - p), seed, site);
  return pfpp::check_launch(__func__);
}
