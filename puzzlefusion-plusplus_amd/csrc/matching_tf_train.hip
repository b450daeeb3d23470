// Training of the matcher's cross-attention layer tf_cross1 (Jigsaw_matching/model/jigsaw/attention_layer.py:17-24, 47-75, 88-97 under
// autograd): what its backward needs beside the GEMMs.
//
//  * attn_rows16_kernel<.., true> (csrc/attn_rows16.h) — the forward of pfpp_attn_rows16 with one more store, lse = m + log(l) of the
//    scaled scores per (row, head).
//  * attn16_dq_kernel — one query per lane (two in the 256-thread form): q scale, dout, dq, D = dout . out and lse in registers, key /
//    value tiles of 64 staged through LDS and read as broadcasts.  Per key: s as the forward forms it, p = exp(s - lse), dp = dout . v,
//    ds = p (dp - D), dq += ds k; dq scale is stored.  D goes to the workspace for the second pass.
//  * attn16_dkv_kernel — one key per lane (two in the 256-thread form): k, v, dk, dv in registers, tiles of 64 queries (q scale, dout,
//    lse, D) staged through LDS and read as broadcasts.  Per query: dv += p dout, dk += ds (q scale).
//    Neither pass has a cross-lane step or an atomic: a (row, head) of dq | dk | dv is summed by one lane in row order, two runs agree
//    bitwise, a sequence reads and writes its own rows only.  The grid form follows the forward's size rule.
//  * layernorm128_bwd_kernel / layernorm128_fold_kernel — backward of layernorm128_kernel from the row before the normalisation (mean
//    and rstd recomputed with the forward's arithmetic); dgamma / dbeta through per-wave partials, folded in fp64 in a fixed order.
//  * relu_bwd_kernel — dh = h > 0 ? dh : 0 in place.
// This unit is compiled without contraction; fused operations are written as fmaf.
#include "pfpp_common.h"
#include "attn_rows16.h"

namespace {

constexpr int TF_C = 128;

// ------------------------------------------------------------------------------------------------ attention backward, dq
template <int QPL, int THREADS>
__global__ __launch_bounds__(THREADS) void attn16_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                            float* __restrict__ dvec, float* __restrict__ dqkv,
                                                            const int32_t* __restrict__ seq_off, const int32_t* __restrict__ seq_len, int H,
                                                            float scale) {
  __shared__ __attribute__((aligned(16))) float s_k[AT_TK][AT_DH];
  __shared__ __attribute__((aligned(16))) float s_v[AT_TK][AT_DH];
  const int tid = threadIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int len = seq_len[s];
  const int q_base = blockIdx.x * (THREADS * QPL);
  if (q_base >= len) return;                                 // workgroup-uniform
  const int64_t row0 = seq_off[s];
  const int64_t ldq = 3 * (int64_t)H * AT_DH, ldo = (int64_t)H * AT_DH;
  const float* kbase = qkv + row0 * ldq + (int64_t)(H + h) * AT_DH;
  const float* vbase = qkv + row0 * ldq + (int64_t)(2 * H + h) * AT_DH;
  float q[QPL][AT_DH], g[QPL][AT_DH], dq[QPL][AT_DH], dd[QPL], ls[QPL];
  bool q_ok[QPL];
  int q_row[QPL];
#pragma unroll
  for (int u = 0; u < QPL; ++u) {
    const int qi = q_base + u * THREADS + tid;
    q_ok[u] = qi < len;
    q_row[u] = q_ok[u] ? qi : len - 1;
    const int64_t r = row0 + q_row[u];
    const float4* src = reinterpret_cast<const float4*>(qkv + r * ldq + (int64_t)h * AT_DH);
    const float4* gsrc = reinterpret_cast<const float4*>(dout + r * ldo + (int64_t)h * AT_DH);
    const float4* osrc = reinterpret_cast<const float4*>(out + r * ldo + (int64_t)h * AT_DH);
    float d = 0.0f;
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i) {
      const float4 v = src[i], gv = gsrc[i], ov = osrc[i];
      q[u][4 * i] = v.x * scale; q[u][4 * i + 1] = v.y * scale; q[u][4 * i + 2] = v.z * scale; q[u][4 * i + 3] = v.w * scale;
      g[u][4 * i] = gv.x; g[u][4 * i + 1] = gv.y; g[u][4 * i + 2] = gv.z; g[u][4 * i + 3] = gv.w;
      d = fmaf(gv.x, ov.x, d); d = fmaf(gv.y, ov.y, d); d = fmaf(gv.z, ov.z, d); d = fmaf(gv.w, ov.w, d);
    }
#pragma unroll
    for (int i = 0; i < AT_DH; ++i) dq[u][i] = 0.0f;
    dd[u] = d;
    ls[u] = lse[r * H + h];
    if (q_ok[u]) dvec[r * H + h] = d;                        // the dk / dv pass reads it
  }
  constexpr int NP = AT_TK * 4 / THREADS;                    // (key, part) pairs per thread, one tile ahead as in the forward
  float4 kreg[NP], vreg[NP];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = i * THREADS + tid, key = e >> 2, part = e & 3;
      kreg[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      vreg[i] = kreg[i];
      if (k0 + key < len) {
        kreg[i] = reinterpret_cast<const float4*>(kbase + (int64_t)(k0 + key) * ldq)[part];
        vreg[i] = reinterpret_cast<const float4*>(vbase + (int64_t)(k0 + key) * ldq)[part];
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < len; k0 += AT_TK) {
    const int kn = min(AT_TK, len - k0);
    __syncthreads();                                         // the previous tile has been read
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = i * THREADS + tid, key = e >> 2, part = e & 3;
      reinterpret_cast<float4*>(&s_k[key][0])[part] = kreg[i];
      reinterpret_cast<float4*>(&s_v[key][0])[part] = vreg[i];
    }
    __syncthreads();
    if (k0 + AT_TK < len) fetch(k0 + AT_TK);
#pragma unroll 2
    for (int j = 0; j < kn; ++j) {                           // keys of the sequence only: kn is workgroup-uniform
      float kr[AT_DH], vr[AT_DH];
#pragma unroll
      for (int i = 0; i < AT_DH / 4; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(&s_k[j][4 * i]), b = *reinterpret_cast<const float4*>(&s_v[j][4 * i]);
        kr[4 * i] = a.x; kr[4 * i + 1] = a.y; kr[4 * i + 2] = a.z; kr[4 * i + 3] = a.w;
        vr[4 * i] = b.x; vr[4 * i + 1] = b.y; vr[4 * i + 2] = b.z; vr[4 * i + 3] = b.w;
      }
#pragma unroll
      for (int u = 0; u < QPL; ++u) {
        float a = 0.0f, dp = 0.0f;
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) a = fmaf(q[u][i], kr[i], a);       // the forward's score, bit for bit
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) dp = fmaf(g[u][i], vr[i], dp);
        const float ds = __expf(a - ls[u]) * (dp - dd[u]);
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) dq[u][i] = fmaf(ds, kr[i], dq[u][i]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < QPL; ++u) {
    if (!q_ok[u]) continue;
    float4* dst = reinterpret_cast<float4*>(dqkv + (row0 + q_row[u]) * ldq + (int64_t)h * AT_DH);
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i)
      dst[i] = make_float4(dq[u][4 * i] * scale, dq[u][4 * i + 1] * scale, dq[u][4 * i + 2] * scale, dq[u][4 * i + 3] * scale);
  }
}

// ------------------------------------------------------------------------------------------------ attention backward, dk | dv
constexpr int DKV_LD = 2 * AT_DH + 4;                        // floats per staged query: q scale [16] | dout [16] | lse, D, -, -

template <int KPL, int THREADS>
__global__ __launch_bounds__(THREADS) void attn16_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                             const float* __restrict__ lse, const float* __restrict__ dvec,
                                                             float* __restrict__ dqkv, const int32_t* __restrict__ seq_off,
                                                             const int32_t* __restrict__ seq_len, int H, float scale) {
  __shared__ __attribute__((aligned(16))) float s_q[AT_TK][DKV_LD];
  const int tid = threadIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int len = seq_len[s];
  const int k_base = blockIdx.x * (THREADS * KPL);
  if (k_base >= len) return;                                 // workgroup-uniform
  const int64_t row0 = seq_off[s];
  const int64_t ldq = 3 * (int64_t)H * AT_DH, ldo = (int64_t)H * AT_DH;
  const float* qbase = qkv + row0 * ldq + (int64_t)h * AT_DH;
  const float* gbase = dout + row0 * ldo + (int64_t)h * AT_DH;
  float k[KPL][AT_DH], v[KPL][AT_DH], dk[KPL][AT_DH], dv[KPL][AT_DH];
  bool k_ok[KPL];
  int k_row[KPL];
#pragma unroll
  for (int u = 0; u < KPL; ++u) {
    const int ki = k_base + u * THREADS + tid;
    k_ok[u] = ki < len;
    k_row[u] = k_ok[u] ? ki : len - 1;
    const float4* ks = reinterpret_cast<const float4*>(qkv + (row0 + k_row[u]) * ldq + (int64_t)(H + h) * AT_DH);
    const float4* vs = reinterpret_cast<const float4*>(qkv + (row0 + k_row[u]) * ldq + (int64_t)(2 * H + h) * AT_DH);
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i) {
      const float4 a = ks[i], b = vs[i];
      k[u][4 * i] = a.x; k[u][4 * i + 1] = a.y; k[u][4 * i + 2] = a.z; k[u][4 * i + 3] = a.w;
      v[u][4 * i] = b.x; v[u][4 * i + 1] = b.y; v[u][4 * i + 2] = b.z; v[u][4 * i + 3] = b.w;
    }
#pragma unroll
    for (int i = 0; i < AT_DH; ++i) { dk[u][i] = 0.0f; dv[u][i] = 0.0f; }
  }
  // a tile of 64 queries x (4 + 4) float4 and their two scalars, one tile ahead of its use as in the forward
  constexpr int NP = AT_TK * 4 / THREADS;
  float4 qreg[NP], greg[NP];
  float sreg = 0.0f;                                         // threads 0 .. 63: lse of query tid; 64 .. 127 (or a second turn): D
  constexpr int NS = THREADS >= 2 * AT_TK ? 1 : 2;
  float sreg2 = 0.0f;
  auto fetch = [&](int q0) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = i * THREADS + tid, qi = e >> 2, part = e & 3;
      qreg[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      greg[i] = qreg[i];
      if (q0 + qi < len) {
        qreg[i] = reinterpret_cast<const float4*>(qbase + (int64_t)(q0 + qi) * ldq)[part];
        greg[i] = reinterpret_cast<const float4*>(gbase + (int64_t)(q0 + qi) * ldo)[part];
      }
    }
    if (NS == 1) {
      const int qi = tid & (AT_TK - 1);
      sreg = 0.0f;
      if (tid < 2 * AT_TK && q0 + qi < len) sreg = (tid < AT_TK ? lse : dvec)[(row0 + q0 + qi) * H + h];
    } else {
      sreg = 0.0f; sreg2 = 0.0f;
      if (q0 + tid < len) { sreg = lse[(row0 + q0 + tid) * H + h]; sreg2 = dvec[(row0 + q0 + tid) * H + h]; }
    }
  };
  fetch(0);
  for (int q0 = 0; q0 < len; q0 += AT_TK) {
    const int qn = min(AT_TK, len - q0);
    __syncthreads();                                         // the previous tile has been read
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int e = i * THREADS + tid, qi = e >> 2, part = e & 3;
      const float4 a = qreg[i];
      reinterpret_cast<float4*>(&s_q[qi][0])[part] = make_float4(a.x * scale, a.y * scale, a.z * scale, a.w * scale);
      reinterpret_cast<float4*>(&s_q[qi][AT_DH])[part] = greg[i];
    }
    if (NS == 1) {
      if (tid < 2 * AT_TK) s_q[tid & (AT_TK - 1)][2 * AT_DH + (tid >> 6)] = sreg;
    } else {
      s_q[tid][2 * AT_DH] = sreg;
      s_q[tid][2 * AT_DH + 1] = sreg2;
    }
    __syncthreads();
    if (q0 + AT_TK < len) fetch(q0 + AT_TK);
#pragma unroll 2
    for (int j = 0; j < qn; ++j) {                           // queries of the sequence only: qn is workgroup-uniform
      float qr[AT_DH], gr[AT_DH];
#pragma unroll
      for (int i = 0; i < AT_DH / 4; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(&s_q[j][4 * i]), b = *reinterpret_cast<const float4*>(&s_q[j][AT_DH + 4 * i]);
        qr[4 * i] = a.x; qr[4 * i + 1] = a.y; qr[4 * i + 2] = a.z; qr[4 * i + 3] = a.w;
        gr[4 * i] = b.x; gr[4 * i + 1] = b.y; gr[4 * i + 2] = b.z; gr[4 * i + 3] = b.w;
      }
      const float2 sd = *reinterpret_cast<const float2*>(&s_q[j][2 * AT_DH]);       // (lse, D) of the query
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        float a = 0.0f, dp = 0.0f;
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) a = fmaf(qr[i], k[u][i], a);       // the forward's score, bit for bit
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) dp = fmaf(gr[i], v[u][i], dp);
        const float p = __expf(a - sd.x);
        const float ds = p * (dp - sd.y);
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) dv[u][i] = fmaf(p, gr[i], dv[u][i]);
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) dk[u][i] = fmaf(ds, qr[i], dk[u][i]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < KPL; ++u) {
    if (!k_ok[u]) continue;
    float4* dkd = reinterpret_cast<float4*>(dqkv + (row0 + k_row[u]) * ldq + (int64_t)(H + h) * AT_DH);
    float4* dvd = reinterpret_cast<float4*>(dqkv + (row0 + k_row[u]) * ldq + (int64_t)(2 * H + h) * AT_DH);
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i) {
      dkd[i] = make_float4(dk[u][4 * i], dk[u][4 * i + 1], dk[u][4 * i + 2], dk[u][4 * i + 3]);
      dvd[i] = make_float4(dv[u][4 * i], dv[u][4 * i + 1], dv[u][4 * i + 2], dv[u][4 * i + 3]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm over 128 channels, backward
constexpr int LNB_MAX_WG = PFPP_LAYERNORM128_BWD_MAX_WG;     // workgroups of four waves; every wave leaves one partial row pair

__global__ __launch_bounds__(256) void layernorm128_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ gamma, float* __restrict__ dx,
                                                               float* __restrict__ part, int64_t rows, float eps, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  const float2 gm = reinterpret_cast<const float2*>(gamma)[lane];
  float dg0 = 0.0f, dg1 = 0.0f, db0 = 0.0f, db1 = 0.0f;
  for (int64_t row = wave; row < rows; row += n_waves) {
    const float2 v = reinterpret_cast<const float2*>(x + row * TF_C)[lane];
    const float2 d = reinterpret_cast<const float2*>(dy + row * TF_C)[lane];
    // mean and rstd as layernorm128_kernel forms them
    float s = v.x + v.y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s * (1.0f / TF_C);
    const float ex = v.x - mean, ey = v.y - mean;
    float q = fmaf(ex, ex, ey * ey);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * (1.0f / TF_C) + eps);
    const float hx = ex * rstd, hy = ey * rstd;              // x hat
    const float gx = d.x * gm.x, gy = d.y * gm.y;
    float a = gx + gy, b = fmaf(gx, hx, gy * hy);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    const float m1 = a * (1.0f / TF_C), m2 = b * (1.0f / TF_C);
    float rx = rstd * ((gx - m1) - hx * m2), ry = rstd * ((gy - m1) - hy * m2);
    float2* dst = reinterpret_cast<float2*>(dx + row * TF_C) + lane;
    if (accumulate) { const float2 old = *dst; rx += old.x; ry += old.y; }
    *dst = make_float2(rx, ry);
    dg0 = fmaf(d.x, hx, dg0); dg1 = fmaf(d.y, hy, dg1);
    db0 += d.x; db1 += d.y;
  }
  float* p = part + wave * (2 * TF_C);                       // [wave][dgamma 128 | dbeta 128]; a wave without rows leaves zeros
  reinterpret_cast<float2*>(p)[lane] = make_float2(dg0, dg1);
  reinterpret_cast<float2*>(p + TF_C)[lane] = make_float2(db0, db1);
}

// eight workgroups, each 32 of the 256 outputs (dgamma | dbeta, channel) x 8 slices of the partials: slice s sums the waves
// w = s, s + 8, ... in that order into four running sums (w / 8 mod 4), in fp64; slice 0 adds the eight slices' sums in slice order
constexpr int LNF_OUT = 32, LNF_SLICES = 8;

__global__ __launch_bounds__(256) void layernorm128_fold_kernel(const float* __restrict__ part, int64_t n_waves, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta) {
  __shared__ double s_sum[LNF_SLICES][LNF_OUT];
  const int o = threadIdx.x & (LNF_OUT - 1), slice = threadIdx.x >> 5;
  const int t = blockIdx.x * LNF_OUT + o;                    // 0 .. 255
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t w0 = slice; w0 < n_waves; w0 += 4 * LNF_SLICES) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t w = w0 + (int64_t)i * LNF_SLICES;
      if (w < n_waves) acc[i] += (double)part[w * (2 * TF_C) + t];
    }
  }
  s_sum[slice][o] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  if (slice == 0) {
    double a = s_sum[0][o];
#pragma unroll
    for (int i = 1; i < LNF_SLICES; ++i) a += s_sum[i][o];
    (t < TF_C ? dgamma : dbeta)[t & (TF_C - 1)] = (float)a;
  }
}

// ------------------------------------------------------------------------------------------------ ReLU backward
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ h, float* __restrict__ dh, int64_t rows, int64_t cols,
                                                       int64_t ld) {
  const int64_t n = rows * cols;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t i = (e / cols) * ld + e % cols;
    dh[i] = h[i] > 0.0f ? dh[i] : 0.0f;                      // 0 and -0 are not above 0
  }
}

}  // namespace

extern "C" int pfpp_attn_rows16_train(const float* qkv, float* out, float* lse, const int32_t* seq_off, const int32_t* seq_len,
                                      int64_t n_seq, int64_t max_len, int64_t H, int64_t dh, float scale, pfpp_stream_t stream) {
  PFPP_REQUIRE(n_seq >= 0 && max_len >= 1 && H >= 1, "bad sizes");
  PFPP_SUPPORTED(dh == AT_DH, "dim_head must be 16 (pfpp_attn_dense_train covers 32 and 64)");
  PFPP_SUPPORTED(n_seq <= 65535 && H <= 65535 && max_len < (1ll << 30), "too many sequences / heads / rows for one launch");
  if (n_seq == 0) return PFPP_OK;
  PFPP_REQUIRE(qkv && out && lse && seq_off && seq_len, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(qkv) && pfpp::aligned16(out), "16-byte alignment");
  attn_rows16_launch<true>(qkv, out, lse, seq_off, seq_len, n_seq, max_len, H, scale, stream);
  return pfpp::check_launch("pfpp_attn_rows16_train");
}

extern "C" int pfpp_attn_rows16_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dvec, float* dqkv,
                                    const int32_t* seq_off, const int32_t* seq_len, int64_t n_seq, int64_t max_len, int64_t H, int64_t dh,
                                    float scale, pfpp_stream_t stream) {
  PFPP_REQUIRE(n_seq >= 0 && max_len >= 1 && H >= 1, "bad sizes");
  PFPP_SUPPORTED(dh == AT_DH, "dim_head must be 16 (pfpp_attn_dense_bwd covers 32 and 64)");
  PFPP_SUPPORTED(n_seq <= 65535 && H <= 65535 && max_len < (1ll << 30), "too many sequences / heads / rows for one launch");
  if (n_seq == 0) return PFPP_OK;
  PFPP_REQUIRE(qkv && out && dout && lse && dvec && dqkv && seq_off && seq_len, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(qkv) && pfpp::aligned16(out) && pfpp::aligned16(dout) && pfpp::aligned16(dqkv), "16-byte alignment");
  hipStream_t st = pfpp::as_stream(stream);
  if (attn_rows16_big(n_seq, max_len, H)) {                  // the forward's rule: sizes only
    const dim3 grid((unsigned)((max_len + 511) / 512), (unsigned)H, (unsigned)n_seq);
    hipLaunchKernelGGL((attn16_dq_kernel<2, 256>), grid, dim3(256), 0, st, qkv, out, dout, lse, dvec, dqkv, seq_off, seq_len, (int)H, scale);
    hipLaunchKernelGGL((attn16_dkv_kernel<2, 256>), grid, dim3(256), 0, st, qkv, dout, lse, dvec, dqkv, seq_off, seq_len, (int)H, scale);
  } else {
    const dim3 grid((unsigned)((max_len + 63) / 64), (unsigned)H, (unsigned)n_seq);
    hipLaunchKernelGGL((attn16_dq_kernel<1, 64>), grid, dim3(64), 0, st, qkv, out, dout, lse, dvec, dqkv, seq_off, seq_len, (int)H, scale);
    hipLaunchKernelGGL((attn16_dkv_kernel<1, 64>), grid, dim3(64), 0, st, qkv, dout, lse, dvec, dqkv, seq_off, seq_len, (int)H, scale);
  }
  return pfpp::check_launch("pfpp_attn_rows16_bwd");
}

extern "C" int pfpp_layernorm128_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta,
                                     float* workspace, int64_t rows, int64_t C, float eps, int accumulate_dx, pfpp_stream_t stream) {
  PFPP_REQUIRE(rows >= 0 && eps >= 0.0f, "bad sizes");
  PFPP_SUPPORTED(C == TF_C, "rows of 128 channels only (pfpp_layernorm_bwd covers 256, 512 and 1024)");
  if (rows == 0) return PFPP_OK;                             // nothing is written, dgamma and dbeta included
  PFPP_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && workspace, "null pointer");
  hipStream_t st = pfpp::as_stream(stream);
  PFPP_REQUIRE(pfpp::aligned16(x) && pfpp::aligned16(dy) && pfpp::aligned16(dx) && pfpp::aligned16(gamma) && pfpp::aligned16(workspace),
               "16-byte alignment");
  const int64_t wgs = (rows + 3) / 4 < LNB_MAX_WG ? (rows + 3) / 4 : LNB_MAX_WG;
  hipLaunchKernelGGL(layernorm128_bwd_kernel, dim3((unsigned)wgs), dim3(256), 0, st, x, dy, gamma, dx, workspace, rows, eps, accumulate_dx);
  hipLaunchKernelGGL(layernorm128_fold_kernel, dim3(2 * TF_C / LNF_OUT), dim3(LNF_OUT * LNF_SLICES), 0, st, workspace, wgs * 4, dgamma, dbeta);
  return pfpp::check_launch("pfpp_layernorm128_bwd");
}

extern "C" int pfpp_relu_bwd(const float* h, float* dh, int64_t rows, int64_t cols, int64_t ld, pfpp_stream_t stream) {
  PFPP_REQUIRE(rows >= 0 && cols >= 0 && ld >= cols, "bad sizes");
  if (rows == 0 || cols == 0) return PFPP_OK;
  PFPP_REQUIRE(h && dh, "null pointer");
  const int64_t n = rows * cols;
  const int64_t blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, pfpp::as_stream(stream), h, dh, rows, cols, ld);
  return pfpp::check_launch("pfpp_relu_bwd");
}
