// attn_rows16_kernel — softmax(q k^T scale) v for 16-wide heads over sequences of any length, shared by csrc/matching_tf.hip
// (pfpp_attn_rows16) and csrc/matching_tf_train.hip (pfpp_attn_rows16_train, which also stores the log-sum-exp of every row).
// One or two queries per lane (by the size of the launch) with their accumulators in registers, keys and values staged through LDS
// in tiles of 64 and read as broadcasts, online softmax per lane (no cross-lane step).  All products are fp32 FMAs; the path depends
// on nothing but the sizes.  AT_LSE adds one store behind the loop and nothing else: with it off the kernel is the one without it.
// Include from a unit compiled without contraction; fused operations are written as fmaf.
#ifndef PFPP_ATTN_ROWS16_H_
#define PFPP_ATTN_ROWS16_H_
#include "pfpp_common.h"

namespace {

constexpr int AT_DH = 16;
constexpr int AT_TK = 64;                                    // keys per staged tile
constexpr int AT_CH = 8;                                     // keys per online-softmax step

// AT_QPL queries per lane, AT_THREADS lanes per workgroup: <2, 256> when the launch has workgroups to spare, <1, 64> when it has few
// (one puzzle in flight).  A query's arithmetic is the same in both: the same tiles of 64 keys in steps of 8.
template <int AT_QPL, int AT_THREADS, bool AT_LSE>
__global__ __launch_bounds__(AT_THREADS) void attn_rows16_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                 float* __restrict__ lse, const int32_t* __restrict__ seq_off,
                                                                 const int32_t* __restrict__ seq_len, int H, float scale) {
  __shared__ __attribute__((aligned(16))) float s_k[AT_TK][AT_DH];
  __shared__ __attribute__((aligned(16))) float s_v[AT_TK][AT_DH];
  const int tid = threadIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int len = seq_len[s];
  constexpr int AT_QB = AT_THREADS * AT_QPL;                 // queries per workgroup
  const int q_base = blockIdx.x * AT_QB;
  if (q_base >= len) return;                                 // workgroup-uniform
  const int64_t row0 = seq_off[s];
  const int64_t ldq = 3 * (int64_t)H * AT_DH;
  const float* kbase = qkv + row0 * ldq + (int64_t)(H + h) * AT_DH;
  const float* vbase = qkv + row0 * ldq + (int64_t)(2 * H + h) * AT_DH;
  float q[AT_QPL][AT_DH], o[AT_QPL][AT_DH], m[AT_QPL], l[AT_QPL];
  bool q_ok[AT_QPL];
  int q_row[AT_QPL];
#pragma unroll
  for (int u = 0; u < AT_QPL; ++u) {
    const int qi = q_base + u * AT_THREADS + tid;
    q_ok[u] = qi < len;
    q_row[u] = q_ok[u] ? qi : len - 1;
    const float4* src = reinterpret_cast<const float4*>(qkv + (row0 + q_row[u]) * ldq + (int64_t)h * AT_DH);
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i) {
      const float4 v = src[i];
      q[u][4 * i] = v.x * scale; q[u][4 * i + 1] = v.y * scale; q[u][4 * i + 2] = v.z * scale; q[u][4 * i + 3] = v.w * scale;
    }
#pragma unroll
    for (int i = 0; i < AT_DH; ++i) o[u][i] = 0.0f;
    m[u] = -__builtin_huge_valf();
    l[u] = 0.0f;
  }
  // a tile of 64 keys x (4 + 4) float4 goes from HBM to registers one tile ahead of its use and from there to LDS: the loads of the
  // next tile are in flight while this one is summed (a workgroup of one wave has nothing else to hide them behind)
  constexpr int AT_NP = AT_TK * 4 / AT_THREADS;              // (key, part) pairs per thread
  float4 kreg[AT_NP], vreg[AT_NP];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AT_NP; ++i) {
      const int e = i * AT_THREADS + tid, key = e >> 2, part = e & 3;
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
    for (int i = 0; i < AT_NP; ++i) {
      const int e = i * AT_THREADS + tid, key = e >> 2, part = e & 3;
      reinterpret_cast<float4*>(&s_k[key][0])[part] = kreg[i];
      reinterpret_cast<float4*>(&s_v[key][0])[part] = vreg[i];
    }
    __syncthreads();
    if (k0 + AT_TK < len) fetch(k0 + AT_TK);
#pragma unroll 1
    for (int j0 = 0; j0 < kn; j0 += AT_CH) {
      float sc[AT_QPL][AT_CH];
#pragma unroll
      for (int e = 0; e < AT_CH; ++e) {
        float kr[AT_DH];
#pragma unroll
        for (int i = 0; i < AT_DH / 4; ++i) {
          const float4 v = *reinterpret_cast<const float4*>(&s_k[j0 + e][4 * i]);
          kr[4 * i] = v.x; kr[4 * i + 1] = v.y; kr[4 * i + 2] = v.z; kr[4 * i + 3] = v.w;
        }
        const bool live = j0 + e < kn;
#pragma unroll
        for (int u = 0; u < AT_QPL; ++u) {
          float a = 0.0f;
#pragma unroll
          for (int i = 0; i < AT_DH; ++i) a = fmaf(q[u][i], kr[i], a);
          sc[u][e] = live ? a : -__builtin_huge_valf();      // keys behind the sequence weigh exp(-inf) = 0
        }
      }
#pragma unroll
      for (int u = 0; u < AT_QPL; ++u) {
        float cm = sc[u][0];                                 // key j0 is always inside the sequence: the maximum is finite
#pragma unroll
        for (int e = 1; e < AT_CH; ++e) cm = fmaxf(cm, sc[u][e]);
        const float mn = fmaxf(m[u], cm);
        const float alpha = __expf(m[u] - mn);               // 0 on the first step (m = -inf)
        m[u] = mn;
        l[u] *= alpha;
#pragma unroll
        for (int i = 0; i < AT_DH; ++i) o[u][i] *= alpha;
#pragma unroll
        for (int e = 0; e < AT_CH; ++e) {
          sc[u][e] = __expf(sc[u][e] - mn);
          l[u] += sc[u][e];
        }
      }
#pragma unroll
      for (int e = 0; e < AT_CH; ++e) {
        float vr[AT_DH];
#pragma unroll
        for (int i = 0; i < AT_DH / 4; ++i) {
          const float4 v = *reinterpret_cast<const float4*>(&s_v[j0 + e][4 * i]);
          vr[4 * i] = v.x; vr[4 * i + 1] = v.y; vr[4 * i + 2] = v.z; vr[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < AT_QPL; ++u)
#pragma unroll
          for (int i = 0; i < AT_DH; ++i) o[u][i] = fmaf(sc[u][e], vr[i], o[u][i]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < AT_QPL; ++u) {
    if (!q_ok[u]) continue;
    const float inv = 1.0f / l[u];
    float4* dst = reinterpret_cast<float4*>(out + (row0 + q_row[u]) * ((int64_t)H * AT_DH) + (int64_t)h * AT_DH);
#pragma unroll
    for (int i = 0; i < AT_DH / 4; ++i)
      dst[i] = make_float4(o[u][4 * i] * inv, o[u][4 * i + 1] * inv, o[u][4 * i + 2] * inv, o[u][4 * i + 3] * inv);
    if (AT_LSE) lse[(row0 + q_row[u]) * H + h] = m[u] + logf(l[u]);          // of the scaled scores: what the backward subtracts
  }
}

// by the sizes alone: with fewer than 512 workgroups of 512 queries (two per CU) the launch is cut into workgroups of one wave and
// 64 queries, so one 5,000-point puzzle fills 632 of them instead of 80.  The backward's two passes use the same rule.
__host__ inline bool attn_rows16_big(int64_t n_seq, int64_t max_len, int64_t H) { return (max_len + 511) / 512 * H * n_seq >= 512; }

template <bool AT_LSE>
__host__ inline void attn_rows16_launch(const float* qkv, float* out, float* lse, const int32_t* seq_off, const int32_t* seq_len,
                                        int64_t n_seq, int64_t max_len, int64_t H, float scale, pfpp_stream_t stream) {
  if (attn_rows16_big(n_seq, max_len, H)) {
    const dim3 grid((unsigned)((max_len + 511) / 512), (unsigned)H, (unsigned)n_seq);
    hipLaunchKernelGGL((attn_rows16_kernel<2, 256, AT_LSE>), grid, dim3(256), 0, pfpp::as_stream(stream), qkv, out, lse, seq_off, seq_len,
                       (int)H, scale);
  } else {
    const dim3 grid((unsigned)((max_len + 63) / 64), (unsigned)H, (unsigned)n_seq);
    hipLaunchKernelGGL((attn_rows16_kernel<1, 64, AT_LSE>), grid, dim3(64), 0, pfpp::as_stream(stream), qkv, out, lse, seq_off, seq_len,
                       (int)H, scale);
  }
}

}  // namespace
#endif  // PFPP_ATTN_ROWS16_H_
