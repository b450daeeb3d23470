// The matcher's two layers between its encoder and its head (Jigsaw_matching/model/jigsaw/attention_layer.py): tf_self1
// (PointTransformerLayer, :159-225) and the attention of tf_cross1 (ScaledDotProductAttention inside CrossAttentionLayer, :9-75).
//
//  * feat_knn_kernel — knn(x, x, 16, batch, batch) + to_dense_batch(fill_value = N) of knn_and_group (:136-139) on 128-channel rows:
//    a workgroup owns 64 queries of one piece, one per lane, each with its row and a sorted top-16 in registers; the piece's rows
//    are split into four contiguous runs, one per wave, streamed through LDS in tiles and read as broadcasts; the three upper waves'
//    lists are merged into wave 0's in run order.  The key is d = sum_c (a_c - b_c)^2 summed in channel order in fp32 without
//    contraction, compared as (bits of d, index): candidates arrive in ascending index order and only a strictly smaller key moves
//    ahead, so a tie keeps the lower index first.  Slots behind min(16, n_piece) hold N.
//  * ptf_aggregate_kernel — linear_p, linear_w, the softmax over the 16 neighbours and the weighted sum (:206-224) of one point
//    per workgroup pass: the [16, 128] relation tile lives in LDS, the 128 -> 16 product on the VALU with the weight row in
//    registers, nothing of size [N, 16, .] is written.  An index outside [0, N) is the reference's appended zero row.
//  * attn_rows16_kernel (csrc/attn_rows16.h, shared with the training unit) — softmax(q k^T scale) v for 16-wide heads over sequences
//    of any length: one or two queries per lane (by the size of the launch) with their
//    accumulators in registers, keys and values staged through LDS in tiles of 64 and read as broadcasts, online softmax per lane
//    (no cross-lane step).  All products are fp32 FMAs; the path depends on nothing but the sizes.
//  * layernorm128_kernel — nn.LayerNorm(128, eps) with weight and bias, a wave per row (the width pfpp_layernorm does not cover).
// No atomics anywhere: two runs agree bitwise.  This unit is compiled without contraction; fused operations are written as fmaf.
#include "pfpp_common.h"
#include "attn_rows16.h"
#include "ptf_common.h"            // TF_C, TF_K, PW_*, AG_LDH: shared with the training unit

namespace {

// ------------------------------------------------------------------------------------------------ neighbours in feature space
constexpr int FK_THREADS = 256;
constexpr int FK_QUERIES = 64;                 // one per lane; the four waves share them and split the candidates
constexpr int FK_TILE = 16;                    // candidate rows per wave and step
constexpr int FK_LD = TF_C;                    // floats per staged row (reads are broadcasts: no padding needed)

struct TopK {
  unsigned key[TF_K];
  int idx[TF_K];
};

// (key, idx) goes to its place among the ascending keys; only a strictly smaller key passes an entry
__device__ __forceinline__ void topk_insert(TopK& t, unsigned key, int idx) {
  if (key < t.key[TF_K - 1]) {
    t.key[TF_K - 1] = key;
    t.idx[TF_K - 1] = idx;
#pragma unroll
    for (int s = TF_K - 1; s > 0; --s) {
      const bool sw = t.key[s] < t.key[s - 1];
      const unsigned ka = t.key[s - 1], kb = t.key[s];
      const int ia = t.idx[s - 1], ib = t.idx[s];
      t.key[s - 1] = sw ? kb : ka;
      t.key[s] = sw ? ka : kb;
      t.idx[s - 1] = sw ? ib : ia;
      t.idx[s] = sw ? ia : ib;
    }
  }
}

__global__ __launch_bounds__(FK_THREADS) void feat_knn_kernel(const float* __restrict__ feats, int64_t ld,
                                                              const int64_t* __restrict__ piece_off, int64_t P, int64_t N,
                                                              int32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][FK_TILE][FK_LD];           // 32 KiB; reused for the merge
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // which piece and which block of its queries: pieces take ceil(n / 64) workgroups each, in order
  int64_t b = blockIdx.x, p = 0;
  int64_t base = 0;
  int n = 0;
  for (; p < P; ++p) {
    base = piece_off[p];
    n = (int)(piece_off[p + 1] - base);
    const int64_t nb = (n + FK_QUERIES - 1) / FK_QUERIES;
    if (b < nb) break;
    b -= nb;
  }
  if (p >= P) return;                                        // the grid is an upper bound
  const int q_local = (int)b * FK_QUERIES + lane;
  const bool q_ok = q_local < n;
  const float4* qrow = reinterpret_cast<const float4*>(feats + (base + (q_ok ? q_local : n - 1)) * ld);
  float qv[TF_C];
#pragma unroll
  for (int c = 0; c < TF_C / 4; ++c) {
    const float4 v = qrow[c];
    qv[4 * c] = v.x; qv[4 * c + 1] = v.y; qv[4 * c + 2] = v.z; qv[4 * c + 3] = v.w;
  }
  TopK top;
#pragma unroll
  for (int s = 0; s < TF_K; ++s) { top.key[s] = 0xFFFFFFFFu; top.idx[s] = (int)N; }
  // wave w walks the candidates [w run, min(n, (w + 1) run)), all waves the same number of steps
  const int run = (n + 3) / 4;
  const int c_lo = wave * run, c_hi = min(n, c_lo + run);
  const int steps = (run + FK_TILE - 1) / FK_TILE;
  for (int st = 0; st < steps; ++st) {
    const int j0 = c_lo + st * FK_TILE;
    __syncthreads();                                         // the previous tile has been read
#pragma unroll
    for (int i = 0; i < FK_TILE * (FK_LD / 4) / 64; ++i) {   // 512 float4 per wave: 8 per lane, rows of 32
      const int e = i * 64 + lane, r = e >> 5, c4 = e & 31;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (j0 + r < c_hi) v = reinterpret_cast<const float4*>(feats + (base + j0 + r) * ld)[c4];
      reinterpret_cast<float4*>(&s_tile[wave][r][0])[c4] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int r0 = 0; r0 < FK_TILE; r0 += 4) {
      if (j0 + r0 >= c_hi) break;                            // wave-uniform
      float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;      // four candidates per pass over the query row
      const float* row = &s_tile[wave][r0][0];
      float4 a0 = *reinterpret_cast<const float4*>(row), a1 = *reinterpret_cast<const float4*>(row + FK_LD),
             a2 = *reinterpret_cast<const float4*>(row + 2 * FK_LD), a3 = *reinterpret_cast<const float4*>(row + 3 * FK_LD);
#pragma unroll
      for (int c = 0; c < TF_C; c += 4) {
        // the next four channels are on their way while these are summed; the scheduling barrier keeps the reads of the whole row
        // from being hoisted to the top of the unrolled body (512 registers, spills)
        const int cn = c + 4 < TF_C ? c + 4 : c;
        const float4 n0 = *reinterpret_cast<const float4*>(row + cn), n1 = *reinterpret_cast<const float4*>(row + FK_LD + cn),
                     n2 = *reinterpret_cast<const float4*>(row + 2 * FK_LD + cn), n3 = *reinterpret_cast<const float4*>(row + 3 * FK_LD + cn);
        float t;
        t = __fsub_rn(qv[c], a0.x); d0 = __fadd_rn(d0, __fmul_rn(t, t));
        t = __fsub_rn(qv[c], a1.x); d1 = __fadd_rn(d1, __fmul_rn(t, t));
        t = __fsub_rn(qv[c], a2.x); d2 = __fadd_rn(d2, __fmul_rn(t, t));
        t = __fsub_rn(qv[c], a3.x); d3 = __fadd_rn(d3, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 1], a0.y); d0 = __fadd_rn(d0, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 1], a1.y); d1 = __fadd_rn(d1, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 1], a2.y); d2 = __fadd_rn(d2, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 1], a3.y); d3 = __fadd_rn(d3, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 2], a0.z); d0 = __fadd_rn(d0, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 2], a1.z); d1 = __fadd_rn(d1, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 2], a2.z); d2 = __fadd_rn(d2, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 2], a3.z); d3 = __fadd_rn(d3, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 3], a0.w); d0 = __fadd_rn(d0, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 3], a1.w); d1 = __fadd_rn(d1, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 3], a2.w); d2 = __fadd_rn(d2, __fmul_rn(t, t));
        t = __fsub_rn(qv[c + 3], a3.w); d3 = __fadd_rn(d3, __fmul_rn(t, t));
        __builtin_amdgcn_sched_barrier(0);
        a0 = n0; a1 = n1; a2 = n2; a3 = n3;
      }
      // a row behind the run gets the key no entry is larger than
      const int j = j0 + r0;
      const unsigned k0 = __float_as_uint(d0);
      const unsigned k1 = j + 1 < c_hi ? __float_as_uint(d1) : 0xFFFFFFFFu;
      const unsigned k2 = j + 2 < c_hi ? __float_as_uint(d2) : 0xFFFFFFFFu;
      const unsigned k3 = j + 3 < c_hi ? __float_as_uint(d3) : 0xFFFFFFFFu;
      // one threshold test for the four: insertions are rare.  It also keeps all four sums in front of the first insertion; used under
      // four separate conditions, three of them are sunk behind it and hold their staged rows alive in registers (spills).
      if (min(min(k0, k1), min(k2, k3)) < top.key[TF_K - 1]) {
        topk_insert(top, k0, (int)(base + j));
        topk_insert(top, k1, (int)(base + j + 1));
        topk_insert(top, k2, (int)(base + j + 2));
        topk_insert(top, k3, (int)(base + j + 3));
      }
    }
  }
  // merge: waves 1..3 hand their lists over through LDS; wave 0 takes them in run order (their indices ascend with the wave)
  __syncthreads();
  unsigned* s_key = reinterpret_cast<unsigned*>(&s_tile[0][0][0]);                   // [3][16][64]
  int* s_idx = reinterpret_cast<int*>(s_key + 3 * TF_K * 64);                        // [3][16][64]: 24 KiB of the 32
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < TF_K; ++s) {
      s_key[((wave - 1) * TF_K + s) * 64 + lane] = top.key[s];
      s_idx[((wave - 1) * TF_K + s) * 64 + lane] = top.idx[s];
    }
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll 1
  for (int e = 0; e < 3 * TF_K; ++e) topk_insert(top, s_key[e * 64 + lane], s_idx[e * 64 + lane]);
  if (q_ok) {
    int4* o = reinterpret_cast<int4*>(out + (base + q_local) * TF_K);
#pragma unroll
    for (int s = 0; s < TF_K / 4; ++s) o[s] = make_int4(top.idx[4 * s], top.idx[4 * s + 1], top.idx[4 * s + 2], top.idx[4 * s + 3]);
  }
}

// ------------------------------------------------------------------------------------------------ point-transformer aggregation
constexpr int AG_THREADS = 256;

__global__ __launch_bounds__(AG_THREADS) void ptf_aggregate_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                                   const float* __restrict__ xv, int64_t ld,
                                                                   const float* __restrict__ xyz, const int32_t* __restrict__ idx_k,
                                                                   const int32_t* __restrict__ idx_v, const float* __restrict__ wp,
                                                                   int64_t N, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_h[TF_K][AG_LDH];       // relu(bn(r)) of the point's 16 neighbours
  __shared__ float s_u[TF_K][TF_K + 1];                                  // hidden layer of linear_w
  __shared__ float s_w[TF_K][TF_K + 1];                                  // logits, then exp(logit - max) per (neighbour, channel)
  __shared__ float s_part[2][TF_C];
  const int tid = threadIdx.x;
  const int c = tid & (TF_C - 1), hf = tid >> 7;             // gather / output role: channel c, neighbours 8 hf .. 8 hf + 7
  const int t = tid >> 4, j = tid & 15;                      // linear_w role: neighbour t, output j
  // weights this thread keeps for every point it sees
  float w3[TF_C];
#pragma unroll
  for (int i = 0; i < TF_C / 4; ++i) {
    const float4 v = reinterpret_cast<const float4*>(wp + PW_W3 + j * TF_C)[i];
    w3[4 * i] = v.x; w3[4 * i + 1] = v.y; w3[4 * i + 2] = v.z; w3[4 * i + 3] = v.w;
  }
  float w4[TF_K];
#pragma unroll
  for (int i = 0; i < TF_K; ++i) w4[i] = wp[PW_W4 + j * TF_K + i];
  const float a2 = wp[PW_A2 + j], c2 = wp[PW_C2 + j], b4 = wp[PW_B4 + j];
  const float p2x = wp[PW_P2W + 3 * c], p2y = wp[PW_P2W + 3 * c + 1], p2z = wp[PW_P2W + 3 * c + 2], p2b = wp[PW_P2B + c];
  const float a1 = wp[PW_A1 + c], c1 = wp[PW_C1 + c];
  float p1w[9], p1s[3], p1t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) p1w[i] = wp[PW_P1W + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { p1s[i] = wp[PW_P1S + i]; p1t[i] = wp[PW_P1T + i]; }

  for (int64_t pt = blockIdx.x; pt < N; pt += gridDim.x) {
    const float px = xyz[3 * pt], py = xyz[3 * pt + 1], pz = xyz[3 * pt + 2];
    const float q = xq[pt * ld + c];
    float pr[8], vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int tt = hf * 8 + u;
      const int ik = idx_k[pt * TF_K + tt], iv = idx_v[pt * TF_K + tt];
      const bool ok_k = (unsigned)ik < (unsigned)N, ok_v = (unsigned)iv < (unsigned)N;   // anything else is the appended zero row
      const int64_t rk = ok_k ? ik : 0, rv = ok_v ? iv : 0;
      const float dx = ok_k ? xyz[3 * rk] - px : 0.0f, dy = ok_k ? xyz[3 * rk + 1] - py : 0.0f, dz = ok_k ? xyz[3 * rk + 2] - pz : 0.0f;
      const float kk = ok_k ? xk[rk * ld + c] : 0.0f;
      vv[u] = ok_v ? xv[rv * ld + c] : 0.0f;
      // linear_p: Linear(3, 3) -> BatchNorm (scale, shift) -> ReLU -> Linear(3, 128)
      const float g0 = fmaxf(fmaf(fmaf(p1w[2], dz, fmaf(p1w[1], dy, p1w[0] * dx)), p1s[0], p1t[0]), 0.0f);
      const float g1 = fmaxf(fmaf(fmaf(p1w[5], dz, fmaf(p1w[4], dy, p1w[3] * dx)), p1s[1], p1t[1]), 0.0f);
      const float g2 = fmaxf(fmaf(fmaf(p1w[8], dz, fmaf(p1w[7], dy, p1w[6] * dx)), p1s[2], p1t[2]), 0.0f);
      pr[u] = fmaf(p2z, g2, fmaf(p2y, g1, fmaf(p2x, g0, p2b)));
      const float r = (kk - q) + pr[u];                      // x_k - x_q + p_r (:208-214)
      s_h[tt][c] = fmaxf(fmaf(r, a1, c1), 0.0f);
    }
    __syncthreads();
    // linear_w[2]: [16 neighbours, 128] x [128, 16]; thread (t, j), four partial sums
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
    for (int i = 0; i < TF_C; i += 4) {
      const float4 h = *reinterpret_cast<const float4*>(&s_h[t][i]);
      s0 = fmaf(h.x, w3[i], s0); s1 = fmaf(h.y, w3[i + 1], s1); s2 = fmaf(h.z, w3[i + 2], s2); s3 = fmaf(h.w, w3[i + 3], s3);
    }
    s_u[t][j] = fmaxf(fmaf((s0 + s1) + (s2 + s3), a2, c2), 0.0f);
    __syncthreads();
    float lg = b4;
#pragma unroll
    for (int i = 0; i < TF_K; ++i) lg = fmaf(s_u[t][i], w4[i], lg);
    s_w[t][j] = lg;
    __syncthreads();
    float mx = s_w[0][j];                                    // softmax over the neighbours (dim 1) per channel j
#pragma unroll
    for (int i = 1; i < TF_K; ++i) mx = fmaxf(mx, s_w[i][j]);
    __syncthreads();
    s_w[t][j] = expf(lg - mx);
    __syncthreads();
    const int jc = c & (TF_K - 1);
    float den = 0.0f;
#pragma unroll
    for (int i = 0; i < TF_K; ++i) den += s_w[i][jc];
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(vv[u] + pr[u], s_w[hf * 8 + u][jc] / den, acc);
    s_part[hf][c] = acc;
    __syncthreads();
    if (hf == 0) out[pt * TF_C + c] = s_part[0][c] + s_part[1][c];
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm over 128 channels
// nn.LayerNorm(128, eps) with weight and bias (pfpp_layernorm covers 256, 512 and 1024 channels): one wave per row, two channels
// per lane, mean and the mean of the squared deviations by butterfly sums (every lane ends with the same bits), 1 / sqrt(var + eps).
__global__ __launch_bounds__(256) void layernorm128_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ out, int64_t rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float2 v = reinterpret_cast<const float2*>(x + row * TF_C)[lane];
  float s = v.x + v.y;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s * (1.0f / TF_C);
  const float dx = v.x - mean, dy = v.y - mean;
  float q = fmaf(dx, dx, dy * dy);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = 1.0f / sqrtf(q * (1.0f / TF_C) + eps);
  const float2 g = reinterpret_cast<const float2*>(gamma)[lane], b = reinterpret_cast<const float2*>(beta)[lane];
  reinterpret_cast<float2*>(out + row * TF_C)[lane] = make_float2(fmaf(dx * rstd, g.x, b.x), fmaf(dy * rstd, g.y, b.y));
}

}  // namespace

extern "C" int pfpp_feat_knn(const float* feats, int64_t ld, const int64_t* piece_off, int64_t P, int64_t N, int64_t C, int64_t K,
                             int64_t max_n, int32_t* idx, pfpp_stream_t stream) {
  PFPP_REQUIRE(P >= 0 && N >= 0 && max_n >= 0 && max_n <= N, "bad sizes");
  PFPP_SUPPORTED(C == TF_C, "rows of 128 channels only");
  PFPP_SUPPORTED(K == TF_K, "K must be 16");
  PFPP_SUPPORTED(max_n <= 8192, "a piece of more than 8192 points");
  PFPP_SUPPORTED(N < (1ll << 31) / TF_K, "index range exceeds int32");
  PFPP_SUPPORTED(P <= 65536, "more than 65536 pieces (every workgroup walks the offsets)");
  if (N == 0 || P == 0) return PFPP_OK;
  PFPP_REQUIRE(feats && piece_off && idx, "null pointer");
  PFPP_REQUIRE(ld >= C && ld % 4 == 0 && pfpp::aligned16(feats) && pfpp::aligned16(idx), "rows must be 16-byte aligned, ld >= C and a multiple of 4");
  const int64_t blocks = (N + FK_QUERIES - 1) / FK_QUERIES + P;          // sum over the pieces of ceil(n / 64) is at most this
  hipLaunchKernelGGL(feat_knn_kernel, dim3((unsigned)blocks), dim3(FK_THREADS), 0, pfpp::as_stream(stream), feats, ld, piece_off, P, N, idx);
  return pfpp::check_launch("pfpp_feat_knn");
}

extern "C" int pfpp_ptf_aggregate(const float* q, const float* k, const float* v, int64_t ld, const float* xyz, const int32_t* idx_k,
                                  const int32_t* idx_v, const float* weights, int64_t N, int64_t C, int64_t K, float* out,
                                  pfpp_stream_t stream) {
  PFPP_REQUIRE(N >= 0, "bad sizes");
  PFPP_SUPPORTED(C == TF_C, "rows of 128 channels only");
  PFPP_SUPPORTED(K == TF_K, "K must be 16");
  PFPP_SUPPORTED(N < (1ll << 31) / TF_K, "index range exceeds int32");
  if (N == 0) return PFPP_OK;
  PFPP_REQUIRE(q && k && v && xyz && idx_k && idx_v && weights && out, "null pointer");
  PFPP_REQUIRE(ld >= C && pfpp::aligned16(weights), "ld >= C, weights 16-byte aligned");
  const int64_t blocks = N < 1024 ? N : 1024;                            // a workgroup walks its points: weights are loaded once
  hipLaunchKernelGGL(ptf_aggregate_kernel, dim3((unsigned)blocks), dim3(AG_THREADS), 0, pfpp::as_stream(stream), q, k, v, ld, xyz, idx_k,
                     idx_v, weights, N, out);
  return pfpp::check_launch("pfpp_ptf_aggregate");
}

extern "C" int pfpp_attn_rows16(const float* qkv, float* out, const int32_t* seq_off, const int32_t* seq_len, int64_t n_seq,
                                int64_t max_len, int64_t H, int64_t dh, float scale, pfpp_stream_t stream) {
  PFPP_REQUIRE(n_seq >= 0 && max_len >= 1 && H >= 1, "bad sizes");
  PFPP_SUPPORTED(dh == AT_DH, "dim_head must be 16 (pfpp_attn_dense covers 32 and 64)");
  PFPP_SUPPORTED(n_seq <= 65535 && H <= 65535 && max_len < (1ll << 30), "too many sequences / heads / rows for one launch");
  if (n_seq == 0) return PFPP_OK;
  PFPP_REQUIRE(qkv && out && seq_off && seq_len, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(qkv) && pfpp::aligned16(out), "16-byte alignment");
  attn_rows16_launch<false>(qkv, out, nullptr, seq_off, seq_len, n_seq, max_len, H, scale, stream);       // <2, 256> or <1, 64> by the sizes
  return pfpp::check_launch("pfpp_attn_rows16");
}

extern "C" int pfpp_layernorm128(const float* x, const float* gamma, const float* beta, float* out, int64_t rows, int64_t C, float eps,
                                 pfpp_stream_t stream) {
  PFPP_REQUIRE(rows >= 0 && eps >= 0.0f, "bad sizes");
  PFPP_SUPPORTED(C == TF_C, "rows of 128 channels only (pfpp_layernorm covers 256, 512 and 1024)");
  PFPP_SUPPORTED((rows + 3) / 4 < (1ll << 31), "grid too large");
  if (rows == 0) return PFPP_OK;
  PFPP_REQUIRE(x && gamma && beta && out, "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(x) && pfpp::aligned16(out) && pfpp::aligned16(gamma) && pfpp::aligned16(beta), "16-byte alignment");
  hipLaunchKernelGGL(layernorm128_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), x, gamma, beta, out, rows, eps);
  return pfpp::check_launch("pfpp_layernorm128");
}
