// The matcher's DGCNN encoder in eval mode (Jigsaw_matching/model/modules/encoder/dgcnn.py:41-56, 130-213), decomposed: with
// W = [W_a | W_b] the pre-activation of slot j of point i is W_a x_j + (W_b - W_a) x_i = u[j] + v[i], BatchNorm is a per-channel
// affine and LeakyReLU is monotone, so a level is one product uv = X [W_a ; W_b - W_a]^T (pfpp_gemm), a search and one pass that
// gathers 20 rows of u.  Nothing of size [N, 20, .] exists.
//
//  * dgcnn_knn_kernel<C> — knn(x, x, 20, batch, batch) + to_dense_batch(fill_value = N, max_num_nodes = 20) of
//    get_graph_feature_dynamic (:47-48) on rows of C = 3, 64 or 128 channels: the design of feat_knn_kernel (csrc/matching_tf.hip)
//    with a list of 20.  A workgroup owns 64 queries of one piece, one per lane, each with its row and a sorted top-20 in registers;
//    the piece's rows are split into four contiguous runs, one per wave, streamed through LDS in tiles of 16 rows and read as
//    broadcasts; the three upper waves' lists are merged into wave 0's in run order.  The key is d = sum_c (a_c - b_c)^2 summed in
//    channel order in fp32 without contraction, compared as (bits of d, index): candidates arrive in ascending index order and only a
//    strictly smaller key moves ahead, so a tie keeps the lower index first.  Slots behind min(20, n_piece) hold N.
//  * dgcnn_edge_kernel<LPR> — z_ij = u[idx[i, j]] + v[i] (0 for a slot that holds N), e_i = max_j z_ij where scale >= 0 and min_j z_ij
//    where scale < 0, out[i] = LeakyReLU(e_i scale + shift): a thread owns four channels of one point, its 20 rows of u are in flight
//    together.  The extremum is written with comparisons (e = z > e ? z : e), so signed zeros resolve by slot order.
//  * leaky_relu_kernel — x = x > 0 ? x : slope x in place over [rows, C] with a row stride.
// No atomics anywhere: two runs agree bitwise.  This unit is compiled without contraction.
#include "pfpp_common.h"

namespace {

constexpr int DG_K = 20;                       // neighbours per point (dgcnn.py:41)
constexpr int DK_THREADS = 256;
constexpr int DK_QUERIES = 64;                 // one per lane; the four waves share them and split the candidates
constexpr int DK_TILE = 16;                    // candidate rows per wave and step
constexpr int DK_MERGE_WORDS = 2 * 3 * DG_K * 64;          // keys and indices of the three upper waves: 30 KiB

struct Top20 {
  unsigned key[DG_K];
  int idx[DG_K];
};

// (key, idx) goes to its place among the ascending keys; only a strictly smaller key passes an entry
__device__ __forceinline__ void top20_insert(Top20& t, unsigned key, int idx) {
  if (key < t.key[DG_K - 1]) {
    t.key[DG_K - 1] = key;
    t.idx[DG_K - 1] = idx;
#pragma unroll
    for (int s = DG_K - 1; s > 0; --s) {
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

// squared distances of the query row to four staged rows (LD floats apart), channel by channel in order
template <int C, int LD>
__device__ __forceinline__ void dist4(const float (&qv)[C], const float* row, float& d0, float& d1, float& d2, float& d3) {
  d0 = d1 = d2 = d3 = 0.0f;
  if constexpr (C == 3) {
    const float4 a0 = *reinterpret_cast<const float4*>(row), a1 = *reinterpret_cast<const float4*>(row + LD),
                 a2 = *reinterpret_cast<const float4*>(row + 2 * LD), a3 = *reinterpret_cast<const float4*>(row + 3 * LD);
    float t;
    t = __fsub_rn(qv[0], a0.x); d0 = __fadd_rn(d0, __fmul_rn(t, t));
    t = __fsub_rn(qv[0], a1.x); d1 = __fadd_rn(d1, __fmul_rn(t, t));
    t = __fsub_rn(qv[0], a2.x); d2 = __fadd_rn(d2, __fmul_rn(t, t));
    t = __fsub_rn(qv[0], a3.x); d3 = __fadd_rn(d3, __fmul_rn(t, t));
    t = __fsub_rn(qv[1], a0.y); d0 = __fadd_rn(d0, __fmul_rn(t, t));
    t = __fsub_rn(qv[1], a1.y); d1 = __fadd_rn(d1, __fmul_rn(t, t));
    t = __fsub_rn(qv[1], a2.y); d2 = __fadd_rn(d2, __fmul_rn(t, t));
    t = __fsub_rn(qv[1], a3.y); d3 = __fadd_rn(d3, __fmul_rn(t, t));
    t = __fsub_rn(qv[2], a0.z); d0 = __fadd_rn(d0, __fmul_rn(t, t));
    t = __fsub_rn(qv[2], a1.z); d1 = __fadd_rn(d1, __fmul_rn(t, t));
    t = __fsub_rn(qv[2], a2.z); d2 = __fadd_rn(d2, __fmul_rn(t, t));
    t = __fsub_rn(qv[2], a3.z); d3 = __fadd_rn(d3, __fmul_rn(t, t));
  } else {
    float4 a0 = *reinterpret_cast<const float4*>(row), a1 = *reinterpret_cast<const float4*>(row + LD),
           a2 = *reinterpret_cast<const float4*>(row + 2 * LD), a3 = *reinterpret_cast<const float4*>(row + 3 * LD);
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      // the next four channels are on their way while these are summed; the scheduling barrier keeps the reads of the whole row
      // from being hoisted to the top of the unrolled body (as in feat_knn_kernel)
      const int cn = c + 4 < C ? c + 4 : c;
      const float4 n0 = *reinterpret_cast<const float4*>(row + cn), n1 = *reinterpret_cast<const float4*>(row + LD + cn),
                   n2 = *reinterpret_cast<const float4*>(row + 2 * LD + cn), n3 = *reinterpret_cast<const float4*>(row + 3 * LD + cn);
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
  }
}

template <int C>
__global__ __launch_bounds__(DK_THREADS) void dgcnn_knn_kernel(const float* __restrict__ feats, int64_t ld,
                                                               const int64_t* __restrict__ piece_off, int64_t P, int64_t N,
                                                               int32_t* __restrict__ out) {
  constexpr int LD = C % 4 == 0 ? C : 4;                     // floats per staged row: a row of 3 is staged as (x, y, z, 0)
  constexpr int TILE_WORDS = 4 * DK_TILE * LD;
  constexpr int LDS_WORDS = TILE_WORDS > DK_MERGE_WORDS ? TILE_WORDS : DK_MERGE_WORDS;
  __shared__ __attribute__((aligned(16))) float s_raw[LDS_WORDS];                    // at most 32 KiB; the tiles, then the merge
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* s_wave = s_raw + wave * DK_TILE * LD;                                       // this wave's tile [DK_TILE][LD]
  // which piece and which block of its queries: pieces take ceil(n / 64) workgroups each, in order
  int64_t b = blockIdx.x, p = 0;
  int64_t base = 0;
  int n = 0;
  for (; p < P; ++p) {
    base = piece_off[p];
    n = (int)(piece_off[p + 1] - base);
    const int64_t nb = (n + DK_QUERIES - 1) / DK_QUERIES;
    if (b < nb) break;
    b -= nb;
  }
  if (p >= P) return;                                        // the grid is an upper bound
  const int q_local = (int)b * DK_QUERIES + lane;
  const bool q_ok = q_local < n;
  const float* qrow = feats + (base + (q_ok ? q_local : n - 1)) * ld;
  float qv[C];
  if constexpr (C % 4 == 0) {
#pragma unroll
    for (int c = 0; c < C / 4; ++c) {
      const float4 v = reinterpret_cast<const float4*>(qrow)[c];
      qv[4 * c] = v.x; qv[4 * c + 1] = v.y; qv[4 * c + 2] = v.z; qv[4 * c + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) qv[c] = qrow[c];
  }
  Top20 top;
#pragma unroll
  for (int s = 0; s < DG_K; ++s) { top.key[s] = 0xFFFFFFFFu; top.idx[s] = (int)N; }
  // wave w walks the candidates [w run, min(n, (w + 1) run)), all waves the same number of steps
  const int run = (n + 3) / 4;
  const int c_lo = wave * run, c_hi = min(n, c_lo + run);
  const int steps = (run + DK_TILE - 1) / DK_TILE;
  for (int st = 0; st < steps; ++st) {
    const int j0 = c_lo + st * DK_TILE;
    __syncthreads();                                         // the previous tile has been read
    if constexpr (C % 4 == 0) {
#pragma unroll
      for (int i = 0; i < DK_TILE * (LD / 4) / 64; ++i) {    // C / 16 float4 per lane
        const int e = i * 64 + lane, r = e / (LD / 4), c4 = e % (LD / 4);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j0 + r < c_hi) v = reinterpret_cast<const float4*>(feats + (base + j0 + r) * ld)[c4];
        reinterpret_cast<float4*>(s_wave + r * LD)[c4] = v;
      }
    } else {
      if (lane < DK_TILE) {                                  // rows of 3 floats are not 16-byte aligned: scalar loads
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j0 + lane < c_hi) {
          const float* src = feats + (base + j0 + lane) * ld;
          v = make_float4(src[0], src[1], src[2], 0.0f);
        }
        reinterpret_cast<float4*>(s_wave)[lane] = v;
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int r0 = 0; r0 < DK_TILE; r0 += 4) {
      if (j0 + r0 >= c_hi) break;                            // wave-uniform
      float d0, d1, d2, d3;                                  // four candidates per pass over the query row
      dist4<C, LD>(qv, s_wave + r0 * LD, d0, d1, d2, d3);
      // a row behind the run gets the key no entry is larger than
      const int j = j0 + r0;
      const unsigned k0 = __float_as_uint(d0);
      const unsigned k1 = j + 1 < c_hi ? __float_as_uint(d1) : 0xFFFFFFFFu;
      const unsigned k2 = j + 2 < c_hi ? __float_as_uint(d2) : 0xFFFFFFFFu;
      const unsigned k3 = j + 3 < c_hi ? __float_as_uint(d3) : 0xFFFFFFFFu;
      // one threshold test for the four: insertions are rare, and all four sums stay in front of the first insertion
      if (min(min(k0, k1), min(k2, k3)) < top.key[DG_K - 1]) {
        top20_insert(top, k0, (int)(base + j));
        top20_insert(top, k1, (int)(base + j + 1));
        top20_insert(top, k2, (int)(base + j + 2));
        top20_insert(top, k3, (int)(base + j + 3));
      }
    }
  }
  // merge: waves 1..3 hand their lists over through LDS; wave 0 takes them in run order (their indices ascend with the wave)
  __syncthreads();
  unsigned* s_key = reinterpret_cast<unsigned*>(s_raw);                              // [3][20][64]
  int* s_idx = reinterpret_cast<int*>(s_key + 3 * DG_K * 64);                        // [3][20][64]
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < DG_K; ++s) {
      s_key[((wave - 1) * DG_K + s) * 64 + lane] = top.key[s];
      s_idx[((wave - 1) * DG_K + s) * 64 + lane] = top.idx[s];
    }
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll 1
  for (int e = 0; e < 3 * DG_K; ++e) top20_insert(top, s_key[e * 64 + lane], s_idx[e * 64 + lane]);
  if (q_ok) {
    int4* o = reinterpret_cast<int4*>(out + (base + q_local) * DG_K);                // 80 bytes per row: 16-byte aligned
#pragma unroll
    for (int s = 0; s < DG_K / 4; ++s) o[s] = make_int4(top.idx[4 * s], top.idx[4 * s + 1], top.idx[4 * s + 2], top.idx[4 * s + 3]);
  }
}

// ------------------------------------------------------------------------------------------------ edge extremum
constexpr int DE_THREADS = 256;

// LPR lanes share a point, four channels each (C_out = 4 LPR): 4, 2 or 1 points per wave
template <int LPR>
__global__ __launch_bounds__(DE_THREADS) void dgcnn_edge_kernel(const float* __restrict__ uv, int64_t ld, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float slope, int64_t N, float* __restrict__ out, int64_t ldo) {
  constexpr int CO = 4 * LPR;
  const int64_t t = (int64_t)blockIdx.x * DE_THREADS + threadIdx.x;
  const int64_t i = t / LPR;
  const int c = 4 * (int)(t % LPR);
  if (i >= N) return;
  int nb[DG_K];
#pragma unroll
  for (int s = 0; s < DG_K / 4; ++s) {
    const int4 v = reinterpret_cast<const int4*>(idx + i * DG_K)[s];
    nb[4 * s] = v.x; nb[4 * s + 1] = v.y; nb[4 * s + 2] = v.z; nb[4 * s + 3] = v.w;
  }
  const float4 v = *reinterpret_cast<const float4*>(uv + i * ld + CO + c);
  float4 u[DG_K];
#pragma unroll
  for (int s = 0; s < DG_K; ++s) {                           // the 20 rows are in flight together; a slot that holds N (or anything
    const bool ok = (unsigned)nb[s] < (unsigned)N;           // outside [0, N)) reads nothing
    u[s] = ok ? *reinterpret_cast<const float4*>(uv + (int64_t)nb[s] * ld + c) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  float4 hi, lo;
#pragma unroll
  for (int s = 0; s < DG_K; ++s) {
    const bool ok = (unsigned)nb[s] < (unsigned)N;
    float4 z;                                                // a padded slot is an all-zero feature row: z = 0, not v
    z.x = ok ? __fadd_rn(u[s].x, v.x) : 0.0f;
    z.y = ok ? __fadd_rn(u[s].y, v.y) : 0.0f;
    z.z = ok ? __fadd_rn(u[s].z, v.z) : 0.0f;
    z.w = ok ? __fadd_rn(u[s].w, v.w) : 0.0f;
    if (s == 0) {
      hi = z; lo = z;
    } else {
      hi.x = z.x > hi.x ? z.x : hi.x; hi.y = z.y > hi.y ? z.y : hi.y; hi.z = z.z > hi.z ? z.z : hi.z; hi.w = z.w > hi.w ? z.w : hi.w;
      lo.x = z.x < lo.x ? z.x : lo.x; lo.y = z.y < lo.y ? z.y : lo.y; lo.z = z.z < lo.z ? z.z : lo.z; lo.w = z.w < lo.w ? z.w : lo.w;
    }
  }
  const float4 sc = *reinterpret_cast<const float4*>(scale + c), sh = *reinterpret_cast<const float4*>(shift + c);
  float4 y;
  y.x = __fadd_rn(__fmul_rn(sc.x >= 0.0f ? hi.x : lo.x, sc.x), sh.x);
  y.y = __fadd_rn(__fmul_rn(sc.y >= 0.0f ? hi.y : lo.y, sc.y), sh.y);
  y.z = __fadd_rn(__fmul_rn(sc.z >= 0.0f ? hi.z : lo.z, sc.z), sh.z);
  y.w = __fadd_rn(__fmul_rn(sc.w >= 0.0f ? hi.w : lo.w, sc.w), sh.w);
  y.x = y.x > 0.0f ? y.x : __fmul_rn(y.x, slope);
  y.y = y.y > 0.0f ? y.y : __fmul_rn(y.y, slope);
  y.z = y.z > 0.0f ? y.z : __fmul_rn(y.z, slope);
  y.w = y.w > 0.0f ? y.w : __fmul_rn(y.w, slope);
  *reinterpret_cast<float4*>(out + i * ldo + c) = y;
}

// ------------------------------------------------------------------------------------------------ LeakyReLU in place
__global__ __launch_bounds__(256) void leaky_relu_kernel(float* __restrict__ x, int64_t rows, int64_t c4n, int64_t ld, float slope) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = t / c4n, c = t % c4n;
  if (r >= rows) return;
  float4* p = reinterpret_cast<float4*>(x + r * ld) + c;
  float4 v = *p;
  v.x = v.x > 0.0f ? v.x : __fmul_rn(v.x, slope);
  v.y = v.y > 0.0f ? v.y : __fmul_rn(v.y, slope);
  v.z = v.z > 0.0f ? v.z : __fmul_rn(v.z, slope);
  v.w = v.w > 0.0f ? v.w : __fmul_rn(v.w, slope);
  *p = v;
}

}  // namespace

extern "C" int pfpp_dgcnn_knn(const float* feats, int64_t ld, const int64_t* piece_off, int64_t P, int64_t N, int64_t C, int64_t K,
                              int64_t max_n, int32_t* idx, pfpp_stream_t stream) {
  PFPP_REQUIRE(P >= 0 && N >= 0 && max_n >= 0 && max_n <= N, "bad sizes");
  PFPP_SUPPORTED(C == 3 || C == 64 || C == 128, "rows of 3, 64 or 128 channels only");
  PFPP_SUPPORTED(K == DG_K, "K must be 20");
  PFPP_SUPPORTED(max_n <= 8192, "a piece of more than 8192 points");
  PFPP_SUPPORTED(N < (1ll << 31) / DG_K, "index range exceeds int32");
  PFPP_SUPPORTED(P <= 65536, "more than 65536 pieces (every workgroup walks the offsets)");
  if (N == 0 || P == 0) return PFPP_OK;
  PFPP_REQUIRE(feats && piece_off && idx, "null pointer");
  PFPP_REQUIRE(ld >= C && pfpp::aligned16(idx), "ld >= C, idx 16-byte aligned");
  PFPP_REQUIRE(C == 3 || (ld % 4 == 0 && pfpp::aligned16(feats)), "rows of 64 / 128 channels must be 16-byte aligned, ld a multiple of 4");
  const int64_t blocks = (N + DK_QUERIES - 1) / DK_QUERIES + P;          // sum over the pieces of ceil(n / 64) is at most this
  const dim3 grid((unsigned)blocks), block(DK_THREADS);
  hipStream_t s = pfpp::as_stream(stream);
  if (C == 3) hipLaunchKernelGGL(dgcnn_knn_kernel<3>, grid, block, 0, s, feats, ld, piece_off, P, N, idx);
  else if (C == 64) hipLaunchKernelGGL(dgcnn_knn_kernel<64>, grid, block, 0, s, feats, ld, piece_off, P, N, idx);
  else hipLaunchKernelGGL(dgcnn_knn_kernel<128>, grid, block, 0, s, feats, ld, piece_off, P, N, idx);
  return pfpp::check_launch("pfpp_dgcnn_knn");
}

extern "C" int pfpp_dgcnn_edge_max(const float* uv, int64_t ld, const int32_t* idx, const float* scale, const float* shift, float slope,
                                   int64_t N, int64_t C_out, int64_t K, float* out, int64_t ldo, pfpp_stream_t stream) {
  PFPP_REQUIRE(N >= 0, "bad sizes");
  PFPP_SUPPORTED(C_out == 64 || C_out == 128 || C_out == 256, "64, 128 or 256 output channels only");
  PFPP_SUPPORTED(K == DG_K, "K must be 20");
  PFPP_SUPPORTED(N < (1ll << 31) / DG_K, "index range exceeds int32");
  if (N == 0) return PFPP_OK;
  PFPP_REQUIRE(uv && idx && scale && shift && out, "null pointer");
  PFPP_REQUIRE(ld >= 2 * C_out && ld % 4 == 0 && ldo >= C_out && ldo % 4 == 0, "ld >= 2 C_out, ldo >= C_out, both multiples of 4");
  PFPP_REQUIRE(pfpp::aligned16(uv) && pfpp::aligned16(idx) && pfpp::aligned16(scale) && pfpp::aligned16(shift) && pfpp::aligned16(out),
               "16-byte alignment");
  const int64_t lpr = C_out / 4;
  const dim3 grid((unsigned)((N * lpr + DE_THREADS - 1) / DE_THREADS)), block(DE_THREADS);
  hipStream_t s = pfpp::as_stream(stream);
  if (C_out == 64) hipLaunchKernelGGL(dgcnn_edge_kernel<16>, grid, block, 0, s, uv, ld, idx, scale, shift, slope, N, out, ldo);
  else if (C_out == 128) hipLaunchKernelGGL(dgcnn_edge_kernel<32>, grid, block, 0, s, uv, ld, idx, scale, shift, slope, N, out, ldo);
  else hipLaunchKernelGGL(dgcnn_edge_kernel<64>, grid, block, 0, s, uv, ld, idx, scale, shift, slope, N, out, ldo);
  return pfpp::check_launch("pfpp_dgcnn_edge_max");
}

extern "C" int pfpp_leaky_relu(float* x, int64_t rows, int64_t C, int64_t ld, float slope, pfpp_stream_t stream) {
  PFPP_REQUIRE(rows >= 0 && C >= 0, "bad sizes");
  if (rows == 0 || C == 0) return PFPP_OK;
  PFPP_REQUIRE(x, "null pointer");
  PFPP_REQUIRE(C % 4 == 0 && ld >= C && ld % 4 == 0 && pfpp::aligned16(x), "C and ld multiples of 4, ld >= C, x 16-byte aligned");
  const int64_t blocks = (rows * (C / 4) + 255) / 256;
  PFPP_SUPPORTED(blocks < (1ll << 31), "grid too large");
  hipLaunchKernelGGL(leaky_relu_kernel, dim3((unsigned)blocks), dim3(256), 0, pfpp::as_stream(stream), x, rows, C / 4, ld, slope);
  return pfpp::check_launch("pfpp_leaky_relu");
}
