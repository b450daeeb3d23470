// Ragged PointNet++ encoder of the matcher (Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/pointnet2_msg.py:48-94,
// pointnet2_dynamic_utils.py): the pieces of any number of puzzles flat in one call, described by CSR offsets.  Nothing is padded
// to the largest piece and nothing looks at which puzzle a piece belongs to.
//
//  * ragged_fps_kernel — torch_cluster.fps(ratio, batch) for all levels of the encoder in one launch: one workgroup per piece
//    walks the piece through the levels (level l + 1 samples the centroids of level l, which the same workgroup wrote).  The
//    arithmetic is fps_kernel's: d = (dx dx + dy dy) + dz dz in fp32 without contraction, running minimum, first argmax.  The
//    points and their running minima live in registers; one barrier per selection.
//  * ragged_knn_kernel — knn(x, y, k, batch_x, batch_y) + to_dense_batch + the `group_first` fix-up: one wave per query selects
//    the min(K, n) nearest points of the query's piece one at a time as the smallest (distance bits, index) key above the last
//    one, so the result is ascending by distance with ties to the lower index; the remaining slots repeat the first.
//  * ragged_group_kernel — the grouped rows [points[idx] | xyz[idx] - new_xyz[s] | 0] of a set-abstraction scale, `pool` rows per
//    centroid (slot j reads neighbour j mod K: a maximum does not see the duplicates of a K = 16 scale in a pool of 32).
//  * ragged_interp_kernel — PointNetFeaturePropagationDynamic's inverse-distance interpolation in the reference's form and order,
//    written next to points1 as the A operand of the level's first linear layer.
// No atomics anywhere: two runs agree bitwise.
#include "pfpp_common.h"

namespace {

constexpr int FPS_THREADS = 256;
constexpr int FPS_WAVES = FPS_THREADS / 64;

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------------ farthest point sampling
// off: [L + 1][P + 1] CSR offsets of the levels (row 0: the input points); start: [L][P] local first index per level and piece;
// idx / new_xyz: the levels' outputs one behind the other (level l at element offset sum_{j < l} off[j + 1][P]).
template <int PT>
__global__ __launch_bounds__(FPS_THREADS) void ragged_fps_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ off,
                                                                 const int64_t* __restrict__ start, int64_t P, int L, int64_t* idx,
                                                                 float* new_xyz) {
  __shared__ unsigned long long s_key[2][FPS_WAVES];
  __shared__ float s_xyz[2][FPS_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t p = blockIdx.x;
  const float* src = xyz;
  int64_t out_base = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t* off_in = off + (int64_t)l * (P + 1);
    const int64_t* off_out = off_in + (P + 1);
    const int64_t in0 = off_in[p], o0 = off_out[p];
    const int n = (int)(off_in[p + 1] - in0), m = (int)(off_out[p + 1] - o0);
    float px[PT], py[PT], pz[PT], dist[PT];
#pragma unroll
    for (int k = 0; k < PT; ++k) {
      const int i = k * FPS_THREADS + tid;
      const bool ok = i < n;
      const float* q = src + (in0 + (ok ? i : 0)) * 3;
      px[k] = (ok && n > 0) ? q[0] : 0.0f;
      py[k] = (ok && n > 0) ? q[1] : 0.0f;
      pz[k] = (ok && n > 0) ? q[2] : 0.0f;
      dist[k] = __builtin_huge_valf();
    }
    int cur = 0;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (m > 0) {
      cur = (int)start[(int64_t)l * P + p];
      cur = cur < 0 ? 0 : (cur >= n ? n - 1 : cur);       // memory safety only: the caller validates the start indices
      const float* q = src + (in0 + cur) * 3;
      cx = q[0]; cy = q[1]; cz = q[2];
    }
    int64_t* o_idx = idx + out_base + o0;
    float* o_xyz = new_xyz + (out_base + o0) * 3;
    for (int s = 0; s < m; ++s) {
      if (tid == 0) {
        o_idx[s] = in0 + cur;
        o_xyz[3 * s] = cx; o_xyz[3 * s + 1] = cy; o_xyz[3 * s + 2] = cz;
      }
      if (s + 1 == m) break;
      unsigned long long best = 0;                         // (distance bits, ~index): the maximum is the first argmax
      float bx = 0.0f, by = 0.0f, bz = 0.0f;
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        const int i = k * FPS_THREADS + tid;
        if (i < n) {
          const float dx = px[k] - cx, dy = py[k] - cy, dz = pz[k] - cz;
          const float d = (dx * dx + dy * dy) + dz * dz;
          dist[k] = fminf(dist[k], d);
          const unsigned long long key = ((unsigned long long)__float_as_uint(dist[k]) << 32) | (0xFFFFFFFFu - (unsigned)i);
          if (key > best) { best = key; bx = px[k]; by = py[k]; bz = pz[k]; }
        }
      }
      unsigned long long w = best;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = shfl_xor_u64(w, o);
        w = t > w ? t : w;
      }
      // the lane that owns the wave's winner hands over its coordinates (keys are unique: they hold the index)
      const unsigned long long own = __ballot(best == w && best != 0);
      const int src_lane = own ? __builtin_ctzll(own) : 0;
      const float wx = __shfl(bx, src_lane, 64), wy = __shfl(by, src_lane, 64), wz = __shfl(bz, src_lane, 64);
      const int buf = s & 1;
      if (lane == 0) {
        s_key[buf][wave] = w;
        s_xyz[buf][wave][0] = wx; s_xyz[buf][wave][1] = wy; s_xyz[buf][wave][2] = wz;
      }
      __syncthreads();
      unsigned long long g = s_key[buf][0];
      int gw = 0;
#pragma unroll
      for (int v = 1; v < FPS_WAVES; ++v) {
        const unsigned long long t = s_key[buf][v];
        if (t > g) { g = t; gw = v; }
      }
      cur = (int)(0xFFFFFFFFu - (unsigned)(g & 0xFFFFFFFFu));
      cx = s_xyz[buf][gw][0]; cy = s_xyz[buf][gw][1]; cz = s_xyz[buf][gw][2];
    }
    out_base += off_out[P];
    src = new_xyz + (out_base - off_out[P]) * 3;          // the next level samples this level's centroids
    __threadfence_block();
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ k nearest neighbours in a piece
__device__ __forceinline__ int64_t csr_find(const int64_t* __restrict__ off, int64_t P, int64_t r) {
  int64_t lo = 0, hi = P;                                  // the piece with off[p] <= r < off[p + 1] (empty pieces are skipped)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void ragged_knn_kernel(const float* __restrict__ pts, const int64_t* __restrict__ pts_off,
                                                         const float* __restrict__ qry, const int64_t* __restrict__ qry_off, int64_t P,
                                                         int64_t M, int K, int32_t* __restrict__ out, int32_t* __restrict__ cnt_out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= M) return;
  const int64_t p = csr_find(qry_off, P, q);
  const int64_t base = pts_off[p];
  const int n = (int)(pts_off[p + 1] - base);
  const float qx = qry[3 * q], qy = qry[3 * q + 1], qz = qry[3 * q + 2];
  const int real = n < K ? n : K;
  unsigned long long last = 0;
  int first = 0;
  for (int r = 0; r < real; ++r) {
    unsigned long long best = ~0ull;
    for (int i = lane; i < n; i += 64) {
      const float* c = pts + (base + i) * 3;
      const float dx = c[0] - qx, dy = c[1] - qy, dz = c[2] - qz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
      if ((r == 0 || key > last) && key < best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long t = shfl_xor_u64(best, o);
      best = t < best ? t : best;
    }
    last = best;
    const int g = (int)(base + (int64_t)(best & 0xFFFFFFFFu));
    if (r == 0) first = g;
    if (lane == 0) out[q * K + r] = g;
  }
  for (int r = real + lane; r < K; r += 64) out[q * K + r] = first;
  if (cnt_out && lane == 0) cnt_out[q] = real;
}

// ------------------------------------------------------------------------------------------------ grouping
__global__ __launch_bounds__(256) void ragged_group_kernel(const float* __restrict__ feats, int64_t ldf, int D, const float* __restrict__ xyz,
                                                           const float* __restrict__ new_xyz, const int32_t* __restrict__ idx, int64_t ldi,
                                                           int K, int pool, int64_t S, float* __restrict__ out, int ldo) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= S * pool * ldo) return;
  const int c = (int)(e % ldo);
  const int64_t row = e / ldo, s = row / pool;
  const int j = (int)(row % pool) % K;
  const int64_t g = idx[s * ldi + j];
  float v = 0.0f;
  if (c < D) v = feats[g * ldf + c];
  else if (c < D + 3) v = xyz[g * 3 + (c - D)] - new_xyz[s * 3 + (c - D)];
  out[e] = v;
}

// ------------------------------------------------------------------------------------------------ feature propagation
__device__ __forceinline__ float fp_dist(const float* a, const float* b) {
  // the reference's expression per coordinate, (a a + b b) - (2 a) b, the three summed in order (no contraction in this unit)
  const float t0 = (a[0] * a[0] + b[0] * b[0]) - (2.0f * a[0]) * b[0];
  const float t1 = (a[1] * a[1] + b[1] * b[1]) - (2.0f * a[1]) * b[1];
  const float t2 = (a[2] * a[2] + b[2] * b[2]) - (2.0f * a[2]) * b[2];
  return (t0 + t1) + t2;
}

__global__ __launch_bounds__(256) void ragged_interp_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                            const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt,
                                                            const float* __restrict__ points2, int D2, const float* __restrict__ points1,
                                                            int D1, int64_t N, int broadcast, float* __restrict__ out, int64_t ldo,
                                                            float* __restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  float4* orow = reinterpret_cast<float4*>(out + i * ldo);
  if (points1) {
    const float4* prow = reinterpret_cast<const float4*>(points1 + i * D1);
    for (int c = lane; c < D1 / 4; c += 64) orow[c] = prow[c];
  }
  orow += D1 / 4;
  if (broadcast) {                                         // the whole call has one centroid (:191-192)
    const float4* r0 = reinterpret_cast<const float4*>(points2);
    for (int c = lane; c < D2 / 4; c += 64) orow[c] = r0[c];
    if (weights && lane < 3) weights[3 * i + lane] = lane == 0 ? 1.0f : 0.0f;
    return;
  }
  const int real = cnt[i];
  int g[3];
  float w[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    g[j] = idx[3 * i + j];
    const float d = j < real ? fp_dist(xyz1 + 3 * i, xyz2 + 3 * (int64_t)g[j]) : 1e8f;      // to_dense_batch(fill_value=1e8)
    w[j] = 1.0f / (d + 1e-8f);
  }
  const float norm = (w[0] + w[1]) + w[2];
  w[0] = w[0] / norm; w[1] = w[1] / norm; w[2] = w[2] / norm;
  if (weights && lane < 3) weights[3 * i + lane] = lane == 0 ? w[0] : (lane == 1 ? w[1] : w[2]);
  const float4* r0 = reinterpret_cast<const float4*>(points2 + (int64_t)g[0] * D2);
  const float4* r1 = reinterpret_cast<const float4*>(points2 + (int64_t)g[1] * D2);
  const float4* r2 = reinterpret_cast<const float4*>(points2 + (int64_t)g[2] * D2);
  for (int c = lane; c < D2 / 4; c += 64) {
    const float4 a = r0[c], b = r1[c], d = r2[c];
    float4 y;
    y.x = (a.x * w[0] + b.x * w[1]) + d.x * w[2];
    y.y = (a.y * w[0] + b.y * w[1]) + d.y * w[2];
    y.z = (a.z * w[0] + b.z * w[1]) + d.z * w[2];
    y.w = (a.w * w[0] + b.w * w[1]) + d.w * w[2];
    orow[c] = y;
  }
}

template <int PT>
int launch_fps(const float* xyz, const int64_t* off, const int64_t* start, int64_t P, int L, int64_t* idx, float* new_xyz, hipStream_t st) {
  hipLaunchKernelGGL(ragged_fps_kernel<PT>, dim3((unsigned)P), dim3(FPS_THREADS), 0, st, xyz, off, start, P, L, idx, new_xyz);
  return pfpp::check_launch("pfpp_ragged_fps");
}

}  // namespace

extern "C" int pfpp_ragged_fps(const float* xyz, const int64_t* level_off, const int64_t* start, int64_t P, int64_t L, int64_t max_n,
                               int64_t* idx, float* new_xyz, pfpp_stream_t stream) {
  PFPP_REQUIRE(P >= 0 && L >= 1 && L <= 8 && max_n >= 0, "bad sizes");
  if (P == 0 || max_n == 0) return PFPP_OK;
  PFPP_REQUIRE(xyz && level_off && start && idx && new_xyz, "null pointer");
  PFPP_SUPPORTED(max_n <= 32 * FPS_THREADS, "a piece of more than 8192 points");
  PFPP_SUPPORTED(P < (1ll << 31), "more than 2^31 pieces");
  hipStream_t st = pfpp::as_stream(stream);
  if (max_n <= 2 * FPS_THREADS) return launch_fps<2>(xyz, level_off, start, P, (int)L, idx, new_xyz, st);
  if (max_n <= 8 * FPS_THREADS) return launch_fps<8>(xyz, level_off, start, P, (int)L, idx, new_xyz, st);
  if (max_n <= 20 * FPS_THREADS) return launch_fps<20>(xyz, level_off, start, P, (int)L, idx, new_xyz, st);
  return launch_fps<32>(xyz, level_off, start, P, (int)L, idx, new_xyz, st);
}

extern "C" int pfpp_ragged_knn(const float* pts, const int64_t* pts_off, const float* queries, const int64_t* query_off, int64_t P,
                               int64_t M, int64_t N, int64_t K, int32_t* idx, int32_t* count, pfpp_stream_t stream) {
  PFPP_REQUIRE(P >= 0 && M >= 0 && N >= 0, "bad sizes");
  PFPP_SUPPORTED(K == 3 || K == 16 || K == 32, "K must be 3, 16 or 32");
  PFPP_SUPPORTED(N < (1ll << 31) && M < (1ll << 31) / 32, "index range exceeds int32");
  if (M == 0) return PFPP_OK;
  PFPP_REQUIRE(pts && pts_off && queries && query_off && idx && P > 0, "null pointer");
  hipLaunchKernelGGL(ragged_knn_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), pts, pts_off, queries,
                     query_off, P, M, (int)K, idx, count);
  return pfpp::check_launch("pfpp_ragged_knn");
}

extern "C" int pfpp_ragged_group(const float* feats, int64_t ldf, int64_t D, const float* xyz, const float* new_xyz, const int32_t* idx,
                                 int64_t ldi, int64_t K, int64_t pool, int64_t S, float* out, int64_t ldo, pfpp_stream_t stream) {
  PFPP_REQUIRE(S >= 0 && D >= 0 && K >= 1 && ldi >= K && pool >= K && pool % K == 0, "bad sizes");
  PFPP_REQUIRE(ldo >= D + 3 && ldo % 4 == 0 && ldf >= D, "ldo must hold D + 3 columns and be a multiple of 4");
  PFPP_SUPPORTED(ldo < (1ll << 20) && S * pool < (1ll << 31), "sizes exceed the kernel's index range");
  if (S == 0) return PFPP_OK;
  PFPP_REQUIRE((feats || D == 0) && xyz && new_xyz && idx && out, "null pointer");
  const int64_t total = S * pool * ldo;
  PFPP_SUPPORTED((total + 255) / 256 < (1ll << 31), "grid too large");
  hipLaunchKernelGGL(ragged_group_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pfpp::as_stream(stream), feats, ldf, (int)D,
                     xyz, new_xyz, idx, ldi, (int)K, (int)pool, S, out, (int)ldo);
  return pfpp::check_launch("pfpp_ragged_group");
}

extern "C" int pfpp_ragged_interp(const float* xyz1, const float* xyz2, const int32_t* idx, const int32_t* count, const float* points2,
                                  int64_t D2, const float* points1, int64_t D1, int64_t N, int64_t S, float* out, int64_t ldo,
                                  float* weights, pfpp_stream_t stream) {
  PFPP_REQUIRE(N >= 0 && S >= 0 && D1 >= 0 && D2 > 0, "bad sizes");
  PFPP_REQUIRE(D1 % 4 == 0 && D2 % 4 == 0 && ldo % 4 == 0 && ldo >= D1 + D2, "D1, D2 and ldo must be multiples of 4, ldo >= D1 + D2");
  PFPP_SUPPORTED(D1 < (1 << 20) && D2 < (1 << 20) && N < (1ll << 31) && S < (1ll << 31), "sizes exceed the kernel's index range");
  if (N == 0) return PFPP_OK;
  PFPP_REQUIRE(S >= 1, "no centroid to interpolate from");
  PFPP_REQUIRE(xyz1 && xyz2 && points2 && out && (points1 || D1 == 0) && (S == 1 || (idx && count)), "null pointer");
  PFPP_REQUIRE(pfpp::aligned16(points2) && pfpp::aligned16(out) && (!points1 || pfpp::aligned16(points1)), "rows must be 16-byte aligned");
  hipLaunchKernelGGL(ragged_interp_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), xyz1, xyz2, idx, count,
                     points2, (int)D2, points1, (int)D1, N, S == 1 ? 1 : 0, out, ldo, weights);
  return pfpp::check_launch("pfpp_ragged_interp");
}
