// Evaluating the matcher: piece-pair poses by RANSAC over the matched critical points, and the ragged nearest-neighbour distance of
// the chamfer metrics (Jigsaw_matching/utils/estimate_transform.py:8-66 called at model/modules/matching_base_model.py:338, and
// utils/eval_utils.py).  The reference hands one pair at a time to open3d's registration_ransac_based_on_correspondence on the
// host (ransac_n = 3, up to 50,000 draws); here every hypothesis of every pair of a batch is scored in one launch.
//
//  * ransac_score_kernel — grid (ceil(H / 256), E), a hypothesis per lane.  Hypothesis h of pair e draws three distinct
//    correspondences from Philox4x32-10 (key = the seed's halves, counter = (h, e, 0, 0)), solves Horn's closed form on them with
//    unit weights (horn_common.h, fp64) and counts the correspondences with |R S_k + t - T_k|^2 < max_dist^2, summing the inliers'
//    squared distances in correspondence order.  The pair's matched points are staged in LDS as fp32, RP_TILE correspondences at a
//    time; every lane reads the same address (a broadcast).  A hypothesis whose two largest eigenvalues are closer than 1e-9 max|N|
//    (collinear or repeated points) scores -1.  The workgroup's winner - largest count, then smallest sumsq, then smallest h, a
//    total order, so the shape of the reduction cannot matter - goes to the workspace.
//  * ransac_finish_kernel — a wave per pair: the winner over the workgroups' winners under the same order, its pose once more,
//    optionally one more Horn over its inliers (refine), R and t rounded to fp32.  Where every hypothesis is degenerate: R = 1,
//    t = cT - cS over all correspondences.
//  * nn_dist_ragged_kernel — pfpp_nn_dist (metrics.hip) over segments of unequal sizes, its arithmetic bit for bit.
// fp64 sums in a fixed order, no float atomics, nothing read from the environment: two runs agree bitwise.
#include "pfpp_common.h"
#include "horn_common.h"

namespace {

constexpr int RP_TILE = PFPP_RANSAC_TILE;      // correspondences staged per step: 6 floats each, 24 KiB
constexpr int RP_WG = 256;                     // hypotheses per workgroup
constexpr double RP_GAP = 1e-9;                // relative eigen-gap under which a hypothesis is degenerate

struct RpBest {                                // a workgroup's (or lane's) winner; 16 bytes
  double sumsq;
  int32_t count;                               // -1: degenerate, -2: no hypothesis
  int32_t h;
};

__device__ __forceinline__ bool rp_better(int ca, double sa, int ha, int cb, double sb, int hb) {
  return ca > cb || (ca == cb && (sa < sb || (sa == sb && ha < hb)));
}

__device__ __forceinline__ double rp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, 0, 0), key (k0, k1) -> the first three words of the output
__device__ __forceinline__ void rp_philox3(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t (&x)[3]) {
  uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2;
}

// three distinct indices below M >= 3 from three words, integer only
__device__ __forceinline__ void rp_draw(uint32_t M, const uint32_t (&x)[3], int (&idx)[3]) {
  const uint32_t i0 = __umulhi(x[0], M);
  uint32_t i1 = __umulhi(x[1], M - 1u);
  if (i1 >= i0) ++i1;
  uint32_t i2 = __umulhi(x[2], M - 2u);
  const uint32_t lo = min(i0, i1), hi = max(i0, i1);
  if (i2 >= lo) ++i2;
  if (i2 >= hi) ++i2;
  idx[0] = (int)i0; idx[1] = (int)i1; idx[2] = (int)i2;
}

// row of pts of a correspondence's end, clamped into [0, R) (memory safety only: the wrapper checks the indices)
__device__ __forceinline__ int64_t rp_row(int64_t off, int32_t i, int64_t R) { return min(max(off + (int64_t)i, (int64_t)0), R - 1); }

// Horn on centred sums: M -> (Rd, degenerate).  nmax = max |N_ij|
__device__ __forceinline__ bool rp_solve(const double (&M)[3][3], double (&Rd)[3][3]) {
  double A[4][4], V[4][4], ev[4], qv[4];
  rg_horn_n(M, A);
  double nmax = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = a; c < 4; ++c) nmax = fmax(nmax, fabs(A[a][c]));
  const int kb = rg_top_eigenvector(A, V, ev, qv);
  rg_quat_rot(qv, Rd);
  double second = -__builtin_huge_val();
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k != kb) second = fmax(second, ev[k]);
  return !(ev[kb] - second > RP_GAP * nmax);
}

// the pose of hypothesis h of pair e: -> Rd, td (fp64); returns true when it is degenerate
__device__ __forceinline__ bool rp_triple_pose(const float* __restrict__ pts, int64_t R, int64_t so, int64_t to, const int32_t* __restrict__ corr,
                                               uint32_t M, uint32_t k0, uint32_t k1, uint32_t h, uint32_t e, double (&Rd)[3][3],
                                               double (&td)[3]) {
  uint32_t x[3];
  int idx[3];
  rp_philox3(h, e, k0, k1, x);
  rp_draw(M, x, idx);
  double s[3][3], t[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t rs = rp_row(so, corr[2 * (int64_t)idx[k]], R), rt = rp_row(to, corr[2 * (int64_t)idx[k] + 1], R);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[k][a] = (double)pts[3 * rs + a];
      t[k][a] = (double)pts[3 * rt + a];
    }
  }
  double cS[3], cT[3], Mm[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cS[a] = ((s[0][a] + s[1][a]) + s[2][a]) / 3.0;
    cT[a] = ((t[0][a] + t[1][a]) + t[2][a]) / 3.0;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Mm[a][c] = ((s[0][a] - cS[a]) * (t[0][c] - cT[c]) + (s[1][a] - cS[a]) * (t[1][c] - cT[c])) + (s[2][a] - cS[a]) * (t[2][c] - cT[c]);
  const bool deg = rp_solve(Mm, Rd);
#pragma unroll
  for (int a = 0; a < 3; ++a) td[a] = cT[a] - ((Rd[a][0] * cS[0] + Rd[a][1] * cS[1]) + Rd[a][2] * cS[2]);
  return deg;
}

__device__ __forceinline__ double rp_dist2(const double (&Rd)[3][3], const double (&td)[3], double sx, double sy, double sz, double tx, double ty,
                                           double tz) {
  const double dx = ((((Rd[0][0] * sx + Rd[0][1] * sy) + Rd[0][2] * sz) + td[0]) - tx);
  const double dy = ((((Rd[1][0] * sx + Rd[1][1] * sy) + Rd[1][2] * sz) + td[1]) - ty);
  const double dz = ((((Rd[2][0] * sx + Rd[2][1] * sy) + Rd[2][2] * sz) + td[2]) - tz);
  return (dx * dx + dy * dy) + dz * dz;
}

// grid (nblk = ceil(H / 256), E).  pair_off int64 [E, 2] = the first rows of the pair's source and target pieces in pts [R, 3];
// corr int32 [corr_off[E], 2] = (i, j) piece-local; wg_best [E, nblk]; counts_out int32 [E, H] or null
__global__ __launch_bounds__(RP_WG) void ransac_score_kernel(const float* __restrict__ pts, int64_t R, const int64_t* __restrict__ pair_off,
                                                             const int32_t* __restrict__ corr, const int64_t* __restrict__ corr_off, int H,
                                                             double max_d2, uint32_t k0, uint32_t k1, RpBest* __restrict__ wg_best,
                                                             int32_t* __restrict__ counts_out) {
  __shared__ float sp[RP_TILE][6];
  __shared__ RpBest sbest[RP_WG / 64];
  const int tid = threadIdx.x, e = blockIdx.y;
  const int64_t h64 = (int64_t)blockIdx.x * RP_WG + tid;
  const bool live = h64 < H;
  const int h = live ? (int)h64 : 0;
  const int64_t so = pair_off[2 * e], to = pair_off[2 * e + 1], c0 = corr_off[e];
  const int M = (int)(corr_off[e + 1] - c0);
  const int32_t* cp = corr + 2 * c0;
  if (M < 3) {                                                       // uniform; no triple to draw (the wrapper refuses such a pair)
    if (live && counts_out) counts_out[(int64_t)e * H + h] = -1;
    if (tid == 0) {
      RpBest b;
      b.sumsq = 0.0; b.count = -1; b.h = h;
      wg_best[(int64_t)e * gridDim.x + blockIdx.x] = b;
    }
    return;
  }
  double Rd[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, td[3] = {0.0, 0.0, 0.0};
  bool deg = false;
  if (live) deg = rp_triple_pose(pts, R, so, to, cp, (uint32_t)M, k0, k1, (uint32_t)h, (uint32_t)e, Rd, td);      // lanes past H only stage
  int count = 0;
  double sumsq = 0.0;
  for (int m0 = 0; m0 < M; m0 += RP_TILE) {
    const int cnt = min(RP_TILE, M - m0);
    __syncthreads();
    for (int k = tid; k < cnt; k += RP_WG) {
      const int64_t rs = rp_row(so, cp[2 * (int64_t)(m0 + k)], R), rt = rp_row(to, cp[2 * (int64_t)(m0 + k) + 1], R);
      sp[k][0] = pts[3 * rs]; sp[k][1] = pts[3 * rs + 1]; sp[k][2] = pts[3 * rs + 2];
      sp[k][3] = pts[3 * rt]; sp[k][4] = pts[3 * rt + 1]; sp[k][5] = pts[3 * rt + 2];
    }
    __syncthreads();
    const int mine = live ? cnt : 0;
    for (int k = 0; k < mine; ++k) {
      const double d2 = rp_dist2(Rd, td, (double)sp[k][0], (double)sp[k][1], (double)sp[k][2], (double)sp[k][3], (double)sp[k][4], (double)sp[k][5]);
      if (d2 < max_d2) {
        ++count;
        sumsq += d2;
      }
    }
  }
  if (deg) { count = -1; sumsq = 0.0; }
  if (!live) { count = -2; sumsq = 0.0; }
  if (live && counts_out) counts_out[(int64_t)e * H + h] = count;
  // the workgroup's winner: a butterfly over the wave, then the four waves' winners in order
  int bc = count, bh = h;
  double bs = sumsq;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
    const double os = __shfl_xor(bs, o, 64);
    if (rp_better(oc, os, oh, bc, bs, bh)) { bc = oc; bs = os; bh = oh; }
  }
  if ((tid & 63) == 0) { sbest[tid >> 6].count = bc; sbest[tid >> 6].sumsq = bs; sbest[tid >> 6].h = bh; }
  __syncthreads();
  if (tid == 0) {
    RpBest b = sbest[0];
#pragma unroll
    for (int w = 1; w < RP_WG / 64; ++w)
      if (rp_better(sbest[w].count, sbest[w].sumsq, sbest[w].h, b.count, b.sumsq, b.h)) b = sbest[w];
    wg_best[(int64_t)e * gridDim.x + blockIdx.x] = b;
  }
}

// grid (E), a wave per pair.  stats fp64 [E, 2] = (sumsq of the winner, inliers the refinement used); info int32 [E, 3] = (best h,
// count, status): status bit 0 = a non-degenerate winner exists, bit 1 = the pose is the refined one
__global__ __launch_bounds__(64) void ransac_finish_kernel(const float* __restrict__ pts, int64_t R, const int64_t* __restrict__ pair_off,
                                                           const int32_t* __restrict__ corr, const int64_t* __restrict__ corr_off, int nblk,
                                                           double max_d2, uint32_t k0, uint32_t k1, int refine,
                                                           const RpBest* __restrict__ wg_best, float* __restrict__ Rout, float* __restrict__ tout,
                                                           double* __restrict__ stats, int32_t* __restrict__ info) {
  const int lane = threadIdx.x, e = blockIdx.x;
  const int64_t so = pair_off[2 * e], to = pair_off[2 * e + 1], c0 = corr_off[e];
  const int M = (int)(corr_off[e + 1] - c0);
  const int32_t* cp = corr + 2 * c0;
  int bc = -2, bh = 0x7fffffff;
  double bs = 0.0;
  for (int k = lane; k < nblk; k += 64) {
    const RpBest b = wg_best[(int64_t)e * nblk + k];
    if (rp_better(b.count, b.sumsq, b.h, bc, bs, bh)) { bc = b.count; bs = b.sumsq; bh = b.h; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
    const double os = __shfl_xor(bs, o, 64);
    if (rp_better(oc, os, oh, bc, bs, bh)) { bc = oc; bs = os; bh = oh; }
  }
  double Rd[3][3], td[3];
  int status = 0;
  double n_ref = 0.0;
  if (bc >= 0) {                                                     // uniform: every lane holds the same winner
    status = 1;
    (void)rp_triple_pose(pts, R, so, to, cp, (uint32_t)M, k0, k1, (uint32_t)bh, (uint32_t)e, Rd, td);
  } else {                                                           // every hypothesis degenerate: R = 1, t = cT - cS over all
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < M; k += 64) {
      const int64_t rs = rp_row(so, cp[2 * (int64_t)k], R), rt = rp_row(to, cp[2 * (int64_t)k + 1], R);
#pragma unroll
      for (int c = 0; c < 3; ++c) { a[c] += (double)pts[3 * rs + c]; a[3 + c] += (double)pts[3 * rt + c]; }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) a[c] = M > 0 ? rp_wave_sum(a[c]) / (double)M : 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      td[r] = a[3 + r] - a[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) Rd[r][c] = r == c ? 1.0 : 0.0;
    }
    bh = -1; bc = -1; bs = 0.0;
  }
  if (refine && status == 1) {                                       // one more Horn over the winner's inliers, unit weights
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < M; k += 64) {
      const int64_t rs = rp_row(so, cp[2 * (int64_t)k], R), rt = rp_row(to, cp[2 * (int64_t)k + 1], R);
      double p[6];
#pragma unroll
      for (int c = 0; c < 3; ++c) { p[c] = (double)pts[3 * rs + c]; p[3 + c] = (double)pts[3 * rt + c]; }
      if (rp_dist2(Rd, td, p[0], p[1], p[2], p[3], p[4], p[5]) < max_d2) {
#pragma unroll
        for (int c = 0; c < 6; ++c) a[c] += p[c];
        a[6] += 1.0;
      }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) a[c] = rp_wave_sum(a[c]);
    n_ref = a[6];
    if (n_ref >= 3.0) {                                              // uniform
      double cS[3], cT[3], Mm[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
      for (int c = 0; c < 3; ++c) { cS[c] = a[c] / n_ref; cT[c] = a[3 + c] / n_ref; }
      for (int k = lane; k < M; k += 64) {
        const int64_t rs = rp_row(so, cp[2 * (int64_t)k], R), rt = rp_row(to, cp[2 * (int64_t)k + 1], R);
        double p[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) { p[c] = (double)pts[3 * rs + c]; p[3 + c] = (double)pts[3 * rt + c]; }
        if (rp_dist2(Rd, td, p[0], p[1], p[2], p[3], p[4], p[5]) < max_d2) {
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Mm[r][c] += (p[r] - cS[r]) * (p[3 + c] - cT[c]);
        }
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Mm[r][c] = rp_wave_sum(Mm[r][c]);
      double R2[3][3];
      if (!rp_solve(Mm, R2)) {                                       // a degenerate inlier set keeps the three-point pose
        status |= 2;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) Rd[r][c] = R2[r][c];
          td[r] = cT[r] - ((R2[r][0] * cS[0] + R2[r][1] * cS[1]) + R2[r][2] * cS[2]);
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      tout[3 * (int64_t)e + r] = (float)td[r];
#pragma unroll
      for (int c = 0; c < 3; ++c) Rout[9 * (int64_t)e + 3 * r + c] = (float)Rd[r][c];
    }
    stats[2 * (int64_t)e] = bs;
    stats[2 * (int64_t)e + 1] = n_ref;
    info[3 * (int64_t)e] = bh;
    info[3 * (int64_t)e + 1] = bc;
    info[3 * (int64_t)e + 2] = status;
  }
}

// ------------------------------------------------------------------------------------------------ ragged nearest distance
constexpr int NNR_TILE = 1024;

// grid (ceil(max_n / 256), S): nn_dist_kernel (metrics.hip) with a segment per blockIdx.y
__global__ __launch_bounds__(256) void nn_dist_ragged_kernel(const float* __restrict__ src, const int64_t* __restrict__ src_off,
                                                             const float* __restrict__ dst, const int64_t* __restrict__ dst_off,
                                                             float* __restrict__ out) {
  __shared__ float tx[NNR_TILE], ty[NNR_TILE], tz[NNR_TILE];
  const int64_t s0 = src_off[blockIdx.y], n = src_off[blockIdx.y + 1] - s0;
  const int64_t d0 = dst_off[blockIdx.y], m = dst_off[blockIdx.y + 1] - d0;
  if ((int64_t)blockIdx.x * 256 >= n) return;                         // uniform: nothing of this segment in this block
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float* s = src + 3 * s0;
  const float* d = dst + 3 * d0;
  const bool ok = i < n;
  const float px = ok ? s[3 * i] : 0.0f, py = ok ? s[3 * i + 1] : 0.0f, pz = ok ? s[3 * i + 2] : 0.0f;
  float best = __builtin_huge_valf();
  for (int64_t j0 = 0; j0 < m; j0 += NNR_TILE) {
    const int cnt = (int)min((int64_t)NNR_TILE, m - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      tx[j] = d[3 * (j0 + j)]; ty[j] = d[3 * (j0 + j) + 1]; tz[j] = d[3 * (j0 + j) + 2];
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) {
      const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
      best = fminf(best, (dx * dx + dy * dy) + dz * dz);
    }
  }
  if (ok) out[s0 + i] = best;
}

}  // namespace

static_assert(sizeof(RpBest) == 16, "pfpp_ransac_pairs_workspace counts 16 bytes per workgroup");

extern "C" int64_t pfpp_ransac_pairs_workspace(int64_t E, int64_t H) {
  if (E < 0 || H < 1) return -1;
  return E * ((H + RP_WG - 1) / RP_WG) * (int64_t)sizeof(RpBest);
}

extern "C" int pfpp_ransac_pairs(const float* pts, int64_t R, int64_t E, const int64_t* pair_off, const int32_t* corr, const int64_t* corr_off,
                                 int64_t H, double max_dist, uint64_t seed, int refine, float* Rout, float* tout, double* stats, int32_t* info,
                                 int32_t* counts_out, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(E >= 0 && R >= 0 && H >= 1, "bad sizes (at least one hypothesis)");
  PFPP_REQUIRE(max_dist > 0.0, "max_dist must be positive");
  PFPP_SUPPORTED(E <= 65535, "more than 65535 pairs in one launch");
  PFPP_SUPPORTED(H <= 0x7fffff00, "more than 2^31 - 256 hypotheses per pair");
  if (E == 0) return PFPP_OK;
  PFPP_REQUIRE(R >= 1, "pairs but no points");
  PFPP_REQUIRE(pts && pair_off && corr && corr_off && Rout && tout && stats && info && workspace, "null pointer");
  PFPP_REQUIRE(workspace_bytes >= pfpp_ransac_pairs_workspace(E, H), "workspace too small (pfpp_ransac_pairs_workspace)");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7u) == 0,
               "workspace and stats must be 8-byte aligned");
  const int nblk = (int)((H + RP_WG - 1) / RP_WG);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  const double max_d2 = max_dist * max_dist;
  hipStream_t st = pfpp::as_stream(stream);
  hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)nblk, (unsigned)E), dim3(RP_WG), 0, st, pts, R, pair_off, corr, corr_off, (int)H, max_d2,
                     k0, k1, static_cast<RpBest*>(workspace), counts_out);
  hipLaunchKernelGGL(ransac_finish_kernel, dim3((unsigned)E), dim3(64), 0, st, pts, R, pair_off, corr, corr_off, nblk, max_d2, k0, k1,
                     refine ? 1 : 0, static_cast<const RpBest*>(workspace), Rout, tout, stats, info);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_nn_dist_ragged(const float* src, const int64_t* src_off, const float* dst, const int64_t* dst_off, float* out,
                                   int64_t segments, int64_t max_n, pfpp_stream_t stream) {
  PFPP_REQUIRE(segments >= 0 && max_n >= 0, "bad sizes");
  PFPP_SUPPORTED(segments <= 65535, "more than 65535 segments per launch");
  if (segments == 0 || max_n == 0) return PFPP_OK;
  PFPP_REQUIRE(src && src_off && dst && dst_off && out, "null pointer");
  hipLaunchKernelGGL(nn_dist_ragged_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)segments), dim3(256), 0, pfpp::as_stream(stream), src,
                     src_off, dst, dst_off, out);
  return pfpp::check_launch(__func__);
}
