// The rigid term of the matcher's training loss (Jigsaw_matching/utils/loss.py:59-142 with utils/pairwise_alignment.py:11-79,
// called at model/jigsaw/joint_seg_align_model.py:379-392 once w_rig_loss > 0) and its gradient with respect to ds_mat.
//
// For every pair p < q of pieces of a puzzle that both own critical points, with W = ds_mat[I_p, I_q] + ds_mat[I_q, I_p]^T,
// S = X[I_p], T = X[I_q] (X = the critical points of part_pcs in row order): r_i = sum_j W_ij, b_i = sum_j W_ij T_j, mat_s = sum_i
// r_i; Horn's closed form on the detached W gives (R, t), rounded to fp32 and constant; A_i = R S_i + t, e_i = r_i A_i - b_i,
// pair_loss = sum_i |e_i|^2; the batch's term is sum_pairs pair_loss mat_s / sum_pairs n1.
//
//  * rigid_pair_sums_kernel — (r_i, b_i) of every row i and every later piece q.  A workgroup owns 64 rows and one piece q and walks
//    the columns of I_q in tiles of 64: the ds_mat[I_p, I_q] tile is read along its rows and the ds_mat[I_q, I_p] tile along ITS
//    rows (both coalesced) into LDS, where the second is read transposed.  A tile starts at the piece's first column, so piece
//    boundaries fall anywhere; four threads share a row, each with 16 of the tile's columns in column order, and the four chains
//    are folded in order at the end.  fp64 sums of exact fp64 sums of two fp32 entries.  The workgroups of the diagonal blocks only
//    look for a positive entry (the reference's `sum(ds_mat[b]) > 0`, which for non-negative entries is `any > 0`).
//  * rigid_pair_pose_kernel — a wave per pair of the whole batch: mat_s, the centroids, M, Horn's N, a cyclic Jacobi of ten sweeps
//    from the identity in fp64, the eigenvector of the first of the largest eigenvalues, R and t (fp32), pair_loss.  N, the
//    Jacobi and the quaternion's rotation are horn_common.h's, shared with matching_pose.hip.
//  * rigid_fold_kernel — numerator and n_sum over the pairs in pair order, rig_loss and the gradient scale w_rig_loss / n_sum.
//  * rigid_grad_kernel — d(w_rig_loss rig_loss) / d ds_mat for one puzzle, element-wise: with a the index in the earlier piece and
//    c the one in the later, scale (2 mat_s e_a . (A_a - T_c) + pair_loss); exact zeros in diagonal blocks and in pairs not kept.
// All sums fp64, no float atomics, every fold in a fixed order: two runs agree bitwise.
#include "pfpp_common.h"
#include "horn_common.h"

namespace {

constexpr int RG_TILE = 64;          // rows per workgroup and columns per step of the pair sums
constexpr int RG_PMAX = 64;          // pieces per puzzle the kernels are built for (the reference has at most 20)
constexpr int RG_STATS = 8;          // doubles per pair record: mat_s, pair_loss, the four eigenvalues (ascending), n1, n2

__device__ __forceinline__ double rg_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ pair sums
// grid (row tiles, P).  rb[(i P + q) 4 + {0, 1, 2, 3}] = (r_i, b_i) against piece q for q > piece(i); other slots are not written.
__global__ __launch_bounds__(256) void rigid_pair_sums_kernel(const float* __restrict__ ds, int64_t ld, int n, const float* __restrict__ pts,
                                                              const int32_t* __restrict__ piece_off, int P, double* __restrict__ rb,
                                                              int32_t* __restrict__ any_pos) {
  __shared__ float sa[RG_TILE][RG_TILE + 1], sb[RG_TILE][RG_TILE + 1];
  __shared__ float st[RG_TILE][3];
  __shared__ double sp[RG_TILE][4][4];
  __shared__ int spiece[RG_TILE];
  __shared__ int spos;
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * RG_TILE, q = blockIdx.y;
  const int c_begin = max(piece_off[q], 0), c_end = min(piece_off[q + 1], n);      // the clamps: memory safety only
  if (c_begin >= c_end) return;                                      // an empty piece (uniform)
  if (tid < RG_TILE) {
    const int i = min(i0 + tid, n - 1);
    int p = 0;
    while (p + 1 < P && piece_off[p + 1] <= i) ++p;
    spiece[tid] = p;
  }
  if (tid == 0) spos = 0;
  __syncthreads();
  if (spiece[0] > q) return;                                         // every row of the tile lies behind piece q (uniform)
  const int rows = min(RG_TILE, n - i0);
  const int ii = tid >> 2, part = tid & 3;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int pos = 0;
  for (int c0 = c_begin; c0 < c_end; c0 += RG_TILE) {
    const int cols = min(RG_TILE, c_end - c0);
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < RG_TILE * RG_TILE / 256; ++k) {
      const int idx = tid + 256 * k;
      const int hi = idx >> 6, lo = idx & 63;
      // ds_mat[I_p, I_q]: row i0 + hi, column c0 + lo;  ds_mat[I_q, I_p]: row c0 + hi, column i0 + lo
      const float a = (hi < rows && lo < cols) ? ds[(int64_t)(i0 + hi) * ld + c0 + lo] : 0.0f;
      const float b = (hi < cols && lo < rows) ? ds[(int64_t)(c0 + hi) * ld + i0 + lo] : 0.0f;
      sa[hi][lo] = a;
      sb[hi][lo] = b;
      pos |= (a > 0.0f) | (b > 0.0f);
    }
    if (tid < cols) {
      st[tid][0] = pts[3 * (int64_t)(c0 + tid)];
      st[tid][1] = pts[3 * (int64_t)(c0 + tid) + 1];
      st[tid][2] = pts[3 * (int64_t)(c0 + tid) + 2];
    }
    __syncthreads();
    const int j1 = min(16 * part + 16, cols);
    for (int j = 16 * part; j < j1; ++j) {
      const double w = (double)sa[ii][j] + (double)sb[j][ii];
      acc[0] += w;
      acc[1] += w * (double)st[j][0];
      acc[2] += w * (double)st[j][1];
      acc[3] += w * (double)st[j][2];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sp[ii][part][k] = acc[k];
  if (pos) spos = 1;                                                 // every writer writes the same value
  __syncthreads();
  if (tid == 0 && spos) atomicOr(any_pos, 1);
  if (tid < RG_TILE && tid < rows && spiece[tid] < q) {
    double* out = rb + ((int64_t)(i0 + tid) * P + q) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = ((sp[tid][0][k] + sp[tid][1][k]) + sp[tid][2][k]) + sp[tid][3][k];
  }
}

// ------------------------------------------------------------------------------------------------ pair pose and loss
// pairs int32 [npairs, 4] = (puzzle, p, q, -); puz_row_off int64 [B + 1] into pts [R, 3] and rb [R, P, 4]; piece_off int32
// [B, P + 1] puzzle-local; status: 1 kept, 0 skipped (the reference's `continue`), -1 not finite in the reference (mat_s == 0 kept)
__global__ __launch_bounds__(64) void rigid_pair_pose_kernel(const int32_t* __restrict__ pairs, const int64_t* __restrict__ puz_row_off,
                                                             const int32_t* __restrict__ piece_off, int P,
                                                             const int32_t* __restrict__ n_valid, const int32_t* __restrict__ any_pos,
                                                             const double* __restrict__ rb, const float* __restrict__ pts,
                                                             float* __restrict__ Rout, float* __restrict__ tout,
                                                             double* __restrict__ stats, int32_t* __restrict__ status) {
  const int lane = threadIdx.x;
  const int64_t pair = blockIdx.x;
  const int b = pairs[4 * pair], p = pairs[4 * pair + 1], q = pairs[4 * pair + 2];
  const int64_t row0 = puz_row_off[b];
  const int32_t* po = piece_off + (int64_t)b * (P + 1);
  const int s0 = po[p], n1 = po[p + 1] - s0, t0 = po[q], n2 = po[q + 1] - t0;
  const float* S = pts + 3 * (row0 + s0);
  const float* T = pts + 3 * (row0 + t0);
  const double* rbp = rb + ((row0 + s0) * P + q) * 4;                // row i of the pair: rbp + i P 4

  // pass 1: mat_s, sum S, sum r S, sum b; sum T
  double a_r = 0.0, a_s[3] = {0.0, 0.0, 0.0}, a_rs[3] = {0.0, 0.0, 0.0}, a_b[3] = {0.0, 0.0, 0.0}, a_t[3] = {0.0, 0.0, 0.0};
  for (int i = lane; i < n1; i += 64) {
    const double* e = rbp + (int64_t)i * P * 4;
    const double r = e[0];
    a_r += r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double sk = (double)S[3 * i + k];
      a_s[k] += sk;
      a_rs[k] += r * sk;
      a_b[k] += e[1 + k];
    }
  }
  for (int j = lane; j < n2; j += 64) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a_t[k] += (double)T[3 * j + k];
  }
  const double mat_s = rg_wave_sum(a_r);
  double cS[3], cT[3], srs[3], sbv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    cS[k] = rg_wave_sum(a_s[k]) / (double)n1;
    cT[k] = rg_wave_sum(a_t[k]) / (double)n2;
    srs[k] = rg_wave_sum(a_rs[k]);
    sbv[k] = rg_wave_sum(a_b[k]);
  }
  // pass 2: M = sum_i (S_i - cS) (b_i - r_i cT)^T
  double M[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int i = lane; i < n1; i += 64) {
    const double* e = rbp + (int64_t)i * P * 4;
    const double r = e[0];
    double sc[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sc[k] = (double)S[3 * i + k] - cS[k];
      bc[k] = e[1 + k] - r * cT[k];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[a][c] += sc[a] * bc[c];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[a][c] = rg_wave_sum(M[a][c]);

  // Horn's N (pairwise_alignment.py:20-47) and its eigenvectors; every lane holds the same numbers
  double A[4][4], V[4][4], ev[4], qv[4], Rd[3][3];
  rg_horn_n(M, A);
  (void)rg_top_eigenvector(A, V, ev, qv);
  rg_quat_rot(qv, Rd);
  // t = sum_i (b_i - r_i R S_i) / mat_s; R and t are handed on rounded to fp32 (pairwise_alignment.py:79)
  const bool zero = mat_s == 0.0;
  float Rf[3][3], tf[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double rs = (Rd[a][0] * srs[0] + Rd[a][1] * srs[1]) + Rd[a][2] * srs[2];
    tf[a] = zero ? 0.0f : (float)((sbv[a] - rs) / mat_s);
#pragma unroll
    for (int c = 0; c < 3; ++c) Rf[a][c] = (float)Rd[a][c];
  }
  // pass 3: pair_loss = sum_i |r_i (R S_i + t) - b_i|^2
  double pl = 0.0;
  for (int i = lane; i < n1; i += 64) {
    const double* e = rbp + (int64_t)i * P * 4;
    const double r = e[0];
    const double sx = (double)S[3 * i], sy = (double)S[3 * i + 1], sz = (double)S[3 * i + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double Aa = (((double)Rf[a][0] * sx + (double)Rf[a][1] * sy) + (double)Rf[a][2] * sz) + (double)tf[a];
      const double ea = r * Aa - e[1 + a];
      pl += ea * ea;
    }
  }
  pl = rg_wave_sum(pl);
  if (lane == 0) {
    // sort the eigenvalues ascending (np.linalg.eigh's order): a fixed network on four values
    double e0 = ev[0], e1 = ev[1], e2 = ev[2], e3 = ev[3], x;
    if (e0 > e1) { x = e0; e0 = e1; e1 = x; }
    if (e2 > e3) { x = e2; e2 = e3; e3 = x; }
    if (e0 > e2) { x = e0; e0 = e2; e2 = x; }
    if (e1 > e3) { x = e1; e1 = e3; e3 = x; }
    if (e1 > e2) { x = e1; e1 = e2; e2 = x; }
    double* so = stats + pair * RG_STATS;
    so[0] = mat_s; so[1] = zero ? 0.0 : pl; so[2] = e0; so[3] = e1; so[4] = e2; so[5] = e3; so[6] = (double)n1; so[7] = (double)n2;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      tout[3 * pair + a] = tf[a];
#pragma unroll
      for (int c = 0; c < 3; ++c) Rout[9 * pair + 3 * a + c] = Rf[a][c];
    }
    // utils/loss.py:98: skipped; a pair with mat_s == 0 that is NOT skipped divides 0 by 0 in t
    status[pair] = !zero ? 1 : ((n_valid[b] > 2 && any_pos[b] != 0) ? 0 : -1);
  }
}

// ------------------------------------------------------------------------------------------------ fold
// out[0] = rig_loss, out[1] = w_rig_loss / n_sum (the gradient's scale), out[2] = n_sum, out[3] = the numerator; where the
// reference is not finite (a status of -1, or no kept pair) rig_loss and the scale are 0.  The pairs' terms are staged through LDS
// 256 at a time and added by one thread in pair order, as the reference's loop adds them.
__global__ __launch_bounds__(256) void rigid_fold_kernel(const double* __restrict__ stats, const int32_t* __restrict__ status, int64_t npairs,
                                                         double w_rig, double* __restrict__ out) {
  __shared__ double snum[256], scnt[256];
  __shared__ int sbad[256];
  double num = 0.0, cnt = 0.0;               // thread 0's running sums
  int bad = 0;
  for (int64_t k0 = 0; k0 < npairs; k0 += 256) {
    const int64_t k = k0 + threadIdx.x;
    const int s = k < npairs ? status[k] : 0;
    snum[threadIdx.x] = s == 1 ? stats[k * RG_STATS + 1] * stats[k * RG_STATS] : 0.0;
    scnt[threadIdx.x] = s == 1 ? stats[k * RG_STATS + 6] : 0.0;
    sbad[threadIdx.x] = s < 0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = (int)min((int64_t)256, npairs - k0);
      for (int i = 0; i < m; ++i) { num += snum[i]; cnt += scnt[i]; bad |= sbad[i]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool ok = !bad && cnt > 0.0;
    out[0] = ok ? num / cnt : 0.0;
    out[1] = ok ? w_rig / cnt : 0.0;
    out[2] = cnt;
    out[3] = num;
  }
}

// ------------------------------------------------------------------------------------------------ gradient
// grid (column blocks of 256, n rows).  pair_index int32 [P, P]: the pair of (p, q), p < q, or -1
__global__ __launch_bounds__(256) void rigid_grad_kernel(int n, const float* __restrict__ pts, const int32_t* __restrict__ piece_off, int P,
                                                         const double* __restrict__ rb, const int32_t* __restrict__ pair_index,
                                                         const float* __restrict__ Rm, const float* __restrict__ tv,
                                                         const double* __restrict__ stats, const int32_t* __restrict__ status,
                                                         const double* __restrict__ fold, float* __restrict__ dP, int64_t ldg) {
  __shared__ int soff[RG_PMAX + 1];
  for (int k = threadIdx.x; k <= P; k += 256) soff[k] = piece_off[k];
  __syncthreads();
  const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int pi = 0, pj = 0;
  while (pi + 1 < P && soff[pi + 1] <= i) ++pi;
  while (pj + 1 < P && soff[pj + 1] <= j) ++pj;
  float g = 0.0f;
  if (pi != pj) {
    const int lo = min(pi, pj), hi = max(pi, pj);
    const int a = pi < pj ? i : j, c = pi < pj ? j : i;               // a in the earlier piece, c in the later
    const int pair = pair_index[lo * P + hi];
    if (pair >= 0 && status[pair] == 1) {
      const double scale = fold[1];
      const double mat_s = stats[(int64_t)pair * RG_STATS], pl = stats[(int64_t)pair * RG_STATS + 1];
      const double* e = rb + ((int64_t)a * P + hi) * 4;
      const double r = e[0];
      const double sx = (double)pts[3 * a], sy = (double)pts[3 * a + 1], sz = (double)pts[3 * a + 2];
      const float* Rp = Rm + 9 * (int64_t)pair;
      double dot = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double Ak = (((double)Rp[3 * k] * sx + (double)Rp[3 * k + 1] * sy) + (double)Rp[3 * k + 2] * sz) + (double)tv[3 * (int64_t)pair + k];
        const double ek = r * Ak - e[1 + k];
        dot += ek * (Ak - (double)pts[3 * c + k]);
      }
      g = (float)(scale * ((2.0 * mat_s) * dot + pl));
    }
  }
  dP[(int64_t)i * ldg + j] = g;
}

}  // namespace

extern "C" int pfpp_rigid_pair_sums(const float* ds_mat, int64_t ld, int64_t n, const float* pts, const int32_t* piece_off, int64_t P,
                                    double* rb, int32_t* any_pos, pfpp_stream_t stream) {
  PFPP_REQUIRE(ds_mat && pts && piece_off && rb && any_pos, "null pointer");
  PFPP_REQUIRE(n >= 0 && ld >= n && P >= 1, "bad sizes");
  PFPP_SUPPORTED(n <= 65535, "more than 65535 critical points in one puzzle");
  PFPP_SUPPORTED(P <= RG_PMAX, "more than 64 pieces in one puzzle");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(rb) & 7u) == 0, "rb must be 8-byte aligned");
  if (n == 0) return PFPP_OK;
  hipLaunchKernelGGL(rigid_pair_sums_kernel, dim3((unsigned)((n + RG_TILE - 1) / RG_TILE), (unsigned)P), dim3(256), 0, pfpp::as_stream(stream),
                     ds_mat, ld, (int)n, pts, piece_off, (int)P, rb, any_pos);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_rigid_pair_pose(int64_t npairs, const int32_t* pairs, const int64_t* puz_row_off, const int32_t* piece_off, int64_t P,
                                    const int32_t* n_valid, const int32_t* any_pos, const double* rb, const float* pts, float* R, float* t,
                                    double* stats, int32_t* status, pfpp_stream_t stream) {
  PFPP_REQUIRE(npairs >= 0 && P >= 1, "bad sizes");
  PFPP_SUPPORTED(P <= RG_PMAX, "more than 64 pieces in one puzzle");
  PFPP_SUPPORTED(npairs <= 0x7fffffff, "more than 2^31 - 1 pairs in one launch");
  if (npairs == 0) return PFPP_OK;
  PFPP_REQUIRE(pairs && puz_row_off && piece_off && n_valid && any_pos && rb && pts && R && t && stats && status, "null pointer");
  hipLaunchKernelGGL(rigid_pair_pose_kernel, dim3((unsigned)npairs), dim3(64), 0, pfpp::as_stream(stream), pairs, puz_row_off, piece_off, (int)P,
                     n_valid, any_pos, rb, pts, R, t, stats, status);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_rigid_fold(int64_t npairs, const double* stats, const int32_t* status, double w_rig_loss, double* out,
                               pfpp_stream_t stream) {
  PFPP_REQUIRE(out && npairs >= 0 && (npairs == 0 || (stats && status)), "null pointer or bad sizes");
  hipLaunchKernelGGL(rigid_fold_kernel, dim3(1), dim3(256), 0, pfpp::as_stream(stream), stats, status, npairs, w_rig_loss, out);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_rigid_grad(int64_t n, const float* pts, const int32_t* piece_off, int64_t P, const double* rb, const int32_t* pair_index,
                               const float* R, const float* t, const double* stats, const int32_t* status, const double* fold, float* dP,
                               int64_t ldg, pfpp_stream_t stream) {
  PFPP_REQUIRE(pts && piece_off && rb && pair_index && fold && dP, "null pointer");
  PFPP_REQUIRE(n >= 0 && ldg >= n && P >= 1, "bad sizes");
  PFPP_SUPPORTED(n <= 65535, "more than 65535 critical points in one puzzle");
  PFPP_SUPPORTED(P <= RG_PMAX, "more than 64 pieces in one puzzle");
  if (n == 0) return PFPP_OK;
  hipLaunchKernelGGL(rigid_grad_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n), dim3(256), 0, pfpp::as_stream(stream), (int)n, pts,
                     piece_off, (int)P, rb, pair_index, R, t, stats, status, fold, dP, ldg);
  return pfpp::check_launch(__func__);
}
