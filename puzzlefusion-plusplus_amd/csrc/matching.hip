// Matcher back end (Jigsaw_matching/model/jigsaw/joint_seg_align_model.py:164-278, 465-513; utils/linear_solvers.py:9-247;
// utils/critical_pcs.py): from per-point descriptors to the doubly-stochastic matrix the host assignment reads.
//
//  * match_classify_compact_kernel — pc_classifier (BatchNorm1d eval folded to scale / shift, ReLU, Conv1d(128, 1, 1)), the label
//    `sigmoid(logit) > 0.5` in fp32, and get_critical_pcs_from_label: one wave per piece walks its points 64 at a time and
//    compacts the local indices of the predicted points in order (the ballot + mbcnt scheme of ball_query_kernel).
//  * match_gather_rows_kernel — the critical rows of part_feats in piece order with affinity_extractor's BatchNorm + ReLU
//    applied on the way (the A operand of the 128 -> 512 GEMM) and the piece slot of every row.
//  * match_normalize_halves_kernel — F.normalize(p = 2, eps = 1e-12) of the two 256-wide halves of a row, in place.
//  * Sinkhorn in potential form.  The reference rewrites log_s <- log_s - LSE(log_s) 20 times next to two N' x N' mask tensors;
//    here log_s_k = L - u - v with L = s / tau read only, a row potential u and a column potential v.  A row sweep is one online
//    log-sum-exp per row (a wave per row); a column sweep writes per-(row block, column) partial (max, sum) pairs that a combine
//    kernel folds in a fixed order (deterministic, no float atomics); the last kernel writes exp(L - u - v) once.  Same-piece
//    entries (the reference's -1e6 mask, which contributes exp(-2e7) = 0 to every sum) are skipped by the piece ids of row and
//    column and come out as exactly 0.
//  * fracture_labels_kernel — compute_label: distance to the nearest point of another piece of the same puzzle, squared
//    distance in nn_dist_kernel's arithmetic with the target tiles in LDS, clamp(1e-12), sqrt, `<` in the reference's order.
#include "pfpp_common.h"
#include "sinkhorn_common.h"

namespace {

using namespace pfpp::sk;

constexpr int MATCH_C = 128;        // PC_FEAT_DIM
constexpr int MATCH_HALF = 256;     // AFF_FEAT_DIM / 2

// ------------------------------------------------------------------------------------------------ classify + compact
__global__ __launch_bounds__(256) void match_classify_compact_kernel(
    const float* __restrict__ feats, const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ w,
    float bias, const uint8_t* __restrict__ labels_in, const int64_t* __restrict__ piece_off, int64_t Pt, float* __restrict__ logits,
    uint8_t* __restrict__ labels, int64_t* __restrict__ crit_idx, int64_t* __restrict__ n_crit) {
  __shared__ float sc[MATCH_C], sh[MATCH_C], sw[MATCH_C];
  if (threadIdx.x < MATCH_C) {
    sc[threadIdx.x] = labels_in ? 0.0f : scale[threadIdx.x];
    sh[threadIdx.x] = labels_in ? 0.0f : shift[threadIdx.x];
    sw[threadIdx.x] = labels_in ? 0.0f : w[threadIdx.x];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= Pt) return;
  const int64_t st = piece_off[p], n = piece_off[p + 1] - st;
  int64_t cnt = 0;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t i = base + lane;
    const bool ok = i < n;
    bool keep = false;
    if (ok) {
      if (labels_in) {
        keep = labels_in[st + i] != 0;
      } else {
        const float4* row = reinterpret_cast<const float4*>(feats + (st + i) * MATCH_C);
        float acc = 0.0f;
#pragma unroll 4
        for (int k = 0; k < MATCH_C / 4; ++k) {
          const float4 x = row[k];
          acc += fmaxf(x.x * sc[4 * k] + sh[4 * k], 0.0f) * sw[4 * k];
          acc += fmaxf(x.y * sc[4 * k + 1] + sh[4 * k + 1], 0.0f) * sw[4 * k + 1];
          acc += fmaxf(x.z * sc[4 * k + 2] + sh[4 * k + 2], 0.0f) * sw[4 * k + 2];
          acc += fmaxf(x.w * sc[4 * k + 3] + sh[4 * k + 3], 0.0f) * sw[4 * k + 3];
        }
        const float logit = acc + bias;
        logits[st + i] = logit;
        // the reference's expression: torch.sigmoid(logit) > 0.5 in fp32 (a tiny positive logit gives exactly 0.5: not `logit > 0`)
        keep = 1.0f / (1.0f + expf(-logit)) > 0.5f;
      }
      if (labels) labels[st + i] = keep ? 1 : 0;
    }
    const unsigned long long m = __ballot(keep);
    const int prefix = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
    if (keep) crit_idx[st + cnt + prefix] = i;         // cnt + prefix <= i: never ahead of the scan, always inside the piece
    cnt += __builtin_popcountll(m);
  }
  for (int64_t i = cnt + lane; i < n; i += 64) crit_idx[st + i] = 0;
  if (lane == 0) n_crit[p] = cnt;
}

// ------------------------------------------------------------------------------------------------ gather of the critical rows
__global__ __launch_bounds__(256) void match_gather_rows_kernel(
    const float* __restrict__ feats, const float* __restrict__ scale, const float* __restrict__ shift, const int64_t* __restrict__ crit_idx,
    const int64_t* __restrict__ piece_off, const int64_t* __restrict__ crit_off, const int32_t* __restrict__ piece_slot, int64_t Pt,
    int64_t R, float* __restrict__ out, int32_t* __restrict__ row_piece) {
  const int sub = threadIdx.x & 31;                      // 32 lanes x float4 = one 128-wide row
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= R) return;
  int64_t lo = 0, hi = Pt;                               // the piece p with crit_off[p] <= r < crit_off[p + 1]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (crit_off[mid] <= r) lo = mid; else hi = mid;
  }
  const int64_t st = piece_off[lo], n = piece_off[lo + 1] - st;
  int64_t i = crit_idx[st + (r - crit_off[lo])];
  i = i < 0 ? 0 : (i >= n ? n - 1 : i);                  // memory safety only: the indices are match_classify_compact_kernel's
  const float4 x = reinterpret_cast<const float4*>(feats + (st + i) * MATCH_C)[sub];
  const float4 a = reinterpret_cast<const float4*>(scale)[sub], b = reinterpret_cast<const float4*>(shift)[sub];
  float4 y;
  y.x = fmaxf(x.x * a.x + b.x, 0.0f); y.y = fmaxf(x.y * a.y + b.y, 0.0f);
  y.z = fmaxf(x.z * a.z + b.z, 0.0f); y.w = fmaxf(x.w * a.w + b.w, 0.0f);
  reinterpret_cast<float4*>(out + r * MATCH_C)[sub] = y;
  if (sub == 0) row_piece[r] = piece_slot[lo];
}

// ------------------------------------------------------------------------------------------------ L2 normalisation of the halves
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void match_normalize_halves_kernel(float* __restrict__ x, int64_t R) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float4* row = reinterpret_cast<float4*>(x + r * (2 * MATCH_HALF));
  float4 a = row[lane], b = row[64 + lane];
  const float sa = wave_sum((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w));
  const float sb = wave_sum((b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w));
  const float da = fmaxf(sqrtf(sa), 1e-12f), db = fmaxf(sqrtf(sb), 1e-12f);      // F.normalize: x / max(|x|_2, eps)
  a.x /= da; a.y /= da; a.z /= da; a.w /= da;
  b.x /= db; b.y /= db; b.z /= db; b.w /= db;
  row[lane] = a; row[64 + lane] = b;
}

// ------------------------------------------------------------------------------------------------ Sinkhorn, potential form
// (lse_push / lse_merge / lse_value, sk_entry and the block sizes: sinkhorn_common.h, shared with the training form)
// u[i] += LSE_j((L_ij - u_i) - v_j) over the columns of other pieces; one wave per row
__global__ __launch_bounds__(256) void sinkhorn_row_kernel(const float* __restrict__ s, int64_t ld, const int32_t* __restrict__ piece, int n,
                                                           float tau, double* __restrict__ u, const double* __restrict__ v) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* row = s + (int64_t)i * ld;
  const double ui = u[i];
  const int pi = piece[i];
  float m = -__builtin_huge_valf();
  double sum = 0.0;
  // four columns per lane in flight: the loads do not wait for the push chain (same order of pushes as one at a time)
  for (int j0 = lane; j0 < n; j0 += 4 * 64) {
    float a[4];
    double vj[4];
    int pj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + 64 * k;
      const int jc = j < n ? j : n - 1;
      a[k] = row[jc]; vj[k] = v[jc];
      pj[k] = j < n ? piece[jc] : pi;                  // past the end counts as the row's own piece: skipped
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pj[k] != pi) lse_push(m, sum, sk_entry(a[k], tau, ui, vj[k]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const double s2 = __shfl_xor(sum, o, 64);
    lse_merge(m, sum, m2, s2);
  }
  if (lane == 0 && sum > 0.0) u[i] = ui + (double)lse_value(m, sum);
}

// partial (max, sum) of column j over the rows of block y
__global__ __launch_bounds__(256) void sinkhorn_col_partial_kernel(const float* __restrict__ s, int64_t ld, const int32_t* __restrict__ piece,
                                                                   int n, float tau, const double* __restrict__ u,
                                                                   const double* __restrict__ v, float* __restrict__ pm,
                                                                   double* __restrict__ ps) {
  __shared__ double su[SK_ROWS];
  __shared__ int sp[SK_ROWS];
  const int i0 = blockIdx.y * SK_ROWS;
  const int rows = min(SK_ROWS, n - i0);
  if ((int)threadIdx.x < rows) { su[threadIdx.x] = u[i0 + threadIdx.x]; sp[threadIdx.x] = piece[i0 + threadIdx.x]; }
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double vj = v[j];
  const int pj = piece[j];
  const float* col = s + (int64_t)i0 * ld + j;
  float m = -__builtin_huge_valf();
  double sum = 0.0;
  for (int r0 = 0; r0 < rows; r0 += 4) {               // four rows in flight, pushed in row order
    float a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = col[(int64_t)min(r0 + k, rows - 1) * ld];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (r0 + k < rows && sp[r0 + k] != pj) lse_push(m, sum, sk_entry(a[k], tau, su[r0 + k], vj));
  }
  pm[(int64_t)blockIdx.y * n + j] = m;
  ps[(int64_t)blockIdx.y * n + j] = sum;
}

// v[j] += LSE over the row blocks.  64 columns per workgroup, the row blocks of a column split over its four waves (the partials of a
// column are nblk strided loads; one thread per column would leave 10 workgroups at N' = 2,492, each waiting on 2 x 39 of them).
// Each quarter takes its maximum first, then its sum in block order; the four quarters
// are folded in order through LDS.  Fixed order throughout: repeatable bit for bit.
__global__ __launch_bounds__(256) void sinkhorn_col_combine_kernel(const float* __restrict__ pm, const double* __restrict__ ps, int n, int nblk,
                                                                   double* __restrict__ v) {
  __shared__ float qm[CB_PARTS][CB_COLS];
  __shared__ double qs[CB_PARTS][CB_COLS];
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int j = blockIdx.x * CB_COLS + c;
  const int per = (nblk + CB_PARTS - 1) / CB_PARTS;
  const int b0 = part * per, b1 = min(nblk, b0 + per);
  float m = -__builtin_huge_valf();
  double sum = 0.0;
  if (j < n) {
#pragma unroll 4
    for (int b = b0; b < b1; ++b) m = fmaxf(m, pm[(int64_t)b * n + j]);
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
      const double sb = ps[(int64_t)b * n + j];
      if (sb > 0.0) sum += sb * (double)expf(pm[(int64_t)b * n + j] - m);        // an empty block has (max, sum) = (-inf, 0)
    }
  }
  qm[part][c] = m;
  qs[part][c] = sum;
  __syncthreads();
  if (part == 0 && j < n) {
    float mm = qm[0][c];
#pragma unroll
    for (int q = 1; q < CB_PARTS; ++q) mm = fmaxf(mm, qm[q][c]);
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < CB_PARTS; ++q)
      if (qs[q][c] > 0.0) tot += qs[q][c] * (double)expf(qm[q][c] - mm);
    if (tot > 0.0) v[j] += (double)lse_value(mm, tot);
  }
}

__global__ __launch_bounds__(256) void sinkhorn_exp_kernel(const float* __restrict__ s, int64_t ld, const int32_t* __restrict__ piece, int n,
                                                           float tau, const double* __restrict__ u, const double* __restrict__ v,
                                                           float* __restrict__ ds) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (j >= n) return;
  const float x = sk_entry(s[(int64_t)i * ld + j], tau, u[i], v[j]);
  ds[(int64_t)i * n + j] = piece[i] == piece[j] ? 0.0f : expf(x);
}

// ------------------------------------------------------------------------------------------------ fracture labels
constexpr int FL_TILE = 1024;

__global__ __launch_bounds__(256) void fracture_labels_kernel(const float* __restrict__ pts, const int64_t* __restrict__ piece_off,
                                                              const int64_t* __restrict__ puz_piece_off, const float* __restrict__ thr,
                                                              float* __restrict__ dist, uint8_t* __restrict__ labels) {
  __shared__ float tx[FL_TILE], ty[FL_TILE], tz[FL_TILE];
  const int64_t b = blockIdx.y;
  const int64_t p0 = puz_piece_off[b], p1 = puz_piece_off[b + 1];
  const int64_t q0 = piece_off[p0], q1 = piece_off[p1];           // the puzzle's points
  const int64_t i = q0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q0 + (int64_t)blockIdx.x * 256 >= q1) return;                // whole block past the puzzle (uniform)
  const bool ok = i < q1;
  int64_t ps = q0, pe = q0;                                        // own piece [ps, pe)
  if (ok) {
    for (int64_t p = p0; p < p1; ++p)
      if (piece_off[p] <= i && i < piece_off[p + 1]) { ps = piece_off[p]; pe = piece_off[p + 1]; }
  }
  const float px = ok ? pts[3 * i] : 0.0f, py = ok ? pts[3 * i + 1] : 0.0f, pz = ok ? pts[3 * i + 2] : 0.0f;
  float best = __builtin_huge_valf();
  for (int64_t j0 = q0; j0 < q1; j0 += FL_TILE) {
    const int cnt = (int)min((int64_t)FL_TILE, q1 - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      tx[j] = pts[3 * (j0 + j)]; ty[j] = pts[3 * (j0 + j) + 1]; tz[j] = pts[3 * (j0 + j) + 2];
    }
    __syncthreads();
    // columns of this tile that belong to the own piece: [a, e)
    const int a = (int)max((int64_t)0, min((int64_t)cnt, ps - j0)), e = (int)max((int64_t)0, min((int64_t)cnt, pe - j0));
#pragma unroll 8
    for (int j = 0; j < a; ++j) {
      const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
      best = fminf(best, (dx * dx + dy * dy) + dz * dz);
    }
#pragma unroll 8
    for (int j = max(a, e); j < cnt; ++j) {
      const float dx = px - tx[j], dy = py - ty[j], dz = pz - tz[j];
      best = fminf(best, (dx * dx + dy * dy) + dz * dz);
    }
  }
  if (ok) {
    const float d = sqrtf(fmaxf(best, 1e-12f));                    // square_distance clamps at 1e-12 before the sqrt
    if (dist) dist[i] = d;
    labels[i] = d < thr[i] ? 1 : 0;
  }
}

}  // namespace

extern "C" int pfpp_match_classify_compact(const float* feats, const float* bn_scale, const float* bn_shift, const float* w, float bias,
                                           const uint8_t* labels_in, const int64_t* piece_off, int64_t Pt, int64_t C, float* logits,
                                           uint8_t* labels, int64_t* critical_pcs_idx, int64_t* n_critical_pcs, pfpp_stream_t stream) {
  PFPP_REQUIRE(piece_off && critical_pcs_idx && n_critical_pcs, "null pointer");
  PFPP_REQUIRE(labels_in || (feats && bn_scale && bn_shift && w && logits), "the classifier needs feats, scale, shift, w and logits");
  PFPP_REQUIRE(Pt >= 0, "bad sizes");
  PFPP_SUPPORTED(C == MATCH_C, "PC_FEAT_DIM other than 128");
  PFPP_REQUIRE(labels_in || pfpp::aligned16(feats), "feats must be 16-byte aligned");
  PFPP_SUPPORTED(Pt <= (int64_t)1 << 30, "too many pieces");
  if (Pt == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_classify_compact_kernel, dim3((unsigned)((Pt + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), feats,
                     bn_scale, bn_shift, w, bias, labels_in, piece_off, Pt, logits, labels, critical_pcs_idx, n_critical_pcs);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_gather_rows(const float* feats, const float* bn_scale, const float* bn_shift, const int64_t* critical_pcs_idx,
                                      const int64_t* piece_off, const int64_t* crit_off, const int32_t* piece_slot, int64_t Pt,
                                      int64_t R, int64_t C, float* out, int32_t* row_piece, pfpp_stream_t stream) {
  PFPP_REQUIRE(feats && bn_scale && bn_shift && critical_pcs_idx && piece_off && crit_off && piece_slot && out && row_piece, "null pointer");
  PFPP_REQUIRE(Pt >= 1 && R >= 0, "bad sizes");
  PFPP_SUPPORTED(C == MATCH_C, "PC_FEAT_DIM other than 128");
  PFPP_REQUIRE(pfpp::aligned16(feats) && pfpp::aligned16(out) && pfpp::aligned16(bn_scale) && pfpp::aligned16(bn_shift),
               "feats, out, scale and shift must be 16-byte aligned");
  PFPP_SUPPORTED(R <= (int64_t)1 << 33, "too many rows");
  if (R == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_gather_rows_kernel, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, pfpp::as_stream(stream), feats, bn_scale,
                     bn_shift, critical_pcs_idx, piece_off, crit_off, piece_slot, Pt, R, out, row_piece);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_normalize_halves(float* x, int64_t R, int64_t D, pfpp_stream_t stream) {
  PFPP_REQUIRE(x && R >= 0, "null pointer or bad sizes");
  PFPP_SUPPORTED(D == 2 * MATCH_HALF, "AFF_FEAT_DIM other than 512");
  PFPP_REQUIRE(pfpp::aligned16(x), "x must be 16-byte aligned");
  PFPP_SUPPORTED(R <= (int64_t)1 << 33, "too many rows");
  if (R == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_normalize_halves_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), x, R);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_sinkhorn_workspace(int64_t n) {
  if (n < 0 || n > 65535) return -1;
  return ((n + SK_ROWS - 1) / SK_ROWS) * n * (int64_t)(sizeof(double) + sizeof(float));       // partial sums fp64, partial maxima fp32
}

extern "C" int pfpp_sinkhorn_masked(const float* s, int64_t ld, const int32_t* piece, int64_t n, float tau, int64_t max_iter, double* u,
                                    double* v, float* ds_mat, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(s && piece && u && v && ds_mat, "null pointer");
  PFPP_REQUIRE(n >= 1 && ld >= n && max_iter >= 0 && tau > 0.0f, "bad sizes");
  PFPP_SUPPORTED(n <= 65535, "more than 65535 critical points in one puzzle");
  PFPP_REQUIRE(workspace && workspace_bytes >= pfpp_sinkhorn_workspace(n), "workspace smaller than pfpp_sinkhorn_workspace(n)");
  hipStream_t st = pfpp::as_stream(stream);
  const int nn = (int)n, nblk = (nn + SK_ROWS - 1) / SK_ROWS;
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "workspace must be 8-byte aligned");
  double* ps = static_cast<double*>(workspace);
  float* pm = reinterpret_cast<float*>(ps + (int64_t)nblk * n);
  if (hipMemsetAsync(u, 0, n * sizeof(double), st) != hipSuccess || hipMemsetAsync(v, 0, n * sizeof(double), st) != hipSuccess) {
    pfpp::set_error("%s: hipMemsetAsync failed", __func__);
    return PFPP_EHIP;
  }
  const unsigned cblk = (unsigned)((nn + 255) / 256);
  for (int64_t it = 0; it < max_iter; ++it) {
    if (it % 2 == 0) {
      hipLaunchKernelGGL(sinkhorn_row_kernel, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, st, s, ld, piece, nn, tau, u, v);
    } else {
      hipLaunchKernelGGL(sinkhorn_col_partial_kernel, dim3(cblk, (unsigned)nblk), dim3(256), 0, st, s, ld, piece, nn, tau, u, v, pm, ps);
      hipLaunchKernelGGL(sinkhorn_col_combine_kernel, dim3((unsigned)((nn + CB_COLS - 1) / CB_COLS)), dim3(256), 0, st, pm, ps, nn, nblk, v);
    }
  }
  hipLaunchKernelGGL(sinkhorn_exp_kernel, dim3(cblk, (unsigned)nn), dim3(256), 0, st, s, ld, piece, nn, tau, u, v, ds_mat);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_fracture_labels(const float* gt_pcs, const int64_t* piece_off, const int64_t* puz_piece_off, const float* thresholds,
                                    int64_t B, int64_t max_points, float* dist, uint8_t* labels, pfpp_stream_t stream) {
  PFPP_REQUIRE(gt_pcs && piece_off && puz_piece_off && thresholds && labels, "null pointer");
  PFPP_REQUIRE(B >= 0 && max_points >= 0, "bad sizes");
  PFPP_SUPPORTED(B <= 65535, "more than 65535 puzzles per launch");
  PFPP_SUPPORTED(max_points <= (int64_t)1 << 30, "too many points in one puzzle");
  if (B == 0 || max_points == 0) return PFPP_OK;
  hipLaunchKernelGGL(fracture_labels_kernel, dim3((unsigned)((max_points + 255) / 256), (unsigned)B), dim3(256), 0,
                     pfpp::as_stream(stream), gt_pcs, piece_off, puz_piece_off, thresholds, dist, labels);
  return pfpp::check_launch(__func__);
}
