// Training of the matcher's head behind part_feats (Jigsaw_matching/model/jigsaw/joint_seg_align_model.py:110-116, 164-268 in
// .train(), _loss_function :280-426; utils/linear_solvers.py:188-207; utils/loss.py:26-56): what the existing train-mode
// BatchNorm, GEMM and AdamW entry points do not cover.
//
//  * Sinkhorn, training form (one puzzle, unmasked).  Forward as in matching.hip — L = s / tau read only, fp64 potentials — but
//    every step writes its potential vector to its own row of pots [max_iter, n], which is all the backward needs: autograd keeps
//    the max_iter rewritten n x n matrices instead.  skt_exp_loss_kernel writes ds_mat = exp((L - u) - v) once and, from the same
//    pass, the permutation loss of the puzzle against one target column per row (no dense gt_perm), fp64 per row, rows folded in a
//    fixed order.
//  * Its backward.  G = dLoss / d log P lives in one n x n fp32 scratch that is updated in place.  Step i of the forward took
//    log P_i = log P_{i-1} - LSE_row (even i) or LSE_col (odd i), so G <- G - P_i * rowsum(G) resp. colsum(G), with P_i recomputed
//    from L and the two potential vectors of step i.  The sums cancel heavily (after a row step rowsum(G) is 0 up to rounding):
//    they are fp64.  Two layouts of the same update: skt_bwd_rows_kernel (a wave per row) leaves the row sums of the updated G,
//    skt_bwd_cols_kernel (a thread per column over 64-row blocks) its ordered column partials — each step is run in the layout
//    whose sums the NEXT step (the other direction) needs, so a step costs one read of s and one read-modify-write of G.  The first
//    pass (INIT) writes G_T = (P - y) P / max(P (1 - P), 1e-12) g, PyTorch's binary_cross_entropy backward times P, in the
//    layout step T - 1 needs.  No float atomics anywhere: two runs agree bitwise.  SEED (pfpp_sinkhorn_train_bwd_seeded): the
//    matrix holds dLoss' / d ds_mat of a further term on entry (the rigid term, matching_rigid.hip) and the first pass adds P * seed.
//  * match_gt_targets_kernel — the target column of every critical row: nearest critical point of another piece of the puzzle.
//  * match_normalize_halves_bwd_kernel, match_cls_bce_kernel (+ its fold), raw gather / scatter-add of the critical rows.
//  * match_colsum_part_kernel + match_colsum_fold_kernel — the bias gradients' column sums in a fixed order.
#include "pfpp_common.h"
#include "sinkhorn_common.h"

namespace {

using namespace pfpp::sk;

constexpr int MT_C = 128;        // PC_FEAT_DIM
constexpr int MT_HALF = 256;     // AFF_FEAT_DIM / 2

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ Sinkhorn forward, training form
// u_out[i] = u_in[i] + LSE_j((L_ij - u_in_i) - v_j); a null potential vector is all zeros.  One wave per row.
__global__ __launch_bounds__(256) void skt_row_kernel(const float* __restrict__ s, int64_t ld, int n, float tau,
                                                      const double* __restrict__ u_in, const double* __restrict__ v,
                                                      double* __restrict__ u_out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* row = s + (int64_t)i * ld;
  const double ui = u_in ? u_in[i] : 0.0;
  float m = -__builtin_huge_valf();
  double sum = 0.0;
  for (int j0 = lane; j0 < n; j0 += 4 * 64) {            // four columns per lane in flight, pushed in column order
    float a[4];
    double vj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + 64 * k;
      const int jc = j < n ? j : n - 1;
      a[k] = row[jc]; vj[k] = v ? v[jc] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + 64 * k < n) lse_push(m, sum, sk_entry(a[k], tau, ui, vj[k]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64);
    const double s2 = __shfl_xor(sum, o, 64);
    lse_merge(m, sum, m2, s2);
  }
  if (lane == 0) u_out[i] = ui + (double)lse_value(m, sum);
}

// partial (max, sum) of column j over the rows of block y
__global__ __launch_bounds__(256) void skt_col_partial_kernel(const float* __restrict__ s, int64_t ld, int n, float tau,
                                                              const double* __restrict__ u, const double* __restrict__ v_in,
                                                              float* __restrict__ pm, double* __restrict__ ps) {
  __shared__ double su[SK_ROWS];
  const int i0 = blockIdx.y * SK_ROWS;
  const int rows = min(SK_ROWS, n - i0);
  if ((int)threadIdx.x < rows) su[threadIdx.x] = u ? u[i0 + threadIdx.x] : 0.0;
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double vj = v_in ? v_in[j] : 0.0;
  const float* col = s + (int64_t)i0 * ld + j;
  float m = -__builtin_huge_valf();
  double sum = 0.0;
  for (int r0 = 0; r0 < rows; r0 += 4) {               // four rows in flight, pushed in row order
    float a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = col[(int64_t)min(r0 + k, rows - 1) * ld];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (r0 + k < rows) lse_push(m, sum, sk_entry(a[k], tau, su[r0 + k], vj));
  }
  pm[(int64_t)blockIdx.y * n + j] = m;
  ps[(int64_t)blockIdx.y * n + j] = sum;
}

// v_out[j] = v_in[j] + LSE over the row blocks, folded in the fixed order of sinkhorn_col_combine_kernel
__global__ __launch_bounds__(256) void skt_col_combine_kernel(const float* __restrict__ pm, const double* __restrict__ ps, int n, int nblk,
                                                              const double* __restrict__ v_in, double* __restrict__ v_out) {
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
      if (sb > 0.0) sum += sb * (double)expf(pm[(int64_t)b * n + j] - m);
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
    v_out[j] = (v_in ? v_in[j] : 0.0) + (double)lse_value(mm, tot);
  }
}

// ds_mat = exp((L - u) - v) and the row's share of sum_ij BCE(P_ij, [j == tgt_i]): both logs clamped at -100 like
// F.binary_cross_entropy; the logs are taken in fp64 of the fp32 entry, the row is summed in fp64.  One wave per row.
__global__ __launch_bounds__(256) void skt_exp_loss_kernel(const float* __restrict__ s, int64_t ld, int n, float tau,
                                                           const double* __restrict__ u, const double* __restrict__ v,
                                                           const int32_t* __restrict__ tgt, float* __restrict__ ds,
                                                           double* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* row = s + (int64_t)i * ld;
  const double ui = u ? u[i] : 0.0;
  const int t = tgt[i];
  double acc = 0.0;
  for (int j = lane; j < n; j += 64) {
    const float p = expf(sk_entry(row[j], tau, ui, v ? v[j] : 0.0));
    ds[(int64_t)i * n + j] = p;
    const double q = j == t ? (double)p : fmax(1.0 - (double)p, 0.0);
    acc -= fmax(log(q), -100.0);
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) rowloss[i] = acc;
}

// out[0] = sum of x[0 .. n) in a fixed order: a strided chain per thread, then a tree over the 256 threads
__global__ __launch_bounds__(256) void skt_fold_kernel(const double* __restrict__ x, int n, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// ------------------------------------------------------------------------------------------------ Sinkhorn backward
// PyTorch's binary_cross_entropy backward, (P - y) / max((1 - P) P, 1e-12) g, times P: dLoss / d log P
__device__ __forceinline__ float skt_g_init(float p, bool y, float g) {
  return (p - (y ? 1.0f : 0.0f)) / fmaxf((1.0f - p) * p, 1e-12f) * g * p;
}
__device__ __forceinline__ float skt_g_update(float gv, float p, double sum) { return (float)((double)gv - (double)p * sum); }

// a wave per row.  INIT: G = G_T from P = ds_mat; else the column step G -= P_i * cs[j].  Leaves rs[i] = the row sum of the new G.
// div: tau in the last pass (ds = G_0 / tau), 1 before.  SEED (with INIT): G holds dLoss' / dP of another term on entry and the pass
// writes G_T + P * seed (pfpp_sinkhorn_train_bwd_seeded).
template <bool INIT, bool SEED = false>
__global__ __launch_bounds__(256) void skt_bwd_rows_kernel(const float* __restrict__ s, int64_t ld, int n, float tau,
                                                           const double* __restrict__ u, const double* __restrict__ v,
                                                           const float* __restrict__ P, const int32_t* __restrict__ tgt, float g,
                                                           const double* __restrict__ cs, float* __restrict__ G, int64_t ldg, float div,
                                                           double* __restrict__ rs) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* row = INIT ? P + (int64_t)i * n : s + (int64_t)i * ld;
  float* grow = G + (int64_t)i * ldg;
  const double ui = (!INIT && u) ? u[i] : 0.0;
  const int t = INIT ? tgt[i] : -1;
  double acc = 0.0;
  for (int j0 = lane; j0 < n; j0 += 4 * 64) {            // four columns per lane in flight, summed in column order
    float a[4], gv[4];
    double vj[4], cj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + 64 * k;
      const int jc = j < n ? j : n - 1;
      a[k] = row[jc];
      if (!INIT) { gv[k] = grow[jc]; vj[k] = v ? v[jc] : 0.0; cj[k] = cs[jc]; }
      if (SEED) gv[k] = grow[jc];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + 64 * k;
      if (j < n) {
        float gn;
        if (INIT) gn = skt_g_init(a[k], j == t, g);
        else gn = skt_g_update(gv[k], expf(sk_entry(a[k], tau, ui, vj[k])), cj[k]);
        if (SEED) gn = gn + a[k] * gv[k];
        gn = gn / div;
        grow[j] = gn;
        acc += (double)gn;
      }
    }
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) rs[i] = acc;
}

// a thread per column over a block of 64 rows.  INIT as above; else the row step G -= P_i * rs[i].  Leaves cp[block, j] = the
// column sum of the new G over the block's rows, in row order.
template <bool INIT, bool SEED = false>
__global__ __launch_bounds__(256) void skt_bwd_cols_kernel(const float* __restrict__ s, int64_t ld, int n, float tau,
                                                           const double* __restrict__ u, const double* __restrict__ v,
                                                           const float* __restrict__ P, const int32_t* __restrict__ tgt, float g,
                                                           const double* __restrict__ rs, float* __restrict__ G, int64_t ldg, float div,
                                                           double* __restrict__ cp) {
  __shared__ double su[SK_ROWS], srs[SK_ROWS];
  __shared__ int st[SK_ROWS];
  const int i0 = blockIdx.y * SK_ROWS;
  const int rows = min(SK_ROWS, n - i0);
  if ((int)threadIdx.x < rows) {
    su[threadIdx.x] = (!INIT && u) ? u[i0 + threadIdx.x] : 0.0;
    srs[threadIdx.x] = INIT ? 0.0 : rs[i0 + threadIdx.x];
    st[threadIdx.x] = INIT ? tgt[i0 + threadIdx.x] : -1;
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double vj = (!INIT && v) ? v[j] : 0.0;
  const float* col = INIT ? P + (int64_t)i0 * n + j : s + (int64_t)i0 * ld + j;
  const int64_t lds_ = INIT ? (int64_t)n : ld;
  float* gcol = G + (int64_t)i0 * ldg + j;
  double acc = 0.0;
  for (int r0 = 0; r0 < rows; r0 += 4) {               // four rows in flight, summed in row order
    float a[4], gv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = min(r0 + k, rows - 1);
      a[k] = col[(int64_t)r * lds_];
      if (!INIT || SEED) gv[k] = gcol[(int64_t)r * ldg];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = r0 + k;
      if (r < rows) {
        float gn;
        if (INIT) gn = skt_g_init(a[k], j == st[r], g);
        else gn = skt_g_update(gv[k], expf(sk_entry(a[k], tau, su[r], vj)), srs[r]);
        if (SEED) gn = gn + a[k] * gv[k];
        gn = gn / div;
        gcol[(int64_t)r * ldg] = gn;
        acc += (double)gn;
      }
    }
  }
  cp[(int64_t)blockIdx.y * n + j] = acc;
}

// cs[j] = sum over the row blocks of cp[b, j]: the blocks of a column split over four waves, each in block order, the four folded in order
__global__ __launch_bounds__(256) void skt_bwd_col_combine_kernel(const double* __restrict__ cp, int n, int nblk, double* __restrict__ cs) {
  __shared__ double qs[CB_PARTS][CB_COLS];
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int j = blockIdx.x * CB_COLS + c;
  const int per = (nblk + CB_PARTS - 1) / CB_PARTS;
  const int b0 = part * per, b1 = min(nblk, b0 + per);
  double sum = 0.0;
  if (j < n) {
#pragma unroll 4
    for (int b = b0; b < b1; ++b) sum += cp[(int64_t)b * n + j];
  }
  qs[part][c] = sum;
  __syncthreads();
  if (part == 0 && j < n) cs[j] = ((qs[0][c] + qs[1][c]) + qs[2][c]) + qs[3][c];
}

// ------------------------------------------------------------------------------------------------ matching ground truth
constexpr int GT_TILE = 1024;

// tgt[r] = the column (local to the puzzle) of the nearest critical point of another piece; -1 when there is none
__global__ __launch_bounds__(256) void match_gt_targets_kernel(const float* __restrict__ gt_pcs, int64_t N, const int64_t* __restrict__ src,
                                                               const int32_t* __restrict__ row_piece, const int64_t* __restrict__ puz_row_off,
                                                               int32_t* __restrict__ tgt) {
  __shared__ float tx[GT_TILE], ty[GT_TILE], tz[GT_TILE], tb[GT_TILE];
  __shared__ int tp[GT_TILE];
  const int64_t r0 = puz_row_off[blockIdx.y], r1 = puz_row_off[blockIdx.y + 1];
  if (r0 + (int64_t)blockIdx.x * 256 >= r1) return;                // whole block past the puzzle (uniform)
  const int64_t r = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = r < r1;
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  int pa = -1;
  if (ok) {
    const int64_t q = min(max(src[r], (int64_t)0), N - 1);         // memory safety only
    ax = gt_pcs[3 * q]; ay = gt_pcs[3 * q + 1]; az = gt_pcs[3 * q + 2];
    pa = row_piece[r];
  }
  const float aa = (ax * ax + ay * ay) + az * az;
  float best = __builtin_huge_valf();
  int arg = -1;
  for (int64_t c0 = r0; c0 < r1; c0 += GT_TILE) {
    const int cnt = (int)min((int64_t)GT_TILE, r1 - c0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const int64_t q = min(max(src[c0 + j], (int64_t)0), N - 1);
      const float bx = gt_pcs[3 * q], by = gt_pcs[3 * q + 1], bz = gt_pcs[3 * q + 2];
      tx[j] = bx; ty[j] = by; tz[j] = bz; tb[j] = (bx * bx + by * by) + bz * bz;
      tp[j] = row_piece[c0 + j];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      // square_distance: -2 a.b + |a|^2 + |b|^2, clamped at 1e-12; ascending columns and a strict `<`: an exact tie keeps the lowest
      const float dot = (ax * tx[j] + ay * ty[j]) + az * tz[j];
      const float d = fmaxf((-2.0f * dot + aa) + tb[j], 1e-12f);
      if (tp[j] != pa && d < best) { best = d; arg = (int)(c0 - r0) + j; }
    }
  }
  if (ok) tgt[r] = arg;
}

// ------------------------------------------------------------------------------------------------ F.normalize backward
// y = x / max(|x|, eps) per 256-wide half: dx = dy / |x| - x (x . dy) / |x|^3, and dy / eps where the norm was clamped
__global__ __launch_bounds__(256) void match_normalize_halves_bwd_kernel(const float* __restrict__ x, const float* dy, float* dx,
                                                                         int64_t R) {      // dx may be dy: neither is __restrict__
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float4* xr = reinterpret_cast<const float4*>(x + r * (2 * MT_HALF));
  const float4* gr = reinterpret_cast<const float4*>(dy + r * (2 * MT_HALF));
  float4* out = reinterpret_cast<float4*>(dx + r * (2 * MT_HALF));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 a = xr[64 * h + lane], d = gr[64 * h + lane];
    const float ss = wave_sum_f32((a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w));
    const float dot = wave_sum_f32((a.x * d.x + a.y * d.y) + (a.z * d.z + a.w * d.w));
    const float nrm = sqrtf(ss);
    const float inv = 1.0f / fmaxf(nrm, 1e-12f);
    const float c = nrm >= 1e-12f ? dot * inv * inv * inv : 0.0f;
    float4 o;
    o.x = d.x * inv - a.x * c; o.y = d.y * inv - a.y * c; o.z = d.z * inv - a.z * c; o.w = d.w * inv - a.w * c;
    out[64 * h + lane] = o;
  }
}

// ------------------------------------------------------------------------------------------------ classifier loss
constexpr int CLS_BLOCKS = 1024;      // partial sums of the classifier loss: at most this many workgroups, folded in order

// per workgroup: sum of binary_cross_entropy_with_logits (fp32 per element like torch, fp64 sum) and the confusion counts of
// fp32 sigmoid(logit) > 0.5 against the label (tp, fp, tn, fn); dlogit = (sigmoid(logit) - y) g / N
__global__ __launch_bounds__(256) void match_cls_bce_kernel(const float* __restrict__ logits, int64_t ldl, const uint8_t* __restrict__ labels,
                                                            int64_t N, float g, float* __restrict__ dlogit, int64_t ldd,
                                                            double* __restrict__ part_loss, long long* __restrict__ part_cnt) {
  __shared__ double sl[256];
  __shared__ int sc[4][256];
  double acc = 0.0;
  int tp = 0, fp = 0, tn = 0, fn = 0;
  const float gn = g / (float)N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const float x = logits[i * ldl];
    const bool y = labels[i] != 0;
    const float sg = 1.0f / (1.0f + expf(-x));
    acc += (double)((fmaxf(x, 0.0f) - (y ? x : 0.0f)) + log1pf(expf(-fabsf(x))));
    if (dlogit) dlogit[i * ldd] = (sg - (y ? 1.0f : 0.0f)) * gn;
    const bool pred = sg > 0.5f;
    tp += pred && y; fp += pred && !y; tn += !pred && !y; fn += !pred && y;
  }
  sl[threadIdx.x] = acc;
  sc[0][threadIdx.x] = tp; sc[1][threadIdx.x] = fp; sc[2][threadIdx.x] = tn; sc[3][threadIdx.x] = fn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sl[threadIdx.x] += sl[threadIdx.x + o];
#pragma unroll
      for (int k = 0; k < 4; ++k) sc[k][threadIdx.x] += sc[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part_loss[blockIdx.x] = sl[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) part_cnt[4 * blockIdx.x + k] = sc[k][0];
  }
}

__global__ __launch_bounds__(64) void match_cls_fold_kernel(const double* __restrict__ part_loss, const long long* __restrict__ part_cnt, int nblk,
                                                            int64_t N, double* __restrict__ loss, int64_t* __restrict__ counts) {
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += part_loss[b];
    loss[0] = acc / (double)N;
  } else if (threadIdx.x <= 4) {
    long long c = 0;
    for (int b = 0; b < nblk; ++b) c += part_cnt[4 * b + (threadIdx.x - 1)];
    counts[threadIdx.x - 1] = c;
  }
}

// ------------------------------------------------------------------------------------------------ validation metrics
// One puzzle of validation_step in one launch of one workgroup: loss = sum_ij BCE(ds_ij, [j == tgt_i]) with skt_exp_loss_kernel's
// terms (fp64 logs of the fp32 entry, both clamped at -100) and (tp, fp, fn) of the assignment col against tgt.  Wave w takes rows w,
// w + 16, ...; a lane keeps one fp64 sum over all its rows and columns, the 64 lanes are folded by the butterfly, the 16 waves in
// order by thread 0: a fixed order, two runs agree bitwise.  An entry that is exactly 0 off the target column adds log(1) = 0 and
// is skipped: in the masked matrix those are the same-piece blocks.
constexpr int VM_WAVES = 16;
__global__ __launch_bounds__(64 * VM_WAVES) void match_val_metrics_kernel(const float* __restrict__ ds, int n, const int32_t* __restrict__ tgt,
                                                                         const int64_t* __restrict__ col, double* __restrict__ loss,
                                                                         int64_t* __restrict__ counts) {
  __shared__ double sl[VM_WAVES];
  __shared__ int stp[VM_WAVES], sgt[VM_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  int tp = 0, gt = 0;
  for (int i = w; i < n; i += VM_WAVES) {
    const float* row = ds + (int64_t)i * n;
    const int t = tgt[i];
    if (lane == 0) { tp += t >= 0 && col[i] == (int64_t)t; gt += t >= 0; }
    for (int j = lane; j < n; j += 64) {
      const float p = row[j];
      if (j != t && p == 0.0f) continue;
      const double q = j == t ? (double)p : fmax(1.0 - (double)p, 0.0);
      acc -= fmax(log(q), -100.0);
    }
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) { sl[w] = acc; stp[w] = tp; sgt[w] = gt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    int64_t ntp = 0, ngt = 0;
    for (int k = 0; k < VM_WAVES; ++k) { tot += sl[k]; ntp += stp[k]; ngt += sgt[k]; }
    loss[0] = tot;
    counts[0] = ntp; counts[1] = (int64_t)n - ntp; counts[2] = ngt - ntp;
  }
}

// ------------------------------------------------------------------------------------------------ raw rows
// out[r] = feats[idx[r]], a zero row where idx[r] is outside [0, N): 32 lanes x float4 = one 128-wide row
__global__ __launch_bounds__(256) void match_gather_raw_kernel(const float* __restrict__ feats, const int64_t* __restrict__ idx, int64_t N,
                                                               int64_t R, float* __restrict__ out) {
  const int sub = threadIdx.x & 31;
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= R) return;
  const int64_t q = idx[r];
  float4 x = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q >= 0 && q < N) x = reinterpret_cast<const float4*>(feats + q * MT_C)[sub];
  reinterpret_cast<float4*>(out + r * MT_C)[sub] = x;
}

// its transpose: out[idx[r]] (+)= in[r]; every point occurs at most once, so plain stores
__global__ __launch_bounds__(256) void match_scatter_raw_kernel(const float* __restrict__ in, const int64_t* __restrict__ idx, int64_t N,
                                                                int64_t R, int accumulate, float* __restrict__ out) {
  const int sub = threadIdx.x & 31;
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= R) return;
  const int64_t q = idx[r];
  if (q < 0 || q >= N) return;
  float4 x = reinterpret_cast<const float4*>(in + r * MT_C)[sub];
  float4* dst = reinterpret_cast<float4*>(out + q * MT_C) + sub;
  if (accumulate) {
    const float4 o = *dst;
    x.x += o.x; x.y += o.y; x.z += o.z; x.w += o.w;
  }
  *dst = x;
}

// ------------------------------------------------------------------------------------------------ ordered column sums
// the bias gradients: part[block, c] = sum of x[r, c] over the block's 64 rows in row order (fp64), then the blocks in block order.
// pfpp_colsum ends in float atomics, whose order differs from run to run; here two runs agree bitwise.
constexpr int OC_ROWS = 64;

__global__ __launch_bounds__(256) void match_colsum_part_kernel(const float* __restrict__ x, int64_t ld, int64_t rows, int cols,
                                                                double* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * OC_ROWS, r1 = min(rows, r0 + OC_ROWS);
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) acc += (double)x[r * ld + c];
  part[(int64_t)blockIdx.y * cols + c] = acc;
}

__global__ __launch_bounds__(256) void match_colsum_fold_kernel(const double* __restrict__ part, int64_t nblk, int cols, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double acc = 0.0;
  for (int64_t b = 0; b < nblk; ++b) acc += part[b * cols + c];
  out[c] = (float)acc;
}

// workspace of the training Sinkhorn: column partials (fp64 sums, fp32 maxima) and two fp64 vectors (row sums / row losses, column sums)
struct SktWs {
  double* ps;
  double* rs;
  double* cs;
  float* pm;
};
SktWs skt_carve(void* workspace, int64_t n, int64_t nblk) {
  SktWs w;
  w.ps = static_cast<double*>(workspace);
  w.rs = w.ps + nblk * n;
  w.cs = w.rs + n;
  w.pm = reinterpret_cast<float*>(w.cs + n);
  return w;
}

}  // namespace

extern "C" int64_t pfpp_sinkhorn_train_workspace(int64_t n) {
  if (n < 0 || n > 65535) return -1;
  const int64_t nblk = (n + SK_ROWS - 1) / SK_ROWS;
  return nblk * n * (int64_t)(sizeof(double) + sizeof(float)) + 2 * n * (int64_t)sizeof(double);
}

extern "C" int pfpp_sinkhorn_train_fwd(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt, double* pots,
                                       float* ds_mat, double* loss, double* row_loss, void* workspace, int64_t workspace_bytes,
                                       pfpp_stream_t stream) {
  PFPP_REQUIRE(s && tgt && ds_mat && loss && (pots || max_iter == 0), "null pointer");
  PFPP_REQUIRE(n >= 1 && ld >= n && max_iter >= 0 && tau > 0.0f, "bad sizes");
  PFPP_SUPPORTED(n <= 65535, "more than 65535 critical points in one puzzle");
  PFPP_REQUIRE(workspace && workspace_bytes >= pfpp_sinkhorn_train_workspace(n), "workspace smaller than pfpp_sinkhorn_train_workspace(n)");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "workspace must be 8-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  const int nn = (int)n, nblk = (nn + SK_ROWS - 1) / SK_ROWS;
  const SktWs w = skt_carve(workspace, n, nblk);
  const unsigned cblk = (unsigned)((nn + 255) / 256), rblk = (unsigned)((nn + 3) / 4);
  const double *u = nullptr, *v = nullptr;          // the potentials after the steps taken so far (null = zeros)
  for (int64_t it = 0; it < max_iter; ++it) {
    double* out = pots + it * n;
    if (it % 2 == 0) {
      hipLaunchKernelGGL(skt_row_kernel, dim3(rblk), dim3(256), 0, st, s, ld, nn, tau, u, v, out);
      u = out;
    } else {
      hipLaunchKernelGGL(skt_col_partial_kernel, dim3(cblk, (unsigned)nblk), dim3(256), 0, st, s, ld, nn, tau, u, v, w.pm, w.ps);
      hipLaunchKernelGGL(skt_col_combine_kernel, dim3((unsigned)((nn + CB_COLS - 1) / CB_COLS)), dim3(256), 0, st, w.pm, w.ps, nn, nblk, v, out);
      v = out;
    }
  }
  double* rows = row_loss ? row_loss : w.rs;        // the per-row losses: the caller's [n], or scratch
  hipLaunchKernelGGL(skt_exp_loss_kernel, dim3(rblk), dim3(256), 0, st, s, ld, nn, tau, u, v, tgt, ds_mat, rows);
  hipLaunchKernelGGL(skt_fold_kernel, dim3(1), dim3(256), 0, st, rows, nn, loss);
  return pfpp::check_launch(__func__);
}

namespace {
// both backward entries: SEED = ds holds a further term's dLoss' / d ds_mat on entry.  The checks report under the entry's name.
template <bool SEED>
int skt_bwd_run(const char* func, const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt, const double* pots,
                const float* ds_mat, float g, float* ds, int64_t ldg, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream) {
  const char* bad = nullptr;
  if (!(s && tgt && ds_mat && ds && (pots || max_iter == 0))) bad = "null pointer";
  else if (!(n >= 1 && ld >= n && ldg >= n && max_iter >= 0 && tau > 0.0f)) bad = "bad sizes";
  else if (n > 65535) {
    pfpp::set_error("%s: unsupported: %s", func, "more than 65535 critical points in one puzzle");
    return PFPP_EUNSUPPORTED;
  } else if (!(workspace && workspace_bytes >= pfpp_sinkhorn_train_workspace(n))) bad = "workspace smaller than pfpp_sinkhorn_train_workspace(n)";
  else if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) bad = "workspace must be 8-byte aligned";
  if (bad) {
    pfpp::set_error("%s: %s", func, bad);
    return PFPP_EINVAL;
  }
  hipStream_t st = pfpp::as_stream(stream);
  const int nn = (int)n, nblk = (nn + SK_ROWS - 1) / SK_ROWS;
  const SktWs w = skt_carve(workspace, n, nblk);
  const dim3 rgrid((unsigned)((nn + 3) / 4)), cgrid((unsigned)((nn + 255) / 256), (unsigned)nblk);
  const unsigned fgrid = (unsigned)((nn + CB_COLS - 1) / CB_COLS);
  const float one = 1.0f;
  // G_T, in the layout whose sums step T - 1 needs: a row step (T - 1 even) reads row sums, a column step column sums
  if (max_iter == 0 || (max_iter - 1) % 2 == 0) {
    hipLaunchKernelGGL((skt_bwd_rows_kernel<true, SEED>), rgrid, dim3(256), 0, st, s, ld, nn, tau, nullptr, nullptr, ds_mat, tgt, g, nullptr, ds, ldg,
                       max_iter == 0 ? tau : one, w.rs);
  } else {
    hipLaunchKernelGGL((skt_bwd_cols_kernel<true, SEED>), cgrid, dim3(256), 0, st, s, ld, nn, tau, nullptr, nullptr, ds_mat, tgt, g, nullptr, ds, ldg, one,
                       w.ps);
    hipLaunchKernelGGL(skt_bwd_col_combine_kernel, dim3(fgrid), dim3(256), 0, st, w.ps, nn, nblk, w.cs);
  }
  for (int64_t it = max_iter - 1; it >= 0; --it) {
    const double* mine = pots + it * n;                              // the vector step `it` wrote
    const double* other = it >= 1 ? pots + (it - 1) * n : nullptr;   // the other direction's, as step `it` read it
    if (it % 2 == 0) {          // row step: G -= P_it * rowsum(G); leaves the column partials the (odd) step before it reads
      hipLaunchKernelGGL(skt_bwd_cols_kernel<false>, cgrid, dim3(256), 0, st, s, ld, nn, tau, mine, other, nullptr, nullptr, 0.0f, w.rs, ds, ldg,
                         it == 0 ? tau : one, w.ps);
      if (it > 0) hipLaunchKernelGGL(skt_bwd_col_combine_kernel, dim3(fgrid), dim3(256), 0, st, w.ps, nn, nblk, w.cs);
    } else {                    // column step: G -= P_it * colsum(G); leaves the row sums the (even) step before it reads
      hipLaunchKernelGGL(skt_bwd_rows_kernel<false>, rgrid, dim3(256), 0, st, s, ld, nn, tau, other, mine, nullptr, nullptr, 0.0f, w.cs, ds, ldg,
                         one, w.rs);
    }
  }
  return pfpp::check_launch(func);
}
}  // namespace

extern "C" int pfpp_sinkhorn_train_bwd(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt,
                                       const double* pots, const float* ds_mat, float g, float* ds, int64_t ldg, void* workspace,
                                       int64_t workspace_bytes, pfpp_stream_t stream) {
  return skt_bwd_run<false>(__func__, s, ld, n, tau, max_iter, tgt, pots, ds_mat, g, ds, ldg, workspace, workspace_bytes, stream);
}

extern "C" int pfpp_sinkhorn_train_bwd_seeded(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt,
                                              const double* pots, const float* ds_mat, float g, float* ds, int64_t ldg, void* workspace,
                                              int64_t workspace_bytes, pfpp_stream_t stream) {
  return skt_bwd_run<true>(__func__, s, ld, n, tau, max_iter, tgt, pots, ds_mat, g, ds, ldg, workspace, workspace_bytes, stream);
}

extern "C" int pfpp_match_gt_targets(const float* gt_pcs, int64_t N, const int64_t* src, const int32_t* row_piece, const int64_t* puz_row_off,
                                     int64_t B, int64_t max_rows, int32_t* tgt, pfpp_stream_t stream) {
  PFPP_REQUIRE(gt_pcs && src && row_piece && puz_row_off && tgt, "null pointer");
  PFPP_REQUIRE(N >= 1 && B >= 0 && max_rows >= 0, "bad sizes");
  PFPP_SUPPORTED(B <= 65535, "more than 65535 puzzles per launch");
  PFPP_SUPPORTED(max_rows <= 65535, "more than 65535 critical points in one puzzle");
  if (B == 0 || max_rows == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_gt_targets_kernel, dim3((unsigned)((max_rows + 255) / 256), (unsigned)B), dim3(256), 0, pfpp::as_stream(stream),
                     gt_pcs, N, src, row_piece, puz_row_off, tgt);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_normalize_halves_bwd(const float* x, const float* dy, float* dx, int64_t R, int64_t D, pfpp_stream_t stream) {
  PFPP_REQUIRE(x && dy && dx && R >= 0, "null pointer or bad sizes");
  PFPP_SUPPORTED(D == 2 * MT_HALF, "AFF_FEAT_DIM other than 512");
  PFPP_REQUIRE(pfpp::aligned16(x) && pfpp::aligned16(dy) && pfpp::aligned16(dx), "x, dy and dx must be 16-byte aligned");
  PFPP_SUPPORTED(R <= (int64_t)1 << 33, "too many rows");
  if (R == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_normalize_halves_bwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, pfpp::as_stream(stream), x, dy, dx, R);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_match_cls_bce_workspace(void) { return CLS_BLOCKS * (int64_t)(sizeof(double) + 4 * sizeof(long long)); }

extern "C" int pfpp_match_cls_bce(const float* logits, int64_t ldl, const uint8_t* labels, int64_t N, float g, double* loss, float* dlogit,
                                  int64_t ldd, int64_t* counts, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(logits && labels && loss && counts && workspace, "null pointer");
  PFPP_REQUIRE(workspace_bytes >= pfpp_match_cls_bce_workspace(), "workspace smaller than pfpp_match_cls_bce_workspace()");
  PFPP_REQUIRE(N >= 1 && ldl >= 1 && (!dlogit || ldd >= 1), "bad sizes");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "workspace must be 8-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  const int nblk = (N + 255) / 256 < CLS_BLOCKS ? (int)((N + 255) / 256) : CLS_BLOCKS;
  double* part_loss = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(part_loss + CLS_BLOCKS);
  hipLaunchKernelGGL(match_cls_bce_kernel, dim3((unsigned)nblk), dim3(256), 0, st, logits, ldl, labels, N, g, dlogit, ldd, part_loss, part_cnt);
  hipLaunchKernelGGL(match_cls_fold_kernel, dim3(1), dim3(64), 0, st, part_loss, part_cnt, nblk, N, loss, counts);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_match_colsum_ordered_workspace(int64_t rows, int64_t cols) {
  if (rows < 0 || cols < 1) return -1;
  return ((rows + OC_ROWS - 1) / OC_ROWS) * cols * (int64_t)sizeof(double);
}

extern "C" int pfpp_match_colsum_ordered(const float* x, int64_t ld, int64_t rows, int64_t cols, float* out, void* workspace,
                                         int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(x && out, "null pointer");
  PFPP_REQUIRE(rows >= 0 && cols >= 1 && ld >= cols, "bad sizes");
  PFPP_SUPPORTED(cols <= 65536 && rows <= (int64_t)65535 * OC_ROWS, "more than 65536 columns or 4193280 rows");
  PFPP_REQUIRE(rows == 0 || (workspace && workspace_bytes >= pfpp_match_colsum_ordered_workspace(rows, cols)),
               "workspace smaller than pfpp_match_colsum_ordered_workspace(rows, cols)");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "workspace must be 8-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  const int64_t nblk = (rows + OC_ROWS - 1) / OC_ROWS;
  const unsigned cblk = (unsigned)((cols + 255) / 256);
  double* part = static_cast<double*>(workspace);
  if (nblk > 0)
    hipLaunchKernelGGL(match_colsum_part_kernel, dim3(cblk, (unsigned)nblk), dim3(256), 0, st, x, ld, rows, (int)cols, part);
  hipLaunchKernelGGL(match_colsum_fold_kernel, dim3(cblk), dim3(256), 0, st, part, nblk, (int)cols, out);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_gather_raw(const float* feats, const int64_t* idx, int64_t N, int64_t R, int64_t C, float* out, pfpp_stream_t stream) {
  PFPP_REQUIRE(feats && idx && out, "null pointer");
  PFPP_REQUIRE(N >= 0 && R >= 0, "bad sizes");
  PFPP_SUPPORTED(C == MT_C, "PC_FEAT_DIM other than 128");
  PFPP_REQUIRE(pfpp::aligned16(feats) && pfpp::aligned16(out), "feats and out must be 16-byte aligned");
  PFPP_SUPPORTED(R <= (int64_t)1 << 33, "too many rows");
  if (R == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_gather_raw_kernel, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, pfpp::as_stream(stream), feats, idx, N, R, out);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_scatter_raw(const float* in, const int64_t* idx, int64_t N, int64_t R, int64_t C, int accumulate, float* out,
                                      pfpp_stream_t stream) {
  PFPP_REQUIRE(in && idx && out, "null pointer");
  PFPP_REQUIRE(N >= 0 && R >= 0, "bad sizes");
  PFPP_SUPPORTED(C == MT_C, "PC_FEAT_DIM other than 128");
  PFPP_REQUIRE(pfpp::aligned16(in) && pfpp::aligned16(out), "in and out must be 16-byte aligned");
  PFPP_SUPPORTED(R <= (int64_t)1 << 33, "too many rows");
  if (R == 0) return PFPP_OK;
  hipLaunchKernelGGL(match_scatter_raw_kernel, dim3((unsigned)((R + 7) / 8)), dim3(256), 0, pfpp::as_stream(stream), in, idx, N, R, accumulate,
                     out);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_match_val_metrics(const float* ds_mat, int64_t n, const int32_t* tgt, const int64_t* col, double* loss, int64_t* counts,
                                      pfpp_stream_t stream) {
  PFPP_REQUIRE(ds_mat && tgt && col && loss && counts, "null pointer");
  PFPP_REQUIRE(n >= 1, "bad sizes");
  PFPP_SUPPORTED(n <= 65535, "more than 65535 critical points in one puzzle");
  hipLaunchKernelGGL(match_val_metrics_kernel, dim3(1), dim3(64 * VM_WAVES), 0, pfpp::as_stream(stream), ds_mat, (int)n, tgt, col, loss, counts);
  return pfpp::check_launch(__func__);
}
