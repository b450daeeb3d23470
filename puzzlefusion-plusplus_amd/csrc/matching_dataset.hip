// The matcher's training batches from a resident mesh store (Jigsaw_matching/dataset/all_piece_matching_dataset.py:
// AllPieceMatchingDataset._get_pcs :195-224 and __getitem__ :226-278) for a selection sel [B] of the store's puzzles.
//
//  * pfpp_mdata_piece_counts — sample_reweighted_points_by_areas (:164-193) per selected puzzle: one workgroup per puzzle stages the
//    parts' areas (the store's `total`) in LDS and one lane restates np.sum's order for 2..32 values, ceil(areas N / total) in
//    int32, the surplus taken from the first argmax, the raise to min_part_point and the `while delta > 0` loop, exactly.  Every
//    puzzle gets exactly N rows, so puzzle b owns rows [b N, (b + 1) N) and nothing here depends on another puzzle.
//  * pfpp_mdata_sample — one thread per output row (b, r): its piece among at most 32 offsets, its sample index s (order[b, r] or
//    the local row), its uniforms (given, or pfpp_rng_u64 keyed by puzzle, slot and s), then pfpp_mesh::sample_point — the face
//    search and fold of sample_surface_kernel.  The fp64 point goes to the workspace at the sample's position (piece offset + s:
//    the order the reference's centroid sums in), gt_pcs = float32 of it at row r.
//  * pfpp_mdata_pose — _recenter_pc and _rotate_pc (:117-139), one workgroup per piece.  np.mean(pc, axis = 0) is the rows added
//    in row order and one division: the rows are staged in LDS in tiles of 256 with coalesced loads, lanes 0..2 carry the three
//    running sums through the tile in row order (a serial chain of n fp64 additions per coordinate), then all lanes rotate
//    p - c by the piece's matrix, ((R0 x + R1 y) + R2 z) with contraction off, and write float32.  The matrix is given, or lane 0
//    draws a unit quaternion by Marsaglia's rejection method (sqrt and division only, so numpy restates it bit for bit).
//
// No float atomics; the status word (csrc/mesh_common.h) takes integer atomicMin only; nothing is read from the environment.
#include <math.h>

#include "mesh_common.h"
#include "pfpp_common.h"

namespace {

using namespace pfpp_mesh;

constexpr int MD_BLOCK = 256;
constexpr int MD_MAX_PARTS = 32;
constexpr int MD_ATTEMPTS = 64;
// the rotations' generator runs under seed ^ MD_ROT_SEED, so its keys never meet the sampling uniforms' (include/pfpp.h)
constexpr uint64_t MD_ROT_SEED = 0xA5B85C5E198ED849ull;

// ------------------------------------------------------------------------------------------------ piece counts
__global__ __launch_bounds__(PFPP_WAVE) void piece_counts_kernel(const double* __restrict__ total, const int64_t* __restrict__ store_part_off,
                                                                 const int64_t* __restrict__ sel, int64_t S, int N, int min_part_point,
                                                                 int max_parts, int64_t* __restrict__ n_pcs, int64_t* __restrict__ piece_off,
                                                                 int64_t* __restrict__ puz_piece_off, uint64_t* status) {
  __shared__ double a[MD_MAX_PARTS];
  __shared__ int32_t nps[MD_MAX_PARTS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t puzzle = sel[b];
  const bool known = puzzle >= 0 && puzzle < S;
  const int64_t p0 = known ? store_part_off[puzzle] : 0;
  const int64_t P64 = known ? store_part_off[puzzle + 1] - p0 : 0;
  const int P = (P64 >= 1 && P64 <= max_parts) ? (int)P64 : 0;
  if (tid < MD_MAX_PARTS) {
    a[tid] = tid < P ? total[p0 + tid] : 0.0;
    nps[tid] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    bool ok = P > 0 && (int64_t)P * (min_part_point > 1 ? min_part_point : 1) <= N;
    if (!ok) report(status, ST_COUNTS, b);
    for (int k = 0; k < P && ok; ++k)
      if (!(a[k] > 0.0) || !isfinite(a[k])) {
        report(status, ST_AREA, p0 + k);
        ok = false;
      }
    if (ok) {
      // np.sum(areas): numpy's pairwise_sum for n <= 128
      double tot;
      if (P < 8) {
        tot = 0.0;
        for (int i = 0; i < P; ++i) tot = tot + a[i];
      } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < P - (P % 8); i += 8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
        }
        tot = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < P; ++i) tot = tot + a[i];
      }
      ok = isfinite(tot);
      if (!ok) report(status, ST_AREA, p0);
      if (ok) {
        // sample_points_by_areas (:164-169)
        int64_t sum = 0;
        for (int k = 0; k < P; ++k) {
          const double c = ceil(a[k] * (double)N / tot);
          nps[k] = (c >= 1.0 && c <= (double)N) ? (int32_t)c : 0;
          ok = ok && nps[k] > 0;
          sum += nps[k];
        }
        int kmax = 0;
        for (int k = 1; k < P; ++k)
          if (nps[k] > nps[kmax]) kmax = k;
        nps[kmax] -= (int32_t)(sum - N);
        // sample_reweighted_points_by_areas (:176-193)
        if (ok && min_part_point > 1) {
          int64_t delta = 0;
          for (int k = 0; k < P; ++k)
            if (nps[k] < min_part_point) {
              delta += min_part_point - nps[k];
              nps[k] = min_part_point;
            }
          for (int it = 0; it <= P && delta > 0; ++it) {          // each pass ends the loop or clamps one more piece
            int k = 0;
            for (int q = 1; q < P; ++q)
              if (nps[q] > nps[k]) k = q;
            if (nps[k] - delta >= min_part_point) {
              nps[k] -= (int32_t)delta;
              delta = 0;
            } else {
              delta -= nps[k] - min_part_point;
              nps[k] = min_part_point;
            }
          }
          ok = delta == 0;
        }
        sum = 0;
        for (int k = 0; k < P; ++k) {
          ok = ok && nps[k] >= 0;
          sum += nps[k];
        }
        ok = ok && sum == N;
        if (!ok) report(status, ST_COUNTS, b);
      }
    }
    if (!ok) {            // keep every later kernel inside the puzzle's N rows: all of them in slot 0
      for (int k = 0; k < MD_MAX_PARTS; ++k) nps[k] = 0;
      nps[0] = N;
    }
    int64_t off = (int64_t)b * N;
    for (int k = 0; k < max_parts; ++k) {
      piece_off[(int64_t)b * max_parts + k] = off;
      n_pcs[(int64_t)b * max_parts + k] = nps[k];
      off += nps[k];
    }
    puz_piece_off[b] = (int64_t)b * max_parts;
    if (b == (int)gridDim.x - 1) {
      piece_off[(int64_t)(b + 1) * max_parts] = off;
      puz_piece_off[b + 1] = (int64_t)(b + 1) * max_parts;
    }
  }
}

// ------------------------------------------------------------------------------------------------ ragged surface samples
__global__ __launch_bounds__(MD_BLOCK) void ragged_sample_kernel(
    const double* __restrict__ verts, const int32_t* __restrict__ faces, const int64_t* __restrict__ vert_off,
    const int64_t* __restrict__ face_off, const double* __restrict__ cdf, const double* __restrict__ total,
    const int64_t* __restrict__ store_part_off, const int64_t* __restrict__ store_data_id, const int64_t* __restrict__ sel, int64_t S,
    const int64_t* __restrict__ piece_off, int N, int max_parts, const int32_t* __restrict__ order, const double* __restrict__ u,
    uint64_t seed, uint32_t split, double* __restrict__ points, float* __restrict__ gt_pcs, int32_t* __restrict__ face_idx,
    uint64_t* status) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * MD_BLOCK + threadIdx.x;
  if (r >= N) return;
  const int64_t base = (int64_t)b * N, row = base + r;
  const double nan = __builtin_nan("");
  const int64_t puzzle = sel[b];
  const int64_t* po = piece_off + (int64_t)b * max_parts;
  int slot = 0;
  for (int k = 1; k < max_parts; ++k)
    if (po[k] - base <= r) slot = k;
  const int64_t o0 = po[slot] - base, n = po[slot + 1] - po[slot];
  const int64_t j = r - o0;
  bool ok = puzzle >= 0 && puzzle < S && o0 >= 0 && j >= 0 && j < n && o0 + n <= N;
  int64_t P = 0, part = 0;
  if (ok) {
    part = store_part_off[puzzle] + slot;
    P = store_part_off[puzzle + 1] - store_part_off[puzzle];
    ok = slot < P;
  }
  if (!ok) {          // the counts kernel reported why; this row holds no sample
    gt_pcs[row * 3 + 0] = gt_pcs[row * 3 + 1] = gt_pcs[row * 3 + 2] = __builtin_nanf("");
    points[row * 3 + 0] = points[row * 3 + 1] = points[row * 3 + 2] = nan;
    if (face_idx) face_idx[row] = -1;
    return;
  }
  int64_t s = j;
  if (order) {
    s = order[row];
    if (s < 0 || s >= n) {
      report(status, ST_ORDER, b);
      s = j;
    }
  }
  const int64_t at = base + o0 + s;          // the sample's position: piece order
  double u0, l0, l1;
  if (u) {
    u0 = u[at * 3 + 0]; l0 = u[at * 3 + 1]; l1 = u[at * 3 + 2];
  } else {
    const uint64_t key = (((uint64_t)store_data_id[puzzle] * (uint64_t)max_parts + (uint64_t)slot) * (uint64_t)N + (uint64_t)s) * 3ull;
    u0 = uniform53(seed, split, key + 0);
    l0 = uniform53(seed, split, key + 1);
    l1 = uniform53(seed, split, key + 2);
  }
  const int64_t fo = face_off[part], nf = face_off[part + 1] - fo;
  const int64_t vo = vert_off[part], nv = vert_off[part + 1] - vo;
  double p[3] = {nan, nan, nan};
  int64_t f = -1;
  if (nf > 0) f = sample_point(verts + vo * 3, faces + fo * 3, nv, nf, cdf + fo, total[part], u0, l0, l1, p);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    points[at * 3 + k] = p[k];
    gt_pcs[row * 3 + k] = (float)p[k];
  }
  if (face_idx) face_idx[row] = (int32_t)f;
}

// ------------------------------------------------------------------------------------------------ centroid, rotation, float32
// Marsaglia (1972): (x1, x2) and (y1, y2) uniform in the unit disc, q = (x1, x2, y1 f, y2 f) with f = sqrt((1 - s1) / s2) is uniform
// on the 3-sphere.  Each pair keeps the first attempt that falls inside; attempt t reads keys (base + t) 4 + {0, 1} and {2, 3}.
__device__ bool marsaglia_quat(uint64_t seed, uint32_t split, uint64_t base, double q[4]) {
  bool have1 = false, have2 = false;
  double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0, s1 = 0.0, s2 = 1.0;
  for (int t = 0; t < MD_ATTEMPTS && !(have1 && have2); ++t) {
    const uint64_t key = (base + (uint64_t)t) * 4ull;
    if (!have1) {
      const double c = 2.0 * uniform53(seed, split, key + 0) - 1.0, d = 2.0 * uniform53(seed, split, key + 1) - 1.0;
      const double s = c * c + d * d;
      if (s < 1.0) { x1 = c; x2 = d; s1 = s; have1 = true; }
    }
    if (!have2) {
      const double c = 2.0 * uniform53(seed, split, key + 2) - 1.0, d = 2.0 * uniform53(seed, split, key + 3) - 1.0;
      const double s = c * c + d * d;
      if (s > 0.0 && s < 1.0) { y1 = c; y2 = d; s2 = s; have2 = true; }
    }
  }
  if (!(have1 && have2)) {
    q[0] = 1.0; q[1] = q[2] = q[3] = 0.0;
    return false;
  }
  const double f = sqrt((1.0 - s1) / s2);
  q[0] = x1; q[1] = x2; q[2] = y1 * f; q[3] = y2 * f;
  return true;
}

__global__ __launch_bounds__(MD_BLOCK) void pose_kernel(const double* __restrict__ points, const int64_t* __restrict__ piece_off,
                                                        const int64_t* __restrict__ store_data_id, const int64_t* __restrict__ sel, int64_t S,
                                                        int64_t rows, int max_parts, const int32_t* __restrict__ order,
                                                        const double* __restrict__ rot, uint64_t seed, uint32_t split,
                                                        float* __restrict__ part_pcs, float* __restrict__ part_quat,
                                                        float* __restrict__ part_trans, double* __restrict__ rot_out) {
  __shared__ double tile[MD_BLOCK * 3];
  __shared__ double cen[3];
  __shared__ double R[9];
  const int piece = blockIdx.x, tid = threadIdx.x;
  const int b = piece / max_parts, slot = piece % max_parts;
  const int64_t r0 = piece_off[piece];
  int64_t n = piece_off[piece + 1] - r0;
  if (r0 < 0 || n < 0 || r0 + n > rows) n = 0;
  if (n == 0) {          // _pad_data: zeros behind the valid pieces
    if (tid < 3) part_trans[(int64_t)piece * 3 + tid] = 0.f;
    if (tid < 4 && part_quat) part_quat[(int64_t)piece * 4 + tid] = 0.f;
    if (tid < 9 && rot_out) rot_out[(int64_t)piece * 9 + tid] = 0.0;
    return;
  }
  // the matrix first (R is read behind the barriers of the first tile)
  if (rot) {
    if (tid < 9) R[tid] = rot[(int64_t)piece * 9 + tid];
  } else if (tid == 0) {
    const int64_t puzzle = sel[b];
    const uint64_t id = (puzzle >= 0 && puzzle < S) ? (uint64_t)store_data_id[puzzle] : 0ull;
    double q[4];
    marsaglia_quat(seed ^ MD_ROT_SEED, split, (id * (uint64_t)max_parts + (uint64_t)slot) * (uint64_t)MD_ATTEMPTS, q);
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    if (part_quat) {          // the quaternion of R^T: rot_mat maps the centred piece to part_pcs, part_quat takes it back
      float* pq = part_quat + (int64_t)piece * 4;
      pq[0] = (float)w; pq[1] = (float)(-x); pq[2] = (float)(-y); pq[3] = (float)(-z);
    }
  }
  // np.mean(pc, axis = 0): the first row, then every further row added in row order, one division
  const double* src = points + r0 * 3;
  double acc = 0.0;
  for (int64_t t0 = 0; t0 < n; t0 += MD_BLOCK) {
    const int m = (int)((n - t0) < MD_BLOCK ? (n - t0) : MD_BLOCK);
    for (int e = tid; e < m * 3; e += MD_BLOCK) tile[e] = src[t0 * 3 + e];
    __syncthreads();
    if (tid < 3) {
      int i = 0;
      if (t0 == 0) { acc = tile[tid]; i = 1; }
      for (; i + 8 <= m; i += 8) {          // eight LDS reads in flight, then the same additions in the same order
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = tile[(i + q) * 3 + tid];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = acc + v[q];
      }
      for (; i < m; ++i) acc = acc + tile[i * 3 + tid];
    }
    __syncthreads();
  }
  if (tid < 3) {
    const double c = acc / (double)n;
    cen[tid] = c;
    part_trans[(int64_t)piece * 3 + tid] = (float)c;
  }
  __syncthreads();
  if (tid < 9 && rot_out) rot_out[(int64_t)piece * 9 + tid] = R[tid];
  const double c0 = cen[0], c1 = cen[1], c2 = cen[2];
  for (int64_t j = tid; j < n; j += MD_BLOCK) {
    int64_t s = j;
    if (order) {
      s = order[r0 + j];
      if (s < 0 || s >= n) s = j;          // reported by the sampling kernel
    }
    const double x = src[s * 3 + 0] - c0, y = src[s * 3 + 1] - c1, z = src[s * 3 + 2] - c2;
    float* out = part_pcs + (r0 + j) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (float)((R[k * 3 + 0] * x + R[k * 3 + 1] * y) + R[k * 3 + 2] * z);
  }
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + MD_BLOCK - 1) / MD_BLOCK); }

inline bool sizes_ok(int64_t B, int64_t S, int64_t N, int64_t max_parts) {
  return B >= 0 && S >= 0 && N >= 1 && max_parts >= 1;
}

}  // namespace

extern "C" int pfpp_mdata_piece_counts(const double* total, const int64_t* store_part_off, const int64_t* sel, int64_t B, int64_t S,
                                       int64_t num_points, int64_t min_part_point, int64_t max_parts, int64_t* n_pcs, int64_t* piece_off,
                                       int64_t* puz_piece_off, uint64_t* status, pfpp_stream_t stream) {
  PFPP_REQUIRE(total && store_part_off && sel && n_pcs && piece_off && puz_piece_off && status, "null pointer");
  PFPP_REQUIRE(sizes_ok(B, S, num_points, max_parts), "bad sizes");
  PFPP_SUPPORTED(max_parts <= MD_MAX_PARTS, "max_num_part > 32");
  PFPP_SUPPORTED(num_points <= 0x7fffffff && min_part_point <= 0x7fffffff && min_part_point >= -0x7fffffff && B <= 0x7fffffff &&
                     B * num_points <= ((int64_t)1 << 40),
                 "more than 2^31 - 1 points per puzzle or puzzles, or 2^40 rows");
  if (B == 0) return PFPP_OK;
  hipLaunchKernelGGL(piece_counts_kernel, dim3((unsigned)B), dim3(PFPP_WAVE), 0, pfpp::as_stream(stream), total, store_part_off, sel, S,
                     (int)num_points, (int)min_part_point, (int)max_parts, n_pcs, piece_off, puz_piece_off, status);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_mdata_sample(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off,
                                 const double* cdf, const double* total, const int64_t* store_part_off, const int64_t* store_data_id,
                                 const int64_t* sel, const int64_t* piece_off, int64_t B, int64_t S, int64_t num_points, int64_t max_parts,
                                 const int32_t* order, const double* u, uint64_t seed, uint32_t split, double* points, float* gt_pcs,
                                 int32_t* face_idx, uint64_t* status, pfpp_stream_t stream) {
  PFPP_REQUIRE(verts && faces && vert_off && face_off && cdf && total && store_part_off && store_data_id && sel && piece_off && points &&
                   gt_pcs && status,
               "null pointer");
  PFPP_REQUIRE(sizes_ok(B, S, num_points, max_parts), "bad sizes");
  PFPP_SUPPORTED(max_parts <= MD_MAX_PARTS, "max_num_part > 32");
  PFPP_SUPPORTED(num_points <= 0x7fffffff && B <= 65535, "more than 2^31 - 1 points per puzzle or 65535 puzzles in a batch");
  if (B == 0) return PFPP_OK;
  hipLaunchKernelGGL(ragged_sample_kernel, dim3(grid_of(num_points), (unsigned)B), dim3(MD_BLOCK), 0, pfpp::as_stream(stream), verts, faces,
                     vert_off, face_off, cdf, total, store_part_off, store_data_id, sel, S, piece_off, (int)num_points, (int)max_parts, order, u,
                     seed, split, points, gt_pcs, face_idx, status);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_mdata_pose(const double* points, const int64_t* piece_off, const int64_t* store_data_id, const int64_t* sel, int64_t B,
                               int64_t S, int64_t num_points, int64_t max_parts, const int32_t* order, const double* rot, uint64_t seed,
                               uint32_t split, float* part_pcs, float* part_quat, float* part_trans, double* rot_out, pfpp_stream_t stream) {
  PFPP_REQUIRE(points && piece_off && store_data_id && sel && part_pcs && part_trans, "null pointer");
  PFPP_REQUIRE(rot || part_quat, "null pointer: part_quat is needed when the rotations are generated");
  PFPP_REQUIRE(sizes_ok(B, S, num_points, max_parts), "bad sizes");
  PFPP_SUPPORTED(max_parts <= MD_MAX_PARTS, "max_num_part > 32");
  PFPP_SUPPORTED(num_points <= 0x7fffffff && B * max_parts <= 0x7fffffff, "more than 2^31 - 1 points per puzzle or piece slots");
  if (B == 0) return PFPP_OK;
  hipLaunchKernelGGL(pose_kernel, dim3((unsigned)(B * max_parts)), dim3(MD_BLOCK), 0, pfpp::as_stream(stream), points, piece_off, store_data_id,
                     sel, S, B * num_points, (int)max_parts, order, rot, seed, split, part_pcs, part_quat, part_trans, rot_out);
  return pfpp::check_launch(__func__);
}
