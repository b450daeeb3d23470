// The matcher's pair rule on the device (pfpp_match_edges, include/pfpp.h "matcher, edges and correspondences"): the assignment of
// a batch of puzzles -> `edges` and per-edge correspondence lists, Jigsaw_matching/model/modules/matching_base_model.py:298-359, and
// the flattening of those lists that puzzlefusion_plusplus/auto_aggl.py:92-126 (get_distance_for_matching_pts,
// utils/node_merge_utils.py:62-89) does for the verifier's edge features.  pfpp_hip/matching_edges.py: pack_matches_reference restates
// the outputs in numpy from pfpp_hip.matching.match_edges and AutoAgglomerative.prepare_matching.
//
// One launch, one workgroup of 512 threads per puzzle; all arithmetic is integer:
//
//  1. the sizes of the puzzle are checked against each other and against the totals the caller states (status 2 otherwise), so that
//     nothing below reads or writes outside the puzzle's own slots.
//  2. one pass over col: range check (status 2), the P x P block counts by LDS integer atomics (order-free), and the inverse
//     permutation into the global workspace.  A second pass reads it back: inv[col[r]] == r for every matched row holds exactly when
//     col is injective on its matched rows (status 1 otherwise), whichever of two rows that claim one column wrote last.
//  3. a thread per triangle slot (idx1 < idx2, row-major) applies the rule: the block (idx1, idx2), or its transposed opposite when
//     that is strictly larger; dropped with fewer than 3 matches, a piece without critical points or a piece behind n_valid.  One wave
//     turns the sizes into offsets (8 slots per lane, a shuffle scan over the lanes).
//  4. a wave per kept slot writes its rows in sorted order without a sort: the rows of piece idx1 ascending (their columns are
//     distinct), or for a transposed block the columns of piece idx1 ascending through the inverse permutation; 64 candidates at a
//     time, compacted in order by ballot + mbcnt (the scheme of match_classify_compact_kernel, csrc/matching.hip).
//
// Every loop is bounded by P, by the slot count or by the puzzle's rows; workgroups do not communicate.
#include "pfpp_common.h"

namespace {

constexpr int ME_MAX_P = PFPP_MATCH_EDGES_MAX_P;
constexpr int ME_MAX_SLOTS = ME_MAX_P * (ME_MAX_P - 1) / 2;      // 496
constexpr int ME_T = 512;
constexpr int ME_WAVES = ME_T / 64;
static_assert(ME_MAX_SLOTS <= 64 * 8, "the offsets are scanned by one wave with 8 slots per lane");
static_assert(ME_MAX_SLOTS <= ME_T, "a thread per triangle slot");

struct EdgesArgs {
  const int64_t* col;            // [total_rows]
  const int64_t* row_off;        // [B + 1]
  const int64_t* n_crit;         // [B, P]
  const int64_t* n_valid;        // [B]
  const int64_t* piece_off;      // [B P + 1]
  const int64_t* crit_idx;       // [total_points]
  int64_t total_rows, total_points;
  int32_t P, max_rows;
  int32_t* counts;               // [B, P, P]
  int32_t* edge_off;             // [B, T + 1]
  int32_t* kept;                 // [B, T]
  int32_t* corr;                 // [total_rows, 2]
  int32_t* idx_a;                // [total_rows]
  int32_t* idx_b;                // [total_rows]
  int32_t* status;               // [B]
  int32_t* inv;                  // workspace [total_rows]
};

// the piece of row r < pstart[P]: the highest p with pstart[p] <= r (an empty piece shares its start with the next one and is skipped)
__device__ __forceinline__ int piece_of(const int* pstart, int P, int r) {
  int lo = 0, hi = P;
#pragma unroll
  for (int s = 0; s < 5; ++s) {                         // 2^5 >= ME_MAX_P
    if (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pstart[mid] <= r) lo = mid; else hi = mid;
    }
  }
  return lo;
}

__global__ __launch_bounds__(ME_T) void match_edges_kernel(const EdgesArgs a) {
  __shared__ int s_pstart[ME_MAX_P + 1];                 // first row of a piece among the puzzle's rows
  __shared__ int s_lstart[ME_MAX_P];                     // first point of a piece among the puzzle's points
  __shared__ int64_t s_pabs[ME_MAX_P + 1];               // piece_off of the puzzle's pieces
  __shared__ int64_t s_nc[ME_MAX_P];
  __shared__ int s_cnt[ME_MAX_P * ME_MAX_P];
  __shared__ int s_m[64 * 8];                            // correspondences of a slot (0 = dropped), zero behind the last slot
  __shared__ int s_off[ME_MAX_SLOTS + 1];
  __shared__ int s_pair[ME_MAX_SLOTS];                   // idx1 | idx2 << 8 | transposed << 16
  __shared__ int s_flag, s_n;
  const int P = a.P, T = P * (P - 1) / 2, t = threadIdx.x, lane = t & 63;
  const int64_t b = blockIdx.x;

  if (t <= P) s_pabs[t] = a.piece_off[b * P + t];
  if (t < P) s_nc[t] = a.n_crit[b * P + t];
  for (int k = t; k < P * P; k += ME_T) s_cnt[k] = 0;
  s_m[t] = 0;
  __syncthreads();
  if (t == 0) {                                          // 1. the sizes, against each other and against the caller's totals
    const int64_t r0 = a.row_off[b], r1 = a.row_off[b + 1], nv = a.n_valid[b];
    bool ok = r0 >= 0 && r1 >= r0 && r1 <= a.total_rows && r1 - r0 <= a.max_rows && nv >= 0 && nv <= P;
    int64_t rows = 0;
    for (int p = 0; p < P; ++p) {
      const int64_t st = s_pabs[p], en = s_pabs[p + 1], nc = s_nc[p];
      ok = ok && st >= 0 && en >= st && en <= a.total_points && en - s_pabs[0] <= 0x7fffffff && nc >= 0 && nc <= en - st;
      s_pstart[p] = (int)rows;
      s_lstart[p] = (int)(st - s_pabs[0]);
      if (ok) rows += nc;                                // nc <= en - st < 2^31 while ok: no overflow
    }
    s_pstart[P] = (int)rows;
    ok = ok && r1 - r0 <= rows;                          // an assignment larger than the critical points (match_edges raises there)
    s_flag = ok ? 0 : 2;
    s_n = ok ? (int)(r1 - r0) : 0;
  }
  __syncthreads();
  const int n = s_n;
  const int64_t r0 = n ? a.row_off[b] : 0;
  const int64_t* __restrict__ col = a.col + r0;
  int32_t* inv = a.inv + r0;

  // 2. range, block counts and the inverse permutation
  for (int j = t; j < n; j += ME_T) inv[j] = -1;
  __syncthreads();
  for (int r = t; r < n; r += ME_T) {
    const int64_t c = col[r];
    if (c < -1 || c >= n) {
      atomicOr(&s_flag, 2);
    } else if (c >= 0) {
      atomicAdd(&s_cnt[piece_of(s_pstart, P, r) * P + piece_of(s_pstart, P, (int)c)], 1);
      __hip_atomic_store(&inv[c], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // two rows of one column: either may stay
    }
  }
  __syncthreads();
  for (int r = t; r < n; r += ME_T) {
    const int64_t c = col[r];
    if (c >= 0 && c < n && __hip_atomic_load(&inv[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != r) atomicOr(&s_flag, 1);
  }
  __syncthreads();
  const int status = (s_flag & 2) ? 2 : (s_flag & 1);

  // 3. the rule per triangle slot, then the offsets
  if (t < T) {
    int i1 = 0, rem = t;
    for (; i1 < P - 1; ++i1) {
      const int len = P - 1 - i1;
      if (rem < len) break;
      rem -= len;
    }
    const int i2 = i1 + 1 + rem;
    const int c12 = s_cnt[i1 * P + i2], c21 = s_cnt[i2 * P + i1];
    const int tr = c12 < c21;                            // ties keep the first
    const int m = tr ? c21 : c12;
    const bool keep = status == 0 && i2 < (int)a.n_valid[b] && s_nc[i1] > 0 && s_nc[i2] > 0 && m >= 3;
    s_m[t] = keep ? m : 0;
    s_pair[t] = i1 | (i2 << 8) | (tr << 16);
  }
  __syncthreads();
  if (t < 64) {
    int v[8], sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = s_m[8 * t + k]; sum += v[k]; }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    int run = incl - sum;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (8 * t + k <= T) s_off[8 * t + k] = run;        // slot T: the puzzle's total (s_m is zero from there on)
      run += v[k];
    }
  }
  __syncthreads();
  for (int k = t; k < P * P; k += ME_T) a.counts[b * P * P + k] = status == 0 ? s_cnt[k] : 0;
  for (int k = t; k <= T; k += ME_T) a.edge_off[b * (T + 1) + k] = s_off[k];
  for (int k = t; k < T; k += ME_T) a.kept[b * T + k] = s_m[k] > 0;
  if (t == 0) a.status[b] = status;

  // 4. a wave per kept slot (s_m is zero everywhere when status != 0).  The kept blocks are disjoint sets of rows: s_off[T] <= n
  for (int slot = t >> 6; slot < T; slot += ME_WAVES) {
    const int m = s_m[slot];
    if (m == 0) continue;                                // whole wave
    const int pr = s_pair[slot], i1 = pr & 0xff, i2 = (pr >> 8) & 0xff;
    const bool tr = (pr >> 16) != 0;
    const int a0 = s_pstart[i1], b0 = s_pstart[i2], b1 = s_pstart[i2 + 1];
    const int a1 = s_pstart[i1 + 1] < n ? s_pstart[i1 + 1] : n;      // an assignment of fewer rows than critical points ends early
    const int64_t base = r0 + s_off[slot];
    const int64_t* __restrict__ crit1 = a.crit_idx + s_pabs[i1];
    const int64_t* __restrict__ crit2 = a.crit_idx + s_pabs[i2];
    const int l1 = s_lstart[i1], l2 = s_lstart[i2];
    int cnt = 0;
    for (int jb = a0; jb < a1; jb += 64) {               // rows of idx1 (or, transposed, its columns) in ascending order
      const int j = jb + lane;
      int64_t other = -1;
      if (j < a1) other = tr ? (int64_t)inv[j] : col[j];
      const bool keep = other >= b0 && other < b1;
      const unsigned long long mask = __ballot(keep);
      const int pos = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
      if (keep && pos < m) {                             // pos < m always: m counted exactly these entries
        const int o1 = j - a0, o2 = (int)other - b0;     // o1 < n_crit[idx1] <= the piece's points, likewise o2: inside crit_idx
        reinterpret_cast<int2*>(a.corr)[base + pos] = make_int2(o1, o2);
        a.idx_a[base + pos] = l1 + (int32_t)crit1[o1];
        a.idx_b[base + pos] = l2 + (int32_t)crit2[o2];
      }
      cnt += __builtin_popcountll(mask);
    }
  }
}

}  // namespace

extern "C" int64_t pfpp_match_edges_workspace(int64_t total_rows) {
  return total_rows < 0 ? -1 : total_rows * (int64_t)sizeof(int32_t);
}

extern "C" int pfpp_match_edges(const int64_t* col, const int64_t* row_off, const int64_t* n_critical_pcs, const int64_t* n_valid,
                                const int64_t* piece_off, const int64_t* critical_pcs_idx, int64_t B, int64_t P, int64_t max_rows,
                                int64_t total_rows, int64_t total_points, int32_t* counts, int32_t* edge_off, int32_t* kept,
                                int32_t* corr, int32_t* idx_a, int32_t* idx_b, int32_t* status, void* workspace,
                                int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(B >= 0 && max_rows >= 0 && total_rows >= 0 && total_points >= 0 && max_rows <= total_rows, "negative size, or max_rows > total_rows");
  PFPP_SUPPORTED(P >= 1 && P <= PFPP_MATCH_EDGES_MAX_P, "P outside 1..32");
  PFPP_SUPPORTED(max_rows <= PFPP_MATCH_EDGES_MAX_ROWS, "more than 65535 rows in one puzzle");
  PFPP_SUPPORTED(B <= PFPP_MATCH_EDGES_MAX_PUZZLES, "more than 65535 puzzles in one launch");
  if (B == 0) return PFPP_OK;
  PFPP_REQUIRE(row_off && n_critical_pcs && n_valid && piece_off && counts && edge_off && status, "null pointer");
  PFPP_REQUIRE(total_rows == 0 || (col && corr && idx_a && idx_b && workspace), "null pointer");
  PFPP_REQUIRE(total_points == 0 || critical_pcs_idx, "null pointer");
  PFPP_REQUIRE(P == 1 || kept, "null pointer");
  PFPP_REQUIRE(workspace_bytes >= pfpp_match_edges_workspace(total_rows), "workspace smaller than pfpp_match_edges_workspace(total_rows)");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0 && (reinterpret_cast<uintptr_t>(corr) & 7u) == 0,
               "workspace must be 4-byte aligned, corr 8-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  EdgesArgs a;
  a.col = col; a.row_off = row_off; a.n_crit = n_critical_pcs; a.n_valid = n_valid; a.piece_off = piece_off; a.crit_idx = critical_pcs_idx;
  a.total_rows = total_rows; a.total_points = total_points; a.P = (int32_t)P; a.max_rows = (int32_t)max_rows;
  a.counts = counts; a.edge_off = edge_off; a.kept = kept; a.corr = corr; a.idx_a = idx_a; a.idx_b = idx_b; a.status = status;
  a.inv = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(match_edges_kernel, dim3((unsigned)B), dim3(ME_T), 0, st, a);
  return pfpp::check_launch(__func__);
}
