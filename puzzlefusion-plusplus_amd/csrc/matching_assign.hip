// The matcher's optimal assignment on the device (pfpp_match_assign, include/pfpp.h "matcher, assignment"): an exact solver of the
// square linear assignment problem, maximise sum_i c[i, col_i], for the masked Sinkhorn outputs of a batch of puzzles in one launch.
// It replaces scipy.optimize.linear_sum_assignment behind Jigsaw_matching/utils/linear_solvers.py:279-340 with the same arithmetic:
// duals and path lengths in fp64 on cost = -(double)c, additions, subtractions and comparisons only, so nothing can be contracted
// and the result is defined bit for bit (pfpp_hip/matching_assign.py: assign_reference restates it in numpy).
//
// Two kernels per launch of at most PFPP_MATCH_ASSIGN_MAX_PUZZLES puzzles, whose descriptors travel in the kernel-argument struct:
//
// * assign_init_kernel, a wave per row over the whole chip: u_i = min_j cost_ij, j*(i) = the lowest column attaining it, and column j
//   goes to the lowest row i with j*(i) = j (integer atomicMin on a row-for-column array; no float atomics).  v = 0.
// * assign_solve_kernel<T, K>, one workgroup of T threads per puzzle: the rows the initialisation left free, in ascending order, each
//   by one shortest augmenting path.  Thread t owns the columns t, t + T, ..: their dist and v live in its registers (K of each),
//   u, row4col, col4row and path in LDS (14 bytes per column: 112 KiB at n = 8,192).  A search step reads one matrix row (one
//   coalesced dword per column), relaxes the unscanned columns, and picks the unscanned column with the smallest (dist, assigned,
//   index): lexicographic, a total order, folded by shuffles within a wave and through one LDS slot per wave across them (two slot
//   sets taken in turn, so a step has one barrier).  The result therefore does not depend on T, K or wave arrival.
//
// Every loop is bounded by n or by the puzzle's step budget; there is no spin-wait and no communication between workgroups.
#include "pfpp_common.h"

namespace {

constexpr int AS_MAX_N = PFPP_MATCH_ASSIGN_MAX_N;
constexpr int AS_PUZZLES = PFPP_MATCH_ASSIGN_MAX_PUZZLES;
constexpr int AS_NO_ROW = 0x7f7f7f7f;      // row4col before the initialisation: the byte pattern hipMemsetAsync writes, above every row

struct AssignPuzzle {
  const float* c;      // [n, n] contiguous
  int64_t off;         // of the puzzle's n entries in col, u, v and row4col
  int64_t budget;      // search steps over all searches of the puzzle
  int32_t n;
  int32_t index;       // of the puzzle in status, steps and augmentations
};
struct AssignArgs {
  AssignPuzzle puz[AS_PUZZLES];
  int64_t* col;
  double* u;
  double* v;
  int32_t* status;
  int64_t* steps;
  int64_t* augmentations;
  int32_t* row4col;    // workspace
};
static_assert(sizeof(AssignArgs) <= 4096, "the kernel-argument segment of pfpp_match_assign is kept within 4 KB");
static_assert(AS_MAX_N <= 32767, "row and column indices are kept as int16 in LDS");

// (d, k) < (bd, bk) in the order of the column choice: smaller dist, then the smaller key (assigned flag in bit 31, index below)
__device__ __forceinline__ void take_smaller(double& bd, uint32_t& bk, double d, uint32_t k) {
  if (d < bd || (d == bd && k < bk)) { bd = d; bk = k; }
}

__global__ __launch_bounds__(256) void assign_init_kernel(const AssignArgs a) {
  const AssignPuzzle& p = a.puz[blockIdx.y];
  const int n = p.n;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;                                    // whole wave
  const float* __restrict__ row = p.c + (int64_t)i * n;
  double best = __builtin_huge_val();
  uint32_t bj = 0xffffffffu;
#pragma unroll 4
  for (int j = lane; j < n; j += 64) {                   // ascending j per lane: the strict test keeps the lowest index
    const double cst = -(double)row[j];
    if (cst < best) { best = cst; bj = (uint32_t)j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const uint32_t oj = __shfl_xor(bj, o, 64);
    take_smaller(best, bj, ob, oj);
  }
  if (lane == 0) {
    a.u[p.off + i] = best;
    if (bj < (uint32_t)n) atomicMin(&a.row4col[p.off + bj], i);
  }
}

struct AssignSlot { double d; uint32_t key; uint32_t pad; };

template <int T, int K>
__global__ __launch_bounds__(T) void assign_solve_kernel(const AssignArgs a) {
  constexpr int W = T / 64, CAP = T * K;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* su = reinterpret_cast<double*>(smem);                          // u [CAP]
  AssignSlot* slots = reinterpret_cast<AssignSlot*>(su + CAP);           // [2][W]
  int16_t* r4c = reinterpret_cast<int16_t*>(slots + 2 * W);              // row of a column, -1 = unassigned [CAP]
  int16_t* c4r = r4c + CAP;                                              // column of a row [CAP]
  int16_t* path = c4r + CAP;                                             // the row a column's dist came from [CAP]
  const AssignPuzzle p = a.puz[blockIdx.x];
  const int n = p.n, t = threadIdx.x;
  if (n > CAP) return;                                                   // the launcher sizes T K from the largest n; never taken
  const float* __restrict__ c = p.c;

  for (int j = t; j < n; j += T) {
    const int r = a.row4col[p.off + j];
    r4c[j] = (int16_t)(r < n ? r : -1);
    c4r[j] = -1;
    su[j] = a.u[p.off + j];
  }
  __syncthreads();
  for (int j = t; j < n; j += T) {
    const int r = r4c[j];
    if (r >= 0) c4r[r] = (int16_t)j;
  }
  __syncthreads();

  double v[K], dist[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0.0;
  int64_t steps = 0, augs = 0;
  int status = 0;

  for (int cur = 0; cur < n && status == 0; ++cur) {
    if (c4r[cur] >= 0) continue;                                         // uniform
    uint32_t scanned = 0, assigned = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      dist[k] = __builtin_huge_val();
      const int j = t + k * T;
      if (j < n && r4c[j] >= 0) assigned |= 1u << k;
    }
    int i = cur, sink = -1;
    double minv = 0.0;
    for (int s = 0; s < n; ++s) {                                        // a step scans one more column: at most n of them
      if (steps == p.budget) { status = 1; break; }
      ++steps;
      const float* __restrict__ row = c + (int64_t)i * n;
      float cv[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = t + k * T;
        cv[k] = j < n ? row[j] : 0.0f;
      }
      const double ui = su[i];
      double bd = __builtin_huge_val();
      uint32_t bk = 0xffffffffu;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = t + k * T;
        if (j < n && !((scanned >> k) & 1u)) {
          const double r = ((minv + (-(double)cv[k])) - ui) - v[k];
          if (r < dist[k]) { dist[k] = r; path[j] = (int16_t)i; }
          take_smaller(bd, bk, dist[k], (((assigned >> k) & 1u) << 31) | (uint32_t)j);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const uint32_t ok = __shfl_xor(bk, o, 64);
        take_smaller(bd, bk, od, ok);
      }
      if constexpr (W > 1) {
        AssignSlot* sl = slots + (int)(steps & 1) * W;                   // the other set than the step before: one barrier per step
        if ((t & 63) == 0) { sl[t >> 6].d = bd; sl[t >> 6].key = bk; }
        __syncthreads();
        bd = sl[0].d; bk = sl[0].key;
#pragma unroll
        for (int q = 1; q < W; ++q) take_smaller(bd, bk, sl[q].d, sl[q].key);
      }
      // no unscanned column (cannot happen while s < n), or none within reach: a matrix with NaN or infinite entries.  Refused here,
      // so that path[] is written for every column that is ever scanned
      if (bk == 0xffffffffu || !(bd < __builtin_huge_val())) { status = 2; break; }
      const int j = (int)(bk & 0x7fffffffu);
      minv = bd;
      if ((j & (T - 1)) == t) scanned |= 1u << (j / T);
      if (!(bk >> 31)) { sink = j; break; }
      i = __builtin_amdgcn_readfirstlane((int)r4c[j]);
    }
    if (status != 0) break;
    if (sink < 0) { status = 2; break; }                                 // n steps without a free column: cannot happen
    // the duals, with the assignment as it stands before augmenting; every row below is owned by one column, cur by none
    if (t == 0) su[cur] = su[cur] + minv;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if ((scanned >> k) & 1u) {
        const int j = t + k * T;
        const double delta = minv - dist[k];
        if (j != sink) {
          const int r = r4c[j];
          su[r] = su[r] + delta;
        }
        v[k] = v[k] - delta;
      }
    }
    __syncthreads();
    if (t == 0) {
      int j = sink;
      for (int g = 0; g < n; ++g) {                                      // a path visits a column once
        const int r = path[j];
        r4c[j] = (int16_t)r;
        const int jn = c4r[r];
        c4r[r] = (int16_t)j;
        j = jn;
        if (r == cur) break;
      }
    }
    __syncthreads();
    ++augs;
  }

  for (int j = t; j < n; j += T) {
    a.col[p.off + j] = c4r[j];
    a.u[p.off + j] = su[j];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int j = t + k * T;
    if (j < n) a.v[p.off + j] = v[k];
  }
  if (t == 0) {
    a.status[p.index] = status;
    a.steps[p.index] = steps;
    a.augmentations[p.index] = augs;
  }
}

template <int T, int K>
void launch_solve(const AssignArgs& a, int count, hipStream_t st) {
  constexpr size_t smem = (size_t)T * K * 14 + 2 * (T / 64) * sizeof(AssignSlot);
  (void)pfpp_allow_dyn_lds<assign_solve_kernel<T, K>>();
  hipLaunchKernelGGL((assign_solve_kernel<T, K>), dim3((unsigned)count), dim3(T), smem, st, a);
}

}  // namespace

extern "C" int64_t pfpp_match_assign_workspace(int64_t B, const int64_t* n) {
  if (B < 1 || !n) return -1;
  int64_t total = 0;
  for (int64_t b = 0; b < B; ++b) {
    if (n[b] < 1 || n[b] > AS_MAX_N) return -1;
    total += n[b];
  }
  return total * (int64_t)sizeof(int32_t);
}

extern "C" int pfpp_match_assign(int64_t B, const float* const* c, const int64_t* n, const int64_t* max_steps, int64_t* col, double* u,
                                 double* v, int32_t* status, int64_t* steps, int64_t* augmentations, void* workspace,
                                 int64_t workspace_bytes, pfpp_stream_t stream) {
  PFPP_REQUIRE(B >= 1, "B < 1");
  PFPP_REQUIRE(c && n && max_steps && col && u && v && status && steps && augmentations && workspace, "null pointer");
  for (int64_t b = 0; b < B; ++b) {                     // every refusal comes before the first launch
    PFPP_REQUIRE(c[b], "null matrix in the list");
    PFPP_REQUIRE(n[b] >= 1, "n < 1");
    PFPP_SUPPORTED(n[b] <= AS_MAX_N, "more than 8192 rows in one puzzle");
    PFPP_REQUIRE(max_steps[b] >= 1, "step budget < 1");
  }
  PFPP_REQUIRE(workspace_bytes >= pfpp_match_assign_workspace(B, n), "workspace smaller than pfpp_match_assign_workspace(B, n)");
  PFPP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "workspace must be 4-byte aligned");
  hipStream_t st = pfpp::as_stream(stream);
  if (hipMemsetAsync(workspace, 0x7f, (size_t)pfpp_match_assign_workspace(B, n), st) != hipSuccess) {
    pfpp::set_error("%s: hipMemsetAsync failed", __func__);
    return PFPP_EHIP;
  }
  AssignArgs a;
  a.col = col; a.u = u; a.v = v; a.status = status; a.steps = steps; a.augmentations = augmentations;
  a.row4col = static_cast<int32_t*>(workspace);
  int64_t off = 0;
  // the chunking pfpp_hip.matching_assign.plan_assign restates: puzzles in order, AS_PUZZLES to a launch, the workgroup shaped by
  // the largest n of the launch
  for (int64_t b0 = 0; b0 < B; b0 += AS_PUZZLES) {
    const int count = (int)(B - b0 < AS_PUZZLES ? B - b0 : AS_PUZZLES);
    int n_max = 0;
    for (int k = 0; k < count; ++k) {
      AssignPuzzle& p = a.puz[k];
      p.c = c[b0 + k]; p.off = off; p.budget = max_steps[b0 + k]; p.n = (int32_t)n[b0 + k]; p.index = (int32_t)(b0 + k);
      off += n[b0 + k];
      n_max = p.n > n_max ? p.n : n_max;
    }
    hipLaunchKernelGGL(assign_init_kernel, dim3((unsigned)((n_max + 3) / 4), (unsigned)count), dim3(256), 0, st, a);
    if (n_max <= 64) launch_solve<64, 1>(a, count, st);
    else if (n_max <= 128) launch_solve<128, 1>(a, count, st);
    else if (n_max <= 256) launch_solve<256, 1>(a, count, st);
    else if (n_max <= 512) launch_solve<512, 1>(a, count, st);
    else if (n_max <= 1024) launch_solve<1024, 1>(a, count, st);
    else if (n_max <= 2048) launch_solve<1024, 2>(a, count, st);
    else if (n_max <= 3072) launch_solve<1024, 3>(a, count, st);
    else if (n_max <= 4096) launch_solve<1024, 4>(a, count, st);
    else if (n_max <= 6144) launch_solve<1024, 6>(a, count, st);
    else launch_solve<1024, 8>(a, count, st);
  }
  return pfpp::check_launch(__func__);
}
