// pc_data generation (generate_pc_data.py via vqvae/dataset/dataset.py:GeometryPartDataset): the per-fragment work of
// _get_pcs (dataset.py:154-181) on a CSR batch of fragments.
//
//  * pfpp_mesh_face_cdf — trimesh.sample.sample_surface's face weights: area |(b-a) x (c-a)| / 2 per face in fp64, written out
//    component by component (the unit is compiled with -ffp-contract=off), and the inclusive prefix sum per part.  One
//    workgroup per part walks its faces in chunks of 256: a wave scan (shuffles), the wave totals through LDS, and a carry that is
//    the chunk's last cdf value, so cdf[F - 1] == total exactly and the sum order is fixed (no atomics).
//  * pfpp_mesh_sample_surface — one thread per (part, sample): face = lower bound of u0 * total in the part's cdf (searched in L2:
//    13 dependent loads at 8k faces, against F / 256 loads per thread to stage the whole cdf in LDS for each block of samples),
//    the fold of (l0, l1) into the triangle and p = ((b - a) l0 + (c - a) l1) + a in the reference's order.  The uniforms are
//    given (u [Pt, N, 3]) or drawn from pfpp_rng_u64 keyed by (seed, split, ((data_id max_parts + slot) N + i) 3 + k), so a
//    puzzle's points never depend on the batch it ran in.  An epilogue kernel (one workgroup per puzzle) takes every part's
//    scale = max - min over its coordinates and the puzzle's reference slot (first max, dataset.py:200-205).
//  * pfpp_mesh_vertex_graph — _check_connectivity (dataset.py:85-127): parts i != j are connected iff a vertex of i equals a vertex
//    of j after np.round(., 5).  Keys llrint(x 1e5) fall into the same equality classes; per puzzle the per-axis minimum key is
//    subtracted and three 21-bit fields are packed into one uint64.  Each puzzle owns an open-addressing table (power-of-two
//    capacity >= 2 x its vertex count): a 64-bit CAS claims a slot, an atomicOr sets the part's bit in the slot's mask; the probe
//    is bounded by the capacity.  A pass over the slots ORs every mask with two or more bits into the puzzle's row masks.
//
// Data-dependent failures (a non-finite vertex, a face index outside its part, a zero or non-finite area sum, a key range the
// packing cannot hold, a full table) are recorded in a device status word by atomicMin of (kind << 32 | index), so the smallest
// kind and index win whatever the schedule; pfpp_mesh_status reads it back.  Integer atomics only: two runs are bitwise equal.
#include <limits.h>
#include <math.h>

#include "mesh_common.h"
#include "pfpp_common.h"

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_MAX_PARTS = 32;
constexpr int KEY_BITS = 21;
constexpr int64_t KEY_RANGE = (int64_t)1 << KEY_BITS;
constexpr uint64_t EMPTY_KEY = ~0ull;
// |x| 1e5 must stay well inside int64 before llrint (the packing refuses far smaller ranges anyway)
constexpr double KEY_MAG_LIMIT = 4503599627370496.0;     // 2^52

using namespace pfpp_mesh;      // the status word and sample_point (mesh_common.h)

// largest p in [0, n) with off[p] <= v (off non-decreasing, off[0] <= v): the CSR row that holds element v
__device__ __forceinline__ int64_t csr_row(const int64_t* __restrict__ off, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;          // invariant: off[lo] <= v, answer < hi
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double tri_area(const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ c) {
  const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
  const double v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];
  const double c0 = u1 * v2 - u2 * v1;
  const double c1 = u2 * v0 - u0 * v2;
  const double c2 = u0 * v1 - u1 * v0;
  return sqrt((c0 * c0 + c1 * c1) + c2 * c2) / 2.0;
}

// ------------------------------------------------------------------------------------------------ face areas + per-part cdf
__global__ __launch_bounds__(MS_BLOCK) void face_cdf_kernel(const double* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const int64_t* __restrict__ vert_off, const int64_t* __restrict__ face_off,
                                                            double* __restrict__ area, double* __restrict__ cdf,
                                                            double* __restrict__ total, uint64_t* status) {
  __shared__ double wave_tot[MS_BLOCK / PFPP_WAVE];
  __shared__ double carry_s;
  const int part = blockIdx.x;
  const int lane = threadIdx.x & (PFPP_WAVE - 1), wave = threadIdx.x / PFPP_WAVE;
  const int64_t vo = vert_off[part], nv = vert_off[part + 1] - vo;
  const int64_t fo = face_off[part], nf = face_off[part + 1] - fo;
  const double* pv = verts + vo * 3;
  double carry = 0.0;
  bool bad_face = false;
  for (int64_t c0 = 0; c0 < nf; c0 += MS_BLOCK) {
    const int64_t f = c0 + threadIdx.x;
    double x = 0.0;
    if (f < nf) {
      const int32_t* fc = faces + (fo + f) * 3;
      const int32_t ia = fc[0], ib = fc[1], ic = fc[2];
      if (ia < 0 || ib < 0 || ic < 0 || ia >= nv || ib >= nv || ic >= nv) {
        bad_face = true;
        x = __builtin_nan("");
      } else {
        x = tri_area(pv + (int64_t)ia * 3, pv + (int64_t)ib * 3, pv + (int64_t)ic * 3);
      }
      if (area) area[fo + f] = x;
    }
    // inclusive wave scan
    for (int d = 1; d < PFPP_WAVE; d <<= 1) {
      const double y = __shfl_up(x, d, PFPP_WAVE);
      if (lane >= d) x = x + y;
    }
    if (lane == PFPP_WAVE - 1) wave_tot[wave] = x;
    __syncthreads();
    double pre = carry;
    for (int w = 0; w < wave; ++w) pre = pre + wave_tot[w];
    const double val = pre + x;
    if (f < nf) cdf[fo + f] = val;
    if (threadIdx.x == MS_BLOCK - 1) carry_s = val;      // inactive lanes add zeros: this is the chunk's last cdf value
    __syncthreads();
    carry = carry_s;
  }
  if (bad_face) report(status, ST_FACE_INDEX, part);
  if (threadIdx.x == 0) {
    total[part] = carry;
    if (!(carry > 0.0) || !isfinite(carry)) report(status, ST_AREA, part);
  }
}

// ------------------------------------------------------------------------------------------------ surface samples
__global__ __launch_bounds__(MS_BLOCK) void sample_surface_kernel(
    const double* __restrict__ verts, const int32_t* __restrict__ faces, const int64_t* __restrict__ vert_off,
    const int64_t* __restrict__ face_off, const double* __restrict__ cdf, const double* __restrict__ total,
    const int32_t* __restrict__ part_puzzle, const int32_t* __restrict__ part_slot, const int64_t* __restrict__ data_id, int N,
    const double* __restrict__ u, uint64_t seed, uint32_t split, int64_t max_parts, double* __restrict__ points,
    int32_t* __restrict__ face_idx) {
  const int part = blockIdx.y;
  const int i = blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)part * N + i;
  double u0, l0, l1;
  if (u) {
    u0 = u[row * 3 + 0]; l0 = u[row * 3 + 1]; l1 = u[row * 3 + 2];
  } else {
    const uint64_t base = (((uint64_t)data_id[part_puzzle[part]] * (uint64_t)max_parts + (uint64_t)part_slot[part]) * (uint64_t)N +
                           (uint64_t)i) * 3ull;
    u0 = uniform53(seed, split, base + 0);
    l0 = uniform53(seed, split, base + 1);
    l1 = uniform53(seed, split, base + 2);
  }
  const int64_t fo = face_off[part], nf = face_off[part + 1] - fo;
  const int64_t vo = vert_off[part], nv = vert_off[part + 1] - vo;
  double* out = points + row * 3;
  if (nf <= 0) {
    out[0] = out[1] = out[2] = __builtin_nan("");
    if (face_idx) face_idx[row] = -1;
    return;
  }
  const int64_t f = sample_point(verts + vo * 3, faces + fo * 3, nv, nf, cdf + fo, total[part], u0, l0, l1, out);
  if (face_idx) face_idx[row] = (int32_t)f;
}

// one workgroup per puzzle: scale of each of its parts (max - min over all N x 3 coordinates) and the first part of largest scale
__global__ __launch_bounds__(MS_BLOCK) void scale_ref_kernel(const double* __restrict__ points, const int64_t* __restrict__ puz_part_off,
                                                             const int32_t* __restrict__ part_slot, int N, double* __restrict__ scale,
                                                             int32_t* __restrict__ ref_slot) {
  __shared__ double red_max[MS_BLOCK], red_min[MS_BLOCK];
  const int b = blockIdx.x;
  const int64_t p0 = puz_part_off[b], p1 = puz_part_off[b + 1];
  double best = 0.0;
  int32_t best_slot = 0;
  for (int64_t p = p0; p < p1; ++p) {
    const double* src = points + p * (int64_t)N * 3;
    double mx = -__builtin_inf(), mn = __builtin_inf();
    for (int64_t e = threadIdx.x; e < (int64_t)N * 3; e += MS_BLOCK) {
      const double v = src[e];
      mx = fmax(mx, v);
      mn = fmin(mn, v);
    }
    red_max[threadIdx.x] = mx;
    red_min[threadIdx.x] = mn;
    __syncthreads();
    for (int s = MS_BLOCK / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s) {
        red_max[threadIdx.x] = fmax(red_max[threadIdx.x], red_max[threadIdx.x + s]);
        red_min[threadIdx.x] = fmin(red_min[threadIdx.x], red_min[threadIdx.x + s]);
      }
      __syncthreads();
    }
    const double sc = red_max[0] - red_min[0];
    if (threadIdx.x == 0) {
      if (scale) scale[p] = sc;
      if (p == p0 || sc > best) { best = sc; best_slot = part_slot[p]; }       // np.argmax: the first maximum
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && ref_slot) ref_slot[b] = best_slot;
}

// ------------------------------------------------------------------------------------------------ vertex contact graph
struct GraphWs {
  unsigned long long* keys;   // [slots], EMPTY_KEY = free
  uint32_t* masks;            // [slots], bit s = part slot s has a vertex with this key
  uint32_t* rows;             // [B, 32], bit j of row i = parts i and j share a key
  int64_t* kmin;              // [B, 3], per-axis minimum key
  int32_t* bad;               // [B], 1 = the puzzle's keys cannot be packed (reported in the status word)
};

__device__ __forceinline__ bool vertex_key(double x, int64_t* k) {
  const double y = x * 1e5;
  if (!(fabs(y) < KEY_MAG_LIMIT)) return false;
  *k = llrint(y);
  return true;
}

// one workgroup per puzzle: per-axis key range; refuses non-finite vertices and ranges the 21-bit fields cannot hold
__global__ __launch_bounds__(MS_BLOCK) void graph_range_kernel(const double* __restrict__ verts, const int64_t* __restrict__ vert_off,
                                                               const int64_t* __restrict__ puz_part_off, GraphWs ws, uint64_t* status) {
  __shared__ long long red[6][MS_BLOCK];
  __shared__ int flag_s;
  const int b = blockIdx.x;
  const int64_t pa = puz_part_off[b], pb = puz_part_off[b + 1];
  const int64_t v0 = vert_off[pa], v1 = vert_off[pb];
  if (threadIdx.x == 0) flag_s = 0;
  __syncthreads();
  long long mn[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, mx[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
  for (int64_t v = v0 + threadIdx.x; v < v1; v += MS_BLOCK) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = verts[v * 3 + k];
      int64_t key;
      if (!isfinite(x)) {
        report(status, ST_NONFINITE, pa + csr_row(vert_off + pa, pb - pa, v));
        flag_s = 1;
      } else if (!vertex_key(x, &key)) {
        report(status, ST_KEY_MAG, b);
        flag_s = 1;
      } else {
        mn[k] = key < mn[k] ? key : mn[k];
        mx[k] = key > mx[k] ? key : mx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = mn[k]; red[3 + k][threadIdx.x] = mx[k]; }
  __syncthreads();
  for (int s = MS_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const long long a = red[k][threadIdx.x + s], c = red[3 + k][threadIdx.x + s];
        if (a < red[k][threadIdx.x]) red[k][threadIdx.x] = a;
        if (c > red[3 + k][threadIdx.x]) red[3 + k][threadIdx.x] = c;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    int bad = flag_s;
    if (!bad && v1 > v0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (red[3 + k][0] - red[k][0] >= KEY_RANGE) bad = 1;
        ws.kmin[b * 3 + k] = red[k][0];
      }
      if (bad) report(status, ST_KEY_RANGE, b);
    }
    ws.bad[b] = bad;
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// one thread per vertex: claim (or find) the slot of its packed key in the puzzle's table and set the part's bit
__global__ __launch_bounds__(MS_BLOCK) void graph_insert_kernel(const double* __restrict__ verts, const int64_t* __restrict__ vert_off,
                                                                const int32_t* __restrict__ part_puzzle, const int32_t* __restrict__ part_slot,
                                                                const int64_t* __restrict__ tab_off, int64_t Pt, int64_t V, GraphWs ws,
                                                                uint64_t* status) {
  const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (v >= V) return;
  const int64_t p = csr_row(vert_off, Pt, v);
  const int b = part_puzzle[p];
  const int slot = part_slot[p];
  if (ws.bad[b] || slot < 0 || slot >= MS_MAX_PARTS) return;
  uint64_t packed = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int64_t key;
    vertex_key(verts[v * 3 + k], &key);           // finite and in range: the range pass refused the puzzle otherwise
    packed |= (uint64_t)(key - ws.kmin[b * 3 + k]) << (KEY_BITS * k);
  }
  const int64_t t0 = tab_off[b];
  const uint64_t cap = (uint64_t)(tab_off[b + 1] - t0);       // a power of two
  unsigned long long* keys = ws.keys + t0;
  uint64_t h = mix64(packed) & (cap - 1);
  for (uint64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long old = atomicCAS(keys + h, (unsigned long long)EMPTY_KEY, (unsigned long long)packed);
    if (old == EMPTY_KEY || old == packed) {
      atomicOr(ws.masks + t0 + h, 1u << slot);
      return;
    }
    h = (h + 1) & (cap - 1);
  }
  report(status, ST_TABLE_FULL, b);
}

// one thread per table slot: a key held by two or more parts connects every pair of them
__global__ __launch_bounds__(MS_BLOCK) void graph_collect_kernel(const int64_t* __restrict__ tab_off, int64_t B, int64_t S, GraphWs ws) {
  const int64_t s = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (s >= S) return;
  const uint32_t m = ws.masks[s];
  if ((m & (m - 1)) == 0) return;
  const int64_t b = csr_row(tab_off, B, s);
  for (uint32_t r = m; r; r &= r - 1) atomicOr(ws.rows + b * MS_MAX_PARTS + __builtin_ctz(r), m);
}

__global__ __launch_bounds__(MS_BLOCK) void graph_write_kernel(GraphWs ws, int64_t B, int M, uint8_t* __restrict__ graph) {
  const int64_t e = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (e >= B * M * M) return;
  const int64_t b = e / ((int64_t)M * M);
  const int i = (int)(e / M % M), j = (int)(e % M);
  graph[e] = (i != j && ((ws.rows[b * MS_MAX_PARTS + i] >> j) & 1u)) ? 1 : 0;
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// workspace layout for S table slots and B puzzles
inline int64_t graph_ws_layout(int64_t S, int64_t B, void* base, GraphWs* ws) {
  int64_t o = 0;
  const int64_t keys = o; o = align256(o + S * 8);
  const int64_t masks = o; o = align256(o + S * 4);
  const int64_t rows = o; o = align256(o + B * MS_MAX_PARTS * 4);
  const int64_t kmin = o; o = align256(o + B * 3 * 8);
  const int64_t bad = o; o = align256(o + B * 4);
  if (ws) {
    char* c = static_cast<char*>(base);
    ws->keys = reinterpret_cast<unsigned long long*>(c + keys);
    ws->masks = reinterpret_cast<uint32_t*>(c + masks);
    ws->rows = reinterpret_cast<uint32_t*>(c + rows);
    ws->kmin = reinterpret_cast<int64_t*>(c + kmin);
    ws->bad = reinterpret_cast<int32_t*>(c + bad);
  }
  return o;
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + MS_BLOCK - 1) / MS_BLOCK); }

}  // namespace

extern "C" int pfpp_mesh_face_cdf(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off, int64_t Pt,
                                  double* area, double* cdf, double* total, uint64_t* status, pfpp_stream_t stream) {
  PFPP_REQUIRE(verts && faces && vert_off && face_off && cdf && total && status, "null pointer");
  PFPP_REQUIRE(Pt >= 0, "bad sizes");
  PFPP_SUPPORTED(Pt <= 0x7fffffff, "more than 2^31 - 1 parts");
  if (Pt == 0) return PFPP_OK;
  hipLaunchKernelGGL(face_cdf_kernel, dim3((unsigned)Pt), dim3(MS_BLOCK), 0, pfpp::as_stream(stream), verts, faces, vert_off, face_off,
                     area, cdf, total, status);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_mesh_sample_surface(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off,
                                        const double* cdf, const double* total, const int32_t* part_puzzle, const int32_t* part_slot,
                                        const int64_t* data_id, const int64_t* puz_part_off, int64_t Pt, int64_t B, int64_t N,
                                        const double* u, uint64_t seed, uint32_t split, int64_t max_parts, double* points,
                                        int32_t* face_idx, double* scale, int32_t* ref_slot, pfpp_stream_t stream) {
  PFPP_REQUIRE(verts && faces && vert_off && face_off && cdf && total && part_puzzle && part_slot && puz_part_off && points,
               "null pointer");
  PFPP_REQUIRE(u || data_id, "null pointer: data_id is needed to generate the uniforms");
  PFPP_REQUIRE(Pt >= 0 && B >= 0 && N >= 1 && max_parts >= 1, "bad sizes");
  PFPP_SUPPORTED(N <= 0x7fffffff && Pt <= 65535 && B <= 0x7fffffff, "at most 65535 parts and 2^31 - 1 points per part");
  if (Pt == 0) return PFPP_OK;
  hipStream_t st = pfpp::as_stream(stream);
  hipLaunchKernelGGL(sample_surface_kernel, dim3(grid_of(N), (unsigned)Pt), dim3(MS_BLOCK), 0, st, verts, faces, vert_off, face_off, cdf,
                     total, part_puzzle, part_slot, data_id, (int)N, u, seed, split, max_parts, points, face_idx);
  int rc = pfpp::check_launch(__func__);
  if (rc != PFPP_OK || B == 0 || (!scale && !ref_slot)) return rc;
  hipLaunchKernelGGL(scale_ref_kernel, dim3((unsigned)B), dim3(MS_BLOCK), 0, st, points, puz_part_off, part_slot, (int)N, scale, ref_slot);
  return pfpp::check_launch(__func__);
}

extern "C" int64_t pfpp_mesh_vertex_graph_workspace(const int64_t* puzzle_nverts_host, int64_t B, int64_t* tab_off_host) {
  if (!puzzle_nverts_host || !tab_off_host || B < 0) return -1;
  int64_t S = 0;
  tab_off_host[0] = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t n = puzzle_nverts_host[b];
    if (n < 0 || n > ((int64_t)1 << 40)) return -1;
    int64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    S += cap;
    tab_off_host[b + 1] = S;
  }
  return graph_ws_layout(S, B, nullptr, nullptr);
}

extern "C" int pfpp_mesh_vertex_graph(const double* verts, const int64_t* vert_off, const int32_t* part_puzzle, const int32_t* part_slot,
                                      const int64_t* puz_part_off, const int64_t* tab_off, int64_t Pt, int64_t B, int64_t V, int64_t S,
                                      int64_t max_parts, uint8_t* graph, void* workspace, int64_t workspace_bytes, uint64_t* status,
                                      pfpp_stream_t stream) {
  PFPP_REQUIRE(verts && vert_off && part_puzzle && part_slot && puz_part_off && tab_off && graph && workspace && status, "null pointer");
  PFPP_REQUIRE(Pt >= 0 && B >= 0 && V >= 0 && S >= 0 && max_parts >= 1, "bad sizes");
  PFPP_SUPPORTED(max_parts <= MS_MAX_PARTS, "max_num_part > 32 (one uint32 mask per key)");
  PFPP_SUPPORTED(B <= 0x7fffffff, "more than 2^31 - 1 puzzles");
  GraphWs ws;
  PFPP_REQUIRE(workspace_bytes >= graph_ws_layout(S, B, workspace, &ws), "workspace smaller than pfpp_mesh_vertex_graph_workspace");
  if (B == 0) return PFPP_OK;
  hipStream_t st = pfpp::as_stream(stream);
  // keys all ones (empty); masks, rows, kmin, bad zero
  const int64_t keys_bytes = reinterpret_cast<char*>(ws.masks) - reinterpret_cast<char*>(ws.keys);
  if (hipMemsetAsync(ws.keys, 0xFF, (size_t)keys_bytes, st) != hipSuccess ||
      hipMemsetAsync(ws.masks, 0, (size_t)(workspace_bytes - keys_bytes), st) != hipSuccess) {
    pfpp::set_error("%s: hipMemsetAsync failed", __func__);
    return PFPP_EHIP;
  }
  hipLaunchKernelGGL(graph_range_kernel, dim3((unsigned)B), dim3(MS_BLOCK), 0, st, verts, vert_off, puz_part_off, ws, status);
  if (V > 0)
    hipLaunchKernelGGL(graph_insert_kernel, dim3(grid_of(V)), dim3(MS_BLOCK), 0, st, verts, vert_off, part_puzzle, part_slot, tab_off, Pt, V,
                       ws, status);
  if (S > 0) hipLaunchKernelGGL(graph_collect_kernel, dim3(grid_of(S)), dim3(MS_BLOCK), 0, st, tab_off, B, S, ws);
  hipLaunchKernelGGL(graph_write_kernel, dim3(grid_of(B * max_parts * max_parts)), dim3(MS_BLOCK), 0, st, ws, B, (int)max_parts, graph);
  return pfpp::check_launch(__func__);
}

extern "C" int pfpp_mesh_status(const uint64_t* status, pfpp_stream_t stream) {
  PFPP_REQUIRE(status, "null pointer");
  hipStream_t st = pfpp::as_stream(stream);
  uint64_t w = 0;
  if (hipMemcpyAsync(&w, status, sizeof(w), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    pfpp::set_error("%s: reading the status word failed", __func__);
    return PFPP_EHIP;
  }
  if (w == ~0ull) return PFPP_OK;
  const uint32_t kind = (uint32_t)(w >> 32), idx = (uint32_t)w;
  switch (kind) {
    case ST_NONFINITE: pfpp::set_error("%s: part %u has a non-finite vertex coordinate", __func__, idx); return PFPP_EINVAL;
    case ST_FACE_INDEX: pfpp::set_error("%s: part %u has a face index outside its vertices", __func__, idx); return PFPP_EINVAL;
    case ST_AREA: pfpp::set_error("%s: part %u: face areas sum to zero or a non-finite value", __func__, idx); return PFPP_EINVAL;
    case ST_KEY_MAG:
      pfpp::set_error("%s: unsupported: puzzle %u has a coordinate beyond 2^52 / 1e5", __func__, idx);
      return PFPP_EUNSUPPORTED;
    case ST_KEY_RANGE:
      pfpp::set_error("%s: unsupported: puzzle %u spans 2^21 or more 1e-5 steps on an axis (the packed key range)", __func__, idx);
      return PFPP_EUNSUPPORTED;
    case ST_TABLE_FULL: pfpp::set_error("%s: unsupported: hash table of puzzle %u is full", __func__, idx); return PFPP_EUNSUPPORTED;
    case ST_ORDER:
      pfpp::set_error("%s: batch puzzle %u: an order entry outside its piece's samples", __func__, idx);
      return PFPP_EINVAL;
    case ST_COUNTS:
      pfpp::set_error("%s: batch puzzle %u: no piece counts (a selection outside the store, more parts than max_parts, or parts x "
                      "min_part_point > num_points)", __func__, idx);
      return PFPP_EINVAL;
    default: pfpp::set_error("%s: unknown status word %llx", __func__, (unsigned long long)w); return PFPP_EINVAL;
  }
}
