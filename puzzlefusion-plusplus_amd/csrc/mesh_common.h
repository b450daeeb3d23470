// What the mesh units share (csrc/mesh_sample.hip, csrc/matching_dataset.hip): the device status word and one surface sample of
// trimesh.sample.sample_surface.  Both units are compiled with -ffp-contract=off, so the function below is the same sequence of
// IEEE operations wherever it is inlined.
#pragma once
#include <math.h>

#include "pfpp_common.h"

namespace pfpp_mesh {

// status kinds (the word is (kind << 32) | index; the host decodes it in pfpp_mesh_status)
enum : uint32_t { ST_NONFINITE = 1, ST_FACE_INDEX = 2, ST_AREA = 3, ST_KEY_MAG = 4, ST_KEY_RANGE = 5, ST_TABLE_FULL = 6, ST_ORDER = 7, ST_COUNTS = 8 };

__device__ __forceinline__ void report(uint64_t* status, uint32_t kind, int64_t index) {
  atomicMin(reinterpret_cast<unsigned long long*>(status), (unsigned long long)(((uint64_t)kind << 32) | (uint32_t)index));
}

// (pfpp_rng_u64 >> 11) 2^-53: a uniform double in [0, 1)
__device__ __forceinline__ double uniform53(uint64_t seed, uint32_t split, uint64_t idx) {
  return (double)(pfpp_rng_u64(seed, split, idx) >> 11) * 0x1.0p-53;
}

// One sample of a part with nf >= 1 faces (part-local indices, nv vertices): the face is the lower bound of u0 total in the part's
// cdf (np.searchsorted side='left', clamped to the last face), (l0, l1) are folded into the triangle and
// p = ((b - a) l0 + (c - a) l1) + a.  A face index outside the part (reported by the cdf pass) gives NaN.  Returns the face.
__device__ __forceinline__ int64_t sample_point(const double* __restrict__ pv, const int32_t* __restrict__ pf, int64_t nv, int64_t nf,
                                                const double* __restrict__ c, double total, double u0, double l0, double l1, double* out) {
  const double pick = u0 * total;
  int64_t lo = 0, hi = nf;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < pick) lo = mid + 1; else hi = mid;
  }
  const int64_t f = lo < nf ? lo : nf - 1;
  // random_lengths[l0 + l1 > 1] -= 1; abs
  if (l0 + l1 > 1.0) { l0 = l0 - 1.0; l1 = l1 - 1.0; }
  l0 = fabs(l0); l1 = fabs(l1);
  const int32_t* fc = pf + f * 3;
  const int32_t ia = fc[0], ib = fc[1], ic = fc[2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= nv || ib >= nv || ic >= nv) {
    out[0] = out[1] = out[2] = __builtin_nan("");
    return f;
  }
  const double* a = pv + (int64_t)ia * 3;
  const double* b = pv + (int64_t)ib * 3;
  const double* cc = pv + (int64_t)ic * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double ak = a[k];
    out[k] = ((b[k] - ak) * l0 + (cc[k] - ak) * l1) + ak;
  }
  return f;
}

}  // namespace pfpp_mesh
