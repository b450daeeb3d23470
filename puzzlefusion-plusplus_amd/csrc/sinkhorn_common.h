// Arithmetic shared by the two forms of the potential Sinkhorn: the masked test-time form (matching.hip) and the unmasked training
// form with its backward (matching_train.hip).  Both read L = s / tau and keep a row potential u and a column potential v.
#pragma once
#include "pfpp_common.h"

namespace pfpp {
namespace sk {

// running (max, sum) of a log-sum-exp: one exp per element, no branch on the data.  The exponentials are fp32 (the reference's), the
// running sum is fp64: at N' = 5,000 a column's sum is 64 pushes and 79 partials long, and a chain of that many fp32 roundings
// is worth 4 - 5e-7 (relative) on the column's potential, more than the reference's pairwise fp32 summation loses.
__device__ __forceinline__ void lse_push(float& m, double& s, float x) {
  const float d = x - m;
  const double e = (double)expf(-fabsf(d));
  if (d > 0.0f) { s = s * e + 1.0; m = x; } else { s += e; }
}
__device__ __forceinline__ void lse_merge(float& m, double& s, float m2, double s2) {
  const float nm = fmaxf(m, m2);
  if (nm == -__builtin_huge_valf()) return;            // both empty
  s = s * (double)expf(m - nm) + s2 * (double)expf(m2 - nm);
  m = nm;
}
__device__ __forceinline__ float lse_value(float m, double s) { return m + logf((float)s); }

constexpr int SK_ROWS = 64;       // rows per block of the column sweep

// The potentials are fp64, the entries fp32.  u and v carry the magnitude of L (up to 1 / tau times the affinity, about 20): kept in
// fp32 they would quantise every normalisation at ulp(20) / 2 = 9.5e-7, where the reference's rewrite form, whose entries are near
// 0 after a normalisation, stays at 3 - 4e-7 from the float64 run.  L = s / tau is the reference's fp32 division; the entry (L - u_i) - v_j is formed in fp64 and
// rounded once; the log-sum-exp itself runs in fp32 like the reference's.
__device__ __forceinline__ float sk_entry(float s, float tau, double ui, double vj) {
  return (float)(((double)(s / tau) - ui) - vj);
}

// folding of the column partials: 64 columns per workgroup, the row blocks of a column split over its four waves
constexpr int CB_COLS = 64, CB_PARTS = 4;

}  // namespace sk
}  // namespace pfpp
