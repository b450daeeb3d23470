// The AdamW update of ONE element, shared by every kernel that applies it: adamw_kernel and adam_multi_kernel (train_ops.hip) and
// the update epilogue of the grouped weight-gradient launch (gemm_pl.hip).  One function, so the kernels agree bit for bit.
//
// The fused multiply-adds are written out under contract(off).  Left to the compiler, the contraction of `v * beta2 + w2 * (g * g)`
// (two products and a sum) and of the other three sums falls as each kernel's instruction selection happens to: the same source
// expression came out as fma(beta2, v, w2 g^2) in one kernel and fma(w2, g^2, beta2 v) in another, one rounding apart.  The forms
// below are the ones adamw_kernel compiled to on gfx950 while it still spelled the update out itself (both instantiations, read from
// the disassembly), pinned: every product that is rounded on its own there is a statement of its own here.
#pragma once
#include "pfpp_common.h"

struct pfpp_adamw_hp {               // lr, betas, eps, weight decay and the bias corrections as the kernels consume them
  float decay;                       // 1 - lr * weight_decay
  float w1, beta2, w2;               // 1 - beta1, beta2, 1 - beta2
  float eps, step_size;              // eps, lr / bc1
  float inv_sqrt_bc2, g_scale;       // 1 / sqrt(bc2), factor applied to the stored gradient
};

inline pfpp_adamw_hp pfpp_adamw_hp_of(float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2, float g_scale) {
  pfpp_adamw_hp h;
  h.decay = 1.0f - lr * weight_decay; h.w1 = 1.0f - beta1; h.beta2 = beta2; h.w2 = 1.0f - beta2;
  h.eps = eps; h.step_size = lr / bc1; h.inv_sqrt_bc2 = 1.0f / sqrtf(bc2); h.g_scale = g_scale;
  return h;
}

// the overflow guard's test: inf or NaN (an element that fails it keeps p, m, v and its planes, and raises the step's flag)
__device__ __forceinline__ bool pfpp_adamw_nonfinite(float g) { return !(fabsf(g) <= 3.0e38f); }

// p, m, v of one element and its (already scaled) gradient g -> the new p; m and v are updated in place
__device__ __forceinline__ float pfpp_adamw_element(float p, float g, float& m, float& v, float decay, float w1, float beta2, float w2,
                                                    float eps, float step_size, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  const float gg = g * g;
  const float vb = v * beta2;
  v = __builtin_fmaf(w2, gg, vb);                    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float d = g - m;
  m = __builtin_fmaf(w1, d, m);                      // exp_avg.lerp_(grad, 1 - beta1)
  const float denom = __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
  const float q = m / denom;
  const float upd = step_size * q;
  return __builtin_fmaf(decay, p, -upd);             // p * (1 - lr * weight_decay) - (lr / bc1) * m / denom
}
