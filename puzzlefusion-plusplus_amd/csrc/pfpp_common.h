// Shared host/device helpers for libpfpp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "attn_choice.h"
#include "pfpp.h"

#define PFPP_WAVE 64

namespace pfpp {

// thread-local "last error" text behind pfpp_last_error()
void set_error(const char* fmt, ...);

// Every entry point converts its stream right before launching: also drop any sticky error an
// earlier, unrelated HIP call of the process left behind, so check_launch() reports only ours.
inline hipStream_t as_stream(pfpp_stream_t s) {
  (void)hipGetLastError();
  return reinterpret_cast<hipStream_t>(s);
}

// after a launch: turn a launch failure into PFPP_EHIP
int check_launch(const char* what);

// kernel selection of the attention entry points for launches issued by THIS thread (attn_choice.h): the arithmetic mode of
// pfpp_set_attention_mode and the cross-check bits of pfpp_set_attention_cross_check
AttnPolicy attn_policy();

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace pfpp

// Template instantiation(s) of the most recent GEMM, set-abstraction stage or attention call of this thread, as a kernel trace prints
// them: written by every launcher of gemm.hip, gemm_pl.hip, gemm_grad.hip, pfpp_sa_train_stage (sa_train.hip) and the attention entry
// points, read by pfpp_last_gemm_kernel (gemm_pl.hip).  A call that launches nothing (empty input, rejected arguments) reports "".
namespace pfpp_gemm_detail {
namespace pl { extern thread_local char last_kernel[96]; }
// A launcher formats the name of its instantiation once (a function-local static) and copies it per launch: no printf on the
// launch path.  80 characters + the longest suffix (17) fit last_kernel.
struct KernelName {
  char s[80];
  explicit KernelName(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(s, sizeof(s), fmt, ap);
    va_end(ap);
  }
};
inline void report_kernel(const KernelName& name, const char* suffix = "") { strcpy(stpcpy(pl::last_kernel, name.s), suffix); }
inline void report_no_kernel() { pl::last_kernel[0] = 0; }
// one launch of a call that may launch several kernels (the attention entries): after report_no_kernel() the names join with '+' in
// launch order.  `name` is a literal; the caller static_asserts that its longest sequence fits last_kernel.
inline void report_kernel_also(const char* name) {
  char* end = pl::last_kernel + strlen(pl::last_kernel);
  if (end != pl::last_kernel) *end++ = '+';
  strcpy(end, name);
}
}  // namespace pfpp_gemm_detail

// launch KERN and report it under `name`: its instantiation as a kernel trace prints it (defaulted template arguments written out)
template <auto KERN, typename... Args>
inline void pfpp_launch_named(const char* name, dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args) {
  pfpp_gemm_detail::report_kernel_also(name);
  hipLaunchKernelGGL(KERN, grid, block, smem, st, args...);
}

// internal (attention_bwd.hip): split-f16 forward of the per-fragment attention, launched by pfpp_attn_blockdiag / _split
int pfpp_attn_blockdiag_f16_launch(const float* qkv, float* out, void* out_hi, void* out_lo, int64_t pairs, int64_t L, int64_t H, float scale,
                                   hipStream_t st);

// x = hi + lo with hi = f16(x), lo = f16(x - hi): x - hi is exact in fp32, so the pair carries 22 bits of
// x for |x| >= 2^-3 and an absolute error <= 3e-8 below that (f16 subnormal spacing 6e-8) — the operand
// format of the PFPP_GEMM_F16X3 path (csrc/gemm.hip).  lo is NOT pre-scaled, so hi.hi, hi.lo and lo.hi
// accumulate into one fp32 accumulator.
struct pfpp_hl { _Float16 hi, lo; };
__device__ __forceinline__ pfpp_hl pfpp_split(float x) {
  pfpp_hl r;
  r.hi = (_Float16)x;
  r.lo = (_Float16)(x - (float)r.hi);
  return r;
}
// assigns into two targets (vector elements are not bindable to references)
#define PFPP_SPLIT_TO(x, HI, LO) do { const pfpp_hl _s = pfpp_split(x); (HI) = _s.hi; (LO) = _s.lo; } while (0)

// optional split-f16 copy of a kernel's result (operand of the plane GEMM, csrc/gemm_pl.hip): planes of scale * value.
// Host side: pfpp_planes (include/pfpp.h) -> pfpp_planes_out by pfpp_planes_arg().
struct pfpp_planes_out { _Float16* hi; _Float16* lo; float scale; };
inline pfpp_planes_out pfpp_planes_arg(const pfpp_planes* p) {
  pfpp_planes_out o;
  o.hi = p ? reinterpret_cast<_Float16*>(p->hi) : nullptr;
  o.lo = p ? reinterpret_cast<_Float16*>(p->lo) : nullptr;
  o.scale = p ? p->scale : 1.0f;
  return o;
}
inline bool pfpp_planes_ok(const pfpp_planes* p) {
  return !p || (p->hi && p->lo && (reinterpret_cast<uintptr_t>(p->hi) & 7u) == 0 && (reinterpret_cast<uintptr_t>(p->lo) & 7u) == 0);
}
__device__ __forceinline__ void pfpp_store4_planes(const pfpp_planes_out& po, int64_t idx, float4 v) {
  typedef _Float16 h4_ __attribute__((ext_vector_type(4)));
  h4_ hi, lo;
  PFPP_SPLIT_TO(v.x * po.scale, hi[0], lo[0]);
  PFPP_SPLIT_TO(v.y * po.scale, hi[1], lo[1]);
  PFPP_SPLIT_TO(v.z * po.scale, hi[2], lo[2]);
  PFPP_SPLIT_TO(v.w * po.scale, hi[3], lo[3]);
  *reinterpret_cast<h4_*>(po.hi + idx) = hi;
  *reinterpret_cast<h4_*>(po.lo + idx) = lo;
}

// counter-based generator behind the dropout sites (pfpp_dropout / pfpp_geglu): splitmix64 finaliser
// of (seed, site, element index); forward and backward regenerate the same keep mask.
__host__ __device__ __forceinline__ uint32_t pfpp_rng_u32(uint64_t seed, uint32_t site, uint64_t idx) {
  uint64_t z = seed ^ ((uint64_t)site * 0xD6E8FEB86659FD93ull);
  z += (idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}
// the full 64-bit word of the same finaliser (mesh surface sampling, csrc/mesh_sample.hip: u = (z >> 11) 2^-53)
__host__ __device__ __forceinline__ uint64_t pfpp_rng_u64(uint64_t seed, uint32_t site, uint64_t idx) {
  uint64_t z = seed ^ ((uint64_t)site * 0xD6E8FEB86659FD93ull);
  z += (idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// keep threshold for drop probability p: keep iff rng >= thresh
inline uint32_t pfpp_drop_thresh(float p) {
  const double t = (double)p * 4294967296.0;
  return t <= 0.0 ? 0u : (t >= 4294967295.0 ? 4294967295u : (uint32_t)t);
}

// A kernel that takes more dynamic LDS than the default cap has to be allowed to, once.  The attribute belongs to the function
// ON a device, so the "done" mask holds one bit per device; KERN is a template argument, so every kernel has its own mask.
template <auto KERN>
inline hipError_t pfpp_allow_dyn_lds(int bytes = 160 * 1024) {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
  return e;
}

#define PFPP_REQUIRE(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) {                                                \
      pfpp::set_error("%s: %s", __func__, msg);                   \
      return PFPP_EINVAL;                                         \
    }                                                             \
  } while (0)

#define PFPP_SUPPORTED(cond, msg)                                 \
  do {                                                            \
    if (!(cond)) {                                                \
      pfpp::set_error("%s: unsupported: %s", __func__, msg);      \
      return PFPP_EUNSUPPORTED;                                   \
    }                                                             \
  } while (0)

// Wave priority of the kernels on the training step's dependency chain (round 5; -DPFPP_CHAIN_PRIO=n at build time, 0 = off):
// s_setprio only arbitrates instruction issue between the waves resident on one SIMD, so chain kernels that share CUs with the next
// iteration's encoder (CU-masked stream) or the weight-gradient stream issue first and the co-runners fill their stalls.  The
// iteration is the chain (4.93 ms alone) stretched by the encoder running under it (5.98 ms; the weight gradients are fully hidden:
// profiles/r05c_ab_masks_and_lab_skips.txt); priority 3 takes 1.3 % off (6.18 -> 6.10 ms alternating on one box,
// profiles/r05d_ab_chain_prio.txt).  Results are unchanged bit for bit (scheduling only).
#ifndef PFPP_CHAIN_PRIO
#define PFPP_CHAIN_PRIO 3
#endif
#ifdef __HIPCC__
__device__ __forceinline__ void pfpp_chain_prio() {
  if constexpr (PFPP_CHAIN_PRIO > 0) __builtin_amdgcn_s_setprio(PFPP_CHAIN_PRIO);
}
#endif
