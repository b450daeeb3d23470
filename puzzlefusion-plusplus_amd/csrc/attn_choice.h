// Which kernel an attention entry point launches: pure functions of the call's sizes and flags and of the calling thread's policy
// (host-only C++, no HIP types; nothing here reads the environment).  The entry points of attention.hip, attention_bwd.hip and
// transformer_ops.hip validate, choose here, launch through one switch and report the launch (pfpp_last_gemm_kernel);
// tests/test_gpu_parity.py::test_attention_kernel_choice_is_pinned pins every rule at both sides of its edges.
#pragma once
#include <limits.h>
#include <stdint.h>

namespace pfpp {

// mode (pfpp_set_attention_mode): -1 = each kernel's default, 0 = exact fp32 matrix instructions, 1 = split-f16, 2 = single-pass
// fp16 (perf mode, never for parity); it governs the FORWARD kernels.  cross (pfpp_set_attention_cross_check): kernels that the
// product never picks by itself, kept as cross-checks of the default ones; 0 in the product.
struct AttnPolicy { int mode; unsigned cross; };
enum : unsigned {
  ATTN_X_DENSE_F32 = 1u,      // dense: the exact-fp32 kernels where split-f16 is the default (forward at mode -1; backward)
  ATTN_X_BD_F32 = 2u,         // block-diagonal: the exact fp32 matrix instructions instead of the split-f16 contraction
  ATTN_X_BD_SCALAR = 4u,      // block-diagonal: the scalar kernels instead of the matrix-instruction ones
  ATTN_X_NO_SHORT = 8u,       // dense forward: the tile walker where the short-sequence kernel would run
  ATTN_X_ALL = 15u,
};

// Split-f16 is the default of the dense forward at dim_head 64: 44.6 -> 26.3 us on the compacted (ragged) token list, where the
// longest sequence's walk over its key tiles is the critical path, and 226 -> 127 us on the all-slots form (32 x 500 keys, masked).
// (Its first version stored V^T with 2-byte LDS writes: 661 us there; pairs of keys as swizzled 4-byte words fixed it.)
// Few short sequences (one puzzle in flight) go to attn_dense_short_kernel, which splits the keys over the waves of 32-query
// workgroups: up to this length, while the tile walker would put no more than this many 128-query workgroups on the chip.
constexpr int ATTN_SHORT_MAX_LEN = 512, ATTN_SHORT_MAX_WGS = 64;
// dim_head 32 takes the split-f16 kernel from this many keys on: the verifier's attention over thousands of candidate edges
// (100-fragment puzzles: 4,950 keys per query) runs 3 f16 MFMAs per 16-deep step instead of 8 fp32 ones; the 190 edges of the
// reference's 20-fragment puzzles keep the exact-fp32 kernel
constexpr int ATTN_F16_DH32_MIN_LEN = 1024;

enum class AttnKern {
  DenseF32, DenseF16, DenseF16Single, DenseShort,      // attn_dense_kernel<dh>, attn_dense_f16_kernel<dh, false / true>, attn_dense_short_kernel<64>
  DenseBwdF32, DenseBwdF16,                            // attn_dense_bwd_{dq,dkv}_kernel<dh>, attn_dense_bwd_{dq,dkv}_f16_kernel
  BdF16, BdMfma, BdScalar,                             // attn_blockdiag[_bwd]_f16_kernel, .._mfma_kernel, attn_blockdiag[_bwd]_kernel
};

// the forward's arithmetic: an explicit mode decides; at the default the cross-check bit does
inline bool attn_fwd_f16(const AttnPolicy& p, unsigned f32_bit) { return p.mode < 0 ? !(p.cross & f32_bit) : p.mode >= 1; }

// pfpp_attn_dense, _split, _train, _train_p.  train: an lse is written (the training forward keeps its fp32-grade statistics, so
// neither the single-pass kernel nor the short one, which has no lse output, serves it)
inline AttnKern choose_attn_dense_fwd(int dh, int64_t max_len, int64_t H, int64_t n_seq, bool train, const AttnPolicy& p) {
  const bool f16 = attn_fwd_f16(p, ATTN_X_DENSE_F32);
  if (p.mode == 2 && !train) return AttnKern::DenseF16Single;
  if (dh == 64 && f16 && !train && !(p.cross & ATTN_X_NO_SHORT) && max_len <= ATTN_SHORT_MAX_LEN &&
      (max_len + 127) / 128 * H * n_seq <= ATTN_SHORT_MAX_WGS)
    return AttnKern::DenseShort;
  if (f16 && (dh == 64 || (dh == 32 && max_len >= ATTN_F16_DH32_MIN_LEN))) return AttnKern::DenseF16;
  return AttnKern::DenseF32;
}

// pfpp_attn_dense_bwd, _p and _parts: the split-f16 passes for the unmasked (ragged) launches at dim_head 64, the fp32 <dh> passes
// otherwise.  The mode is NOT consulted: it governs the forward (include/pfpp.h), and exact_fp32() has never switched a backward
// kernel.  Plane output exists in the split-f16 passes only.
inline AttnKern choose_attn_dense_bwd(int dh, bool masked, const AttnPolicy& p) {
  return dh == 64 && !masked && !(p.cross & ATTN_X_DENSE_F32) ? AttnKern::DenseBwdF16 : AttnKern::DenseBwdF32;
}

// pfpp_attn_blockdiag, _split.  pairs = fragments x heads (the split-f16 kernel takes one workgroup per pair)
inline AttnKern choose_attn_blockdiag_fwd(int64_t pairs, const AttnPolicy& p) {
  if (p.cross & ATTN_X_BD_SCALAR) return AttnKern::BdScalar;
  return attn_fwd_f16(p, ATTN_X_BD_F32) && pairs <= INT_MAX ? AttnKern::BdF16 : AttnKern::BdMfma;
}

// pfpp_attn_blockdiag_bwd, _p.  The mode is not consulted here either.  Only the matrix-instruction kernels write planes, so a call
// with planes gets one of them whatever ATTN_X_BD_SCALAR says; with that bit alone and no planes the scalar kernel runs.
inline AttnKern choose_attn_blockdiag_bwd(bool planes, const AttnPolicy& p) {
  if ((p.cross & ATTN_X_BD_SCALAR) && !planes) return AttnKern::BdScalar;
  return p.cross & ATTN_X_BD_F32 ? AttnKern::BdMfma : AttnKern::BdF16;
}

}  // namespace pfpp
