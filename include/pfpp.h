/*
 * pfpp.h — C ABI of libpfpp_hip.so: the MI355X (gfx950) kernels behind the
 * denoise-and-verify hot path of PuzzleFusion++.
 *
 * The reference has no native code on this path: every function below replaces
 * a group of stock-PyTorch / third-party ops.  Each entry cites the reference
 * lines it replaces (paths relative to the reference checkout).  The only
 * native precedent in the reference tree is Jigsaw_matching/utils/chamfer/cuda/
 * chamfer.cpp:8-23 (contiguity checks on the host side, raw pointers + sizes
 * into the launcher); this header follows the same split: the Python wrappers
 * validate dtype / contiguity / shapes, the C side takes plain pointers.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *   - all tensors are dense row-major; "ld*" = leading dimension in elements;
 *   - fp32 everywhere (the reference runs precision 32,
 *     config/denoiser/global_config.yaml:39); indices are int32 at this
 *     boundary (the Python mirror widens to int64 where the reference API
 *     returns int64);
 *   - `stream` is a hipStream_t passed as void*; kernels are only enqueued,
 *     never synchronised; nothing is allocated or freed by the library;
 *   - return value: PFPP_OK (0) or a negative PFPP_E* code.  Nothing throws
 *     across the ABI.  pfpp_last_error() returns a static string describing
 *     the most recent failure on the calling thread.
 */
#ifndef PFPP_H_
#define PFPP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFPP_OK 0
#define PFPP_EINVAL (-1)     /* bad size / alignment / null pointer            */
#define PFPP_EUNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define PFPP_EHIP (-3)       /* hipGetLastError() != hipSuccess after launch   */

typedef void* pfpp_stream_t;

/* ---- library ------------------------------------------------------------ */
#define PFPP_ABI_VERSION 2
int pfpp_version(void);                 /* ABI version = PFPP_ABI_VERSION (2: pfpp_build_info, per-thread attention mode) */
/* "abi=2;arch=gfx950;fma_mix_insts=off;packed_fp32_ops=off;chain_prio=3": the code-generation switches this binary was compiled
 * with.  Two of them are CORRECTNESS switches: a binding must refuse a library that does not say "off" for both
 * (pfpp_hip/_lib.py does; PFPP_PACKED_FP32=1 is the lab override for the second) */
const char* pfpp_build_info(void);
const char* pfpp_last_error(void);
/* sizeof(struct pfpp_<name>) as this library was compiled ("gemm_planes_args", "tlayers_args", ...), -1 for an unknown name: a binding
 * that mirrors the structs (pfpp_hip/_lib.py) checks its own layout against it when it loads, so a stale mirror fails loudly    */
int64_t pfpp_abi_sizeof(const char* name);
/* number of compute units of the current device (for grid sizing in hosts) */
int pfpp_device_cu_count(void);
/* arithmetic of the attention FORWARD kernels for launches issued by the CALLING THREAD (thread-local like pfpp_last_error: the
 * library keeps no process-global mutable state) (pfpp_attn_dense*, pfpp_attn_blockdiag*; diffusers Attention,
 * attention.py:46-72 via denoiser_transformer.py:46-72): -1 = each kernel's default (split-f16 where there is such a kernel),
 * 0 = exact fp32 matrix instructions (the range fallback of the sampler loops, pfpp_hip.ops.exact_fp32),
 * 1 = split-f16, 2 = single-pass fp16 (perf mode of BASELINE configs[4]; never a parity mode). */
int pfpp_set_attention_mode(int mode);
int pfpp_get_attention_mode(void);
/* cross-check kernels of the attention entry points, thread-local like the mode and 0 by default: a mask of 1 = DENSE_F32 (dense
 * attention: exact-fp32 kernels where split-f16 is the default, forward at mode -1 and backward), 2 = BD_F32 (block-diagonal: exact
 * fp32 matrix instructions), 4 = BD_SCALAR (block-diagonal: the scalar kernels; a call with plane output keeps a matrix-instruction
 * kernel), 8 = NO_SHORT (dense forward: the tile walker where the short-sequence kernel would run).  The product leaves it 0; the
 * tests compare the kernels it selects with the default ones.  PFPP_EINVAL for an unknown bit.  No environment variable selects an
 * attention kernel.  Every attention entry point names the kernel(s) it launched in pfpp_last_gemm_kernel(). */
int pfpp_set_attention_cross_check(unsigned bits);
unsigned pfpp_get_attention_cross_check(void);

/* ---- a1: SE(3) rotate + valid-fragment gather ----------------------------
 * Denoiser._apply_rots (puzzlefusion_plusplus/denoiser/model/denoiser.py:55-63,
 * = auto_aggl.py:70-78) followed by the boolean gather denoiser.py:69.
 *   q = pose[slot,3:7] / ||q||   (w,x,y,z);  out = (q * (0,p) * conj(q)).xyz
 * evaluated in exactly pytorch3d's quaternion_raw_multiply operation order with
 * no FMA contraction, so the rotated coordinates are bit-identical to the CPU
 * path (FPS downstream is an argmax chain and must not fork).
 *   part_pcs [n_slots, N, 3], pose [n_slots, 7], slot [F] (flattened b*P+p of
 *   each valid fragment, ascending) -> out [F, N, 3]                          */
int pfpp_se3_rotate_gather(const float* part_pcs, const float* pose,
                           const int32_t* slot, float* out,
                           int64_t F, int64_t N, pfpp_stream_t stream);

/* ---- a19: pose apply  R(q^)p + t  ----------------------------------------
 * utils/node_merge_utils.py:43-53 get_final_pose_pts (normalise=1) and the
 * per-part body of get_final_pose_pts_dynamic :16-41 (normalise=0: pytorch3d
 * quaternion_apply does not normalise).  pts [n, N, 3], pose [n,7]=(t, q).
 * `scale` (may be NULL) multiplies the points first (auto_aggl.py:160-162). */
int pfpp_pose_apply(const float* pts, const float* pose, const float* scale,
                    float* out, int64_t n, int64_t N, int normalise,
                    pfpp_stream_t stream);

/* ---- a2: farthest point sampling -----------------------------------------
 * torch_cluster.fps(random_start=False) as called at utils/pn2_utils.py:131-137
 * + the centroid gather index_points :139.  Start index 0, d = (dx*dx + dy*dy)
 * + dz*dz in fp32 without FMA, running min, next = first argmax.
 *   xyz [F, N, 3] -> idx [F, S] (local indices), new_xyz [F, S, 3]
 * Supported: 1 <= S <= N <= 4096.                                           */
int pfpp_fps(const float* xyz, int32_t* idx, float* new_xyz,
             int64_t F, int64_t N, int64_t S, pfpp_stream_t stream);

/* ---- a3: ball query ---------------------------------------------------------
 * square_distance + query_ball_point, utils/pn2_utils.py:21-42, 92-112.
 * d = ((-2*dot) + |c|^2) + |p|^2 with dot = fma(c2,p2, fma(c1,p1, c0*p0))
 * (what the CPU BLAS K=3 matmul evaluates) and squared norms (x*x+y*y)+z*z;
 * a point is kept unless d > r2; the first `nsample` kept indices in index
 * order are returned, padded with the first kept index.
 *   xyz [F,N,3], new_xyz [F,S,3] -> idx [F,S,nsample]; nsample <= 64.       */
int pfpp_ball_query(const float* xyz, const float* new_xyz, int32_t* idx,
                    int64_t F, int64_t N, int64_t S, int64_t nsample,
                    float r2, pfpp_stream_t stream);

/* ---- a2 + a3 for the three set-abstraction levels at once ------------------
 * PN2.encode (vqvae/model/modules/pn2.py:57-68) runs sample_and_group (utils/pn2_utils.py:127-151) three times; the
 * sampling part (farthest_point_sample :131-134 + query_ball_point :92-111) depends on the coordinates only.  One
 * launch, one workgroup per fragment: level l samples S_l points out of the S_(l-1) centroids of the level above (level 0: the
 * N input points) and ball-queries them with radius^2 r2_l.  Outputs exactly what pfpp_fps / pfpp_ball_query return for
 * each level (bit-identical).  N <= 2048, levels[0].S <= 256, levels[1].S <= 128, nsample <= 64.                        */
typedef struct pfpp_sample_level {
  int64_t S, nsample;
  float r2;
  int32_t* fps_idx;    /* [F, S] or NULL */
  float* new_xyz;      /* [F, S, 3] */
  int32_t* ball_idx;   /* [F, S, nsample] */
} pfpp_sample_level;
int pfpp_sample_levels(const float* xyz, int64_t F, int64_t N, const pfpp_sample_level* levels /* [3] */, pfpp_stream_t stream);

/* ---- a4: grouping --------------------------------------------------------
 * index_points x3 + concat, utils/pn2_utils.py:139-146, written channels-last
 * as the A operand of the first set-abstraction GEMM:
 *   row (f,s,j) = [ feats[f, idx, 0:D] | xyz[f,idx]-new_xyz[f,s] | 0-pad ]
 * (features first so the D-wide copy is 16-byte aligned; the packed conv
 * weight has its input columns permuted the same way).
 *   feats [F,N,D] or NULL (D=0), out [F*S*ns, ldo], ldo >= D+3, ldo % 4 == 0 */
int pfpp_group_gather(const float* xyz, const float* new_xyz,
                      const float* feats, const int32_t* idx, float* out,
                      int64_t F, int64_t N, int64_t S, int64_t ns, int64_t D,
                      int64_t ldo, pfpp_stream_t stream);

/* ---- GEMM: C = epilogue(A . op(W)) on fp32 MFMA ----------------------------
 * The one contraction kernel behind a5 (1x1 conv + BN + ReLU + max over
 * nsample, utils/pn2_utils.py:209-214), a6 (conv6, pn2.py:65), a9 (Linear
 * 148->512 / 147->512, denoiser_transformer.py:131-134), a11 (AdaLN linear,
 * attention.py:22), a12-a14 (to_q/k/v, QK^T, PV, to_out, GEGLU feed-forward,
 * attention.py:77-90), a15 (output heads, denoiser_transformer.py:138-147)
 * and a18 (verifier, verifier_transformer.py:42-66).
 * v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate.
 *
 *   A [M,K] row-major (lda);  W is [N,K] row-major (w_kmajor=0, the layout of
 *   torch Linear / 1x1-conv weights) or [K,N] row-major (w_kmajor=1);
 *   C [M,N] (ldc) — or [M/pool, N] when pool > 0.
 *   lda, ldw multiples of 4, A/W 16-byte aligned.
 * Batched: blockIdx.z = z; operand X is offset by (z / zdiv)*sX0 + (z % zdiv)*sX1.
 * Epilogue order: v = acc; v = v*scale[n] + shift[n] (if scale) else v += bias[n]
 * (if bias); activation; v += R[m,n] (if residual); store or max-pool.       */
enum {
  PFPP_ACT_NONE = 0,
  PFPP_ACT_RELU = 1,
  PFPP_ACT_SILU = 2,
  PFPP_ACT_GELU = 3,  /* exact erf GELU */
  PFPP_ACT_GEGLU = 4  /* C[m,j] = u * gelu(g): u,g = value/gate columns; W packed
                         as 32-column value block followed by its 32-column gate
                         block (see pfpp_hip.pack_geglu); C has N/2 columns   */
};

/* arithmetic of the contraction (see csrc/gemm.hip):
 *   PFPP_GEMM_F32   v_mfma_f32_32x32x2_f32, exact fp32 products (157 TFLOP/s roofline)
 *   PFPP_GEMM_F16X3 split-f16: x = hi + lo (hi = f16(x), lo = f16(x - hi)), A.W = hi.hi + hi.lo + lo.hi on
 *                   v_mfma_f32_32x32x16_f16 — fp32-grade error (dropped term 2^-22 relative; elements
 *                   below 2^-3 carry an absolute error <= 3e-8) at up to 16/3 of the fp32-MFMA rate;
 *                   needs |x| < 65504; not available with w_kmajor.
 *                   W may be handed over pre-split (w_hi/w_lo: fp16 [N, ldw] planes, ldw = K rounded
 *                   up to 8 and zero padded) or as fp32 (split on the fly). */
enum { PFPP_GEMM_F32 = 0, PFPP_GEMM_F16X3 = 1, PFPP_GEMM_F16 = 2 };

/*   PFPP_GEMM_F16   single-pass fp16 on pre-split operands (a_hi / w_hi planes only, ONE v_mfma_f32_32x32x16_f16 per product,
 *                   fp32 accumulate): the perf mode of BASELINE.json configs[4].  ~1e-3 relative error: not the parity mode. */
typedef struct pfpp_gemm_args {
  const float* A; const float* W; float* C;
  const void* w_hi; const void* w_lo;   /* pre-split fp16 planes of W, or NULL */
  const void* a_hi; const void* a_lo;   /* pre-split fp16 planes of A [M, lda] (then A may be NULL; needs
                                           w_hi/w_lo, K % 32 == 0, lda % 8 == 0), or NULL              */
  void* c_hi; void* c_lo;               /* if set: write the result as split planes [.., ldc] instead of C */
  const float* bias;      /* [N] or NULL */
  const float* scale;     /* [N] or NULL (then shift must be set) */
  const float* shift;     /* [N] */
  const float* residual;  /* [M, ldr] or NULL; batched with C's strides */
  int64_t M, N, K;
  int64_t lda, ldw, ldc, ldr;
  int32_t w_kmajor;       /* 0: W[N,K]; 1: W[K,N] */
  int32_t act;            /* PFPP_ACT_* */
  int32_t pool;           /* 0, 32 or 64: max over groups of `pool` rows */
  int32_t batch, zdiv;    /* batch >= 1; zdiv >= 1 */
  int32_t precision;      /* PFPP_GEMM_* */
  int64_t sA0, sA1, sW0, sW1, sC0, sC1;
  int64_t sV0, sV1;       /* batch strides of bias / scale / shift */
  float alpha;            /* acc *= alpha before the epilogue (1.0 = off) */
  /* train-mode BatchNorm fusion (set-abstraction MLPs with the encoder in .train(), see pfpp_bn_finalize):
   * a_mul/a_add [K]: A is read as relu(A*a_mul[k] + a_add[k]);  stats: fp64 [stats_copies][2][N], receives
   * (atomically) the column sums and sums of squares of the bias-added result;  c_min: with pool > 0 the
   * per-group minimum [M/pool, ldc] next to the maximum in C.  All NULL/0 = off.                        */
  const float* a_mul; const float* a_add;
  double* stats; int32_t stats_copies;
  float* c_min;
  /* optional split-K workspace (skinny GEMMs: few output tiles, long K — the B = 1 sampler step): when lent, the
   * library may cut K over several workgroups per tile; partials are parked in split_ws (>= split_ws_bytes), the
   * last workgroup of a tile (tickets in split_cnt, split_cnt_len ints, all zero between launches) adds them in chunk
   * order and runs the epilogue — results are deterministic.  Must not be shared by launches that may overlap.  */
  float* split_ws; int64_t split_ws_bytes;
  int32_t* split_cnt; int64_t split_cnt_len;
  /* fused grouping (a4 + a5, utils/pn2_utils.py:127-151 followed by the first 1x1 convolution, :210-213): when
   * gather_idx is set, row r = (f*S + s)*ns + j of the A operand is never materialised — it is read in place as
   *   [ A[f*gather_N + gather_idx[r], 0:D] | gather_xyz[f, idx] - gather_ctr[f*S + s] | 0 ],  D = lda, K = D + 4
   * i.e. exactly what pfpp_group_gather writes (A = the level's input features [F*N, D], unused when D = 0).
   * Needs the f16x3 path with pre-split W, D % 32 == 0, batch 1, no a_mul.  NULL = off.                      */
  const int32_t* gather_idx; const float* gather_xyz; const float* gather_ctr;
  int32_t gather_N, gather_S, gather_ns;
} pfpp_gemm_args;

int pfpp_gemm(const pfpp_gemm_args* args, pfpp_stream_t stream);

/* Optional split-f16 copy of a kernel's result, the operand format of pfpp_gemm_planes: hi = f16(scale * v),
 * lo = f16(scale * v - hi), same indexing as the fp32 result.  scale is a power of two (gradients are lifted into the
 * normal fp16 range; the consuming GEMM divides it out through alpha).  hi / lo: 8-byte aligned fp16 buffers.       */
typedef struct pfpp_planes { void* hi; void* lo; float scale; } pfpp_planes;

/* Plane-producing forms of the training kernels (a17): same arithmetic as the entry points they extend (cited
 * there), with the result additionally — or, where the fp32 pointer may be NULL, only — written as pfpp_planes for the
 * following pfpp_gemm_planes launches: no separate conversion pass over the activations / gradients.
 *   pfpp_split_planes          planes of an fp32 tensor (n % 4 == 0)
 *   pfpp_colsum_planes         out[c] += out_scale * sum_r (hi + lo)[r, c]   (bias gradients of dY given as planes)
 *   pfpp_geglu_p / _bwd_p      pfpp_geglu / pfpp_geglu_bwd; u (dz) may be NULL
 *   pfpp_dropout_layernorm_p   pfpp_dropout_layernorm; n_out may be NULL
 *   pfpp_layernorm_bwd_p       pfpp_layernorm_bwd(_dropout): `dropout` selects the fused dropout of the backward chain
 *                              (drop_out may then be NULL); ret_planes = planes of the value the chain continues with
 *                              (dropped-out gradient, or the updated dx without dropout), dx_planes = planes of the updated dx
 *   pfpp_attn_dense_train_p    pfpp_attn_dense_train; out may be NULL
 *   pfpp_attn_dense_bwd_p, pfpp_attn_blockdiag_bwd_p    dqkv may be NULL (split-f16 / matrix-core kernels only)      */
int pfpp_split_planes(const float* x, int64_t n, const pfpp_planes* planes, pfpp_stream_t stream);
int pfpp_colsum_planes(const void* hi, const void* lo, float* out, int64_t rows, int64_t cols, int64_t ld,
                       float out_scale, pfpp_stream_t stream);
int pfpp_geglu_p(const float* z, float* u, int64_t rows, int64_t inner, float p, uint64_t seed, uint32_t site,
                 const pfpp_planes* u_planes, pfpp_stream_t stream);
int pfpp_geglu_bwd_p(const float* z, const float* du, float* dz, int64_t rows, int64_t inner, float p, uint64_t seed,
                     uint32_t site, const pfpp_planes* dz_planes, pfpp_stream_t stream);
int pfpp_dropout_layernorm_p(const float* y, const float* res, float* h_out, float* n_out, const float* mod,
                             int64_t ld_mod, const float* gamma, const float* beta, const int32_t* group_batch,
                             int64_t group_rows, int64_t rows_per_batch, int64_t rows, int64_t C, float eps, float p,
                             uint64_t seed, uint32_t site, const pfpp_planes* n_planes, pfpp_stream_t stream);
int pfpp_layernorm_bwd_p(const float* x, const float* dy, const float* mod, int64_t ld_mod, const float* gamma,
                         const int32_t* group_batch, int64_t group_rows, int64_t rows_per_batch, float* dx,
                         float* dmult, float* dadd, int64_t ld_d, int64_t rows, int64_t C, float eps, float* drop_out,
                         float p, uint64_t seed, uint32_t site, int32_t dropout, const pfpp_planes* ret_planes,
                         const pfpp_planes* dx_planes, pfpp_stream_t stream);
int pfpp_attn_dense_train_p(const float* qkv, float* out, float* lse, const int32_t* seq_off, const int32_t* seq_len,
                            const uint8_t* key_valid, int64_t kv_stride, int64_t n_seq, int64_t max_len, int64_t H,
                            int64_t dh, float scale, const pfpp_planes* out_planes, pfpp_stream_t stream);
int pfpp_attn_dense_bwd_p(const float* qkv, const float* out, const float* dout, const float* lse, float* dvec,
                          float* dqkv, const int32_t* seq_off, const int32_t* seq_len, const uint8_t* key_valid,
                          int64_t kv_stride, int64_t n_seq, int64_t max_len, int64_t H, int64_t dh, float scale,
                          const pfpp_planes* dqkv_planes, pfpp_stream_t stream);
int pfpp_attn_blockdiag_bwd_p(const float* qkv, const float* dout, float* dqkv, int64_t n_frag, int64_t L, int64_t H,
                              int64_t dh, float scale, const pfpp_planes* dqkv_planes, pfpp_stream_t stream);

/* ---- GEMM on pre-split fp16 planes, all three products of a Linear layer ----------------------------------
 * The PFPP_GEMM_F16X3 contraction (see pfpp_gemm) with BOTH operands given as hi/lo fp16 planes, staged by LDS-DMA:
 *   forward   y  = x . W^T   (diffusers Attention to_q/to_k/to_v/to_out, FeedForward net.0.proj / net.2:
 *                             denoiser/model/modules/attention.py:46-72; TransformerEncoderLayer linears,
 *                             verifier_transformer.py:28-37):          A = x [M,K] row-major, W [N,K] row-major
 *   dX = dY . W   (autograd of the same layers in Denoiser.training_step, denoiser.py:128-145):
 *                             A = dY [M,K=out] row-major, W [K=out, N=in] k-major (w_kmajor = 1: the weight as stored)
 *   dW = dY^T . X                                             A = dY [K=rows, M=out] k-major, W = X [K=rows, N=in] k-major
 * k-major operands are read in place (no transposed copies).  K % 32 == 0, except for dW (both operands k-major),
 * where the contraction may have any length (rows beyond K are never read).  C [M, ldc] fp32 = act(alpha * A.W + bias) + residual, or with accumulate:
 * C += alpha * A.W (+ bias + residual once).  A K split (splits > 1) goes through the workspace `ws` when one is lent
 * (dense per-chunk slabs + a reduction launch, deterministic) and through fp32 atomics otherwise (accumulate only).
 * splits = 0 / variant = 0: chosen by the library.  Results of the non-accumulating form are bit-identical to
 * pfpp_gemm(PFPP_GEMM_F16X3) on the same planes.                                                               */
/* a K split's second pass, handed back instead of launched (pfpp_gemm_planes_args.defer): the slabs of `splits` chunks wait in ws
 * (and the partial column sums in csum_ws); pfpp_slab_reduce_group adds up to PFPP_SLAB_GROUP_MAX of them in ONE launch — the six weight
 * gradients of a transformer block leave one reduction behind instead of six.  splits == 0: the GEMM wrote C itself, nothing to do. */
#define PFPP_SLAB_GROUP_MAX 8
typedef struct pfpp_slab_job {
  const float* ws; float* C; const float* csum_ws; float* csum;
  int32_t M, N; int64_t ldc; int32_t splits, accumulate;
} pfpp_slab_job;
/* C (+)= sum over the chunks, chunk order (bit-identical to the reduction pfpp_gemm_planes launches itself); jobs with splits == 0 skipped */
int pfpp_slab_reduce_group(const pfpp_slab_job* jobs, int32_t n_jobs, pfpp_stream_t stream);

typedef struct pfpp_gemm_planes_args {
  const void* a_hi; const void* a_lo;   /* fp16 planes of A */
  const void* w_hi; const void* w_lo;   /* fp16 planes of W */
  float* C;
  const float* bias;                    /* [N] or NULL */
  const float* residual;                /* [M, ldr] or NULL */
  int64_t M, N, K;                      /* output rows / columns, contraction length */
  int64_t lda, ldw, ldc, ldr;           /* plane leading dimensions in halfs, C / residual in floats */
  int32_t a_kmajor, w_kmajor;
  int32_t act;                          /* PFPP_ACT_NONE / RELU / SILU / GELU */
  int32_t accumulate;
  int32_t splits, variant;
  float alpha;
  int32_t single_pass;                  /* 1: PFPP_GEMM_F16 arithmetic (hi planes only); forward layout only */
  float* ws; int64_t ws_bytes;          /* optional K-split workspace (>= splits * M * N floats): chunks write dense slabs, a second
                                           launch adds them in chunk order (deterministic); without it a K split uses atomics   */
  float* colsum; float colsum_alpha;    /* dW form only (both operands k-major): colsum[m] += colsum_alpha * sum_k A[k][m], i.e. the bias
                                           gradient sum over rows of dY (nn.Linear backward) computed from the fragments the GEMM reads
                                           anyway; with a workspace K split it needs room for splits * M more floats             */
  pfpp_slab_job* defer;                 /* NULL, or (no bias / residual / activation): a workspace K split leaves its reduction in *defer for
                                           pfpp_slab_reduce_group; ws must stay untouched until that runs                        */
} pfpp_gemm_planes_args;

int pfpp_gemm_planes(const pfpp_gemm_planes_args* args, pfpp_stream_t stream);

/* ---- the weight gradients of one transformer block in ONE launch ------------------------------------------------
 * dW_j += dY_j^T . X_j and db_j += colsum(dY_j) for up to PFPP_DW_GROUP_MAX Linear layers whose backward shares the contraction (the
 * K token rows of the step): autograd of to_q/k/v, to_out.0, ff.net.0.proj, ff.net.2 of one EncoderLayer
 * (denoiser/model/modules/attention.py:46-72, 77-90) in Denoiser.training_step (denoiser.py:128-145).  dy [K, M = out] and x [K, N = in]
 * are k-major fp16 planes read in place (leading dimensions M and N; scales folded out: gw += dY^T.X / (dy.scale * x.scale),
 * gb += colsum(dY) / dy.scale; gb may be NULL).  Every output tile runs the whole contraction in one accumulator chain (no K split,
 * no workspace, no reduction launch; deterministic); the problems' tiles are dealt to the XCDs as one concatenated list.
 * variant: 0 = the library's choice (= 2: 256 x 128 tiles, 160 workgroups for a block's six problems); alternatives:
 * 3 = 128 x 128 tiles, 6 / 7 = 128 x 64 (three / two stages).
 * A job with an update block (upd != NULL) does not touch gw at all: a tile that has walked the whole contraction holds the FINAL
 * gradient of its weights, g = acc * (1 / (dy.scale * x.scale)) — bit for bit what the plain job stores into a ZEROED gw — and applies
 * pfpp_adamw_guarded's update (zero_grad: there is nothing to clear) to the matching elements of p, m, v, hi, lo [M, N] in its
 * epilogue: same element function (csrc/adamw_element.h), same non-finite test (the element keeps p, m, v and its planes, the flag is
 * raised and the count grows by one).  Valid where the gradient has this one producer and the update is its one consumer, which
 * would zero it: the caller's invariant (pfpp_tlayers_bwd: opt_fused_dw).  gb is accumulated as ever.  The hyper-parameters and the
 * flag belong to the launch: every update block of a call must carry the same ones.  */
#define PFPP_DW_GROUP_MAX 8
typedef struct pfpp_dw_update {
  float *p, *m, *v;    /* [M, N] fp32: parameter, first and second moment */
  void *hi, *lo;       /* [M, N] split-f16 planes of p (both or neither) */
  float lr, beta1, beta2, eps, weight_decay, bc1, bc2, g_scale;      /* as pfpp_adamw_guarded takes them */
  int32_t* overflow;   /* int32[2] or NULL (no guard) */
} pfpp_dw_update;
typedef struct pfpp_dw_job {
  pfpp_planes dy;      /* [K, M] */
  pfpp_planes x;       /* [K, N] */
  float* gw;           /* [M, N] fp32, accumulated in place (with upd: neither read nor written; may be NULL) */
  float* gb;           /* [M] fp32 or NULL */
  int64_t M, N;
  const pfpp_dw_update* upd;   /* NULL: accumulate into gw */
} pfpp_dw_job;
int pfpp_gemm_dw_group(const pfpp_dw_job* jobs, int32_t n_jobs, int64_t K, int32_t variant, pfpp_stream_t stream);
/* name of the kernel instantiation the calling thread's last pfpp_gemm, pfpp_gemm_planes, pfpp_gemm_dw_group, pfpp_gemm_grad or
 * pfpp_gemm_grad_group call launched ("" after a pfpp_gemm call that launched nothing; "+pl_reduce_kernel" appended where a slab
 * reduction followed): lets a profiler-side tool attribute event timings to kernel names.  gemm_pl_kernel's eighth field is a
 * constant 0 (a template parameter that no longer exists; the positions of the others are kept).  pfpp_sa_train_stage and the
 * attention entry points (pfpp_attn_dense*, pfpp_attn_blockdiag*) report here too: several launches of one call joined with '+' in
 * launch order, "" after a refused call.  So do pfpp_gemm_wd / _f16 and pfpp_gemm_small / _v (the calls a sequencer such as
 * pfpp_tlayers_eval makes included: after it, the name is that of its last such GEMM) */
const char* pfpp_last_gemm_kernel(void);

/* ---- a4 + a5 + a6 fused, for a set-abstraction level without input features ---------------------------
 * PointNetSetAbstraction.forward with points = None (utils/pn2_utils.py:197-217; sa1 of PN2,
 * vqvae/model/modules/pn2.py:16): sample_and_group's centred neighbourhoods (:127-151), three
 * [1x1 conv -> BatchNorm2d (eval: folded into scale s_i / shift t_i, see pfpp_gemm) -> ReLU] and torch.max over
 * nsample (:216), in one kernel: out [F*S, C3].  idx = the ball-query result [F,S,ns]; w*_hi / w*_lo = pre-split
 * fp16 planes of the folded weights [C1, 8] (K = 3 + a zero, padded to 8), [C2, C1], [C3, C2].
 * Same arithmetic as pfpp_group_gather + 3 x pfpp_gemm(PFPP_GEMM_F16X3).  ns == 32, (C1, C2, C3) == (64, 64, 128). */
int pfpp_sa_mlp3_fused(const float* xyz, const float* new_xyz, const int32_t* idx,
                       const void* w0_hi, const void* w0_lo, const void* w1_hi, const void* w1_lo,
                       const void* w2_hi, const void* w2_lo, const float* s0, const float* t0, const float* s1,
                       const float* t1, const float* s2, const float* t2, float* out, int64_t F, int64_t N,
                       int64_t S, int64_t ns, int64_t C1, int64_t C2, int64_t C3, pfpp_stream_t stream);

/* Same for a level WITH input features (sa2 of PN2, pn2.py:17): grouping (pn2_utils.py:127-151, rows
 * [feats[f, idx] (D) | xyz[f, idx] - new_xyz (3)]) and the FIRST TWO [1x1 conv -> BatchNorm2d(eval, folded) -> ReLU]
 * (:210-213) in one kernel: out [F*S*ns, C2] = the input of the level's third convolution (then pfpp_gemm with
 * pool = ns).  w0 planes [C1, D + 8] in the column order of pfpp_group_gather (features first), w1 planes [C2, C1].
 * ns == 64, D == C1 == C2 == 128. */
int pfpp_sa_mlp2_fused(const float* feats, const float* xyz, const float* new_xyz, const int32_t* idx,
                       const void* w0_hi, const void* w0_lo, const void* w1_hi, const void* w1_lo,
                       const float* s0, const float* t0, const float* s1, const float* t1, float* out,
                       int64_t F, int64_t N, int64_t S, int64_t ns, int64_t D, int64_t C1, int64_t C2,
                       pfpp_stream_t stream);
/* the same with the result (also / only) as split-f16 planes of scale 1 — the A operand of the third convolution's plane GEMM
 * (csrc/gemm_pl.hip) with no conversion pass; `out` may then be NULL */
int pfpp_sa_mlp2_fused_p(const float* feats, const float* xyz, const float* new_xyz, const int32_t* idx,
                         const void* w0_hi, const void* w0_lo, const void* w1_hi, const void* w1_lo,
                         const float* s0, const float* t0, const float* s1, const float* t1, float* out,
                         const pfpp_planes* out_planes, int64_t F, int64_t N, int64_t S, int64_t ns, int64_t D, int64_t C1,
                         int64_t C2, pfpp_stream_t stream);
/* The same level with its FIRST convolution taken per point instead of per grouped row (it is linear): u [F*N, C1] = [feats | xyz] .
 * W1^T without bias (pfpp_gemm's fused grouping with the identity index and zero centroids; the folded shift t0 carries the bias), and
 * the value on the grouped row (s, p) is u[p] - W1_xyz . new_xyz[s].  out = the planes pfpp_sa_mlp2_fused_p writes, within fp32 rounding
 * of W1_xyz . (x - c) against W1_xyz . x - W1_xyz . c; 42 GFLOP of grouped first-layer work at F = 154 are not computed.
 * w0 planes are read for their three xyz columns only.  max_workgroups: 0 or the CU count the stream may use. */
int pfpp_sa_mlp2_table_p(const float* u, const float* new_xyz, const int32_t* idx, const void* w0_hi, const void* w0_lo,
                         const void* w1_hi, const void* w1_lo, const float* s0, const float* t0, const float* s1, const float* t1,
                         const pfpp_planes* out, int64_t F, int64_t N, int64_t S, int64_t ns, int64_t D, int64_t C1, int64_t C2,
                         int64_t max_workgroups, pfpp_stream_t stream);
/* First layer alone, for the levels whose second layer is a plane GEMM (sa3 in eval mode): out = relu(s0 * (u[idx] - W1_xyz . new_xyz) + t0)
 * as split-f16 planes [F*S*ns, C1] — what pfpp_gemm's fused grouping with the folded BatchNorm epilogue writes, as an elementwise pass over
 * the per-point table (no matrix work on the F*S*ns grouped rows).  ns == 64; (D, C1) = (256, 256) or (128, 128). */
int pfpp_sa_table_planes(const float* u, const float* new_xyz, const int32_t* idx, const void* w0_hi, const void* w0_lo,
                         const float* s0, const float* t0, const pfpp_planes* out, int64_t F, int64_t N, int64_t S, int64_t ns,
                         int64_t D, int64_t C1, pfpp_stream_t stream);

/* ---- a5 in TRAIN mode (the frozen encoder stays in .train(): train_denoiser.py:33-35, utils/pn2_utils.py:203-216 with
 * BatchNorm2d on BATCH statistics) without writing the layers' activations: one launch per layer ("stage") of the chain.
 * Stage k recomputes the chain from the level's input (grouping by ball-query index included, pn2_utils.py:127-151) through
 * layers 1..k-1 — normalised with their already finalised statistics: relu(fma(conv + bias, a_mul, a_add)), the (a_mul, a_add)
 * of pfpp_bn_finalize — and accumulates sum(y_k), sum(y_k^2) of the raw layer-k output y_k = conv + bias into `stats`
 * ([stats_copies][2][C_k] doubles, the buffer pfpp_bn_finalize reads and clears).
 *   feats == NULL (sa1, pn2.py:16): ns == 32, (C1, C2, C3) == (64, 64, 128), stages 1..3; stage 3 also writes the
 *     per-neighbourhood max and min of y_3 (out_max, out_min [F*S, C3]; then pfpp_bn_minmax_apply).
 *   feats != NULL (sa2, pn2.py:17): ns == 64, D == C1 == C2 == 128, C3 == 256, stages 1..3; stage 2 also writes the raw rows
 *     y_2 (y_out [F*S*ns, C2]: the third layer's weights do not fit in LDS next to the others); stage 3 READS y_out, applies
 *     relu(fma(y_2, a_mul[1], a_add[1])), runs the third convolution with its weight planes resident in LDS and writes the sums
 *     of y_3 and out_max / out_min [F*S, C3] (only w_hi[2] / w_lo[2] / bias[2] / a_mul[1] / a_add[1] are read).
 *   feats != NULL with D == 256 (sa3, pn2.py:18): ns == 64, widths 256 / 256 / 512.  No two of its weight matrices fit in LDS together,
 *     so every stage is ONE layer: stage 1 gathers and writes the raw rows y_1 (y_out [F*S*ns, 256]), stage 2 reads them (y_in),
 *     normalises with a_mul[0] / a_add[0] and writes y_2 (y_out), stage 3 reads y_2 (y_in, a_mul[1] / a_add[1]) and writes the sums and
 *     out_max / out_min [F*S, 512]; a workgroup keeps a 128-column slice of the layer's weight planes in LDS.
 * Weight planes as for pfpp_sa_mlp3_fused / pfpp_sa_mlp2_fused (raw conv weights, BatchNorm NOT folded).
 * max_workgroups: persistent grid size (0 = 256, one workgroup per CU; pass the CU count of a CU-masked stream). */
typedef struct pfpp_sa_train_args {
  const float* xyz;            /* [F, N, 3] */
  const float* new_xyz;        /* [F, S, 3] */
  const float* feats;          /* [F, N, D] or NULL */
  const int32_t* idx;          /* [F, S, ns] */
  const void* w_hi[3];         /* fp16 planes of the conv weights, layers 1..3 (those beyond `stage` may be NULL) */
  const void* w_lo[3];
  const float* bias[3];        /* conv biases */
  const float* a_mul[2];       /* finalised BatchNorm affine of layers 1, 2 (needed for layers < stage) */
  const float* a_add[2];
  double* stats;               /* [stats_copies][2][C_stage] */
  int64_t stats_copies;
  float* y_out;                /* feats != NULL: written by stage 2, read by stage 3 (D == 256: written by stages 1 and 2) */
  const float* y_in;           /* D == 256 only: the raw rows of the previous layer (stages 2 and 3) */
  const float* u_in;           /* optional, levels with features: U [F*N, C1] = the first conv applied PER POINT ([feats | xyz] . W1^T + b1,
                                  i.e. pfpp_gemm's fused grouping with the identity index and zero centroids).  conv1 is linear, so on a
                                  grouped row it equals U[idx] - W1_xyz . centroid: with u_in stage 1 only takes the statistics of that
                                  (no matrix work) and stage 2 gathers its input rows from U (writes y_out [F*S*ns, C2]); stage 3 is
                                  unchanged */
  float* out_max;              /* stage 3 */
  float* out_min;
  int64_t F, N, S, ns, D, C1, C2, C3;
  int32_t stage;
  int64_t max_workgroups;
  const int32_t* sched;        /* optional, ns == 64: pfpp_sa_pad_schedule(idx).  A neighbourhood with at most 32 points in range is taken as
                                  ONE half of 32 rows (its rows 32..63 are copies of row 0: 32 y_0 and 32 y_0^2 to the sums, nothing to max /
                                  min).  Of the raw second-layer rows stage 2 writes and stage 3 reads the LIVE ones only (slots below the
                                  neighbourhood's count; a copy is read as row 0), so the stages of one level must all get the schedule or
                                  none.  Table-fed stages 1-2 (u_in), stage 3 of both levels */
} pfpp_sa_train_args;
int pfpp_sa_train_stage(const pfpp_sa_train_args* args, pfpp_stream_t stream);

/* Padding schedule of a 64-neighbour level for pfpp_sa_train_args.sched.  query_ball_point (utils/pn2_utils.py:103-123) sorts the in-range
 * point indices ascending and fills the remaining nsample slots with the first one: slots cnt .. 63 repeat slot 0.  cnt = 1 + the highest
 * slot that differs from slot 0 is found slot by slot, so the schedule is exact for any index list.
 * sched [3 G + 1] int32: [0, G) the neighbourhoods with cnt > 32 (two live halves; ascending), then those with one; [G] the number of the
 * former; [G + 1, 2 G + 1) cnt by neighbourhood; [2 G + 1, 3 G + 1) cnt in schedule order.  idx [G, 64].  Two small launches per level. */
int pfpp_sa_pad_schedule(const int32_t* idx, int64_t G, int64_t ns, int32_t* sched, pfpp_stream_t stream);


/* ---- a7/a8: vector quantisation + scatter ----------------------------------
 * VectorQuantizer.forward, vqvae/model/modules/quantizer.py:26-71 as used by
 * VQVAE.encode (denoiser/model/modules/encoder.py:20-38): for every
 * `dim`-wide sub-vector z: d_j = (|z|^2 + |e_j|^2) - 2*(z.e_j), first argmin,
 * out = z + (e_j - z) (straight-through value, quantizer.py:63).  Results are
 * scattered straight into the zero-initialised padded tensor at row
 * slot[f] (denoiser.py:72-76): z_e [F, rows_per_frag, dim] ->
 * z_q [n_slots, rows_per_frag, dim]; codes [F, rows_per_frag] (may be NULL).
 * dim == 16, n_codes <= 1024.                                               */
int pfpp_vq_encode(const float* z_e, const float* codebook, const int32_t* slot,
                   float* z_q, int32_t* codes, int64_t F, int64_t rows_per_frag,
                   int64_t dim, int64_t n_codes, pfpp_stream_t stream);

/* scatter rows: out[slot[f], :] = in[f, :]  (xyz scatter, denoiser.py:76)   */
int pfpp_scatter_rows(const float* in, const int32_t* slot, float* out,
                      int64_t F, int64_t row_elems, pfpp_stream_t stream);

/* ---- a9: token features ---------------------------------------------------
 * DenoiserTransformer._gen_cond, denoiser_transformer.py:117-135 with
 * EmbedderNerf.embed utils/model_utils.py:68-69 (include_input, 10 log-spaced
 * frequencies 2^0..2^9, [sin, cos] per frequency):
 *   shape_feat[(bp,l), :] = [latent(64) | PE(xyz)(63) | PE(scale)(21) | 0-pad]
 *   pose_feat[bp, :]      = [PE(x)(147) | 0-pad]
 *   latent [n, L, 64], xyz [n, L, 3], scale [n], x [n, 7];  ld = 148.       */
int pfpp_token_features(const float* latent, const float* xyz, const float* scale,
                        const float* x, float* shape_feat, float* pose_feat,
                        int64_t n, int64_t L, pfpp_stream_t stream);

/* token assembly, denoiser_transformer.py:150-156,173-185 + PositionalEncoding
 * utils/model_utils.py:18-21:
 *   tok[(b,p,l), :] = shape_emb[(b,p,l), :] + x_emb[(b,p), :]
 *                     + ref_emb[ref[b,p] ? 1 : 0, :] + pe[p, :]              */
int pfpp_token_combine(const float* shape_emb, const float* x_emb,
                       const float* ref_emb, const uint8_t* ref_part,
                       const float* pe, float* tok, int64_t B, int64_t P,
                       int64_t L, int64_t C, pfpp_stream_t stream);
/* pfpp_token_features / pfpp_token_combine_list / pfpp_token_combine_bwd for a compacted fragment list that is still stored at its
 * padded slots: listed fragment f is read from row slot[f] of latent [n_slots, L, 64], xyz, scale, x and ref_part [n_slots] — the
 * valid-fragment gather of DenoiserTransformer.forward's inputs (denoiser.py:66-77) without the five gathered copies */
int pfpp_token_features_slots(const float* latent, const float* xyz, const float* scale, const float* x,
                              const int32_t* slot, float* shape_feat, float* pose_feat, int64_t n, int64_t L,
                              pfpp_stream_t stream);
int pfpp_token_combine_slots(const float* shape_emb, const float* x_emb, const float* ref_emb,
                             const uint8_t* ref_part, const float* pe, const int32_t* frag_pos, const int32_t* slot,
                             float* tok, int64_t n, int64_t L, int64_t C, pfpp_stream_t stream);
int pfpp_token_combine_bwd_slots(const float* dtok, const uint8_t* ref_part, const int32_t* slot, float* dx_emb,
                                 float* dref_emb, int64_t n, int64_t L, int64_t C, pfpp_stream_t stream);
/* same for a compacted fragment list (padded slots dropped): n fragments, frag_pos[f] = p (row of pe) */
int pfpp_token_combine_list(const float* shape_emb, const float* x_emb,
                            const float* ref_emb, const uint8_t* ref_part,
                            const float* pe, const int32_t* frag_pos, float* tok,
                            int64_t n, int64_t L, int64_t C, pfpp_stream_t stream);

/* ---- a11: AdaLN ---------------------------------------------------------------
 * MyAdaLayerNorm, denoiser/model/modules/attention.py:21-25.
 * pfpp_silu_embed: out[i, b, :] = silu(tables[i][t[b], :]) for the n_tab
 * embedding tables (one per norm); tables [n_tab, n_emb, C] is a packed copy.
 * pfpp_layernorm: y = LN(x) (eps, biased variance, no affine) then
 *   mod != NULL : y*(1+mod[b, 0:C]) + mod[b, C:2C]   (b = row / rows_per_batch)
 *   gamma != NULL : y*gamma + beta                   (norm3 / verifier norms)
 * x may alias y.                                                              */
int pfpp_silu_embed(const float* tables, const int64_t* t, float* out,
                    int64_t n_tab, int64_t n_emb, int64_t B, int64_t C,
                    pfpp_stream_t stream);
int pfpp_layernorm(const float* x, float* y, const float* mod, int64_t ld_mod,
                   const float* gamma, const float* beta, int64_t rows,
                   int64_t C, int64_t rows_per_batch, float eps,
                   pfpp_stream_t stream);
/* batch of a row given by an explicit per-group map instead of row / rows_per_batch:
 * b = group_batch[row / group_rows]  (compacted fragment lists: group = fragment, group_rows = L) */
int pfpp_layernorm_grouped(const float* x, float* y, const float* mod, int64_t ld_mod,
                           const int32_t* group_batch, int64_t group_rows, int64_t rows,
                           int64_t C, float eps, pfpp_stream_t stream);
/* same, but the result is written as split-f16 planes (hi, lo) for the PFPP_GEMM_F16X3 path */
int pfpp_layernorm_split(const float* x, void* y_hi, void* y_lo, const float* mod, int64_t ld_mod,
                         const float* gamma, const float* beta, int64_t rows,
                         int64_t C, int64_t rows_per_batch, float eps,
                         pfpp_stream_t stream);
/* pfpp_layernorm_grouped with the normalised rows written as split-f16 planes (input of the next GEMM) */
int pfpp_layernorm_grouped_split(const float* x, void* y_hi, void* y_lo, const float* mod, int64_t ld_mod,
                                 const int32_t* group_batch, int64_t group_rows, int64_t rows, int64_t C,
                                 float eps, pfpp_stream_t stream);

/* ---- a10/a12: block-diagonal self-attention --------------------------------
 * EncoderLayer self-attn (attention.py:77-80) with the block-diagonal mask of
 * DenoiserTransformer._gen_mask (denoiser_transformer.py:158-162): every
 * fragment's L tokens attend only to each other, so the [B,T,T] mask is never
 * built.  qkv [n_frag*L, 3*H*dh] (q | k | v), out [n_frag*L, H*dh];
 * softmax(q.k^T * scale).  L <= 32, dh == 64.                               */
int pfpp_attn_blockdiag(const float* qkv, float* out, int64_t n_frag, int64_t L,
                        int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
/* out_hi/out_lo != NULL: additionally/instead write split-f16 planes (out may then be NULL) */
int pfpp_attn_blockdiag_split(const float* qkv, void* out_hi, void* out_lo, int64_t n_frag, int64_t L,
                              int64_t H, int64_t dh, float scale, pfpp_stream_t stream);

/* ---- a13/a18: masked row softmax for the dense attentions -------------------
 * S [rows_total, ld] in place: p = softmax(S[r, 0:T] * scale) over the keys j
 * with key_valid[batch(r), j] != 0 (batch(r) = r / rows_per_batch); masked
 * keys and the pad columns [T, ld) get exactly 0.  key_valid [n_batch, T]
 * (uint8): gen_mask of denoiser_transformer.py:163-164 / src_key_padding_mask
 * of verifier_transformer.py:62.                                             */
int pfpp_softmax_rows(float* S, const uint8_t* key_valid, int64_t rows_total,
                      int64_t rows_per_batch, int64_t T, int64_t ld, float scale,
                      pfpp_stream_t stream);

/* ---- a13/a18: fused dense masked attention ------------------------------------------------------
 * softmax(Q K^T * scale + key mask) V per (sequence, head) straight from a packed projection
 * qkv [rows, 3*H*dh] (q | k | v): EncoderLayer global attention (attention.py:82-85 with gen_mask of
 * denoiser_transformer.py:163-164) and the verifier's self-attention (verifier_transformer.py:62,
 * src_key_padding_mask).  Scores stay in registers (online softmax); exact fp32 MFMA products.
 * Sequence s occupies rows [seq_off[s], seq_off[s] + seq_len[s]); key_valid (may be NULL) is
 * [n_seq, kv_stride] uint8 with 0 = key masked out.  out [rows, H*dh].  dh in {32, 64}.         */
int pfpp_attn_dense(const float* qkv, float* out, const int32_t* seq_off, const int32_t* seq_len,
                    const uint8_t* key_valid, int64_t kv_stride, int64_t n_seq, int64_t max_len,
                    int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
int pfpp_attn_dense_split(const float* qkv, void* out_hi, void* out_lo, const int32_t* seq_off,
                          const int32_t* seq_len, const uint8_t* key_valid, int64_t kv_stride,
                          int64_t n_seq, int64_t max_len, int64_t H, int64_t dh, float scale,
                          pfpp_stream_t stream);

/* ---- a15: mean pool over the L tokens of a fragment -----------------------
 * denoiser_transformer.py:139-142.  x [n*L, C] -> out [n, C]                 */
int pfpp_mean_pool(const float* x, float* out, int64_t n, int64_t L, int64_t C,
                   pfpp_stream_t stream);

/* ---- a16: DDPM ancestral step + reference-part re-pin ----------------------
 * diffusers-0.21.4 DDPMScheduler.step as configured by PiecewiseScheduler
 * (denoiser/model/modules/custom_diffusers.py:60-69) followed by
 * `x[ref_part] = reference[ref_part]` (denoiser.py:184-185, auto_aggl.py:149-150)
 *   x0 = (x - c_eps*eps)/c_div;  out = c_x0*x0 + c_x*x (+ c_noise*noise)
 * coefficients are computed on the host in fp32 in the scheduler's op order;
 * noise may be NULL (t == 0).  All tensors [n, 7]; ref_part [n] uint8 or NULL */
int pfpp_ddpm_step(const float* x, const float* eps, const float* noise,
                   const uint8_t* ref_part, const float* reference, float* out,
                   int64_t n, float c_eps, float c_div, float c_x0, float c_x,
                   float c_noise, pfpp_stream_t stream);

/* add_noise (denoiser.py:92): out = sa[b]*x0 + sb[b]*noise, per-puzzle scalars */
int pfpp_add_noise(const float* x0, const float* noise, const float* sqrt_ab,
                   const float* sqrt_1mab, float* out, int64_t B,
                   int64_t per_batch, pfpp_stream_t stream);

/* ---- a18: verifier token embedding ------------------------------------------
 * verifier_transformer.py:52-56: tok = feat_emb[(b,e), :] + [pe[i0] | pe[i1]]
 * feat_emb [n, C] (output of the 7->C GEMM), edge_idx [n, 2] int64,
 * pe [max_len, C/2].                                                         */
int pfpp_verifier_embed(const float* feat_emb, const int64_t* edge_idx,
                        const float* pe, float* tok, int64_t n, int64_t C,
                        int64_t max_len, pfpp_stream_t stream);

/* ---- a19: pose composition ---------------------------------------------------
 * utils/node_merge_utils.py:275-306 get_param / :246-272
 * extract_final_pred_trans_rots: M = [R(q[pivot[i]]) | t[pivot[i]]], optionally
 * M <- M @ init_pose[i] (has_init[i] != 0), then (t, matrix_to_quaternion(R)).
 * pose [P,7], pivot [n] int32, init_pose [n,16] row-major 4x4, out [n,7].
 * quaternion_to_matrix / matrix_to_quaternion follow pytorch3d.  */
int pfpp_pose_compose(const float* pose, const int32_t* pivot,
                      const float* init_pose, const uint8_t* has_init,
                      float* out, int64_t n, pfpp_stream_t stream);

/* ---- 8f-1: verifier edge features -----------------------------------------------------------------
 * pfpp_pose_apply_points: body of get_final_pose_pts_dynamic (utils/node_merge_utils.py:16-41): a flat
 * list of points, point i is moved by pose[pose_idx[i]] = (t, q): quaternion_apply (normalise = 0 there)
 * then + t.
 * pfpp_edge_histogram: get_distance_for_matching_pts (:62-89) + _make_cd_to_bins (auto_aggl.py:385-389):
 * edge e owns the matched pairs [edge_off[e], edge_off[e+1]) of (idx_a, idx_b) (indices into pts);
 * d_i = min_j |a_i-b_j|^2 + min_j |b_i-a_j|^2 is counted into the 6 bins
 * [0,1e-3) [1e-3,5e-3) [5e-3,1e-2) [1e-2,5e-2) [5e-2,1e-1) [1e-1,100) -> hist [n_edges, 6] int32.  */
int pfpp_pose_apply_points(const float* pts, const int32_t* pose_idx, const float* pose, float* out,
                           int64_t n, int normalise, pfpp_stream_t stream);
int pfpp_edge_histogram(const float* pts, const int32_t* idx_a, const int32_t* idx_b,
                        const int32_t* edge_off, int32_t* hist, int64_t n_edges, int64_t max_m,
                        pfpp_stream_t stream);
/* pfpp_edge_features_batch: the verifier input of several puzzles of a pfpp_match_edges batch in one launch:
 * get_distance_for_matching_pts (utils/node_merge_utils.py:62-89), _make_cd_to_bins (auto_aggl.py:385-389), the scatter
 * into the upper triangle and the normalisation (auto_aggl.py:193-201).  T = P (P - 1) / 2 slots per puzzle.
 * pts [total_points, 3] = the transformed by-area points of the whole batch, puzzle b from point pt_off[b] (int64 [B]);
 * idx_a, idx_b (point indices within the puzzle), row_off int64 [B + 1] and edge_off int32 [B, T + 1] exactly as
 * pfpp_match_edges takes and writes them (a slot's rows are row_off[b] + [edge_off[b, s], edge_off[b, s + 1])); puz int32 [nb] =
 * the puzzles of this call, each in [0, B), in any order; out float32 [nb, T, 7].
 * Per (puzzle, slot): pfpp_edge_histogram's six counts h (the same device function: (dx dx + dy dy) + dz dz, fminf, fa + fb,
 * the same thresholds, d >= 100 dropped), then out = (h / max(sum h, 1) in fp32, sum h): bit for bit what the per-puzzle route
 * (pfpp_edge_histogram, index_put by triangle position, normalise_edge_hist) gives.  A slot without rows is seven zeros; every
 * slot of every listed puzzle is written.  No float atomics: the result depends neither on the grid nor on the other puzzles of
 * the call.  An entry of puz outside [0, B), or a slot with more than max_m rows, is written as zeros and reads nothing.
 * PFPP_EUNSUPPORTED before any launch for P > 32, max_m > 6000 or more than 65535 puzzles; nb = 0 does nothing.  */
int pfpp_edge_features_batch(const float* pts, const int64_t* pt_off, const int32_t* idx_a, const int32_t* idx_b,
                             const int64_t* row_off, const int32_t* edge_off, const int32_t* puz, float* out,
                             int64_t nb, int64_t B, int64_t P, int64_t max_m, pfpp_stream_t stream);

/* ---- 8f-4: GPU-side augmentation of GeometryLatentDataset.__getitem__ (denoiser/dataset/dataset.py:165-215) ---
 * For a batch of stored puzzles part_pcs_gt [B,P,N,3] (assembled frame, padded): rotate the whole assembly by
 * R(q_global)^T, recentre on the reference part, then per part recentre + rotate by R(q_part)^T and divide by
 * the max-abs coordinate.  q_global [B,4] / q_part [B,P,4] are the quaternions the dataset stores (pose_gt_r /
 * part_rots, scalar first).  Outputs: part_pcs [B,P,N,3], part_trans [B,P,3], part_scale [B,P], init_pose_t [B,3];
 * padded slots (p >= num_parts[b]) get zeros and scale 1.  float64 means/rotations like the numpy original.
 * workspace: pfpp_fragment_prepare_workspace(B, P) bytes.  N <= 2048.                                       */
int64_t pfpp_fragment_prepare_workspace(int64_t B, int64_t P);
int pfpp_fragment_prepare(const float* part_pcs_gt, const int32_t* num_parts, const int32_t* ref_idx,
                          const float* q_global, const float* q_part, float* part_pcs, float* part_trans,
                          float* part_scale, float* init_pose_t, int64_t B, int64_t P, int64_t N,
                          void* workspace, pfpp_stream_t stream);

/* ---- the test split's initial frames for a group of puzzles (denoiser/dataset/dataset.py:86-109 behind :165-215) ----
 * pfpp_test_frames = pfpp_fragment_prepare (the same two kernels: part_pcs, part_trans, part_scale and init_pose_t are bit for
 * bit what it writes for the same inputs) and then the by-area points of the assembled shapes taken into every piece's
 * initial frame (_anchor_coords, _move_to_init_pose). by_area float32 [M, 3] = gt_pc_by_area of the B puzzles concatenated,
 * pt_off int64 [B+1] (pt_off[B] = M), n_pcs int32 [B, P] = by-area points per piece slot, by_area_out float32 [M, 3].
 * For point x of piece p of puzzle b, in float64:
 *     a = R(q_global[b])^T x - c_ref[b];   c = a - (double)(float) t[b, p];   y = R(q_part[b, p])^T c, stored as float32
 * with c_ref (= init_pose_t) and t (= part_trans; rounded to float32 first, as the host subtracts the float32 cur_trans) from
 * the fp64 centroid workspace through the device function frag_prepare_kernel uses, and both quaternions normalised as
 * there.  A point's piece is the first p with i < n_pcs[b, 0] + .. + n_pcs[b, p].  A point past sum n_pcs[b], in a slot
 * p >= num_parts[b], or of a puzzle whose ref_idx is no slot is written as zeros and not read; offsets are clamped to [0, M]
 * (memory safety only: pfpp_hip.augment.test_frames_batch refuses such input).  No atomics: a puzzle's result depends neither
 * on the grid nor on the other puzzles of the call.  workspace: pfpp_fragment_prepare_workspace(B, P) bytes.
 * PFPP_EUNSUPPORTED before any launch for N > 2048, B > 65535, P > 32 or M >= 2^31; B = 0 does nothing.                  */
int pfpp_test_frames(const float* part_pcs_gt, const int32_t* num_parts, const int32_t* ref_idx, const float* q_global,
                     const float* q_part, float* part_pcs, float* part_trans, float* part_scale, float* init_pose_t,
                     const float* by_area, const int64_t* pt_off, const int32_t* n_pcs, float* by_area_out, int64_t B,
                     int64_t P, int64_t N, int64_t M, void* workspace, pfpp_stream_t stream);

/* ---- 8f-2: merge step of auto_aggl (utils/node_merge_utils.py:159-222) -------------------------------------
 * pfpp_estimate_normals: pytorch3d.ops.estimate_pointcloud_normals(neighborhood_size=K) per part:
 * pts [P, N, 3] -> normals [P, N, 3] (K nearest neighbours incl. the point, covariance about the
 * neighbourhood mean, eigenvector of the smallest eigenvalue, majority-side sign).  K in {10, 20, 32}.
 * pfpp_merge_keep_mask: keep[i,k] = 0 iff for some j != i  d[i,j,k] + d[j,i,k] < threshold and
 * normals[i,k].normals[j,k] < 0;  d [P,P,N] = nearest-neighbour distances part i -> part j (pfpp_nn_dist).
 * pfpp_fps_start: pfpp_fps with an explicit first index per fragment (torch_cluster.fps random_start,
 * node_merge_utils.py:219); N up to 32768.                                                              */
int pfpp_estimate_normals(const float* pts, float* normals, int64_t P, int64_t N, int64_t K,
                          pfpp_stream_t stream);
int pfpp_merge_keep_mask(const float* d, const float* normals, uint8_t* keep, int64_t P, int64_t N,
                         float threshold, pfpp_stream_t stream);
int pfpp_fps_start(const float* xyz, int32_t* idx, float* new_xyz, int64_t F, int64_t N, int64_t S,
                   const int32_t* start, pfpp_stream_t stream);

/* ---- 8f-3: evaluation metrics (denoiser/evaluation/evaluator.py, transform.py) ---------------------------
 * pfpp_nn_dist: out[b, i] = min_j |src[b,i] - dst[b,j]|^2 — the KNN-1 term of chamferdist.ChamferDistance
 * (squared L2, knn_points); calc_part_acc (evaluator.py:88-121) and calc_shape_cd (:124-153) call it in
 * both directions.  src [batch, n, 3], dst [batch, m, 3], out [batch, n].
 * pfpp_quat_to_euler_xyz: transform.quaternion_to_euler (transform.py:70-86) = pytorch3d
 * quaternion_to_matrix + matrix_to_euler_angles("XYZ"); quat [n,4] (w first) -> euler [n,3].             */
int pfpp_nn_dist(const float* src, const float* dst, float* out, int64_t batch, int64_t n, int64_t m,
                 pfpp_stream_t stream);
int pfpp_quat_to_euler_xyz(const float* quat, float* euler, int64_t n, int to_degree,
                           pfpp_stream_t stream);

/* =====================================================================================================
 * a17: training — backward of the DenoiserTransformer, loss and optimizer
 * (Denoiser.forward/_loss/training_step/configure_optimizers, denoiser/model/denoiser.py:80-145,230-241).
 * The encoder is frozen in the reference (train_denoiser.py:33-35): gradients stop at the tokens.
 * ===================================================================================================== */

/* ---- backward GEMMs (csrc/gemm_grad.hip) ----------------------------------------------------------
 *   C[M,N] (+)= alpha * sum_k A(m,k) * W(n,k)
 *   a_kmajor = 0: A(m,k) = A[m*lda + k]     a_kmajor = 1: A(m,k) = A[k*lda + m]
 *   w_kmajor = 0: W(n,k) = W[n*ldw + k]     w_kmajor = 1: W(n,k) = W[k*ldw + n]
 * dX = dY . W        : A = dY, W = the [out,in] weight with w_kmajor = 1
 * dW = dY^T . X      : A = dY (a_kmajor = 1), W = X (w_kmajor = 1), K = rows
 * split-f16 arithmetic (PFPP_GEMM_F16X3); a_scale / w_scale are powers of two applied before the
 * f16 split (gradients are tiny) and divided out of the result.  split_k = 0 picks the number of K
 * chunks; more than one chunk needs accumulate = 1 (fp32 atomics into a zero-initialised C).     */
typedef struct pfpp_gemm_grad_args {
  const float* A; const float* W; float* C;
  int64_t M, N, K;
  int64_t lda, ldw, ldc;
  int32_t a_kmajor, w_kmajor;
  int32_t accumulate;
  int32_t split_k;
  int32_t batch;
  int64_t sA, sW, sC;
  float a_scale, w_scale, alpha;
  float* colsum;        /* NULL, or (weight-gradient form: a_kmajor = 1, batch = 1) colsum[m] += sum_k A[m, k] — the bias gradient of
                           the same torch.nn.Linear (unscaled dY), accumulated with atomics from the A tiles as they are staged */
} pfpp_gemm_grad_args;
int pfpp_gemm_grad(const pfpp_gemm_grad_args* args, pfpp_stream_t stream);
/* Up to 8 independent weight-gradient problems (both operands k-major, batch 1) in ONE launch: the six dW of a transformer
 * layer (attention.py:60-90: to_q/k/v, to_out, ff.net.0.proj, ff.net.2 of the self- and global-attention blocks) each have
 * few output tiles and a contraction over all tokens; launched together they fill the chip without cutting K into many
 * atomically-accumulated chunks.  Replaces what autograd does one Linear at a time (torch.nn.Linear backward,
 * denoiser_transformer.py:79-101 layers).  split_k of each problem: 0 = chosen for the group. */
int pfpp_gemm_grad_group(const pfpp_gemm_grad_args* args, int count, pfpp_stream_t stream);

/* out[z, c] (+)= sum_r x[z, r, c]  (bias gradients).  x rows of stride ld, batches of stride sx / so */
int pfpp_colsum(const float* x, float* out, int64_t rows, int64_t cols, int64_t ld,
                int64_t batch, int64_t sx, int64_t so, int accumulate, pfpp_stream_t stream);

/* ---- counter-based dropout --------------------------------------------------------------------------
 * keep(i) = rng(seed, site, i) >= p * 2^32 ; y = x * keep / (1 - p).  The same (seed, site) gives the
 * same mask in forward and backward, so masks are never stored.  Sites of the denoiser: token dropout
 * (PositionalEncoding, utils/model_utils.py:18-21, p = 0.1), the dropout after each attention
 * out-projection and inside each FeedForward (diffusers Attention.to_out[1] / FeedForward.net[1],
 * attention.py:46-72 with dropout_rate of config/denoiser/model.yaml).
 * pfpp_dropout: out = (res ? res : 0) + x*keep/(1-p)   (x may alias out)
 * pfpp_dropout_mask: the keep mask itself as uint8 (tests, oracle)                                  */
int pfpp_dropout(const float* x, const float* res, float* out, int64_t n, float p,
                 uint64_t seed, uint32_t site, pfpp_stream_t stream);
int pfpp_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, uint32_t site,
                      pfpp_stream_t stream);

/* ---- GEGLU (diffusers FeedForward "geglu", attention.py:67-72) with its dropout, training form ------
 * z [rows, 2*inner] = proj output (value columns [0,inner), gate columns [inner, 2*inner))
 * fwd: u[r,c] = drop(z[r,c] * gelu_erf(z[r,inner+c]))
 * bwd: dz[r,c] = du' * gelu(g) ; dz[r,inner+c] = du' * v * gelu'(g) with du' = du*keep/(1-p)        */
int pfpp_geglu(const float* z, float* u, int64_t rows, int64_t inner, float p, uint64_t seed,
               uint32_t site, pfpp_stream_t stream);
int pfpp_geglu_bwd(const float* z, const float* du, float* dz, int64_t rows, int64_t inner, float p,
                   uint64_t seed, uint32_t site, pfpp_stream_t stream);

/* elementwise activation and its backward on a flat buffer (output heads: SiLU)                     */
int pfpp_act(const float* pre, float* out, int64_t n, int act, pfpp_stream_t stream);
int pfpp_act_bwd(const float* pre, const float* dy, float* dx, int64_t n, int act, pfpp_stream_t stream);

/* ---- LayerNorm backward (MyAdaLayerNorm attention.py:21-25, norm3) ----------------------------------
 * y = xhat * mult + add with  mult = 1 + mod[b, 0:C], add = mod[b, C:2C]  (mod != NULL, AdaLN)
 *                       or    mult = gamma, add = beta                    (gamma != NULL)
 *   dx[r, :]      += rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * mult
 *   dmult[b, c]   += sum_r dy * xhat       dadd[b, c] += sum_r dy      (b = 0 for the affine form)
 * batch of a row: group_batch[row / group_rows] if group_batch else row / rows_per_batch; group_rows
 * rows are handled per workgroup (rows_per_batch % group_rows == 0).  dmult/dadd rows have stride ld_d.
 * C in {256, 512}.                                                                                   */
int pfpp_layernorm_bwd(const float* x, const float* dy, const float* mod, int64_t ld_mod,
                       const float* gamma, const int32_t* group_batch, int64_t group_rows,
                       int64_t rows_per_batch, float* dx, float* dmult, float* dadd, int64_t ld_d,
                       int64_t rows, int64_t C, float eps, pfpp_stream_t stream);

/* The same with the dropout that follows each LayerNorm in the backward chain fused in (EncoderLayer's
 * dropout after the attention out-projections attention.py:46-52, PositionalEncoding's token dropout
 * model_utils.py:18-21): drop_out[r, c] = keep(seed, site, r*C + c) ? dx_new[r, c] / (1 - p) : 0 — the mask of
 * pfpp_dropout over a [rows, C] tensor, so forward and backward sites regenerate each other's masks.      */
int pfpp_layernorm_bwd_dropout(const float* x, const float* dy, const float* mod, int64_t ld_mod,
                               const float* gamma, const int32_t* group_batch, int64_t group_rows,
                               int64_t rows_per_batch, float* dx, float* dmult, float* dadd, int64_t ld_d,
                               int64_t rows, int64_t C, float eps, float* drop_out, float p, uint64_t seed,
                               uint32_t site, pfpp_stream_t stream);

/* Forward counterpart: h_out = (res or 0) + dropout(y; p, seed, site), n_out = LayerNorm(h_out) with the
 * (mod | gamma, beta | none) forms and the row -> batch mapping of pfpp_layernorm / pfpp_layernorm_grouped
 * (group_batch != NULL: batch = group_batch[row / group_rows], else row / rows_per_batch).  h_out may alias
 * y or res.  h_out has the bits of pfpp_dropout, n_out those of pfpp_layernorm up to the contraction of the
 * affine step (an ulp).  C in {256, 512}.                                                                 */
int pfpp_dropout_layernorm(const float* y, const float* res, float* h_out, float* n_out, const float* mod,
                           int64_t ld_mod, const float* gamma, const float* beta, const int32_t* group_batch,
                           int64_t group_rows, int64_t rows_per_batch, int64_t rows, int64_t C, float eps,
                           float p, uint64_t seed, uint32_t site, pfpp_stream_t stream);

/* ---- attention backward ---------------------------------------------------------------------------
 * dqkv [rows, 3*H*dh] receives (dq | dk | dv) of softmax(q.k^T * scale) v.
 * pfpp_attn_dense_train: pfpp_attn_dense that also writes lse[row, h] = log sum_j exp(s_ij) (needed by
 * the backward).  pfpp_attn_dense_bwd: two passes without atomics — dq per query block, dk/dv per key
 * block, both recomputing the probabilities from q, k and lse.
 * Rows outside every sequence / fragment are not written; masked keys receive dk = dv = 0; a sequence
 * without a valid key is outside the contract.  key_valid rows are kv_stride >= max(seq_len) bytes apart.
 * Range of dout.  The exact-fp32 kernels (key mask given, or dim_head 32) have fp32's range.  The split-f16
 * kernels (dense: dim_head 64 without a key mask; block-diagonal) lift dout by 2^12 and
 * dS = P (dout . v - D) scale by 2^14 times a power of two chosen per query row from max|dout row| (1 for
 * |dout| in [1.2e-4, 0.125)) before an fp16 hi / lo split: supported is |dout| < 16; from there on the
 * result is non-finite (inf / NaN), never a finite wrong value.  Downwards the 2e-5 accuracy of dqkv holds
 * to |dout| ~ 1e-6 and degrades gradually below ~1e-8.  DESIGN.md 4.1.                                  */
int pfpp_attn_blockdiag_bwd(const float* qkv, const float* dout, float* dqkv, int64_t n_frag,
                            int64_t L, int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
int pfpp_attn_dense_train(const float* qkv, float* out, float* lse, const int32_t* seq_off,
                          const int32_t* seq_len, const uint8_t* key_valid, int64_t kv_stride,
                          int64_t n_seq, int64_t max_len, int64_t H, int64_t dh, float scale,
                          pfpp_stream_t stream);
int pfpp_attn_dense_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                        float* dvec /* workspace [rows, H] */, float* dqkv, const int32_t* seq_off, const int32_t* seq_len,
                        const uint8_t* key_valid, int64_t kv_stride, int64_t n_seq, int64_t max_len,
                        int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
/* the same in separately launchable parts (bit 0: D = rowsum(dout . out) -> dvec, bit 1: dq, bit 2: dk/dv): once D is
 * there dq and dk/dv are independent (disjoint columns of dqkv) and may be issued on two streams.               */
int pfpp_attn_dense_bwd_parts(const float* qkv, const float* out, const float* dout, const float* lse,
                              float* dvec, float* dqkv, const int32_t* seq_off, const int32_t* seq_len,
                              const uint8_t* key_valid, int64_t kv_stride, int64_t n_seq, int64_t max_len,
                              int64_t H, int64_t dh, float scale, int parts, pfpp_stream_t stream);

/* ---- small backward pieces ----------------------------------------------------------------------------
 * mean_pool_bwd:   dx[(f,l), :] = dpooled[f, :] / L                         (denoiser_transformer.py:139-142)
 * token_combine_bwd: dx_emb[f, :] = sum_l dtok[(f,l), :]; dref_emb[ref[f], :] += dx_emb[f, :]
 *                  (the shape-embedding gradient is dtok itself; pe is a buffer)
 * silu_embed_bwd:  dtables[i][t[b], :] += dse[i, b, :] * silu'(tables[i][t[b], :]); puzzles with equal t[b] are summed in index
 *                  order without atomics (deterministic: data-parallel ranks scattering the same gathered list stay bit-equal) */
int pfpp_mean_pool_bwd(const float* dpooled, float* dx, int64_t n, int64_t L, int64_t C,
                       pfpp_stream_t stream);
int pfpp_token_combine_bwd(const float* dtok, const uint8_t* ref_part, float* dx_emb, float* dref_emb,
                           int64_t n, int64_t L, int64_t C, pfpp_stream_t stream);
int pfpp_silu_embed_bwd(const float* tables, const int64_t* t, const float* dse, float* dtables,
                        int64_t n_tab, int64_t n_emb, int64_t B, int64_t C, pfpp_stream_t stream);
/* the same, and the rows t[.] are marked in `active` (uint32 [ceil(n_emb / 32)], bit r = row r has received a gradient since the bitmap
 * was cleared) for pfpp_adamw_rows_active; n_emb <= 4096 */
int pfpp_silu_embed_bwd_mark(const float* tables, const int64_t* t, const float* dse, float* dtables,
                             int64_t n_tab, int64_t n_emb, int64_t B, int64_t C, uint32_t* active, pfpp_stream_t stream);

/* ---- backward of the AdaLN modulation linears (MyAdaLayerNorm.forward, attention.py:21-25: mods_j = Linear_j(silu(emb_j(t))), one per
 * norm, 2 * num_layers of them) in two launches per 32 puzzles, plain fp32, fixed summation order (csrc/ada_bwd.hip):
 *   g_w[j][n, k] += sum_b dmods[j][b, n] se[j][b, k]     g_b[j][n] += sum_b dmods[j][b, n]     dse[j][b, k] = sum_n dmods[j][b, n] w[j][n, k]
 * dmods [n_ada, B, N2], se / dse [n_ada, B, C], w / g_w [n_ada, N2, C], g_b [n_ada, N2]; scratch: pfpp_ada_linear_bwd_scratch_floats()
 * floats (16-byte aligned).  Replaces a column sum and two tiled gradient GEMMs (the contraction of the weight gradient is only B deep). */
/* ---- backward of the token embedding in one launch (DenoiserTransformer._gen_cond / _add_ref_part_emb / forward,
 * denoiser_transformer.py:117-135, 150-156, 173-185; csrc/embed_train.hip).  The forward leaves the EXTENDED feature rows
 *   F[m] = [shape features (148) | pose features of the token's fragment (147) | [ref_part = 0] | [ref_part = 1] | 1 | 0 ...]  (320 columns)
 * transposed as split-f16 planes ft_hi / ft_lo [320, Mp] (Mp = pfpp_token_features_t_cols(n, L): n L rounded up to 16, zero padded;
 * arguments as pfpp_token_features_slots plus ref_part [slots]); pfpp_token_embed_bwd contracts dtok [n L, C] with them over the tokens:
 *   g_shape_w [C, 148] += dtok^T sf   g_param_w [C, 147] += (sum_l dtok)^T pf   g_shape_b, g_param_b [C] += sum_m dtok[m]
 *   g_ref_emb [2, C]: row r += the sum of dtok over the tokens of fragments with ref_part = r
 * split-f16 products of (g_scale * dtok) (g_scale a power of two, divided out), fixed summation order, no atomics. */
/* training forward: the operand of pfpp_embed_tokens_small built from the fp32 parameters of the step — [W_shape (148) | W_param (147) | 0]
 * [C, 320] as fragment-blocked split-f16 planes fhi / flo (C * 320 halfs each, scale 1) and bias [C] = b_shape + b_param */
int pfpp_embed_pack_weights(const float* w_shape, const float* w_param, const float* b_shape, const float* b_param, void* fhi, void* flo,
                            float* bias, int64_t C, pfpp_stream_t stream);
int64_t pfpp_token_features_t_cols(int64_t n, int64_t L);
int pfpp_token_features_t(const float* latent, const float* xyz, const float* scale, const float* x, const int32_t* slot,
                          const uint8_t* ref_part, void* ft_hi, void* ft_lo, int64_t n, int64_t L, pfpp_stream_t stream);
int pfpp_token_embed_bwd(const float* dtok, const void* ft_hi, const void* ft_lo, float* g_shape_w, float* g_shape_b, float* g_param_w,
                         float* g_param_b, float* g_ref_emb, int64_t n, int64_t L, int64_t C, float g_scale, pfpp_stream_t stream);

int64_t pfpp_ada_linear_bwd_scratch_floats(int64_t n_ada, int64_t N2);
int pfpp_ada_linear_bwd(const float* dmods, const float* se, const float* w, float* g_w, float* g_b, float* dse, float* scratch,
                        int64_t n_ada, int64_t B, int64_t C, int64_t N2, pfpp_stream_t stream);

/* ---- loss (Denoiser._loss, denoiser.py:118-126) ---------------------------------------------------------
 * loss = mean over the selected rows (valid, non-reference fragments) x 7 of (pred - target)^2;
 * dpred = grad_out * 2 (pred - target) / (7 * n_sel) on selected rows, 0 elsewhere.  loss [1].       */
int pfpp_mse_loss(const float* pred, const float* target, const uint8_t* sel, float* loss,
                  float* dpred, int64_t n, int64_t width, float grad_out, pfpp_stream_t stream);
/* the same with the selection computed in the kernel: row r counts iff valid[r] != 0 and ref[r] == 0 (part_valids & ~ref_part,
 * denoiser.py:118-121, never materialised); amax (optional, needs dpred): receives max |dpred| of the call */
int pfpp_mse_loss_masked(const float* pred, const float* target, const float* valid, const uint8_t* ref, float* loss,
                         float* dpred, float* amax, int64_t n, int64_t width, float grad_out, pfpp_stream_t stream);

/* ---- AdamW (configure_optimizers, denoiser.py:230-241; torch.optim.AdamW semantics) ---------------------
 * p *= 1 - lr*wd; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g^2;
 * p -= (lr / bc1) * m / (sqrt(v)/sqrt(bc2) + eps)      with bc1 = 1-b1^t, bc2 = 1-b2^t, g *= g_scale.
 * hi/lo (may be NULL): refreshed split-f16 planes of p for the forward GEMMs.                        */
int pfpp_adamw(float* p, const float* g, float* m, float* v, void* hi, void* lo, int64_t n,
               float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
               float bc2, float g_scale, pfpp_stream_t stream);
/* the same, and with zero_grad != 0 the gradient buffer is cleared in the same pass (optimizer.step() + optimizer.zero_grad(),
 * the pair a training loop issues back to back) */
int pfpp_adamw_zero(float* p, float* g, float* m, float* v, void* hi, void* lo, int64_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                    float bc2, float g_scale, int zero_grad, pfpp_stream_t stream);
/* the same with the overflow guard of a loss-scaled optimizer (what torch.cuda.amp.GradScaler.step does around
 * configure_optimizers' AdamW, denoiser.py:230-241, when the backward runs on fp16 operands), entirely on the device:
 * overflow (int32[2], device memory): [0] = flag, [1] = count.  An element whose (scaled) gradient is inf / NaN is left untouched
 * (p, m, v, planes unchanged; its gradient is still cleared when zero_grad != 0), sets the flag and adds to the count.  The kernel
 * never READS the flag: which elements are skipped depends on their own gradient only, so the result is independent of workgroup
 * scheduling and identical on data-parallel replicas.  The caller clears overflow[] between steps and reads it when it likes. */
int pfpp_adamw_guarded(float* p, float* g, float* m, float* v, void* hi, void* lo, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                       float bc2, float g_scale, int zero_grad, int32_t* overflow, pfpp_stream_t stream);
/* pfpp_adamw_guarded over n_ranges ranges [off[k], off[k] + len[k]) of the same buffers in ONE launch (off, len: HOST arrays of element
 * offsets / counts, at most PFPP_ADAMW_RANGES_MAX; empty ranges are skipped): the biases, LayerNorm affine and padding of a transformer
 * layer's slice, whose matrices pfpp_gemm_dw_group updates in its epilogue (pfpp_dw_update).  Element for element what
 * pfpp_adamw_guarded(p + off[k], ..., len[k], ...) gives, overflow flag and count included. */
#define PFPP_ADAMW_RANGES_MAX 16
int pfpp_adamw_ranges(float* p, float* g, float* m, float* v, void* hi, void* lo, const int64_t* off, const int64_t* len, int32_t n_ranges,
                      float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2, float g_scale,
                      int zero_grad, int32_t* overflow, pfpp_stream_t stream);
/* Adam over a list of tensors in a handful of launches (Jigsaw_matching/model/modules/matching_base_model.py:499-515: one
 * torch.optim.Adam / AdamW over self.parameters(), which torch steps tensor by tensor or through its own multi-tensor path).  p, g, m,
 * v: HOST arrays of n_tensors device pointers, n: host array of element counts (>= 0; a tensor with n == 0 is skipped and may have null
 * pointers), bc1 / bc2: host arrays of the tensors' own bias corrections 1 - beta^step (torch keeps `step` per parameter; a parameter
 * without a gradient in earlier steps has a smaller one).  Per element the update is pfpp_adamw's, bit for bit (no planes, no
 * zero_grad, no guard): both kernels call the one element function of csrc/adamw_element.h, whose fused multiply-adds are written
 * out under contract(off).  g is not written.  The descriptors travel
 * in the kernel-argument struct
 * (<= 4 KB, no device-side table): a launch holds at most PFPP_ADAM_MULTI_MAX_TENSORS tensors and PFPP_ADAM_MULTI_MAX_BLOCKS
 * workgroups of PFPP_ADAM_MULTI_CHUNK elements; tensors are taken in order, and one that the block capacity cuts goes on in the next
 * launch.  Pointers need 4-byte alignment only.  Refused before any launch: n_tensors < 0, a null array, a null pointer of a
 * non-empty tensor, n < 0, bc <= 0.  n_tensors == 0 is a no-op. */
#define PFPP_ADAM_MULTI_MAX_TENSORS 36
#define PFPP_ADAM_MULTI_MAX_BLOCKS 384
#define PFPP_ADAM_MULTI_CHUNK 8192
int pfpp_adam_multi(int64_t n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                    const float* bc1, const float* bc2, float lr, float beta1, float beta2, float eps, float weight_decay,
                    float g_scale, pfpp_stream_t stream);
/* the same update restricted by ROWS of a stack of embedding tables [n_tables, rows_per_table, C] (the 12 AdaLN timestep tables,
 * MyAdaLayerNorm.emb = nn.Embedding(num_embeds_ada_norm, dim), attention.py:18-25): a step touches only the rows of the batch's
 * timesteps t [n_t] (int64, device), every other row has an exactly zero gradient and its update (moment decay, weight decay, the
 * step of the decayed first moment) depends on nothing of this step's backward.  mode 0: every row EXCEPT t[.] — issued at the
 * start of the backward, off the iteration's exposed tail; mode 1: only the rows t[.] (each once, whatever the duplicates in t) —
 * after their gradients are final.  Both together = one pfpp_adamw_guarded over the stack, element for element.          */
int pfpp_adamw_rows(float* p, float* g, float* m, float* v, void* hi, void* lo, int64_t n_tables, int64_t rows_per_table, int64_t C,
                    const int64_t* t, int64_t n_t, int mode, float lr, float beta1, float beta2, float eps, float weight_decay,
                    float bc1, float bc2, float g_scale, int zero_grad, int32_t* overflow, pfpp_stream_t stream);
/* pfpp_adamw_guarded over the stack restricted to the rows whose bit is set in `active` (pfpp_silu_embed_bwd_mark: every row that has
 * ever received a gradient).  A row that never did has g = m = v = 0, and with weight decay as small as the reference's
 * (configure_optimizers, denoiser.py:230-237: lr 2e-4, weight_decay 1e-6 -> fl32(1 - lr wd) = 1) its AdamW update is exactly the
 * identity: of the 3,072 rows per table only the 1,000 training timesteps can ever be indexed, two thirds of the tables' 18.9 M parameters
 * are never read or written.  When fl32(1 - lr * weight_decay) != 1 every row is taken (the plain update).  The caller owns the
 * bitmap's meaning: set every bit after restoring optimizer state it does not know the history of. */
int pfpp_adamw_rows_active(float* p, float* g, float* m, float* v, void* hi, void* lo, int64_t n_tables, int64_t rows_per_table, int64_t C,
                           const uint32_t* active, float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2,
                           float g_scale, int zero_grad, int32_t* overflow, pfpp_stream_t stream);

/* ---- train-mode BatchNorm of the (frozen, but .train()) encoder (utils/pn2_utils.py:211-214) -------------
 * The reference freezes the encoder's parameters only (train_denoiser.py:33-35); under Lightning's
 * model.train() its BatchNorm2d layers normalise with batch statistics and keep updating their buffers.
 * bn_stats: per column mean and biased variance over the rows of x [rows, C] (ld), accumulated in fp64
 * (torch's CPU kernel accumulates in double); when running_mean != NULL the running statistics are
 * updated like torch: r = (1-momentum)*r + momentum*stat, with the unbiased variance.
 * workspace: at least pfpp_bn_stats_workspace(rows, C) bytes.
 * bn_apply: y = relu(x*a + b) with a = gamma/sqrt(var+eps), b = beta - mean*a (the form ATen's CPU kernel
 * uses), optional max over groups of `pool` consecutive rows (the set-abstraction max, pn2_utils.py:216):
 * y [rows/pool, ldy].  C % 4 == 0, C <= 1024.                                                         */
/* fused form: the producing GEMM accumulates stats (see pfpp_gemm_args.stats); bn_finalize turns them into
 * mean/var (optional outputs), updates the running buffers, writes the affine a = gamma/sqrt(var+eps),
 * b = beta - mean*a for the consuming GEMM's a_mul/a_add, and clears stats for the next use.
 * bn_minmax_apply: y = relu(a*(a >= 0 ? mx : mn) + b) == max over the pool group of relu(a*x + b).    */
int pfpp_bn_finalize(double* stats, int64_t copies, int64_t rows, int64_t C, const float* gamma,
                     const float* beta, float eps, float momentum, float* running_mean,
                     float* running_var, float* mean, float* var, float* a_mul, float* a_add,
                     pfpp_stream_t stream);
int pfpp_bn_minmax_apply(const float* mx, const float* mn, const float* a_mul, const float* a_add,
                         float* y, int64_t rows, int64_t C, pfpp_stream_t stream);
int64_t pfpp_bn_stats_workspace(int64_t rows, int64_t C);
int pfpp_bn_stats(const float* x, int64_t rows, int64_t C, int64_t ld, float* mean, float* var,
                  float* running_mean, float* running_var, float momentum, void* workspace,
                  pfpp_stream_t stream);
int pfpp_bn_apply(const float* x, int64_t rows, int64_t C, int64_t ld, const float* mean,
                  const float* var, const float* gamma, const float* beta, float eps, float* y,
                  int64_t ldy, int64_t pool, pfpp_stream_t stream);

/* ---- a17: the transformer blocks of the training step, sequenced from C ------------------------------------
 * EncoderLayer.forward (denoiser/model/modules/attention.py:74-92) for a range of the layers of
 * DenoiserTransformer.forward (denoiser_transformer.py:187-196) in train mode, and its backward (autograd of
 * Denoiser.training_step, denoiser.py:128-145): the SAME launches with the SAME arguments that the host issues one by
 * one through the entry points above (pfpp_layernorm_*_split / pfpp_dropout_layernorm_p, pfpp_gemm_planes,
 * pfpp_attn_blockdiag_split, pfpp_attn_dense_train_p, pfpp_geglu_p; backward: pfpp_gemm_planes in its dX / dW forms,
 * pfpp_geglu_bwd_p, pfpp_layernorm_bwd_p, pfpp_attn_*_bwd_p, pfpp_adamw_guarded) — enqueued from one call, so that the
 * ~240 launches of the six blocks cost the host what hipLaunchKernel costs, not a marshalled foreign call each.
 * Activations live in caller-owned arenas: layer i's saved tensors at fwd_arena + i * fwd_layer_bytes (layout private to
 * the library, pfpp_tlayers_fwd_bytes() bytes; the layer's output [M, C] fp32 sits at pfpp_tlayers_fwd_hout_offset()),
 * the backward's temporaries in bwd_arena (pfpp_tlayers_bwd_bytes()).  Weight planes are the caller's (scale 1 unless
 * stated in .scale).  Weight / bias gradients ACCUMULATE into the fp32 buffers of pfpp_tlayer_grads.                    */
typedef struct pfpp_tlayer_params {
  pfpp_planes qkv1, o1, qkv2, o2, ff1, ff2;      /* [3C,C] (to_q|to_k|to_v), [C,C], [3C,C], [C,C], [2 inner, C], [C, inner] */
  const float *bo1, *bo2, *g3, *b3, *bff1, *bff2; /* to_out.0.bias x2, norm3.weight / bias, ff.net.0.proj.bias, ff.net.2.bias */
} pfpp_tlayer_params;
typedef struct pfpp_tlayer_grads {
  float *qkv1_w, *o1_w, *o1_b, *qkv2_w, *o2_w, *o2_b, *g3, *b3, *ff1_w, *ff1_b, *ff2_w, *ff2_b;
} pfpp_tlayer_grads;
typedef struct pfpp_tlayer_adamw {              /* the layer's contiguous slice of the flat parameter buffers */
  float *p, *g, *m, *v; void *hi, *lo; int64_t n;
} pfpp_tlayer_adamw;
typedef struct pfpp_tlayers_args {
  int32_t n_layers;
  const pfpp_tlayer_params* layers;             /* [n_layers] (host memory) */
  const pfpp_tlayer_grads* grads;               /* [n_layers], backward only */
  const pfpp_tlayer_adamw* adamw;               /* [n_layers] or NULL: optimizer-in-backward on the side stream (needs side != NULL) */
  int64_t M, C, H, L, inner, Fv, B;             /* tokens (= Fv * L), width, heads, latent points, GEGLU inner width, fragments, puzzles */
  float* h_in;                                  /* [M, C] tokens; token dropout is applied IN PLACE when p_tok > 0 */
  const float* mods;                            /* [2 n_layers, B, 2C] AdaLN (scale | shift) rows */
  const int32_t* frag_b;                        /* [Fv] puzzle of every fragment */
  const int32_t *seq_off, *seq_len;             /* [n_seq] token range of every puzzle */
  int64_t n_seq, max_len;
  float att_scale, p_tok, p_lay;
  uint64_t seed;
  void* fwd_arena; int64_t fwd_layer_bytes;
  float *ws_main, *ws_side; int64_t ws_bytes;   /* K-split workspaces of pfpp_gemm_planes, one per stream */
  /* backward */
  void* bwd_arena; int64_t bwd_bytes;
  float grad_scale;                             /* power of two lifting gradient planes into the fp16 range */
  float* dh;                                    /* [M, C] running gradient of the residual stream, updated in place */
  pfpp_planes dhp;                              /* its planes (grad_scale * dh) on entry */
  pfpp_planes* dhp_out;                         /* optional: where the planes of the gradient leaving the range are (inside bwd_arena) */
  float* dmods;                                 /* [2 n_layers, B, 2C] AdaLN row gradients (accumulated) */
  float* dtok;                                  /* [M, C] gradient w.r.t. the tokens (needed when the range reaches layer 0) */
  float lr, beta1, beta2, eps, weight_decay, bc1, bc2, opt_g_scale; int32_t opt_zero_grad; int32_t* overflow;   /* with adamw */
  /* optional (NULL: the tiled kernel everywhere): scratch of at least pfpp_tlayers_frag_bytes() for the fragment-blocked copies of a
   * layer's weights — the qkv / out / second feed-forward linears of the forward and their input gradients then run through
   * pfpp_gemm_wd.  With room for every layer of the call's range (n x pfpp_tlayers_frag_bytes()) the range's weights are blocked by ONE
   * launch at the top of the call instead of one per layer */
  void* frag_ws; int64_t frag_ws_bytes;
  /* optional (ada_se == NULL: the caller does this after the call), backward, side != NULL: the two AdaLN linears of every block
   * (MyAdaLayerNorm.linear, attention.py:21-25: mods_j = silu(table_j[t]) . W_j^T + b_j, j = 2 i, 2 i + 1) take their gradients as soon
   * as block i's backward is through — gb_j += colsum(dmods_j), gw_j += dmods_j^T . se_j, and the gradient w.r.t. the embedded timestep
   * dse_j = dmods_j . W_j — on the side stream, followed (with adamw) by the AdamW update of W_j / b_j (ada_adamw_w / _b [n_layers]:
   * the block's slices [2 i, 2 i + 2) of the stacked parameters): none of it is left for the exposed tail of the iteration */
  const float* ada_se;                          /* [2 n_layers, B, C] silu(table[t]) rows of the forward */
  float* ada_dse;                               /* [2 n_layers, B, C] out */
  const float* ada_w;                           /* [2 n_layers, 2C, C] fp32 weights (read before their update) */
  float* ada_gw; float* ada_gb;                 /* [2 n_layers, 2C, C], [2 n_layers, 2C] gradients, accumulated */
  const pfpp_tlayer_adamw* ada_adamw_w;         /* [n_layers] or NULL */
  const pfpp_tlayer_adamw* ada_adamw_b;         /* [n_layers] or NULL */
  /* backward, != 0: the caller vouches that the matrices' ranges of the gradient buffers are ZERO on entry.  Where the layer's update
   * is also armed with opt_zero_grad on a side stream and the grouped weight-gradient launch is on, a block's six matrices are then
   * updated in that launch's epilogue (pfpp_dw_update) and never pass through memory — their gradient ranges stay zero — and the rest
   * of the layer's slice takes one pfpp_adamw_ranges launch where pfpp_adamw_guarded ran.  Same p, m, v, planes and flag, bit for bit. */
  int32_t opt_fused_dw;
} pfpp_tlayers_args;
int64_t pfpp_tlayers_frag_bytes(int64_t C, int64_t inner);
int64_t pfpp_tlayers_fwd_bytes(int64_t M, int64_t C, int64_t H, int64_t inner);
int64_t pfpp_tlayers_fwd_hout_offset(int64_t M, int64_t C, int64_t H, int64_t inner);
int64_t pfpp_tlayers_bwd_bytes(int64_t M, int64_t C, int64_t H, int64_t inner);
int pfpp_tlayers_fwd(const pfpp_tlayers_args* args, int32_t layer_lo, int32_t layer_hi, pfpp_stream_t stream);
/* layers layer_hi-1 ... layer_lo; side = stream of the weight-gradient GEMMs (NULL: the main stream) */
int pfpp_tlayers_bwd(const pfpp_tlayers_args* args, int32_t layer_lo, int32_t layer_hi, pfpp_stream_t stream, pfpp_stream_t side);

/* The same blocks in EVAL mode for a compacted fragment list (the sampler / auto_aggl step, denoiser.py:172-185 ->
 * DenoiserTransformer.forward, denoiser_transformer.py:187-196): h [M, C] fp32 is updated in place through n_layers blocks; the
 * launches are those of pfpp_layernorm_grouped_split / pfpp_layernorm_split, pfpp_gemm (packed weights: planes of scale * W, the
 * GEGLU pair interleaved 32 value / 32 gate rows, gate applied in the epilogue), pfpp_attn_blockdiag_split and pfpp_attn_dense_split,
 * enqueued from one call.  norm / att [M, C] and u [M, inner] are scratch planes, qkv [M, 3C] scratch fp32 (caller-owned);
 * split_ws / split_cnt: the split-K workspace of pfpp_gemm (see pfpp_gemm_args).                                              */
/* fhi / flo (optional, NULL = absent): the same planes FRAGMENT-BLOCKED for the few-token kernels (pfpp_layernorm_linear_small): block
 * (row tile r = n / 32, k-step s = k / 16) is 1 KB = 64 x 8 halfs, entry 32 (k % 16 / 8) + n % 32 holds W[n][16 s + 8 (k % 16 / 8) .. + 8) — the
 * B operand of one v_mfma_f32_32x32x16_f16 as the 64 lanes hold it; blocks ordered [r][s].  N % 32 == 0, K % 16 == 0, no row padding. */
typedef struct pfpp_pw { const float* f32; const void* hi; const void* lo; float scale; int64_t ldw; const void* fhi; const void* flo; } pfpp_pw;
typedef struct pfpp_elayer_params {
  pfpp_pw qkv1, o1, qkv2, o2, ff1, ff2;            /* [3C,C], [C,C], [3C,C], [C,C], [2 inner (interleaved), C], [C, inner] */
  const float *bo1, *bo2, *g3, *b3, *bff1, *bff2;
} pfpp_elayer_params;
typedef struct pfpp_tlayers_eval_args {
  int32_t n_layers;
  const pfpp_elayer_params* layers;
  int64_t M, C, H, L, inner, Fv, B;
  float* h;
  const float* mods;                               /* [2 n_layers, B, 2C] */
  const int32_t* frag_b; const int32_t *seq_off, *seq_len;
  int64_t n_seq, max_len;
  float att_scale;
  int32_t single_pass;                             /* 1: PFPP_GEMM_F16 on the GEMMs (perf mode) */
  pfpp_planes norm, att, u; float* qkv;
  float* split_ws; int64_t split_ws_bytes; int32_t* split_cnt; int64_t split_cnt_len;
  int64_t lnlin_max_rows;                          /* M <= this: LayerNorm + the following linear as one launch (pfpp_layernorm_linear_small) */
  int32_t wd_gemm;                                 /* 1: above lnlin_max_rows the qkv / out / second feed-forward linears through pfpp_gemm_wd */
} pfpp_tlayers_eval_args;
int pfpp_tlayers_eval(const pfpp_tlayers_eval_args* args, pfpp_stream_t stream);
/* LayerNorm fused into the linear layer that follows it, for small token counts (one puzzle in flight): y = LN(x) . W^T (+ bias), the
 * normalised rows never reach HBM (MyAdaLayerNorm / nn.LayerNorm + to_q|k|v resp. the GEGLU projection, attention.py:21-25,77-90, eval
 * mode).  mod [B, 2C] (scale | shift) with group_batch / group_rows as in pfpp_layernorm_grouped, or gamma / beta.  Plain form: out
 * [M, ldc] fp32.  GEGLU form (u_planes set; w = packed 32 value | 32 gate rows, bias packed likewise): u = (v + b_v) * gelu(g + b_g)
 * as planes [M, ldu], N = 2 * inner.  C = 512, N % 64 == 0.  LayerNorm arithmetic = pfpp_layernorm*; the contraction is summed in a
 * different (fixed) order than pfpp_gemm's: equal to the two-launch path to fp32 rounding.  pfpp_tlayers_eval uses it for M <= lnlin_max_rows
 * (pfpp_hip passes 2048: up to there the few-token kernels beat the tiled GEMMs in the auto_aggl loop; 0 = never).                                                                                                  */
/* Token embedding for few tokens, one launch (denoiser_transformer.py:117-135, 150-156, 173-185; EmbedderNerf, utils/model_utils.py:68-69):
 * tok[(f, l), :] = shape_embedding([latent | PE(xyz) | PE(scale)]) + param_fc(PE(x_f)) + ref_part_emb[ref_f] + pe[frag_pos_f] for the n listed
 * fragments (slot: listed fragment -> slot of latent / xyz / scale / x / ref_part, or NULL).  w_cat = the CONCATENATED weight
 * [W_shape (148 columns) | W_param (147) | 0 ... ] [C, 320] with its fragment-blocked planes, bias = shape bias + param bias.  Replaces
 * pfpp_token_features + two pfpp_gemm + pfpp_token_combine for small n L (pfpp_hip: <= 2,048 tokens); equal to them to fp32 rounding
 * (both linear layers share one accumulation).  L >= 11, C % 32 == 0.                                                                */
int pfpp_embed_tokens_small(const float* latent, const float* xyz, const float* scale, const float* x, const int32_t* slot,
                            const pfpp_pw* w_cat, const float* bias, const float* ref_emb, const uint8_t* ref_part, const float* pe,
                            const int32_t* frag_pos, float* tok, int64_t n, int64_t L, int64_t C, pfpp_stream_t stream);
/* Plane GEMM for few rows: out [M, ldc] = A . W^T / (A.scale * w.scale) + bias + residual, A = planes [M, lda] of a [M, K] operand, w
 * with its fragment-blocked planes (fhi / flo).  The out-projections of both attentions and the second feed-forward linear with their
 * residual adds (attention.py:77-90), eval mode; out may be the residual (in place).  K % 512 == 0, N % 32 == 0.  Same products as
 * pfpp_gemm's split-f16 path, one k-ordered chain per output (equal to it to fp32 rounding); pfpp_tlayers_eval uses it for
 * M <= lnlin_max_rows.  Kernel choice (csrc/gemm_small.hip choose_gemm_small, reported by pfpp_last_gemm_kernel): the contraction
 * split over eight waves (gemm_small_ks_kernel<8, 2>) for K = 2048 at M <= 512, one chain per output (gemm_small_kernel) otherwise.
 * pfpp_gemm_small_v: variant 0 = that choice (what pfpp_gemm_small passes), 1 = the one-chain kernel at every shape (the cross-check
 * of the split kernel), anything else PFPP_EINVAL.  No environment variable selects a kernel here or in pfpp_gemm_wd.              */
int pfpp_gemm_small(const pfpp_planes* A, int64_t lda, const pfpp_pw* w, const float* bias, const float* residual, int64_t ldr, float* out,
                    int64_t ldc, int64_t M, int64_t N, int64_t K, pfpp_stream_t stream);
int pfpp_gemm_small_v(const pfpp_planes* A, int64_t lda, const pfpp_pw* w, const float* bias, const float* residual, int64_t ldr, float* out,
                      int64_t ldc, int64_t M, int64_t N, int64_t K, int32_t variant, pfpp_stream_t stream);
/* The same operation above the few-token range, weights never staged through LDS (csrc/gemm_wd.hip): out [M, ldc] = (A . W^T) / (A.scale *
 * w.scale) + bias + residual with A = row-major planes [M, lda] and w's fragment-blocked planes read straight into the matrix operands
 * (attn.to_q|k|v / attn.to_out[0] / ff.net[2] of attention.py:77-90, eval mode: static weights).  N % 128 == 0, K % 32 == 0, 16-byte
 * aligned rows; out may be the residual.  Bit-identical to pfpp_gemm's split-f16 plane path on the same operands (same products, same
 * order, same epilogue); pfpp_tlayers_eval uses it for M > lnlin_max_rows when args.wd_gemm is set.                                      */
int pfpp_gemm_wd(const pfpp_planes* A, int64_t lda, const pfpp_pw* w, const float* bias, const float* residual, int64_t ldr, float* out,
                 int64_t ldc, int64_t M, int64_t N, int64_t K, pfpp_stream_t stream);
int pfpp_gemm_wd_supported(int64_t M, int64_t N, int64_t K);
/* the same in the single-pass fp16 mode (hi planes only, one matrix instruction per product: PFPP_GEMM_F16 of pfpp_gemm — BASELINE configs[4]'s
 * "fp16 MFMA" perf mode, never a parity mode); bit-identical to pfpp_gemm's single-pass plane path */
int pfpp_gemm_wd_f16(const pfpp_planes* A, int64_t lda, const pfpp_pw* w, const float* bias, const float* residual, int64_t ldr, float* out,
                     int64_t ldc, int64_t M, int64_t N, int64_t K, pfpp_stream_t stream);
/* Fragment-blocked copies of row-major weight planes w [N, ldw] (N x K used), one launch for up to PFPP_REBLOCK_MAX weights: fhi / flo
 * receive the layout of pfpp_pw.fhi / flo of W (transposed == 0: N % 32 == 0, K % 16 == 0) or of W^T [K, N] (transposed == 1: the operand
 * of dX = dY . W for pfpp_gemm_wd; N % 64 == 0, K % 64 == 0).  Training weights change every step: pfpp_tlayers_fwd / _bwd make the
 * copies of a layer where they read them (args.frag_ws), so that a copy can never be stale.                                         */
#define PFPP_REBLOCK_MAX 32
typedef struct pfpp_reblock_job { pfpp_planes w; int64_t N, K, ldw; void *fhi, *flo; int32_t transposed; } pfpp_reblock_job;
int pfpp_reblock_planes(const pfpp_reblock_job* jobs, int32_t n, pfpp_stream_t stream);
int pfpp_layernorm_linear_small(const float* x, const float* mod, int64_t ld_mod, const float* gamma, const float* beta,
                                const int32_t* group_batch, int64_t group_rows, const pfpp_pw* w, const float* bias, float* out,
                                int64_t ldc, const pfpp_planes* u_planes, int64_t ldu, int64_t M, int64_t N, int64_t C, float eps,
                                pfpp_stream_t stream);

/* ---- a15: the two output heads as one launch each way -------------------------------------------------------
 * DenoiserTransformer._out (denoiser_transformer.py:138-147) after the mean over the L latent points: pooled [R, C] ->
 * mlp_out_trans / mlp_out_rot (Linear(C,C) - SiLU - Linear(C,C/2) - SiLU - Linear(C/2, 3 | 4), :58-61) -> out[row, 0:3] |
 * out[row, 3:7], row = slot ? slot[r] : r (the scatter back to the padded fragment slots).  a0 / v0 [2, R, C] and a1 / v1
 * [2, R, C/2] (pre-activations and SiLU values of both heads, trans first) are saved for the backward when given (all or none).
 * Weights: split-f16 planes of scale * W (row-major [out, in]) for the two wide layers, fp32 for the last.  C = 512.
 * pfpp_heads_bwd: from dout (unscaled; row r of the heads is dout[slot ? slot[r] : r, 0:7]) it writes da0 [2, R, C], da1 [2, R, C/2] (the dY operands of the four wide
 * weight-gradient GEMMs, which stay with pfpp_gemm_grad_group), accumulates dW4 / db4 / db2 / db0 of both heads with atomics,
 * writes each head's share of d pooled to dp [2, R, C] and, when dx is given, dx [(r, l), :] = (dp[0] + dp[1])[r, :] / L
 * (the backward of the mean pool, :139-142).  grad_scale: power of two lifting the gradient planes into the fp16 range.   */
typedef struct pfpp_head_params {
  pfpp_planes w0, w2;                         /* [C, C], [C/2, C] */
  const float *w4, *b0, *b2, *b4;             /* [3 | 4, C/2], [C], [C/2], [3 | 4] */
  pfpp_planes f0, f2;                         /* optional (hi == NULL: absent): w0 / w2 fragment-blocked as pfpp_pw.fhi / flo — static (eval)
                                                 weights; pfpp_heads_fwd then loads the MFMA operands with fully coalesced instructions */
} pfpp_head_params;
typedef struct pfpp_head_grads { float *w4, *b4, *b2, *b0; } pfpp_head_grads;
int pfpp_heads_fwd(const float* pooled, const pfpp_head_params* trans, const pfpp_head_params* rot, int64_t R, int64_t C,
                   float* a0, float* v0, float* a1, float* v1, float* out, const int32_t* slot, int64_t ldo,
                   pfpp_stream_t stream);
int pfpp_heads_bwd(const float* dout, const int32_t* slot, const pfpp_head_params* trans, const pfpp_head_params* rot, int64_t R, int64_t C,
                   const float* a0, const float* v0, const float* a1, const float* v1, float* da0, float* da1, float* dp,
                   const pfpp_head_grads* g_trans, const pfpp_head_grads* g_rot, float grad_scale, float* dx, int64_t L,
                   pfpp_stream_t stream);

/* ==== verifier training (csrc/verifier_train.hip) ====================================================================
 * Verifier.training_step / _loss / configure_optimizers (verifier/model/verifier.py:20-69, 100-107) around
 * VerifierTransformer.forward (verifier_transformer.py:45-58) in train mode: nn.TransformerEncoderLayer(d_model 256, nhead 8,
 * dim_feedforward 2048, dropout 0.1, activation gelu, batch_first, post-norm).  The projections, LayerNorm + dropout sites,
 * gradient GEMMs and AdamW are the denoiser's kernels above; these are the verifier-only pieces.  Dropout masks use the
 * generator of pfpp_dropout (keep = rng(seed, site, counter) >= p * 2^32) and are regenerated in the backward.
 *
 * Self-attention with dropout on the probabilities (nn.MultiheadAttention(dropout=0.1) with key_padding_mask = ~edge_valids,
 * verifier_transformer.py:55 -> torch.nn.functional.multi_head_attention_forward): qkv [B*E, 3*H*dh] = (q | k | v) of the
 * in-projection, out [B*E, H*dh] = dropout(softmax(q k^T * scale + mask)) v, lse [B*E, H] = log sum_j exp(s_ij) over the valid
 * keys.  keep(b, h, q, k) = rng(seed, site, ((b*H + h)*E + q)*E + k).  Masked keys have P = 0 exactly.  A sequence without a
 * valid key produces out = 0, lse = +inf and zero gradients (torch produces NaN there).  One workgroup per (sequence, head),
 * exact fp32; dh = 32 and E <= 256 only (PFPP_EUNSUPPORTED otherwise).
 * pfpp_verifier_attn_bwd: dqkv [B*E, 3*H*dh] = (dq | dk | dv) in one launch, using D_i = dO_i . O_i (holds with dropout on P).
 * pfpp_verifier_attn_dropout_mask: the keep mask as uint8 [B, H, E, E] (tests).                                          */
int pfpp_verifier_attn_fwd(const float* qkv, float* out, float* lse, const uint8_t* key_valid, int64_t B, int64_t E, int64_t H,
                           int64_t dh, float scale, float p, uint64_t seed, uint32_t site, pfpp_stream_t stream);
int pfpp_verifier_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                           const uint8_t* key_valid, int64_t B, int64_t E, int64_t H, int64_t dh, float scale, float p, uint64_t seed,
                           uint32_t site, pfpp_stream_t stream);
int pfpp_verifier_attn_dropout_mask(uint8_t* keep, int64_t B, int64_t H, int64_t E, float p, uint64_t seed, uint32_t site,
                                    pfpp_stream_t stream);

/* mlp_out + weighted BCE (verifier_transformer.py:57, verifier.py:20-47), one pass over h6 [M, C] (C = 256):
 *   logits[r] = h6[r] . w + b[0]  (every row);  over the N valid rows (valid[r] != 0), weight w_r = neg_weight if target == 0 else 1:
 *   loss = sum_r w_r (max(x,0) - x y + log1p(exp(-|x|))) / N   (mean over N, not over sum w; 0 when N = 0)
 *   dlogit[r] = w_r (sigmoid(x) - y) / N (0 for invalid rows), dh6 = dlogit (x) w (optional), dw += sum_r dlogit h6, db += sum_r dlogit
 *   stats int32[4] = (tp, fp, tn, fn) of pred = fp32 sigmoid(x) > 0.5 against target > 0.5;  amax (optional) = max |dlogit|.
 * Other modes: dlogit_in != NULL (the head's backward for an upstream gradient of the logits): d = dlogit_in[r] on every row, no
 * loss / counts (written as 0); target == NULL and dlogit_in == NULL: logits only.
 * Gradients are unscaled fp32 (the gradient GEMMs lift their operands, pfpp_gemm_grad a_scale).  workspace: fp64
 * [pfpp_verifier_head_bce_workspace()] zeroed once by the caller; every call leaves it zeroed again (not shared by concurrent calls). */
int pfpp_verifier_head_bce(const float* h6, const float* w, const float* b, const float* target, const uint8_t* valid,
                           const float* dlogit_in, int64_t M, int64_t C, float neg_weight, float* logits, float* dlogit, float* dh6, float* dw, float* db, float* loss,
                           int32_t* stats, float* amax, double* workspace, pfpp_stream_t stream);
int64_t pfpp_verifier_head_bce_workspace(void);

/* GELU (exact erf) + dropout of the feed-forward (TransformerEncoderLayer._ff_block: dropout(gelu(linear1(x)))), flat n (% 4 == 0):
 *   fwd: u = gelu(z) keep / (1-p);   bwd: dz = gelu'(z) keep / (1-p) du;   keep = rng(seed, site, i)                              */
int pfpp_verifier_gelu_dropout(const float* z, float* u, int64_t n, float p, uint64_t seed, uint32_t site, pfpp_stream_t stream);
int pfpp_verifier_gelu_dropout_bwd(const float* z, const float* du, float* dz, int64_t n, float p, uint64_t seed, uint32_t site,
                                   pfpp_stream_t stream);

/* ---- VQ-VAE pre-training (vqvae/model/fracture_ae.py; csrc/vqvae_train.hip) ----------------------------------------
 * pfpp_chamfer_fwd: chamferdist.ChamferDistance(r, p, bidirectional=True) (pn2.py:83-97, vq_vae.py:75-89): for every source
 * point r[b, i] (= off[b, i] + ctr[b, i / rep] when ctr is given: pc_offset + xyz[:, :, None]) the squared distance to, and the
 * index of, its nearest target point, and the same from every target point to the sources.  The distances equal
 * pfpp_nn_dist's bit for bit; an exact tie keeps the lowest index.  off [batch, n, 3], ctr [batch, n / rep, 3], tgt
 * [batch, m, 3]; d_src / i_src [batch, n], d_tgt / i_tgt [batch, m].
 * pfpp_chamfer_bwd: grad[b, i] = 2 s [(r_i - p_{i_src(i)}) + sum_{j : i_tgt(j) = i} (r_i - p_j)] with s = scale (* gscale[0]
 * when given, a device scalar) — d loss / d r (= d / d off); written as a gather per source point.
 * pfpp_chamfer_reduce: loss[0] = scale (sum d_src + sum d_tgt), fp64 accumulation in a fixed order.                     */
int pfpp_chamfer_fwd(const float* off, const float* ctr, int64_t rep, const float* tgt, float* d_src, int32_t* i_src,
                     float* d_tgt, int32_t* i_tgt, int64_t batch, int64_t n, int64_t m, pfpp_stream_t stream);
int pfpp_chamfer_bwd(const float* off, const float* ctr, int64_t rep, const float* tgt, const int32_t* i_src, const int32_t* i_tgt,
                     float* grad, int64_t batch, int64_t n, int64_t m, float scale, const float* gscale, pfpp_stream_t stream);
int pfpp_chamfer_reduce(const float* d_src, int64_t n_src, const float* d_tgt, int64_t n_tgt, float scale, float* loss,
                        pfpp_stream_t stream);
/* pfpp_vq_train: the training side of VectorQuantizer.forward (quantizer.py:45-67) from z [R, D] and the codes pfpp_vq_encode
 * wrote (n = R D): out[0] = embedding_loss = (1 + beta) mean((e - z)^2), out[1] = perplexity = exp(-sum_k p_k log(p_k + 1e-10)),
 * dz = g 2 (z - e) / n (the first term's gradient; the decoder's straight-through gradient is the caller's), dcodebook[k] =
 * g 2 beta sum_{code = k} (e_k - z) / n (a gather per code), g = g_emb[0] or 1.  dz / dcodebook may be NULL.  D = 16.
 * workspace: pfpp_vq_train_workspace(R, K) bytes.                                                                         */
int pfpp_vq_train(const float* z, const float* codebook, const int32_t* codes, int64_t R, int64_t K, int64_t D, float beta,
                  const float* g_emb, float* dz, float* dcodebook, float* out, void* workspace, pfpp_stream_t stream);
int64_t pfpp_vq_train_workspace(int64_t R, int64_t K);
/* pfpp_sa_pool_bwd: backward of max_p relu(BN(y)) over groups of `pool` rows (pn2_utils.py:210-214, BatchNorm on the batch
 * statistics mean / var): dh [groups * pool, C] = dout[g, c] on the first row of group g that attains the max when it is > 0,
 * 0 elsewhere.  h is recomputed from y with pfpp_bn_apply's arithmetic.
 * pfpp_bn_relu_bwd: backward of h = relu(BN_train(y)) (nn.BatchNorm2d in .train(), pn2_utils.py:211-213): dz = dh (h > 0);
 * pass 1 reduces sum dz and sum dz xhat per channel over all rows in fp64 (dbeta += , dgamma += ), pass 2 writes
 * dy = gamma / sqrt(var + eps) (dz - mean dz - xhat mean(dz xhat)).  dy may alias dh.  amax (optional, device [1]): max |dy|
 * taken in the second pass (the gradient scale of the GEMMs that read dy).  C in {64, ..., 1024};
 * workspace: pfpp_bn_relu_bwd_workspace(rows, C) bytes.
 * pfpp_group_gather_bwd: backward of pfpp_group_gather's feature columns: dfeats [F, N, D] = sum over the slots (s, k) with
 * idx[f, s, k] = p of dA[(f S + s) ns + k, :D]  (a gather per point, no float atomics; overwrites dfeats).                 */
int pfpp_sa_pool_bwd(const float* y, int64_t groups, int64_t pool, int64_t C, int64_t ld, const float* mean, const float* var,
                     const float* gamma, const float* beta, float eps, const float* dout, float* dh, pfpp_stream_t stream);
int pfpp_bn_relu_bwd(const float* y, const float* dh, int64_t rows, int64_t C, int64_t ld, const float* mean, const float* var,
                     const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, float* dy, float* amax,
                     void* workspace, pfpp_stream_t stream);
int64_t pfpp_bn_relu_bwd_workspace(int64_t rows, int64_t C);
int pfpp_group_gather_bwd(const float* dA, int64_t lda, const int32_t* idx, float* dfeats, int64_t F, int64_t N, int64_t S,
                          int64_t ns, int64_t D, pfpp_stream_t stream);

/* ---- pc_data generation from fracture meshes (generate_pc_data.py:17-45; csrc/mesh_sample.hip) ----------------------------------
 * Batch layout: CSR over the Pt parts of B puzzles, the parts of a puzzle contiguous and in slot order.  verts fp64 [V, 3],
 * faces int32 [F, 3] (part-local vertex indices), vert_off / face_off int64 [Pt + 1], part_puzzle / part_slot int32 [Pt],
 * puz_part_off int64 [B + 1], data_id int64 [B].  Data-dependent failures are not return codes of the launching calls (the
 * kernels are only enqueued): they are recorded in `status`, one device uint64 the caller sets to all ones, and
 * pfpp_mesh_status — the one entry here that waits for its stream — turns it into PFPP_EINVAL / PFPP_EUNSUPPORTED with
 * pfpp_last_error naming the part or puzzle.
 * pfpp_mesh_face_cdf: trimesh.sample.sample_surface's weights (vqvae/dataset/dataset.py:177): area [F] = |(b-a) x (c-a)| / 2 in
 * fp64 (optional), cdf [F] = per-part inclusive prefix sum, total [Pt] = cdf of the part's last face.  A part whose total is 0 or
 * not finite, or a face index outside its part, is an EINVAL.
 * pfpp_mesh_sample_surface: sample_surface(mesh, N) per part (dataset.py:176-179): face = first j with cdf[j] >= u0 total
 * (searchsorted side='left', clamped to F - 1), (l0, l1) -= 1 when l0 + l1 > 1, then |.|, p = ((b-a) l0 + (c-a) l1) + a.
 * Uniforms u [Pt, N, 3] = (u0, l0, l1) when given; when u is NULL they are (pfpp_rng_u64(seed, split, idx) >> 11) 2^-53 with
 * idx = ((data_id max_parts + slot) N + i) 3 + k.  points [Pt, N, 3] fp64; face_idx int32 [Pt, N], scale fp64 [Pt] (max - min
 * over a part's coordinates, dataset.py:200) and ref_slot int32 [B] (first argmax of scale, :203) are optional.
 * pfpp_mesh_vertex_graph: _check_connectivity (dataset.py:85-127): graph bool [B, max_parts, max_parts], parts i != j connected iff
 * a vertex of i and one of j are equal after np.round(., 5), keys llrint(x 1e5).  max_parts <= 32.  A non-finite coordinate is an
 * EINVAL; a puzzle whose keys span 2^21 or more on an axis (about 20.97 units) is an EUNSUPPORTED.
 * pfpp_mesh_vertex_graph_workspace: from the per-puzzle vertex counts (host [B]) writes tab_off_host [B + 1] (the puzzles' hash
 * table regions, power-of-two capacities >= 2 x vertex count; its device copy is the tab_off argument, S = tab_off_host[B]) and
 * returns the workspace bytes, -1 on bad arguments.                                                                             */
int pfpp_mesh_face_cdf(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off, int64_t Pt,
                       double* area, double* cdf, double* total, uint64_t* status, pfpp_stream_t stream);
int pfpp_mesh_sample_surface(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off,
                             const double* cdf, const double* total, const int32_t* part_puzzle, const int32_t* part_slot,
                             const int64_t* data_id, const int64_t* puz_part_off, int64_t Pt, int64_t B, int64_t N, const double* u,
                             uint64_t seed, uint32_t split, int64_t max_parts, double* points, int32_t* face_idx, double* scale,
                             int32_t* ref_slot, pfpp_stream_t stream);
int64_t pfpp_mesh_vertex_graph_workspace(const int64_t* puzzle_nverts_host, int64_t B, int64_t* tab_off_host);
int pfpp_mesh_vertex_graph(const double* verts, const int64_t* vert_off, const int32_t* part_puzzle, const int32_t* part_slot,
                           const int64_t* puz_part_off, const int64_t* tab_off, int64_t Pt, int64_t B, int64_t V, int64_t S,
                           int64_t max_parts, uint8_t* graph, void* workspace, int64_t workspace_bytes, uint64_t* status,
                           pfpp_stream_t stream);
int pfpp_mesh_status(const uint64_t* status, pfpp_stream_t stream);

/* ---- the matcher's training batches from a resident mesh store (Jigsaw_matching/dataset/all_piece_matching_dataset.py;
 * csrc/matching_dataset.hip) ------------------------------------------------------------------------------------------------------
 * The store is the CSR batch above over the S puzzles of a whole split (store_part_off = its puz_part_off [S + 1], store_data_id
 * = its data_id [S]) with cdf and total of one pfpp_mesh_face_cdf call.  sel int64 [B] picks the puzzles of a batch (device; a
 * repeated index is allowed, the caller refuses indices outside [0, S)).  Every puzzle gets exactly num_points rows: puzzle b of
 * the batch owns rows [b num_points, (b + 1) num_points) of every [B num_points, .] output, so no size depends on the device.
 * Failures found on the device go into `status` (pfpp_mesh_status): a part whose area is zero or not finite, a selection outside
 * the store, parts x min_part_point > num_points, an order entry outside its piece.  max_parts <= 32.
 * pfpp_mdata_piece_counts: sample_reweighted_points_by_areas (:164-193) with areas = total: np.sum in numpy's order (below 8
 * values in sequence; else eight running sums over blocks of 8 folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest in sequence),
 * nps = int32(ceil(areas num_points / sum)), the first argmax absorbs sum(nps) - num_points, then (min_part_point > 1) pieces below
 * min_part_point are raised to it and `while delta > 0` takes the excess from the first argmax, both branches.  n_pcs int64
 * [B, max_parts] (zeros behind the puzzle's parts), piece_off int64 [B max_parts + 1] (row offsets, empty slots as empty ranges),
 * puz_piece_off int64 [B + 1] = b max_parts: the layout the matcher's head and encoder take.
 * pfpp_mdata_sample: _get_pcs's mesh.sample (:217-220) for row r of puzzle b: its piece and local row j from piece_off, sample
 * index s = order[b, r] (int32 [B, num_points], the reference's _shuffle_pc :141-148) or j; uniforms (u0, l0, l1) = u[b, o + s]
 * (float64 [B, num_points, 3], piece order, o = the piece's first row) or (pfpp_rng_u64(seed, split, idx) >> 11) 2^-53 with
 * idx = ((data_id max_parts + slot) num_points + s) 3 + k.  `split` carries the split and the epoch: split = (epoch << 1) | s
 * with s = 0 for train and 1 for val, epoch < 2^31.  The face search and the fold are pfpp_mesh_sample_surface's.  points fp64
 * [B, num_points, 3] (workspace) holds the sample at row o + s; gt_pcs float32 [B num_points, 3] = float32(point) at row r;
 * face_idx int32 [B num_points] is optional.
 * pfpp_mdata_pose: _recenter_pc and _rotate_pc (:117-139) per piece slot: c = (rows o .. o + n - 1 of points added in row order) / n,
 * part_trans float32 [B max_parts, 3] = c; part_pcs float32 [B num_points, 3] row o + j = float32((R0 x + R1 y) + R2 z) per output
 * coordinate, (x, y, z) = points[o + s] - c, no contraction.  rot float64 [B max_parts, 3, 3] gives R (part_quat is then the
 * caller's and may be NULL); with rot NULL R is the matrix of a quaternion (w, x, y, z) = (x1, x2, y1 f, y2 f), f = sqrt((1 - s1)
 * / s2), drawn by Marsaglia's rejection: attempt t < 64 reads c = 2 U(idx + 0) - 1, d = 2 U(idx + 1) - 1 for the first pair (kept
 * when c c + d d < 1) and idx + 2, idx + 3 for the second (kept when 0 < s < 1), idx = ((data_id max_parts + slot) 64 + t) 4, U
 * keyed by (seed ^ 0xA5B85C5E198ED849, split); a pair with no attempt inside gives the identity.  part_quat float32
 * [B max_parts, 4] = (w, -x, -y, -z), the quaternion of R^T (:136).  Empty slots get zeros.  rot_out float64 [B max_parts, 3, 3]
 * (optional) receives R.                                                                                                         */
int pfpp_mdata_piece_counts(const double* total, const int64_t* store_part_off, const int64_t* sel, int64_t B, int64_t S,
                            int64_t num_points, int64_t min_part_point, int64_t max_parts, int64_t* n_pcs, int64_t* piece_off,
                            int64_t* puz_piece_off, uint64_t* status, pfpp_stream_t stream);
int pfpp_mdata_sample(const double* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* face_off, const double* cdf,
                      const double* total, const int64_t* store_part_off, const int64_t* store_data_id, const int64_t* sel,
                      const int64_t* piece_off, int64_t B, int64_t S, int64_t num_points, int64_t max_parts, const int32_t* order,
                      const double* u, uint64_t seed, uint32_t split, double* points, float* gt_pcs, int32_t* face_idx, uint64_t* status,
                      pfpp_stream_t stream);
int pfpp_mdata_pose(const double* points, const int64_t* piece_off, const int64_t* store_data_id, const int64_t* sel, int64_t B,
                    int64_t S, int64_t num_points, int64_t max_parts, const int32_t* order, const double* rot, uint64_t seed,
                    uint32_t split, float* part_pcs, float* part_quat, float* part_trans, double* rot_out, pfpp_stream_t stream);

/* ---- matcher back end: descriptors -> matching_data (Jigsaw_matching/; csrc/matching.hip) ---------------------------------------
 * Batch layout: the points of all puzzles flat, [N, 128] descriptors / [N, 3] coordinates; piece_off int64 [Pt + 1] are the point
 * offsets of the Pt pieces (the pieces of a puzzle contiguous and in slot order, empty slots as empty ranges), puz_piece_off int64
 * [B + 1] the piece ranges of the puzzles.  Nothing is padded to the largest puzzle.
 * pfpp_match_classify_compact (model/jigsaw/joint_seg_align_model.py:164-170 + utils/critical_pcs.py:4-18): logit = bias + sum_k
 * relu(x_k scale_k + shift_k) w_k (BatchNorm1d in eval folded to scale / shift), label = fp32 sigmoid(logit) > 0.5; then per piece
 * the local indices of its labelled points in ascending order at the piece's offset of critical_pcs_idx [N] (zero behind them)
 * and their count in n_critical_pcs [Pt].  With labels_in (uint8 [N]) the classifier is skipped and those labels are compacted
 * (compute_label's path, :203-219); labels (uint8 [N], optional) receives the labels used.  C = 128.
 * pfpp_match_gather_rows (:110-116, :234 first two layers): out [R, 128] = relu(BatchNorm(feats[critical rows])) in piece order,
 * row_piece int32 [R] = piece_slot of the row's piece; crit_off int64 [Pt + 1] = exclusive prefix sum of n_critical_pcs, R =
 * crit_off[Pt].
 * pfpp_match_normalize_halves (:237-247): F.normalize(p = 2, eps = 1e-12) of x[:, :256] and x[:, 256:], in place.  D = 512.
 * pfpp_sinkhorn_masked (:251-268, utils/linear_solvers.py:9-247 per-sample branch, one puzzle): s [n, n] (row stride ld), piece
 * int32 [n]; L = s / tau in fp32; potentials u, v fp64 [n] start at 0; iteration k even: u_i += LSE_j((L_ij - u_i) - v_j), odd: the same for
 * v_j over i, both over the entries whose row and column pieces differ (the reference's -1e6 mask contributes exp(-2e7) = 0);
 * ds_mat [n, n] = exp((L - u) - v), exactly 0 where the pieces are equal.  The matrix is only read; column sweeps go through
 * workspace partials folded in a fixed order, so two runs agree bitwise.  workspace: pfpp_sinkhorn_workspace(n) bytes (-1 for
 * n outside [0, 65535]).  A puzzle in which fewer than two pieces have rows is the caller's to skip (every entry masked).
 * pfpp_fracture_labels (:465-484): dist[i] = sqrt(max(min_j |p_i - p_j|^2, 1e-12)) over the points j of the OTHER pieces of i's
 * puzzle (pfpp_nn_dist's arithmetic; inf when there is none), labels[i] = dist[i] < thresholds[i].  max_points = the largest
 * puzzle's point count; dist is optional.                                                                                      */
int pfpp_match_classify_compact(const float* feats, const float* bn_scale, const float* bn_shift, const float* w, float bias,
                                const uint8_t* labels_in, const int64_t* piece_off, int64_t Pt, int64_t C, float* logits,
                                uint8_t* labels, int64_t* critical_pcs_idx, int64_t* n_critical_pcs, pfpp_stream_t stream);
int pfpp_match_gather_rows(const float* feats, const float* bn_scale, const float* bn_shift, const int64_t* critical_pcs_idx,
                           const int64_t* piece_off, const int64_t* crit_off, const int32_t* piece_slot, int64_t Pt, int64_t R,
                           int64_t C, float* out, int32_t* row_piece, pfpp_stream_t stream);
int pfpp_match_normalize_halves(float* x, int64_t R, int64_t D, pfpp_stream_t stream);
int64_t pfpp_sinkhorn_workspace(int64_t n);
int pfpp_sinkhorn_masked(const float* s, int64_t ld, const int32_t* piece, int64_t n, float tau, int64_t max_iter, double* u, double* v,
                         float* ds_mat, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream);
int pfpp_fracture_labels(const float* gt_pcs, const int64_t* piece_off, const int64_t* puz_piece_off, const float* thresholds,
                         int64_t B, int64_t max_points, float* dist, uint8_t* labels, pfpp_stream_t stream);

/* ---- matcher front end: ragged PointNet++ encoder (Jigsaw_matching/model/modules/encoder/pointnet2_pointwise/; csrc/pointnet_ragged.hip)
 * Layout: the points of all pieces of all puzzles flat, [N, 3]; a level is described by CSR offsets int64 [P + 1] over the P pieces.
 * Which puzzle a piece belongs to plays no part (the reference asserts one puzzle per call, pointnet2_dynamic_utils.py:122).
 * pfpp_ragged_fps (torch_cluster.fps(x, batch, ratio, random_start) as called at pointnet2_dynamic_utils.py:123, for the L levels of
 * pointnet2_msg.py:82-85 in one launch): level_off int64 [L + 1, P + 1], row 0 the input points, row l the centroids of level l (the
 * caller's counts: ceil(fl32(fl32(ratio) fl32(n))) per piece); start int64 [L, P] the local first index per level and piece.  Level l
 * samples the centroids of level l - 1.  pfpp_fps_start's arithmetic: d = (dx dx + dy dy) + dz dz in fp32 without contraction, running
 * minimum, first argmax.  idx int64 / new_xyz float: the levels one behind the other (level l at row sum_{j<l} level_off[j + 1][P]);
 * an index is global in the flat array of the level it samples from, pieces in order, selection order inside a piece.
 * max_n = the largest piece (<= 8192 points).
 * pfpp_ragged_knn (knn(x, y, k, batch_x, batch_y) + to_dense_batch(fill_value) + the group_first fix-up, :131-136 and :197-205): for each
 * of the M queries (CSR query_off over the same P pieces) the min(K, n_piece) nearest of its piece's points by (dx dx + dy dy) + dz dz,
 * ascending, ties to the lower index, as global indices int32 [M, K]; the remaining slots repeat the first.  count int32 [M] (optional)
 * receives min(K, n_piece).  K = 3, 16 or 32; N = number of points.
 * pfpp_ragged_group (:138-146): out row (s, j), j < pool, = [ feats[g, 0:D] | xyz[g] - new_xyz[s] | 0 ] with g = idx[s ldi + j mod K]: the
 * column order of pfpp_group_gather; `pool` rows per centroid (pool % K == 0: a K = 16 scale fills a max-pool of 32 with duplicates).
 * pfpp_ragged_interp (PointNetFeaturePropagationDynamic.forward :191-217): out [N, ldo] row i = [ points1[i, 0:D1] | sum_j w_j
 * points2[idx[i, j]] ], w_j = r_j / ((r_0 + r_1) + r_2), r_j = 1 / (d_j + 1e-8), d_j = sum over the coordinates in order of
 * (a a + b b) - (2 a) b (a = xyz1[i], b = xyz2[idx[i, j]]; fp32, no contraction) for j < count[i] and 1e8 behind; idx / count are
 * pfpp_ragged_knn's with K = 3.  S == 1 is the reference's broadcast of the one centroid (:191-192; idx / count unused).  weights
 * [N, 3] (optional) receives w.  D1, D2, ldo multiples of 4, rows 16-byte aligned.                                               */
int pfpp_ragged_fps(const float* xyz, const int64_t* level_off, const int64_t* start, int64_t P, int64_t L, int64_t max_n,
                    int64_t* idx, float* new_xyz, pfpp_stream_t stream);
int pfpp_ragged_knn(const float* pts, const int64_t* pts_off, const float* queries, const int64_t* query_off, int64_t P, int64_t M,
                    int64_t N, int64_t K, int32_t* idx, int32_t* count, pfpp_stream_t stream);
int pfpp_ragged_group(const float* feats, int64_t ldf, int64_t D, const float* xyz, const float* new_xyz, const int32_t* idx,
                      int64_t ldi, int64_t K, int64_t pool, int64_t S, float* out, int64_t ldo, pfpp_stream_t stream);
int pfpp_ragged_interp(const float* xyz1, const float* xyz2, const int32_t* idx, const int32_t* count, const float* points2, int64_t D2,
                       const float* points1, int64_t D1, int64_t N, int64_t S, float* out, int64_t ldo, float* weights,
                       pfpp_stream_t stream);

/* ---- matcher middle: point-transformer and cross-attention layers (Jigsaw_matching/model/jigsaw/attention_layer.py; csrc/matching_tf.hip)
 * Layout as above: the points of all pieces of all puzzles flat, piece_off int64 [P + 1].
 * pfpp_feat_knn (knn_and_group :136-139: knn(x, x, k, batch_x, batch_x) + to_dense_batch(fill_value = N, max_num_nodes = k)): for every
 * row of feats [N, C] (row stride ld floats, so a third of a packed projection is searched in place) the min(K, n_piece) nearest
 * rows OF ITS PIECE in feature space as global indices int32 [N, K], ascending by key, ties to the lower index; the remaining slots
 * hold N.  The key is d = 0; for c = 0 .. C - 1 in order: t = a_c - b_c; d = d + t t, in fp32 without contraction, compared as (bits
 * of d, index).  C = 128, K = 16.  max_n = the largest piece as the caller states it: the entry refuses more than 8192 (the limit
 * of the encoder in front, pfpp_ragged_fps) and the kernel itself does not depend on it.  The launch has ceil(N / 64) + P workgroups
 * and each finds its piece by a linear walk over piece_off: meant for the hundreds of pieces of a batch of puzzles (P <= 65536).
 * pfpp_ptf_aggregate (PointTransformerLayer.forward :206-224 behind the projections and the two searches): per point i and slot t
 *   p_r = linear_p(xyz[idx_k[i, t]] - xyz[i]),  r = (k[idx_k[i, t]] - q[i]) + p_r,  w = softmax_t(linear_w(r)),
 *   out[i, 16 s + c] = sum_t (v[idx_v[i, t], 16 s + c] + p_r[i, t, 16 s + c]) w[i, t, c];
 * an index outside [0, N) is the reference's appended row: zero features and a zero offset (it stays in the softmax).  q, k, v
 * [N, C] share the row stride ld.  weights: PFPP_PTF_WEIGHT_FLOATS floats, BatchNorm in eval mode as (scale, shift) behind its
 * linear layer, at the offsets  0 linear_p.0.weight [3, 3] | 12 its BatchNorm scale [3] | 16 shift [3] (with the bias) | 20
 * linear_p.3.weight [128, 3] | 404 linear_p.3.bias | 532 linear_w.0 scale [128] | 660 shift [128] | 788 linear_w.2.weight [16, 128] |
 * 2836 linear_w.3 scale [16] | 2852 shift [16] (with the bias of linear_w.2) | 2868 linear_w.5.weight [16, 16] | 3124 linear_w.5.bias.
 * All products are fp32 FMAs; nothing of size [N, K, .] is written.  C = 128, K = 16.
 * pfpp_attn_rows16 (ScaledDotProductAttention :17-24 inside MultiHeadAttention :47-69, mask = None): pfpp_attn_dense's arguments
 * without a key mask for dh = 16: softmax((q scale) k^T) v per (sequence, head) from qkv [rows, 3 H 16] (q | k | v), out [rows, H 16];
 * online softmax, fp32 FMAs, one arithmetic whatever the thread's attention mode or the environment says.  Sequences of any length.
 * pfpp_layernorm128 (nn.LayerNorm(d_model, eps=1e-6) of MultiHeadAttention :45, :73 and PositionwiseFeedForward :85, :95): out[r] =
 * (x[r] - mean) / sqrt(mean((x[r] - mean)^2) + eps) gamma + beta over rows of C = 128 channels, the width pfpp_layernorm (256, 512,
 * 1024) does not cover; out may alias x.                                                                                          */
#define PFPP_PTF_WEIGHT_FLOATS 3140
int pfpp_feat_knn(const float* feats, int64_t ld, const int64_t* piece_off, int64_t P, int64_t N, int64_t C, int64_t K, int64_t max_n,
                  int32_t* idx, pfpp_stream_t stream);
int pfpp_ptf_aggregate(const float* q, const float* k, const float* v, int64_t ld, const float* xyz, const int32_t* idx_k,
                       const int32_t* idx_v, const float* weights, int64_t N, int64_t C, int64_t K, float* out, pfpp_stream_t stream);
int pfpp_attn_rows16(const float* qkv, float* out, const int32_t* seq_off, const int32_t* seq_len, int64_t n_seq, int64_t max_len,
                     int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
int pfpp_layernorm128(const float* x, const float* gamma, const float* beta, float* out, int64_t rows, int64_t C, float eps,
                      pfpp_stream_t stream);

/* ---- matcher front end: DGCNN encoder in eval mode (Jigsaw_matching/model/modules/encoder/dgcnn.py:41-56, 130-213; csrc/dgcnn.hip)
 * Layout as above: the points of all pieces flat, piece_off int64 [P + 1].  A level conv_l(get_graph_feature_dynamic(x)).max(-1) is
 * computed without the [N, 20, 2 C_in] tensor: with conv_l.0.weight = [W_a | W_b] split along its input columns, slot j of point i has
 * the pre-activation W_a x_j + (W_b - W_a) x_i, so uv = X [W_a ; W_b - W_a]^T [N, 2 C_out] is one pfpp_gemm, and BatchNorm (eval:
 * a per-channel scale, shift) and LeakyReLU commute with the extremum over the slots.
 * pfpp_dgcnn_knn (:47-48: knn(x, x, 20, batch_x, batch_x) + to_dense_batch(fill_value = N, max_num_nodes = 20)): pfpp_feat_knn's
 * arguments, key and order for K = 20 and C = 3, 64 or 128: for every row of feats [N, C] (row stride ld floats) the min(K, n_piece)
 * nearest rows OF ITS PIECE (the row itself included) as global indices int32 [N, K], ascending by key, ties to the lower index; the
 * remaining slots hold N.  The key is d = 0; for c = 0 .. C - 1 in order: t = a_c - b_c; d = d + t t, in fp32 without contraction,
 * compared as (bits of d, index).  Rows of 64 / 128 channels must be 16-byte aligned (ld % 4 == 0); rows of 3 need ld >= 3 only.
 * max_n = the largest piece as the caller states it (more than 8192 is refused); ceil(N / 64) + P workgroups, P <= 65536.
 * pfpp_dgcnn_edge_max (:49-56 + conv_l + .max(dim=-1), :175-189): uv [N, 2 C_out] (row stride ld; u = columns [0, C_out), v the
 * rest), idx int32 [N, K]; per point i and channel c
 *   z_j = u[idx[i, j], c] + v[i, c]   (one fp32 add)   for idx[i, j] in [0, N),    z_j = 0 for any other index (the padded slot:
 *                                                       the reference multiplies both halves of that slot's feature by the mask)
 *   e   = max_j z_j where scale[c] >= 0,  min_j z_j where scale[c] < 0      (slots in order: e = z_0; e = z_j > e ? z_j : e, resp. <)
 *   y   = e scale[c] + shift[c]   (one fp32 multiply, then one fp32 add; not fused)
 *   out[i ldo + c] = y > 0 ? y : y slope.
 * out points at the first column to write of a buffer with row stride ldo (x1 .. x4 land in the [N, 512] operand of conv5).
 * C_out = 64, 128 or 256, K = 20; ld, ldo multiples of 4 and every pointer 16-byte aligned.
 * pfpp_leaky_relu (nn.LeakyReLU(negative_slope) of conv5, :158-160): x[r ld + c] = x > 0 ? x : x slope in place over [rows, C];
 * C and ld multiples of 4, x 16-byte aligned.                                                                                    */
int pfpp_dgcnn_knn(const float* feats, int64_t ld, const int64_t* piece_off, int64_t P, int64_t N, int64_t C, int64_t K, int64_t max_n,
                   int32_t* idx, pfpp_stream_t stream);
int pfpp_dgcnn_edge_max(const float* uv, int64_t ld, const int32_t* idx, const float* scale, const float* shift, float slope, int64_t N,
                        int64_t C_out, int64_t K, float* out, int64_t ldo, pfpp_stream_t stream);
int pfpp_leaky_relu(float* x, int64_t rows, int64_t C, int64_t ld, float slope, pfpp_stream_t stream);

/* ---- matcher front end, training: the DGCNN encoder in .train() under autograd (dgcnn.py:41-56, 130-213; csrc/dgcnn_train.hip) in the
 * decomposed form above.  In train mode the BatchNorm of a level (nn.BatchNorm2d over [1, C, N, 20], :141-155) normalises with the
 * statistics of ALL R = 20 N slot rows of the call, padded all-zero rows included; z_ij = u[idx_ij] + v[i] is never stored.
 * C_out = 64, 128 or 256, K = 20, rows of ld floats (ld % 4 == 0), pointers 16-byte aligned (winner: 4-byte).  workspace:
 * PFPP_DGCNN_TRAIN_WS_DOUBLES doubles whatever the sizes are.  No atomics: two runs agree bitwise.
 * pfpp_dgcnn_edge_stats (conv_l = Conv2d + BatchNorm2d in .train() + the max over the slots, :141-155, :189-203): one gather pass over u;
 *   e[i C + c] = max_j z_ij where gamma[c] >= 0, min_j z_ij where gamma[c] < 0, by comparisons in slot order (the first slot wins a
 *   tie); winner[i C + c] = that slot (0 .. 19, a padded slot included); the sums of z and z^2 over all 20 N rows as fp64 partials per
 *   workgroup (a workgroup takes ceil(N / G) consecutive points), folded in a fixed order and left at workspace[PFPP_DGCNN_TRAIN_MAX_WG *
 *   512 ..] as sum z [C] | sum z^2 [C]; coef [4 C] = a | b | mean | rstd with rstd = 1 / sqrt(var + eps) (biased variance), a = gamma
 *   rstd, b = beta - mean a; running_mean / running_var (optional, together) move by `momentum` with the unbiased variance.  N >= 1.
 * pfpp_dgcnn_bn_leaky_apply (BatchNorm + nn.LeakyReLU, :141-160): out[r ldo + c] = t > 0 ? t : t slope with t = y a + b as one fp32
 *   multiply and one fp32 add, not fused; coef as above (or pfpp_ragged_bn_stats' for conv5, :158-160).  C % 4 == 0, C <= 1024.
 * pfpp_dgcnn_bn_leaky_bwd (autograd of the same): g = g1 + g2 (g2 optional), h[r C + c] = y a + b > 0 ? g : g slope (the forward's
 *   operations), dbeta = sum_r h, dgamma = sum_r h (y - mean) rstd as fp64 partials folded in a fixed order, means [2 C] = dbeta /
 *   count | dgamma / count.  dy (optional, may alias h): dy = a ((h - m1) - (y - mean) rstd m2), the BatchNorm backward when the rows
 *   are all of its rows (conv5: count = rows).  For a level y = e, rows = N, count = 20 N and the two gathers below finish the step.
 * pfpp_dgcnn_edge_bwd_dv / pfpp_dgcnn_edge_bwd_du (autograd of get_graph_feature_dynamic + conv_l + max, :41-56, :189-203): with n_i the
 *   real slots of i and c_p the number of (i, j) with idx_ij = p,
 *     dv[i] = a (h_i [the winning slot of i is real] - n_i m1 - m2 rstd (sum_{j real} u[idx_ij] + n_i (v[i] - mean)))
 *     du[p] = a (sum_{(i,j): idx_ij = p} h_i [winner_i = j] - c_p m1 - m2 rstd (c_p (u[p] - mean) + sum_{(i,j): idx_ij = p} v[i]))
 *   written to duv [N, 2 C_out] = du | dv.  du walks inverse lists: the flat positions e = 20 i + j whose index is p are
 *   ent[off[p] .. off[p + 1]), of any length (n_ent = the number of real slots; the padded slots have no list).  The sums run in fp64
 *   in list order and are rounded once.                                                                                           */
#define PFPP_DGCNN_TRAIN_MAX_WG 1024
#define PFPP_DGCNN_TRAIN_WS_DOUBLES (PFPP_DGCNN_TRAIN_MAX_WG * 512 + 1024)
int pfpp_dgcnn_edge_stats(const float* uv, int64_t ld, const int32_t* idx, const float* gamma, const float* beta, double eps, double momentum,
                          float* running_mean, float* running_var, int64_t N, int64_t C_out, int64_t K, float* e, unsigned char* winner,
                          float* coef, double* workspace, pfpp_stream_t stream);
int pfpp_dgcnn_bn_leaky_apply(const float* y, int64_t rows, int64_t C, int64_t ld, const float* coef, float slope, float* out, int64_t ldo,
                              pfpp_stream_t stream);
int pfpp_dgcnn_bn_leaky_bwd(const float* y, int64_t ld, const float* g1, int64_t ldg1, const float* g2, int64_t ldg2, int64_t rows, int64_t C,
                            const float* coef, float slope, double count, float* h, float* dgamma, float* dbeta, float* means, float* dy,
                            double* workspace, pfpp_stream_t stream);
int pfpp_dgcnn_edge_bwd_dv(const float* uv, int64_t ld, const int32_t* idx, const unsigned char* winner, const float* h, const float* coef,
                           const float* means, int64_t N, int64_t C_out, int64_t K, float* duv, pfpp_stream_t stream);
int pfpp_dgcnn_edge_bwd_du(const float* uv, int64_t ld, const int64_t* off, const int32_t* ent, int64_t n_ent, const unsigned char* winner,
                           const float* h, const float* coef, const float* means, int64_t N, int64_t C_out, int64_t K, float* duv,
                           pfpp_stream_t stream);

/* ---- matcher head, training behind part_feats (Jigsaw_matching/model/jigsaw/joint_seg_align_model.py in .train(); csrc/matching_train.hip)
 * Train-mode BatchNorm + ReLU, the linear layers, the affinity products and Adam go through pfpp_bn_stats / pfpp_bn_apply /
 * pfpp_bn_relu_bwd, pfpp_gemm / pfpp_gemm_grad and pfpp_adamw; these entries are the rest of the step.
 * pfpp_sinkhorn_train_fwd (utils/linear_solvers.py:188-207 unmasked, as called at joint_seg_align_model.py:266-268 in training, and
 * utils/loss.py:26-56 for one puzzle): s [n, n] (row stride ld); L = s / tau in fp32; fp64 potentials from 0; step k even: u_i +=
 * LSE_j((L_ij - u_i) - v_j), odd: the same for v_j over i; the vector step k wrote is kept in pots [max_iter, n] (fp64).  ds_mat [n, n]
 * = exp((L - u) - v); loss [1] (fp64) = sum_ij BCE(ds_mat_ij, [j == tgt_i]) with both logs clamped at -100, summed in fp64 in a fixed
 * order; tgt int32 [n], -1 = a row without a target (no dense gt_perm is built); row_loss (optional, fp64 [n]) receives the rows' shares.
 * pfpp_sinkhorn_train_bwd (autograd of those lines): ds [n, n] (row stride ldg) = dLoss / ds, g = the upstream scale (w_mat_loss /
 * sum_b n_b).  With G = dLoss / d log P: G_T = (P - y) P / max(P (1 - P), 1e-12) g (F.binary_cross_entropy's backward times P);
 * for k = max_iter - 1 .. 0, P_k = exp((L - u_k) - v_k) from the stored potentials: even k: G -= P_k * rowsum(G), odd k: G -= P_k *
 * colsum(G); ds = G_0 / tau.  G is ds itself, updated in place; the sums are fp64, the column sums through ordered partials; no
 * float atomics, two runs agree bitwise; max_iter + 1 passes over the matrix, nothing of size [max_iter, n, n] is kept.
 * workspace (both): pfpp_sinkhorn_train_workspace(n) bytes, -1 for n outside [0, 65535].
 * pfpp_match_gt_targets (joint_seg_align_model.py:333-364): src int64 [R] = the global point index of every critical row (the rows
 * of a puzzle contiguous, puz_row_off int64 [B + 1]), row_piece int32 [R] its piece; tgt int32 [R] = the puzzle-local column of the
 * nearest critical point of ANOTHER piece of the puzzle, by max(-2 a.b + |a|^2 + |b|^2, 1e-12) in fp32, an exact tie to the lowest
 * column; -1 where no other piece has a critical point (the reference's argmin lands in the own piece and `mask` zeroes it).
 * max_rows = the largest puzzle's row count (<= 65535).
 * pfpp_match_normalize_halves_bwd (:237-247): backward of pfpp_match_normalize_halves from the rows x before the normalisation:
 * dx = dy / |x| - x (x . dy) / |x|^3 per half, dy / eps where |x| < eps = 1e-12.  dx may alias dy.  D = 512.
 * pfpp_match_cls_bce (:298-323): loss [1] (fp64) = mean binary_cross_entropy_with_logits(logits, labels) (fp32 per element, fp64 sum, fixed
 * order), dlogit (optional) = (sigmoid(logit) - y) g / N, counts int64 [4] = (tp, fp, tn, fn) of fp32 sigmoid(logit) > 0.5 against
 * the label (what torchmetrics' binary accuracy / precision / recall / f1 are made of).  logits / dlogit are read / written with the
 * strides ldl / ldd (a column of a wider matrix).  workspace: at least pfpp_match_cls_bce_workspace() bytes (workspace_bytes).
 * pfpp_match_gather_raw (:110-116): out [R, 128] = feats[idx[r]] without BatchNorm or ReLU, a zero row where idx[r] is outside
 * [0, N) (the zero padding of critical_feats up to the batch's largest N').  pfpp_match_scatter_raw: its transpose, out[idx[r]]
 * = or += in[r] (accumulate); each point may occur at most once (plain stores, no atomics).                                      */
int64_t pfpp_sinkhorn_train_workspace(int64_t n);
int pfpp_sinkhorn_train_fwd(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt, double* pots,
                            float* ds_mat, double* loss, double* row_loss, void* workspace, int64_t workspace_bytes,
                            pfpp_stream_t stream);
int pfpp_sinkhorn_train_bwd(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt, const double* pots,
                            const float* ds_mat, float g, float* ds, int64_t ldg, void* workspace, int64_t workspace_bytes,
                            pfpp_stream_t stream);
int pfpp_match_gt_targets(const float* gt_pcs, int64_t N, const int64_t* src, const int32_t* row_piece, const int64_t* puz_row_off,
                          int64_t B, int64_t max_rows, int32_t* tgt, pfpp_stream_t stream);
int pfpp_match_normalize_halves_bwd(const float* x, const float* dy, float* dx, int64_t R, int64_t D, pfpp_stream_t stream);
int64_t pfpp_match_cls_bce_workspace(void);
int pfpp_match_cls_bce(const float* logits, int64_t ldl, const uint8_t* labels, int64_t N, float g, double* loss, float* dlogit,
                       int64_t ldd, int64_t* counts, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream);
int pfpp_match_gather_raw(const float* feats, const int64_t* idx, int64_t N, int64_t R, int64_t C, float* out, pfpp_stream_t stream);
int pfpp_match_scatter_raw(const float* in, const int64_t* idx, int64_t N, int64_t R, int64_t C, int accumulate, float* out,
                           pfpp_stream_t stream);

/* ---- matcher head, training: the rigid term (Jigsaw_matching/utils/loss.py:59-142 with utils/pairwise_alignment.py:11-79, called at
 * model/jigsaw/joint_seg_align_model.py:379-392 once w_rig_loss > 0; csrc/matching_rigid.hip, the seeded backward in
 * csrc/matching_train.hip).  The reference loops over the piece pairs of every puzzle in Python and solves Horn's 4 x 4 eigenproblem
 * per pair in numpy on the host; here the term and its gradient are four kernels and nothing is read back.
 * A puzzle's n critical rows are in piece order: piece_off int32 [P + 1] (puzzle-local, piece_off[P] = n, P <= 64) are the pieces'
 * first rows; pts float32 [n, 3] = the critical points taken from part_pcs in row order.  For a pair p < q with n1, n2 > 0 rows:
 * W = ds_mat[I_p, I_q] + ds_mat[I_q, I_p]^T, r_i = sum_j W_ij, b_i = sum_j W_ij T_j (S = pts[I_p], T = pts[I_q]), mat_s = sum_i r_i.
 * pfpp_rigid_pair_sums (loss.py:89-97, :124-127): one pass over ds_mat [n, n] (row stride ld): rb fp64 [n, P, 4] receives (r_i, b_i) of
 * every row i against every LATER piece q; the other slots are not written.  The transposed half is read along its rows and
 * transposed through LDS.  any_pos int32 [1] (zeroed by the caller) is set when an entry of ds_mat is positive (:75, :98).
 * pfpp_rigid_pair_pose (pairwise_alignment.py:11-79, loss.py:109-135): all pairs of a batch in one launch, a wave per pair.  pairs int32
 * [npairs, 4] = (puzzle, p, q, unused) in pair order; puz_row_off int64 [B + 1] = the puzzles' first rows in the batch-wide pts [R, 3]
 * and rb [R, P, 4]; piece_off int32 [B, P + 1]; n_valid int32 [B]; any_pos int32 [B].  Unweighted centroids, M = sum_i (S_i - cS)
 * (b_i - r_i cT)^T, Horn's N, a cyclic Jacobi of ten sweeps from the identity in fp64, the eigenvector of the FIRST of the largest
 * eigenvalues (N = 0 gives R = 1, as LAPACK does for the reference), t = sum_i (b_i - r_i R S_i) / mat_s; R [npairs, 9] and t
 * [npairs, 3] are rounded to fp32 and constant from here on.  stats fp64 [npairs, 8] = (mat_s, pair_loss = sum_i |r_i (R S_i + t) -
 * b_i|^2, the four eigenvalues ascending, n1, n2); status int32 [npairs]: 1 kept, 0 skipped (:98: n_valid > 2, mat_s == 0 and a
 * positive entry), -1 where the reference divides 0 by 0 (mat_s == 0 otherwise; pair_loss and t are stored as 0).
 * pfpp_rigid_fold (:134-135, :142): out fp64 [4] = (rig_loss = sum pair_loss mat_s / n_sum over the kept pairs, in pair order;
 * w_rig_loss / n_sum; n_sum = sum n1; the numerator).  Where the reference is not finite - a status of -1 anywhere, or nothing kept -
 * rig_loss and the scale are 0: the term is reported as 0 and has zero gradient.  npairs = 0 is that case, not an error.
 * pfpp_rigid_grad (autograd of :120-135 with R, t constant): dP [n, n] (row stride ldg) = d(w_rig_loss rig_loss) / d ds_mat of one
 * puzzle: with a the row in the earlier piece and c the row in the later one, out[1] (2 mat_s e_a . (A_a - T_c) + pair_loss), the
 * same for [a, c] and [c, a]; exact zeros in diagonal blocks and in pairs not kept.  pair_index int32 [P, P]: the pair of (p, q), p <
 * q, or -1.  pts, piece_off, rb are the puzzle's own (offset by its first row); R, t, stats, status the batch's; fold = out above.
 * All sums fp64 in a fixed order, no float atomics: two runs agree bitwise.  n = 0 and npairs = 0 launch nothing.
 * pfpp_sinkhorn_train_bwd_seeded: pfpp_sinkhorn_train_bwd with ds holding a further term's dLoss' / d ds_mat on entry (zero padding
 * columns included): G_T = the BCE term + P * seed, then the same max_iter passes; a zero seed gives pfpp_sinkhorn_train_bwd's result.
 * pfpp_match_colsum_ordered: out[c] = sum_r x[r, c] over x [rows, cols] (row stride ld), OVERWRITTEN: fp64 partials of 64 rows in row
 * order, folded in block order, rounded once.  The head's two bias gradients: pfpp_colsum ends in float atomics whose order differs
 * from run to run, and the step is compared bitwise between runs.  workspace: pfpp_match_colsum_ordered_workspace(rows, cols) bytes
 * (-1 for rows < 0 or cols < 1); rows = 0 writes zeros.                                                                           */
int pfpp_rigid_pair_sums(const float* ds_mat, int64_t ld, int64_t n, const float* pts, const int32_t* piece_off, int64_t P, double* rb,
                         int32_t* any_pos, pfpp_stream_t stream);
int pfpp_rigid_pair_pose(int64_t npairs, const int32_t* pairs, const int64_t* puz_row_off, const int32_t* piece_off, int64_t P,
                         const int32_t* n_valid, const int32_t* any_pos, const double* rb, const float* pts, float* R, float* t,
                         double* stats, int32_t* status, pfpp_stream_t stream);
int pfpp_rigid_fold(int64_t npairs, const double* stats, const int32_t* status, double w_rig_loss, double* out, pfpp_stream_t stream);
int pfpp_rigid_grad(int64_t n, const float* pts, const int32_t* piece_off, int64_t P, const double* rb, const int32_t* pair_index,
                    const float* R, const float* t, const double* stats, const int32_t* status, const double* fold, float* dP,
                    int64_t ldg, pfpp_stream_t stream);
int pfpp_sinkhorn_train_bwd_seeded(const float* s, int64_t ld, int64_t n, float tau, int64_t max_iter, const int32_t* tgt,
                                   const double* pots, const float* ds_mat, float g, float* ds, int64_t ldg, void* workspace,
                                   int64_t workspace_bytes, pfpp_stream_t stream);
int64_t pfpp_match_colsum_ordered_workspace(int64_t rows, int64_t cols);
int pfpp_match_colsum_ordered(const float* x, int64_t ld, int64_t rows, int64_t cols, float* out, void* workspace, int64_t workspace_bytes,
                              pfpp_stream_t stream);

/* ---- matcher, validation metrics of one puzzle (Jigsaw_matching/model/jigsaw/joint_seg_align_model.py:366-377 with utils/loss.py:26-56
 * on the masked doubly-stochastic matrix, and :405-415, which the reference runs as per-puzzle Python over N' x N' matrices;
 * csrc/matching_train.hip).  ds_mat [n, n] contiguous = the masked Sinkhorn output (same-piece entries exactly 0), tgt int32 [n] from
 * pfpp_match_gt_targets (-1 = no target), col int64 [n] = the assignment's column of every row.  loss [1] (fp64) = sum_ij BCE(ds_mat_ij,
 * [j == tgt_i]), both logs clamped at -100, exactly pfpp_sinkhorn_train_fwd's loss of the same matrix, summed in fp64 in a fixed order
 * (two runs agree bitwise; no float atomics).  counts int64 [3] = (tp, fp, fn): tp = #{i: col_i == tgt_i}, fp = n - tp, fn = #{i: tgt_i
 * >= 0} - tp, i.e. pred . gt, pred . (1 - gt), (1 - pred) . gt for a perm_mat with one 1 per row.  One launch; 1 <= n <= 65535. */
int pfpp_match_val_metrics(const float* ds_mat, int64_t n, const int32_t* tgt, const int64_t* col, double* loss, int64_t* counts,
                           pfpp_stream_t stream);

/* ---- matcher, assignment: the optimal assignment of a batch of puzzles on the device (hungarian / _hung_kernel,
 * Jigsaw_matching/utils/linear_solvers.py:279-340, which hands every puzzle's matrix to scipy.optimize.linear_sum_assignment on the
 * host, one after the other; csrc/matching_assign.hip).  For each puzzle b: c[b] = a device pointer to its float32 [n_b, n_b]
 * contiguous matrix (the masked Sinkhorn output); the result maximises sum_i c[i, col_i] over permutations.  c, n and max_steps are
 * HOST arrays of length B; the outputs are device arrays in which puzzle b owns the n_b entries behind those of the puzzles before
 * it (col int64, u and v fp64: the duals of cost = -(double)c) and entry b (status int32, steps and augmentations int64).
 * The algorithm, in fp64 additions, subtractions and comparisons only (bit for bit pfpp_hip.matching_assign.assign_reference):
 * u_i = min_j cost_ij, v = 0; column j goes to the lowest row whose lowest minimal column it is; the rows left free are taken in
 * ascending order, each by one shortest augmenting path whose step relaxes the unscanned columns from the current row,
 * r = ((minv + cost_ij) - u_i) - v_j, and scans the unscanned column with the smallest (dist, assigned, index), an unassigned one
 * being the sink; then u and v of the scanned set move by minv - dist_j as in scipy's solver.  One workgroup per puzzle, all
 * puzzles of a launch concurrently, PFPP_MATCH_ASSIGN_MAX_PUZZLES to a launch (their descriptors travel in the kernel arguments).
 * max_steps[b] bounds the search steps of puzzle b over all its searches: when it is used up status[b] = 1 and col of that
 * puzzle is unspecified (status 0 = solved; 2 = a search found no column within finite reach, i.e. the matrix holds NaN or infinite
 * entries, col unspecified as well); no loop of the kernels is unbounded.  workspace: pfpp_match_assign_workspace(B, n)
 * bytes (-1 for B < 1, a null n or an n_b outside 1..PFPP_MATCH_ASSIGN_MAX_N), 4-byte aligned.  Two runs agree bitwise.        */
#define PFPP_MATCH_ASSIGN_MAX_N 8192
#define PFPP_MATCH_ASSIGN_MAX_PUZZLES 64
int64_t pfpp_match_assign_workspace(int64_t B, const int64_t* n);
int pfpp_match_assign(int64_t B, const float* const* c, const int64_t* n, const int64_t* max_steps, int64_t* col, double* u, double* v,
                      int32_t* status, int64_t* steps, int64_t* augmentations, void* workspace, int64_t workspace_bytes,
                      pfpp_stream_t stream);

/* ---- matcher, edges and correspondences: the pair rule of compute_global_transformation on the device
 * (Jigsaw_matching/model/modules/matching_base_model.py:298-359 up to the _save_data call, which turns the assignment into `edges` and
 * per-edge correspondence lists one puzzle at a time on the host), together with the flattening of those lists that the assembly
 * loop does before its edge features (puzzlefusion_plusplus/auto_aggl.py:92-126 here, get_distance_for_matching_pts,
 * utils/node_merge_utils.py:62-89, in the reference); csrc/matching_edges.hip.  All B puzzles of a batch in one launch, a workgroup
 * per puzzle; integer arithmetic only; bit for bit pfpp_hip.matching_edges.pack_matches_reference.
 * Inputs (device, in the dtypes the head holds them): col int64 [total_rows] = the assignment as pfpp_match_assign writes it, one
 * column per row, local to the puzzle, -1 = unmatched; row_off int64 [B + 1]: puzzle b owns the N'_b = row_off[b + 1] - row_off[b]
 * rows from row_off[b] (zero rows: no edges); n_critical_pcs int64 [B, P]; n_valid int64 [B]; piece_off int64 [B P + 1] = point
 * offsets of the pieces in slot order (pfpp_hip.matching.Layout.piece_off); critical_pcs_idx int64 [total_points], flat.
 * max_rows >= every N'_b, total_rows and total_points are stated by the HOST; a puzzle whose device-side sizes contradict them
 * or each other gets status 2 and is not read further.
 * The rule, for every idx1 < idx2 < n_valid with critical points in both pieces: the block (rows of idx1, columns of idx2) of the
 * assignment, or its transposed opposite (rows of idx2, columns of idx1) when that holds STRICTLY more matches; a pair with fewer
 * than 3 matches is dropped; its rows (ordinal in idx1, ordinal in idx2) in lexicographic order.
 * Outputs (device, int32, as pfpp_edge_histogram takes them), T = P (P - 1) / 2 triangle slots in row-major order:
 *   counts [B, P, P]     matches per (piece of the row, piece of the column)
 *   edge_off [B, T + 1]  offsets of the slots' correspondences, relative to the puzzle's slice; a dropped pair is an empty range
 *   kept [B, T]          1 = the slot is an edge
 *   corr [total_rows, 2] the piece-local critical ordinals (what the matching_data file holds), puzzle b from row row_off[b]
 *   idx_a, idx_b [total_rows]  point indices within the puzzle: start(part) + critical_pcs_idx[start(part) + ordinal]
 *   status [B]           0 fine; 1 col is not injective on its matched rows; 2 an entry of col outside [-1, N'_b), or sizes that
 *                        contradict each other (N'_b > max_rows or > sum n_critical_pcs, n_valid outside [0, P], an n_critical_pcs
 *                        outside [0, points of the piece], offsets that decrease or leave the stated totals)
 * The kept blocks are disjoint sets of rows, so a puzzle has at most N'_b correspondences and its slice of corr / idx_a / idx_b is
 * its slice of col; entries behind its last correspondence are not written.  A puzzle with non-zero status gets zero counts and no
 * edges.  A puzzle's result does not depend on the rest of the batch; two runs agree bitwise; no loop is unbounded.
 * PFPP_EUNSUPPORTED before any launch for P outside 1..PFPP_MATCH_EDGES_MAX_P, max_rows > PFPP_MATCH_EDGES_MAX_ROWS or
 * B > PFPP_MATCH_EDGES_MAX_PUZZLES; B = 0 does nothing.  workspace (the inverse permutation, kept in global memory so that N' is
 * not bounded by LDS): pfpp_match_edges_workspace(total_rows) bytes (-1 for a negative count), 4-byte aligned; corr 8-byte aligned.
 * col, corr, idx_a, idx_b and workspace may be null when total_rows = 0, critical_pcs_idx when total_points = 0.                  */
#define PFPP_MATCH_EDGES_MAX_P 32
#define PFPP_MATCH_EDGES_MAX_ROWS 65535
#define PFPP_MATCH_EDGES_MAX_PUZZLES 65535
int64_t pfpp_match_edges_workspace(int64_t total_rows);
int pfpp_match_edges(const int64_t* col, const int64_t* row_off, const int64_t* n_critical_pcs, const int64_t* n_valid,
                     const int64_t* piece_off, const int64_t* critical_pcs_idx, int64_t B, int64_t P, int64_t max_rows,
                     int64_t total_rows, int64_t total_points, int32_t* counts, int32_t* edge_off, int32_t* kept, int32_t* corr,
                     int32_t* idx_a, int32_t* idx_b, int32_t* status, void* workspace, int64_t workspace_bytes, pfpp_stream_t stream);

/* ---- matcher middle, training: the backward of the cross-attention layer tf_cross1 (Jigsaw_matching/model/jigsaw/attention_layer.py in
 * .train() under autograd; csrc/matching_tf_train.hip).  The layer has no dropout (:15, :44, :86, :92 are commented out) and its
 * norms are nn.LayerNorm: its training-time forward is the eval forward.  The linear layers' gradients go through pfpp_gemm in its
 * exact-fp32 mode, the bias gradients through pfpp_colsum; these entries are the rest.
 * pfpp_attn_rows16_train (:17-24 inside :47-69): pfpp_attn_rows16 with one more output, lse [rows, H] = log sum_j exp((q scale) . k_j)
 * per (row, head).  out is bit for bit what pfpp_attn_rows16 writes, in both launch forms, chosen by the same size rule.
 * pfpp_attn_rows16_bwd (autograd of :17-24 and of the head split / merge :55-69): dqkv [rows, 3 H 16] = dq | dk | dv from qkv, out and
 * lse of the forward and dout [rows, H 16].  Two passes that recompute p = exp(s - lse), s formed as the forward forms it: dq with a
 * query per lane over staged key tiles (D = dout . out per (row, head) is computed in its prologue and written to dvec, a workspace
 * [rows, H]), then dk | dv with a key per lane over staged query tiles.  ds = p (dout . v - D), dq = sum_j ds k scale, dk = sum_i ds q
 * scale, dv = sum_i p dout.  fp32 FMAs, no atomics, no cross-lane step: two runs agree bitwise; a sequence reads and writes its own
 * rows; rows outside every sequence are not written.  The grid form is chosen by the sizes alone with the forward's rule.  dh = 16.
 * pfpp_layernorm128_bwd (autograd of :73 and :95): x = the rows BEFORE the normalisation; mean and rstd are recomputed with
 * pfpp_layernorm128's arithmetic.  With xh = (x - mean) rstd and g = dy gamma: dx (=, or += with accumulate_dx: the residual branch's
 * gradient is already there) rstd (g - mean(g) - xh mean(g xh)); dgamma = sum_r dy xh and dbeta = sum_r dy are OVERWRITTEN, through one
 * fp32 partial per wave of at most PFPP_LAYERNORM128_BWD_MAX_WG workgroups folded in fp64 in a fixed order (no atomics).  workspace:
 * PFPP_LAYERNORM128_BWD_WS_FLOATS floats, whatever rows is.  dx may alias dy when accumulate_dx is 0.  rows = 0 writes nothing.  C = 128.
 * pfpp_relu_bwd (autograd of F.relu :91): dh[r, c] = h[r, c] > 0 ? dh[r, c] : 0 in place over [rows, cols] with the row stride ld of
 * both; h = the ReLU's output (or its input: the sign test is the same).                                                           */
#define PFPP_LAYERNORM128_BWD_MAX_WG 256
#define PFPP_LAYERNORM128_BWD_WS_FLOATS (PFPP_LAYERNORM128_BWD_MAX_WG * 4 * 2 * 128)
int pfpp_attn_rows16_train(const float* qkv, float* out, float* lse, const int32_t* seq_off, const int32_t* seq_len, int64_t n_seq,
                           int64_t max_len, int64_t H, int64_t dh, float scale, pfpp_stream_t stream);
int pfpp_attn_rows16_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dvec /* workspace [rows, H] */,
                         float* dqkv, const int32_t* seq_off, const int32_t* seq_len, int64_t n_seq, int64_t max_len, int64_t H,
                         int64_t dh, float scale, pfpp_stream_t stream);
int pfpp_layernorm128_bwd(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, float* workspace,
                          int64_t rows, int64_t C, float eps, int accumulate_dx, pfpp_stream_t stream);
int pfpp_relu_bwd(const float* h, float* dh, int64_t rows, int64_t cols, int64_t ld, pfpp_stream_t stream);

/* ---- matcher middle, training: the point-transformer layer tf_self1 (attention_layer.py:159-225 in .train() under autograd;
 * csrc/matching_ptf_train.hip) behind the projection GEMM and the two searches.  Its three norms are BatchNorm1d over the channels of
 * [N, 16, C]: the training forward normalises with the statistics of all 16 N rows of the call (padded slots included, biased variance,
 * eps) and moves the running buffers (momentum, unbiased variance).  q, k, v, xyz, idx_k, idx_v, ld as in pfpp_ptf_aggregate.
 * pack: PFPP_PTF_TRAIN_FLOATS floats.  The caller fills the raw weights:
 *   [0, 9) linear_p[0].weight, [12, 15) linear_p[0].bias, [36, 420) linear_p[3].weight [128][3], [420, 548) linear_p[3].bias,
 *   [1060, 3108) linear_w[2].weight [16][128], [3108, 3124) linear_w[2].bias, [3188, 3444) linear_w[5].weight [16][16],
 *   [3444, 3460) linear_w[5].bias;
 * the entries write the rest: per BatchNorm scale = gamma rstd | shift = beta - mean scale | rstd | -mean rstd at 16 / 548 / 3124 (vectors
 * of 3 in slots of 4, of 128, of 16), and the backward's means of dz | dz x hat at 3460 (BatchNorm(16)) and 3492 (BatchNorm(128)).
 * Every per-channel sum is an fp64 partial per workgroup (at most PFPP_PTF_TRAIN_MAX_WG) in workspace (PFPP_PTF_TRAIN_WS_DOUBLES doubles,
 * whatever N is), folded in a fixed order into sums (fp64, device): no atomics, two runs agree bitwise.  Nothing with N 16 128 elements
 * is written; u, w, du are [N, 16, 16].  pre_dump (may be null; tests): the float32 values the launch compares with 0.
 * Forward, in this order:
 *   pfpp_ptf_train_bn3_stats    sums [6] = sum a | sum a^2, a = linear_p[0](g_p)
 *   pfpp_ptf_train_bn_finalise  which = 0 (BatchNorm(3)), 1 (128), 2 (16); rows = 16 N: sums [2 C] -> pack, running buffers
 *   pfpp_ptf_train_bn128_stats  sums [256] of r = x_k[ik] - x_q + p_r; pre_dump [N, 16, 3]
 *   pfpp_ptf_train_tile         u [N, 16, 16] = linear_w[2](relu(bn(r))), sums [32]; pre_dump [N, 16, 128]
 *   pfpp_ptf_train_finish       w [N, 16, 16] = the softmax weights, out [N, 128]; pre_dump [N, 16, 16]
 * Backward of sum(out dout), in this order:
 *   pfpp_ptf_train_bwd_w        dz2 [N, 16, 16]; sums [PFPP_PTF_TRAIN_BWD_W_SUMS] = dW5 [16][16] | db5 | sum dz2 = dbeta | sum dz2 x hat = dgamma
 *   pfpp_ptf_train_bwd_u        du <- the input gradient of BatchNorm(16), IN PLACE over dz2; sums [.._BWD_U_SUMS] = dW2 [16][128] | dbeta [128] | dgamma [128]
 *   pfpp_ptf_train_bwd_r        dqkv[:, 0:128] = dx_q; sums [.._BWD_R_SUMS] = dW3 [128][3] | db3 [128] | 27 moments over all rows with dz0 the
 *                               gradient at the BatchNorm(3) output, xh0 its normalised input, d = g_p: sum dz0_m [3] | sum dz0_m xh0_m [3] |
 *                               sum dz0_m d_l [3][3] | sum xh0_m d_l [3][3] | sum d_l [3]
 *   pfpp_ptf_train_bwd_gather   dqkv[:, 128:256] = dx_k, [:, 256:384] = dx_v: row m sums the entries e = point 16 + slot of ent_k[off_k[m] ..
 *                               off_k[m + 1]) (the slots whose idx_k is m; ascending) in that order, likewise for v; a row in no list gets zeros
 * The gradients of linear_p[0].bias and linear_w[2].bias are zero in exact arithmetic (a batch-statistics BatchNorm follows) and are
 * not computed.                                                                                                                    */
#define PFPP_PTF_TRAIN_FLOATS 3748
#define PFPP_PTF_TRAIN_MAX_WG 1024
#define PFPP_PTF_TRAIN_BWD_W_SUMS 304
#define PFPP_PTF_TRAIN_BWD_U_SUMS 2304
#define PFPP_PTF_TRAIN_BWD_R_SUMS 539
#define PFPP_PTF_TRAIN_WS_DOUBLES (PFPP_PTF_TRAIN_MAX_WG * PFPP_PTF_TRAIN_BWD_U_SUMS)
int pfpp_ptf_train_bn3_stats(const float* xyz, const int32_t* idx_k, const float* pack, int64_t N, int64_t K, double* workspace, double* sums,
                             pfpp_stream_t stream);
int pfpp_ptf_train_bn_finalise(const double* sums, int64_t which, int64_t rows, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* pack, pfpp_stream_t stream);
int pfpp_ptf_train_bn128_stats(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, const float* pack, int64_t N,
                               int64_t C, int64_t K, double* workspace, double* sums, float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_tile(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, const float* pack, int64_t N,
                        int64_t C, int64_t K, float* u, double* workspace, double* sums, float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_finish(const float* v, int64_t ld, const float* xyz, const int32_t* idx_k, const int32_t* idx_v, const float* pack, int64_t N,
                          int64_t C, int64_t K, const float* u, float* w, float* out, float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_bwd_w(const float* dout, const float* w, const float* u, const float* v, int64_t ld, const float* xyz, const int32_t* idx_k,
                         const int32_t* idx_v, float* pack, int64_t N, int64_t C, int64_t K, float* dz2, double* workspace, double* sums,
                         float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_bwd_u(const float* q, const float* k, int64_t ld, const float* xyz, const int32_t* idx_k, float* pack, int64_t N, int64_t C,
                         int64_t K, const float* u, float* du, double* workspace, double* sums, float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_bwd_r(const float* dout, const float* w, const float* du, const float* q, const float* k, int64_t ld, const float* xyz,
                         const int32_t* idx_k, const float* pack, int64_t N, int64_t C, int64_t K, float* dqkv, int64_t ldg, double* workspace,
                         double* sums, float* pre_dump, pfpp_stream_t stream);
int pfpp_ptf_train_bwd_gather(const float* dout, const float* w, const float* du, const float* q, const float* k, int64_t ld, const float* xyz,
                              const float* pack, int64_t N, int64_t C, int64_t K, const int64_t* off_k, const int32_t* ent_k,
                              const int64_t* off_v, const int32_t* ent_v, float* dqkv, int64_t ldg, pfpp_stream_t stream);

/* ---- matcher front end, training: the ragged PointNet++ encoder in .train() under autograd (pointnet2_pointwise/pointnet2_msg.py:48-94,
 * pointnet2_dynamic_utils.py; csrc/pointnet_ragged_train.hip) around the exact-fp32 GEMMs.  Sampling, search, grouping and interpolation
 * are the forward's entries.  Each of the 33 convolutions in front of conv1 is followed by a BatchNorm on the statistics of ALL rows of the call and a ReLU
 * (pointnet2_dynamic_utils.py:147-150 BatchNorm2d over [1, C, K, S]; :220-222 BatchNorm1d over [1, C, N]).  C % 4 == 0, C <= 1024; rows of
 * ld floats, ld % 4 == 0, 16-byte aligned.  workspace: PFPP_RAGGED_TRAIN_WS_DOUBLES doubles whatever the sizes are.  No atomics: two runs
 * agree bitwise.
 * pfpp_ragged_bn_stats (nn.BatchNorm2d / 1d in .train(), :150 and :222): sums of y and y^2 per channel over the rows, one fp64 partial per
 *   workgroup (a workgroup takes ceil(rows / G) consecutive rows, G = min(PFPP_RAGGED_TRAIN_MAX_WG, ceil(rows / 64))), folded in a fixed
 *   order; coef [4 C] = a | b | mean | rstd with rstd = 1 / sqrt(var + eps) (biased variance), a = gamma rstd, b = beta - mean a;
 *   running_mean / running_var (optional, together) move by `momentum` with the unbiased variance, in fp64, rounded once (eps and
 *   momentum are doubles, as in torch).  rows >= 2.
 * pfpp_ragged_bn_apply (:150 F.relu(bn(conv)) and the max over the K rows of a neighbourhood :151): out [rows, ldo] = max(fma(y, a, b), 0);
 *   with pool > 0 out [rows / pool, ldo] = the max over each `pool` consecutive rows and winner int32 [rows / pool, C] (optional) = the first
 *   row of the group that attains it, -1 when every row is <= 0.
 * pfpp_ragged_pool_bwd (autograd of torch.max(., 2)[0] :151): dh [groups pool, C] = dout[g, c] (row stride ldd) on the winning row as
 *   pfpp_ragged_bn_apply finds it, 0 elsewhere.
 * pfpp_ragged_bn_relu_bwd (autograd of :150 / :222): dz = dh where fma(y, a, b) > 0 — the forward's expression, bit for bit — else 0;
 *   dbeta = sum dz and dgamma = sum dz xhat (fp64 sums, OVERWRITTEN), xhat = (y - mean) rstd; dy [rows, C] = gamma rstd ((dz - mean dz) -
 *   xhat mean(dz xhat)).  dh is [rows, C] contiguous; dy may alias dh.
 * pfpp_ragged_group_bwd (autograd of the gathers :138-142): dfeats[p, 0:D] (=, or += with accumulate) sum over the entries e of
 *   ent[off[p] .. off[p + 1]) in that order of dA[(e / K) pool + e % K, 0:D]; e = s K + j names slot j of centroid s (idx [S, K] flat),
 *   off int64 [Np + 1], ent int32 [S K] ascending per point.  A point in no list gets zeros (or keeps its value).  The coordinate columns
 *   D .. D + 2 of dA are not read: the coordinates are inputs.
 * pfpp_ragged_interp_bwd (autograd of :208-211): dpoints2[s, 0:D2] = sum over the entries e = 3 i + j of ent[off[s] .. off[s + 1]) of
 *   weights[e] dout[i, D1 : D1 + D2] (padded slots included: they carry the first index and the weight 1e8 gives); S == 1 (:191-192, the
 *   broadcast; weights / off / ent unused): dpoints2[0] = the column sums over all N rows, fp64 partials folded in a fixed order.     */
#define PFPP_RAGGED_TRAIN_MAX_WG 256
#define PFPP_RAGGED_TRAIN_WS_DOUBLES (PFPP_RAGGED_TRAIN_MAX_WG * 2 * 1024 + 1024)
int pfpp_ragged_bn_stats(const float* y, int64_t rows, int64_t C, int64_t ld, const float* gamma, const float* beta, double eps, double momentum,
                         float* running_mean, float* running_var, float* coef, double* workspace, pfpp_stream_t stream);
int pfpp_ragged_bn_apply(const float* y, int64_t rows, int64_t C, int64_t ld, const float* coef, float* out, int64_t ldo, int64_t pool,
                         int32_t* winner, pfpp_stream_t stream);
int pfpp_ragged_pool_bwd(const float* y, int64_t groups, int64_t pool, int64_t C, int64_t ld, const float* coef, const float* dout, int64_t ldd,
                         float* dh, pfpp_stream_t stream);
int pfpp_ragged_bn_relu_bwd(const float* y, const float* dh, int64_t rows, int64_t C, int64_t ld, const float* coef, const float* gamma,
                            float* dgamma, float* dbeta, float* dy, double* workspace, pfpp_stream_t stream);
int pfpp_ragged_group_bwd(const float* dA, int64_t lda, int64_t D, const int64_t* off, const int32_t* ent, int64_t S, int64_t K, int64_t pool,
                          int64_t Np, float* dfeats, int64_t ldf, int accumulate, pfpp_stream_t stream);
int pfpp_ragged_interp_bwd(const float* dout, int64_t ldo, int64_t D1, int64_t D2, const float* weights, const int64_t* off, const int32_t* ent,
                           int64_t N, int64_t S, float* dpoints2, double* workspace, pfpp_stream_t stream);

/* ---- matcher, evaluation: piece-pair poses by RANSAC and the ragged nearest distance (Jigsaw_matching/utils/estimate_transform.py:8-66
 * called at model/modules/matching_base_model.py:338; utils/eval_utils.py's chamfer terms; csrc/matching_pose.hip).  The reference gives
 * one piece pair at a time to open3d's registration_ransac_based_on_correspondence on the host (ransac_n = 3, 50,000 draws at most, early
 * stop by confidence); here all H hypotheses of all E pairs of a batch are scored in one launch, every one of them, with counter-based
 * draws.
 * pfpp_ransac_pairs: pts float32 [R, 3]; pair_off int64 [E, 2] = the first rows of pair e's source and target piece in pts; corr int32
 * [corr_off[E], 2] = (i, j), piece-local: correspondence k of pair e (corr_off int64 [E + 1], M_e = corr_off[e + 1] - corr_off[e] >= 3)
 * matches S_k = pts[pair_off[e, 0] + i] to T_k = pts[pair_off[e, 1] + j].  Hypothesis h < H of pair e: (x0, x1, x2, -) =
 * Philox4x32-10(key = (seed & 0xffffffff, seed >> 32), counter = (h, e, 0, 0)); i0 = mulhi32(x0, M), i1 = mulhi32(x1, M - 1), plus one
 * if >= i0, i2 = mulhi32(x2, M - 2), plus one if >= min(i0, i1), then plus one if >= max(i0, i1).  Its pose is Horn's closed form
 * (pairwise_alignment.py:11-79) with unit weights on the three correspondences in fp64: centroids, M = sum (S - cS) (T - cT)^T, N,
 * the ten-sweep Jacobi of pfpp_rigid_pair_pose, the eigenvector of the first of the largest eigenvalues, t = cT - R cS.  Its score:
 * count = #{k : |R S_k + t - T_k|^2 < max_dist^2} and sumsq = the sum of those squared distances in correspondence order, fp64.  A
 * hypothesis whose two largest eigenvalues differ by no more than 1e-9 max |N_ij| is degenerate and scores count = -1.  The winner has
 * the largest count, then the smallest sumsq, then the smallest h: a total order, so the result does not depend on the grid.
 * Outputs per pair: Rout [E, 9], tout [E, 3] (fp32, rounded once from fp64); stats fp64 [E, 2] = (sumsq, the inliers the refinement
 * used); info int32 [E, 3] = (best h, count, status).  status bit 0: a non-degenerate winner exists - otherwise R = 1, t = cT - cS over
 * all correspondences, h = count = -1; bit 1 (refine != 0 only): the pose is Horn's over the winner's inliers (unit weights, fp64 sums
 * in a fixed order) - not set, and the three-point pose kept, when fewer than 3 inliers or a degenerate N.  count and sumsq are the
 * three-point pose's either way.  counts_out int32 [E, H] (may be null; tests): every hypothesis's count.  The matched points are
 * staged PFPP_RANSAC_TILE correspondences at a time; a larger pair is walked in tiles.  Indices are clamped into pts for memory safety
 * only.  workspace: pfpp_ransac_pairs_workspace(E, H) bytes (-1 for E < 0 or H < 1), 8-byte aligned.  E = 0 launches nothing.
 * pfpp_nn_dist_ragged: pfpp_nn_dist over `segments` segments of unequal sizes in one launch: for i in [src_off[s], src_off[s + 1]):
 * out[i] = min over j in [dst_off[s], dst_off[s + 1]) of |src[i] - dst[j]|^2, bit for bit pfpp_nn_dist's arithmetic; +inf where the
 * segment has no target; an empty segment writes nothing.  src_off, dst_off int64 [segments + 1] on the device; max_n >= the longest
 * source segment (it sizes the grid).                                                                                              */
#define PFPP_RANSAC_TILE 1024
int64_t pfpp_ransac_pairs_workspace(int64_t E, int64_t H);
int pfpp_ransac_pairs(const float* pts, int64_t R, int64_t E, const int64_t* pair_off, const int32_t* corr, const int64_t* corr_off, int64_t H,
                      double max_dist, uint64_t seed, int refine, float* Rout, float* tout, double* stats, int32_t* info, int32_t* counts_out,
                      void* workspace, int64_t workspace_bytes, pfpp_stream_t stream);
int pfpp_nn_dist_ragged(const float* src, const int64_t* src_off, const float* dst, const int64_t* dst_off, float* out, int64_t segments,
                        int64_t max_n, pfpp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PFPP_H_ */
