/* egovlp_hip.h -- C ABI of libegovlp_hip.so: the MI355X (gfx950) kernels behind the EgoVLP
 * EgoClip pre-training hot path.
 *
 * The reference (showlab/EgoVLP) has NO native boundary: its hot path is reached through Python
 * `nn.Module`s and every device kernel is implicit ATen/cuBLAS/cuDNN.  This header is the
 * boundary a maintainer binds instead: each entry point below replaces the implicit kernels issued
 * by the cited reference lines.  The binding is ctypes (egovlp_amd/_lib.py).
 *
 * Conventions
 *  - plain pointers + sizes only; all pointers are DEVICE pointers (HBM) unless noted; buffers are
 *    BORROWED for the duration of the enqueue (the caller -- PyTorch's caching allocator -- owns them);
 *  - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it (graph-capturable:
 *    no allocation, no synchronisation, no host readback inside);
 *  - return value: 0 = ok, 1 = invalid argument (nothing enqueued), >=2 = 2 + hipError_t of the launch;
 *  - re-entrant and stateless (called from the autograd engine thread and DDP hooks as well);
 *  - bf16 tensors are raw uint16 bit patterns.  "split planes" (x_hi, x_lo): x_hi = bf16(x),
 *    x_lo = bf16(x - x_hi); x_lo may be NULL wherever `passes == 1` / documented optional;
 *  - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef EGOVLP_HIP_H
#define EGOVLP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t egv_bf16;

/* Version of this ABI (struct layouts, argument lists, mode / format codes).  egv_version() returns the number the LIBRARY was built
 * with and egv_abi_check() compares a caller's view of it -- version and the sizes of the ABI structs -- with the library's: a
 * binding generated from another header fails loudly at load time instead of passing garbage in trailing fields (round 5 grew
 * egv_block_geom and the mode bits without either).                                                                              */
#define EGV_ABI_VERSION 6

enum { EGV_ACT_NONE = 0, EGV_ACT_GELU = 1, EGV_ACT_GELU_BWD = 2, EGV_ACT_RELU_BWD = 3 };

/* Every format and mode code of this ABI, named once; what each means stands at the field or argument that takes it.  The Python
 * mirror is the CODES table of egovlp_amd/_lib.py; tests/test_abi.py holds the two together, name by name.                       */
/* egv_gemm_desc.out_fmt: the format of (out_hi, out_lo) */
enum { EGV_OUT_BF16_SPLIT = 0, EGV_OUT_F16X2 = 1, EGV_OUT_F16 = 2, EGV_OUT_F16_SPLIT = 3, EGV_OUT_F16_GRAD = 4 };
/* egv_gemm_desc.aux_bf16: what aux_in / aux_out hold */
enum { EGV_AUX_F32 = 0, EGV_AUX_Z_BF16 = 1, EGV_AUX_DGELU_BF16 = 2, EGV_AUX_DGELU_F16 = 3 };
/* the format of the attention output planes: a field of the mode word of egv_divided_attn_fwd / _bwd */
enum { EGV_ATTN_OUT_BF16_SPLIT = 0, EGV_ATTN_OUT_BF16_F16 = 1, EGV_ATTN_OUT_F16X2 = 2, EGV_ATTN_OUT_F16 = 3 };
/* the mode word of egv_divided_attn_fwd / _bwd: EGV_ATTN_TIME | fmt << EGV_ATTN_OUT_SHIFT | the FWD_ or BWD_ bits of the call */
enum { EGV_ATTN_TIME = 1, EGV_ATTN_OUT_SHIFT = 1, EGV_ATTN_OUT_MASK = 3,
       EGV_ATTN_FWD_QKV_F16 = 8, EGV_ATTN_BWD_GRAD_F16 = 8, EGV_ATTN_BWD_QKV_F16 = 16 };
/* dx_fmt of egv_layernorm_bwd_fmt / _partial: bits */
enum { EGV_LN_DX_F16 = 1, EGV_LN_DY_F16 = 2 };
/* role of egv_f16x2_encode[_multi] */
enum { EGV_F16X2_FIRST = 0, EGV_F16X2_SECOND = 1, EGV_F16X2_GRAD_CAST = 2 };
/* egv_block_geom.train: bits */
enum { EGV_TRAIN_KEEP = 1, EGV_TRAIN_CLS_TAIL = 2 };
/* egv_block_geom.f16_single: bits, one per pair of Linears */
enum { EGV_SINGLE_FC1 = 1, EGV_SINGLE_FC2 = 2, EGV_SINGLE_QKV = 4, EGV_SINGLE_PROJ = 8 };
/* kv_fmt / d_fmt of egv_cls_attn_fwd / _bwd */
enum { EGV_CLS_KV_BF16 = 0, EGV_CLS_KV_F16 = 1 };
/* dx_mode of egv_cls_linear_dgrad */
enum { EGV_CLS_DX_STORE = 0, EGV_CLS_DX_ADD_F32 = 1, EGV_CLS_DX_ADD_F16 = 2 };

/* ---- GEMM --------------------------------------------------------------------------------------
 * C[M,N] = alpha * A[M,K] . B[N,K]^T, then (in this order) + bias[n], activation, + residual[m,n].
 * Replaces nn.Linear / Conv2d-as-GEMM forward, dgrad and wgrad: model/video_transformer.py:41-50
 * (Mlp fc1/fc2), :70,76 (patch-embed conv), :88-89,103,135 (qkv/proj); HF DistilBERT q/k/v/out_lin,
 * ffn.lin1/lin2; model/model.py:72-79 (projections).  passes = 1: bf16 operands (hi planes only);
 * passes = 3: split-bf16 operands, fp32-grade product (three bf16 MFMA products); passes = 2: "f16x2" operands (see
 * egv_f16x2_encode: a_hi / a_lo = the two fp16 planes of a first-operand encoding, b_hi / b_lo of a second-operand encoding;
 * big-tile NT kernel only, un-split) -- the same fp32-grade product from TWO fp16 MFMA products; passes = 4: ONE fp16 MFMA product of
 * plain fp16 planes (a_hi = fp16(A), b_hi = fp16(B) = plane 1 of a second-operand f16x2 encoding; a_lo / b_lo ignored; big-tile NT
 * kernel only, un-split; epilogues: bias + residual -> fp32 / split planes, or EGV_ACT_GELU -> EGV_OUT_F16X2 / EGV_OUT_F16) -- 2^-11 per operand:
 * for the Linears whose share of the 1e-3 parity budget allows it -- and, with trans == 1, the weight gradient of the
 * FP16 BACKWARD (dW = dY^T X on fp16(S dY) and the forward's fp16 activation plane, split-K allowed; alpha rescales the product --
 * 1 / (1 - 2^-6) when X is plane 1 of an f16x2 first-operand encoding -- but not the column sums).  Requirements: K % 32 == 0, N % 4 == 0,
 * lda % 8 == ldb % 8 == 0, 16-byte aligned base pointers.
 *  act = EGV_ACT_GELU      : v = gelu(v); if aux_out != NULL the pre-activation is stored there first
 *  act = EGV_ACT_GELU_BWD  : v *= gelu'(aux_in[m,n])           (fc2 dgrad -> dZ; aux_in NULL is an invalid argument)
 *  act = EGV_ACT_RELU_BWD  : v  = aux_in[m,n] > 0 ? v : 0      (likewise)
 * Outputs: any subset of out_f32 / (out_hi[, out_lo]).  Split-K (ksplit > 1, used by wgrad where
 * K = #tokens): raw partial sums go to partial[ksplit][M][N] and a second kernel reduces them into
 * out_f32 (ldo must equal N; accumulate == 1 adds to the existing contents; accumulate == 2, trans == 1 only: the slabs are left
 * un-reduced for egv_splitk_reduce_multi); no epilogue then.
 * What "no epilogue" means, per kernel (csrc/gemm_dispatch.h says which one a shape takes): a split-K launch of the 128x128 kernel applies
 * the WHOLE epilogue in its reduce (alpha, bias, activation, residual, every output; accumulate must be 0); a split-K launch of the
 * big-tile kernel writes the plain sum of the products to out_f32 -- NT: alpha, bias, act and residual are NOT applied even when given;
 * trans == 1: alpha scales the products (not the column sums).  `accumulate` is read by that slab reduce only: an un-split launch
 * (ksplit <= 1) overwrites its outputs whatever `accumulate` says.
 * Plane outputs of EGV_ACT_GELU / EGV_ACT_GELU_BWD from the big-tile kernel require N % 8 == 0 (the columns two tiles share are computed
 * twice, and only then bit-identically: gemm_dispatch.h); every other combination takes any N % 4 == 0.   */
typedef struct egv_gemm_desc {
  const egv_bf16* a_hi; const egv_bf16* a_lo; int64_t lda;
  const egv_bf16* b_hi; const egv_bf16* b_lo; int64_t ldb;
  int32_t M, N, K, passes;
  float alpha;
  int32_t act;
  const float* bias;
  const float* residual; int64_t ldr;
  const float* aux_in; float* aux_out; int64_t ldaux;
  float* out_f32; int64_t ldo;
  egv_bf16* out_hi; egv_bf16* out_lo; int64_t ldoh;
  int32_t ksplit, accumulate;
  float* partial;
  int32_t trans;    /* (see below) */
  int32_t aux_bf16; /* a CODE, not a flag (the name is older than its values): what aux_in / aux_out [M, ldaux] hold.
                       EGV_AUX_F32: the fp32 pre-activation.  Every other code is 16 bits per element, big-tile kernel and the GELU
                       epilogues only.  EGV_AUX_Z_BF16: the pre-activation as bf16 (saved by fc1 for fc2's dgrad: half the bytes
                       when backward runs single-pass bf16 anyway).
                       EGV_AUX_DGELU_BF16: bf16 of gelu'(pre-activation) itself -- EGV_ACT_GELU stores the derivative (it has
                       Phi and phi in registers) and EGV_ACT_GELU_BWD multiplies by the stored value, no second erf.
                       EGV_AUX_DGELU_F16: the same derivative stored as FP16 (passes == 2 / 4 launches only; plane outputs and
                       neither out_f32 nor residual next to them -- anything else is an invalid argument: only the plane epilogue
                       reads and writes fp16 there): the fp16 backward, where bf16's 2^-9 on gelu' would cap the accuracy of dZ.
                       trans = 0: A[M,K], B[N,K] (contraction index contiguous).  1 ("TN", wgrad): A is stored [K, lda] with
                       its M rows as COLUMNS and B is stored [K, ldb] with N columns, C[m,n] = sum_k A[k,m] B[k,n] --
                       no transposed copy of either operand is ever made (CDNA4 transpose-read from LDS).  Requires
                       M >= 256, N >= 256, both multiples of 8; K is arbitrary (rows past K are zero-filled).        */
  float* colsum;    /* trans == 1 only, optional: colsum[m] = sum_k A[k,m] (the bias gradient), from the same pass;
                       with ksplit > 1, partial must hold ksplit*M*N + ksplit*M floats.                              */
  int32_t grid_cap; /* persistent workgroups of the big-tile kernel for THIS launch: 0 = one per CU (256); data-parallel
                       callers pass e.g. 248 so that the RCCL kernels of the overlapped gradient all-reduce find free CUs.
                       Multiples of 8 in [8, 256]; anything else is an invalid argument.  (Per call, not per process: the
                       library keeps no state between calls.)                                                         */
  int32_t out_fmt;  /* format of (out_hi, out_lo).  EGV_OUT_BF16_SPLIT: split-bf16 planes.  Every other format is fp16: an un-split NT
                       launch with passes == 2 or 4 that writes planes only (out_hi given, ldoh % 8 == 0; no out_f32, no residual, a
                       16-bit aux_out if any) -- anything else is an invalid argument.
                       EGV_OUT_F16X2: the f16x2 operand format below, first-operand role (two fp16 planes; out_lo required).
                       EGV_OUT_F16: ONE plane of plain, saturating fp16 in out_hi (out_lo unused): the operand of a passes == 4
                       consumer.  Both: EGV_ACT_GELU only (fc1 -> fc2 of the forward).
                       EGV_OUT_F16_SPLIT: out_hi = fp16(v), out_lo = fp16(v - out_hi) (out_lo required), EGV_ACT_NONE only: the qkv
                       planes that the fp16 attention multiplies.
                       EGV_OUT_F16_GRAD: ONE plane of UN-CLAMPED fp16 in out_hi (a scaled gradient beyond fp16's range becomes inf,
                       which the loss-scale logic answers with a skipped step): the gradients of the fp16 backward, from a launch
                       that runs ONE fp16 product per k-tile (passes == 4; passes == 2 where csrc/gemm_dispatch.h runs it as two
                       k-segments) -- EGV_ACT_NONE without bias (dO of a plain dgrad), or EGV_ACT_GELU_BWD on a saved derivative
                       (aux_bf16 EGV_AUX_DGELU_BF16 / _F16): dZ.                                                                   */
  egv_bf16* out_bf; /* out_fmt != EGV_OUT_BF16_SPLIT, optional: bf16(value) as a further plane [M, ldoh] -- the single-pass operand the backward GEMMs
                       (wgrad) read, since an fp16 plane cannot share an MFMA with bf16 gradients.                               */
} egv_gemm_desc;
int egv_gemm_nt(const egv_gemm_desc* d, void* stream);
/* The split-K reduction of SEVERAL trans == 1 launches (weight gradients) in ONE launch: a descriptor with ksplit > 1 and
 * accumulate == 2 leaves its slabs in `partial` (ksplit x M x N products, then ksplit x M column sums) and writes nothing else;
 * this call sums them: out[i][0 .. mn[i]) = sum_z partial[i][z], colsum[i][0 .. m[i]) likewise (colsum / its entries may be NULL).
 * HOST arrays of `count` <= 8 device pointers / sizes; mn[i] = M x N of launch i (a multiple of 4), ksplit[i] >= 2.  egv_block_bwd
 * finishes the six weight gradients of a SpaceTimeBlock this way when they share one stream.                                      */
int egv_splitk_reduce_multi(int32_t count, const float* const* partial, float* const* out, const int64_t* mn, const int32_t* ksplit,
                            float* const* colsum, const int32_t* m, void* stream);
/* ---- format kernels (HBM-bound) -----------------------------------------------------------------
 * fp32 [rows, cols] -> split planes, optionally also the TRANSPOSED planes t_*[cols, ldt] (ldt >= rows,
 * columns rows..ldt-1 are zero-filled so a following GEMM can contract over a K padded to 32) and the
 * column sums colsum[cols] (= bias gradient; overwritten).  Any output may be NULL.               */
int egv_split_f32(const float* x, int64_t ldx, int32_t rows, int32_t cols,
                  egv_bf16* hi, egv_bf16* lo, int64_t ldo,
                  egv_bf16* t_hi, egv_bf16* t_lo, int64_t ldt, float* colsum, void* stream);
/* The same for `count` tensors in one launch (host arrays of device pointers / sizes; no column sums): the once-per-
 * optimizer-step refresh of every weight's operand planes W[N,K] and W^T[K,N] (~100 tensors per step).
 * t_cols[i] = columns of the transposed planes tensor i owns (rows[i] <= t_cols[i] <= ldt[i]; rows[i] .. t_cols[i]-1 are
 * zero-filled) -- several tensors may share one pair of transposed planes side by side (DistilBERT's fused q/k/v weight).
 * Everything is validated before the first launch: an invalid tensor anywhere in the list enqueues nothing.               */
int egv_split_f32_multi(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows, const int32_t* cols,
                        egv_bf16* const* hi, egv_bf16* const* lo, const int64_t* ldo, egv_bf16* const* t_hi,
                        egv_bf16* const* t_lo, const int64_t* ldt, const int32_t* t_cols, void* stream);
/* The same with one more optional output per tensor: t16[i] (NULL entries allowed, t16 itself may be NULL) = the TRANSPOSED matrix
 * as ONE plane of plain fp16 [cols, ldt] (saturating), same geometry rules as t_hi -- W^T for the dgrad GEMMs of the fp16 backward
 * (egv_gemm_nt passes == 4 with b_hi = this plane).                                                                              */
int egv_split_f32_multi_t16(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows, const int32_t* cols,
                            egv_bf16* const* hi, egv_bf16* const* lo, const int64_t* ldo, egv_bf16* const* t_hi,
                            egv_bf16* const* t_lo, const int64_t* ldt, const int32_t* t_cols, uint16_t* const* t16, void* stream);
/* split planes [rows, cols] -> transposed planes [cols, ldt] (+ zero pad, + colsum of hi+lo).        */
int egv_transpose_planes(const egv_bf16* hi, const egv_bf16* lo, int64_t ldx, int32_t rows, int32_t cols,
                         egv_bf16* t_hi, egv_bf16* t_lo, int64_t ldt, float* colsum, void* stream);

/* ---- the f16x2 operand format (forward GEMMs of the video tower; csrc/f16x2.h) ----------------------------------------------
 * A fp32-grade product from TWO fp16 MFMA products instead of three bf16 ones.  With e = 2^-6:
 *   first operand  (activations):  a1 = fp16((1 - e) a),  a2 = fp16(a - a1)
 *   second operand (weights):      b1 = fp16(b),          b2 = fp16(b1 + (b - b1) / e)
 *   A . B^T ~= A1 B1^T + A2 B2^T :  a2 b2 = (e a - rho)(b1 + (b - b1) / e) returns the e a b1 that a1 left out, carries b's residual
 * and cancels a1's rounding error rho; the roundings that are not compensated are attenuated by e or 2^-12 / e (~2^-17 per product:
 * 5.3e-6 on random operands where split-bf16 x3 gives 4.4e-6; embeddings 3.2e-5 from the fp32 oracle where it gives 2.7e-5).
 * An operand [rows, cols] (cols % 8 == 0) is two fp16 planes [rows, ld] (ld % 8 == 0) -- the geometry of split-bf16 planes.
 * bf (optional): bf16(x) [rows, ld], the operand of single-pass backward GEMMs.  role: EGV_F16X2_FIRST = first operand, EGV_F16X2_SECOND =
 * second operand; EGV_F16X2_GRAD_CAST (egv_f16x2_encode only) = ONE plane of plain, UN-CLAMPED fp16 in p1 (p2 / bf unused): a scaled
 * gradient entering the fp16 backward as fp32.
 * Replaces nothing in the reference (fp32 there); producers: this converter (weights, tests), egv_layernorm_fwd_f16x2, the
 * EGV_ACT_GELU epilogue with out_fmt = EGV_OUT_F16X2.  Range: fp16 (saturating at 65504; below ~4e-3 a2 loses relative, not absolute, accuracy):
 * forward operands only.                                                                                                          */
int egv_f16x2_encode(const float* x, int64_t ldx, int32_t rows, int32_t cols, uint16_t* p1, uint16_t* p2, egv_bf16* bf,
                     int64_t ldo, int32_t role, void* stream);
/* `count` tensors in one launch (HOST arrays of device pointers / sizes): the once-per-optimizer-step refresh of the weights.
 * Everything is validated before the first launch: an invalid tensor anywhere in the list enqueues nothing.                       */
int egv_f16x2_encode_multi(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows, const int32_t* cols,
                           uint16_t* const* p1, uint16_t* const* p2, const int64_t* ldo, int32_t role, void* stream);
/* nn.LayerNorm (model/video_transformer.py:146,156,159 -> the qkv / fc1 Linears) with the output written in the f16x2 format,
 * first-operand role (+ optional bf16 plane); y2 == NULL: ONE plane of plain fp16 in y1 instead (the operand of a passes == 4
 * product); cols % 8 == 0, cols <= 1024; mean / rstd [rows] saved for egv_layernorm_bwd.                                          */
int egv_layernorm_fwd_f16x2(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int32_t rows,
                            int32_t cols, uint16_t* y1, uint16_t* y2, egv_bf16* ybf, int64_t ldy, float* mean, float* rstd,
                            void* stream);

/* ---- one call per SpaceTimeBlock ----------------------------------------------------------------------------------
 * SpaceTimeBlock.forward (model/video_transformer.py:163-177: t = timeattn(norm3(x)); tr = x + t; s = attn(norm1(tr)); sr = x + s;
 * out = sr + mlp(norm2(sr))) and its backward, enqueued from C: the same kernels with the same arguments in the same order as the
 * per-kernel entry points above (LayerNorm -> qkv GEMM -> divided attention -> proj GEMM, twice, then fc1 / GELU / fc2), with every
 * intermediate in ONE caller-provided arena per direction -- what costs the host ~50 tensor allocations and ~30 calls per block
 * otherwise.  Token-major [M = B (1 + T n), D] fp32 residual stream; D = 64 H.
 * fwd_passes: 3 = split-bf16 three-product, 1 = single-pass bf16, 2 = the f16x2 format (two fp16 products in the qkv / fc1 / fc2
 * Linears, or one where f16_single says so; attention and, unless the backward is fp16, the proj Linears stay split-bf16).
 * bwd_passes: 3 (fwd_passes 3 only), 1 (any forward), or 4 = ONE fp16 product on loss-scaled gradients (fwd_passes 2 only: it reads
 * the forward's own fp16 planes).  train & EGV_TRAIN_KEEP keeps what the backward needs (z_bf16 != 0: fc1 saves gelu'(z) in 16 bits -- bf16, fp16
 * for bwd_passes 4; single-product backwards, required with fwd_passes 2 -- instead of the fp32 pre-activation).  Every decision that
 * follows from these five words is made once, in csrc/block_plan.h.
 * The forward arena must stay untouched until egv_block_bwd has run on it.
 * CLS tail (train & EGV_TRAIN_CLS_TAIL; the tower's LAST block, whose output is read on the B CLS rows only -- norm(x)[:, 0], :330): `out` of
 * egv_block_fwd is the dense [B, D] fp32 CLS rows and io.g_out of egv_block_bwd their [B, D] gradient (io.g_hi NULL); d_x stays
 * [M, D].  The time branch, norm1 and the k / v rows of the space qkv Linear run over all rows as before; the space attention's CLS
 * query, the space proj, norm2, fc1 / GELU and fc2 run on B rows in fp32 from the fp32 MASTER weights (the egv_cls_* entry points
 * below).  Those masters -- contiguous W[N,K] of weights 2 .. 5 -- travel in the plane slots of the other direction, which the call
 * does not read: wt_hi[2 .. 5] for egv_block_fwd, w_hi[2 .. 5] for egv_block_bwd (cast to const float*); w_hi / w_lo[3 .. 5] (fwd) and
 * wt_hi / wt_lo[3 .. 5] (bwd) are unused.  wgrad_ksplit[2] is that of the k / v rows' gradient [2 D, D]; [3 .. 5] are ignored.  Arena
 * sizes, egv_block_fwd_offsets (-1 for planes the tail does not write; `sr` and `z` hold B rows) follow the bit; the gradient layout
 * does not.                                                                                                                     */
typedef struct egv_block_geom {
  int32_t B, T, n, H, D, Hd;
  int32_t fwd_passes, bwd_passes, train /* EGV_TRAIN_KEEP: keep what the backward needs | EGV_TRAIN_CLS_TAIL */, z_bf16;
  float eps;
  int32_t grid_cap;     /* as egv_gemm_desc.grid_cap */
  int32_t f16_single;   /* fwd_passes == 2 only: which Linears of THIS block run ONE fp16 product (egv_gemm_nt passes == 4) instead of
                           the two of the f16x2 format -- EGV_SINGLE_FC1 (norm2 then writes one plain fp16 plane), EGV_SINGLE_FC2 (the GELU
                           epilogue of fc1 then writes h as one plain fp16 plane), EGV_SINGLE_QKV: both qkv Linears (norm3 / norm1 write
                           one plain fp16 plane), EGV_SINGLE_PROJ: both proj Linears (the attention kernels write fp16(value) as their second
                           output plane; w_hi[1] / w_hi[3] are then the weights' f16x2 encodings like those of the other single-
                           product Linears).  0 elsewhere.  Which blocks may is the caller's precision policy.        */
} egv_block_geom;
typedef struct egv_block_params {                 /* weight index: 0 timeattn.qkv, 1 timeattn.proj, 2 attn.qkv, 3 attn.proj, 4 fc1, 5 fc2 */
  const float *n3w, *n3b, *n1w, *n1b, *n2w, *n2b; /* LayerNorm affine (norm3 = temporal, norm1 = spatial, norm2 = MLP)              */
  const float* bias[6];
  const egv_bf16 *w_hi[6], *w_lo[6]; int64_t ldw[6];     /* W[N,K] planes (forward)                                              */
  const egv_bf16 *wt_hi[6], *wt_lo[6]; int64_t ldwt[6];  /* W^T[K,N] planes (dgrad; may be NULL for egv_block_fwd)               */
} egv_block_params;
int64_t egv_block_fwd_arena_bytes(const egv_block_geom* g);
/* byte offsets into the forward arena of: n3_hi, timeattn-out hi, n1_hi, attn-out hi, n2_hi, h_hi, qkv_t hi, qkv_s hi, tr, sr, z   */
int egv_block_fwd_offsets(const egv_block_geom* g, int64_t* off11);
int egv_block_fwd(const egv_block_geom* g, const egv_block_params* p, const float* x, float* out, void* arena, void* stream);
/* Backward.  g_out: dL/d out fp32 [M, D]; g_hi / g_lo: the same as planes if the caller has them (else NULL: split here).
 * Outputs: d_x fp32 [M, D] and its planes dx_hi[, dx_lo]; `grads`: ONE fp32 buffer holding dW x 6, db x 6 and the three
 * LayerNorms' (dgamma, dbeta) at the offsets of egv_block_grad_layout (order: weights 0..5, biases 0..5, norm3 g/b, norm1 g/b,
 * norm2 g/b).  Weight-gradient GEMM i runs on side_stream[i] behind side_event[i] recorded on `stream` (NULL: on `stream`) with
 * wgrad_ksplit[i] k-slices (slabs in the backward arena); the caller joins the side streams.                                     */
typedef struct egv_block_bwd_io {
  const float* g_out; const egv_bf16 *g_hi, *g_lo;
  const float* x; const void* fwd_arena; void* bwd_arena;
  float* d_x; egv_bf16 *dx_hi, *dx_lo;
  float* grads;
  void* side_stream[6]; void* side_event[6];
  int32_t wgrad_ksplit[6];
} egv_block_bwd_io;
int64_t egv_block_bwd_arena_bytes(const egv_block_geom* g, const int32_t* wgrad_ksplit6);
int egv_block_grad_layout(const egv_block_geom* g, int64_t* offsets18, int64_t* total_floats);
int egv_block_bwd(const egv_block_geom* g, const egv_block_params* p, const egv_block_bwd_io* io, void* stream);

/* ---- one call per DistilBERT TransformerBlock -----------------------------------------------------------------
 * HF modeling_distilbert.py TransformerBlock.forward (:227-259; built by the reference at model/model.py:31-36 and called at :122):
 * sa = LN(out_lin(MHA(x)) + x); out = LN(lin2(gelu(lin1(sa))) + sa), and its backward, enqueued from C on ONE stream: the same
 * kernels with the same arguments in the same order as the per-kernel entry points (egv_split_f32, egv_gemm_nt, egv_text_attn_*,
 * egv_layernorm_*, egv_dropout).  The split-K factors of the M = B*L GEMMs come from the caller (>= 1 each): nt_ksplit_fwd for the
 * q/k/v (fused), out_lin, lin1, lin2 products, nt_ksplit_bwd for dZ, d_sa, d_ctx, d_x in that order, wgrad_ksplit per weight.
 * Weight index: 0 = q/k/v fused [3D, D] (rows q | k | v), 1 = out_lin, 2 = lin1, 3 = lin2.  attn_p / ffn_p: the dropout
 * probabilities (0 outside train()) with their seeds, seed_dev as in egv_text_attn_fwd.                                          */
typedef struct egv_text_geom {
  int32_t B, L, H, D, Hd;
  int32_t fwd_passes, bwd_passes, train;
  float eps, attn_p, ffn_p;
  int32_t grid_cap;
  uint64_t attn_seed, ffn_seed;
  const uint64_t* seed_dev;
  int32_t nt_ksplit_fwd[4], nt_ksplit_bwd[4], wgrad_ksplit[4];
} egv_text_geom;
typedef struct egv_text_params {
  const float *ln1w, *ln1b, *ln2w, *ln2b;          /* sa_layer_norm, output_layer_norm                                     */
  const float* bias[4];
  const egv_bf16 *w_hi[4], *w_lo[4]; int64_t ldw[4];     /* W[N,K] planes (forward)                                       */
  const egv_bf16 *wt_hi[4], *wt_lo[4]; int64_t ldwt[4];  /* W^T[K,N] planes (dgrad; may be NULL for the forward call)     */
} egv_text_params;
int64_t egv_text_layer_fwd_arena_bytes(const egv_text_geom* g);
int egv_text_layer_fwd(const egv_text_geom* g, const egv_text_params* p, const float* x /* [B*L, D] */, const int64_t* mask /* [B, L] */,
                       float* out, void* arena, void* stream);
int64_t egv_text_layer_bwd_arena_bytes(const egv_text_geom* g);
/* offsets (floats) into `grads` of: dW x 4, db x 4, sa_layer_norm dgamma, dbeta, output_layer_norm dgamma, dbeta               */
int egv_text_layer_grad_layout(const egv_text_geom* g, int64_t* offsets12, int64_t* total_floats);
int egv_text_layer_bwd(const egv_text_geom* g, const egv_text_params* p, const float* g_out, const int64_t* mask, const void* fwd_arena,
                       void* bwd_arena, float* d_x, float* grads, void* stream);

/* ---- LayerNorm ----------------------------------------------------------------------------------
 * nn.LayerNorm over the last dim (video eps 1e-6: model/video_transformer.py:146,156,159,228,253;
 * DistilBERT eps 1e-12).  Optional fused pre-add: the normalised input is x + x_add (DistilBERT's
 * post-LN `LN(sublayer + x)`), and that sum is stored to sum_out if non-NULL.  Outputs: split planes
 * and/or fp32; mean/rstd [rows] are saved for backward.                                            */
int egv_layernorm_fwd(const float* x, const float* x_add, int64_t ldx, const float* gamma, const float* beta,
                      float eps, int32_t rows, int32_t cols, float* sum_out,
                      egv_bf16* y_hi, egv_bf16* y_lo, float* y_f32, int64_t ldy,
                      float* mean, float* rstd, void* stream);
/* dx[r,:] = (add1 + add2)[r,:] + LN'(dy; x, gamma, mean, rstd)[r,:];  dgamma/dbeta [cols] overwritten.
 * dy is given EITHER as fp32 (dy) OR as split-bf16 planes (dy_hi[, dy_lo]; dy == NULL) -- the dgrad GEMM that produces
 * it can write planes directly; lddy is the leading dimension of whichever is used.
 * dx_hi/dx_lo (optional, contiguous [rows, cols]): the same dx as split-bf16 planes, i.e. already in the operand
 * format of the dgrad / wgrad GEMMs that consume it.  `work`: 2 * cols * egv_layernorm_bwd_parts(rows) floats.     */
int egv_layernorm_bwd_parts(int32_t rows);
int egv_layernorm_bwd(const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy,
                      const float* x, int64_t ldx, const float* gamma,
                      const float* mean, const float* rstd, int32_t rows, int32_t cols,
                      const float* add1, const float* add2, float* dx, int64_t lddx,
                      egv_bf16* dx_hi, egv_bf16* dx_lo, float* dgamma, float* dbeta, float* work, void* stream);
/* The same with the plane formats as an argument, dx_fmt = 0 or an OR of: EGV_LN_DX_F16 -- the dx planes are ONE plane of UN-CLAMPED
 * fp16 in dx_hi (dx_lo must be NULL) instead of split-bf16 (dx_hi[, dx_lo]): the operand of the next dgrad / wgrad GEMMs of the fp16
 * backward; EGV_LN_DY_F16 -- dy is ONE plane of un-clamped fp16 in dy_hi (dy and dy_lo NULL), what the dgrad GEMM in front writes in
 * the fp16 backward (egv_gemm_desc.out_fmt EGV_OUT_F16_GRAD): half the bytes of an fp32 dy on both sides, one more fp16 rounding of a scaled gradient.                */
int egv_layernorm_bwd_fmt(const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy,
                          const float* x, int64_t ldx, const float* gamma,
                          const float* mean, const float* rstd, int32_t rows, int32_t cols,
                          const float* add1, const float* add2, float* dx, int64_t lddx,
                          egv_bf16* dx_hi, egv_bf16* dx_lo, int32_t dx_fmt, float* dgamma, float* dbeta, float* work, void* stream);

/* The two stages of the backward as separate entry points: egv_layernorm_bwd_partial = everything but the reduction of the per-block
 * partial sums (dx [+ planes] are final; dgamma / dbeta are zeroed, `work` holds the partials), egv_layernorm_bwd_reduce = ONE launch
 * that finishes up to four such backwards of the same (rows, cols) (HOST arrays of `count` device pointers) -- egv_block_bwd reduces
 * the three LayerNorms of a SpaceTimeBlock with one launch instead of three.                                                       */
int egv_layernorm_bwd_partial(const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy,
                              const float* x, int64_t ldx, const float* gamma,
                              const float* mean, const float* rstd, int32_t rows, int32_t cols,
                              const float* add1, const float* add2, float* dx, int64_t lddx,
                              egv_bf16* dx_hi, egv_bf16* dx_lo, int32_t dx_fmt, float* dgamma, float* dbeta, float* work, void* stream);
int egv_layernorm_bwd_reduce(int32_t count, const float* const* work, int32_t rows, int32_t cols, float* const* dgamma,
                             float* const* dbeta, void* stream);

/* ---- video tokens -------------------------------------------------------------------------------
 * Patch gather for the 16x16/s16 conv (model/video_transformer.py:70-77): video [B*T,C,H,W] fp32 ->
 * A[(bt*gh + py)*gw + px][c*P*P + i*P + j] split planes, K = C*P*P (a multiple of 32 for P=16/C=3).   */
int egv_patch_gather(const float* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                     egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* The same gather straight from decoded uint8 frames [B*T,C,H,W]: ToTensor's x/255 and
 * Normalize's (x - mean[c]) / std[c] (data_loader/transforms.py:38-39; base/base_dataset.py `frames.float() / 255`) are
 * applied in the kernel, fp32, same operation order = bit-identical planes; `mean` / `std` are HOST arrays of C <= 4 floats. */
int egv_patch_gather_u8(const uint8_t* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                        const float* mean, const float* std, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* The same gather with the TRAIN transform of the loader fused in (data_loader/transforms.py:14-19): per clip a crop box
 * (top, left, h, w) and a flip flag -- boxes[B][5] int32 on the DEVICE, the host's random draws -- select the region of the
 * decoded uint8 clip [B*T, C, Hs, Ws] that is resized (bilinear, align_corners = False semantics, on x / 255) to R x R,
 * mirrored when flip != 0, normalised and written as patch planes (R % P == 0, R % 4 == 0).  The box must lie inside the frame. */
int egv_patch_gather_u8_aug(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R,
                            int32_t P, const int32_t* boxes, const float* mean, const float* std, egv_bf16* a_hi,
                            egv_bf16* a_lo, int64_t lda, void* stream);
/* egv_patch_gather_u8_aug with the transform's third stage, ColorJitter(brightness, saturation, hue) (torchvision 0.13's tensor path;
 * data_loader/transforms.py:16), between the flip and Normalize.  color[B][4] fp32 on the DEVICE, the host's draws per clip:
 * (brightness factor, saturation factor, hue shift in [-0.5, 0.5], code).  code = three base-4 digits stored exactly in the float,
 * the first applied op lowest: 0 nothing, 1 brightness, 2 saturation, 3 hue -- which ops run, in torchvision's random order.  On RGB
 * in [0, 1]: brightness clamp(f x); saturation clamp(f x + (1 - f) gray), gray = 0.2989 r + 0.587 g + 0.114 b; hue rgb -> hsv,
 * h -> (h + d) mod 1, hsv -> rgb.  The kernel reads (int)code & 63: no table value addresses anything; a non-finite factor gives NaN
 * pixels in that clip's frames only.  C == 3 and color != NULL, else EGV_ERR_ARG (nothing launched), as for everything
 * egv_patch_gather_u8_aug refuses.  Contrast (not settable in the reference's configs) is not implemented. */
int egv_patch_gather_u8_aug_color(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R,
                                  int32_t P, const int32_t* boxes, const float* color, const float* mean, const float* std,
                                  egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* The same gather with the VAL / TEST transform of the loader fused in (data_loader/transforms.py:49-60: Resize(S) -> CenterCrop(S)
 * -> Resize(R) -> Normalize, applied to x / 255 in fp32; bilinear, align_corners = False, no antialias).  `frames` is a bank of F
 * decoded uint8 frames [F, C, Hs, Ws]; output frame bt is made from bank frame index[bt] (`index`: int32 [BT] on the DEVICE, entries
 * clamped into [0, F-1]; NULL = bt, then BT <= F), so windows of a clip -- overlapping, sub-sampled, a ragged last batch -- are
 * rows of a table and the frames are never copied.  Stage 1: short side -> S, long side -> int(S * long / short); centre crop at
 * int(round((H1 - S) / 2.0)); stage 2: S x S -> R x R, every tap of it a bilinear sample of the source (four source bytes per output
 * pixel where the short side already equals S, sixteen otherwise).  Planes as egv_patch_gather_u8_aug (R % P == 0, R % 4 == 0,
 * P even, a_lo == NULL: one plane); `mean` / `std` HOST arrays of C <= 4 floats.  EGV_ERR_ARG (nothing launched) for anything else. */
int egv_patch_gather_u8_eval(const uint8_t* frames, int32_t F, const int32_t* index, int32_t BT, int32_t C, int32_t Hs,
                             int32_t Ws, int32_t S, int32_t R, int32_t P, const float* mean, const float* std,
                             egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* x[b,0,:] = cls + pos[0]; x[b,1+f*n+i,:] = pe[(b*T+f)*n+i,:] + pos[1+i] + temporal[f]
 * (model/video_transformer.py:305-320; pos tiling by the MODEL's num_frames, sliced to T).          */
int egv_assemble_tokens(const float* pe, const float* cls, const float* pos, const float* temporal,
                        int32_t B, int32_t T, int32_t n, int32_t D, float* x, void* stream);
/* backward of the above: d_pe (gather), d_cls, d_pos [n+1,D], d_temporal [T_model,D] (rows >= T zeroed). */
int egv_assemble_tokens_bwd(const float* dx, int32_t B, int32_t T, int32_t n, int32_t D, int32_t T_model,
                            float* d_pe, float* d_cls, float* d_pos, float* d_temporal, void* stream);

/* ---- patch dropout (extension; timm's VisionTransformer(patch_drop_rate), FLIP's masking; the reference's tower,
 * model/video_transformer.py:302-328, always runs all n = patches_per_frame positions) ---------------------------------------------
 * A train-mode forward keeps K of the n patch positions of every clip -- a TUBE: the same positions in all T frames, which the time
 * attention (:114, one position across frames) needs -- and the tower runs over S = 1 + T*K tokens, [CLS, frame 0's kept patches in
 * ascending position order, frame 1's ...].  keep: int32 [B, K] on the DEVICE.  Every kernel that reads the table clamps an entry
 * outside [0, n) into it, so a bad table cannot make a kernel leave its buffers.
 *
 * egv_patch_keep_draw: the key of (clip b, position j) is h = egv_mix32(egv_mix32((uint32)idx ^ s0) ^ (uint32)(idx >> 32) ^ s1),
 * idx = b*n + j, (s0, s1) = the words of `seed` XOR-ed with seed_dev[0..1] when seed_dev is given (the hash of egv_dropout /
 * egv_drop_path_*).  j is kept <=> fewer than K positions of the clip have a smaller (h, j) pair (lexicographic: ties break by
 * index); keep[b] lists the kept positions in ascending order.  One workgroup per clip, no atomics: deterministic.
 * 1 <= K <= n <= 1024, keep != NULL; EGV_ERR_ARG (nothing launched) otherwise.  K == n gives 0 .. n-1.                            */
int egv_patch_keep_draw(int32_t B, int32_t n, int32_t K, uint64_t seed, const uint64_t* seed_dev, int32_t* keep, void* stream);
/* The three gathers over the kept patches only (VideoPatchEmbed :72-77 on a subset): output row bt*K + j is patch keep[bt / T][j]
 * of frame bt, bit-identical to row bt*n + keep[bt / T][j] of egv_patch_gather / _u8 / _u8_aug (same x / 255, Normalize and bilinear
 * arithmetic, same split); columns C*P*P .. lda-1 are left untouched.  lda % 4 == 0, 1 <= K <= patches per frame.                 */
int egv_patch_gather_sel(const float* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                         const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
int egv_patch_gather_u8_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                            const float* mean, const float* std, const int32_t* keep, int32_t K, egv_bf16* a_hi,
                            egv_bf16* a_lo, int64_t lda, void* stream);
int egv_patch_gather_u8_aug_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R,
                                int32_t P, const int32_t* boxes, const float* mean, const float* std, const int32_t* keep,
                                int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* egv_patch_gather_u8_aug_color over the kept patches: the bits of its rows bt*n + keep[bt / T][j]. */
int egv_patch_gather_u8_aug_color_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R,
                                      int32_t P, const int32_t* boxes, const float* color, const float* mean, const float* std,
                                      const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
/* ---- Mixup / CutMix inside the gather (extension; timm's Mixup, the VideoMAE / MViT fine-tuning recipe -- the reference has neither)
 * The host draws two tables per batch of B = BT / T clips (data_loader/transforms.py mix_params), both on the DEVICE:
 *   mix_idx int32 [B, 6]: (partner, op, y0, y1, x0, x1);  mix_lam fp32 [B].
 * With A_x the fully transformed clip x (for the train transform: its own crop box, flip, colour row and Normalize) and p = partner,
 * the output rows of clip b hold
 *   op 1 (mixup):   lam * A_b + (1 - lam) * A_p -- on the normalised values, in exactly this order: the two products, then their sum,
 *                   (1 - lam) formed in fp32, nothing contracted; lam = 1 gives A_b's bits and lam = 0 A_p's;
 *   op 2 (cutmix):  A_p in rows [y0, y1) x columns [x0, x1) of the OUTPUT frame (H x W; R x R under the train transform), the same
 *                   box in all T frames (a tube), A_b elsewhere -- a selection: every element is a bit copy of the unmixed gather;
 *   op 0 (and 3):   A_b, the bits of the entry without a mix.
 * The partner enters unmixed (no chains).  The kernels clamp partner into [0, B) and the box into the frame and read op & 3: no table
 * value addresses anything unclamped.  keep (NULL: all patches, then K is not read): the patch-dropout table of the *_sel entries;
 * clip b's kept positions select the output rows and the partner is read at those positions.  No backward: the gather has no
 * gradient to the pixels.
 * egv_patch_gather_mix: clips that need no resampling -- u8 == 0: fp32 [B*T,C,H,W] (mean / std not read), else decoded uint8 with
 * HOST mean / std -- and otherwise the arguments and refusals of egv_patch_gather[_u8][_sel].
 * egv_patch_gather_u8_aug_mix: the fused train transform; color NULL: no jitter, else C == 3; otherwise the arguments and refusals
 * of egv_patch_gather_u8_aug[_color][_sel].  A NULL mix table is EGV_ERR_ARG, nothing launched.                                   */
int egv_patch_gather_mix(const void* video, int32_t u8, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                         const float* mean, const float* std, const int32_t* mix_idx, const float* mix_lam, const int32_t* keep,
                         int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream);
int egv_patch_gather_u8_aug_mix(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R, int32_t P,
                                const int32_t* boxes, const float* color, const float* mean, const float* std,
                                const int32_t* mix_idx, const float* mix_lam, const int32_t* keep, int32_t K, egv_bf16* a_hi,
                                egv_bf16* a_lo, int64_t lda, void* stream);
/* x[b,0,:] = cls + pos[0]; x[b,1+f*K+j,:] = (pe[(b*T+f)*K+j,:] + pos[1+keep[b][j]]) + temporal[f] (:305-320 on the kept tokens):
 * the sum order of egv_assemble_tokens, so the rows are bit-identical to the matching rows of the full assembly.                  */
int egv_assemble_tokens_sel(const float* pe, const float* cls, const float* pos, const float* temporal, const int32_t* keep,
                            int32_t B, int32_t T, int32_t n, int32_t K, int32_t D, float* x, void* stream);
/* backward of the above: d_pe [B*T*K, D], d_cls, d_pos [n+1, D] (row 1+j sums dx over the frames of the clips that kept j and is
 * exactly zero where no clip did), d_temporal [T_model, D] (rows >= T zeroed).                                                     */
int egv_assemble_tokens_bwd_sel(const float* dx, const int32_t* keep, int32_t B, int32_t T, int32_t n, int32_t K, int32_t D,
                                int32_t T_model, float* d_pe, float* d_cls, float* d_pos, float* d_temporal, void* stream);

/* ---- divided space-time attention ------------------------------------------------------------------
 * VarAttention core (model/video_transformer.py:104-133) on the fused qkv buffer [B, S, 3, H, 64] given as split-bf16
 * planes (exactly what the qkv GEMM epilogue writes; qkv_lo is ignored / may be NULL when passes == 1).
 * S = 1 + T*n, token order 1 + f*n + i.  q is scaled by 64^-0.5 inside.  mode 0 = space (group = (b,f,h): n queries x
 * (CLS + n) keys, bf16 MFMA, scores never leave LDS / registers), mode EGV_ATTN_TIME = time (group = (b,i,h): T queries x (CLS + T)
 * keys, bf16 MFMA as well).  The CLS query row (attends to all S keys, :112) rides in every group as an extra query; its
 * partials are merged by a small combine kernel.  Output: split planes [B, S, H*64]; lse [B, H, S] (log-sum-exp of each
 * query row, saved for backward).  `work`: egv_divided_attn_fwd_work_floats(...) floats.
 * Sizes: space groups of up to 288 keys (n <= 287: ViT-B/16 and ViT-L/14 at 224^2) keep K / V of a group in LDS; larger n (288^2 ..
 * 448^2 inputs) runs key-tiled kernels (64-key tiles, online softmax; the backward tiles keys and queries) with the same arguments,
 * workspaces, precision combinations and output formats.  No structural upper bound on n (S = 1 + T*n must fit int32); largest
 * size tested: n = 784 (785 keys).  Time groups: T <= 16 frames are ONE 16-row tile per location (csrc/attn_time_mfma.hip),
 * 16 < T <= 64 are 2 - 4 tiles held by one workgroup (csrc/attn_time_long.hip) with the same arguments, workspaces, precision
 * combinations and output formats; EGV_ATTN_TIME with T > 64 returns EGV_ERR_ARG (space mode has no bound on T).  head dim 64 only.
 * The mode word: mode = (0 space | EGV_ATTN_TIME) | fmt << EGV_ATTN_OUT_SHIFT | (0 | EGV_ATTN_FWD_QKV_F16).  fmt (EGV_ATTN_OUT_MASK wide;
 * any but EGV_ATTN_OUT_BF16_SPLIT with passes == 3 only) = the format of the output planes:
 *   EGV_ATTN_OUT_BF16_SPLIT  split-bf16 (out_hi = bf16(v), out_lo = bf16(v - out_hi)): a three-product proj;
 *   EGV_ATTN_OUT_BF16_F16    out_hi = bf16(v) (what a bf16 backward reads), out_lo = fp16(v): the operand of a proj Linear that runs ONE
 *                            fp16 product;
 *   EGV_ATTN_OUT_F16X2       the f16x2 operand format, first-operand role (out_hi = a1, out_lo = a2): a TWO-product proj whose backward
 *                            is fp16;
 *   EGV_ATTN_OUT_F16         out_hi = fp16(v), out_lo unused (may be NULL): a one-product proj whose backward is fp16 as well.
 * EGV_ATTN_FWD_QKV_F16 (passes == 3 only): the qkv planes are an fp16 split (egv_gemm_desc.out_fmt EGV_OUT_F16_SPLIT) and the kernels
 * multiply fp16.  Any other bit is an invalid argument.                                                                            */
int egv_divided_attn_fwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, int32_t B, int32_t T, int32_t n, int32_t H,
                         int32_t mode, int32_t passes, egv_bf16* out_hi, egv_bf16* out_lo, float* lse, float* work,
                         void* stream);
int64_t egv_divided_attn_fwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode);
/* Backward: out_* = the forward output planes, dout_* = gradient w.r.t. them (planes, e.g. from the proj dgrad
 * epilogue).  dqkv [B,S,3,H,64] is written ONCE as split planes -- every dK / dV row already contains the CLS query's
 * contribution -- i.e. directly in the operand format of the qkv dgrad / wgrad GEMMs.  Only the CLS token's own
 * gradients are accumulated in fp32 (atomics) and converted by a finish kernel.
 * `work`: egv_divided_attn_bwd_work_floats(...) floats.
 * mode: EGV_ATTN_TIME; fmt << EGV_ATTN_OUT_SHIFT = the format the forward wrote out_* in (as above: delta = rowsum(dO o O) decodes it;
 * every format but EGV_ATTN_OUT_BF16_SPLIT takes out_lo = NULL, the fp16 ones passes == 1 only); EGV_ATTN_BWD_GRAD_F16 (passes == 1
 * only) = dqkv_hi receives ONE plane of UN-CLAMPED fp16 instead of bf16 (the fp16 backward; q / k / v / dO are still read as bf16
 * planes); EGV_ATTN_BWD_QKV_F16 (with EGV_ATTN_BWD_GRAD_F16 and passes == 1 only) = q / k / v (qkv_hi: the first plane of an
 * fp16-split qkv) and dO (dout_hi) are fp16 planes: fp16 MFMA products throughout.  A refused call (EGV_ERR_ARG) enqueues nothing. */
int egv_divided_attn_bwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, const egv_bf16* out_hi, const egv_bf16* out_lo,
                         const egv_bf16* dout_hi, const egv_bf16* dout_lo, const float* lse, int32_t B, int32_t T,
                         int32_t n, int32_t H, int32_t mode, int32_t passes, egv_bf16* dqkv_hi, egv_bf16* dqkv_lo,
                         float* work, void* stream);
int64_t egv_divided_attn_bwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H);

/* ---- the CLS tail of the last video block (csrc/cls_tail.hip) ------------------------------------------------------------
 * forward_features ends with norm(x)[:, 0] (model/video_transformer.py:330): of the last SpaceTimeBlock's output only the B CLS rows
 * are read, so its space-attention output, space proj, norm2, fc1 / GELU, fc2 run on R = B rows (egv_block_fwd / _bwd with EGV_TRAIN_CLS_TAIL in
 * egv_block_geom.train).  These are the R-row pieces: Linears in plain fp32 straight from the fp32 master weights W[N,K] (latency-
 * sized: W is streamed once; no operand planes), and the attention of ONE query row per (clip, head).  Every sum runs in a fixed
 * order (no float atomics).  R >= 1; N % 4 == 0, K % 4 == 0, every leading dimension % 4 == 0, 16-byte aligned base pointers.
 *
 * y[R,N] = x[R,K] . W[N,K]^T + bias, then act (EGV_ACT_NONE / EGV_ACT_GELU, exact erf; z_out != NULL: the fp32 pre-activation is
 * stored there, [R, N] contiguous), then + residual[r, n].  x rows may be strided (ldx = S D picks the CLS rows of [B, S, D]).      */
int egv_cls_linear_fwd(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias /* or NULL */, int32_t R, int32_t N,
                       int32_t K, int32_t act, float* z_out, const float* residual /* or NULL */, int64_t ldr, float* y, int64_t ldy,
                       void* stream);
/* dX[R,K] = dY[R,N] . W[N,K]  (x gelu'(z[r,k]) when z != NULL: z = the [R, K] pre-activation egv_cls_linear_fwd saved).  dx_mode:
 * EGV_CLS_DX_STORE = dX fp32 [R, lddx] is overwritten; EGV_CLS_DX_ADD_F32 = added to the fp32 there; EGV_CLS_DX_ADD_F16 = added to a
 * plane of UN-CLAMPED fp16 (dx is uint16 [R, lddx]):
 * the B CLS rows of a gradient the big dgrad GEMM wrote for all rows.  `work`: egv_cls_linear_work_floats(R, N, K) floats.           */
int64_t egv_cls_linear_work_floats(int32_t R, int32_t N, int32_t K);
int egv_cls_linear_dgrad(const float* dy, int64_t lddy, const float* W, int64_t ldw, int32_t R, int32_t N, int32_t K, const float* z,
                         void* dx, int64_t lddx, int32_t dx_mode, float* work, void* stream);
/* the rank-R weight gradient dW[N,K] = dY[R,N]^T . X[R,K] (overwritten, row stride lddw) and db[n] = sum_r dY[r,n] (or NULL)        */
int egv_cls_linear_wgrad(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t R, int32_t N, int32_t K, float* dW,
                         int64_t lddw, float* db, void* stream);
/* dst[r, 0 .. cols) += src[r, 0 .. cols): R strided fp32 rows                                                                      */
int egv_cls_rows_add(float* dst, int64_t lddst, const float* src, int64_t ldsrc, int32_t R, int32_t cols, void* stream);
/* Attention of the CLS query (model/video_transformer.py:112: cls_out = attn(cls_q, k, v) over all S = 1 + T n keys of its clip, the
 * CLS key / value row an ordinary key): q fp32 [B, H 64] (scaled by 64^-0.5 inside), k / v = operand planes with rows b S + j and the
 * head's 64 columns at h 64 (row stride ldkv elements; value = hi + lo, lo may be NULL); kv_fmt EGV_CLS_KV_BF16 = bf16 planes,
 * EGV_CLS_KV_F16 = fp16 planes.
 * The keys are streamed (online softmax): no bound on S.  out fp32 [B, H 64]; lse [B, H] = log sum_j exp(q . k_j / 8).               */
int egv_cls_attn_fwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi, const uint16_t* v_lo,
                     int64_t ldkv, int32_t kv_fmt, int32_t B, int32_t S, int32_t H, float* out, int64_t ldo, float* lse, void* stream);
/* Backward: dq fp32 [B, H 64] (contiguous) and dK / dV of EVERY key row, written once as gradient planes of row stride lddkv --
 * d_fmt EGV_CLS_KV_BF16: split-bf16 (dk_lo / dv_lo may be NULL), EGV_CLS_KV_F16: ONE plane of un-clamped fp16 in dk_hi / dv_hi -- the operand format of the qkv
 * dgrad / wgrad GEMMs.  out / d_out fp32 [B, H 64] contiguous.                                                                      */
int egv_cls_attn_bwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi, const uint16_t* v_lo,
                     int64_t ldkv, int32_t kv_fmt, const float* out, const float* d_out, const float* lse, int32_t B, int32_t S,
                     int32_t H, float* dq, uint16_t* dk_hi, uint16_t* dk_lo, uint16_t* dv_hi, uint16_t* dv_lo, int64_t lddkv,
                     int32_t d_fmt, void* stream);

/* ---- DistilBERT pieces ----------------------------------------------------------------------------
 * Embeddings (modeling_distilbert.py:82-118): e[b,l,:] = word[ids[b,l]] + pos[l] (fp32 sum; LN is a
 * separate egv_layernorm_fwd).  Backward scatters d_e into d_word (atomic adds; d_word/d_pos must be
 * zero-initialised by the caller) and reduces d_pos.                                               */
int egv_embed_fwd(const int64_t* ids, const float* word, const float* pos, int32_t B, int32_t L, int32_t D,
                  float* e, void* stream);
int egv_embed_bwd(const int64_t* ids, const float* d_e, int32_t B, int32_t L, int32_t D, int64_t pad_id /* -1: none */,
                  float* d_word, float* d_pos, void* stream);
/* Masked multi-head attention (modeling_distilbert.py:122-203) on separate q,k,v [B, L, H*64] fp32;
 * mask [B, L] int64 (0 = padded key -> -inf).  Output split planes [B, L, H*64]; probs are recomputed
 * in backward from lse [B,H,L].  L <= 288 runs the LDS-resident kernels, longer sequences the key-tiled ones (same
 * arguments, same dropout mask function); no structural upper bound on L, largest size tested 512 (DistilBERT's positions). */
int egv_text_attn_fwd(const float* q, const float* k, const float* v, int64_t ldqkv, const int64_t* mask, int32_t B,
                      int32_t L, int32_t H, int32_t passes, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                      egv_bf16* out_hi, egv_bf16* out_lo, float* lse, void* stream);
/* q, k, v (and dq, dk, dv) rows are ldqkv (lddqkv) floats apart: H*64 for separate tensors, 3*H*64 when they are the
 * three column blocks of one fused [B*L, 3*H*64] projection output (one GEMM instead of three).
 * dropout_p > 0: HF's attention dropout (softmax -> dropout -> . V, modeling_distilbert.py eager attention) with the
 * counter-based mask keep(seed, ((b*H + h)*L + query)*L + key); the backward regenerates it from the same (dropout_p, seed).
 * seed_dev (optional, DEVICE, one uint64): XOR-ed into `seed` by the kernel when it runs -- the part of the seed that changes
 * from replay to replay of a step captured into a HIP graph (launch arguments are frozen at capture).                      */
int egv_text_attn_bwd(const float* q, const float* k, const float* v, int64_t ldqkv, const int64_t* mask,
                      const float* d_out, const float* lse, int32_t B, int32_t L, int32_t H, int32_t passes,
                      float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* dq, float* dk, float* dv,
                      int64_t lddqkv, float* delta_work /* B*H*L floats */, void* stream);
/* Zero-fill (hipMemsetAsync on `stream`) of a buffer the caller has just allocated.                                    */
int egv_zero(void* p, int64_t bytes, void* stream);
/* Elementwise dropout of DistilBERT (embedding output, FFN output): out[i] = x[i] * M'(i) + (add ? add[i] : 0) with
 * M'(i) = keep(seed, i) ? 1 / (1 - p) : 0.  The same call with x = dy is its backward.  16-byte aligned pointers.      */
int egv_dropout(const float* x, const float* add, float* out, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev,
                void* stream);

/* ---- stochastic depth of the SpaceTimeBlock (timm DropPath with scale_by_keep, model/video_transformer.py:155,171,175) ----------
 * One Bernoulli(1 - p) draw per SAMPLE and residual branch: s[b] = keep(seed, b) ? 1 / (1 - p) : 0 -- the counter-based mask of
 * egv_dropout with the element index set to the sample number b (p == 0: all ones).  A pure function of (p, seed ^ *seed_dev, b):
 * nothing is stored, the backward regenerates the forward's draws; seed_dev as in egv_text_attn_fwd.  0 <= p < 1.
 * egv_drop_path_scales: out[b] = s[b], b < B (tests, logging, reference helpers).                                                 */
int egv_drop_path_scales(int32_t B, float p, uint64_t seed, const uint64_t* seed_dev, float* out, void* stream);
/* out[m, :] = resid[m, :] + s[m / rows_per_sample] * y[m, :] on contiguous fp32 [rows, cols] (cols % 4 == 0, 16-byte aligned,
 * rows * cols / 4 < 2^31 - 2^19); `out` may be `y`.  The product and the sum are rounded separately (= `resid + s * y` of any fp32
 * host); rows of a dropped sample are copies of resid and y is not read for them.                                                 */
int egv_drop_path_add(const float* y, const float* resid, float* out, int32_t rows, int32_t cols, int32_t rows_per_sample,
                      float p, uint64_t seed, const uint64_t* seed_dev, void* stream);
/* The backward: the operand planes of s[m / rows_per_sample] * g[m, :] (g fp32 [rows, ldg], cols % 8 == 0, ldg % 4 == 0,
 * ldo % 8 == 0, 16-byte aligned), the product rounded to fp32 first.  passes 1 / 3: split-bf16 hi[, lo] planes, bit for bit what
 * egv_split_f32 writes from the scaled matrix; passes 4: ONE plane of un-clamped fp16 in `hi` (lo unused), bit for bit
 * egv_f16x2_encode role 2.                                                                                                        */
int egv_drop_path_grad(const float* g, int64_t ldg, int32_t rows, int32_t cols, int32_t rows_per_sample, float p, uint64_t seed,
                       const uint64_t* seed_dev, int32_t passes, uint16_t* hi, uint16_t* lo, int64_t ldo, void* stream);

/* ---- contrastive head ---------------------------------------------------------------------------------
 * sim_matrix x3 + EgoNCE/NormSoftmaxLoss forward AND backward in one launch
 * (model/model.py:189-197; model/loss.py:13-25,34-53; trainer/trainer_egoclip.py:130-137).
 * text, video [n, D] fp32 (the all-gathered global batch); noun [n, dn], verb [n, dv] multi-hot fp32
 * (NULL for NormSoftmaxLoss: mask = I).  Writes loss[1], sim [n,n] (optional), and the gradients of
 * the loss w.r.t. text and video [n, D] (optional).  n <= 1024 (beyond: egv_egonce_long_fwd_bwd).  `use_noun/use_verb` mirror EgoNCE's ctor. */
int egv_egonce_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb,
                       int32_t n, int32_t D, int32_t dn, int32_t dv, float temperature, float eps,
                       int32_t use_noun, int32_t use_verb,
                       float* loss, float* sim, float* d_text, float* d_video, float* work, void* stream);
int64_t egv_egonce_work_floats(int32_t n, int32_t D);
/* The same head for ANY n in [1, 65536] (D <= 256, D % 4 == 0; noun and verb both given or both NULL), with no n x n buffer: the
 * similarity tiles are recomputed on the fp32-input MFMA and streamed (csrc/egonce_long.hip), so there is no `sim` output.  The
 * workspace (egv_egonce_long_work_floats floats) is linear in n plus a bounded number of partial tiles.  Same loss and gradients as
 * egv_egonce_fwd_bwd; deterministic.  Data contract: noun / verb are non-negative multi-hots -- only (entry > 0) is used, as bits;
 * a negative or NaN entry makes the loss NaN (a device-side flag, no host sync).  d_text / d_video may each be NULL. */
int egv_egonce_long_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb,
                            int32_t n, int32_t D, int32_t dn, int32_t dv, float temperature, float eps,
                            int32_t use_noun, int32_t use_verb,
                            float* loss, float* d_text, float* d_video, float* work, void* stream);
int64_t egv_egonce_long_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv);
/* The same head in the reference's own decomposition (kept for API compatibility with code that calls
 * model.model.sim_matrix and model.loss.EgoNCE(x, mask_v, mask_n) separately):
 *  sim_matrix forward (any n, m, D): an/bn = normalised rows (saved for backward), norms [n+m], out [n,m];
 *  sim_matrix backward: g [n,m] -> da [n,D], db [m,D] (either may be NULL);
 *  EgoNCE / NormSoftmaxLoss on a given similarity matrix x [n,n] (sim_v/sim_n NULL => mask = I): loss[1], dx. */
int egv_sim_matrix_fwd(const float* a, const float* b, int32_t n, int32_t m, int32_t D, float eps,
                       float* an, float* bn, float* norms, float* out, void* stream);
int egv_sim_matrix_bwd(const float* g, const float* an, const float* bn, const float* norms, int32_t n, int32_t m,
                       int32_t D, float eps, float* da, float* db, void* stream);
int egv_egonce_from_sim(const float* x, const float* sim_v, const float* sim_n, int32_t n, float temperature,
                        int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                        float* work /* n*n + 6n floats */, void* stream);
/* Learnable temperature: the three heads above with the logit scale s = log(1 / tau) (CLIP's logit_scale) read from the DEVICE --
 * `logit_scale` points to one fp32, 1 / tau = expf(s) is formed by the kernels, nothing is read back -- in place of the by-value
 * `temperature` of model/loss.py:8-11,28-32 (`x / self.temperature`, :15-16,44-45).  Same kernels, same loss and embedding
 * gradients; next to them `d_logit_scale` (one fp32) receives
 *   dL/ds = sum_ij G_ij x_ij,      G = dL/dx (the matrix the gradient kernels already form), x = sim_matrix(text, video),
 * reduced without float atomics (per-row / per-workgroup partials, then one workgroup in double, fixed order): two calls give the
 * same bits.  d_logit_scale is written when gradients are (short head: d_text or d_video; long head: d_text, whose walk carries the
 * sum; from_sim: dx) and must be non-NULL then; with no gradient pointer the loss alone is computed.  The short head's workspace
 * is egv_egonce_work_floats as before; the long head's egv_egonce_long_work_floats (it includes the partials: linear in n). */
int egv_egonce_fwd_bwd_ls(const float* text, const float* video, const float* noun, const float* verb,
                          int32_t n, int32_t D, int32_t dn, int32_t dv, const float* logit_scale, float eps,
                          int32_t use_noun, int32_t use_verb,
                          float* loss, float* sim, float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream);
int egv_egonce_long_fwd_bwd_ls(const float* text, const float* video, const float* noun, const float* verb,
                               int32_t n, int32_t D, int32_t dn, int32_t dv, const float* logit_scale, float eps,
                               int32_t use_noun, int32_t use_verb,
                               float* loss, float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream);
int egv_egonce_from_sim_ls(const float* x, const float* sim_v, const float* sim_n, int32_t n, const float* logit_scale,
                           int32_t use_noun, int32_t use_verb, float* loss, float* dx, float* d_logit_scale,
                           float* work /* n*n + 7n floats */, void* stream);
/* EgoNCE / NormSoftmaxLoss with a QUEUE of past embeddings (csrc/egonce_long.hip: the long head's walk with queue tiles): the normalised rows of earlier steps are extra
 * constant columns of both softmaxes -- more negatives and, for EgoNCE, more positives (a queued clip that shares a noun and a verb
 * with an anchor) at no encoder cost.  With K = filled valid slots the head walks the rectangle of n batch rows against n + K columns
 * per direction, 2 n (n + K) pairs, and forms no queue x queue term; K = 0 is egv_egonce_long_fwd_bwd's loss.  Formulas: the top of
 * csrc/egonce_long.hip.  The queue lives in caller-owned DEVICE buffers in the kernels' own layout, which egv_egonce_queue_layout
 * returns (Dp floats per embedding row, W 32-bit words per noun / verb row; 1 on a bad D / dn / dv):
 *   q_text, q_video [Q, Dp] fp32;  q_words [Q, W] uint32 (may be NULL when W == 0: no noun / verb vectors);
 *   q_state int32 {head, filled}, both 0 for an empty queue.  Slots >= filled are never used, whatever they hold.
 * Limits: 1 <= n <= 65536, Q % 64 == 0, 64 <= Q <= 65536, n <= Q, D <= 256, D % 4 == 0; anything else returns 1 before any launch.
 * egv_egonce_queue_fwd_bwd reads the queue and `filled` on the device (no host read; the launch is sized by Q) and writes loss[1]
 * and, when given, d_text AND d_video [n, D] (both or neither; NULL: the loss alone).  The temperature is `temperature` by value, or,
 * with `logit_scale` non-NULL, 1 / tau = expf(*logit_scale) read on the device; then d_logit_scale[1] = dL/ds (the _ls convention,
 * queue columns included) is written with the gradients and must be non-NULL with them.  Queue rows get no gradient.  Data contract
 * of noun / verb as egv_egonce_long_fwd_bwd (a negative or NaN entry: NaN loss).  Deterministic: no float atomics.
 * egv_egonce_queue_push, after the head on the same stream and with the same n, D, dn, dv, `work` and `loss`: copies the n normalised
 * rows and packed words the head left in `work` into slots (head + i) mod Q, then head <- (head + n) mod Q and
 * filled <- min(Q, filled + n) in a launch of its own.  If *loss is not finite nothing is copied and the state stays as it is. */
int64_t egv_egonce_queue_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv, int32_t Q);
int egv_egonce_queue_layout(int32_t D, int32_t dn, int32_t dv, int32_t* Dp, int32_t* W);
int egv_egonce_queue_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb,
                             int32_t n, int32_t D, int32_t dn, int32_t dv,
                             const float* q_text, const float* q_video, const uint32_t* q_words, int32_t Q, const int32_t* q_state,
                             float temperature, const float* logit_scale, float eps, int32_t use_noun, int32_t use_verb,
                             float* loss, float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream);
int egv_egonce_queue_push(const float* work, const float* loss, int32_t n, int32_t D, int32_t dn, int32_t dv,
                          float* q_text, float* q_video, uint32_t* q_words, int32_t Q, int32_t* q_state, void* stream);
/* Pairwise sigmoid head (SigLIP) with EgoNCE's positives, for ANY n in [1, 65536] (D <= 256, D % 4 == 0; noun and verb both given or
 * both NULL: mask = I, plain SigLIP), csrc/sigmoid_head.hip.  With tn / vn the normalised rows (sim_matrix's rule, `eps`),
 *   x_ij = tn_i . vn_j,  u_ij = exp(s) x_ij + b,  z_ij = +1 where m_ij else -1,  loss = (1 / n) sum_ij softplus(-z_ij u_ij),
 * m the mask of egv_egonce_long_fwd_bwd (same data contract: only (entry > 0) of noun / verb is used; a negative or NaN entry makes the
 * loss NaN through a device-side flag).  `logit_scale` (s) and `logit_bias` (b) point to one fp32 each on the DEVICE and are never read
 * on the host.  No n x n buffer: the similarity tiles are formed on the fp32-input MFMA and streamed, loss and gradient in ONE walk per
 * direction; the workspace (egv_sigmoid_head_work_floats floats; 0 for bad sizes) is linear in n plus a bounded number of partial tiles.
 * Outputs: loss[1]; optionally d_text and d_video [n, D] (both or neither); optionally, with them, d_scale[1] = dL/ds = sum_ij G_ij x_ij
 * and d_bias[1] = dL/db (both or neither), G = dL/dx.  No gradient pointer: the loss alone (evaluation).  No float atomics: two calls
 * give the same bits.  Arguments are checked before any launch: a bad one returns 1 and launches nothing. */
int egv_sigmoid_head_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb,
                             int32_t n, int32_t D, int32_t dn, int32_t dv, const float* logit_scale, const float* logit_bias,
                             float eps, int32_t use_noun, int32_t use_verb,
                             float* loss, float* d_text, float* d_video, float* d_scale, float* d_bias, float* work, void* stream);
int64_t egv_sigmoid_head_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv);
/* The same loss on a given similarity matrix x [n, n] (n <= 4096, as egv_egonce_from_sim; sim_v / sim_n NULL => mask = I; otherwise
 * mask = sim_v * sim_n + I > 0, `use_noun` only: sim_n + I, else sim_v + I): loss[1], optionally dx [n, n], optionally with dx
 * d_scale[1] and d_bias[1] (both or neither).  One element-wise pass with block partials and a fixed-order final sum. */
int egv_sigmoid_from_sim(const float* x, const float* sim_v, const float* sim_n, int32_t n, const float* logit_scale,
                         const float* logit_bias, int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                         float* d_scale, float* d_bias, float* work /* 3072 floats */, void* stream);

/* Max-margin ranking losses of the fine-tuning heads (model/loss.py:55-133) on a square similarity matrix x [n, n]:
 *   loss = mean_{kept (i,j)} relu(w_i m - x_ii + x_ij) + relu(w_i m - x_ii + x_ji),   w = NULL: MaxMarginRankingLoss (w_i = 1),
 *   w = weight [n]: AdaptiveMaxMarginRankingLoss; fix_norm != 0 drops the diagonal pairs (mean over 2 n (n - 1) terms).
 * dx (optional) receives d loss / d x.  n <= 4096.                                                                       */
int egv_maxmargin_fwd_bwd(const float* x, const float* weight, int32_t n, float margin, int32_t fix_norm,
                          float* loss, float* dx, void* stream);

/* The ranking-loss head in one call: sim_matrix (model/model.py:189-197) + MaxMarginRankingLoss / AdaptiveMaxMarginRankingLoss
 * (model/loss.py:55-133) + the backward of both, for the all-gathered global batch text, video [n, D] fp32:
 *   x_ij = <t_i / max(|t_i|, eps), v_j / max(|v_j|, eps)>,  loss as egv_maxmargin_fwd_bwd on x (weight [n] or NULL, fix_norm),
 *   d_text, d_video [n, D] (optional) = d loss / d text, d video through the normalisation, eps clamp included;
 *   sim [n, n] (optional) receives x -- no n x n array is written otherwise.
 * Deterministic: no floating-point atomics, fixed summation orders; two calls on the same input give identical bits.
 * n <= 1024, D <= 256, D % 4 == 0 (and n >= 2 with fix_norm), else EGV_ERR_ARG before any launch.  work:
 * egv_maxmargin_head_work_floats(n, D) floats; work, d_text and d_video 16-byte aligned.                                  */
int egv_maxmargin_head_fwd_bwd(const float* text, const float* video, const float* weight /* [n] or NULL */,
                               int32_t n, int32_t D, float margin, int32_t fix_norm, float eps,
                               float* loss, float* sim /* optional [n,n] */, float* d_text, float* d_video /* optional */,
                               float* work, void* stream);
int64_t egv_maxmargin_head_work_floats(int32_t n, int32_t D);

/* Softmax cross-entropy of the classification fine-tunes (OSCC / PNR heads): model/loss.py:135-141 (nn.CrossEntropyLoss with its
 * defaults) on the [rows, cols] scores of FrozenInTime(video_only=True) (trainer/trainer_oscc.py:335-338).
 *   loss = mean over rows with target != ignore_index of (logsumexp(x_r) - x_r[target_r]);  NaN when no row is valid (as torch);
 *   dlogits (optional, [rows, ldd]) = (softmax(x_r) - onehot(target_r)) / #valid rows, 0 for ignored rows.
 *   A target outside [0, cols) that is not ignore_index is an error (torch: device assert): loss and dlogits come back NaN.
 * Deterministic (fixed summation order).  rows <= 2^20, cols <= 65536.                                                     */
int egv_cross_entropy_fwd_bwd(const float* logits, int64_t ld, const int64_t* target, int32_t rows, int32_t cols,
                              int64_t ignore_index, float* loss, float* dlogits, int64_t ldd, void* stream);

/* ---- classification head of the OSCC / PNR fine-tunes (csrc/cls_head.hip) -------------------------------------------------
 * The narrow Linear behind the video tower (model/model.py:76, projection_dim = 2 | 16 | 17), its loss and backward over the
 * all-gathered batch (trainer/trainer_oscc.py:335-338, trainer/trainer_pnr.py:341-350) and the validation scores
 * (model/metric.py:342-397).  fp32 in memory, sums carried in fp64; deterministic (no atomics, fixed summation orders: two calls
 * on the same input give identical bits).  Limits: C <= 64, K <= 1024 with K % 4 == 0, local rows B <= 256, gathered rows
 * n <= 4096; anything else is EGV_ERR_ARG before any launch.
 *
 * scores[r, c] = bias[c] + sum_k feats[r, k] W[c, k]  for feats [B, K] (leading dimension ldf, ldf % 4 == 0, 16-byte aligned),
 * W [C, K] (16-byte aligned), bias [C] or NULL; written to scores[r * ld + c], ld >= C: the first C columns of the row block
 * the collective sends.                                                                                                     */
int egv_cls_head_fwd(const float* feats, int64_t ldf, const float* W, const float* bias /* or NULL */, int32_t B, int32_t K,
                     int32_t C, float* scores, int64_t ld, void* stream);
/* Loss and backward on the gathered block packed [n, ld]: columns [0, C) the scores x, column col_target the class index t,
 * column col_state (or -1) the PNR state; both integer-valued floats.  With s = mean of the state column (1 when col_state < 0):
 *   loss = s (1/n) sum_r (logsumexp(x_r) - x_r[t_r])                     = CE (OSCC)  |  mean(state.T * CE) (PNR)
 *   g_r  = s (softmax(x_r) - onehot(t_r)) / n  for the LOCAL rows r in [row0, row0 + B)   (AllGather_multi.backward's slice)
 *   db [C] = sum_r g_r,  dW [C, K] = g^T feats,  dfeats [B, ldd] = g W        (each optional: NULL = skip; feats [B, ldf] local)
 *   pred [n] (optional) = argmax of every score row, lowest index on ties.
 * A target outside [0, C) makes the loss and every gradient NaN (as egv_cross_entropy_fwd_bwd).  work: n + 1 doubles.       */
int egv_cls_head_loss_bwd(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                          int32_t row0, int32_t B, const float* feats, int64_t ldf, const float* W, int32_t K,
                          float* loss, float* dW, float* db, float* dfeats, int64_t ldd, int32_t* pred, double* work,
                          void* stream);
/* egv_cls_head_loss_bwd on SOFT targets (extension: label smoothing and Mixup / CutMix; torch's label_smoothing rule, which is timm's
 * mixup_target).  Two more columns of the block -- col_target2 the partner's class t2 (-1: t2 = t), col_lam the mixing weight lam
 * (-1: lam = 1) -- and eps = label_smoothing in [0, 1] give the target distribution of row r
 *   q_r  = (1 - eps) (lam_r e(t_r) + (1 - lam_r) e(t2_r)) + eps / C
 *   loss = s (1/n) sum_r (logsumexp(x_r) - sum_c q_rc x_rc),   g_r = s (softmax(x_r) - q_r) / n.
 * dW, db, dfeats, pred (the argmax of the SCORES), s, the limits, the fp64 sums, the fixed summation order and the work buffer are
 * those of egv_cls_head_loss_bwd; a t OR t2 outside [0, C) makes the loss and every gradient NaN.  The columns are distinct. */
int egv_cls_head_loss_bwd_soft(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                               int32_t col_target2, int32_t col_lam, float label_smoothing, int32_t row0, int32_t B,
                               const float* feats, int64_t ldf, const float* W, int32_t K, float* loss, float* dW, float* db,
                               float* dfeats, int64_t ldd, int32_t* pred, double* work, void* stream);
/* egv_cross_entropy_fwd_bwd on the same soft targets, for given scores: target2 (int64 [rows]) and lam (fp32 [rows]) may each be NULL
 * (t2 = t, lam = 1).  Rows with target == ignore_index drop out of the numerator and of the count, as in torch; a valid row whose t
 * or t2 lies outside [0, cols) makes loss and dlogits NaN.  Sums over classes and rows in fp64, fixed order.                   */
int egv_cross_entropy_soft_fwd_bwd(const float* logits, int64_t ld, const int64_t* target, const int64_t* target2, const float* lam,
                                   float label_smoothing, int32_t rows, int32_t cols, int64_t ignore_index, float* loss,
                                   float* dlogits, int64_t ldd, void* stream);
/* Validation accumulator: accum = double[4] on the device {sum of hits, rows seen, sum of err_sec, positives seen}, updated in
 * place with the rows of a gathered block in ascending order.
 *   col_state < 0 (OSCC, model/metric.py:342-353): hit = argmax(x_r) == t_r; accum[0] += hits, accum[1] += n.
 *   col_state >= 0 (PNR, :355-397), rows with state 1 only: mapped = float32((end - start) / 16) * float32(argmax(x_r)) in fp32
 *   (the 16 is the reference's literal), err_sec = |mapped - (pnr - start)| / fps in fp64 with fps = (double)packed[r, col_fps] +
 *   (double)packed[r, col_fps + 1] (an fp64 frame rate such as 29.97 split in two floats); accum[2] += err_sec, accum[3] += 1,
 *   accum[1] += n.  col_target is not read for PNR.                                                                           */
int egv_cls_eval_update(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                        int32_t col_fps, int32_t col_start, int32_t col_end, int32_t col_pnr, double* accum, void* stream);

/* Dual-softmax re-scaling of a retrieval similarity matrix x [n texts, m videos] (run/test_epic.py:137-143, --dual_softmax):
 *   y = softmax(x / temp, dim 1) * x;  out = softmax(y, dim 0).  work: n*m floats.  temp = 500 in the reference.        */
int egv_dual_softmax(const float* x, int32_t n, int32_t m, float temp, float* work, float* out, void* stream);

/* ---- retrieval scoring (model/metric.py mir_metrics / map, utils/nDCG.py, utils/mAP.py) ---------------------
 * Per query row i of a similarity matrix S (fp32) and a relevancy matrix R, both stored [n1, n2] row-major with leading
 * dimensions lds / ldr (elements), the two scores of the row's ranking pi_i (S descending):
 *   DCG_i = sum_p R[i, pi_i(p)] * [p < K_i] / log2(p + 2),            K_i = #{j : R[i, j] > 0}          (calculate_DCG + calculate_k_counts)
 *   AP_i  = (1 / n_i) sum_{p : R[i, pi_i(p)] == 1} c_i(p) / (p + 1),   c_i(p) = sum_{q <= p} R[i, pi_i(q)], n_i = #{j : R[i, j] == 1}
 * c_i(p) is the running sum of the relevancies, as calculate_mAP's cumsum takes it: the number of positives up to p when R is
 * binary (model/metric.py map).  n_i == 0 gives NaN (0 / 0), as the reference.
 *   transposed == 0: the queries are the n1 rows; dcg_out / ap_out hold n1 doubles (either may be NULL, not both).
 *   transposed == 1: the queries are the n2 columns (S^T scored against R^T); the outputs hold n2 doubles, and `work`
 *     (egv_rank_scores_work_bytes(n1, n2) bytes, 8-byte aligned; unused and may be NULL otherwise) receives the transposed copies.
 *     Nothing goes to the host in either direction.
 *   S == NULL: the ideal ranking, S := R (calculate_IDCG) -- the row is ordered by its relevancies in R's own precision.
 *   affine_half != 0: the ranking is that of (s + 1) / 2 evaluated in fp32 (mir_metrics), ties it creates included.
 * TIE RULE: equal similarities (-0 == +0) are ranked by ascending column index (of the query's row, i.e. ascending row index of
 *   S when transposed).  NaN similarities are not supported.
 * LIMIT: the query row length (n2, or n1 when transposed) is at most EGV_RANK_MAX_ROW; the number of queries is unlimited.
 *   A longer row returns 1 and launches nothing, as every invalid argument does.
 * RELEVANCY PRECISION: r_is_f64 != 0: R is double, else float.  The tests `> 0` and `== 1` and the sums run on the value
 *   converted to double, so a caller that hands over fp32 must make sure that the conversion from its fp64 original was exact
 *   (0, 1, dyadic fractions) -- otherwise pass the fp64 matrix.
 * All sums, the discount and the divisions are fp64; fixed summation order, no atomics (bitwise reproducible).            */
#define EGV_RANK_MAX_ROW 16384
int egv_rank_scores(const float* S, int64_t lds, int32_t transposed, const void* R, int32_t r_is_f64, int64_t ldr,
                    int32_t n1, int32_t n2, int32_t affine_half, double* dcg_out, double* ap_out, void* work, void* stream);
int64_t egv_rank_scores_work_bytes(int32_t n1, int32_t n2);

/* ---- Recall@K: ground-truth ranks, top-k lists, row normalisation (csrc/recall.hip) -----------------------------------
 * Replaces the sort-and-subtract ranking of model/metric.py t2v_metrics (:20-124) and v2t_metrics (:127-216): the position
 * of the ground-truth distance in the sorted row is a count.  S is fp32 [n1, n2] row-major, leading dimension lds (elements).
 *   transposed == 0: the queries are the n1 rows, a row has n2 columns.
 *   transposed == 1: the queries are the n2 columns of S (v2t_metrics receives [texts, videos], :143); S is transposed on the
 *     device into `work` (egv_gt_ranks_work_bytes(n1, n2) bytes, 4-byte aligned; may be NULL otherwise) and a "row" below is a
 *     column of S with n1 entries.  n1 <= 65535 * 32 in this form.
 * Query r is row row0 + r of a larger problem (row0 >= 0: a chunk of rows can be ranked on its own).  Its ground truth is
 *   seg_wide == 0: the single column (row0 + r) / qpv                  (t2v: caption i belongs to video i / qpv, :39-43)
 *   seg_wide != 0: the qpv columns from (row0 + r) * qpv               (v2t: the captions of video i, :176)
 * col_valid (NULL = all valid): one uint8 per column of the row, nonzero = the column exists (query_masks, :167).
 *   g    = max of S over the valid columns of the segment                            (the closest ground-truth caption, :188-189)
 *   rank = #{valid j : s_j > g}                                   tie_avg == 0 ("optimistically", :66, :71-73)
 *   rank = #{valid j : s_j > g} + (#{valid j : s_j == g} - 1) / 2  tie_avg != 0 ("averaging", :157, :187)
 *   rank = +inf when the segment has no valid column (:175).
 * rank_out holds one double per query.  Comparisons are IEEE fp32 (-0 == +0); NaN is not supported.  A row may have up to
 * 2^31 - 1 columns; the counters are integers, so two calls give the same bits.  A segment that leaves the row returns 1 and
 * launches nothing, as every invalid argument does.                                                                          */
int egv_gt_ranks(const float* S, int64_t lds, int32_t transposed, int32_t n1, int32_t n2, int64_t row0, int32_t qpv,
                 int32_t seg_wide, const uint8_t* col_valid, int32_t tie_avg, double* rank_out, void* work, void* stream);
int64_t egv_gt_ranks_work_bytes(int32_t n1, int32_t n2);
/* Per row of S [rows, cols] the k <= EGV_TOPK_MAX largest (value, column) pairs among the valid columns, descending value, ties
 * by ascending column (-0 == +0; the TIE RULE of egv_rank_scores): vals fp32 [rows, k] (the entries themselves), idx int64
 * [rows, k].  With fewer than k valid columns the tail is -inf / -1.  Any row length up to 2^31 - 1.                          */
#define EGV_TOPK_MAX 64
int egv_topk_rows(const float* S, int64_t lds, int32_t rows, int32_t cols, const uint8_t* col_valid, int32_t k, float* vals,
                  int64_t* idx, void* stream);
/* out[r, :] = x[r, :] / max(|x[r, :]|_2, eps): the normalisation of sim_matrix (model/model.py:189-197) as an op of its own.
 * x [rows, D] with leading dimension ldx, out with ldo; out may be x.                                                         */
int egv_row_normalize(const float* x, int64_t ldx, int32_t rows, int32_t D, float eps, float* out, int64_t ldo, void* stream);

/* ---- gradient exchange (data parallel) ------------------------------------------------------------------
 * Replaces the fp32 bucket copies of DistributedDataParallel (base/base_trainer.py:258): `count` fp32 gradient tensors
 * (HOST arrays of device pointers / sizes) are scaled by `scale` (= 1 / world size), rounded to bf16 (RNE) and written to
 * flat[offsets[i] .. offsets[i] + numel[i]) -- the buffer RCCL all-reduces -- and read back into the fp32 tensors
 * afterwards.  offsets are in elements; multiples of 8 keep every access 16 bytes wide.  Tensors with numel <= 0 are
 * skipped.  Everything is validated before the first launch: a NULL pointer or a negative offset of a non-empty tensor
 * anywhere in the list enqueues nothing.                                                                              */
int egv_grad_pack_bf16(int32_t count, const float* const* grads, const int64_t* numel, egv_bf16* flat,
                       const int64_t* offsets, float scale, void* stream);
int egv_grad_unpack_bf16(int32_t count, float* const* grads, const int64_t* numel, const egv_bf16* flat,
                         const int64_t* offsets, void* stream);
/* The local reduction of the DIRECT gradient exchange (all-to-all of bucket slices over all xGMI links, then all-gather; SURVEY
 * 5 / 8(e): xGMI is point to point, a ring keeps 5 of the 7 links idle): recv holds `world` slices of slice_elems bf16 each (this
 * rank's slice of every peer's bucket); out[i] = bf16(sum_p float(recv[p][i])) -- fp32 accumulation, ONE rounding.
 * slice_elems % 8 == 0, 16-byte aligned pointers, world <= 64.                                                            */
int egv_slice_sum_bf16(const egv_bf16* recv, int32_t world, int64_t slice_elems, egv_bf16* out, void* stream);

/* ---- optimizer ----------------------------------------------------------------------------------------
 * transformers==4.2.1 AdamW (run/train_egoclip.py:73, configs/pt/egoclip.json:49-54) over a list of
 * tensors given as HOST arrays of device pointers (copied into kernel arguments in chunks), fused with
 * the refresh of the split-bf16 weight planes the GEMMs read (w_hi/w_lo may be NULL per tensor).
 * hyper_dev (optional, DEVICE, 4 floats {lr, step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t), grad_scale, skip}): when given,
 * the kernel takes the step-dependent scalars from there instead of lr / step / grad_scale, and does NOTHING when skip != 0 --
 * the block egv_loss_scale_update writes on the same stream (dynamic loss scale of the fp16 backward: whether the step is applied,
 * the 1 / S that un-scales the gradients and the bias correction at the number of APPLIED steps are decided on the device).
 * Tensors with numel <= 0 are skipped.  Everything is validated before the first launch: a NULL p / g / m / v of a non-empty
 * tensor anywhere in the list enqueues nothing.                                                                               */
int egv_adamw_multi(int32_t count, float* const* p, const float* const* g, float* const* m, float* const* v,
                    egv_bf16* const* w_hi, egv_bf16* const* w_lo, const int64_t* numel,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                    int32_t correct_bias, float grad_scale, const float* hyper_dev, void* stream);
/* Gradient accumulation of the embedding-cache step (egovlp_amd/trainer/cached_step.py; no counterpart in the reference, whose
 * trainer/trainer_egoclip.py:123-141 runs one backward per step): dst[i][j] += src[i][j] in fp32 for `count` tensors given as HOST
 * arrays of device pointers / sizes, as above.  One call for the whole model (the table is copied into kernel arguments 120 tensors at
 * a time); 16-byte accesses where both bases of a pair are 16-byte aligned, scalar otherwise and for the last numel % 4 elements;
 * every element has one writer, so the result does not depend on the grid.  count == 0 enqueues nothing; a negative size, a NULL
 * pointer of a non-empty tensor or a pair whose ranges overlap (dst == src included: harmless, but never meant) is an invalid
 * argument (nothing enqueued).  An inf / NaN in either
 * operand survives the sum, so egv_grad_nonfinite_multi on the accumulators sees the overflow of any chunk.                       */
int egv_grad_accumulate_multi(int32_t count, float* const* dst, const float* const* src, const int64_t* numel, void* stream);

/* ---- exponential moving average of the weights (no counterpart in the reference) ------------------------------------------
 * A shadow copy e of every parameter p follows e += w * (p - e), w = 1 - decay, after each optimizer step that was APPLIED; for
 * evaluation the two sets are exchanged in place.  Everything is decided on the device, nothing synchronises the host.
 *   state (8 x 32 bits, DEVICE): [0] int32 t, updates applied so far; [1] float w, the weight of this update (0: the pass below does
 *                                nothing); [2] int32 updates skipped so far; [3] float the decay in effect (logs); [4..7] zero, reserved.
 * egv_ema_decide (one thread): skip_flag (DEVICE, may be NULL; the [3] element of the hyper_dev block of the optimizer step) non-zero:
 * w = 0, state[2] += 1, t stays.  Otherwise, in double: d = warmup ? min(decay, (1 + t) / (10 + t)) : decay; w = (float)(1 - d);
 * state[3] = (float)d; t += 1.  0 <= decay < 1; anything else, or a NULL state, is an invalid argument (nothing enqueued).
 * egv_ema_update_multi: ema[i][j] = fmaf(w, p[i][j] - ema[i][j], ema[i][j]) with w = state[1] read on the device (w == 0: every block
 * returns at once), for `count` tensors given as HOST arrays of device pointers / sizes.  One call for the whole model (the table is
 * copied into kernel arguments 120 tensors at a time); 16-byte accesses where both bases of a pair are 16-byte aligned, scalar otherwise
 * and for the last numel % 4 elements; every element has one writer.  12 B of HBM traffic per element.
 * egv_swap_multi: a[i] <-> b[i], bit for bit (NaN payloads included), same list format; swapping twice is the identity.
 * Both validate as egv_grad_accumulate_multi: count == 0 enqueues nothing, a size of 0 is skipped; a negative count or size, a NULL
 * pointer of a non-empty tensor or a pair whose ranges overlap is an invalid argument, and then nothing is enqueued.               */
int egv_ema_decide(int32_t* state, const float* skip_flag, float decay, int32_t warmup, void* stream);
int egv_ema_update_multi(int32_t count, float* const* ema, const float* const* p, const int64_t* numel, const int32_t* state,
                         void* stream);
int egv_swap_multi(int32_t count, float* const* a, float* const* b, const int64_t* numel, void* stream);

/* ---- dynamic loss scale (the fp16 backward) ---------------------------------------------------------------
 * The reference back-propagates in fp32 (trainer/trainer_egoclip.py:139-141); here the backward GEMMs of the video blocks can run on
 * fp16 operands, whose range needs the gradients scaled: the loss is multiplied by S before backward() and AdamW divides by it.
 * S lives in DEVICE memory and follows torch.cuda.amp.GradScaler's rule without any host synchronisation:
 *   state (8 x 32 bits): [0] float S; [1] int32 good steps since S last changed; [2] int32 found_inf; [3] int32 steps skipped so far;
 *                        [4..7] float {lr, step_size, 1 / S, skip} -- the hyper_dev block of egv_adamw_multi.
 * egv_grad_nonfinite_multi: state[2] |= 1 if any of the `count` gradient tensors (HOST arrays of device pointers / sizes) holds an
 * inf or NaN (an overflowed fp16 plane poisons every gradient behind it: gradient planes are written un-clamped).
 * egv_loss_scale_update (one thread): advance != 0: found_inf ? (skip = 1, skipped += 1, S = max(S * backoff_factor, 1), good = 0)
 * : (skip = 0, good += 1; good == growth_interval ? S = min(S * growth_factor, max_scale), good = 0), found_inf = 0, 1 / S of the
 * scale the step RAN with -> state[6]; then {lr, step_size at t = step - skipped, state[6], state[7]} -> hyper_out (NULL: state + 4;
 * advance == 0 fills a further parameter group's block from the decision already taken).
 * egv_grad_nonfinite_multi skips tensors with numel <= 0; everything is validated before the first launch: a NULL pointer of a
 * non-empty tensor anywhere in the list enqueues nothing.                                                                         */
int egv_grad_nonfinite_multi(int32_t count, const float* const* grads, const int64_t* numel, int32_t* state, void* stream);
int egv_loss_scale_update(int32_t* state, float* hyper_out, float lr, float beta1, float beta2, int32_t step, int32_t correct_bias,
                          float growth_factor, float backoff_factor, int32_t growth_interval, float max_scale, int32_t advance,
                          void* stream);

/* ---- gradient clipping by global norm (no counterpart in the reference, which never clips) -------------------------------
 * torch.nn.utils.clip_grad_norm_ over all parameters, decided on the device and folded into the factor egv_adamw_multi already
 * multiplies every gradient by (hyper_dev[2]): no host synchronisation, no second read of the gradients.
 * egv_grad_sqnorm_parts: the number of partial sums (floats) egv_grad_sqnorm_multi writes for a list: one per block, a block
 * covers 65 536 elements of one tensor, empty tensors take none; -1 for a negative count / size or a list beyond 2^31 - 1 blocks.
 * egv_grad_sqnorm_multi: the scan of egv_grad_nonfinite_multi (state[2] |= 1 on an inf / NaN; `state` may be NULL: no scan) and
 * sum(g * g) in ONE read of the `count` fp32 gradient tensors (HOST arrays of device pointers / sizes; any 4-byte-aligned base,
 * 16-byte loads where the base allows them).  partials[0 .. parts) receive one fp32 sum per block, in list order; no
 * floating-point atomics: the same input gives the same bits, whatever the schedule; a partial is within 1.6e-5 relative of the
 * exact sum of its squares.  Everything is validated before the first launch: a negative count / size, a NULL pointer of a
 * non-empty tensor, or parts_capacity (floats behind `partials`) below the count above is an invalid argument and enqueues
 * nothing.
 * egv_grad_clip_update (one workgroup): norm^2 = the `parts` partials summed in a fixed order in double; norm = sqrt(norm^2) *
 * (state ? state[6], the 1 / S egv_loss_scale_update(advance) left for this step : grad_scale); coef = min(1, max_norm / (norm +
 * 1e-6)); a norm that is not finite (with `state`: also a step the scaler skips) makes the step NOT APPLIED: coef = 0, skip = 1.
 *   norm block (8 x 32 bits, DEVICE): [0] float norm (un-scaled, before clipping); [1] float coef; [2] int32 this step's norm was
 *                        not finite; [3] int32 steps clipped so far (coef < 1); [4] int32 steps not applied so far; [5..7] unused.
 * Then every one of the n_hyper (1..64) hyper blocks (`hyper`: HOST array of device pointers to 4 floats each, the hyper_dev of
 * the egv_adamw_multi calls that follow) gets [2] = (1 / S or grad_scale) * coef and [3] = skip.  With `state` the blocks must
 * already hold what egv_loss_scale_update wrote ([0], [1] stay; lr / step_size are ignored and may be NULL); without it [0] = lr[k],
 * [1] = step_size[k] (HOST arrays) are filled in as well.  max_norm > 0.                                                        */
int egv_grad_sqnorm_parts(int32_t count, const int64_t* numel);
int egv_grad_sqnorm_multi(int32_t count, const float* const* grads, const int64_t* numel, float* partials, int32_t parts_capacity,
                          int32_t* state, void* stream);
int egv_grad_clip_update(const float* partials, int32_t parts, const int32_t* state, float grad_scale, float max_norm,
                         int32_t n_hyper, float* const* hyper, const float* lr, const float* step_size, int32_t* norm_block,
                         void* stream);

/* ---- LAMB: layer-wise adaptive rates (You et al. 2020; no counterpart in the reference) ----------------------------------
 * Per tensor, with ge = g * grad_scale:  m = b1 m + (1 - b1) ge;  v = b2 v + (1 - b2) ge^2;  u = c * m / (sqrt(v) + eps) + wd * p;
 * r = ||p|| / ||u|| if (adapt and ||p|| > 0 and ||u|| > 0) else 1;  r = min(r, 1) if trust_clip;  p = p - lr * r * u.
 * c = sqrt(1 - b2^t) / (1 - b1^t) (1 when correct_bias == 0): eps stays OUTSIDE the correction, so u is, per unit lr, the direction
 * egv_adamw_multi applies -- timm's Lamb and apex's FusedLAMB correct m and v separately.  Three calls on one stream, all taking
 * `count` tensors as HOST arrays of device pointers / sizes (fp32, any 4-byte-aligned base; 16-byte accesses where every base of a
 * tensor is 16-byte aligned) and the SAME list in the SAME order:
 * egv_lamb_parts: the number of partial PAIRS stage 1 writes: one per 16 384-element piece of a tensor, empty tensors take none;
 * -1 for a negative count / size or a list beyond 2^31 - 1 pieces.
 * egv_lamb_stage1_multi: writes m and v, reduces p^2 and u^2 of every piece in a fixed order (no floating-point atomics) into
 * partials[2 * piece], partials[2 * piece + 1]; pieces are numbered through the list in order.  p and g are only read.
 * parts_capacity: pairs behind `partials`, at least egv_lamb_parts.
 * egv_lamb_ratio: one workgroup per tensor sums its run of pairs in double, in a fixed order, and stores r into ratios[i] (fp32,
 * `count` floats, i = the tensor's index in the list; an empty tensor gets 1 and shifts nothing).  parts must equal egv_lamb_parts.
 * egv_lamb_stage2_multi: recomputes u from p and the new m, v with stage 1's expression; p = fmaf(-(lr * ratios[i]), u, p).
 * lr == 0: p is not written (the moments of stage 1 advanced).
 * hyper_dev (DEVICE, may be NULL): {lr, step_size, grad_scale, skip} as for egv_adamw_multi; the kernels then take lr and grad_scale
 * from it and c = step_size / lr (the host's c when lr == 0), and with skip != 0 all three return before any store: parameters,
 * moments and ratios stay bit-identical.  Everything is validated before the first launch: a negative count / size, step < 1, a NULL
 * pointer of a non-empty tensor or too small a capacity is an invalid argument and enqueues nothing.
 * HBM traffic: 16 B + 8 B (stage 1) + 12 B + 4 B (stage 2) = 40 B per parameter; egv_adamw_multi moves 28 B.                     */
int egv_lamb_parts(int32_t count, const int64_t* numel);
int egv_lamb_stage1_multi(int32_t count, const float* const* p, const float* const* g, float* const* m, float* const* v,
                          const int64_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                          int32_t correct_bias, float grad_scale, const float* hyper_dev, float* partials, int32_t parts_capacity,
                          void* stream);
int egv_lamb_ratio(int32_t count, const int64_t* numel, const float* partials, int32_t parts, int32_t adapt, int32_t trust_clip,
                   const float* hyper_dev, float* ratios, void* stream);
int egv_lamb_stage2_multi(int32_t count, float* const* p, const float* const* m, const float* const* v, const int64_t* numel,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, int32_t correct_bias,
                          const float* hyper_dev, const float* ratios, void* stream);

/* ---- misc -----------------------------------------------------------------------------------------------
 * gather rows: out[r,:] = x[idx_stride * r * ld ...] helper for CLS-row extraction is done with strides in
 * egv_layernorm_fwd (ldx = S*D, rows = B).  relu on fp32 -> split planes: */
int egv_relu_split(const float* x, int64_t ldx, int32_t rows, int32_t cols, egv_bf16* hi, egv_bf16* lo,
                   int64_t ldo, void* stream);
/* scatter rows of a small matrix into a zeroed big one: dst[r * ld_dst + c] = src[r, c] (CLS-row grads). */
int egv_version(void);
/* 0 = the caller's header agrees with the library: abi_version == EGV_ABI_VERSION and the four struct sizes (sizeof egv_gemm_desc,
 * egv_block_geom, egv_block_params, egv_block_bwd_io) match; 1 otherwise.                                                          */
int egv_abi_check(int32_t abi_version, int64_t sizeof_gemm_desc, int64_t sizeof_block_geom, int64_t sizeof_block_params,
                  int64_t sizeof_block_bwd_io);
/* diagnostics, not on the product path: `iters` rounds of 40 independent MFMA 16x16x32 bf16 per wave, `waves` (1..8) waves
 * per workgroup, one workgroup per CU, no memory traffic -- the chip's sustained MFMA rate (tools/mfma_peak.py). */
int egv_diag_mfma_peak(int32_t iters, int32_t waves, float* out, void* stream);
/* diagnostics, not on the product path: a copy of `bytes` (multiple of 1024) from src to dst on the GEMM's own memory paths,
 * to calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters on a known byte count (tools/traffic_calib.py).
 * mode bits: 1 = loads by LDS-DMA (global_load_lds dwordx4, the operand path of the big GEMM; else plain 16-byte loads),
 * 2 = non-temporal stores (else write-back), 4 = read only, 8 = write only.  Valid: 0, 1, 2, 3, 4, 5, 8, 10. */
int egv_diag_traffic_calib(int32_t mode, const void* src, void* dst, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
