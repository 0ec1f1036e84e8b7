// Which GEMM kernel runs, on what grid: the argument rules of egv_gemm_nt and the choice of kernel family, instance, grid, block and
// LDS for the launch it makes and for the split-K reduce behind it.  Each rule is stated here once; the entry point calls the check,
// then the pick, and only then enqueues (gemm_nt.hip), and gemm_big.hip maps a pick to one of its instances.
// Everything above the __HIPCC__ part is plain C++ (tests/test_gemm_dispatch_cpu.py compiles it on its own).
#pragma once
#include <stdint.h>

#include "egovlp_hip.h"

#ifndef EGV_OK
#define EGV_OK 0
#define EGV_ERR_ARG 1
#endif

constexpr int64_t GEMM_MAX_GRID = 0x7fffffff;     // blocks in x -- and work ids, which the kernels count in an int
constexpr int64_t GEMM_MAX_GRID_Y = 65535;        // the k-slices of the small kernel are its grid.y
constexpr int GEMM_BIG_WGS = 256;                 // the big kernel is persistent: one workgroup per CU unless grid_cap says fewer
constexpr int GEMM_BIG_MIN_TILES = 128;           // fewer 256x256 work items than this leave the chip to the 128x128 kernel

// GEMM_SMALL  gemm_nt.hip: 128x128 tile, 32-deep k-steps; NT only, passes 1 / 3 (small M, or K not a multiple of 64)
// GEMM_BIG    gemm_big.hip: (256 | 320) x 256 tile, persistent workgroups; every TN problem, every fp16 product
enum GemmFamily { GEMM_SMALL, GEMM_BIG };

// epilogue flavours of the big kernel (template parameter: each instance carries only its own epilogue code)
enum { EPI_RAW = 0,      // store the accumulators (split-K partial slab, or plain fp32 output)
       EPI_LINEAR = 1,   // + bias, + residual -> fp32 and/or planes
       EPI_GELU = 2,     // + bias, pre-activation -> aux_out, gelu -> fp32 and/or planes
       EPI_GELU_BWD = 3, // * gelu'(aux_in) -> fp32 and/or planes
       EPI_GENERIC = 4,  // everything at run time (alpha, ReLU', ...)
       EPI_GELU_X2 = 5 };// EPI_GELU with the activation written as fp16 operand planes -- EGV_OUT_F16X2: the f16x2 format (csrc/f16x2.h,
                         // first-operand role, two planes); EGV_OUT_F16: ONE plane of plain fp16 (the consumer runs a single fp16 product)
                         // -- [+ bf16 plane for the backward], the saved gelu' as bf16: fc1 forward of the f16x2 mode

// What follows a split-K launch.  GEMM_RED_NONE      un-split
//                                 GEMM_RED_EPILOGUE  small kernel: sum the slabs and apply the full fused epilogue
//                                 GEMM_RED_SLAB      big kernel: sum the slabs into out_f32 (+ the column-sum slab behind them)
//                                 GEMM_RED_CALLER    accumulate == 2: the slabs stay for egv_splitk_reduce_multi
enum GemmReduce { GEMM_RED_NONE, GEMM_RED_EPILOGUE, GEMM_RED_SLAB, GEMM_RED_CALLER };

// Which gemm_big_kernel<MF, TN, EPI, PROD, MIXED> exist: gemm_big.hip instantiates exactly these and the pick names no other.
// PROD: 0 = one bf16 product per k-tile (passes 3: three k-segments), 1 = the same loop on the fp16 opcode, 2 = fused f16x2,
// 3 = fused bf16x3.  TN: the weight gradient, single products, slabs or plain fp32.  MIXED: 320- and 256-row bands in one launch.
constexpr bool gemm_big_instance(int mf, bool tn, int epi, int prod, bool mixed) {
  if ((mf != 4 && mf != 5) || prod < 0 || prod > 3 || epi < EPI_RAW || epi > EPI_GELU_X2) return false;
  if (tn) return mf == 4 && epi == EPI_RAW && prod <= 1 && !mixed;
  if (mixed) return mf == 5 && prod >= 2 && (epi == EPI_LINEAR || epi == EPI_GELU || (epi == EPI_GELU_X2 && prod == 2));
  if (prod == 1) return epi == EPI_RAW || epi == EPI_LINEAR || epi == EPI_GELU_X2 || epi == EPI_GELU_BWD;
  if (prod == 2) return epi == EPI_RAW || epi == EPI_LINEAR || epi == EPI_GELU || epi == EPI_GELU_X2;
  return epi != EPI_GELU_X2;
}
constexpr int GEMM_BIG_IDS = 2 * 2 * 6 * 4 * 2;
constexpr int gemm_big_id(int mf, int tn, int epi, int prod, int mixed) { return ((((mf - 4) * 2 + tn) * 6 + epi) * 4 + prod) * 2 + mixed; }

// ------------------------------------------------------------------------------------------------ shared by the check and the pick
inline int64_t gemm_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t gemm_ksplit(const egv_gemm_desc& p) { return p.ksplit > 1 ? p.ksplit : 1; }
inline bool gemm_fp16(const egv_gemm_desc& p) { return p.passes == 2 || p.passes == 4; }      // f16x2 / one plain fp16 plane
inline int64_t gemm_tiles(const egv_gemm_desc& p, int bm, int bn) { return gemm_ceil_div(p.M, bm) * gemm_ceil_div(p.N, bn); }

// big tiles for the token-major GEMMs, every TN (wgrad) problem and every fp16 product -- it is the only kernel that multiplies
// those; the 128x128 kernel where M is too small to fill big tiles (DistilBERT's M = 1024 GEMMs make 12, projections) or K is
// not a multiple of 64.  -> GEMM_BIG, GEMM_SMALL, or -1: no kernel runs this.
// The big kernel shifts its last tile row / column inwards, so it needs one whole tile; TN writes plain fp32 and nothing else.
inline int gemm_family(const egv_gemm_desc& p) {
  const bool big_ok = p.M >= 256 && p.N >= 256 &&
                      (p.trans ? p.M % 8 == 0 && p.N % 8 == 0 && p.out_f32 && p.act == EGV_ACT_NONE && !p.bias && !p.residual && !p.out_hi
                               : p.K % 64 == 0);
  if (p.trans || gemm_fp16(p)) return big_ok ? GEMM_BIG : -1;
  const int64_t tiles = gemm_tiles(p, 256, 256);              // (the product with ksplit is formed below 128 tiles only: no overflow)
  return big_ok && (tiles >= GEMM_BIG_MIN_TILES || tiles * gemm_ksplit(p) >= GEMM_BIG_MIN_TILES) ? GEMM_BIG : GEMM_SMALL;
}

// PROD of a big launch.  f16x2 (passes 2) runs the fused two-product loop or -- x2_seg bit 1: always, bit 0: K, N <= 768 -- two
// k-segments of the plain fp16 loop, which wins for short contractions (profiles/r06g_x2seg_bench.txt); bf16x3 runs the fused
// three-product loop unless a diagnostics build turns f3 off; TN is a single-product loop.
inline int gemm_prod(const egv_gemm_desc& p, int x2_seg, int f3) {
  if (p.passes == 4) return 1;
  if (p.passes == 2) return ((x2_seg & 2) || ((x2_seg & 1) && p.K <= 768 && p.N <= 768)) ? 1 : 2;
  return (p.passes == 3 && f3 && !p.trans) ? 3 : 0;
}

// 4-element pieces, 256 per block: the M x N product slab, then (TN with colsum) the M column sums behind it
inline int64_t gemm_reduce_blocks1(const egv_gemm_desc& p) { return gemm_ceil_div((int64_t)p.M * p.N / 4, 256); }
inline int64_t gemm_reduce_blocks2(const egv_gemm_desc& p) { return p.colsum ? gemm_ceil_div(p.M / 4, 256) : 0; }

// -------------------------------------------------------------------------------------------------------------------------- check
// EGV_OK or EGV_ERR_ARG.  Nothing behind an EGV_OK refuses for an argument reason; nothing is enqueued before it.
inline int gemm_check(const egv_gemm_desc& p, int x2_seg) {
  const bool fp16 = gemm_fp16(p);
  const int64_t ks = gemm_ksplit(p);
  // operands, sizes, ranges
  if (!p.a_hi || !p.b_hi || p.passes < 1 || p.passes > 4) return EGV_ERR_ARG;
  if ((p.passes == 2 || p.passes == 3) && (!p.a_lo || !p.b_lo)) return EGV_ERR_ARG;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.N % 4 != 0 || p.lda % 8 != 0 || p.ldb % 8 != 0 || (!p.trans && p.K % 32 != 0))
    return EGV_ERR_ARG;                                                    // (TN: any K, rows past it come from a zero page)
  if (p.out_fmt < EGV_OUT_BF16_SPLIT || p.out_fmt > EGV_OUT_F16_GRAD || p.aux_bf16 < EGV_AUX_F32 || p.aux_bf16 > EGV_AUX_DGELU_F16) return EGV_ERR_ARG;
  if (p.grid_cap != 0 && (p.grid_cap < 8 || p.grid_cap > GEMM_BIG_WGS || p.grid_cap % 8 != 0)) return EGV_ERR_ARG;
  if ((ks > 1 && !p.partial) || (p.colsum && !p.trans)) return EGV_ERR_ARG;
  if ((p.act == EGV_ACT_GELU_BWD || p.act == EGV_ACT_RELU_BWD) && !p.aux_in) return EGV_ERR_ARG;        // (the epilogues read it unasked)
  const int family = gemm_family(p);
  if (family < 0) return EGV_ERR_ARG;
  // what only the big kernel, and only its fp16 products, can do
  if (p.aux_bf16 != EGV_AUX_F32 && (family != GEMM_BIG || p.act == EGV_ACT_RELU_BWD)) return EGV_ERR_ARG;   // 16-bit aux: the GELU epilogues
  if ((p.aux_bf16 == EGV_AUX_DGELU_F16 || p.out_fmt != EGV_OUT_BF16_SPLIT) && !fp16) return EGV_ERR_ARG;                        // fp16 gelu', fp16 plane outputs
  // ... and fp16 gelu' is known to the plane epilogue alone (planes and nothing else): the rolled one takes every 16-bit aux for bf16
  if (p.aux_bf16 == EGV_AUX_DGELU_F16 && (p.act == EGV_ACT_GELU || p.act == EGV_ACT_GELU_BWD) && (!p.out_hi || p.residual || p.out_f32)) return EGV_ERR_ARG;
  // The big kernel computes the columns its shifted last tile shares with the tile before it twice and stores both results.  Its plane
  // epilogue gives a lane 8 consecutive columns, so with N % 8 != 0 an element sits in the other half of a lane's piece the second time.
  // The linear epilogues are the same fp32 additions there; the erf ones are not bit for bit (read from the ISA of
  // gemm_big_kernel<5, false, EPI_GELU_BWD, 3>: hipcc contracts `1 - half` of gelu_parts to an fma in the second half of the piece and
  // leaves a multiply and a subtract in the first), and two planes stored by two workgroups can then pair the hi of one result
  // with the lo of the other: one bf16 ulp of the value (tests/test_gpu_gemm_elements.py, refused-gelu-planes-N260).  A single
  // plane cannot pair, but which of two results it holds would still depend on the order of two workgroups: refused alike.
  if (family == GEMM_BIG && p.out_hi && p.N % 8 != 0 && (p.act == EGV_ACT_GELU || p.act == EGV_ACT_GELU_BWD)) return EGV_ERR_ARG;
  // fp16 operands / outputs (csrc/f16x2.h): NT un-split, or (passes 4) the TN weight gradient of the fp16 backward with its k-slices
  if (fp16 && (p.trans ? p.passes == 2 || p.out_fmt != EGV_OUT_BF16_SPLIT : ks > 1)) return EGV_ERR_ARG;
  if (p.trans && p.alpha != 1.0f && !(p.alpha > 0.f)) return EGV_ERR_ARG;                      // (a NaN is refused)
  if (fp16 && !p.trans) {
    // the epilogues the fp16 instances have.  One product (also the two k-segments of f16x2) -- forward: fc2 / proj (bias + residual
    // -> fp32), qkv (bias -> planes), fc1 (GELU -> fp16 operand planes); fp16 backward: every dgrad (-> fp32 / planes; fc2's with the
    // GELU' epilogue).  Fused f16x2: forward products only.
    const int prod = gemm_prod(p, x2_seg, 1);
    if (p.alpha != 1.0f) return EGV_ERR_ARG;
    if (prod == 1 ? !(p.act == EGV_ACT_NONE || (p.act == EGV_ACT_GELU && p.out_fmt != EGV_OUT_BF16_SPLIT) || (p.act == EGV_ACT_GELU_BWD && !p.bias))
                  : !(p.act == EGV_ACT_NONE || p.act == EGV_ACT_GELU))
      return EGV_ERR_ARG;
    if (p.out_fmt != EGV_OUT_BF16_SPLIT) {
      // fp16 plane outputs, planes only: the GELU epilogue (h for fc2: the f16x2 format, two planes, or one plain plane); the plain
      // epilogue as an fp16 split (the qkv planes of the fp16 attention); and -- one fp16 product only -- un-clamped gradient
      // planes: dZ from the GELU' epilogue on a saved derivative, dO from a plain dgrad
      const bool gelu_fwd = p.act == EGV_ACT_GELU && (p.out_fmt == EGV_OUT_F16X2 || p.out_fmt == EGV_OUT_F16);
      const bool gelu_bwd16 = prod == 1 && p.act == EGV_ACT_GELU_BWD && p.out_fmt == EGV_OUT_F16_GRAD && p.aux_in && p.aux_bf16 >= EGV_AUX_DGELU_BF16;
      const bool lin_split = p.act == EGV_ACT_NONE && p.out_fmt == EGV_OUT_F16_SPLIT && p.out_lo;
      const bool lin_grad = prod == 1 && p.act == EGV_ACT_NONE && p.out_fmt == EGV_OUT_F16_GRAD && !p.bias;
      if (!(gelu_fwd || gelu_bwd16 || lin_split || lin_grad) || !p.out_hi || (p.out_fmt == EGV_OUT_F16X2 && !p.out_lo) || p.residual ||
          p.out_f32 || (p.aux_out && p.aux_bf16 == EGV_AUX_F32) || p.ldoh % 8 != 0)
        return EGV_ERR_ARG;
    }
  }
  // split-K: the small kernel's reduce applies the epilogue and does not accumulate; the big kernel's slabs are summed into a dense
  // out_f32 (accumulate 1: added to it), or (accumulate 2, TN only) left to the caller.  (colsum: M % 4 == 0 follows from TN's M % 8.)
  if (ks > 1 && (family == GEMM_SMALL ? p.accumulate != 0 : !p.out_f32 || p.ldo != p.N || (p.accumulate == 2 && !p.trans)))
    return EGV_ERR_ARG;
  // grids, exactly: blocks in x and work ids (the big kernel: at most as many as 256-row tiles make) within an int, k-slices in y
  if (family == GEMM_SMALL ? gemm_tiles(p, 128, 128) > GEMM_MAX_GRID || ks > GEMM_MAX_GRID_Y
                           : gemm_tiles(p, 256, 256) > GEMM_MAX_GRID / ks)
    return EGV_ERR_ARG;
  if (ks > 1 && gemm_reduce_blocks1(p) + gemm_reduce_blocks2(p) > GEMM_MAX_GRID) return EGV_ERR_ARG;
  return EGV_OK;
}

// --------------------------------------------------------------------------------------------------------------------------- pick
struct GemmPick {
  int family, passes;                              // passes: the small kernel's instance, 1 or 3
  int mf, tn, epi, prod, mixed, nb5;               // the big kernel's instance (gemm_big_instance); mixed: its 320-row bands, a kernel argument
  int block, lds;                                  // threads, dynamic LDS bytes
  int64_t grid_x, grid_y;
  int reduce;                                      // GemmReduce, and its blocks (of 256 threads): those past reduce_blocks1 sum the column sums
  int64_t reduce_grid, reduce_blocks1;
};

// rows per block tile as MF = 4 (256) or 5 (320): whichever minimises (rounds on 256 CUs) x (tile cost); ties go to 320.  M = 25 120
// tokens (B = 32, T = 4) gives 79 x 3 = 237 tiles of 320x256 for the N = 768 GEMMs, one round, where 256x256 needs 297 = two.
inline int gemm_pick_mf(const egv_gemm_desc& p) {
  if (p.trans || p.M < 320) return 4;
  const int64_t cost4 = gemm_ceil_div(gemm_tiles(p, 256, 256) * gemm_ksplit(p), 256) * 4;
  const int64_t cost5 = gemm_ceil_div(gemm_tiles(p, 320, 256) * gemm_ksplit(p), 256) * 5;
  return cost5 <= cost4 ? 5 : 4;
}

// Mixed row bands (see gemm_big_kernel): -> nb5 (number of 320-row bands, the rest are 256 rows), or -1 when the uniform 320-row
// tiling is at least as good.  Same number of rounds R as the uniform tiling; as many bands as R rounds of `grid` workgroups can
// take; cost = 5 per round that still contains a 320-row tile + 4 per round of 256-row tiles only.
inline int64_t gemm_pick_mixed_bands(const egv_gemm_desc& p, int64_t grid) {
  if (p.M < 640 || grid < 8) return -1;
  const int64_t tn = gemm_ceil_div(p.N, 256);
  const int64_t R = gemm_ceil_div(gemm_tiles(p, 320, 256), grid);
  if (R < 2) return -1;
  const int64_t NB = (R * grid) / tn;                             // bands R rounds can hold
  int64_t nb5 = (p.M - 256 * NB + 63) / 64;                       // 320 nb5 + 256 (NB - nb5) >= M
  if (nb5 < 0) nb5 = 0;
  if (nb5 > NB) return -1;
  const int64_t r5 = gemm_ceil_div(nb5 * tn, grid);               // rounds that contain a 320-row tile
  return 5 * r5 + 4 * (R - r5) < 5 * R ? nb5 : -1;
}

// The launch of a CHECKED descriptor.  x2_seg, f3: the EGV_X2_SEG / EGV_GEMM_F3 knobs (defaults 2, 1).
inline GemmPick gemm_pick(const egv_gemm_desc& p, int x2_seg, int f3) {
  GemmPick g = {};
  const int64_t ks = gemm_ksplit(p);
  g.family = gemm_family(p);
  if (g.family == GEMM_SMALL) {
    g.passes = p.passes == 3 ? 3 : 1;
    g.grid_x = gemm_tiles(p, 128, 128); g.grid_y = ks;
    g.block = 256; g.lds = 2 * (g.passes == 3 ? 4 : 2) * 128 * 32 * 2;      // two stages of 2 or 4 [128][32] bf16 planes
  } else {
    // persistent workgroups: one per CU (144 KiB of LDS each); a grid that is a multiple of 8 keeps v % 8 == blockIdx % 8
    // (XCD affinity).  p.grid_cap < 256 leaves CUs to the RCCL kernels of an overlapped collective (per launch: no process state).
    const int64_t cap = p.grid_cap > 0 ? p.grid_cap : GEMM_BIG_WGS;
    const bool nothing_fused = !p.bias && !p.residual && !p.out_hi;
    g.mf = gemm_pick_mf(p); g.tn = p.trans != 0; g.prod = gemm_prod(p, x2_seg, f3);
    if (p.trans || ks > 1) g.epi = EPI_RAW;                        // wgrad / split-K slab: plain fp32, no epilogue
    else if (p.alpha == 1.0f && p.act == EGV_ACT_NONE) g.epi = nothing_fused && p.out_f32 ? EPI_RAW : EPI_LINEAR;
    else if (p.alpha == 1.0f && p.act == EGV_ACT_GELU) g.epi = p.out_fmt != EGV_OUT_BF16_SPLIT ? EPI_GELU_X2 : EPI_GELU;
    else if (p.alpha == 1.0f && p.act == EGV_ACT_GELU_BWD && !p.bias) g.epi = EPI_GELU_BWD;
    else g.epi = EPI_GENERIC;
    // the two multi-round forward shapes of the step (qkv: plane outputs; fc1: GELU + planes + saved gelu') with mixed row bands
    const bool may_mix = g.prod >= 2 && g.mf == 5 && (g.epi == EPI_GELU || g.epi == EPI_GELU_X2 || (g.epi == EPI_LINEAR && !nothing_fused));
    const int64_t nb5 = may_mix ? gemm_pick_mixed_bands(p, cap) : -1;
    g.mixed = nb5 >= 0; g.nb5 = g.mixed ? (int)nb5 : 0;
    const int64_t bands = g.mixed ? nb5 + gemm_ceil_div(p.M - nb5 * 320, 256) : gemm_ceil_div(p.M, g.mf * 64);
    const int64_t work = bands * gemm_ceil_div(p.N, 256) * ks;
    g.grid_x = work < cap ? work : cap; g.grid_y = 1;
    g.block = 512; g.lds = 2 * (g.mf * 64 + 256) * 128;            // two stages of (rows + 256 columns) x 128 B
  }
  g.reduce = ks == 1 ? GEMM_RED_NONE : g.family == GEMM_SMALL ? GEMM_RED_EPILOGUE : p.accumulate == 2 ? GEMM_RED_CALLER : GEMM_RED_SLAB;
  if (g.reduce == GEMM_RED_EPILOGUE || g.reduce == GEMM_RED_SLAB)
    g.reduce_blocks1 = gemm_reduce_blocks1(p), g.reduce_grid = g.reduce_blocks1 + gemm_reduce_blocks2(p);
  return g;
}

// ------------------------------------------------------------------------------------------------------- across the two GEMM files
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// gemm_big.hip: the process's EGV_X2_SEG (and, diagnostics build, EGV_GEMM_F3) knobs, read once; one launch of a GEMM_BIG pick
void egv_gemm_env(int* x2_seg, int* f3);
int egv_gemm_big_launch(const GemmPick& g, const egv_gemm_desc& p, hipStream_t s);
#endif
