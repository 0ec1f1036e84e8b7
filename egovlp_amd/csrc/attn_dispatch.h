// Which attention kernel runs, on what grid: the argument rules of the four attention entry points (egv_divided_attn_fwd / _bwd,
// egv_text_attn_fwd / _bwd) and the choice of kernel family, fragment count, block, LDS and grid for every launch they make.
// Each rule is stated here once; the entry points call a check, then a pick per kernel, and only then enqueue, and the kernel
// files map a pick to one of their instances (att_launch, attn_common.h).
// Everything above the __HIPCC__ part is plain C++ (tests/test_attn_dispatch_cpu.py compiles it on its own).
#pragma once
#include <stdint.h>

#include "../../include/egovlp_hip.h"      // by its place in the tree: the CPU tests compile this file with csrc alone on the include path

#ifndef EGV_OK
#define EGV_OK 0
#define EGV_ERR_ARG 1
#endif

constexpr int64_t ATT_MAX_GRID = 0x7fffffff;      // blocks of a one-dimensional grid
constexpr int ATT_MAX_FRAMES = 64;                // frames of a time-attention group
constexpr int ATT_PERSIST_WGS = 256;              // the streaming forward is persistent: one 16-wave workgroup per CU walks the groups
constexpr int ATT_TILE_ROWS = 64;                 // key-tiled kernels: rows per LDS tile, two tiles in the ring
constexpr int ATT_TILE_WAVES = 8;                 //   and 16 rows per wave: blocks of 128 queries (dK / dV: keys)

// ------------------------------------------------------------------------------------------------------------------- checks
// Arguments as plain values: sizes, the mode word, passes, and which pointers are there (`required`: all that must be).  EGV_OK or
// EGV_ERR_ARG; on EGV_OK *d holds the decoded mode and which optional planes the kernels are given (the others are passed as null).

// egv_divided_attn_*: B clips, T frames, n locations, H heads; S = 1 + T n tokens per clip
inline int att_check_divided_sizes(int B, int T, int n, int H, int time, int passes) {
  if (B <= 0 || T <= 0 || n <= 0 || H <= 0 || (passes != 1 && passes != 3)) return EGV_ERR_ARG;
  if ((int64_t)T * n >= 0x7fffffff || (int64_t)B * H > ATT_MAX_GRID) return EGV_ERR_ARG;      // S is an int; the CLS helpers run B H blocks
  if (time && T > ATT_MAX_FRAMES) return EGV_ERR_ARG;
  return EGV_OK;
}

struct AttDividedFwd {
  int time;               // EGV_ATTN_TIME: time attention, else space
  int out_fmt;            // EGV_ATTN_OUT_*: format of the output planes, three-product forward only
  int f16;                // EGV_ATTN_FWD_QKV_F16: the qkv planes are an fp16 split: fp16 MFMA products, three-product forward only
  bool qkv_lo, out_lo;
};
inline int att_check_divided_fwd(int B, int T, int n, int H, int mode, int passes, bool required, bool qkv_lo, bool out_lo,
                                 AttDividedFwd* d) {
  if (!required || mode < 0 || mode > (EGV_ATTN_TIME | EGV_ATTN_OUT_MASK << EGV_ATTN_OUT_SHIFT | EGV_ATTN_FWD_QKV_F16)) return EGV_ERR_ARG;
  *d = {mode & EGV_ATTN_TIME, (mode >> EGV_ATTN_OUT_SHIFT) & EGV_ATTN_OUT_MASK, (mode & EGV_ATTN_FWD_QKV_F16) != 0, qkv_lo, out_lo};
  if (att_check_divided_sizes(B, T, n, H, d->time, passes)) return EGV_ERR_ARG;
  if ((d->f16 || d->out_fmt != EGV_ATTN_OUT_BF16_SPLIT) && passes != 3) return EGV_ERR_ARG;
  if (d->out_fmt == EGV_ATTN_OUT_F16) d->out_lo = false;                     // ONE plane of fp16(value)
  if (passes == 3 && (!qkv_lo || (!d->out_lo && d->out_fmt != EGV_ATTN_OUT_F16))) return EGV_ERR_ARG;
  if (passes == 1) d->qkv_lo = d->out_lo = false;
  return EGV_OK;
}

struct AttDividedBwd {
  int time;               // EGV_ATTN_TIME
  int o_fmt;              // EGV_ATTN_OUT_*: the format the forward wrote its output planes in
  int g_fmt;              // EGV_ATTN_BWD_GRAD_F16: dqkv in the format the GEMMs that read it call EGV_OUT_F16_GRAD (ONE plane of un-clamped
                          // fp16) instead of EGV_OUT_BF16_SPLIT; passes == 1 only
  int f16;                // EGV_ATTN_BWD_QKV_F16: q / k / v / dO are fp16 planes; with EGV_ATTN_BWD_GRAD_F16 and passes == 1 only
  bool qkv_lo, out_lo, dout_lo, dqkv_lo;
};
inline int att_check_divided_bwd(int B, int T, int n, int H, int mode, int passes, bool required, bool qkv_lo, bool out_lo,
                                 bool dout_lo, bool dqkv_lo, AttDividedBwd* d) {
  if (!required || mode < 0 || mode > (EGV_ATTN_TIME | EGV_ATTN_OUT_MASK << EGV_ATTN_OUT_SHIFT | EGV_ATTN_BWD_GRAD_F16 | EGV_ATTN_BWD_QKV_F16)) return EGV_ERR_ARG;
  *d = {mode & EGV_ATTN_TIME, (mode >> EGV_ATTN_OUT_SHIFT) & EGV_ATTN_OUT_MASK, (mode & EGV_ATTN_BWD_GRAD_F16) ? EGV_OUT_F16_GRAD : EGV_OUT_BF16_SPLIT,
        (mode & EGV_ATTN_BWD_QKV_F16) != 0, qkv_lo, out_lo, dout_lo, dqkv_lo};
  if (att_check_divided_sizes(B, T, n, H, d->time, passes)) return EGV_ERR_ARG;
  if (d->f16 && !d->g_fmt) return EGV_ERR_ARG;
  if ((d->o_fmt >= EGV_ATTN_OUT_F16X2 || d->g_fmt) && passes != 1) return EGV_ERR_ARG;      // fp16 outputs: an fp16 backward
  if (d->o_fmt != EGV_ATTN_OUT_BF16_SPLIT) d->out_lo = false;                            // only the split-bf16 format has a residual plane
  if (passes == 3 && (!qkv_lo || (!out_lo && d->o_fmt == EGV_ATTN_OUT_BF16_SPLIT) || !dout_lo || !dqkv_lo)) return EGV_ERR_ARG;
  // single-pass: first planes only -- except the forward's output, whose residual plane (if the caller has one: a three-pass forward)
  // makes delta = rowsum(dO o O) exact in O at no cost
  if (passes == 1) d->qkv_lo = d->dout_lo = d->dqkv_lo = false;
  return EGV_OK;
}

// egv_text_attn_*: B captions of L tokens, H heads; ld = elements between consecutive tokens of q / k / v (of dq / dk / dv)
inline int att_check_text_sizes(int B, int L, int H, int passes, int64_t ld, float dropout_p) {
  if (B <= 0 || L <= 0 || H <= 0 || (passes != 1 && passes != 3)) return EGV_ERR_ARG;
  if (ld < (int64_t)H * 64 || ld % 4 != 0) return EGV_ERR_ARG;
  return (dropout_p >= 0.f && dropout_p < 1.f) ? EGV_OK : EGV_ERR_ARG;      // a NaN is refused
}
inline int att_check_text_fwd(int B, int L, int H, int passes, bool required, bool* out_lo, int64_t ldqkv, float dropout_p) {
  if (!required || att_check_text_sizes(B, L, H, passes, ldqkv, dropout_p)) return EGV_ERR_ARG;
  if (passes == 3 && !*out_lo) return EGV_ERR_ARG;
  if (passes == 1) *out_lo = false;
  return EGV_OK;
}
inline int att_check_text_bwd(int B, int L, int H, int passes, bool required, int64_t ldqkv, int64_t lddqkv, float dropout_p) {
  if (!required || att_check_text_sizes(B, L, H, passes, ldqkv, dropout_p)) return EGV_ERR_ARG;
  return att_check_text_sizes(B, L, H, passes, lddqkv, dropout_p);
}

// -------------------------------------------------------------------------------------------------------------------- picks
enum AttFamily {
  ATT_RESIDENT,           // all K / V (dK / dV: Q / dO) of a group in LDS, a query tile's scores in registers: up to 288 rows
  ATT_STREAM,             // space, 65 .. 288 rows: the same LDS image, 16 (8) waves that stream the score fragments
  ATT_TEXT_STREAM,        // text dQ, 65 .. 288 rows: two walks over the keys (delta, then dQ)
  ATT_KEY_TILED,          // more than 288 rows: 64-row tiles through a two-buffer ring
  ATT_TIME_TILE,          // time, T <= 16: one 16-row tile per wave holds 16 / TP locations
  ATT_TIME_LONG           // time, 16 < T <= 64: NT = ceil(T / 16) tiles, one workgroup of NT waves per location
};

struct AttPick {
  int family;
  int frags;              // resident / streaming: NKF = NF 16-row fragments; time-tile: TP; time-long: NT; key-tiled: 0
  int products;           // 1 or 3 MFMA products per multiply
  int f16;                // fp16 operands
  int waves;              // per workgroup
  int threads, lds, grid; // block, dynamic LDS bytes (0: the kernel's LDS is static), blocks
  int nblk;               // key-tiled: 128-row blocks per group (a kernel argument); 1 elsewhere
};

inline int att_pick_set(AttPick* p, int family, int frags, int products, int f16, int waves, int64_t lds, int64_t blocks, int64_t nblk = 1) {
  if (blocks < 1 || blocks > ATT_MAX_GRID) return EGV_ERR_ARG;
  *p = {family, frags, products, f16, waves, 64 * waves, (int)lds, (int)blocks, (int)nblk};
  return EGV_OK;
}

inline int64_t att_space_groups(int B, int T, int H) { return (int64_t)B * T * H; }      // text: B H
inline int64_t att_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the padded row count as 16-row fragments: 2 (DistilBERT L <= 32, the tiny test configs), 4, 14 (ViT-B/16: 197 keys), 18 (ViT-L/14: 257);
// 0: more than 288 rows (higher input resolutions, long captions), the key-tiled kernels
inline int att_row_frags(int rows) { return rows <= 32 ? 2 : rows <= 64 ? 4 : rows <= 224 ? 14 : rows <= 288 ? 18 : 0; }

// `nvec` fp32 vectors ride with the operand planes: the key bias (forward, streaming dQ), lse and delta (the other backward kernels)
constexpr int64_t att_resident_lds(int frags, int products, int nvec) { return (int64_t)frags * 16 * ((products == 3 ? 4 : 2) * 128 + nvec * 4); }
constexpr int64_t att_tiled_lds(int products, int nvec) { return 2 * att_resident_lds(ATT_TILE_ROWS / 16, products, nvec); }

// Space (space = true: `groups` = B T H, nq = n + 1 query rows with the CLS query, nk = n + 1 keys) and text (groups = B H,
// nq = nk = L).  In the backward ONE fragment count covers both the key and the query extent.
inline int att_pick_fwd(bool space, int64_t groups, int nq, int nk, int products, int f16, AttPick* p) {
  if (groups < 1 || groups > ATT_MAX_GRID) return EGV_ERR_ARG;      // a kernel argument of the persistent kernel
  const int frags = att_row_frags(nk);
  if (!frags) {
    const int64_t nqb = att_ceil_div(nq, ATT_TILE_WAVES * 16);
    return att_pick_set(p, ATT_KEY_TILED, 0, products, f16, ATT_TILE_WAVES, att_tiled_lds(products, 1), groups * nqb, nqb);
  }
  const int64_t lds = att_resident_lds(frags, products, 1);
  // a three-product space forward of the 197- / 257-key sizes always streams (13 / 17 query tiles on 16 waves; the register-resident
  // instance would spill); three-product mode keeps four planes in LDS (one workgroup per CU), so every resident instance runs 8 waves
  if (space && frags >= 14 && products == 3)
    return att_pick_set(p, ATT_STREAM, frags, products, f16, 16, lds, groups < ATT_PERSIST_WGS ? groups : ATT_PERSIST_WGS);
  return att_pick_set(p, ATT_RESIDENT, frags, products, f16, 8, lds, groups);
}
inline int att_pick_dq(bool space, int64_t groups, int nq, int nk, int products, int f16, AttPick* p) {
  const int frags = att_row_frags(nk > nq ? nk : nq);
  if (!frags) {
    const int64_t nqb = att_ceil_div(nq, ATT_TILE_WAVES * 16);
    return att_pick_set(p, ATT_KEY_TILED, 0, products, f16, ATT_TILE_WAVES, att_tiled_lds(products, 1), groups * nqb, nqb);
  }
  if (frags >= 14 && space)
    return att_pick_set(p, ATT_STREAM, frags, products, f16, products == 3 ? 16 : 8, att_resident_lds(frags, products, 1), groups);
  return att_pick_set(p, frags >= 14 ? ATT_TEXT_STREAM : ATT_RESIDENT, frags, products, f16, (products == 3 && frags < 14) ? 4 : 8,
                      att_resident_lds(frags, products, 2), groups);
}
inline int att_pick_dkv(bool /*space: one dK / dV kernel serves both*/, int64_t groups, int nq, int nk, int products, int f16, AttPick* p) {
  const int frags = att_row_frags(nk > nq ? nk : nq);
  if (!frags) {
    const int64_t nkb = att_ceil_div(nk, ATT_TILE_WAVES * 16);
    return att_pick_set(p, ATT_KEY_TILED, 0, products, f16, ATT_TILE_WAVES, att_tiled_lds(products, 2), groups * nkb, nkb);
  }
  return att_pick_set(p, ATT_RESIDENT, frags, products, f16, products == 3 ? 4 : 8, att_resident_lds(frags, products, 2), groups);
}

// Time: T <= 16 frames are TP = 4, 8 or 16 rows of a 16-row tile, a wave owns 16 / TP locations of one (clip, head): forward 4 waves per
// block over all (clip, unit, head); backward WPB = 4 (three products: 2) consecutive units of ONE (clip, head) per block.
// 16 < T <= 64: NT = 2, 3 or 4 tiles, one workgroup of NT waves per (clip, location, head).  The kernels' LDS is static.
inline int att_pick_time(bool bwd, int B, int T, int n, int H, int products, int f16, AttPick* p) {
  if (T < 1 || T > ATT_MAX_FRAMES) return EGV_ERR_ARG;
  if (T > 16) return att_pick_set(p, ATT_TIME_LONG, (T + 15) / 16, products, f16, (T + 15) / 16, 0, (int64_t)B * n * H);
  const int tp = T <= 4 ? 4 : T <= 8 ? 8 : 16;
  const int64_t units = att_ceil_div(n, 16 / tp);
  if (!bwd) return att_pick_set(p, ATT_TIME_TILE, tp, products, f16, 4, 0, att_ceil_div((int64_t)B * units * H, 4));
  const int wpb = products == 3 ? 2 : 4;
  return att_pick_set(p, ATT_TIME_TILE, tp, products, f16, wpb, 0, (int64_t)B * H * att_ceil_div(units, wpb));
}

// ----------------------------------------------------------------------------------------------- across the attention files
#ifdef __HIPCC__
#include "common.h"

struct AttGeom;
struct AttGrad;

// what a time-attention call carries from the entry point to the launch: the kernels' own arguments
struct AttTimeFwd {
  const bf16_t *qh, *ql;
  int B, T, n, H;
  bf16_t *oh, *ol;
  float *lse, *ws;
  int out_fmt;
};
struct AttTimeBwd {
  const bf16_t *qh, *ql, *doh, *dol;
  const float *lse, *delta;
  int B, T, n, H;
  bf16_t *gh, *gl;
  float* dcls;
  int gfmt;
};

// attn_mfma_fwd.hip / attn_mfma_bwd.hip: the space attention of a checked and picked call
int egv_attn_space_fwd_impl(const AttPick& p, const bf16_t* qkv_hi, const bf16_t* qkv_lo, int B, int T, int n, int H, bf16_t* out_hi,
                            bf16_t* out_lo, float* lse, float* cls_ws, int out_fmt, hipStream_t s);
int egv_attn_space_bwd_impl(const AttPick& dq, const AttPick& dkv, const bf16_t* qkv_hi, const bf16_t* qkv_lo, const bf16_t* out_hi,
                            const bf16_t* out_lo, const bf16_t* do_hi, const bf16_t* do_lo, const float* lse, float* delta, float* dcls,
                            int B, int T, int n, int H, bf16_t* dqkv_hi, bf16_t* dqkv_lo, int o_fmt, int g_fmt, hipStream_t s);
// attn_long.hip (ATT_KEY_TILED); `mode` is MODE_SPACE or MODE_TEXT
int egv_attn_long_fwd(int mode, const AttPick& p, const AttGeom& g, bf16_t* oh, bf16_t* ol, long ostride, float* lse, float* cls_ws,
                      hipStream_t s);
int egv_attn_long_bwd(int mode, const AttPick& dq, const AttPick& dkv, const AttGeom& g, const AttGrad& gr, hipStream_t s);
// attn_time_mfma.hip (ATT_TIME_TILE), attn_time_long.hip (ATT_TIME_LONG)
int egv_attn_time_tile_fwd(const AttPick& p, const AttTimeFwd& a, hipStream_t s);
int egv_attn_time_tile_bwd(const AttPick& p, const AttTimeBwd& a, hipStream_t s);
int egv_attn_time_long_fwd(const AttPick& p, const AttTimeFwd& a, hipStream_t s);
int egv_attn_time_long_bwd(const AttPick& p, const AttTimeBwd& a, hipStream_t s);
// attn_small.hip: the CLS row's combine (forward), delta (backward prologue: also zeroes dcls) and finish kernels, B H blocks each
int egv_attn_cls_combine_impl(const float* ws, int B, int G, int S, int H, bf16_t* oh, bf16_t* ol, float* lse, int out_fmt,
                              hipStream_t s);
int egv_attn_cls_delta_impl(const bf16_t* oh, const bf16_t* ol, const bf16_t* doh, const bf16_t* dol, int B, int S, int H,
                            float* delta, float* dcls, int o_fmt, int f16, hipStream_t s);
int egv_attn_cls_finish_impl(const float* dcls, int B, int S, int H, bf16_t* gh, bf16_t* gl, int gfmt, hipStream_t s);
#endif
