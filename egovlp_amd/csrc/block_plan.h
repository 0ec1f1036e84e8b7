// The operand-format plan of one SpaceTimeBlock call: which geometries egv_block_fwd / _bwd accept, and -- a function of fwd_passes,
// bwd_passes, f16_single, train and z_bf16 alone -- how many products each of the six Linears runs on which planes, which planes every
// hand-over between two kernels has and in which format, what the backward reads and writes, and from that the layout of the two
// arenas.  Each decision is stated here once; block.hip checks, plans, lays out and enqueues.  Plain C++
// (tests/test_block_plan_cpu.py compiles it on its own; model/layer_common.py::block_plan is its Python mirror, pinned there).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "egovlp_hip.h"
#include "layer_call.h"

// the six Linears, in the order of egv_block_params
enum { LIN_TQKV, LIN_TPROJ, LIN_SQKV, LIN_SPROJ, LIN_FC1, LIN_FC2 };
// first operand of a forward Linear, of the (first, second) plane pair its producer wrote
enum { OPND_BOTH, OPND_FIRST, OPND_SECOND };
enum { WFMT_BF16, WFMT_F16X2 };          // weight planes: split-bf16 (hi[, lo]) or the f16x2 encoding (csrc/f16x2.h, second-operand role)

constexpr float BLOCK_A1_INV = 1.0f / (1.0f - 0.015625f);      // csrc/f16x2.h: a1 = fp16((1 - 2^-6) x)

// train, tail: egv_block_geom.train EGV_TRAIN_KEEP (keep what the backward needs), EGV_TRAIN_CLS_TAIL
// ---- per Linear
// passes      forward products, as egv_gemm_desc.passes: 1 bf16, 3 split-bf16, 2 f16x2, 4 ONE fp16 product
// operand     OPND_*: which saved planes are its first operand (the proj Linears read the attention's SECOND plane alone when that
//             plane holds fp16(value) next to a bf16 plane, EGV_ATTN_OUT_BF16_F16)
// w_fmt       WFMT_*: the format of w_hi / w_lo it multiplies;  w_lo: the forward reads w_lo (every format but one bf16 product)
// walpha      weight-gradient rescale: 1 / (1 - 2^-6) where the fp16 backward reads a1 of an f16x2 encoding as X
// ---- per hand-over: planes and formats
// ln_f16      LayerNorm outputs through egv_layernorm_fwd_f16x2 (fp16 planes) instead of split-bf16
// lnq_lo, ln2_lo, qkv_lo, attn_lo, h_lo   second plane of norm3 / norm1 (-> qkv), of norm2 (-> fc1), of qkv, the attention outputs, h
// bf          bf16 copies of the LayerNorm outputs and of h: the single-pass bf16 backward of an f16x2 forward reads them
// qkv_fmt     out_fmt of the qkv GEMMs: EGV_OUT_BF16_SPLIT, or EGV_OUT_F16_SPLIT (the fp16 attention's operands)
// attn_passes attention forward: split-bf16 three-product operands in the f16x2 mode
// attn_fmt    what the attention writes, EGV_ATTN_OUT_*: split-bf16, bf16 + fp16(value), f16x2 planes, ONE plane of fp16(value)
// attn_mode_fwd, attn_mode_bwd   the mode words of egv_divided_attn_fwd / _bwd without EGV_ATTN_TIME (block_attn_mode adds it)
// kv_fmt      egv_cls_attn_*: EGV_CLS_KV_BF16 or EGV_CLS_KV_F16 planes (k / v operands and, in the backward, dk / dv)
// h_fmt       out_fmt of fc1: EGV_OUT_BF16_SPLIT, EGV_OUT_F16X2, or EGV_OUT_F16 (ONE plain fp16 plane)
// z_code      aux_bf16 of fc1 / the fc2 dgrad: EGV_AUX_F32 (the pre-activation), EGV_AUX_DGELU_BF16, EGV_AUX_DGELU_F16;  z_bytes per element, 0: not kept
// ---- backward
// bwd_passes  passes of every GEMM of the backward (4: one fp16 product on un-clamped fp16 gradients)
// bwd_lo      three-product backward: lo planes of gradients, saved operands and W^T;  saved_bf: its activation operands are the bf16 copies
// grad_fmt    out_fmt of dZ, dO and the three LayerNorm-backward inputs: EGV_OUT_BF16_SPLIT (LayerNorm inputs: fp32) or EGV_OUT_F16_GRAD
// ln_fmt      dx_fmt of egv_layernorm_bwd_partial (EGV_LN_* bits);  attn_bwd_passes: of egv_divided_attn_bwd
// attn_bwd_o_lo  the attention backward is handed O's second plane (delta exact in O) -- not when that plane is fp16
// cls_dx_mode egv_cls_linear_dgrad onto the d_n1 the big dgrad wrote: EGV_CLS_DX_ADD_F32, or _ADD_F16 (a plane of un-clamped fp16)
struct BlockPlan {
  bool train, tail;
  int passes[6], operand[6], w_fmt[6];
  float walpha[6];
  bool w_lo, ln_f16, lnq_lo, ln2_lo, qkv_lo, attn_lo, h_lo, bf;
  int qkv_fmt, attn_passes, attn_fmt, attn_mode_fwd, attn_mode_bwd, kv_fmt, h_fmt, z_code, z_bytes;
  int bwd_passes, grad_fmt, ln_fmt, attn_bwd_passes, cls_dx_mode;
  bool bwd_lo, saved_bf, attn_bwd_o_lo;
};

inline int block_check(const egv_block_geom& g) {
  if (g.B <= 0 || g.T <= 0 || g.n <= 0 || g.H <= 0 || g.D != g.H * 64 || g.Hd <= 0 || g.D % 32 || g.Hd % 32) return EGV_ERR_ARG;
  const int P = g.fwd_passes, Pb = g.bwd_passes;
  // (forward, backward): bf16 (1, 1); split-bf16 three-product (3, 3) or (3, 1); f16x2 (2, 1), or (2, 4): one FP16 product on scaled
  // gradients, which reads the forward's own fp16 planes
  if (!((Pb == 1 && P >= 1 && P <= 3) || (Pb == 3 && P == 3) || (Pb == 4 && P == 2))) return EGV_ERR_ARG;
  if (g.train < 0 || g.train > (EGV_TRAIN_KEEP | EGV_TRAIN_CLS_TAIL)) return EGV_ERR_ARG;
  if (P == 2 && (g.train & EGV_TRAIN_KEEP) && !g.z_bf16) return EGV_ERR_ARG;      // the fc1 epilogue of the f16x2 format saves gelu' in 16 bits
  if (g.f16_single < 0 || g.f16_single > (EGV_SINGLE_FC1 | EGV_SINGLE_FC2 | EGV_SINGLE_QKV | EGV_SINGLE_PROJ) || (g.f16_single && P != 2)) return EGV_ERR_ARG;
  return EGV_OK;
}

inline BlockPlan block_plan(const egv_block_geom& g) {
  BlockPlan pl = {};
  const int P = g.fwd_passes;
  const bool x2 = P == 2, h16 = g.bwd_passes == 4, lo = P != 1;      // h16, the fp16 backward: no bf16 copies, fp16 planes only
  const int s = g.f16_single;
  const bool one[6] = {(s & EGV_SINGLE_QKV) != 0, (s & EGV_SINGLE_PROJ) != 0, (s & EGV_SINGLE_QKV) != 0, (s & EGV_SINGLE_PROJ) != 0,
                       (s & EGV_SINGLE_FC1) != 0, (s & EGV_SINGLE_FC2) != 0};      // ONE fp16 product
  pl.train = (g.train & EGV_TRAIN_KEEP) != 0;
  pl.tail = (g.train & EGV_TRAIN_CLS_TAIL) != 0;
  pl.attn_passes = x2 ? 3 : P;
  pl.attn_fmt = h16 ? (one[LIN_TPROJ] ? EGV_ATTN_OUT_F16 : EGV_ATTN_OUT_F16X2) : (one[LIN_TPROJ] ? EGV_ATTN_OUT_BF16_F16 : EGV_ATTN_OUT_BF16_SPLIT);
  for (int i = 0; i < 6; ++i) {
    if (i == LIN_TPROJ || i == LIN_SPROJ) {      // by attention format: bf16 planes; fp16(value) beside them; f16x2 planes; fp16(value) alone
      const int passes[4] = {pl.attn_passes, 4, 2, 4}, operand[4] = {OPND_BOTH, OPND_SECOND, OPND_BOTH, OPND_FIRST};
      pl.passes[i] = passes[pl.attn_fmt];
      pl.operand[i] = operand[pl.attn_fmt];
      pl.w_fmt[i] = pl.attn_fmt != EGV_ATTN_OUT_BF16_SPLIT ? WFMT_F16X2 : WFMT_BF16;
    } else {
      pl.passes[i] = one[i] ? 4 : P;
      pl.operand[i] = one[i] ? OPND_FIRST : OPND_BOTH;
      pl.w_fmt[i] = x2 ? WFMT_F16X2 : WFMT_BF16;
    }
    pl.walpha[i] = h16 && !one[i] ? BLOCK_A1_INV : 1.0f;
  }
  pl.w_lo = lo;
  pl.ln_f16 = x2;
  pl.lnq_lo = lo && !one[LIN_TQKV];
  pl.ln2_lo = lo && !one[LIN_FC1];
  pl.qkv_lo = lo;
  pl.attn_lo = lo && pl.attn_fmt != EGV_ATTN_OUT_F16;
  pl.h_lo = lo && !one[LIN_FC2];
  pl.bf = x2 && pl.train && !h16;
  pl.qkv_fmt = h16 ? EGV_OUT_F16_SPLIT : EGV_OUT_BF16_SPLIT;
  // the fp16 attention multiplies fp16 (qkv planes = an fp16 split); its backward writes dqkv as fp16 and reads q / k / v / dO as fp16
  pl.attn_mode_fwd = (pl.attn_fmt << EGV_ATTN_OUT_SHIFT) | (h16 ? EGV_ATTN_FWD_QKV_F16 : 0);
  pl.attn_mode_bwd = (pl.attn_fmt << EGV_ATTN_OUT_SHIFT) | (h16 ? EGV_ATTN_BWD_GRAD_F16 | EGV_ATTN_BWD_QKV_F16 : 0);
  pl.kv_fmt = h16 ? EGV_CLS_KV_F16 : EGV_CLS_KV_BF16;
  pl.h_fmt = x2 ? (one[LIN_FC2] ? EGV_OUT_F16 : EGV_OUT_F16X2) : EGV_OUT_BF16_SPLIT;
  pl.z_code = g.z_bf16 ? (h16 ? EGV_AUX_DGELU_F16 : EGV_AUX_DGELU_BF16) : EGV_AUX_F32;
  pl.z_bytes = pl.train ? (g.z_bf16 ? 2 : 4) : 0;
  pl.bwd_passes = g.bwd_passes;
  pl.bwd_lo = g.bwd_passes == 3;
  pl.saved_bf = x2 && !h16;
  pl.grad_fmt = h16 ? EGV_OUT_F16_GRAD : EGV_OUT_BF16_SPLIT;
  pl.ln_fmt = h16 ? EGV_LN_DX_F16 | EGV_LN_DY_F16 : 0;
  pl.attn_bwd_passes = h16 ? 1 : g.bwd_passes;
  pl.attn_bwd_o_lo = pl.attn_fmt == EGV_ATTN_OUT_BF16_SPLIT;
  pl.cls_dx_mode = h16 ? EGV_CLS_DX_ADD_F16 : EGV_CLS_DX_ADD_F32;
  return pl;
}

// the mode word of one attention branch: the plan's word and the branch bit
inline int block_attn_mode(int word, int time) { return word | (time ? EGV_ATTN_TIME : 0); }

// ------------------------------------------------------------------------------------------------------------------- geometry
// tokens, tokens per clip, widths, and (N, K) of W[N,K] in the order of egv_block_params: tqkv, tproj, sqkv, sproj, fc1, fc2
struct Geo { int64_t M, S, D, Hd, nk[6][2]; };

inline Geo geo_of(const egv_block_geom& g) {
  const int64_t S = 1 + (int64_t)g.T * g.n, D = g.D, Hd = g.Hd;
  return {(int64_t)g.B * S, S, D, Hd, {{3 * D, D}, {D, D}, {3 * D, D}, {D, D}, {Hd, D}, {D, Hd}}};
}

// gradient buffer: [dW x 6][db x 6][dgamma3, dbeta3, dgamma1, dbeta1, dgamma2, dbeta2]
inline void grad_layout(const egv_block_geom& g, int64_t off[18], int64_t& total) {
  layer_grad_layout(geo_of(g).nk, 6, g.D, 6, off, total);
}

// ------------------------------------------------------------------------------------------------------------- the two arenas
// what one attention branch (LayerNorm -> qkv -> attention; time: norm3, space: norm1) leaves in the forward arena
struct FwdBranch { int64_t n_hi, n_lo, mean, rstd, qkv_hi, qkv_lo, a_hi, a_lo, lse, work, n_bf; };

// forward arena: what the block's kernels hand to each other and what the backward needs again (-1: absent)
struct FwdLayout {
  FwdBranch t, s;
  int64_t tr, sr, n2_hi, n2_lo, mean2, rstd2, h_hi, h_lo, z;
  int64_t n2_bf, h_bf;     // (and t.n_bf, s.n_bf) f16x2 forward of a training step: bf16 copies for the single-pass bf16 backward
  // CLS-tail mode: fp32 [B, .] rows -- LN1(tr) and its scratch statistics, the CLS query, the attention output, LN2's output,
  // gelu(fc1).  There s.qkv_* are the k | v planes [M, 2 D], s.lse is [B, H], sr / mean2 / rstd2 / z hold B rows (z: the fp32
  // pre-activation) and s.a_*, s.work, n2_*, h_*, n2_bf, h_bf are absent.
  int64_t n1c, mean1c, rstd1c, qc, oc, n2c, hc;
  int64_t total;
};

inline FwdLayout fwd_layout(const egv_block_geom& g, const BlockPlan& pl) {
  const Geo o = geo_of(g);
  FwdLayout L;
  Bump b;
  auto plane = [&](int64_t cols, bool there = true) { return there ? b.take(o.M * cols * 2) : (int64_t)-1; };
  // LayerNorm output and statistics, qkv planes [M, qkv_cols], and (attn: not behind the tail's norm1) attention output, lse, workspace
  auto branch = [&](FwdBranch& r, int64_t qkv_cols, int time, bool attn) {
    r.n_hi = plane(o.D); r.n_lo = plane(o.D, pl.lnq_lo);
    r.mean = b.take(o.M * 4); r.rstd = b.take(o.M * 4);
    r.qkv_hi = plane(qkv_cols); r.qkv_lo = plane(qkv_cols, pl.qkv_lo);
    r.a_hi = plane(o.D, attn); r.a_lo = plane(o.D, attn && pl.attn_lo);
    r.lse = attn ? b.take((int64_t)g.B * g.H * o.S * 4) : b.take((int64_t)g.B * g.H * 4);
    r.work = attn ? b.take(egv_divided_attn_fwd_work_floats(g.B, g.T, g.n, g.H, time) * 4) : (int64_t)-1;
  };
  branch(L.t, 3 * o.D, 1, true);
  L.tr = b.take(o.M * o.D * 4);
  L.n1c = L.mean1c = L.rstd1c = L.qc = L.oc = L.n2c = L.hc = -1;
  if (pl.tail) {
    const int64_t B = g.B;
    branch(L.s, 2 * o.D, 0, false);
    L.n2_hi = L.n2_lo = L.h_hi = L.h_lo = L.n2_bf = L.h_bf = -1;
    L.n1c = b.take(B * o.D * 4); L.mean1c = b.take(B * 4); L.rstd1c = b.take(B * 4);
    L.qc = b.take(B * o.D * 4); L.oc = b.take(B * o.D * 4);
    L.sr = b.take(B * o.D * 4);
    L.n2c = b.take(B * o.D * 4); L.mean2 = b.take(B * 4); L.rstd2 = b.take(B * 4);
    L.hc = b.take(B * o.Hd * 4);
    L.z = pl.train ? b.take(B * o.Hd * 4) : (int64_t)-1;
    L.t.n_bf = plane(o.D, pl.bf); L.s.n_bf = plane(o.D, pl.bf);
    L.total = b.off;
    return L;
  }
  branch(L.s, 3 * o.D, 0, true);
  L.sr = b.take(o.M * o.D * 4);
  L.n2_hi = plane(o.D); L.n2_lo = plane(o.D, pl.ln2_lo);
  L.mean2 = b.take(o.M * 4); L.rstd2 = b.take(o.M * 4);
  L.h_hi = plane(o.Hd); L.h_lo = plane(o.Hd, pl.h_lo);
  L.z = pl.z_bytes ? b.take(o.M * o.Hd * pl.z_bytes) : (int64_t)-1;
  L.t.n_bf = plane(o.D, pl.bf); L.s.n_bf = plane(o.D, pl.bf); L.n2_bf = plane(o.D, pl.bf); L.h_bf = plane(o.Hd, pl.bf);
  L.total = b.off;
  return L;
}

// what the backward of one attention branch writes: the gradient of the branch output (fp32 and planes, from the LayerNorm backward
// behind it), dO, dqkv, and the input of the LayerNorm backward in front of it (fp32, or one fp16 plane in the same buffer)
struct BwdBranch { int64_t d_res, dres_hi, dres_lo, do_hi, do_lo, dqkv_hi, dqkv_lo, d_n; };

struct BwdLayout {
  int64_t g_hi, g_lo, dz_hi, dz_lo, d_n2;
  BwdBranch s, t;
  int64_t ln_work[3], attn_work, partial[6];
  // CLS-tail mode: fp32 [B, .] rows (dZ, d_n2, d_sr, dO, dq of the CLS rows), the two-stage dgrad's slabs; s.dqkv_* are the dk | dv
  // planes [M, 2 D] there and g_*, dz_*, d_n2, s.d_res, s.dres_*, s.do_* are absent
  int64_t dzc, dn2c, dsrc, doc, dqc, lin_work;
  int64_t total;
};

inline BwdLayout bwd_layout(const egv_block_geom& g, const BlockPlan& pl, const int32_t* ksplit) {
  const Geo o = geo_of(g);
  BwdLayout L;
  Bump b;
  auto plane = [&](int64_t cols, bool there = true) { return there ? b.take(o.M * cols * 2) : (int64_t)-1; };
  auto branch = [&](BwdBranch& r, int64_t qkv_cols, bool full) {
    r.d_res = full ? b.take(o.M * o.D * 4) : (int64_t)-1;
    r.dres_hi = plane(o.D, full); r.dres_lo = plane(o.D, full && pl.bwd_lo);
    r.do_hi = plane(o.D, full); r.do_lo = plane(o.D, full && pl.bwd_lo);
    r.dqkv_hi = plane(qkv_cols); r.dqkv_lo = plane(qkv_cols, pl.bwd_lo);
  };
  L.dzc = L.dn2c = L.dsrc = L.doc = L.dqc = L.lin_work = -1;
  if (pl.tail) {
    const int64_t B = g.B;
    L.g_hi = L.g_lo = L.dz_hi = L.dz_lo = L.d_n2 = -1;
    L.dzc = b.take(B * o.Hd * 4); L.dn2c = b.take(B * o.D * 4); L.dsrc = b.take(B * o.D * 4); L.doc = b.take(B * o.D * 4);
    L.dqc = b.take(B * o.D * 4);
    L.lin_work = b.take(egv_cls_linear_work_floats(g.B, (int32_t)std::max(o.D, o.Hd), (int32_t)std::max(o.D, o.Hd)) * 4);
    branch(L.s, 2 * o.D, false);
  } else {
    L.g_hi = plane(o.D); L.g_lo = plane(o.D, pl.bwd_lo);
    L.dz_hi = plane(o.Hd); L.dz_lo = plane(o.Hd, pl.bwd_lo);
    L.d_n2 = b.take(o.M * o.D * 4);
    branch(L.s, 3 * o.D, true);
  }
  L.s.d_n = b.take(o.M * o.D * 4);
  branch(L.t, 3 * o.D, true);
  L.t.d_n = b.take(o.M * o.D * 4);
  for (int i = 0; i < 3; ++i) L.ln_work[i] = b.take(2 * o.D * (int64_t)egv_layernorm_bwd_parts((int32_t)o.M) * 4);   // one per LayerNorm: reduced together at the end
  L.attn_work = b.take(egv_divided_attn_bwd_work_floats(g.B, g.T, g.n, g.H) * 4);
  for (int i = 0; i < 6; ++i) {
    const int ks = (ksplit && !(pl.tail && i > LIN_SQKV)) ? ksplit[i] : 1;      // tail: the space proj / fc1 / fc2 gradients are rank-B updates
    const int64_t N = pl.tail && i == LIN_SQKV ? 2 * o.D : o.nk[i][0];              // and the space qkv GEMM covers the k / v rows
    L.partial[i] = ks > 1 ? b.take((int64_t)ks * (N * o.nk[i][1] + N) * 4) : (int64_t)-1;
  }
  L.total = b.off;
  return L;
}
