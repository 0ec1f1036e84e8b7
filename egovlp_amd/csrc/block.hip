// One C-ABI call per SpaceTimeBlock forward and one per backward (model/video_transformer.py:163-177 and its autograd
// transpose): the host enqueues the block's ~11 / ~25 kernels from C with pointers into ONE workspace arena per direction, instead
// of ~50 Python-level tensor allocations and ~30 ctypes calls.  Nothing new is computed here: every launch below is one of the
// library's own entry points (egv_layernorm_*, egv_gemm_nt, egv_divided_attn_*), with the arguments the per-kernel Python path
// (egovlp_amd/model/video_transformer.py::_SpaceTimeBlockFn, kept as the reference) gives them, in the same order -- results are
// bit-identical (tests/test_gpu_block.py).  Which geometries are accepted, every operand format and the layout of the two arenas are
// csrc/block_plan.h's; a call here is check, plan, layout, enqueue.
// CLS-tail mode (egv_block_geom.train EGV_TRAIN_CLS_TAIL, the tower's last block): only the B CLS rows of the output are wanted, so what follows the
// k / v projection of the space branch runs on B rows through the egv_cls_* entry points (csrc/cls_tail.hip; tests/test_gpu_cls_tail.py).
#include <hip/hip_runtime.h>

#include "common.h"
#include "block_plan.h"

namespace {

// What both directions need before they enqueue -- the plan, the forward layout, the sizes -- and the forward.
struct Call {
  const egv_block_geom& g;
  const egv_block_params& p;
  const BlockPlan pl;
  const Geo o;
  const FwdLayout F;
  const int32_t M, D, Hd;
  void* stream;
  Call(const egv_block_geom& g_, const egv_block_params& p_, void* stream_)
      : g(g_), p(p_), pl(block_plan(g_)), o(geo_of(g_)), F(fwd_layout(g_, pl)), M((int32_t)o.M), D((int32_t)o.D), Hd((int32_t)o.Hd), stream(stream_) {}

  // forward Linear i on the plane pair (first, second) its producer wrote (rows = 0: every row of W; else `rows` rows from `row0`)
  egv_gemm_desc linear(int i, const egv_bf16* first, const egv_bf16* second, int64_t row0 = 0, int64_t rows = 0) const {
    const int opnd = pl.operand[i];
    const int64_t N = rows ? rows : o.nk[i][0], K = o.nk[i][1], skip = row0 * p.ldw[i];
    egv_gemm_desc d = nt_desc(opnd == OPND_SECOND ? second : first, opnd == OPND_BOTH ? second : nullptr, K, p.w_hi[i] + skip,
                              p.w_lo[i] ? p.w_lo[i] + skip : nullptr, p.ldw[i], M, N, K, pl.passes[i], g.grid_cap);
    d.bias = p.bias[i] + row0;
    return d;
  }

  // LayerNorm -> operand planes of the qkv / fc1 Linears: split-bf16, or fp16 planes (+ the bf16 copy the backward reads)
  int layernorm(char* A, const float* in, const float* gw, const float* gb, int64_t y_hi, int64_t y_lo, int64_t y_bf, int64_t mean, int64_t rstd) const {
    if (pl.ln_f16)
      return egv_layernorm_fwd_f16x2(in, D, gw, gb, g.eps, M, D, at<uint16_t>(A, y_hi), at<uint16_t>(A, y_lo), at<egv_bf16>(A, y_bf), D,
                                     at<float>(A, mean), at<float>(A, rstd), stream);
    return egv_layernorm_fwd(in, nullptr, D, gw, gb, g.eps, M, D, nullptr, at<egv_bf16>(A, y_hi), at<egv_bf16>(A, y_lo), nullptr, D,
                             at<float>(A, mean), at<float>(A, rstd), stream);
  }

  // the qkv Linear of a branch (weight wi) on its LayerNorm output; the tail's covers the k / v rows D .. 3 D of W[3 D, D]
  int qkv_linear(char* A, const FwdBranch& r, int wi, int64_t row0 = 0, int64_t rows = 0) const {
    egv_gemm_desc d = linear(wi, at<egv_bf16>(A, r.n_hi), at<egv_bf16>(A, r.n_lo), row0, rows);
    d.out_hi = at<egv_bf16>(A, r.qkv_hi); d.out_lo = at<egv_bf16>(A, r.qkv_lo); d.ldoh = d.N;
    d.out_fmt = pl.qkv_fmt;
    return egv_gemm_nt(&d, stream);
  }

  // one attention branch: res = x + proj(attention(qkv(LayerNorm(in)))) -- time: norm3, weights 0 / 1; space: norm1, weights 2 / 3
  int attn_branch(char* A, const FwdBranch& r, int time, const float* in, const float* gw, const float* gb, const float* x, float* res) const {
    const int wi = time ? LIN_TQKV : LIN_SQKV;
    EGV_TRY(layernorm(A, in, gw, gb, r.n_hi, r.n_lo, r.n_bf, r.mean, r.rstd));
    EGV_TRY(qkv_linear(A, r, wi));
    egv_bf16 *a_hi = at<egv_bf16>(A, r.a_hi), *a_lo = at<egv_bf16>(A, r.a_lo);
    EGV_TRY(egv_divided_attn_fwd(at<egv_bf16>(A, r.qkv_hi), at<egv_bf16>(A, r.qkv_lo), g.B, g.T, g.n, g.H, block_attn_mode(pl.attn_mode_fwd, time), pl.attn_passes,
                                 a_hi, a_lo, at<float>(A, r.lse), at<float>(A, r.work), stream));
    egv_gemm_desc d = linear(wi + 1, a_hi, a_lo);
    d.residual = x; d.ldr = D; d.out_f32 = res; d.ldo = D;
    return egv_gemm_nt(&d, stream);
  }

  int forward(const float* x, float* out, char* A) const {
    for (int i = 0; i < (pl.tail ? 3 : 6); ++i)
      if (!p.w_hi[i] || (pl.w_lo && !p.w_lo[i])) return EGV_ERR_ARG;
    const FwdLayout& L = F;
    float *tr = at<float>(A, L.tr), *sr = at<float>(A, L.sr);
    // ---- temporal attention branch (:166-167)
    EGV_TRY(attn_branch(A, L.t, 1, x, p.n3w, p.n3b, x, tr));
    if (pl.tail) {
      // ---- CLS tail: only the B CLS rows of `out` are wanted (out is [B, D]).  norm1 and k / v of every token (rows D .. 3 D of the qkv
      // weight) as in the full branch; everything behind them on B rows, in fp32 from the master weights (csrc/cls_tail.hip)
      EGV_TRY(layernorm(A, tr, p.n1w, p.n1b, L.s.n_hi, L.s.n_lo, L.s.n_bf, L.s.mean, L.s.rstd));
      const float *w_q = (const float*)p.wt_hi[2], *w_proj = (const float*)p.wt_hi[3], *w_fc1 = (const float*)p.wt_hi[4],
                  *w_fc2 = (const float*)p.wt_hi[5];
      if (!w_q || !w_proj || !w_fc1 || !w_fc2) return EGV_ERR_ARG;
      const int32_t B = g.B;
      const int64_t ldc = o.S * o.D;       // from one clip's CLS row to the next
      EGV_TRY(qkv_linear(A, L.s, LIN_SQKV, D, 2 * D));
      float *n1c = at<float>(A, L.n1c), *qc = at<float>(A, L.qc), *oc = at<float>(A, L.oc), *n2c = at<float>(A, L.n2c), *hc = at<float>(A, L.hc);
      EGV_TRY(egv_layernorm_fwd(tr, nullptr, ldc, p.n1w, p.n1b, g.eps, B, D, nullptr, nullptr, nullptr, n1c, D, at<float>(A, L.mean1c),
                                at<float>(A, L.rstd1c), stream));
      EGV_TRY(egv_cls_linear_fwd(n1c, D, w_q, D, p.bias[2], B, D, D, EGV_ACT_NONE, nullptr, nullptr, 0, qc, D, stream));
      const uint16_t *kv_hi = at<uint16_t>(A, L.s.qkv_hi), *kv_lo = at<uint16_t>(A, L.s.qkv_lo);
      EGV_TRY(egv_cls_attn_fwd(qc, D, kv_hi, kv_lo, kv_hi + D, kv_lo ? kv_lo + D : nullptr, 2 * D, pl.kv_fmt, B, (int32_t)o.S, g.H, oc, D,
                               at<float>(A, L.s.lse), stream));
      EGV_TRY(egv_cls_linear_fwd(oc, D, w_proj, D, p.bias[3], B, D, D, EGV_ACT_NONE, nullptr, x, ldc, sr, D, stream));
      EGV_TRY(egv_layernorm_fwd(sr, nullptr, D, p.n2w, p.n2b, g.eps, B, D, nullptr, nullptr, nullptr, n2c, D, at<float>(A, L.mean2),
                                at<float>(A, L.rstd2), stream));
      EGV_TRY(egv_cls_linear_fwd(n2c, D, w_fc1, D, p.bias[4], B, Hd, D, EGV_ACT_GELU, at<float>(A, L.z), nullptr, 0, hc, Hd, stream));
      return egv_cls_linear_fwd(hc, Hd, w_fc2, Hd, p.bias[5], B, D, Hd, EGV_ACT_NONE, nullptr, sr, D, out, D, stream);
    }
    // ---- spatial attention branch (:168-171; the residual is the block INPUT x, :171)
    EGV_TRY(attn_branch(A, L.s, 0, tr, p.n1w, p.n1b, x, sr));
    // ---- MLP (:175, :46-52): exact-erf GELU in the fc1 epilogue
    EGV_TRY(layernorm(A, sr, p.n2w, p.n2b, L.n2_hi, L.n2_lo, L.n2_bf, L.mean2, L.rstd2));
    egv_bf16 *h_hi = at<egv_bf16>(A, L.h_hi), *h_lo = at<egv_bf16>(A, L.h_lo);
    egv_gemm_desc d = linear(LIN_FC1, at<egv_bf16>(A, L.n2_hi), at<egv_bf16>(A, L.n2_lo));
    d.act = EGV_ACT_GELU; d.out_hi = h_hi; d.out_lo = h_lo; d.ldoh = Hd;
    // h as fp16 operand planes (+ bf16 copy when training): the f16x2 format, or one plain plane when fc2 runs a single product
    d.out_fmt = pl.h_fmt; d.out_bf = at<egv_bf16>(A, L.h_bf);
    if (pl.train) {
      d.aux_out = at<float>(A, L.z); d.ldaux = Hd;
      d.aux_bf16 = pl.z_code;              // 16 bits: gelu'(z) itself (bf16; fp16 for the fp16 backward), else the fp32 pre-activation
    }
    EGV_TRY(egv_gemm_nt(&d, stream));
    d = linear(LIN_FC2, h_hi, h_lo);
    d.residual = sr; d.ldr = D; d.out_f32 = out; d.ldo = D;
    return egv_gemm_nt(&d, stream);
  }
};

// The backward of a call.
// The fp16 backward (bwd_passes 4).  Every gradient of the pass carries the loss scale S (egv_loss_scale_*; linear all the way, so nothing
// here knows S).  Operand planes: dY = ONE plane of un-clamped fp16 (LayerNorm-backward, the GELU' epilogue, the attention backward
// write it so; g_hi / dx_hi of the io struct are such planes too); X = plane 1 of the forward's own fp16 operand (plain fp16(x), or
// a1 = fp16((1 - e) x) of an f16x2 encoding: the weight gradient is rescaled by 1 / (1 - e)); W^T = fp16 planes in p.wt_hi.  The
// attention backward multiplies fp16 as well: q / k / v = the hi plane of the fp16-split qkv planes the forward wrote, dO = an fp16 plane
// from the proj dgrad epilogue, P and dS rounded to fp16 (2^-11 per operand; with a bf16 attention backward the weight gradients of the
// first blocks stayed at 1.8e-2 whatever the GEMMs did, profiles/r06_fp16_backward_bringup.txt).
struct Bwd : Call {
  const egv_block_bwd_io& io;
  const BwdLayout L;
  const char* FA;
  char* A;
  float* grads;
  int64_t goff[18], gtot;
  // The split-K slabs of the six weight gradients are reduced by ONE launch at the end of the call (egv_splitk_reduce_multi) when all
  // six run on the same stream -- the single wgrad side stream, or the main stream --: 12 reduce launches per step instead of 72 on
  // the stream whose queue drains last.  Weight gradients dealt to different streams keep their own reduce.
  bool defer_reduce;

  Bwd(const egv_block_geom& g_, const egv_block_params& p_, const egv_block_bwd_io& io_, void* stream_)
      : Call(g_, p_, stream_), io(io_), L(bwd_layout(g_, pl, io_.wgrad_ksplit)), FA((const char*)io_.fwd_arena), A((char*)io_.bwd_arena),
        grads(io_.grads), defer_reduce(true) {
    grad_layout(g, goff, gtot);
    for (int i = 1; i < 6; ++i) defer_reduce = defer_reduce && io.side_stream[i] == io.side_stream[0];
#ifdef EGV_NO_MULTI_REDUCE
    defer_reduce = false;
#endif
  }

  // an operand the forward saved, as this backward reads it: its bf16 copy where the forward wrote fp16 planes for a bf16 backward
  void saved(int64_t hi, int64_t lo, int64_t bf, const egv_bf16*& h, const egv_bf16*& l) const {
    saved_planes(FA, pl.bwd_passes, pl.saved_bf ? bf : hi, lo, h, l);
  }

  // the weight gradient dW[N,K] = dY^T X (TN kernel, bias gradient from the same pass) of weight i, on its side stream if it has one
  // (row0 / rows: the tail's space qkv gradient covers the k / v rows D .. 3 D of dW only)
  int wgrad(int i, const egv_bf16* dy_hi, const egv_bf16* dy_lo, const egv_bf16* x_hi, const egv_bf16* x_lo, int64_t row0 = 0, int64_t rows = 0) const {
    const int64_t N = rows ? rows : o.nk[i][0], K = o.nk[i][1];
    hipStream_t main_s = (hipStream_t)stream, s = main_s;
    if (io.side_stream[i]) {
      s = (hipStream_t)io.side_stream[i];
      if (hipEventRecord((hipEvent_t)io.side_event[i], main_s) != hipSuccess) return EGV_ERR_LAUNCH;
      if (hipStreamWaitEvent(s, (hipEvent_t)io.side_event[i], 0) != hipSuccess) return EGV_ERR_LAUNCH;
    }
    egv_gemm_desc d = tn_desc(dy_hi, dy_lo, N, x_hi, x_lo, K, N, K, M, pl.bwd_passes, grads + goff[i] + row0 * K, grads + goff[6 + i] + row0,
                              io.wgrad_ksplit[i], at<float>(A, L.partial[i]), g.grid_cap);
    d.alpha = pl.walpha[i];
    if (defer_reduce && d.ksplit > 1) d.accumulate = 2;        // slabs only; reduced at the end of the call
    return egv_gemm_nt(&d, s);
  }

  // the data gradient dX[M,K] = dY . W of weight i (col0 / cols: the tail's contracts over the k / v columns D .. 3 D of W^T only)
  egv_gemm_desc dgrad(int i, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t col0 = 0, int64_t cols = 0) const {
    const int64_t N = cols ? cols : o.nk[i][0];
    return nt_desc(dy_hi, dy_lo, N, p.wt_hi[i] + col0, p.wt_lo[i] ? p.wt_lo[i] + col0 : nullptr, p.ldwt[i], M, o.nk[i][1], N, pl.bwd_passes, g.grid_cap);
  }
  // ... into planes [M, cols] (dZ, dO): split-bf16, or one plane of un-clamped fp16
  int to_planes(egv_gemm_desc& d, egv_bf16* hi, egv_bf16* lo) const {
    d.out_hi = hi; d.out_lo = lo; d.ldoh = d.N; d.out_fmt = pl.grad_fmt;
    return egv_gemm_nt(&d, stream);
  }
  // ... into the input of a LayerNorm backward (d_n2, d_n1, d_n3): fp32; in the fp16 backward ONE plane of un-clamped fp16 in the same
  // buffer (half the bytes written here and read there: 77 -> 38.6 MB per launch at M = 25 120)
  int to_ln(egv_gemm_desc d, float* buf) const {
    if (pl.grad_fmt == EGV_OUT_F16_GRAD) return to_planes(d, (egv_bf16*)buf, nullptr);
    d.out_f32 = buf; d.ldo = D;
    return egv_gemm_nt(&d, stream);
  }
  // dx = add1 + add2 + LN'(d_n) of the LayerNorm whose forward read `x`: fp32 and planes; the affine gradients' partial sums into ln_work[w]
  int ln_bwd(const float* d_n, const float* x, int64_t ldx, const float* gw, int64_t mean, int64_t rstd, int32_t rows, const float* add1,
             const float* add2, float* dx, egv_bf16* dx_hi, egv_bf16* dx_lo, int fmt, int gi, int w) const {
    const bool plane = (fmt & EGV_LN_DY_F16) != 0;
    return egv_layernorm_bwd_partial(plane ? nullptr : d_n, plane ? (const egv_bf16*)d_n : nullptr, nullptr, D, x, ldx, gw, at<float>(FA, mean),
                                     at<float>(FA, rstd), rows, D, add1, add2, dx, D, dx_hi, dx_lo, fmt, grads + goff[gi], grads + goff[gi + 1],
                                     at<float>(A, L.ln_work[w]), stream);
  }

  // backward of one attention branch behind its output gradient planes r.dres_*: proj wgrad, proj dgrad -> dO, attention backward,
  // qkv wgrad, qkv dgrad -> r.d_n
  int attn_branch_bwd(const FwdBranch& f, const BwdBranch& r, int time) const {
    const int wi = time ? LIN_TQKV : LIN_SQKV;
    const egv_bf16 *n_hi, *n_lo, *a_hi, *a_lo, *q_hi, *q_lo;
    saved(f.n_hi, f.n_lo, f.n_bf, n_hi, n_lo);
    saved(f.a_hi, f.a_lo, f.a_hi, a_hi, a_lo);
    saved(f.qkv_hi, f.qkv_lo, f.qkv_hi, q_hi, q_lo);
    egv_bf16 *dres_hi = at<egv_bf16>(A, r.dres_hi), *dres_lo = at<egv_bf16>(A, r.dres_lo), *do_hi = at<egv_bf16>(A, r.do_hi), *do_lo = at<egv_bf16>(A, r.do_lo);
    egv_bf16 *dq_hi = at<egv_bf16>(A, r.dqkv_hi), *dq_lo = at<egv_bf16>(A, r.dqkv_lo);
    EGV_TRY(wgrad(wi + 1, dres_hi, dres_lo, a_hi, a_lo));
    egv_gemm_desc d = dgrad(wi + 1, dres_hi, dres_lo);
    EGV_TRY(to_planes(d, do_hi, do_lo));
    // the attention backward takes the forward output's second plane whenever it is a bf16 lo plane, also in a single-pass backward
    // (delta = rowsum(dO o O) exact in O: egv_divided_attn_bwd)
    EGV_TRY(egv_divided_attn_bwd(q_hi, q_lo, a_hi, pl.attn_bwd_o_lo ? at<egv_bf16>(FA, f.a_lo) : nullptr, do_hi, do_lo, at<float>(FA, f.lse), g.B, g.T,
                                 g.n, g.H, block_attn_mode(pl.attn_mode_bwd, time), pl.attn_bwd_passes, dq_hi, dq_lo, at<float>(A, L.attn_work), stream));
    EGV_TRY(wgrad(wi, dq_hi, dq_lo, n_hi, n_lo));
    return to_ln(dgrad(wi, dq_hi, dq_lo), at<float>(A, r.d_n));
  }

  int backward() const {
    if (pl.tail && io.g_hi) return EGV_ERR_ARG;         // the tail's g_out is [B, D] fp32: there are no planes of it
    for (int i = 0; i < (pl.tail ? 3 : 6); ++i)
      if (!p.wt_hi[i] || (pl.bwd_lo && !p.wt_lo[i])) return EGV_ERR_ARG;
    if (pl.bwd_lo && (!io.dx_lo || (io.g_hi && !io.g_lo))) return EGV_ERR_ARG;
    const float *tr = at<float>(FA, F.tr), *sr = at<float>(FA, F.sr);
    float* d_sr = at<float>(A, L.s.d_res);    // null in tail mode (the CLS rows' d_sr is added to d_tr below)
    float* d_n1 = at<float>(A, L.s.d_n);
    if (pl.tail) {
      // ---- CLS tail: g_out is [B, D]; every other row of the block output has no gradient, so the MLP, norm2, the space proj and the
      // space attention's query side run on B rows in fp32 from the master weights (csrc/cls_tail.hip), and the attention backward
      // writes dK / dV of every key from the one CLS query
      const float *w_q = (const float*)p.w_hi[2], *w_proj = (const float*)p.w_hi[3], *w_fc1 = (const float*)p.w_hi[4],
                  *w_fc2 = (const float*)p.w_hi[5];
      if (!w_q || !w_proj || !w_fc1 || !w_fc2) return EGV_ERR_ARG;
      const int32_t B = g.B;
      const float* G = io.g_out;
      const float *n1c = at<float>(FA, F.n1c), *qc = at<float>(FA, F.qc), *oc = at<float>(FA, F.oc), *n2c = at<float>(FA, F.n2c),
                  *hc = at<float>(FA, F.hc);
      float *dzc = at<float>(A, L.dzc), *dn2c = at<float>(A, L.dn2c), *dsrc = at<float>(A, L.dsrc), *doc = at<float>(A, L.doc),
            *dqc = at<float>(A, L.dqc), *lw = at<float>(A, L.lin_work);
      EGV_TRY(egv_cls_linear_dgrad(G, D, w_fc2, Hd, B, D, Hd, at<float>(FA, F.z), dzc, Hd, EGV_CLS_DX_STORE, lw, stream));
      EGV_TRY(egv_cls_linear_wgrad(G, D, hc, Hd, B, D, Hd, grads + goff[5], Hd, grads + goff[11], stream));
      EGV_TRY(egv_cls_linear_dgrad(dzc, Hd, w_fc1, D, B, Hd, D, nullptr, dn2c, D, EGV_CLS_DX_STORE, lw, stream));
      EGV_TRY(egv_cls_linear_wgrad(dzc, Hd, n2c, D, B, Hd, D, grads + goff[4], D, grads + goff[10], stream));
      EGV_TRY(ln_bwd(dn2c, sr, D, p.n2w, F.mean2, F.rstd2, B, G, nullptr, dsrc, nullptr, nullptr, 0, 16, 0));
      EGV_TRY(egv_cls_linear_wgrad(dsrc, D, oc, D, B, D, D, grads + goff[3], D, grads + goff[9], stream));
      EGV_TRY(egv_cls_linear_dgrad(dsrc, D, w_proj, D, B, D, D, nullptr, doc, D, EGV_CLS_DX_STORE, lw, stream));
      uint16_t *dkv_hi = at<uint16_t>(A, L.s.dqkv_hi), *dkv_lo = at<uint16_t>(A, L.s.dqkv_lo);
      const uint16_t *kv_hi = at<uint16_t>(FA, F.s.qkv_hi), *kv_lo = at<uint16_t>(FA, F.s.qkv_lo);
      EGV_TRY(egv_cls_attn_bwd(qc, D, kv_hi, kv_lo, kv_hi + D, kv_lo ? kv_lo + D : nullptr, 2 * D, pl.kv_fmt, oc, doc, at<float>(FA, F.s.lse), B,
                               (int32_t)o.S, g.H, dqc, dkv_hi, dkv_lo, dkv_hi + D, dkv_lo ? dkv_lo + D : nullptr, 2 * D, pl.kv_fmt, stream));
      // the space qkv weight: its q rows from the B CLS rows, its k / v rows from every token (the TN kernel, on the wgrad stream)
      EGV_TRY(egv_cls_linear_wgrad(dqc, D, n1c, D, B, D, D, grads + goff[2], D, grads + goff[8], stream));
      const egv_bf16 *n1_hi, *n1_lo;
      saved(F.s.n_hi, F.s.n_lo, F.s.n_bf, n1_hi, n1_lo);
      EGV_TRY(wgrad(LIN_SQKV, (const egv_bf16*)dkv_hi, (const egv_bf16*)dkv_lo, n1_hi, n1_lo, D, 2 * D));
      EGV_TRY(to_ln(dgrad(LIN_SQKV, (const egv_bf16*)dkv_hi, (const egv_bf16*)dkv_lo, D, 2 * D), d_n1));
      EGV_TRY(egv_cls_linear_dgrad(dqc, D, w_q, D, B, D, D, nullptr, d_n1, o.S * o.D, pl.cls_dx_mode, lw, stream));
    } else {
      // ---- G as planes (handed over by the next block's LayerNorm-backward, or formatted here)
      const egv_bf16 *g_hi = io.g_hi, *g_lo = pl.bwd_lo ? io.g_lo : nullptr;
      if (!g_hi) {
        egv_bf16 *gh = at<egv_bf16>(A, L.g_hi), *gl = at<egv_bf16>(A, L.g_lo);
        if (pl.grad_fmt == EGV_OUT_F16_GRAD) EGV_TRY(egv_f16x2_encode(io.g_out, D, M, D, gh, nullptr, nullptr, D, EGV_F16X2_GRAD_CAST, stream));
        else EGV_TRY(egv_split_f32(io.g_out, D, M, D, gh, gl, D, nullptr, nullptr, 0, nullptr, stream));
        g_hi = gh; g_lo = gl;
      }
      // ---- MLP backward: dZ = (G . W2) * gelu'(z) leaves the fc2-dgrad epilogue already in its operand format
      const egv_bf16 *n2_hi, *n2_lo, *h_hi, *h_lo;
      saved(F.n2_hi, F.n2_lo, F.n2_bf, n2_hi, n2_lo);
      saved(F.h_hi, F.h_lo, F.h_bf, h_hi, h_lo);
      egv_bf16 *dz_hi = at<egv_bf16>(A, L.dz_hi), *dz_lo = at<egv_bf16>(A, L.dz_lo);
      egv_gemm_desc d = dgrad(LIN_FC2, g_hi, g_lo);
      d.act = EGV_ACT_GELU_BWD; d.aux_in = at<float>(FA, F.z); d.ldaux = Hd; d.aux_bf16 = pl.z_code;
      EGV_TRY(to_planes(d, dz_hi, dz_lo));
      EGV_TRY(wgrad(LIN_FC2, g_hi, g_lo, h_hi, h_lo));
      EGV_TRY(wgrad(LIN_FC1, dz_hi, dz_lo, n2_hi, n2_lo));
      float* d_n2 = at<float>(A, L.d_n2);
      EGV_TRY(to_ln(dgrad(LIN_FC1, dz_hi, dz_lo), d_n2));
      EGV_TRY(ln_bwd(d_n2, sr, D, p.n2w, F.mean2, F.rstd2, M, io.g_out, nullptr, d_sr, at<egv_bf16>(A, L.s.dres_hi), at<egv_bf16>(A, L.s.dres_lo),
                     pl.ln_fmt, 16, 0));
      // ---- spatial attention backward
      EGV_TRY(attn_branch_bwd(F.s, L.s, 0));
    }
    float* d_tr = at<float>(A, L.t.d_res);
    EGV_TRY(ln_bwd(d_n1, tr, D, p.n1w, F.s.mean, F.s.rstd, M, nullptr, nullptr, d_tr, at<egv_bf16>(A, L.t.dres_hi), at<egv_bf16>(A, L.t.dres_lo), pl.ln_fmt,
                   14, 1));
    // tail: d_sr exists on the CLS rows only; it joins dx through d_tr (fp32; the planes above are what the time branch reads)
    if (pl.tail) EGV_TRY(egv_cls_rows_add(d_tr, o.S * o.D, at<float>(A, L.dsrc), D, g.B, D, stream));
    // ---- temporal attention backward
    EGV_TRY(attn_branch_bwd(F.t, L.t, 1));
    // x feeds norm3, the tr residual and the sr residual: dx = d_tr + d_sr + LN3'(d_n3)
    EGV_TRY(ln_bwd(at<float>(A, L.t.d_n), io.x, D, p.n3w, F.t.mean, F.t.rstd, M, d_tr, d_sr, io.d_x, io.dx_hi, pl.bwd_lo ? io.dx_lo : nullptr, pl.ln_fmt, 12, 2));
    if (defer_reduce) {
      const float* part[6]; float* outp[6]; float* csp[6]; int64_t mn[6]; int32_t ksv[6], mv[6];
      int cnt = 0;
      for (int i = 0; i < 6; ++i) {
        if (io.wgrad_ksplit[i] <= 1 || (pl.tail && i > LIN_SQKV)) continue;
        const int64_t row0 = (pl.tail && i == LIN_SQKV) ? D : 0;          // tail: the k / v rows of the space qkv gradient
        const int64_t N = o.nk[i][0] - row0, K = o.nk[i][1];
        part[cnt] = at<float>(A, L.partial[i]); outp[cnt] = grads + goff[i] + row0 * K; csp[cnt] = grads + goff[6 + i] + row0;
        mn[cnt] = N * K; ksv[cnt] = io.wgrad_ksplit[i]; mv[cnt] = (int32_t)N;
        ++cnt;
      }
      // on the stream the weight gradients ran on (stream order: behind the last of them)
      if (cnt) EGV_TRY(egv_splitk_reduce_multi(cnt, part, outp, mn, ksv, csp, mv, io.side_stream[0] ? io.side_stream[0] : stream));
    }
    // the affine gradients of the three LayerNorms: their per-block partial sums are reduced by ONE launch (three before)
    const float* w3[3] = {at<float>(A, L.ln_work[0]), at<float>(A, L.ln_work[1]), at<float>(A, L.ln_work[2])};
    float* g3[3] = {grads + goff[16], grads + goff[14], grads + goff[12]};
    float* b3[3] = {grads + goff[17], grads + goff[15], grads + goff[13]};
    if (pl.tail) {                          // norm2 ran on the B CLS rows: its partial sums are those of a B-row launch
      EGV_TRY(egv_layernorm_bwd_reduce(1, w3, g.B, D, g3, b3, stream));
      return egv_layernorm_bwd_reduce(2, w3 + 1, M, D, g3 + 1, b3 + 1, stream);
    }
    return egv_layernorm_bwd_reduce(3, w3, M, D, g3, b3, stream);
  }
};

bool ok(const egv_block_geom* g) { return g && block_check(*g) == EGV_OK; }

}  // namespace

extern "C" int64_t egv_block_fwd_arena_bytes(const egv_block_geom* g) { return ok(g) ? fwd_layout(*g, block_plan(*g)).total : -1; }

extern "C" int64_t egv_block_bwd_arena_bytes(const egv_block_geom* g, const int32_t* wgrad_ksplit) {
  return ok(g) ? bwd_layout(*g, block_plan(*g), wgrad_ksplit).total : -1;
}

extern "C" int egv_block_grad_layout(const egv_block_geom* g, int64_t* offsets18, int64_t* total_floats) {
  if (!ok(g) || !offsets18 || !total_floats) return EGV_ERR_ARG;
  grad_layout(*g, offsets18, *total_floats);
  return EGV_OK;
}

// Byte offsets (into the forward arena) of what Python keeps handles to: the planes the attached gradient hand-over and the
// tests look at.  order: n3_hi, at_hi, n1_hi, as_hi, n2_hi, h_hi, qkvt_hi, qkvs_hi, tr, sr, z  (-1: absent)
extern "C" int egv_block_fwd_offsets(const egv_block_geom* g, int64_t* off11) {
  if (!ok(g) || !off11) return EGV_ERR_ARG;
  const FwdLayout L = fwd_layout(*g, block_plan(*g));
  const int64_t v[11] = {L.t.n_hi, L.t.a_hi, L.s.n_hi, L.s.a_hi, L.n2_hi, L.h_hi, L.t.qkv_hi, L.s.qkv_hi, L.tr, L.sr, L.z};
  std::copy(v, v + 11, off11);
  return EGV_OK;
}

extern "C" int egv_block_fwd(const egv_block_geom* g, const egv_block_params* p, const float* x, float* out, void* arena, void* stream) {
  if (!ok(g) || !p || !x || !out || !arena) return EGV_ERR_ARG;
  return Call(*g, *p, stream).forward(x, out, (char*)arena);
}

extern "C" int egv_block_bwd(const egv_block_geom* g, const egv_block_params* p, const egv_block_bwd_io* io, void* stream) {
  if (!ok(g) || !p || !io || !(g->train & EGV_TRAIN_KEEP)) return EGV_ERR_ARG;
  if (!io->g_out || !io->x || !io->fwd_arena || !io->bwd_arena || !io->d_x || !io->dx_hi || !io->grads) return EGV_ERR_ARG;
  return Bwd(*g, *p, *io, stream).backward();
}
