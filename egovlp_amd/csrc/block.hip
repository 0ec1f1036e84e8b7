// One C-ABI call per SpaceTimeBlock forward and one per backward (model/video_transformer.py:163-177 and its autograd
// transpose): the host enqueues the block's ~11 / ~25 kernels from C with pointers into ONE workspace arena per direction, instead
// of ~50 Python-level tensor allocations and ~30 ctypes calls.  Nothing new is computed here: every launch below is one of the
// library's own entry points (egv_layernorm_*, egv_gemm_nt, egv_divided_attn_*), with the arguments the per-kernel Python path
// (egovlp_amd/model/video_transformer.py::_SpaceTimeBlockFn, kept as the reference) gives them, in the same order -- results are
// bit-identical (tests/test_gpu_block.py).  The layout of the two arenas is a pure function of the geometry (egv_block_layout).
// CLS-tail mode (egv_block_geom.train bit 1, the tower's last block): only the B CLS rows of the output are wanted, so what follows the
// k / v projection of the space branch runs on B rows through the egv_cls_* entry points (csrc/cls_tail.hip; tests/test_gpu_cls_tail.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "layer_call.h"

namespace {

// forward arena: what the block's kernels hand to each other and what the backward needs again
struct FwdLayout {
  int64_t n3_hi, n3_lo, mean3, rstd3, qkvt_hi, qkvt_lo, at_hi, at_lo, lse_t, work_t;
  int64_t tr, n1_hi, n1_lo, mean1, rstd1, qkvs_hi, qkvs_lo, as_hi, as_lo, lse_s, work_s;
  int64_t sr, n2_hi, n2_lo, mean2, rstd2, h_hi, h_lo, z;
  int64_t n3_bf, n1_bf, n2_bf, h_bf;     // f16x2 forward (P == 2) of a training step: bf16 copies for the single-pass backward
  // CLS-tail mode (egv_block_geom.train bit 1): fp32 [B, .] rows -- LN1(tr) and its scratch statistics, the CLS query, the attention
  // output, LN2's output, gelu(fc1).  There qkvs_* are the k | v planes [M, 2 D], lse_s is [B, H], sr / mean2 / rstd2 / z hold B rows
  // (z: the fp32 pre-activation) and as_*, work_s, n2_*, h_*, n2_bf, h_bf are absent.
  int64_t n1c, mean1c, rstd1c, qc, oc, n2c, hc;
  int64_t total;
};

struct Geo {
  int64_t M, S, D, Hd;
  int P, Pb;
};

inline bool is_train(const egv_block_geom& g) { return (g.train & 1) != 0; }
inline bool is_tail(const egv_block_geom& g) { return (g.train & 2) != 0; }

Geo geo_of(const egv_block_geom& g) {
  Geo o;
  o.S = 1 + (int64_t)g.T * g.n;
  o.M = (int64_t)g.B * o.S;
  o.D = g.D;
  o.Hd = g.Hd;
  o.P = g.fwd_passes;
  o.Pb = g.bwd_passes;
  return o;
}

bool geom_ok(const egv_block_geom& g) {
  if (g.B <= 0 || g.T <= 0 || g.n <= 0 || g.H <= 0 || g.D != g.H * 64 || g.Hd <= 0 || g.D % 32 || g.Hd % 32) return false;
  // bwd_passes: 3 = split-bf16 three-product, 1 = one bf16 product, 4 = one FP16 product on scaled gradients (the fp16 backward: needs
  // the f16x2 / f16mix forward, whose saved operands ARE fp16 planes -- no bf16 copies are written then)
  if (g.fwd_passes < 1 || g.fwd_passes > 3 || (g.bwd_passes != 1 && g.bwd_passes != 3 && g.bwd_passes != 4)) return false;
  if (g.bwd_passes == 3 && g.fwd_passes != 3) return false;
  if (g.bwd_passes == 4 && g.fwd_passes != 2) return false;
  if (g.train < 0 || g.train > 3) return false;
  if (g.fwd_passes == 2 && (g.bwd_passes == 3 || (is_train(g) && !g.z_bf16))) return false;   // f16x2 forward: single-product backward, 16-bit saved gelu'
  if (g.f16_single < 0 || g.f16_single > 15 || (g.f16_single && g.fwd_passes != 2)) return false;
  return true;
}

FwdLayout fwd_layout(const egv_block_geom& g) {
  const Geo o = geo_of(g);
  const bool lo = o.P != 1;              // split-bf16 (P == 3) and f16x2 (P == 2) operands are two planes
  const bool h16 = o.Pb == 4;            // fp16 backward: it reads the forward's own fp16 planes
  const bool bf = o.P == 2 && is_train(g) && !h16;
  const bool tail = is_tail(g);
  FwdLayout L;
  Bump b;
  auto plane = [&](int64_t cols) { return b.take(o.M * cols * 2); };
  auto plane_lo = [&](int64_t cols) { return lo ? b.take(o.M * cols * 2) : (int64_t)-1; };
  auto plane_bf = [&](int64_t cols) { return bf ? b.take(o.M * cols * 2) : (int64_t)-1; };
  // f16x2 forward with single-product Linears (g.f16_single): their first operand is ONE plain fp16 plane
  const bool q1 = (g.f16_single & 4) != 0;
  L.n3_hi = plane(o.D); L.n3_lo = q1 ? (int64_t)-1 : plane_lo(o.D);
  L.mean3 = b.take(o.M * 4); L.rstd3 = b.take(o.M * 4);
  L.qkvt_hi = plane(3 * o.D); L.qkvt_lo = plane_lo(3 * o.D);
  const bool a1p = h16 && (g.f16_single & 8);   // attention output as ONE fp16 plane (one-product proj, fp16 backward)
  L.at_hi = plane(o.D); L.at_lo = a1p ? (int64_t)-1 : plane_lo(o.D);
  L.lse_t = b.take((int64_t)g.B * g.H * o.S * 4);
  L.work_t = b.take(egv_divided_attn_fwd_work_floats(g.B, g.T, g.n, g.H, 1) * 4);
  L.tr = b.take(o.M * o.D * 4);
  L.n1_hi = plane(o.D); L.n1_lo = q1 ? (int64_t)-1 : plane_lo(o.D);
  L.mean1 = b.take(o.M * 4); L.rstd1 = b.take(o.M * 4);
  L.n1c = L.mean1c = L.rstd1c = L.qc = L.oc = L.n2c = L.hc = -1;
  if (tail) {
    const int64_t B = g.B;
    L.qkvs_hi = plane(2 * o.D); L.qkvs_lo = plane_lo(2 * o.D);
    L.as_hi = L.as_lo = L.work_s = L.n2_hi = L.n2_lo = L.h_hi = L.h_lo = L.n2_bf = L.h_bf = -1;
    L.lse_s = b.take(B * g.H * 4);
    L.n1c = b.take(B * o.D * 4); L.mean1c = b.take(B * 4); L.rstd1c = b.take(B * 4);
    L.qc = b.take(B * o.D * 4); L.oc = b.take(B * o.D * 4);
    L.sr = b.take(B * o.D * 4);
    L.n2c = b.take(B * o.D * 4); L.mean2 = b.take(B * 4); L.rstd2 = b.take(B * 4);
    L.hc = b.take(B * o.Hd * 4);
    L.z = is_train(g) ? b.take(B * o.Hd * 4) : (int64_t)-1;
    L.n3_bf = plane_bf(o.D); L.n1_bf = plane_bf(o.D);
    L.total = b.off;
    return L;
  }
  L.qkvs_hi = plane(3 * o.D); L.qkvs_lo = plane_lo(3 * o.D);
  L.as_hi = plane(o.D); L.as_lo = a1p ? (int64_t)-1 : plane_lo(o.D);
  L.lse_s = b.take((int64_t)g.B * g.H * o.S * 4);
  L.work_s = b.take(egv_divided_attn_fwd_work_floats(g.B, g.T, g.n, g.H, 0) * 4);
  L.sr = b.take(o.M * o.D * 4);
  L.n2_hi = plane(o.D); L.n2_lo = (g.f16_single & 1) ? (int64_t)-1 : plane_lo(o.D);
  L.mean2 = b.take(o.M * 4); L.rstd2 = b.take(o.M * 4);
  L.h_hi = plane(o.Hd); L.h_lo = (g.f16_single & 2) ? (int64_t)-1 : plane_lo(o.Hd);
  L.z = is_train(g) ? b.take(o.M * o.Hd * (g.z_bf16 ? 2 : 4)) : (int64_t)-1;
  L.n3_bf = plane_bf(o.D); L.n1_bf = plane_bf(o.D); L.n2_bf = plane_bf(o.D); L.h_bf = plane_bf(o.Hd);
  L.total = b.off;
  return L;
}

// weights of a block, in the order of egv_block_params: tqkv, tproj, sqkv, sproj, fc1, fc2  ->  (N, K) of W[N,K]
void wshape(const Geo& o, int i, int64_t& N, int64_t& K) {
  switch (i) {
    case 0: case 2: N = 3 * o.D; K = o.D; break;
    case 1: case 3: N = o.D; K = o.D; break;
    case 4: N = o.Hd; K = o.D; break;
    default: N = o.D; K = o.Hd; break;
  }
}

// gradient buffer: [dW x 6][db x 6][dgamma3, dbeta3, dgamma1, dbeta1, dgamma2, dbeta2] back to back, offsets in floats
void grad_layout(const egv_block_geom& g, int64_t off[18], int64_t& total) {
  const Geo o = geo_of(g);
  int64_t p = 0;
  auto take = [&](int64_t n) { const int64_t q = p; p += n; return q; };   // back to back: every size is a multiple of 4 floats (D % 32 == 0)
  for (int i = 0; i < 6; ++i) { int64_t N, K; wshape(o, i, N, K); off[i] = take(N * K); }
  for (int i = 0; i < 6; ++i) { int64_t N, K; wshape(o, i, N, K); off[6 + i] = take(N); }
  for (int i = 0; i < 6; ++i) off[12 + i] = take(o.D);
  total = p;
}

struct BwdLayout {
  int64_t g_hi, g_lo, dz_hi, dz_lo, d_n2, d_sr, dsr_hi, dsr_lo, das_hi, das_lo, dqkvs_hi, dqkvs_lo, d_n1, d_tr, dtr_hi, dtr_lo, dat_hi,
      dat_lo, dqkvt_hi, dqkvt_lo, d_n3, ln_work[3], attn_work, partial[6];
  // CLS-tail mode: fp32 [B, .] rows (dZ, d_n2, d_sr, dO, dq of the CLS rows), the two-stage dgrad's slabs; dqkvs_* are the dk | dv
  // planes [M, 2 D] there and g_*, dz_*, dsr_*, das_* are absent
  int64_t dzc, dn2c, dsrc, doc, dqc, lin_work;
  int64_t total;
};

BwdLayout bwd_layout(const egv_block_geom& g, const int32_t* ksplit) {
  const Geo o = geo_of(g);
  const bool lo = o.Pb == 3;
  BwdLayout L;
  Bump b;
  auto plane = [&](int64_t cols) { return b.take(o.M * cols * 2); };
  auto plane_lo = [&](int64_t cols) { return lo ? b.take(o.M * cols * 2) : (int64_t)-1; };
  const bool tail = is_tail(g);
  L.dzc = L.dn2c = L.dsrc = L.doc = L.dqc = L.lin_work = -1;
  if (tail) {
    const int64_t B = g.B;
    L.g_hi = L.g_lo = L.dz_hi = L.dz_lo = L.d_n2 = L.d_sr = L.dsr_hi = L.dsr_lo = L.das_hi = L.das_lo = -1;
    L.dzc = b.take(B * o.Hd * 4); L.dn2c = b.take(B * o.D * 4); L.dsrc = b.take(B * o.D * 4); L.doc = b.take(B * o.D * 4);
    L.dqc = b.take(B * o.D * 4);
    L.lin_work = b.take(egv_cls_linear_work_floats(g.B, (int32_t)std::max(o.D, o.Hd), (int32_t)std::max(o.D, o.Hd)) * 4);
    L.dqkvs_hi = plane(2 * o.D); L.dqkvs_lo = plane_lo(2 * o.D);
  } else {
    L.g_hi = plane(o.D); L.g_lo = plane_lo(o.D);
    L.dz_hi = plane(o.Hd); L.dz_lo = plane_lo(o.Hd);
    L.d_n2 = b.take(o.M * o.D * 4);
    L.d_sr = b.take(o.M * o.D * 4);
    L.dsr_hi = plane(o.D); L.dsr_lo = plane_lo(o.D);
    L.das_hi = plane(o.D); L.das_lo = plane_lo(o.D);
    L.dqkvs_hi = plane(3 * o.D); L.dqkvs_lo = plane_lo(3 * o.D);
  }
  L.d_n1 = b.take(o.M * o.D * 4);
  L.d_tr = b.take(o.M * o.D * 4);
  L.dtr_hi = plane(o.D); L.dtr_lo = plane_lo(o.D);
  L.dat_hi = plane(o.D); L.dat_lo = plane_lo(o.D);
  L.dqkvt_hi = plane(3 * o.D); L.dqkvt_lo = plane_lo(3 * o.D);
  L.d_n3 = b.take(o.M * o.D * 4);
  for (int i = 0; i < 3; ++i) L.ln_work[i] = b.take(2 * o.D * (int64_t)egv_layernorm_bwd_parts((int32_t)o.M) * 4);   // one per LayerNorm: reduced together at the end
  L.attn_work = b.take(egv_divided_attn_bwd_work_floats(g.B, g.T, g.n, g.H) * 4);
  for (int i = 0; i < 6; ++i) {
    int64_t N, K;
    wshape(o, i, N, K);
    const int ks = (ksplit && !(tail && i > 2)) ? ksplit[i] : 1;      // tail: the space proj / fc1 / fc2 gradients are rank-B updates
    if (tail && i == 2) N = 2 * o.D;                                    // and the space qkv GEMM covers the k / v rows
    L.partial[i] = ks > 1 ? b.take((int64_t)ks * (N * K + N) * 4) : (int64_t)-1;
  }
  L.total = b.off;
  return L;
}

}  // namespace

extern "C" int64_t egv_block_fwd_arena_bytes(const egv_block_geom* g) { return (g && geom_ok(*g)) ? fwd_layout(*g).total : -1; }

extern "C" int64_t egv_block_bwd_arena_bytes(const egv_block_geom* g, const int32_t* wgrad_ksplit) {
  return (g && geom_ok(*g)) ? bwd_layout(*g, wgrad_ksplit).total : -1;
}

extern "C" int egv_block_grad_layout(const egv_block_geom* g, int64_t* offsets18, int64_t* total_floats) {
  if (!g || !geom_ok(*g) || !offsets18 || !total_floats) return EGV_ERR_ARG;
  grad_layout(*g, offsets18, *total_floats);
  return EGV_OK;
}

// Byte offsets (into the forward arena) of what Python keeps handles to: the planes the attached gradient hand-over and the
// tests look at.  order: n3_hi, at_hi, n1_hi, as_hi, n2_hi, h_hi, qkvt_hi, qkvs_hi, tr, sr, z  (-1: absent)
extern "C" int egv_block_fwd_offsets(const egv_block_geom* g, int64_t* off11) {
  if (!g || !geom_ok(*g) || !off11) return EGV_ERR_ARG;
  const FwdLayout L = fwd_layout(*g);
  const int64_t v[11] = {L.n3_hi, L.at_hi, L.n1_hi, L.as_hi, L.n2_hi, L.h_hi, L.qkvt_hi, L.qkvs_hi, L.tr, L.sr, L.z};
  for (int i = 0; i < 11; ++i) off11[i] = v[i];
  return EGV_OK;
}

extern "C" int egv_block_fwd(const egv_block_geom* gp, const egv_block_params* pp, const float* x, float* out, void* arena, void* stream) {
  if (!gp || !pp || !x || !out || !arena || !geom_ok(*gp)) return EGV_ERR_ARG;
  const egv_block_geom& g = *gp;
  const egv_block_params& p = *pp;
  const Geo o = geo_of(g);
  const FwdLayout L = fwd_layout(g);
  const int P = o.P;
  const int Pa = P == 2 ? 3 : P;         // attention and the proj Linears: split-bf16 three-product operands in the f16x2 mode
  const int32_t M = (int32_t)o.M, D = (int32_t)o.D, Hd = (int32_t)o.Hd;
  for (int i = 0; i < (is_tail(g) ? 3 : 6); ++i)
    if (!p.w_hi[i] || (P != 1 && !p.w_lo[i])) return EGV_ERR_ARG;
  const int P_fc1 = (g.f16_single & 1) ? 4 : P, P_fc2 = (g.f16_single & 2) ? 4 : P, P_qkv = (g.f16_single & 4) ? 4 : P;   // 4: ONE fp16 product
  const bool proj1 = (g.f16_single & 8) != 0;      // proj Linears: ONE fp16 product on the attention's fp16(value) plane (its second output plane)
  const bool h16 = o.Pb == 4;                      // fp16 backward: no bf16 copies; the attention output is fp16 planes only (format 3: ONE
                                                   // plane of fp16(value), one-product proj; format 2: f16x2 planes, TWO-product proj)
  const int afmt = h16 ? (proj1 ? 3 : 2) : (proj1 ? 1 : 0);
  const int amode = (afmt << 1) | (h16 ? 8 : 0);     // fp16 backward: the attention itself runs on fp16 operands (qkv planes = an fp16 split)
  // the proj GEMM of one attention branch: operand planes and product count by format
  auto proj_desc = [&](const egv_bf16* a_hi, const egv_bf16* a_lo, int wi) {
    if (afmt == 3) return nt_desc(a_hi, nullptr, D, p.w_hi[wi], p.w_lo[wi], p.ldw[wi], M, D, D, 4, g.grid_cap);
    if (afmt == 2) return nt_desc(a_hi, a_lo, D, p.w_hi[wi], p.w_lo[wi], p.ldw[wi], M, D, D, 2, g.grid_cap);
    if (afmt == 1) return nt_desc(a_lo, nullptr, D, p.w_hi[wi], p.w_lo[wi], p.ldw[wi], M, D, D, 4, g.grid_cap);
    return nt_desc(a_hi, a_lo, D, p.w_hi[wi], p.w_lo[wi], p.ldw[wi], M, D, D, Pa, g.grid_cap);
  };
  char* A = (char*)arena;
  // LayerNorm -> operand planes of the qkv / fc1 Linears: split-bf16, or f16x2 (first-operand role, + the bf16 copy the backward reads)
  auto ln = [&](const float* in, const float* gw, const float* gb, egv_bf16* y_hi, egv_bf16* y_lo, int64_t bf_off, float* mean, float* rstd) -> int {
    if (P == 2)
      return egv_layernorm_fwd_f16x2(in, D, gw, gb, g.eps, M, D, (uint16_t*)y_hi, (uint16_t*)y_lo, at<egv_bf16>(A, bf_off), D, mean, rstd, stream);
    return egv_layernorm_fwd(in, nullptr, D, gw, gb, g.eps, M, D, nullptr, y_hi, y_lo, nullptr, D, mean, rstd, stream);
  };
  egv_bf16 *n3_hi = at<egv_bf16>(A, L.n3_hi), *n3_lo = at<egv_bf16>(A, L.n3_lo);
  egv_bf16 *qt_hi = at<egv_bf16>(A, L.qkvt_hi), *qt_lo = at<egv_bf16>(A, L.qkvt_lo);
  egv_bf16 *at_hi = at<egv_bf16>(A, L.at_hi), *at_lo = at<egv_bf16>(A, L.at_lo);
  egv_bf16 *n1_hi = at<egv_bf16>(A, L.n1_hi), *n1_lo = at<egv_bf16>(A, L.n1_lo);
  egv_bf16 *qs_hi = at<egv_bf16>(A, L.qkvs_hi), *qs_lo = at<egv_bf16>(A, L.qkvs_lo);
  egv_bf16 *as_hi = at<egv_bf16>(A, L.as_hi), *as_lo = at<egv_bf16>(A, L.as_lo);
  egv_bf16 *n2_hi = at<egv_bf16>(A, L.n2_hi), *n2_lo = at<egv_bf16>(A, L.n2_lo);
  egv_bf16 *h_hi = at<egv_bf16>(A, L.h_hi), *h_lo = at<egv_bf16>(A, L.h_lo);
  float *tr = at<float>(A, L.tr), *sr = at<float>(A, L.sr);

  // ---- temporal attention branch (:166-167)
  EGV_TRY(ln(x, p.n3w, p.n3b, n3_hi, n3_lo, L.n3_bf, at<float>(A, L.mean3), at<float>(A, L.rstd3)));
  {
    egv_gemm_desc d = nt_desc(n3_hi, n3_lo, D, p.w_hi[0], p.w_lo[0], p.ldw[0], M, 3 * D, D, P_qkv, g.grid_cap);
    d.bias = p.bias[0]; d.out_hi = qt_hi; d.out_lo = qt_lo; d.ldoh = 3 * D;
    if (h16) d.out_fmt = 3;              // qkv as an fp16 split (fp16(x), fp16(x - hi)): the fp16 attention's operand planes
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  EGV_TRY(egv_divided_attn_fwd(qt_hi, qt_lo, g.B, g.T, g.n, g.H, 1 | amode, Pa, at_hi, at_lo, at<float>(A, L.lse_t), at<float>(A, L.work_t), stream));
  {
    egv_gemm_desc d = proj_desc(at_hi, at_lo, 1);
    d.bias = p.bias[1]; d.residual = x; d.ldr = D; d.out_f32 = tr; d.ldo = D;
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  // ---- spatial attention branch (:168-171; the residual is the block INPUT x, :171)
  EGV_TRY(ln(tr, p.n1w, p.n1b, n1_hi, n1_lo, L.n1_bf, at<float>(A, L.mean1), at<float>(A, L.rstd1)));
  if (is_tail(g)) {
    // ---- CLS tail: only the B CLS rows of `out` are wanted (out is [B, D]).  k / v of every token (rows D .. 3 D of the qkv weight) on
    // the GEMM above's kernel; everything behind them on B rows, in fp32 from the master weights (csrc/cls_tail.hip)
    const float *w_q = (const float*)p.wt_hi[2], *w_proj = (const float*)p.wt_hi[3], *w_fc1 = (const float*)p.wt_hi[4],
                *w_fc2 = (const float*)p.wt_hi[5];
    if (!w_q || !w_proj || !w_fc1 || !w_fc2) return EGV_ERR_ARG;
    const int32_t B = g.B;
    const int64_t ldc = o.S * o.D;       // from one clip's CLS row to the next
    {
      const int64_t skip = (int64_t)D * p.ldw[2];          // the q rows of W[3 D, D]
      egv_gemm_desc d = nt_desc(n1_hi, n1_lo, D, p.w_hi[2] + skip, p.w_lo[2] ? p.w_lo[2] + skip : nullptr, p.ldw[2], M, 2 * D, D, P_qkv, g.grid_cap);
      d.bias = p.bias[2] + D; d.out_hi = qs_hi; d.out_lo = qs_lo; d.ldoh = 2 * D;
      if (h16) d.out_fmt = 3;
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
    float *n1c = at<float>(A, L.n1c), *qc = at<float>(A, L.qc), *oc = at<float>(A, L.oc), *n2c = at<float>(A, L.n2c), *hc = at<float>(A, L.hc);
    EGV_TRY(egv_layernorm_fwd(tr, nullptr, ldc, p.n1w, p.n1b, g.eps, B, D, nullptr, nullptr, nullptr, n1c, D, at<float>(A, L.mean1c),
                              at<float>(A, L.rstd1c), stream));
    EGV_TRY(egv_cls_linear_fwd(n1c, D, w_q, D, p.bias[2], B, D, D, EGV_ACT_NONE, nullptr, nullptr, 0, qc, D, stream));
    const uint16_t* kv_lo = P == 1 ? nullptr : (const uint16_t*)qs_lo;
    EGV_TRY(egv_cls_attn_fwd(qc, D, (const uint16_t*)qs_hi, kv_lo, (const uint16_t*)qs_hi + D, kv_lo ? kv_lo + D : nullptr, 2 * D, h16 ? 1 : 0, B,
                             (int32_t)o.S, g.H, oc, D, at<float>(A, L.lse_s), stream));
    EGV_TRY(egv_cls_linear_fwd(oc, D, w_proj, D, p.bias[3], B, D, D, EGV_ACT_NONE, nullptr, x, ldc, sr, D, stream));
    EGV_TRY(egv_layernorm_fwd(sr, nullptr, D, p.n2w, p.n2b, g.eps, B, D, nullptr, nullptr, nullptr, n2c, D, at<float>(A, L.mean2),
                              at<float>(A, L.rstd2), stream));
    EGV_TRY(egv_cls_linear_fwd(n2c, D, w_fc1, D, p.bias[4], B, Hd, D, EGV_ACT_GELU, at<float>(A, L.z), nullptr, 0, hc, Hd, stream));
    EGV_TRY(egv_cls_linear_fwd(hc, Hd, w_fc2, Hd, p.bias[5], B, D, Hd, EGV_ACT_NONE, nullptr, sr, D, out, D, stream));
    return EGV_OK;
  }
  {
    egv_gemm_desc d = nt_desc(n1_hi, n1_lo, D, p.w_hi[2], p.w_lo[2], p.ldw[2], M, 3 * D, D, P_qkv, g.grid_cap);
    d.bias = p.bias[2]; d.out_hi = qs_hi; d.out_lo = qs_lo; d.ldoh = 3 * D;
    if (h16) d.out_fmt = 3;
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  EGV_TRY(egv_divided_attn_fwd(qs_hi, qs_lo, g.B, g.T, g.n, g.H, 0 | amode, Pa, as_hi, as_lo, at<float>(A, L.lse_s), at<float>(A, L.work_s), stream));
  {
    egv_gemm_desc d = proj_desc(as_hi, as_lo, 3);
    d.bias = p.bias[3]; d.residual = x; d.ldr = D; d.out_f32 = sr; d.ldo = D;
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  // ---- MLP (:175, :46-52): exact-erf GELU in the fc1 epilogue
  EGV_TRY(ln(sr, p.n2w, p.n2b, n2_hi, n2_lo, L.n2_bf, at<float>(A, L.mean2), at<float>(A, L.rstd2)));
  {
    egv_gemm_desc d = nt_desc(n2_hi, n2_lo, D, p.w_hi[4], p.w_lo[4], p.ldw[4], M, Hd, D, P_fc1, g.grid_cap);
    d.bias = p.bias[4]; d.act = EGV_ACT_GELU; d.out_hi = h_hi; d.out_lo = h_lo; d.ldoh = Hd;
    // h as fp16 operand planes (+ bf16 copy when training): the f16x2 format, or one plain plane when fc2 runs a single product
    if (P == 2) { d.out_fmt = P_fc2 == 4 ? 2 : 1; d.out_bf = at<egv_bf16>(A, L.h_bf); }
    if (is_train(g)) {
      d.aux_out = at<float>(A, L.z); d.ldaux = Hd;
      d.aux_bf16 = g.z_bf16 ? (h16 ? 3 : 2) : 0;      // 16 bits: gelu'(z) itself (bf16; fp16 for the fp16 backward), else the fp32 pre-activation
    }
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  {
    egv_gemm_desc d = nt_desc(h_hi, h_lo, Hd, p.w_hi[5], p.w_lo[5], p.ldw[5], M, D, Hd, P_fc2, g.grid_cap);
    d.bias = p.bias[5]; d.residual = sr; d.ldr = D; d.out_f32 = out; d.ldo = D;
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  return EGV_OK;
}

extern "C" int egv_block_bwd(const egv_block_geom* gp, const egv_block_params* pp, const egv_block_bwd_io* iop, void* stream) {
  if (!gp || !pp || !iop || !geom_ok(*gp) || !(gp->train & 1)) return EGV_ERR_ARG;
  const egv_block_geom& g = *gp;
  const egv_block_params& p = *pp;
  const egv_block_bwd_io& io = *iop;
  if (!io.g_out || !io.x || !io.fwd_arena || !io.bwd_arena || !io.d_x || !io.dx_hi || !io.grads) return EGV_ERR_ARG;
  const bool tail = is_tail(g);
  if (tail && io.g_hi) return EGV_ERR_ARG;         // the tail's g_out is [B, D] fp32: there are no planes of it
  const Geo o = geo_of(g);
  const int Pb = o.Pb;
  const FwdLayout F = fwd_layout(g);
  const BwdLayout L = bwd_layout(g, io.wgrad_ksplit);
  int64_t goff[18], gtot;
  grad_layout(g, goff, gtot);
  const int32_t M = (int32_t)o.M, D = (int32_t)o.D, Hd = (int32_t)o.Hd;
  for (int i = 0; i < (tail ? 3 : 6); ++i)
    if (!p.wt_hi[i] || (Pb == 3 && !p.wt_lo[i])) return EGV_ERR_ARG;
  if (Pb == 3 && (!io.dx_lo || (io.g_hi && !io.g_lo))) return EGV_ERR_ARG;
  // The fp16 backward (Pb == 4).  Every gradient of the pass carries the loss scale S (egv_loss_scale_*; linear all the way, so nothing
  // here knows S).  Operand planes: dY = ONE plane of un-clamped fp16 (LayerNorm-backward, the GELU' epilogue, the attention backward
  // write it so; g_hi / dx_hi of the io struct are such planes too); X = plane 1 of the forward's own fp16 operand (plain fp16(x), or
  // a1 = fp16((1 - e) x) of an f16x2 encoding: the weight gradient is rescaled by 1 / (1 - e)); W^T = fp16 planes in p.wt_hi.  The
  // attention backward multiplies fp16 as well: q / k / v = the hi plane of the fp16-split qkv planes the forward wrote, dO = an fp16 plane
  // from the proj dgrad epilogue, P and dS rounded to fp16 (2^-11 per operand; with a bf16 attention backward the weight gradients of the
  // first blocks stayed at 1.8e-2 whatever the GEMMs did, profiles/r06_fp16_backward_bringup.txt).
  const bool h16 = Pb == 4;
  constexpr float A1_INV = 1.0f / (1.0f - 0.015625f);         // csrc/f16x2.h: a1 = fp16((1 - 2^-6) x)
  const char* FA = (const char*)io.fwd_arena;
  char* A = (char*)io.bwd_arena;
  hipStream_t main_s = (hipStream_t)stream;
  const bool x2 = o.P == 2 && !h16;      // f16x2 forward, bf16 backward: the activations' single-pass operands are their bf16 copies
  const egv_bf16 *n3_hi, *n3_lo, *at_hi, *at_lo, *n1_hi, *n1_lo, *as_hi, *as_lo, *n2_hi, *n2_lo, *h_hi, *h_lo, *qt_hi, *qt_lo, *qs_hi, *qs_lo;
  saved_planes(FA, Pb, x2 ? F.n3_bf : F.n3_hi, F.n3_lo, n3_hi, n3_lo);
  saved_planes(FA, Pb, F.at_hi, F.at_lo, at_hi, at_lo);
  saved_planes(FA, Pb, x2 ? F.n1_bf : F.n1_hi, F.n1_lo, n1_hi, n1_lo);
  saved_planes(FA, Pb, F.as_hi, F.as_lo, as_hi, as_lo);
  saved_planes(FA, Pb, x2 ? F.n2_bf : F.n2_hi, F.n2_lo, n2_hi, n2_lo);
  saved_planes(FA, Pb, x2 ? F.h_bf : F.h_hi, F.h_lo, h_hi, h_lo);
  saved_planes(FA, Pb, F.qkvt_hi, F.qkvt_lo, qt_hi, qt_lo);
  saved_planes(FA, Pb, F.qkvs_hi, F.qkvs_lo, qs_hi, qs_lo);
  // the attention backward takes the forward output's lo plane whenever the forward wrote one, also in a single-pass backward
  // (delta = rowsum(dO o O) exact in O: egv_divided_attn_bwd)
  // (not when that plane holds fp16(value) for a single-product proj, egv_block_geom.f16_single bit 3: delta then comes from the bf16 plane)
  const bool proj1 = (g.f16_single & 8) != 0;
  const egv_bf16 *as_lo_f = (proj1 || h16) ? nullptr : at<egv_bf16>(FA, F.as_lo), *at_lo_f = (proj1 || h16) ? nullptr : at<egv_bf16>(FA, F.at_lo);
  const int afmt = h16 ? (proj1 ? 3 : 2) : (proj1 ? 1 : 0);       // the format egv_block_fwd wrote the attention outputs in
  const int amode = (afmt << 1) | (h16 ? 8 | 16 : 0);             // + dqkv as fp16, + q / k / v / dO read as fp16 (fp16 products throughout)
  // weight-gradient rescale: X is a1 of an f16x2 encoding wherever the op does NOT run one product (egv_block_geom.f16_single)
  const float walpha[6] = {h16 && !(g.f16_single & 4) ? A1_INV : 1.0f, h16 && !proj1 ? A1_INV : 1.0f, h16 && !(g.f16_single & 4) ? A1_INV : 1.0f,
                           h16 && !proj1 ? A1_INV : 1.0f, h16 && !(g.f16_single & 1) ? A1_INV : 1.0f, h16 && !(g.f16_single & 2) ? A1_INV : 1.0f};
  const int Pg = Pb;                     // passes code of every GEMM of the pass (4: one fp16 product)
  const float *tr = at<float>(FA, F.tr), *sr = at<float>(FA, F.sr);
  float* grads = io.grads;

  // The split-K slabs of the six weight gradients are reduced by ONE launch at the end of the call (egv_splitk_reduce_multi) when all
  // six run on the same stream -- the single wgrad side stream, or the main stream --: 12 reduce launches per step instead of 72 on
  // the stream whose queue drains last.  Weight gradients dealt to different streams keep their own reduce.
  bool defer_reduce = true;
  for (int i = 1; i < 6; ++i) defer_reduce = defer_reduce && io.side_stream[i] == io.side_stream[0];
#ifdef EGV_NO_MULTI_REDUCE
  defer_reduce = false;
#endif
  // the weight gradient dW[N,K] = dY^T X (TN kernel, bias gradient from the same pass) of weight i, on its side stream if it has one
  // (row0 / rows: the tail's space qkv gradient covers the k / v rows D .. 3 D of dW only)
  auto wgrad = [&](int i, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy, const egv_bf16* x_hi, const egv_bf16* x_lo,
                   int64_t ldx, int64_t row0 = 0, int64_t rows = 0) -> int {
    int64_t N, K;
    wshape(o, i, N, K);
    if (rows) N = rows;
    hipStream_t s = main_s;
    if (io.side_stream[i]) {
      s = (hipStream_t)io.side_stream[i];
      if (hipEventRecord((hipEvent_t)io.side_event[i], main_s) != hipSuccess) return EGV_ERR_LAUNCH;
      if (hipStreamWaitEvent(s, (hipEvent_t)io.side_event[i], 0) != hipSuccess) return EGV_ERR_LAUNCH;
    }
    egv_gemm_desc d = tn_desc(dy_hi, dy_lo, lddy, x_hi, x_lo, ldx, N, K, M, Pg, grads + goff[i] + row0 * K, grads + goff[6 + i] + row0, io.wgrad_ksplit[i],
                              at<float>(A, L.partial[i]), g.grid_cap);
    d.alpha = walpha[i];
    if (defer_reduce && d.ksplit > 1) d.accumulate = 2;        // slabs only; reduced below
    return egv_gemm_nt(&d, s);
  };

  // the three dgrads that feed a LayerNorm backward (d_n2, d_n1, d_n3): fp32; in the fp16 backward ONE plane of un-clamped fp16 in the
  // same buffer (half the bytes written here and read there: 77 -> 38.6 MB per launch at M = 25 120)
  auto ln_in = [&](egv_gemm_desc& d, float* buf) {
    if (h16) { d.out_hi = (egv_bf16*)buf; d.ldoh = D; d.out_fmt = 4; }
    else { d.out_f32 = buf; d.ldo = D; }
  };
  const int ln_fmt = h16 ? 3 : 0;        // egv_layernorm_bwd_partial: dx plane (bit 0) and dy plane (bit 1) as un-clamped fp16
  float* d_sr = at<float>(A, L.d_sr);    // null in tail mode (the CLS rows' d_sr is added to d_tr below)
  float* d_n1 = at<float>(A, L.d_n1);
  if (tail) {
    // ---- CLS tail: g_out is [B, D]; every other row of the block output has no gradient, so the MLP, norm2, the space proj and the
    // space attention's query side run on B rows in fp32 from the master weights (csrc/cls_tail.hip), and the attention backward
    // writes dK / dV of every key from the one CLS query
    const float *w_q = (const float*)p.w_hi[2], *w_proj = (const float*)p.w_hi[3], *w_fc1 = (const float*)p.w_hi[4],
                *w_fc2 = (const float*)p.w_hi[5];
    if (!w_q || !w_proj || !w_fc1 || !w_fc2) return EGV_ERR_ARG;
    const int32_t B = g.B;
    const int64_t ldc = o.S * o.D;
    const float* G = io.g_out;
    const float *n1c = at<float>(FA, F.n1c), *qc = at<float>(FA, F.qc), *oc = at<float>(FA, F.oc), *n2c = at<float>(FA, F.n2c),
                *hc = at<float>(FA, F.hc);
    float *dzc = at<float>(A, L.dzc), *dn2c = at<float>(A, L.dn2c), *dsrc = at<float>(A, L.dsrc), *doc = at<float>(A, L.doc),
          *dqc = at<float>(A, L.dqc), *lw = at<float>(A, L.lin_work);
    EGV_TRY(egv_cls_linear_dgrad(G, D, w_fc2, Hd, B, D, Hd, at<float>(FA, F.z), dzc, Hd, 0, lw, stream));
    EGV_TRY(egv_cls_linear_wgrad(G, D, hc, Hd, B, D, Hd, grads + goff[5], Hd, grads + goff[11], stream));
    EGV_TRY(egv_cls_linear_dgrad(dzc, Hd, w_fc1, D, B, Hd, D, nullptr, dn2c, D, 0, lw, stream));
    EGV_TRY(egv_cls_linear_wgrad(dzc, Hd, n2c, D, B, Hd, D, grads + goff[4], D, grads + goff[10], stream));
    EGV_TRY(egv_layernorm_bwd_partial(dn2c, nullptr, nullptr, D, sr, D, p.n2w, at<float>(FA, F.mean2), at<float>(FA, F.rstd2), B, D, G, nullptr,
                                      dsrc, D, nullptr, nullptr, 0, grads + goff[16], grads + goff[17], at<float>(A, L.ln_work[0]), stream));
    EGV_TRY(egv_cls_linear_wgrad(dsrc, D, oc, D, B, D, D, grads + goff[3], D, grads + goff[9], stream));
    EGV_TRY(egv_cls_linear_dgrad(dsrc, D, w_proj, D, B, D, D, nullptr, doc, D, 0, lw, stream));
    uint16_t *dkv_hi = (uint16_t*)at<egv_bf16>(A, L.dqkvs_hi), *dkv_lo = (uint16_t*)at<egv_bf16>(A, L.dqkvs_lo);
    const uint16_t *kv_hi = (const uint16_t*)at<egv_bf16>(FA, F.qkvs_hi), *kv_lo = (const uint16_t*)at<egv_bf16>(FA, F.qkvs_lo);
    EGV_TRY(egv_cls_attn_bwd(qc, D, kv_hi, kv_lo, kv_hi + D, kv_lo ? kv_lo + D : nullptr, 2 * D, h16 ? 1 : 0, oc, doc, at<float>(FA, F.lse_s), B,
                             (int32_t)o.S, g.H, dqc, dkv_hi, dkv_lo, dkv_hi + D, dkv_lo ? dkv_lo + D : nullptr, 2 * D, h16 ? 1 : 0, stream));
    // the space qkv weight: its q rows from the B CLS rows, its k / v rows from every token (the TN kernel, on the wgrad stream)
    EGV_TRY(egv_cls_linear_wgrad(dqc, D, n1c, D, B, D, D, grads + goff[2], D, grads + goff[8], stream));
    EGV_TRY(wgrad(2, (const egv_bf16*)dkv_hi, (const egv_bf16*)dkv_lo, 2 * D, n1_hi, n1_lo, D, D, 2 * D));
    {
      egv_gemm_desc d = nt_desc((const egv_bf16*)dkv_hi, (const egv_bf16*)dkv_lo, 2 * D, p.wt_hi[2] + D, p.wt_lo[2] ? p.wt_lo[2] + D : nullptr,
                                p.ldwt[2], M, D, 2 * D, Pg, g.grid_cap);
      ln_in(d, d_n1);
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
    EGV_TRY(egv_cls_linear_dgrad(dqc, D, w_q, D, B, D, D, nullptr, d_n1, ldc, h16 ? 2 : 1, lw, stream));
  } else {
    // ---- G as planes (handed over by the next block's LayerNorm-backward, or split here)
    const egv_bf16 *g_hi = io.g_hi, *g_lo = Pb == 3 ? io.g_lo : nullptr;
    if (!g_hi) {
      egv_bf16 *gh = at<egv_bf16>(A, L.g_hi), *gl = at<egv_bf16>(A, L.g_lo);
      if (h16) EGV_TRY(egv_f16x2_encode(io.g_out, D, M, D, gh, nullptr, nullptr, D, 2, stream));
      else EGV_TRY(egv_split_f32(io.g_out, D, M, D, gh, gl, D, nullptr, nullptr, 0, nullptr, stream));
      g_hi = gh; g_lo = gl;
    }
    // ---- MLP backward: dZ = (G . W2) * gelu'(z) leaves the fc2-dgrad epilogue already split
    egv_bf16 *dz_hi = at<egv_bf16>(A, L.dz_hi), *dz_lo = at<egv_bf16>(A, L.dz_lo);
    {
      egv_gemm_desc d = nt_desc(g_hi, g_lo, D, p.wt_hi[5], p.wt_lo[5], p.ldwt[5], M, Hd, D, Pg, g.grid_cap);
      d.act = EGV_ACT_GELU_BWD; d.aux_in = at<float>(FA, F.z); d.ldaux = Hd; d.aux_bf16 = g.z_bf16 ? (h16 ? 3 : 2) : 0;
      d.out_hi = dz_hi; d.out_lo = dz_lo; d.ldoh = Hd;
      if (h16) d.out_fmt = 4;               // dZ as one plane of un-clamped fp16
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
    EGV_TRY(wgrad(5, g_hi, g_lo, D, h_hi, h_lo, Hd));
    EGV_TRY(wgrad(4, dz_hi, dz_lo, Hd, n2_hi, n2_lo, D));
    float* d_n2 = at<float>(A, L.d_n2);
    {
      egv_gemm_desc d = nt_desc(dz_hi, dz_lo, Hd, p.wt_hi[4], p.wt_lo[4], p.ldwt[4], M, D, Hd, Pg, g.grid_cap);
      ln_in(d, d_n2);
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
    egv_bf16 *dsr_hi = at<egv_bf16>(A, L.dsr_hi), *dsr_lo = at<egv_bf16>(A, L.dsr_lo);
    EGV_TRY(egv_layernorm_bwd_partial(h16 ? nullptr : d_n2, h16 ? (const egv_bf16*)d_n2 : nullptr, nullptr, D, sr, D, p.n2w, at<float>(FA, F.mean2),
                              at<float>(FA, F.rstd2), M, D, io.g_out, nullptr,
                              d_sr, D, dsr_hi, dsr_lo, ln_fmt, grads + goff[16], grads + goff[17], at<float>(A, L.ln_work[0]), stream));
    // ---- spatial attention backward
    EGV_TRY(wgrad(3, dsr_hi, dsr_lo, D, as_hi, as_lo, D));
    egv_bf16 *das_hi = at<egv_bf16>(A, L.das_hi), *das_lo = at<egv_bf16>(A, L.das_lo);
    {
      egv_gemm_desc d = nt_desc(dsr_hi, dsr_lo, D, p.wt_hi[3], p.wt_lo[3], p.ldwt[3], M, D, D, Pg, g.grid_cap);
      d.out_hi = das_hi; d.out_lo = das_lo; d.ldoh = D;
      if (h16) d.out_fmt = 4;              // dO as one plane of un-clamped fp16
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
    egv_bf16 *dqs_hi = at<egv_bf16>(A, L.dqkvs_hi), *dqs_lo = at<egv_bf16>(A, L.dqkvs_lo);
    EGV_TRY(egv_divided_attn_bwd(qs_hi, qs_lo, as_hi, as_lo_f, das_hi, das_lo, at<float>(FA, F.lse_s), g.B, g.T, g.n, g.H, 0 | amode, h16 ? 1 : Pb, dqs_hi, dqs_lo,
                                 at<float>(A, L.attn_work), stream));
    EGV_TRY(wgrad(2, dqs_hi, dqs_lo, 3 * D, n1_hi, n1_lo, D));
    {
      egv_gemm_desc d = nt_desc(dqs_hi, dqs_lo, 3 * D, p.wt_hi[2], p.wt_lo[2], p.ldwt[2], M, D, 3 * D, Pg, g.grid_cap);
      ln_in(d, d_n1);
      EGV_TRY(egv_gemm_nt(&d, stream));
    }
  }
  float* d_tr = at<float>(A, L.d_tr);
  egv_bf16 *dtr_hi = at<egv_bf16>(A, L.dtr_hi), *dtr_lo = at<egv_bf16>(A, L.dtr_lo);
  EGV_TRY(egv_layernorm_bwd_partial(h16 ? nullptr : d_n1, h16 ? (const egv_bf16*)d_n1 : nullptr, nullptr, D, tr, D, p.n1w, at<float>(FA, F.mean1),
                            at<float>(FA, F.rstd1), M, D, nullptr, nullptr,
                            d_tr, D, dtr_hi, dtr_lo, ln_fmt, grads + goff[14], grads + goff[15], at<float>(A, L.ln_work[1]), stream));
  // tail: d_sr exists on the CLS rows only; it joins dx through d_tr (fp32; the planes above are what the time branch reads)
  if (tail) EGV_TRY(egv_cls_rows_add(d_tr, o.S * o.D, at<float>(A, L.dsrc), D, g.B, D, stream));
  // ---- temporal attention backward
  EGV_TRY(wgrad(1, dtr_hi, dtr_lo, D, at_hi, at_lo, D));
  egv_bf16 *dat_hi = at<egv_bf16>(A, L.dat_hi), *dat_lo = at<egv_bf16>(A, L.dat_lo);
  {
    egv_gemm_desc d = nt_desc(dtr_hi, dtr_lo, D, p.wt_hi[1], p.wt_lo[1], p.ldwt[1], M, D, D, Pg, g.grid_cap);
    d.out_hi = dat_hi; d.out_lo = dat_lo; d.ldoh = D;
    if (h16) d.out_fmt = 4;
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  egv_bf16 *dqt_hi = at<egv_bf16>(A, L.dqkvt_hi), *dqt_lo = at<egv_bf16>(A, L.dqkvt_lo);
  EGV_TRY(egv_divided_attn_bwd(qt_hi, qt_lo, at_hi, at_lo_f, dat_hi, dat_lo, at<float>(FA, F.lse_t), g.B, g.T, g.n, g.H, 1 | amode, h16 ? 1 : Pb, dqt_hi, dqt_lo,
                               at<float>(A, L.attn_work), stream));
  EGV_TRY(wgrad(0, dqt_hi, dqt_lo, 3 * D, n3_hi, n3_lo, D));
  float* d_n3 = at<float>(A, L.d_n3);
  {
    egv_gemm_desc d = nt_desc(dqt_hi, dqt_lo, 3 * D, p.wt_hi[0], p.wt_lo[0], p.ldwt[0], M, D, 3 * D, Pg, g.grid_cap);
    ln_in(d, d_n3);
    EGV_TRY(egv_gemm_nt(&d, stream));
  }
  // x feeds norm3, the tr residual and the sr residual: dx = d_tr + d_sr + LN3'(d_n3)
  EGV_TRY(egv_layernorm_bwd_partial(h16 ? nullptr : d_n3, h16 ? (const egv_bf16*)d_n3 : nullptr, nullptr, D, io.x, D, p.n3w, at<float>(FA, F.mean3),
                            at<float>(FA, F.rstd3), M, D, d_tr, d_sr,
                            io.d_x, D, io.dx_hi, Pb == 3 ? io.dx_lo : nullptr, ln_fmt, grads + goff[12], grads + goff[13],
                            at<float>(A, L.ln_work[2]), stream));
  if (defer_reduce) {
    const float* part[6]; float* outp[6]; float* csp[6]; int64_t mn[6]; int32_t ksv[6], mv[6];
    int cnt = 0;
    for (int i = 0; i < 6; ++i) {
      if (io.wgrad_ksplit[i] <= 1 || (tail && i > 2)) continue;
      int64_t N, K;
      wshape(o, i, N, K);
      const int64_t row0 = (tail && i == 2) ? D : 0;          // tail: the k / v rows of the space qkv gradient
      N -= row0;
      part[cnt] = at<float>(A, L.partial[i]); outp[cnt] = grads + goff[i] + row0 * K; csp[cnt] = grads + goff[6 + i] + row0;
      mn[cnt] = N * K; ksv[cnt] = io.wgrad_ksplit[i]; mv[cnt] = (int32_t)N;
      ++cnt;
    }
    // on the stream the weight gradients ran on (stream order: behind the last of them)
    if (cnt) EGV_TRY(egv_splitk_reduce_multi(cnt, part, outp, mn, ksv, csp, mv, io.side_stream[0] ? io.side_stream[0] : stream));
  }
  // the affine gradients of the three LayerNorms: their per-block partial sums are reduced by ONE launch (three before)
  {
    const float* w3[3] = {at<float>(A, L.ln_work[0]), at<float>(A, L.ln_work[1]), at<float>(A, L.ln_work[2])};
    float* g3[3] = {grads + goff[16], grads + goff[14], grads + goff[12]};
    float* b3[3] = {grads + goff[17], grads + goff[15], grads + goff[13]};
    if (tail) {                          // norm2 ran on the B CLS rows: its partial sums are those of a B-row launch
      EGV_TRY(egv_layernorm_bwd_reduce(1, w3, g.B, D, g3, b3, stream));
      EGV_TRY(egv_layernorm_bwd_reduce(2, w3 + 1, M, D, g3 + 1, b3 + 1, stream));
    } else {
      EGV_TRY(egv_layernorm_bwd_reduce(3, w3, M, D, g3, b3, stream));
    }
  }
  return EGV_OK;
}
