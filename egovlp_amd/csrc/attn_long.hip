// Key-tiled ("long") attention for groups of more than 288 keys: the space attention of the SpaceTimeTransformer at input
// resolutions above 224^2 (288^2 / 16: 325 keys, 336^2 / 14 and 384^2 / 16: 577, 448^2 / 16: 785) and DistilBERT's masked MHA
// up to its 512 positions.  The kernels of attn_mfma_fwd.hip / attn_mfma_bwd.hip keep ALL of a group's K and V in LDS and the
// scores of a query tile against all keys in registers, which ends at 288 keys; here the long axis is walked in 64-row tiles
// that go through a two-buffer LDS ring, so nothing grows with the key count and there is no structural upper bound (largest
// size tested: 785 keys, tests/test_gpu_attn_long.py).
//
//   forward : workgroup = (group, block of 128 queries): 8 waves, one 16-query tile each.  The workgroup walks the group's keys in
//             tiles of 64 (K and V planes in the swizzled image of attn_common.h); a wave keeps the online-softmax state of its
//             tile -- running maximum (exp2 domain), running sum, O accumulator rescaled ONCE per 64-key tile -- and writes what
//             the LDS-resident forward writes: output planes in every EGV_ATTN_OUT_* format, lse, and (space mode) the CLS query's
//             un-normalised partial for egv_attn_cls_combine.  The CLS query rides as query row n, as there.
//   dQ      : the same ownership and the same K / V ring; probabilities are rebuilt from the saved lse, so nothing is rescaled.
//             Space mode takes delta = rowsum(dO o O) from the forward's output planes (the CLS row's from egv_attn_cls_delta);
//             the text mode has no saved output, so it walks the keys twice (delta = sum_k P dP, then dQ), as
//             attn_bwd_dq_text_stream_kernel does.  delta is written for the second kernel.
//   dK / dV : workgroup = (group, block of 128 keys): a wave owns a 16-key fragment and the workgroup walks the QUERIES (Q and dO
//             planes, lse and delta) in tiles of 64 through the same ring.  CLS key / CLS query gradients go to the fp32 dcls
//             accumulators with atomics, exactly as in the short kernels.
//
// Tile choice.  A (group, 128-query) block instead of a whole group per workgroup: a 785-key group has 50 query tiles, and a
// wave that carried more than one tile's (q, m, l, O) through the key walk would leave the 128-VGPR budget below.  64 keys per
// tile: four score fragments per wave and tile keep one max / rescale per 24 (8) MFMAs of Q.K^T and 24 (8) of P.V, and a tile of
// all four planes is 32 KiB, so the two-buffer ring of the three-product instances is 64.5 KiB and TWO workgroups fit the 160 KiB
// of a CU.  One barrier per tile: tile t + 1 is staged into the other buffer by the same waves right before they compute on
// tile t, so its global loads are in flight under the MFMAs of the other waves and of the CU's second workgroup.
// Designed occupancy: 2 workgroups x 8 waves per CU = 4 waves per SIMD (<= 128 VGPRs, no scratch; the single-product instances
// use 32.5 KiB and are bounded by registers, not LDS).  K / V of a group are re-read once per 128-query block (3 to 7 times) --
// from L2: a group's planes are 0.3 - 0.4 MB and its blocks are neighbours in the grid.
//
// Every (passes, f16, out_fmt) / (passes, o_fmt, g_fmt, f16) / text (passes, dropout) combination of the short path is accepted
// and the same ones are rejected (one check serves both: attn_dispatch.h); operand loading, the fp16 split and the output formats
// are those of attn_common.h.  The text mode's dropout mask is the counter-based one of common.h at the ABSOLUTE element index
// ((b H + h) S + q) S + k.
#include "attn_common.h"
#include "egovlp_hip.h"

namespace {

constexpr int LONG_ROWS = ATT_TILE_ROWS;                     // rows (keys; queries in dK / dV) per LDS tile
constexpr int LONG_WAVES = ATT_TILE_WAVES;                   // waves per workgroup: 128 queries (keys in dK / dV) per block
constexpr int LONG_PLANE = LONG_ROWS * ATT_ROW_BYTES;        // 8 KiB
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

constexpr int long_buf_bytes(int passes, int nvec) { return (passes == 3 ? 4 : 2) * LONG_PLANE + nvec * LONG_ROWS * (int)sizeof(float); }
static_assert(2 * long_buf_bytes(3, 2) == att_tiled_lds(3, 2) && 2 * long_buf_bytes(1, 1) == att_tiled_lds(1, 1), "the ring the picks ask for");

// waves per SIMD the instances are compiled for: 4 (two 8-wave workgroups per CU, <= 128 VGPRs).  The three-product TEXT instances
// (fp32 sources split in registers, 64-bit dropout indices) need 134 / 142 VGPRs and would spill under that bound: they keep 3,
// i.e. one workgroup per CU -- captions of more than 288 tokens are not on the benchmarked path.
constexpr int long_min_waves(int mode, int passes) { return (mode == MODE_TEXT && passes == 3) ? 3 : 4; }

// one tile of a group's K and V (rows k0 .. k0 + 63, zero-filled past the last key) and its additive key bias
template <int MODE, int PASSES>
__device__ __forceinline__ void long_stage_kv(char* buf, const AttGeom& g, const AttGroup<MODE>& grp, int k0) {
  char* k_hi = buf;
  char* v_hi = buf + LONG_PLANE;
  char* k_lo = (PASSES == 3) ? buf + 2 * LONG_PLANE : nullptr;
  char* v_lo = (PASSES == 3) ? buf + 3 * LONG_PLANE : nullptr;
  float* kbias = (float*)(buf + ((PASSES == 3) ? 4 : 2) * LONG_PLANE);
  const long hoff = (long)grp.h * ATT_D;
  const long HD = (long)g.H * ATT_D;
  const int nrows = min(LONG_ROWS, g.nk - k0);
  if (MODE == MODE_SPACE) {
    att_stage_planes(k_hi, k_lo, g.ph, g.pl, nrows, LONG_ROWS, [&](int r) { return grp.k_tok(g, k0 + r) * g.tok_stride + HD + hoff; });
    att_stage_planes(v_hi, v_lo, g.ph, g.pl, nrows, LONG_ROWS, [&](int r) { return grp.k_tok(g, k0 + r) * g.tok_stride + 2 * HD + hoff; });
  } else {
    att_stage(k_hi, k_lo, nrows, LONG_ROWS, 1.0f, [&](int r) { return g.k + grp.k_tok(g, k0 + r) * g.tok_stride + hoff; });
    att_stage(v_hi, v_lo, nrows, LONG_ROWS, 1.0f, [&](int r) { return g.v + grp.k_tok(g, k0 + r) * g.tok_stride + hoff; });
  }
  for (int j = threadIdx.x; j < LONG_ROWS; j += blockDim.x) {
    const int kj = k0 + j;
    float bias = (kj < g.nk) ? 0.f : -1e30f;
    if (MODE == MODE_TEXT && kj < g.nk && g.mask[(long)grp.b * g.S + kj] == 0) bias = -1e30f;
    kbias[j] = bias;
  }
}

// ------------------------------------------------------------------------------------------------ forward
template <int MODE, int PASSES, bool F16 = false>
__global__ __launch_bounds__(LONG_WAVES * 64, long_min_waves(MODE, PASSES)) void attn_long_fwd_kernel(const AttGeom g, bf16_t* __restrict__ out_hi,
                                                                        bf16_t* __restrict__ out_lo, long out_stride,
                                                                        float* __restrict__ lse, float* __restrict__ cls_ws,
                                                                        const int nqb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool SP = (MODE == MODE_SPACE);
  constexpr int BUF = long_buf_bytes(PASSES, 1);
  constexpr int LO = 2 * LONG_PLANE;                 // k_lo - k_hi == v_lo - v_hi
  constexpr int KB = ((PASSES == 3) ? 4 : 2) * LONG_PLANE;

  const AttGroup<MODE> grp(g, (int)(blockIdx.x / (unsigned)nqb));
  const int qb = (int)(blockIdx.x % (unsigned)nqb);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long hoff = (long)grp.h * ATT_D;
  const int gq = lane >> 4;
  const int nq_all = SP ? g.nq + 1 : g.nq;           // + the CLS query row
  const int qt = qb * LONG_WAVES + wave;
  const bool active = qt * 16 < nq_all;              // wave-uniform; a wave without a tile still stages and meets the barriers
  const int qi = qt * 16 + (lane & 15);
  const bool is_cls = SP && qi >= g.nq;              // rows past n all alias the CLS row; only qi == n is stored
  const long qtok = is_cls ? grp.tok0 : grp.q_tok(g, min(qi, g.nq - 1));
  bf16x8_t qh[2], ql[2];
  if (SP) {
    att_gfrag_planes(g.ph, g.pl, qtok * g.tok_stride + hoff, 0, lane, qh[0], ql[0]);
    att_gfrag_planes(g.ph, g.pl, qtok * g.tok_stride + hoff, 1, lane, qh[1], ql[1]);
  } else {
    const float* qrow = g.q + qtok * g.tok_stride + hoff;
    att_gfrag(qrow, 0, lane, 1.0f, qh[0], ql[0]);
    att_gfrag(qrow, 1, lane, 1.0f, qh[1], ql[1]);
  }
  const uint64_t rowbase = (((uint64_t)grp.b * g.H + grp.h) * g.S + (uint64_t)min(qi, g.nq - 1)) * g.S;
  const EgvDrop dr = egv_drop_resolve(g.drop);

  float m = -3e38f, l = 0.f;                         // m: uniform over the four lane groups of a query; l: this lane group's part
  f32x4_t o[4];
#pragma unroll
  for (int df = 0; df < 4; ++df) o[df] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int ntk = (g.nk + LONG_ROWS - 1) / LONG_ROWS;
  long_stage_kv<MODE, PASSES>(smem, g, grp, 0);
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < ntk; ++t) {
    if (t + 1 < ntk) long_stage_kv<MODE, PASSES>(smem + ((t + 1) & 1) * BUF, g, grp, (t + 1) * LONG_ROWS);
    if (active) {
      const char* k_hi = smem + (t & 1) * BUF;
      const char* v_hi = k_hi + LONG_PLANE;
      const float* kbias = (const float*)(k_hi + KB);
      f32x4_t s[4];
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        s[kf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8_t ah = att_frag_cols(k_hi, kf * 16, ks, lane);
          bf16x8_t al = ah;
          if (PASSES == 3) al = att_frag_cols(k_hi + LO, kf * 16, ks, lane);
          s[kf] = att_mma<PASSES, F16>(ah, al, qh[ks], ql[ks], s[kf]);
        }
        const f32x4_t kb = *(const f32x4_t*)(kbias + kf * 16 + 4 * gq);
        s[kf] = s[kf] * (0.125f * LOG2E) + kb;       // q *= 64^-0.5 (video_transformer.py:106), applied to the scores; exp2 domain
      }
      if (SP && t == 0 && is_cls && grp.f > 0 && gq == 0) s[0][0] = -1e30f;     // CLS key x CLS query: group 0 only
      float cm = -3e38f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) cm = fmaxf(cm, fmaxf(fmaxf(s[kf][0], s[kf][1]), fmaxf(s[kf][2], s[kf][3])));
      cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      const float mn = fmaxf(m, cm);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);        // first tile: 2^(-3e38 - mn) = 0 and l, o are 0 anyway
      m = mn;
      float ps = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kf][r] = __builtin_amdgcn_exp2f(s[kf][r] - mn);
          ps += s[kf][r];
        }
      l = l * alpha + ps;
      if (MODE == MODE_TEXT && g.drop.thresh != 0u) {
        // dropout on the attention weights (softmax -> dropout -> . V): survivors scaled by 1 / (1 - p), the normaliser l is the
        // softmax's; the mask index is the absolute (b, h, q, k) one of the short kernels
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kf][r] *= egv_drop_scale(dr, rowbase + (uint64_t)(t * LONG_ROWS + kf * 16 + 4 * gq + r));
      }
#pragma unroll
      for (int df = 0; df < 4; ++df) o[df] = o[df] * alpha;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float pv[8] = {s[2 * c][0], s[2 * c][1], s[2 * c][2], s[2 * c][3],
                       s[2 * c + 1][0], s[2 * c + 1][1], s[2 * c + 1][2], s[2 * c + 1][3]};
        bf16x8_t ph, pl;
        att_split8<F16>(pv, ph, pl);
#pragma unroll
        for (int df = 0; df < 4; ++df) {
          const bf16x8_t vh = att_frag_rows(v_hi, 32 * c, df * 16, lane);
          bf16x8_t vl = vh;
          if (PASSES == 3) vl = att_frag_rows(v_hi + LO, 32 * c, df * 16, lane);
          o[df] = att_mma<PASSES, F16>(vh, vl, ph, pl, o[df]);
        }
      }
    }
    __syncthreads();                                 // tile t + 1 is staged, and every wave is done with tile t's buffer
  }
  if (!active) return;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (SP && qi == g.nq) {
    // CLS query x this frame's keys: un-normalised partial for egv_attn_cls_combine (natural units)
    float* w = cls_ws + (((long)grp.b * g.H + grp.h) * g.T + grp.f) * 68;
#pragma unroll
    for (int df = 0; df < 4; ++df) *(f32x4_t*)(w + df * 16 + 4 * gq) = o[df];
    if (gq == 0) {
      w[64] = m * LN2;
      w[65] = l;
    }
  } else if (qi < g.nq) {
    const float inv = 1.0f / l;
    bf16_t* oh = out_hi + qtok * out_stride + hoff;
    bf16_t* ol = out_lo ? out_lo + qtok * out_stride + hoff : nullptr;          // EGV_ATTN_OUT_F16 / single product: no second plane
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      uint32_t h0, h1, l0, l1;
      att_out2(o[df][0] * inv, o[df][1] * inv, g.out_fmt, h0, l0);
      att_out2(o[df][2] * inv, o[df][3] * inv, g.out_fmt, h1, l1);
      const int d = df * 16 + 4 * gq;
      egv_store<EGV_NT_SPACE_ATTN>(oh + d, (u32x2_t){h0, h1});
      if (ol) egv_store<EGV_NT_SPACE_ATTN>(ol + d, (u32x2_t){l0, l1});
    }
    if (gq == 0 && lse) lse[((long)grp.b * g.H + grp.h) * g.S + (qtok - grp.tok0)] = (m + __log2f(l)) * LN2;
  }
}

// ------------------------------------------------------------------------------------------------ dQ
template <int MODE, int PASSES, bool F16 = false>
__global__ __launch_bounds__(LONG_WAVES * 64, long_min_waves(MODE, PASSES)) void attn_long_dq_kernel(const AttGeom g, const AttGrad gr, const int nqb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool SP = (MODE == MODE_SPACE);
  constexpr int BUF = long_buf_bytes(PASSES, 1);
  constexpr int LO = 2 * LONG_PLANE;
  constexpr int KB = ((PASSES == 3) ? 4 : 2) * LONG_PLANE;

  const AttGroup<MODE> grp(g, (int)(blockIdx.x / (unsigned)nqb));
  const int qb = (int)(blockIdx.x % (unsigned)nqb);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long hoff = (long)grp.h * ATT_D;
  const int gq = lane >> 4;
  const int nq_all = SP ? g.nq + 1 : g.nq;
  const int qt = qb * LONG_WAVES + wave;
  const bool active = qt * 16 < nq_all;
  const int qi = qt * 16 + (lane & 15);
  const bool is_cls = SP && qi >= g.nq;
  const long tok = is_cls ? grp.tok0 : grp.q_tok(g, min(qi, g.nq - 1));
  const long lrow = ((long)grp.b * g.H + grp.h) * g.S + (tok - grp.tok0);
  const float L2 = gr.lse[lrow] * LOG2E;             // P = 2^(s 64^-0.5 log2 e + bias - L log2 e)
  bf16x8_t qh[2], ql[2], gh[2], gl[2];
  float delta = 0.f;
  if (SP) {
    bf16x8_t oh[2], ol[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      att_gfrag_planes(g.ph, g.pl, tok * g.tok_stride + hoff, ks, lane, qh[ks], ql[ks]);
      att_gfrag_planes(gr.doh, gr.dol, tok * gr.do_stride + hoff, ks, lane, gh[ks], gl[ks]);
      att_gfrag_planes(gr.oh, gr.ol, tok * gr.do_stride + hoff, ks, lane, oh[ks], ol[ks]);
    }
    // delta = rowsum(dO o O) from the forward's output planes, as in attn_bwd_dq_stream_kernel
    delta = frag_dot8<F16>(gh[0], gl[0], gr.dol != nullptr, oh[0], ol[0], gr.ol != nullptr, gr.o_fmt) +
            frag_dot8<F16>(gh[1], gl[1], gr.dol != nullptr, oh[1], ol[1], gr.ol != nullptr, gr.o_fmt);
    delta += __shfl_xor(delta, 16, 64);
    delta += __shfl_xor(delta, 32, 64);
    if (is_cls) delta = gr.delta[lrow];              // the CLS row's delta spans all frame groups: precomputed
  } else {
    const float* qrow = g.q + tok * g.tok_stride + hoff;
    const float* grow = gr.d_out + tok * gr.do_stride + hoff;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      att_gfrag(qrow, ks, lane, 1.0f, qh[ks], ql[ks]);
      att_gfrag(grow, ks, lane, 1.0f, gh[ks], gl[ks]);
    }
  }
  const uint64_t rowbase = (((uint64_t)grp.b * g.H + grp.h) * g.S + (uint64_t)min(qi, g.nq - 1)) * g.S;
  const EgvDrop dr = egv_drop_resolve(g.drop);

  f32x4_t dq[4];
#pragma unroll
  for (int df = 0; df < 4; ++df) dq[df] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // the text mode walks the keys twice (no saved output planes to take delta from): walk 0 sums delta = sum_k P dP, walk 1 forms dQ
  const int ntk = (g.nk + LONG_ROWS - 1) / LONG_ROWS;
  const int nit = SP ? ntk : 2 * ntk;
  long_stage_kv<MODE, PASSES>(smem, g, grp, 0);
  __syncthreads();
#pragma unroll 1
  for (int it = 0; it < nit; ++it) {
    if (it + 1 < nit) {
      const int tn = (it + 1 >= ntk) ? it + 1 - ntk : it + 1;
      long_stage_kv<MODE, PASSES>(smem + ((it + 1) & 1) * BUF, g, grp, tn * LONG_ROWS);
    }
    const bool second = SP || it >= ntk;             // uniform
    const int t = (it >= ntk) ? it - ntk : it;
    if (!SP && it == ntk) {
      delta += __shfl_xor(delta, 16, 64);
      delta += __shfl_xor(delta, 32, 64);
    }
    if (active) {
      const char* k_hi = smem + (it & 1) * BUF;
      const char* v_hi = k_hi + LONG_PLANE;
      const float* kbias = (const float*)(k_hi + KB);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float dsv[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int kf = 2 * c + h;
          f32x4_t sc = {0.f, 0.f, 0.f, 0.f};
          f32x4_t d = sc;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8_t ah = att_frag_cols(k_hi, kf * 16, ks, lane);
            bf16x8_t al = ah;
            if (PASSES == 3) al = att_frag_cols(k_hi + LO, kf * 16, ks, lane);
            sc = att_mma<PASSES, F16>(ah, al, qh[ks], ql[ks], sc);
            const bf16x8_t bh = att_frag_cols(v_hi, kf * 16, ks, lane);
            bf16x8_t bl = bh;
            if (PASSES == 3) bl = att_frag_cols(v_hi + LO, kf * 16, ks, lane);
            d = att_mma<PASSES, F16>(bh, bl, gh[ks], gl[ks], d);
          }
          const f32x4_t kb = *(const f32x4_t*)(kbias + kf * 16 + 4 * gq);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pr = __builtin_amdgcn_exp2f(sc[r] * (0.125f * LOG2E) + (kb[r] - L2));
            if (SP && t == 0 && kf == 0 && r == 0 && is_cls && grp.f > 0 && gq == 0) pr = 0.f;   // CLS key x CLS query: group 0 only
            float dp = d[r];
            if (MODE == MODE_TEXT && g.drop.thresh != 0u)                                        // dP = (dO . V) o M'
              dp *= egv_drop_scale(dr, rowbase + (uint64_t)(t * LONG_ROWS + kf * 16 + 4 * gq + r));
            if (second) dsv[4 * h + r] = pr * (dp - delta);
            else delta += pr * dp;
          }
        }
        if (second) {
          bf16x8_t sh, sl;
          att_split8<F16>(dsv, sh, sl);
#pragma unroll
          for (int df = 0; df < 4; ++df) {
            const bf16x8_t kh = att_frag_rows(k_hi, 32 * c, df * 16, lane);
            bf16x8_t kl = kh;
            if (PASSES == 3) kl = att_frag_rows(k_hi + LO, 32 * c, df * 16, lane);
            dq[df] = att_mma<PASSES, F16>(kh, kl, sh, sl, dq[df]);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  if (SP && qi == g.nq) {
    float* a = gr.dcls + ((long)grp.b * g.H + grp.h) * 192;
#pragma unroll
    for (int df = 0; df < 4; ++df)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(a + df * 16 + 4 * gq + r, dq[df][r]);
  } else if (qi < g.nq) {
    if (SP) {
#pragma unroll
      for (int df = 0; df < 4; ++df)
        store_planes4(gr.gh, gr.gl, tok * gr.tok_stride + hoff + df * 16 + 4 * gq, dq[df] * 0.125f, gr.g_fmt);
    } else {
      float* out = gr.dq + tok * gr.tok_stride + hoff;
#pragma unroll
      for (int df = 0; df < 4; ++df) *(f32x4_t*)(out + df * 16 + 4 * gq) = dq[df] * 0.125f;
    }
    if (gq == 0) gr.delta[lrow] = delta;
  }
}

// ----------------------------------------------------------------------------------------------- dK / dV
template <int MODE, int PASSES, bool F16 = false>
__global__ __launch_bounds__(LONG_WAVES * 64, long_min_waves(MODE, PASSES)) void attn_long_dkv_kernel(const AttGeom g, const AttGrad gr, const int nkb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool SP = (MODE == MODE_SPACE);
  constexpr int BUF = long_buf_bytes(PASSES, 2);
  constexpr int LO = 2 * LONG_PLANE;                 // q_lo - q_hi == do_lo - do_hi
  constexpr int VEC = ((PASSES == 3) ? 4 : 2) * LONG_PLANE;

  const AttGroup<MODE> grp(g, (int)(blockIdx.x / (unsigned)nkb));
  const int kblk = (int)(blockIdx.x % (unsigned)nkb);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long hoff = (long)grp.h * ATT_D;
  const long HD = (long)g.H * ATT_D;
  const int gq = lane >> 4;
  const int nq_all = SP ? g.nq + 1 : g.nq;           // query row n = the clip's CLS query (MODE_SPACE)
  auto qrow_tok = [&](int r) { return (SP && r >= g.nq) ? grp.tok0 : grp.q_tok(g, r); };

  // one tile of the group's queries: Q and dO planes (zero rows past the last query), lse (exp2 domain) and delta
  auto stage_q = [&](char* buf, int q0) {
    char* q_hi = buf;
    char* o_hi = buf + LONG_PLANE;
    char* q_lo = (PASSES == 3) ? buf + 2 * LONG_PLANE : nullptr;
    char* o_lo = (PASSES == 3) ? buf + 3 * LONG_PLANE : nullptr;
    float* lse_s = (float*)(buf + VEC);
    float* del_s = lse_s + LONG_ROWS;
    const int nrows = min(LONG_ROWS, nq_all - q0);
    if (SP) {
      att_stage_planes(q_hi, q_lo, g.ph, g.pl, nrows, LONG_ROWS, [&](int r) { return qrow_tok(q0 + r) * g.tok_stride + hoff; });
      att_stage_planes(o_hi, o_lo, gr.doh, gr.dol, nrows, LONG_ROWS, [&](int r) { return qrow_tok(q0 + r) * gr.do_stride + hoff; });
    } else {
      att_stage(q_hi, q_lo, nrows, LONG_ROWS, 1.0f, [&](int r) { return g.q + grp.q_tok(g, q0 + r) * g.tok_stride + hoff; });
      att_stage(o_hi, o_lo, nrows, LONG_ROWS, 1.0f, [&](int r) { return gr.d_out + grp.q_tok(g, q0 + r) * gr.do_stride + hoff; });
    }
    for (int i = threadIdx.x; i < LONG_ROWS; i += blockDim.x) {
      float L = 1e30f, dl = 0.f;                     // padded query rows: P = 2^(s - 1e30) = 0
      if (q0 + i < nq_all) {
        const long lrow = ((long)grp.b * g.H + grp.h) * g.S + (qrow_tok(q0 + i) - grp.tok0);
        L = gr.lse[lrow];
        dl = gr.delta[lrow];
      }
      lse_s[i] = L * LOG2E;
      del_s[i] = dl;
    }
  };

  const int kf = kblk * LONG_WAVES + wave;
  const bool active = kf * 16 < g.nk;                // wave-uniform
  const int kj = kf * 16 + (lane & 15);
  const int kc = min(kj, g.nk - 1);
  const long ktok = grp.k_tok(g, kc);
  bf16x8_t kh[2], kl[2], vh[2], vl[2];
  if (SP) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      att_gfrag_planes(g.ph, g.pl, ktok * g.tok_stride + HD + hoff, ks, lane, kh[ks], kl[ks]);
      att_gfrag_planes(g.ph, g.pl, ktok * g.tok_stride + 2 * HD + hoff, ks, lane, vh[ks], vl[ks]);
    }
  } else {
    const float* krow = g.k + ktok * g.tok_stride + hoff;
    const float* vrow = g.v + ktok * g.tok_stride + hoff;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      att_gfrag(krow, ks, lane, 1.0f, kh[ks], kl[ks]);
      att_gfrag(vrow, ks, lane, 1.0f, vh[ks], vl[ks]);
    }
  }
  float kb = (kj < g.nk) ? 0.f : -1e30f;             // (0 or -1e30: the same in the exp2 domain)
  if (MODE == MODE_TEXT && kj < g.nk && g.mask[(long)grp.b * g.S + kj] == 0) kb = -1e30f;
  const bool excl_cls = SP && grp.f > 0 && kj == 0;  // CLS key x CLS query is counted in frame-group 0 only
  const EgvDrop dr = egv_drop_resolve(g.drop);
  const uint64_t grpbase = ((uint64_t)grp.b * g.H + grp.h) * g.S;

  f32x4_t dk[4], dv[4];
#pragma unroll
  for (int df = 0; df < 4; ++df) {
    dk[df] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    dv[df] = dk[df];
  }

  const int ntq = (nq_all + LONG_ROWS - 1) / LONG_ROWS;
  stage_q(smem, 0);
  __syncthreads();
#pragma unroll 1
  for (int t = 0; t < ntq; ++t) {
    if (t + 1 < ntq) stage_q(smem + ((t + 1) & 1) * BUF, (t + 1) * LONG_ROWS);
    if (active) {
      const char* q_hi = smem + (t & 1) * BUF;
      const char* o_hi = q_hi + LONG_PLANE;
      const float* lse_s = (const float*)(q_hi + VEC);
      const int q0 = t * LONG_ROWS;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float pv[8], dsv[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r0 = 32 * c + 16 * h;
          f32x4_t s = {0.f, 0.f, 0.f, 0.f};
          f32x4_t d = s;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8_t ah = att_frag_cols(q_hi, r0, ks, lane);
            bf16x8_t al = ah;
            if (PASSES == 3) al = att_frag_cols(q_hi + LO, r0, ks, lane);
            s = att_mma<PASSES, F16>(ah, al, kh[ks], kl[ks], s);
            const bf16x8_t bh = att_frag_cols(o_hi, r0, ks, lane);
            bf16x8_t bl = bh;
            if (PASSES == 3) bl = att_frag_cols(o_hi + LO, r0, ks, lane);
            d = att_mma<PASSES, F16>(bh, bl, vh[ks], vl[ks], d);
          }
          const f32x4_t L4 = *(const f32x4_t*)(lse_s + r0 + 4 * gq);
          const f32x4_t D4 = *(const f32x4_t*)(lse_s + LONG_ROWS + r0 + 4 * gq);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qrow = q0 + r0 + 4 * gq + r;
            float pr = __builtin_amdgcn_exp2f(s[r] * (0.125f * LOG2E) + (kb - L4[r]));
            if (excl_cls && qrow == g.nq) pr = 0.f;
            float mk = 1.0f;                         // dropout mask of the forward for (query qrow, key kj), DistilBERT only
            if (MODE == MODE_TEXT && g.drop.thresh != 0u)
              mk = egv_drop_scale(dr, (grpbase + (uint64_t)min(qrow, g.nq - 1)) * g.S + kc);
            pv[4 * h + r] = pr * mk;                       // dV = (P o M')^T dO
            dsv[4 * h + r] = pr * (d[r] * mk - D4[r]);     // dS = P o (dP - delta), dP = (dO . V) o M'
          }
        }
        bf16x8_t ph, pl, sh, sl;
        att_split8<F16>(pv, ph, pl);
        att_split8<F16>(dsv, sh, sl);
#pragma unroll
        for (int df = 0; df < 4; ++df) {
          const bf16x8_t gh = att_frag_rows(o_hi, 32 * c, df * 16, lane);
          bf16x8_t gl = gh;
          if (PASSES == 3) gl = att_frag_rows(o_hi + LO, 32 * c, df * 16, lane);
          const bf16x8_t qh = att_frag_rows(q_hi, 32 * c, df * 16, lane);
          bf16x8_t ql = qh;
          if (PASSES == 3) ql = att_frag_rows(q_hi + LO, 32 * c, df * 16, lane);
          dv[df] = att_mma<PASSES, F16>(gh, gl, ph, pl, dv[df]);
          dk[df] = att_mma<PASSES, F16>(qh, ql, sh, sl, dk[df]);
        }
      }
    }
    __syncthreads();
  }
  if (!active || kj >= g.nk) return;
  if (SP && kj == 0) {
    // the CLS key / value are shared by the T frame-groups of a clip: raw fp32 accumulation (finish kernel scales)
    float* a = gr.dcls + ((long)grp.b * g.H + grp.h) * 192;
#pragma unroll
    for (int df = 0; df < 4; ++df)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        atomicAdd(a + 64 + df * 16 + 4 * gq + r, dk[df][r]);
        atomicAdd(a + 128 + df * 16 + 4 * gq + r, dv[df][r]);
      }
  } else if (SP) {
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const long o = ktok * gr.tok_stride + hoff + df * 16 + 4 * gq;
      store_planes4(gr.gh, gr.gl, o + HD, dk[df] * 0.125f, gr.g_fmt);
      store_planes4(gr.gh, gr.gl, o + 2 * HD, dv[df], gr.g_fmt);
    }
  } else {
    float* okp = gr.dk + ktok * gr.tok_stride + hoff;
    float* ovp = gr.dv + ktok * gr.tok_stride + hoff;
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const int d = df * 16 + 4 * gq;
      *(f32x4_t*)(okp + d) = dk[df] * 0.125f;
      *(f32x4_t*)(ovp + d) = dv[df];
    }
  }
}

}  // namespace

// The picks (attn_dispatch.h) carry the blocks of 128 rows per group -- a kernel argument -- and the one-dimensional grid groups x
// blocks.  fp16 operands exist in the space instances the LDS-resident path has them in: three-product forward, one-product backward.
int egv_attn_long_fwd(int mode, const AttPick& p, const AttGeom& g, bf16_t* oh, bf16_t* ol, long ostride, float* lse, float* cls_ws,
                      hipStream_t s) {
  return att_instance<0>(p, [&](auto, auto passes, auto f16) -> int {
    constexpr int PASSES = passes;
    constexpr bool F16 = f16;
    if constexpr (!F16 || PASSES == 3)
      if (mode == MODE_SPACE) return att_launch(attn_long_fwd_kernel<MODE_SPACE, PASSES, F16>, p, s, g, oh, ol, ostride, lse, cls_ws, p.nblk);
    if constexpr (!F16)
      if (mode == MODE_TEXT) return att_launch(attn_long_fwd_kernel<MODE_TEXT, PASSES, false>, p, s, g, oh, ol, ostride, lse, cls_ws, p.nblk);
    return EGV_ERR_ARG;
  });
}

int egv_attn_long_bwd(int mode, const AttPick& dq, const AttPick& dkv, const AttGeom& g, const AttGrad& gr, hipStream_t s) {
  return att_instance<0>(dq, [&](auto, auto passes, auto f16) -> int {
    constexpr int PASSES = passes;
    constexpr bool F16 = f16;
    if constexpr (!F16 || PASSES == 1)
      if (mode == MODE_SPACE) {
        const int rc = att_launch(attn_long_dq_kernel<MODE_SPACE, PASSES, F16>, dq, s, g, gr, dq.nblk);
        return rc ? rc : att_launch(attn_long_dkv_kernel<MODE_SPACE, PASSES, F16>, dkv, s, g, gr, dkv.nblk);
      }
    if constexpr (!F16)
      if (mode == MODE_TEXT) {
        const int rc = att_launch(attn_long_dq_kernel<MODE_TEXT, PASSES, false>, dq, s, g, gr, dq.nblk);
        return rc ? rc : att_launch(attn_long_dkv_kernel<MODE_TEXT, PASSES, false>, dkv, s, g, gr, dkv.nblk);
      }
    return EGV_ERR_ARG;
  });
}
