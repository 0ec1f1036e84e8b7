// Pairwise sigmoid contrastive head (SigLIP: Zhai et al. 2023) with EgoNCE's positives, for any n in [1, 65 536]:
//   tn_i = text_i / max(|text_i|, eps), vn_j likewise;   x_ij = tn_i . vn_j;   t = exp(s);   u_ij = t x_ij + b
//   z_ij = +1 where m_ij, else -1;   L = (1 / n) sum_ij softplus(-z_ij u_ij)
// with m the mask of the EgoNCE heads (the stats step at the top of egonce_long.hip; no noun / verb vectors: m = I, plain SigLIP),
// s the logit scale and b the logit bias, both read from the DEVICE.  With p_ij = sigmoid(-z_ij u_ij):
//   G_ij = dL/dx_ij = -(t / n) z_ij p_ij;   d tn = G vn,  d vn = G^T tn (+ the backward of the normalisation)
//   dL/ds = sum_ij G_ij x_ij;   dL/db = -(1 / n) sum_ij z_ij p_ij
// Every pair is its own binary decision, so there are no row or column statistics: loss and gradient come out of ONE walk of the
// tile grid per direction, where the long EgoNCE head walks it for statistics and again for gradients.  Nothing of size n x n is in
// memory; all arithmetic fp32 on the fp32-input MFMA (egonce_tile.h); every reduction runs in a fixed order (no float atomics).
//
//   prep    the long head's (egonce_tile.h): tn / vn zero-padded to Dp, the packed noun / verb words, norms, the bad-entry flags.
//   walk    the walk of egonce_tile.h (prologue, tile pieces, second product and store are its pieces); this head's own part is the
//           arithmetic on a tile's pairs: u, p and G in the fragment's registers.  Launched with roles
//           (tn, vn) and (vn, tn): the mask is symmetric.  In the (tn, vn) walk each lane also sums its loss terms, G x and z p (per
//           tile first, then into the running sums); the workgroup stores ONE partial of each per (row tile, column range).
//           Rows and columns >= n of the last tile are masked out of all of them: a padded pair has u = b, a FINITE loss term.
//           Without gradient outputs only the (tn, vn) walk runs, without the second product.
//   finish  egonce_tile.h: sum of the gradient partials in a fixed order + the backward of the normalisation.
//   reduce  one workgroup: the loss, scale and bias partials in a fixed order in double -> loss (NaN if any flag), d_scale, d_bias.
//
// egv_sigmoid_from_sim is the same loss on a GIVEN similarity matrix (mask = sim_v * sim_n + I > 0, as egv_egonce_from_sim forms it):
// one element-wise pass with block partials and the same reduce.
#include "egonce_tile.h"
#include "egovlp_hip.h"

namespace {

constexpr int SIG_WALK_WGS = 512;      // column ranges are chosen so that a walk has about this many workgroups: two per CU, which is
                                       // what its registers allow (the gradient partials of 512 workgroups are 32 MB at 4 096 rows)
constexpr int SIG_SIM_BLOCKS = 1024;    // from_sim: at most this many blocks, each with one partial of the three sums

struct SigLayout : EglPrepLayout {
  int tps, ns;
  long gpart, lpart;   // offsets in floats, behind the prep outputs
};

inline SigLayout sig_layout(int n, int D, int dn, int dv) {
  SigLayout L{egl_prep_layout(n, D, dn, dv)};
  egl_split(L.ntiles, L.ntiles, SIG_WALK_WGS, L.tps, L.ns);
  const long np = L.np;
  long o = L.total;
  L.gpart = o;  o += (long)L.ns * np * L.Dp;
  L.lpart = o;  o += 3L * L.ns * L.ntiles;           // loss, sum G x, sum z p: one partial of each per workgroup of the walk
  L.total = o;
  return L;
}

// one pair: a = -z u;  sp = softplus(a) = max(a, 0) + log1p(exp(-|a|)),  zp = z sigmoid(a); finite for any finite u
template <bool SP = true>
__device__ __forceinline__ void sig_pair(float u, bool pos, float& sp, float& zp) {
  const float a = pos ? -u : u;
  const float e = expf(-fabsf(a));
  sp = SP ? fmaxf(a, 0.f) + log1pf(e) : 0.f;
  const float p = (a >= 0.f ? 1.0f : e) / (1.0f + e);
  zp = pos ? p : -p;
}

// ------------------------------------------------------------------------------------------------ walk
template <int DP, bool GRAD, bool SUMS>
__global__ __launch_bounds__(256, 2) void sig_walk_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const uint32_t* __restrict__ words, int n, int np, int W, int wn,
                                                          int mode, const float* __restrict__ logit_scale,
                                                          const float* __restrict__ logit_bias, int tps,
                                                          float* __restrict__ gpart /* [ranges][np][DP] */,
                                                          float* __restrict__ lpart /* [3][ranges][tiles]; SUMS only */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sh[4];
  EGL_WALK_LDS(DP);
  const float t = expf(logit_scale[0]), b = logit_bias[0];
  const float sc = -t / (float)n;
  float ls = 0.f, gx = 0.f, zs = 0.f;                 // this lane's share of sum softplus, sum G X, sum z p
  EGL_WALK_BEGIN(DP, A, np, ntiles, tps);
  const bool live = gi < n;

  f32x4_t acc[DP / 64][4];
  egl_acc_zero<DP>(acc);

#pragma unroll 1
  for (int tl = t0; tl < t1; ++tl) {
    const int j0 = tl * EGL_TILE;
    __syncthreads();                                  // every wave is done with the previous tile
    egl_stage_tile<DP>(bt, B, j0);
    egl_mask_tile(words, words, W, wn, mode, i0, j0, 1, mb);
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    float tls = 0.f, tgx = 0.f, tzs = 0.f;            // the tile's 16 terms first: the running sums take one addition per tile
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xv = x[jf][r];
        float sp, zp;
        sig_pair<SUMS>(fmaf(t, xv, b), ((mbits[jf] >> (4 * g + r)) & 1u) != 0u, sp, zp);
        const bool ok = live && j0 + jf * 16 + 4 * g + r < n;     // padded rows / columns: u = b there, a finite term
        const float gv = ok ? sc * zp : 0.f;
        tls += ok ? sp : 0.f;
        tzs += ok ? zp : 0.f;
        tgx += gv * xv;
        x[jf][r] = gv;
      }
    ls += tls;
    gx += tgx;
    zs += tzs;
    if constexpr (GRAD) {
      EGL_SECOND_PRODUCT(DP);
    }
  }
  if constexpr (GRAD) EGL_STORE_GPART(DP, gpart, np);
  if constexpr (SUMS) {
    const long cnt = (long)gridDim.y * ntiles, at = (long)blockIdx.y * ntiles + blockIdx.x;
    ls = egv_block_sum_256(ls, sh);
    gx = egv_block_sum_256(gx, sh);
    zs = egv_block_sum_256(zs, sh);
    if (threadIdx.x == 0) {
      lpart[at] = ls;
      lpart[cnt + at] = gx;
      lpart[2 * cnt + at] = zs;
    }
  }
}

// ------------------------------------------------------------------------------------------------ reduce
// part: [3][count] partials of sum softplus, sum G x and sum z p -> loss = S0 / n, d_scale = gscale * S1, d_bias = -S2 / n.  One
// workgroup, double, fixed order.  flags (optional): any non-zero entry of [n] makes the loss NaN.
__global__ __launch_bounds__(256) void sig_reduce_kernel(const float* __restrict__ part, int count, int n,
                                                         const float* __restrict__ flags, float* __restrict__ loss,
                                                         float* __restrict__ d_scale, float* __restrict__ d_bias) {
  __shared__ double red[256];
  int bad = 0;
  if (flags)
    for (int i = threadIdx.x; i < n; i += 256) bad |= flags[i] != 0.f;
  bad = __syncthreads_or(bad);
  const double s0 = egv_sum_partials_256(part, count, red);
  __syncthreads();
  const double s1 = egv_sum_partials_256(part + count, count, red);
  __syncthreads();
  const double s2 = egv_sum_partials_256(part + 2L * count, count, red);
  if (threadIdx.x == 0) {
    loss[0] = bad ? __builtin_nanf("") : (float)(s0 / (double)n);
    if (d_scale) d_scale[0] = (float)s1;
    if (d_bias) d_bias[0] = (float)(-s2 / (double)n);
  }
}

// ------------------------------------------------------------------------------------------------ from a given similarity matrix
// the mask of egonce_mask_from_sim_kernel (egonce.hip): sim_v * sim_n + I > 0; noun only: sim_n + I; else sim_v + I; no sims: I
__global__ __launch_bounds__(256) void sig_from_sim_kernel(const float* __restrict__ x, const float* __restrict__ sim_v,
                                                           const float* __restrict__ sim_n, int n, int use_noun, int use_verb,
                                                           const float* __restrict__ logit_scale,
                                                           const float* __restrict__ logit_bias, float* __restrict__ dx,
                                                           float* __restrict__ part /* [3][blocks] */) {
  __shared__ float sh[4];
  const float t = expf(logit_scale[0]), b = logit_bias[0];
  const float sc = -t / (float)n;
  const long nn = (long)n * n;
  float ls = 0.f, gx = 0.f, zs = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nn; i += (long)gridDim.x * 256) {
    const float d = (i / n == i % n) ? 1.f : 0.f;
    float m = d;
    if (sim_v || sim_n) {
      if (use_noun && use_verb) m = sim_v[i] * sim_n[i] + d;
      else if (use_noun) m = sim_n[i] + d;
      else m = sim_v[i] + d;
    }
    const float xv = x[i];
    float sp, zp;
    sig_pair(fmaf(t, xv, b), m > 0.f, sp, zp);
    const float gv = sc * zp;
    ls += sp;
    gx += gv * xv;
    zs += zp;
    if (dx) dx[i] = gv;
  }
  ls = egv_block_sum_256(ls, sh);
  gx = egv_block_sum_256(gx, sh);
  zs = egv_block_sum_256(zs, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ls;
    part[gridDim.x + blockIdx.x] = gx;
    part[2 * gridDim.x + blockIdx.x] = zs;
  }
}

// grad: with the second product (gpart); sums: with the loss, scale and bias partials (lpart).  A walk with neither has no output.
template <int DP>
int sig_launch_walk(const SigLayout& L, bool grad, bool sums, const float* A, const float* B, const uint32_t* words, int n, int mode,
                    const float* logit_scale, const float* logit_bias, float* gpart, float* lpart, hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4;
  if (!grad && !sums) return EGV_ERR_ARG;
  auto k = !grad ? sig_walk_kernel<DP, false, true> : sums ? sig_walk_kernel<DP, true, true> : sig_walk_kernel<DP, true, false>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns), dim3(256), lds, s, A, B, words, n, L.np, L.W, L.wn, mode, logit_scale, logit_bias, L.tps,
             gpart, lpart);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

}  // namespace

extern "C" int64_t egv_sigmoid_head_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv) {
  if (!egl_args_ok(n, D, dn, dv)) return 0;
  return sig_layout(n, D, dn, dv).total;
}

extern "C" int egv_sigmoid_head_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                        int32_t D, int32_t dn, int32_t dv, const float* logit_scale, const float* logit_bias,
                                        float eps, int32_t use_noun, int32_t use_verb, float* loss, float* d_text, float* d_video,
                                        float* d_scale, float* d_bias, float* work, void* stream) {
  if (!text || !video || !loss || !work || !logit_scale || !logit_bias) return EGV_ERR_ARG;
  if ((noun != nullptr) != (verb != nullptr)) return EGV_ERR_ARG;
  // the embedding gradients come together, the parameter gradients come together, and the latter ride on the former's walk
  if ((d_text != nullptr) != (d_video != nullptr) || (d_scale != nullptr) != (d_bias != nullptr) || (d_scale && !d_text))
    return EGV_ERR_ARG;
  if (!noun) dn = dv = 0;
  if (!egl_args_ok(n, D, dn, dv)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const SigLayout L = sig_layout(n, D, dn, dv);
  float* tn = work + L.tn;
  float* vn = work + L.vn;
  const uint32_t* words = (const uint32_t*)(work + L.words);
  const float* norms = work + L.norms;
  const float* flags = work + L.flags;
  float* gpart = work + L.gpart;
  float* lpart = work + L.lpart;
  const int mode = egl_mask_mode(noun, use_noun, use_verb);

  int rc = egl_launch_prep(L, text, video, noun, verb, n, D, dn, dv, eps, work, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_DP(sig_launch_walk, L, d_text != nullptr, true, tn, vn, words, n, mode, logit_scale, logit_bias,
                 d_text ? gpart : nullptr, lpart, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(sig_reduce_kernel, dim3(1), dim3(256), 0, s, lpart, L.ns * L.ntiles, n, flags, loss, d_scale, d_bias);
  EGV_CHECK_LAUNCH();
  if (d_text) {
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns, tn, norms, L.np, D, L.Dp, eps, d_text);
    EGV_CHECK_LAUNCH();
    rc = EGL_BY_DP(sig_launch_walk, L, true, false, vn, tn, words, n, mode, logit_scale, logit_bias, gpart, nullptr, s);
    if (rc != EGV_OK) return rc;
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns, vn, norms + L.np, L.np, D, L.Dp, eps, d_video);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_sigmoid_from_sim(const float* x, const float* sim_v, const float* sim_n, int32_t n, const float* logit_scale,
                                    const float* logit_bias, int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                                    float* d_scale, float* d_bias, float* work /* 3072 floats */, void* stream) {
  if (!x || !loss || !work || !logit_scale || !logit_bias || n <= 0 || n > 4096) return EGV_ERR_ARG;
  if ((d_scale != nullptr) != (d_bias != nullptr) || (d_scale && !dx)) return EGV_ERR_ARG;
  if (sim_v || sim_n) {                               // the matrices the mask's mode reads
    if ((use_noun && !sim_n) || ((use_verb || !use_noun) && !sim_v)) return EGV_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const long nn = (long)n * n;
  const int blocks = (int)((nn + 1023) / 1024 < SIG_SIM_BLOCKS ? (nn + 1023) / 1024 : SIG_SIM_BLOCKS);
  EGV_LAUNCH(sig_from_sim_kernel, dim3(blocks), dim3(256), 0, s, x, sim_v, sim_n, n, use_noun, use_verb, logit_scale, logit_bias,
             dx, work);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(sig_reduce_kernel, dim3(1), dim3(256), 0, s, work, blocks, n, (const float*)nullptr, loss, d_scale, d_bias);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
