// Contrastive head for global batches past the 1 024 rows of egonce.hip: the same loss and the same gradients
// (the formulas at the top of egonce.hip), with nothing of size n x n in memory.  The similarity tile X = A_I . B_J^T is formed on
// the fp32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit an fp32 fma chain, so the numerics are those of the fp32 short head), the EgoNCE
// mask comes from bit-packed noun / verb rows, and the row statistics are kept online while the column tiles stream through
// LDS.  All arithmetic fp32; every reduction runs in a fixed order (no float atomics), so a call is deterministic.
// The pieces the sigmoid head (sigmoid_head.hip) shares -- prep, the LDS tile, the mask tile, the X^T product, the split and finish --
// live in egonce_tile.h.
//
//   prep    one workgroup per row: |t|, |v|, the normalised rows tn / vn zero-padded from D to Dp (64 or 256), and the
//           noun / verb rows packed into bit words (bit = entry > 0; each part padded to a multiple of 4 words).  Rows
//           n .. np - 1 (np = n rounded up to 64) are written as zeros, so no tile load needs a bound.  A negative or NaN
//           noun / verb entry sets the row's flag; the loss kernel turns any flag into a NaN loss (no host sync).
//   stats   workgroup = (64 rows of A, a range of 64-row tiles of B); a wave owns 16 rows and keeps their operand in
//           registers.  Per tile: X^T fragments, the 64 x 64 mask tile from AND / OR of the packed words, and per lane the
//           running maximum, Z = sum a and P = sum m a, rescaled online.  Launched twice: (tn, vn) gives the row statistics
//           of the loss; (vn, tn) gives the column statistics, because the mask is symmetric:
//             m_ij = (rows i, j share a noun AND share a verb) OR i == j        (use_noun only: share a noun; else verb)
//           which under the data contract -- noun / verb are non-negative multi-hots -- is sim_v * sim_n + I > 0.
//   loss    one workgroup: merges the column-range partials of both directions in a fixed order, writes the final statistics
//           and sums the n loss terms in double.
//   grad    the stats walk again; G_IJ = -1/(n tau) [m a_r / P_i - a_r / Z_i + m a_c / Q_j - a_c / C_j] is formed in the
//           registers of the X^T fragment, which IS the operand layout of the next product (lane = row i, lane group = k),
//           so dA_I += G_IJ . B_J runs on the same MFMA with B_J read from the LDS tile.  Launched twice with the roles
//           swapped; raw partials per column range go to the workspace.
//   finish  one workgroup per row: sums the partials in a fixed order and applies the backward of the normalisation
//           (egv_norm_bwd).
//   scale   learnable temperature only (egv_egonce_long_fwd_bwd_ls: 1 / tau = exp(s) read from the device by every kernel above):
//           dL/ds = sum_ij G_ij X_ij.  In the grad walk with roles (tn, vn) the X^T fragment and G_IJ sit in the same registers, so
//           each lane accumulates G X (masked exactly like G), the workgroup reduces and stores ONE partial per (row tile, column
//           range); one workgroup adds the partials in a fixed order in double.  The swapped walk would give the same number and
//           is not used.  The loss kernel runs BEFORE the walk, so this sum is a launch of its own, of the same shape.
//
// k order.  The 16x16x4 MFMA takes k = lane >> 4 from each lane.  A lane reads FOUR consecutive floats (one 16-byte LDS read)
// and feeds element t to MFMA t, so MFMA t of chunk c sums k = 16 c + 4 (lane >> 4) + t; both operands use the same map, which
// only permutes the order of the fma chain.  The second product uses the same trick on the OUTPUT column: MFMA t of a 64-wide
// chunk produces d = 64 c + 4 (lane & 15) + t, so a lane ends with four consecutive d and stores 16 bytes.
#define EGV_SCALE_GRAD_KERNEL
#include "egonce_tile.h"
#include "egovlp_hip.h"

namespace {

constexpr int EGL_STAT_WGS = 512;     // column ranges are chosen so that a launch has about this many workgroups (2 per CU)
constexpr float EGL_NEG = -3e38f;

struct EglLayout : EglPrepLayout {
  int tps_s, ns_s, tps_g, ns_g;
  long spart, stat, gpart, lpart;   // offsets in floats, behind the prep outputs
};

inline EglLayout egl_layout(int n, int D, int dn, int dv) {
  EglLayout L{egl_prep_layout(n, D, dn, dv)};
  egl_split(L.ntiles, EGL_STAT_WGS, L.tps_s, L.ns_s);
  egl_split(L.ntiles, EGL_GRAD_WGS, L.tps_g, L.ns_g);
  const long np = L.np;
  long o = L.total;
  L.spart = o;  o += 2L * L.ns_s * 3 * np;
  L.stat = o;   o += 6 * np;
  L.gpart = o;  o += (long)L.ns_g * np * L.Dp;
  L.lpart = o;  o += (long)L.ns_g * L.ntiles;          // dL/d(logit scale): one partial per workgroup of the grad walk
  L.total = o;
  return L;
}

// ------------------------------------------------------------------------------------------------ statistics
template <int DP>
__global__ __launch_bounds__(256, 2) void egl_stats_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                           const uint32_t* __restrict__ words, int n, int np, int W, int wn,
                                                           int mode, float inv_tau,
                                                           const float* __restrict__ logit_scale, int tps,
                                                           float* __restrict__ part /* [ranges][3][np] */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LD = DP + 4;
  float* bt = (float*)smem;
  uint32_t* mb = (uint32_t*)(bt + EGL_TILE * LD);
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * EGL_TILE;
  const int ntiles = np / EGL_TILE;
  const int t0 = blockIdx.y * tps, t1 = min(ntiles, t0 + tps);
  const int gi = i0 + wave * 16 + li;

  f32x4_t a[DP / 16];
#pragma unroll
  for (int c = 0; c < DP / 16; ++c) a[c] = *(const f32x4_t*)(A + (long)gi * DP + 16 * c + 4 * g);

  float m = EGL_NEG, Z = 0.f, P = 0.f;                // this lane's share of row gi: the columns 16 jf + 4 g + r of every tile
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const int j0 = t * EGL_TILE;
    __syncthreads();                                  // every wave is done with the previous tile
    egl_stage_tile<DP>(bt, B, j0);
    egl_mask_tile(words, W, wn, mode, i0, j0, mb);
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    float cm = EGL_NEG;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + jf * 16 + 4 * g + r < n) cm = fmaxf(cm, x[jf][r]);
    const float mn = fmaxf(m, cm);
    const float alpha = __expf((m - mn) * inv_tau);   // first tile: exp(-inf) = 0 and Z, P are 0 anyway
    float zs = 0.f, ps = 0.f;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (j0 + jf * 16 + 4 * g + r < n) ? __expf((x[jf][r] - mn) * inv_tau) : 0.f;
        zs += e;
        ps += ((mbits[jf] >> (4 * g + r)) & 1u) ? e : 0.f;
      }
    Z = Z * alpha + zs;
    P = P * alpha + ps;
    m = mn;
  }
  // the four lane groups of a row
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float mo = __shfl_xor(m, off, 64), Zo = __shfl_xor(Z, off, 64), Po = __shfl_xor(P, off, 64);
    const float M = fmaxf(m, mo);
    const float s1 = __expf((m - M) * inv_tau), s2 = __expf((mo - M) * inv_tau);
    Z = Z * s1 + Zo * s2;
    P = P * s1 + Po * s2;
    m = M;
  }
  if (g == 0 && gi < n) {
    float* p = part + (long)blockIdx.y * 3 * np;
    p[gi] = m;
    p[np + gi] = Z;
    p[2 * np + gi] = P;
  }
}

// ------------------------------------------------------------------------------------------------ loss
__global__ __launch_bounds__(1024) void egl_loss_kernel(const float* __restrict__ spart /* [2][ranges][3][np] */, int ns, int n,
                                                        int np, float inv_tau, const float* __restrict__ logit_scale,
                                                        const float* __restrict__ flags,
                                                        float* __restrict__ stat /* [2][3][np] */, float* __restrict__ loss) {
  __shared__ double red[1024];
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  double s = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    float term = 0.f;
    for (int dir = 0; dir < 2; ++dir) {
      const float* p = spart + (long)dir * ns * 3 * np;
      float M = EGL_NEG;
      for (int r = 0; r < ns; ++r) M = fmaxf(M, p[(long)r * 3 * np + i]);
      float Z = 0.f, P = 0.f;
      for (int r = 0; r < ns; ++r) {
        const float w = __expf((p[(long)r * 3 * np + i] - M) * inv_tau);
        Z += p[((long)r * 3 + 1) * np + i] * w;
        P += p[((long)r * 3 + 2) * np + i] * w;
      }
      float* o = stat + (long)dir * 3 * np;
      o[i] = M;
      o[np + i] = Z;
      o[2 * np + i] = P;
      term += __logf(P) - __logf(Z);
    }
    s += (double)term;
    bad |= flags[i] != 0.f;
  }
  red[threadIdx.x] = s;
  bad = __syncthreads_or(bad);
  for (int h = 512; h >= 1; h >>= 1) {                // pairwise, fixed order
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = bad ? __builtin_nanf("") : (float)(-red[0] / (double)n);
}

// ------------------------------------------------------------------------------------------------ gradient
template <int DP>
__global__ __launch_bounds__(256, 2) void egl_grad_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const uint32_t* __restrict__ words,
                                                          const float* __restrict__ own /* [3][np]: statistics of A's rows */,
                                                          const float* __restrict__ oth /* [3][np]: of B's rows */, int n,
                                                          int np, int W, int wn, int mode, float inv_tau, float sc,
                                                          const float* __restrict__ logit_scale, int tps,
                                                          float* __restrict__ gpart /* [ranges][np][DP] */,
                                                          float* __restrict__ lpart /* [ranges][tiles] or NULL */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sh[4];
  constexpr int LD = DP + 4;
  float* bt = (float*)smem;
  uint32_t* mb = (uint32_t*)(bt + EGL_TILE * LD);
  float* cs = (float*)(mb + EGL_TILE * 4);            // [3][64]: max, 1 / Z, 1 / P of the tile's B rows
  if (logit_scale) {                                  // uniform
    inv_tau = expf(logit_scale[0]);
    sc = -inv_tau / (float)n;
  }
  float gx = 0.f;                                     // this lane's share of sum G X
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * EGL_TILE;
  const int ntiles = np / EGL_TILE;
  const int t0 = blockIdx.y * tps, t1 = min(ntiles, t0 + tps);
  const int gi = i0 + wave * 16 + li;

  f32x4_t a[DP / 16];
#pragma unroll
  for (int c = 0; c < DP / 16; ++c) a[c] = *(const f32x4_t*)(A + (long)gi * DP + 16 * c + 4 * g);
  const bool live = gi < n;
  const float mo = live ? own[gi] : 0.f;
  const float izo = live ? 1.0f / own[np + gi] : 0.f;
  const float ipo = live ? 1.0f / own[2 * np + gi] : 0.f;

  f32x4_t acc[DP / 64][4];
#pragma unroll
  for (int c = 0; c < DP / 64; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[c][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const int j0 = t * EGL_TILE;
    __syncthreads();
    egl_stage_tile<DP>(bt, B, j0);
    egl_mask_tile(words, W, wn, mode, i0, j0, mb);
    if (threadIdx.x < EGL_TILE) {
      const int gj = j0 + threadIdx.x;
      const bool ok = gj < n;
      cs[threadIdx.x] = ok ? oth[gj] : 0.f;
      cs[64 + threadIdx.x] = ok ? 1.0f / oth[np + gj] : 0.f;
      cs[128 + threadIdx.x] = ok ? 1.0f / oth[2 * np + gj] : 0.f;
    }
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
#pragma unroll
    for (int jf = 0; jf < 4; ++jf) {
      const f32x4_t cm4 = *(const f32x4_t*)(cs + jf * 16 + 4 * g);
      const f32x4_t iz4 = *(const f32x4_t*)(cs + 64 + jf * 16 + 4 * g);
      const f32x4_t ip4 = *(const f32x4_t*)(cs + 128 + jf * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xv = x[jf][r];
        const float eo = __expf((xv - mo) * inv_tau);         // under the maximum of A's row
        const float ec = __expf((xv - cm4[r]) * inv_tau);     // under the maximum of B's row
        const float mm = ((mbits[jf] >> (4 * g + r)) & 1u) ? 1.f : 0.f;
        const float gv = sc * (eo * (mm * ipo - izo) + ec * (mm * ip4[r] - iz4[r]));
        const float gm = (live && j0 + jf * 16 + 4 * g + r < n) ? gv : 0.f;
        gx += gm * xv;
        x[jf][r] = gm;
      }
    }
    // dA[i][d] += sum_j G[i][j] B[j][d]: x[jf][r] is the A operand of k-step (jf, r) as it stands (k = j = 16 jf + 4 g + r)
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < DP / 64; ++c) {
          const f32x4_t bv = *(const f32x4_t*)(bt + (jf * 16 + 4 * g + r) * LD + 64 * c + 4 * li);
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc[c][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[jf][r], bv[tt], acc[c][tt], 0, 0, 0);
        }
  }
  // acc[c][tt][rr]: row i0 + 16 wave + 4 g + rr, column 64 c + 4 li + tt
  float* out = gpart + ((long)blockIdx.y * np + i0 + wave * 16 + 4 * g) * DP + 4 * li;
#pragma unroll
  for (int c = 0; c < DP / 64; ++c)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      *(f32x4_t*)(out + (long)rr * DP + 64 * c) = (f32x4_t){acc[c][0][rr], acc[c][1][rr], acc[c][2][rr], acc[c][3][rr]};
  if (lpart) {                                        // uniform over the workgroup
    gx = egv_block_sum_256(gx, sh);
    if (threadIdx.x == 0) lpart[(long)blockIdx.y * ntiles + blockIdx.x] = gx;
  }
}

template <int DP>
int egl_launch_stats(const EglLayout& L, const float* A, const float* B, const uint32_t* words, int n, int mode, float inv_tau,
                     const float* logit_scale, float* part, hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4;
  auto k = egl_stats_kernel<DP>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_s), dim3(256), lds, s, A, B, words, n, L.np, L.W, L.wn, mode, inv_tau, logit_scale, L.tps_s,
             part);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

template <int DP>
int egl_launch_grad(const EglLayout& L, const float* A, const float* B, const uint32_t* words, const float* own,
                    const float* oth, int n, int mode, float inv_tau, const float* logit_scale, float* gpart, float* lpart,
                    hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4 + 3 * EGL_TILE * 4;
  auto k = egl_grad_kernel<DP>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_g), dim3(256), lds, s, A, B, words, own, oth, n, L.np, L.W, L.wn, mode, inv_tau,
             -inv_tau / (float)n, logit_scale, L.tps_g, gpart, lpart);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

}  // namespace

extern "C" int64_t egv_egonce_long_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv) {
  if (!egl_args_ok(n, D, dn, dv)) return 0;
  return egl_layout(n, D, dn, dv).total;
}

// the long head; logit_scale != NULL: 1 / tau = exp(*logit_scale) on the device (inv_tau unused) and, with d_text, *d_logit_scale
static int egl_head(const float* text, const float* video, const float* noun, const float* verb, int32_t n, int32_t D, int32_t dn,
                    int32_t dv, float inv_tau, const float* logit_scale, float eps, int32_t use_noun, int32_t use_verb,
                    float* loss, float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream) {
  if (!text || !video || !loss || !work) return EGV_ERR_ARG;
  if ((noun != nullptr) != (verb != nullptr)) return EGV_ERR_ARG;
  if (!noun) dn = dv = 0;
  if (!egl_args_ok(n, D, dn, dv)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const EglLayout L = egl_layout(n, D, dn, dv);
  float* tn = work + L.tn;
  float* vn = work + L.vn;
  const uint32_t* words = (const uint32_t*)(work + L.words);
  const float* norms = work + L.norms;
  const float* flags = work + L.flags;
  float* spart = work + L.spart;
  float* stat = work + L.stat;
  float* gpart = work + L.gpart;
  float* lpart = d_logit_scale ? work + L.lpart : nullptr;
  const int mode = egl_mask_mode(noun, use_noun, use_verb);
  const long np = L.np;

  int rc = egl_launch_prep(L, text, video, noun, verb, n, D, dn, dv, eps, work, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_DP(egl_launch_stats, L, tn, vn, words, n, mode, inv_tau, logit_scale, spart, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_DP(egl_launch_stats, L, vn, tn, words, n, mode, inv_tau, logit_scale,
                  spart + (long)L.ns_s * 3 * np, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(egl_loss_kernel, dim3(1), dim3(1024), 0, s, spart, L.ns_s, n, L.np, inv_tau, logit_scale, flags, stat, loss);
  EGV_CHECK_LAUNCH();
  if (d_text) {
    rc = EGL_BY_DP(egl_launch_grad, L, tn, vn, words, stat, stat + 3 * np, n, mode, inv_tau, logit_scale, gpart, lpart, s);
    if (rc != EGV_OK) return rc;
    if (lpart) {
      EGV_LAUNCH(egv_scale_grad_kernel, dim3(1), dim3(256), 0, s, lpart, L.ns_g * L.ntiles, d_logit_scale);
      EGV_CHECK_LAUNCH();
    }
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, tn, norms, L.np, D, L.Dp, eps, d_text);
    EGV_CHECK_LAUNCH();
  }
  if (d_video) {
    rc = EGL_BY_DP(egl_launch_grad, L, vn, tn, words, stat + 3 * np, stat, n, mode, inv_tau, logit_scale, gpart,
                   nullptr, s);
    if (rc != EGV_OK) return rc;
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, vn, norms + np, L.np, D, L.Dp, eps, d_video);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_egonce_long_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                       int32_t D, int32_t dn, int32_t dv, float temperature, float eps, int32_t use_noun,
                                       int32_t use_verb, float* loss, float* d_text, float* d_video, float* work,
                                       void* stream) {
  if (!(temperature > 0.f)) return EGV_ERR_ARG;
  return egl_head(text, video, noun, verb, n, D, dn, dv, 1.0f / temperature, nullptr, eps, use_noun, use_verb, loss, d_text,
                  d_video, nullptr, work, stream);
}

extern "C" int egv_egonce_long_fwd_bwd_ls(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                          int32_t D, int32_t dn, int32_t dv, const float* logit_scale, float eps,
                                          int32_t use_noun, int32_t use_verb, float* loss, float* d_text, float* d_video,
                                          float* d_logit_scale, float* work, void* stream) {
  if (!logit_scale) return EGV_ERR_ARG;
  // the scale's gradient comes out of the (tn, vn) walk: it needs d_text
  if ((d_text || d_video) && !(d_text && d_logit_scale)) return EGV_ERR_ARG;
  return egl_head(text, video, noun, verb, n, D, dn, dv, 0.f, logit_scale, eps, use_noun, use_verb, loss, d_text, d_video,
                  d_text ? d_logit_scale : nullptr, work, stream);
}
