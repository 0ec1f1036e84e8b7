// Contrastive head: sim_matrix (x3) + EgoNCE / NormSoftmaxLoss, forward AND analytic backward.
//   model/model.py:189-197 (sim_matrix), model/loss.py:13-25 (NormSoftmaxLoss), :34-53 (EgoNCE),
//   trainer/trainer_egoclip.py:130-137 (the three sim_matrix calls feeding the loss).
// The whole problem is n = W*B <= 1024 rows (256 at 8 GPUs x 32): latency-bound, not throughput-bound,
// so the design goal is few launches and no host round trip: 5 small kernels replace the ~40 ATen
// launches + autograd graph of the reference, and the gradient w.r.t. both embeddings comes out of
// the same call.  All arithmetic fp32.
//   x_ij   = <t_i/max(|t_i|,eps), v_j/max(|v_j|,eps)>
//   m_ij   = (simv_ij * simn_ij + [i==j]) > 0                       (EgoNCE, noun & verb)
//   loss   = -1/n sum_i [log sum_j m_ij a_ij - log sum_j a_ij]      a_ij = exp(x_ij / tau)
//            -1/n sum_i [log sum_j m_ij a_ji - log sum_j a_ji]
// Learnable temperature (the *_ls entry points): 1 / tau = exp(s) is read from the device, and with G = dL/dx
//   dL/ds  = sum_ij G_ij x_ij                                       s = log(1 / tau)
// falls out of the gradient kernel, which holds x_ij and G_ij: one block_sum per row into n partials, then one
// workgroup adds them in a fixed order in double.  No float atomics: two calls give the same bits.
#include "common.h"
#include "egovlp_hip.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* sh) {  // 256 threads
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// A: per row i: clamped norms + normalised text / video rows
__global__ __launch_bounds__(256) void egonce_norm_kernel(const float* __restrict__ text, const float* __restrict__ video,
                                                          const float* __restrict__ noun, const float* __restrict__ verb,
                                                          int n, int D, int dn, int dv, float eps,
                                                          float* __restrict__ tn, float* __restrict__ vn,
                                                          float* __restrict__ stats /* [4][n]: |t|,|v|,|noun|c,|verb|c */) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  float st = 0.f, sv = 0.f, sn = 0.f, sb = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float a = text[(long)i * D + d], b = video[(long)i * D + d];
    st += a * a;
    sv += b * b;
  }
  if (noun)
    for (int d = threadIdx.x; d < dn; d += 256) {
      const float a = noun[(long)i * dn + d];
      sn += a * a;
    }
  if (verb)
    for (int d = threadIdx.x; d < dv; d += 256) {
      const float a = verb[(long)i * dv + d];
      sb += a * a;
    }
  const float nt = sqrtf(block_sum(st, sh));
  const float nv = sqrtf(block_sum(sv, sh));
  const float nno = sqrtf(block_sum(sn, sh));
  const float nve = sqrtf(block_sum(sb, sh));
  const float ct = fmaxf(nt, eps), cv = fmaxf(nv, eps);
  for (int d = threadIdx.x; d < D; d += 256) {
    tn[(long)i * D + d] = text[(long)i * D + d] / ct;
    vn[(long)i * D + d] = video[(long)i * D + d] / cv;
  }
  if (threadIdx.x == 0) {
    stats[0 * n + i] = nt;
    stats[1 * n + i] = nv;
    stats[2 * n + i] = fmaxf(nno, eps);
    stats[3 * n + i] = fmaxf(nve, eps);
  }
}

// B: row i of x and of the mask; row statistics rmax_i, Z_i, P_i
__global__ __launch_bounds__(256) void egonce_rows_kernel(const float* __restrict__ tn, const float* __restrict__ vn,
                                                          const float* __restrict__ noun, const float* __restrict__ verb,
                                                          const float* __restrict__ stats, int n, int D, int dn, int dv,
                                                          float inv_tau, int use_noun, int use_verb,
                                                          float* __restrict__ x, float* __restrict__ mask,
                                                          float* __restrict__ rstat /* [3][n] */) {
  extern __shared__ float rowbuf[];  // [D + dn + dv]
  __shared__ float sh[4];
  const int i = blockIdx.x;
  float* ti = rowbuf;
  float* ni = rowbuf + D;
  float* bi = ni + dn;
  for (int d = threadIdx.x; d < D; d += 256) ti[d] = tn[(long)i * D + d];
  if (noun)
    for (int d = threadIdx.x; d < dn; d += 256) ni[d] = noun[(long)i * dn + d];
  if (verb)
    for (int d = threadIdx.x; d < dv; d += 256) bi[d] = verb[(long)i * dv + d];
  __syncthreads();
  float lmax = -3e38f;
  for (int j = threadIdx.x; j < n; j += 256) {
    float acc = 0.f;
    const float* vj = vn + (long)j * D;
    for (int d = 0; d < D; d += 4) {
      const f32x4_t b = *(const f32x4_t*)(vj + d);
      acc += ti[d] * b[0] + ti[d + 1] * b[1] + ti[d + 2] * b[2] + ti[d + 3] * b[3];
    }
    float m = (i == j) ? 1.f : 0.f;
    if (noun || verb) {
      float sn = 0.f, sv = 0.f;
      if (noun && use_noun) {
        const float* nj = noun + (long)j * dn;
        for (int d = 0; d < dn; ++d) sn += ni[d] * nj[d];
        sn = (sn / stats[2 * n + i]) / stats[2 * n + j];
      }
      if (verb && use_verb) {
        const float* bj = verb + (long)j * dv;
        for (int d = 0; d < dv; ++d) sv += bi[d] * bj[d];
        sv = (sv / stats[3 * n + i]) / stats[3 * n + j];
      }
      float mm;
      if (use_noun && use_verb) mm = sv * sn + m;   // loss.py:36-37
      else if (use_noun) mm = sn + m;               // :38-39
      else mm = sv + m;                             // :40-41
      m = mm > 0.f ? 1.f : 0.f;                     // :47
    }
    x[(long)i * n + j] = acc;
    mask[(long)i * n + j] = m;
    lmax = fmaxf(lmax, acc);
  }
}

// B2: row statistics rmax_i, Z_i = sum_j a_ij, P_i = sum_j m_ij a_ij
__global__ __launch_bounds__(256) void egonce_rowstat_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                             int n, float inv_tau, const float* __restrict__ logit_scale,
                                                             float* __restrict__ rstat) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  float lmax = -3e38f;
  for (int j = threadIdx.x; j < n; j += 256) lmax = fmaxf(lmax, x[(long)i * n + j]);
  const float rmax = block_max(lmax, sh);
  float z = 0.f, p = 0.f;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float a = __expf((x[(long)i * n + j] - rmax) * inv_tau);
    z += a;
    p += a * mask[(long)i * n + j];
  }
  z = block_sum(z, sh);
  p = block_sum(p, sh);
  if (threadIdx.x == 0) {
    rstat[0 * n + i] = rmax;
    rstat[1 * n + i] = z;
    rstat[2 * n + i] = p;
  }
}

// mask from precomputed similarity matrices (API-compatible EgoNCE.forward(x, mask_v, mask_n), loss.py:34-47)
__global__ __launch_bounds__(256) void egonce_mask_from_sim_kernel(const float* __restrict__ sim_v,
                                                                   const float* __restrict__ sim_n, int n, int use_noun,
                                                                   int use_verb, float* __restrict__ mask) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * n) return;
  const float d = (i / n == i % n) ? 1.f : 0.f;
  float m = d;
  if (sim_v || sim_n) {
    if (use_noun && use_verb) m = sim_v[i] * sim_n[i] + d;
    else if (use_noun) m = sim_n[i] + d;
    else m = sim_v[i] + d;
  }
  mask[i] = m > 0.f ? 1.f : 0.f;
}

// generic sim_matrix pieces: row normalisation, C = An . Bn^T, and the backward through both
__global__ __launch_bounds__(256) void rownorm_kernel(const float* __restrict__ a, int D, float eps,
                                                      float* __restrict__ an, float* __restrict__ norms) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float v = a[(long)i * D + d];
    s += v * v;
  }
  const float nrm = sqrtf(block_sum(s, sh));
  const float c = fmaxf(nrm, eps);
  for (int d = threadIdx.x; d < D; d += 256) an[(long)i * D + d] = a[(long)i * D + d] / c;
  if (threadIdx.x == 0) norms[i] = nrm;
}
__global__ __launch_bounds__(256) void dot_nt_kernel(const float* __restrict__ an, const float* __restrict__ bn, int m,
                                                     int D, float* __restrict__ out) {
  extern __shared__ float rowbuf[];
  const int i = blockIdx.x;
  for (int d = threadIdx.x; d < D; d += 256) rowbuf[d] = an[(long)i * D + d];
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += 256) {
    const float* bj = bn + (long)j * D;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc += rowbuf[d] * bj[d];
    out[(long)i * m + j] = acc;
  }
}
// d_a[i,:] = normalisation-backward( sum_j G[i,j] (or G[j,i] if transposed) * bn[j,:] )
__global__ __launch_bounds__(256) void sim_bwd_kernel(const float* __restrict__ G, int transposed, int rows, int cols,
                                                      const float* __restrict__ an, const float* __restrict__ bn,
                                                      const float* __restrict__ norms, int D, float eps,
                                                      float* __restrict__ da) {
  __shared__ float sh[4];
  const int i = blockIdx.x;  // row of a (rows of them); sums over `cols` rows of b
  const float nrm = norms[i];
  float proj = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    float g = 0.f;
    for (int j = 0; j < cols; ++j) {
      const float gij = transposed ? G[(long)j * rows + i] : G[(long)i * cols + j];
      g += gij * bn[(long)j * D + d];
    }
    da[(long)i * D + d] = g;  // stash the raw gradient w.r.t. the normalised row
    proj += g * an[(long)i * D + d];
  }
  proj = block_sum(proj, sh);
  for (int d = threadIdx.x; d < D; d += 256) {
    const float g = da[(long)i * D + d];
    da[(long)i * D + d] = nrm > eps ? (g - an[(long)i * D + d] * proj) / nrm : g / eps;
  }
}

// C: column statistics for column c: cmax_c, C_c = sum_r a_rc, Q_c = sum_r m_cr a_rc
__global__ __launch_bounds__(256) void egonce_cols_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                          int n, float inv_tau, const float* __restrict__ logit_scale,
                                                          float* __restrict__ cstat /* [3][n] */) {
  __shared__ float sh[4];
  const int c = blockIdx.x;
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  float lmax = -3e38f;
  for (int r = threadIdx.x; r < n; r += 256) lmax = fmaxf(lmax, x[(long)r * n + c]);
  const float cmax = block_max(lmax, sh);
  float s = 0.f, q = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) {
    const float a = __expf((x[(long)r * n + c] - cmax) * inv_tau);
    s += a;
    q += a * mask[(long)c * n + r];
  }
  s = block_sum(s, sh);
  q = block_sum(q, sh);
  if (threadIdx.x == 0) {
    cstat[0 * n + c] = cmax;
    cstat[1 * n + c] = s;
    cstat[2 * n + c] = q;
  }
}

// D: G_ij = dL/dx_ij (row i per block); ls_part[i] = sum_j G_ij x_ij, row i's share of dL/d(logit scale), when asked for
__global__ __launch_bounds__(256) void egonce_grad_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                          const float* __restrict__ rstat, const float* __restrict__ cstat,
                                                          int n, float inv_tau, const float* __restrict__ logit_scale,
                                                          float* __restrict__ G, float* __restrict__ ls_part) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  float gx = 0.f;
  const float rmax = rstat[i], Zi = rstat[n + i], Pi = rstat[2 * n + i];
  const float sc = -inv_tau / (float)n;
  for (int j = threadIdx.x; j < n; j += 256) {
    const float xv = x[(long)i * n + j];
    const float ar = __expf((xv - rmax) * inv_tau);             // row-normalised numerator
    const float ac = __expf((xv - cstat[j]) * inv_tau);         // column-normalised numerator
    const float g_row = mask[(long)i * n + j] * ar / Pi - ar / Zi;
    const float g_col = mask[(long)j * n + i] * ac / cstat[2 * n + j] - ac / cstat[n + j];
    const float g = sc * (g_row + g_col);
    G[(long)i * n + j] = g;
    gx += g * xv;
  }
  if (ls_part) {                                                  // uniform over the workgroup
    gx = block_sum(gx, sh);
    if (threadIdx.x == 0) ls_part[i] = gx;
  }
}

// dL/d(logit scale) = sum of the n row partials; one workgroup, double, fixed order
__global__ __launch_bounds__(256) void egonce_scale_grad_kernel(const float* __restrict__ ls_part, int n,
                                                                float* __restrict__ d_logit_scale) {
  __shared__ double red[256];
  const double s = egv_sum_partials_256(ls_part, n, red);
  if (threadIdx.x == 0) d_logit_scale[0] = (float)s;
}

// E: loss scalar + embedding gradients.  Block i, thread d.
__global__ __launch_bounds__(256) void egonce_embgrad_kernel(const float* __restrict__ G, const float* __restrict__ tn,
                                                             const float* __restrict__ vn,
                                                             const float* __restrict__ stats, int n, int D, float eps,
                                                             float* __restrict__ d_text, float* __restrict__ d_video) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  const float nt = stats[i], nv = stats[n + i];
  for (int d0 = 0; d0 < D; d0 += 256) {
    const int d = d0 + threadIdx.x;
    float gt = 0.f, gv = 0.f;
    if (d < D) {
      for (int j = 0; j < n; ++j) {
        gt += G[(long)i * n + j] * vn[(long)j * D + d];
        gv += G[(long)j * n + i] * tn[(long)j * D + d];
      }
    }
    // D <= 256 in the hot path; for larger D the projection term needs a full-row dot, handled below
    if (D <= 256) {
      const float th = d < D ? tn[(long)i * D + d] : 0.f;
      const float vh = d < D ? vn[(long)i * D + d] : 0.f;
      const float pt = block_sum(th * gt, sh);
      const float pv = block_sum(vh * gv, sh);
      if (d < D) {
        if (d_text) d_text[(long)i * D + d] = nt > eps ? (gt - th * pt) / nt : gt / eps;
        if (d_video) d_video[(long)i * D + d] = nv > eps ? (gv - vh * pv) / nv : gv / eps;
      }
    }
  }
}

__global__ __launch_bounds__(256) void egonce_loss_kernel(const float* __restrict__ rstat, const float* __restrict__ cstat,
                                                          int n, float* __restrict__ loss) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256)
    s += (__logf(rstat[2 * n + i]) - __logf(rstat[n + i])) + (__logf(cstat[2 * n + i]) - __logf(cstat[n + i]));
  s = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = -s / (float)n;
}

}  // namespace

extern "C" int64_t egv_egonce_work_floats(int32_t n, int32_t D) {
  return 2LL * n * D + 3LL * n * n + 16LL * n;
}

// the short head; logit_scale != NULL: 1 / tau = exp(*logit_scale) on the device and, with the gradients, *d_logit_scale
static int egonce_head(const float* text, const float* video, const float* noun, const float* verb, int32_t n, int32_t D,
                       int32_t dn, int32_t dv, float inv_tau, const float* logit_scale, float eps, int32_t use_noun,
                       int32_t use_verb, float* loss, float* sim, float* d_text, float* d_video, float* d_logit_scale,
                       float* work, void* stream) {
  if (!text || !video || !loss || !work || n <= 0 || n > 1024 || D <= 0 || D > 256 || D % 4 != 0) return EGV_ERR_ARG;
  if ((noun != nullptr) != (verb != nullptr)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* tn = work;
  float* vn = tn + (long)n * D;
  float* x = sim ? sim : vn + (long)n * D;
  float* mask = vn + (long)n * D + (long)n * n;
  float* G = mask + (long)n * n;
  float* stats = G + (long)n * n;  // 4n
  float* rstat = stats + 4 * n;    // 3n
  float* cstat = rstat + 3 * n;    // 3n
  float* ls_part = cstat + 3 * n;  // n (the workspace has 16n behind the matrices)
  EGV_LAUNCH(egonce_norm_kernel, dim3(n), dim3(256), 0, s, text, video, noun, verb, n, D, dn, dv, eps, tn, vn,
                     stats);
  EGV_CHECK_LAUNCH();
  const size_t lds = (size_t)(D + (noun ? dn + dv : 0)) * sizeof(float);
  EGV_LAUNCH(egonce_rows_kernel, dim3(n), dim3(256), lds, s, tn, vn, noun, verb, stats, n, D, dn, dv, inv_tau,
                     use_noun, use_verb, x, mask, rstat);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_rowstat_kernel, dim3(n), dim3(256), 0, s, x, mask, n, inv_tau, logit_scale, rstat);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_cols_kernel, dim3(n), dim3(256), 0, s, x, mask, n, inv_tau, logit_scale, cstat);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_loss_kernel, dim3(1), dim3(256), 0, s, rstat, cstat, n, loss);
  EGV_CHECK_LAUNCH();
  if (d_text || d_video) {
    EGV_LAUNCH(egonce_grad_kernel, dim3(n), dim3(256), 0, s, x, mask, rstat, cstat, n, inv_tau, logit_scale, G,
               d_logit_scale ? ls_part : nullptr);
    EGV_CHECK_LAUNCH();
    if (d_logit_scale) {
      EGV_LAUNCH(egonce_scale_grad_kernel, dim3(1), dim3(256), 0, s, ls_part, n, d_logit_scale);
      EGV_CHECK_LAUNCH();
    }
    EGV_LAUNCH(egonce_embgrad_kernel, dim3(n), dim3(256), 0, s, G, tn, vn, stats, n, D, eps, d_text, d_video);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_egonce_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb,
                                  int32_t n, int32_t D, int32_t dn, int32_t dv, float temperature, float eps,
                                  int32_t use_noun, int32_t use_verb, float* loss, float* sim, float* d_text,
                                  float* d_video, float* work, void* stream) {
  return egonce_head(text, video, noun, verb, n, D, dn, dv, 1.0f / temperature, nullptr, eps, use_noun, use_verb, loss, sim,
                     d_text, d_video, nullptr, work, stream);
}

extern "C" int egv_egonce_fwd_bwd_ls(const float* text, const float* video, const float* noun, const float* verb,
                                     int32_t n, int32_t D, int32_t dn, int32_t dv, const float* logit_scale, float eps,
                                     int32_t use_noun, int32_t use_verb, float* loss, float* sim, float* d_text,
                                     float* d_video, float* d_logit_scale, float* work, void* stream) {
  if (!logit_scale) return EGV_ERR_ARG;
  if ((d_text || d_video) && !d_logit_scale) return EGV_ERR_ARG;
  return egonce_head(text, video, noun, verb, n, D, dn, dv, 0.f, logit_scale, eps, use_noun, use_verb, loss, sim, d_text,
                     d_video, (d_text || d_video) ? d_logit_scale : nullptr, work, stream);
}

// API-compatible pieces -------------------------------------------------------------------------------
extern "C" int egv_sim_matrix_fwd(const float* a, const float* b, int32_t n, int32_t m, int32_t D, float eps,
                                  float* an, float* bn, float* norms /* [n+m] */, float* out, void* stream) {
  if (!a || !b || !an || !bn || !norms || !out || n <= 0 || m <= 0 || D <= 0 || D > 8192) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(rownorm_kernel, dim3(n), dim3(256), 0, s, a, D, eps, an, norms);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(rownorm_kernel, dim3(m), dim3(256), 0, s, b, D, eps, bn, norms + n);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(dot_nt_kernel, dim3(n), dim3(256), (size_t)D * sizeof(float), s, an, bn, m, D, out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_sim_matrix_bwd(const float* g, const float* an, const float* bn, const float* norms, int32_t n,
                                  int32_t m, int32_t D, float eps, float* da, float* db, void* stream) {
  if (!g || !an || !bn || !norms || n <= 0 || m <= 0 || D <= 0) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (da) {
    EGV_LAUNCH(sim_bwd_kernel, dim3(n), dim3(256), 0, s, g, 0, n, m, an, bn, norms, D, eps, da);
    EGV_CHECK_LAUNCH();
  }
  if (db) {
    EGV_LAUNCH(sim_bwd_kernel, dim3(m), dim3(256), 0, s, g, 1, m, n, bn, an, norms + n, D, eps, db);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

static int egonce_from_sim(const float* x, const float* sim_v, const float* sim_n, int32_t n, float inv_tau,
                           const float* logit_scale, int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                           float* d_logit_scale, float* work /* n*n + 6n floats, + n with d_logit_scale */, void* stream) {
  if (!x || !loss || !work || n <= 0 || n > 4096) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* mask = work;
  float* rstat = mask + (long)n * n;
  float* cstat = rstat + 3 * n;
  float* ls_part = cstat + 3 * n;
  const long nn = (long)n * n;
  EGV_LAUNCH(egonce_mask_from_sim_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, sim_v, sim_n, n,
                     use_noun, use_verb, mask);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_rowstat_kernel, dim3(n), dim3(256), 0, s, x, mask, n, inv_tau, logit_scale, rstat);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_cols_kernel, dim3(n), dim3(256), 0, s, x, mask, n, inv_tau, logit_scale, cstat);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egonce_loss_kernel, dim3(1), dim3(256), 0, s, rstat, cstat, n, loss);
  EGV_CHECK_LAUNCH();
  if (dx) {
    EGV_LAUNCH(egonce_grad_kernel, dim3(n), dim3(256), 0, s, x, mask, rstat, cstat, n, inv_tau, logit_scale, dx,
               d_logit_scale ? ls_part : nullptr);
    EGV_CHECK_LAUNCH();
    if (d_logit_scale) {
      EGV_LAUNCH(egonce_scale_grad_kernel, dim3(1), dim3(256), 0, s, ls_part, n, d_logit_scale);
      EGV_CHECK_LAUNCH();
    }
  }
  return EGV_OK;
}

extern "C" int egv_egonce_from_sim(const float* x, const float* sim_v, const float* sim_n, int32_t n,
                                   float temperature, int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                                   float* work /* n*n + 6n floats */, void* stream) {
  return egonce_from_sim(x, sim_v, sim_n, n, 1.0f / temperature, nullptr, use_noun, use_verb, loss, dx, nullptr, work, stream);
}

extern "C" int egv_egonce_from_sim_ls(const float* x, const float* sim_v, const float* sim_n, int32_t n,
                                      const float* logit_scale, int32_t use_noun, int32_t use_verb, float* loss, float* dx,
                                      float* d_logit_scale, float* work /* n*n + 7n floats */, void* stream) {
  if (!logit_scale || (dx && !d_logit_scale)) return EGV_ERR_ARG;
  return egonce_from_sim(x, sim_v, sim_n, n, 0.f, logit_scale, use_noun, use_verb, loss, dx, dx ? d_logit_scale : nullptr, work,
                         stream);
}

// ---- max-margin ranking losses (model/loss.py:55-133; the EPIC-MIR / Charades fine-tuning heads on the same similarity
// matrix) ----------------------------------------------------------------------------------------------------------------
//   loss = mean over the kept (i, j) of  relu(w_i m - x_ii + x_ij) + relu(w_i m - x_ii + x_ji)
// (w_i = 1: MaxMarginRankingLoss; w_i = weight[i]: AdaptiveMaxMarginRankingLoss); fix_norm drops the diagonal pairs, so the
// mean runs over 2 n (n - 1) terms instead of 2 n^2.  The gradient is local in x:
//   d x_ab (a != b) = ( [w_a m - x_aa + x_ab > 0] + [w_b m - x_bb + x_ab > 0] ) / count
//   d x_aa          = - sum_{j != a} ( [w_a m - x_aa + x_aj > 0] + [w_a m - x_aa + x_ja > 0] ) / count
// One workgroup per row a; the loss is accumulated with one atomicAdd per row into a zeroed scalar.
namespace {
__global__ __launch_bounds__(256) void maxmargin_kernel(const float* __restrict__ x, const float* __restrict__ w, int n,
                                                        float margin, int fix_norm, float inv_count,
                                                        float* __restrict__ loss, float* __restrict__ dx) {
  const int a = blockIdx.x;
  const float xaa = x[(long)a * n + a];
  const float ma = (w ? w[a] : 1.0f) * margin;
  float lsum = 0.f, dsum = 0.f;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const float xaj = x[(long)a * n + j], xja = x[(long)j * n + a];
    const float t1 = ma - xaa + xaj, t2 = ma - xaa + xja;
    if (j != a) {
      lsum += fmaxf(t1, 0.f) + fmaxf(t2, 0.f);
      const float i1 = t1 > 0.f ? 1.f : 0.f, i2 = t2 > 0.f ? 1.f : 0.f;
      dsum += i1 + i2;
      if (dx) {
        const float mj = (w ? w[j] : 1.0f) * margin;
        const float t3 = mj - x[(long)j * n + j] + xaj;        // the column-direction term of row j that contains x_aj
        dx[(long)a * n + j] = (i1 + (t3 > 0.f ? 1.f : 0.f)) * inv_count;
      }
    } else if (!fix_norm) {
      lsum += 2.f * fmaxf(ma, 0.f);                             // x_aa cancels: constant terms, no gradient
    }
  }
  __shared__ float red[2][4];
  lsum = wave_sum(lsum);
  dsum = wave_sum(dsum);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lsum;
    red[1][threadIdx.x >> 6] = dsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(loss, (red[0][0] + red[0][1] + red[0][2] + red[0][3]) * inv_count);
    if (dx) dx[(long)a * n + a] = -(red[1][0] + red[1][1] + red[1][2] + red[1][3]) * inv_count;
  }
}
}  // namespace

// ---- dual-softmax re-scaling of a retrieval similarity matrix (run/test_epic.py:137-143) ------------------------------------
//   y = softmax(x / temp, dim = 1) * x        (row-wise prior: one wave per row, the row is streamed three times from L2)
//   z = softmax(y, dim = 0)                   (column-wise: a workgroup owns 64 columns; lanes walk the rows coalesced)
namespace {
__global__ __launch_bounds__(256) void dual_softmax_rows_kernel(const float* __restrict__ x, int n, int m, float inv_temp,
                                                                float* __restrict__ y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* xr = x + (long)row * m;
  float mx = -3.0e38f;
  for (int j = lane; j < m; j += 64) mx = fmaxf(mx, xr[j] * inv_temp);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < m; j += 64) sum += __expf(xr[j] * inv_temp - mx);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  float* yr = y + (long)row * m;
  for (int j = lane; j < m; j += 64) yr[j] = __expf(xr[j] * inv_temp - mx) * inv * xr[j];
}

__global__ __launch_bounds__(256) void dual_softmax_cols_kernel(const float* __restrict__ y, int n, int m, float* __restrict__ z) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  const bool live = col < m;
  float mx = -3.0e38f;
  for (int i = part; i < n; i += 4) if (live) mx = fmaxf(mx, y[(long)i * m + col]);
  red[part][threadIdx.x & 63] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][threadIdx.x & 63], red[1][threadIdx.x & 63]), fmaxf(red[2][threadIdx.x & 63], red[3][threadIdx.x & 63]));
  __syncthreads();
  float sum = 0.f;
  for (int i = part; i < n; i += 4) if (live) sum += __expf(y[(long)i * m + col] - mx);
  red[part][threadIdx.x & 63] = sum;
  __syncthreads();
  sum = red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63] + red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63];
  const float inv = 1.0f / sum;
  for (int i = part; i < n; i += 4) if (live) z[(long)i * m + col] = __expf(y[(long)i * m + col] - mx) * inv;
}
}  // namespace

extern "C" int egv_dual_softmax(const float* x, int32_t n, int32_t m, float temp, float* work, float* out, void* stream) {
  if (!x || !work || !out || n <= 0 || m <= 0 || !(temp > 0.f)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(dual_softmax_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x, n, m, 1.0f / temp, work);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(dual_softmax_cols_kernel, dim3((m + 63) / 64), dim3(256), 0, s, work, n, m, out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_maxmargin_fwd_bwd(const float* x, const float* weight, int32_t n, float margin, int32_t fix_norm,
                                     float* loss, float* dx, void* stream) {
  if (!x || !loss || n <= 0 || n > 4096 || (fix_norm && n < 2)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(loss, 0, sizeof(float), s) != hipSuccess) return EGV_ERR_LAUNCH;
  const double count = fix_norm ? 2.0 * n * (n - 1.0) : 2.0 * n * (double)n;
  EGV_LAUNCH(maxmargin_kernel, dim3(n), dim3(256), 0, s, x, weight, n, margin, fix_norm, (float)(1.0 / count), loss, dx);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}


// ---- softmax cross-entropy of the classification fine-tunes (OSCC / PNR: model/loss.py:135-141 = nn.CrossEntropyLoss with its
// defaults, mean over the targets != ignore_index; trainer/trainer_oscc.py:335-338 feeds it the [B, 2] / [B, 17] scores of
// FrozenInTime(video_only=True) and int64 labels).  One workgroup: a wave per row (log-sum-exp by wave shuffles), the row losses
// are summed in a fixed order through LDS, so the result is deterministic; d_logits = (softmax - onehot) / #valid.
namespace {
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits, long ld, const long long* __restrict__ target,
                                                            int rows, int cols, long long ignore_index, float* __restrict__ loss,
                                                            float* __restrict__ dlogits, long ldd) {
  __shared__ float part[4];
  __shared__ int cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // pass 1: number of valid rows (the gradient scale), then pass 2: losses and gradients
  // A label outside [0, cols) that is not ignore_index is an ERROR (torch raises a device assert): it must neither be skipped
  // silently nor inflate the mean's denominator -- the loss comes back NaN (and the gradient of every row with it).
  __shared__ int bad[4];
  int nvalid = 0, nbad = 0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const long long t = target[r];
    nvalid += (t != ignore_index);
    nbad += (t != ignore_index && (t < 0 || t >= cols));
  }
  nvalid = (int)wave_sum((float)nvalid);
  nbad = (int)wave_sum((float)nbad);
  if (lane == 0) { cnt[wave] = nvalid; bad[wave] = nbad; }
  __syncthreads();
  const int valid = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  const bool any_bad = (bad[0] + bad[1] + bad[2] + bad[3]) > 0;
  const float inv = valid > 0 ? 1.0f / (float)valid : 0.f;
  float acc = 0.f;
  for (int r = wave; r < rows; r += 4) {
    const float* x = logits + (long)r * ld;
    const long long t = target[r];
    const bool on = t != ignore_index && t >= 0 && t < cols;
    float m = -3.0e38f;
    for (int c = lane; c < cols; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < cols; c += 64) se += __expf(x[c] - m);
    se = wave_sum(se);
    const float lse = m + __logf(se);
    if (on) acc += lse - x[t];
    if (dlogits) {
      float* d = dlogits + (long)r * ldd;
      for (int c = lane; c < cols; c += 64)
        d[c] = any_bad ? __builtin_nanf("") : (on ? (__expf(x[c] - lse) - (c == (int)t ? 1.f : 0.f)) * inv : 0.f);
    }
  }
  if (lane == 0) part[wave] = acc;      // every lane of a wave holds the same acc
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (valid > 0 && !any_bad) ? (part[0] + part[1] + part[2] + part[3]) * inv : __builtin_nanf("");
}
}  // namespace

extern "C" int egv_cross_entropy_fwd_bwd(const float* logits, int64_t ld, const int64_t* target, int32_t rows, int32_t cols,
                                         int64_t ignore_index, float* loss, float* dlogits, int64_t ldd, void* stream) {
  if (!logits || !target || !loss || rows <= 0 || cols <= 0 || rows > (1 << 20) || cols > 65536 || ld < cols) return EGV_ERR_ARG;
  if (dlogits && ldd < cols) return EGV_ERR_ARG;
  EGV_LAUNCH(cross_entropy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, (const long long*)target, rows, cols,
             (long long)ignore_index, loss, dlogits, (long)ldd);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
