// LAMB (You et al. 2020) on the device: Adam moments, a per-tensor trust ratio r = ||p|| / ||u||, p -= lr * r * u.  Three launches per
// launch group of the optimizer, no host synchronisation, no floating-point atomics:
//   egv_lamb_stage1_multi  reads p, g, m, v; writes m, v; forms u = c * m / (sqrt(v) + eps) + wd * p in registers and reduces p^2 and
//                          u^2 to ONE pair of fp32 partials per block.  Neither p nor g is written.
//   egv_lamb_ratio         one workgroup per tensor: its run of partial pairs summed in double in a fixed order -> r into a device array.
//   egv_lamb_stage2_multi  reads p, m, v; recomputes u with the expression of stage 1 (lamb_dir below); p = fmaf(-(lr * r), u, p).
// The direction is the one adamw_kernel (csrc/adamw.hip) applies, per unit lr: eps OUTSIDE the bias correction c = sqrt(1 - b2^t) /
// (1 - b1^t).  With a hyper block {lr, step_size, (1 / S) * coef, skip} (egv_loss_scale_update, egv_grad_clip_update) c = step_size / lr
// is formed on the device, so t counts the steps actually APPLIED; a skipped step returns from all three kernels before any store.
// Work list: (tensor, CHUNK-element piece) per block, as adamw_kernel; 16-byte pieces where all bases are 16-byte aligned, a scalar loop
// otherwise and for the tensor's last n % 4 elements.  HBM traffic: 16 B + 8 B (stage 1), 12 B + 4 B (stage 2) = 40 B per parameter.
#include "common.h"
#include "egovlp_hip.h"
#include "multi_tensor.h"

namespace {

constexpr int LAMB_MAX_T = 48;          // tensors per launch of the two element-wise stages
constexpr int LAMB_RATIO_MAX_T = 192;   // tensors (= workgroups) per launch of the ratio kernel
constexpr int CHUNK = 16384;            // elements per block

struct LambTable {
  float* p[LAMB_MAX_T];
  const float* g[LAMB_MAX_T];           // stage 1 only
  float* m[LAMB_MAX_T];
  float* v[LAMB_MAX_T];
  long numel[LAMB_MAX_T];
  int slot[LAMB_MAX_T];                 // index in the caller's list: the tensor's ratio is ratios[slot]
  MtIndex<LAMB_MAX_T> ix;
};
static_assert(sizeof(LambTable) <= 4096, "the table travels in the kernel arguments");

struct RatioTable {
  int start[LAMB_RATIO_MAX_T];          // first partial pair of the tensor
  int parts[LAMB_RATIO_MAX_T];          // how many it has (0: an empty tensor)
  int slot[LAMB_RATIO_MAX_T];
  MtIndex<LAMB_RATIO_MAX_T> ix;
};
static_assert(sizeof(RatioTable) <= 4096, "the table travels in the kernel arguments");

// The hyper block of this step overrides the host's scalars.  -> false: the step is skipped, nothing may be stored.
// c = step_size / lr (two roundings away from the exact correction); lr == 0 leaves the host's c: p does not move then, and the ratio
// stays defined.
__device__ __forceinline__ bool lamb_hyper(const float* __restrict__ hyper, float& lr, float& c, float& grad_scale) {
  if (!hyper) return true;
  if (hyper[3] != 0.f) return false;
  lr = hyper[0];
  if (lr != 0.f) c = hyper[1] / lr;
  grad_scale = hyper[2];
  return true;
}

__device__ __forceinline__ void lamb_moments(float g, float grad_scale, float b1, float b2, float& m, float& v) {
  const float ge = g * grad_scale;
  m = m * b1 + (1.0f - b1) * ge;
  v = v * b2 + (1.0f - b2) * ge * ge;
}

// u, from the NEW moments: the one expression both stages evaluate (explicit fmaf: no contraction choice is left to the compiler)
__device__ __forceinline__ float lamb_dir(float p, float m, float v, float c, float eps, float wd) {
  return fmaf(wd, p, c * (m / (sqrtf(v) + eps)));
}

__global__ __launch_bounds__(256) void lamb_stage1_kernel(const LambTable t, float lr, float b1, float b2, float eps, float wd, float c,
                                                          float grad_scale, const float* __restrict__ hyper,
                                                          float* __restrict__ partials, int first) {
  __shared__ float sh[8];
  if (!lamb_hyper(hyper, lr, c, grad_scale)) return;
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  const float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  float* __restrict__ v = t.v[ti];
  const long end = min(n, base + CHUNK);
  const bool vec = (((((size_t)p) | ((size_t)g) | ((size_t)m) | ((size_t)v)) & 15) == 0);
  const long vend = vec ? min(end, n & ~3L) : base;
  // lane accumulators: four per norm on the 16-byte path (<= 16 adds each), the first one alone on the scalar path (<= 64 adds)
  float ap[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
  long i = base + threadIdx.x * 4;
  for (; i + 1024 < vend; i += 2 * 1024) {          // two independent sets of four 16-byte loads per lane in flight
    f32x4_t pv[2], gv[2], mv[2], vv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      pv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i + k * 1024);
      gv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i + k * 1024);
      mv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(m + i + k * 1024);
      vv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(v + i + k * 1024);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float me = mv[k][e], ve = vv[k][e];
        lamb_moments(gv[k][e], grad_scale, b1, b2, me, ve);
        mv[k][e] = me;
        vv[k][e] = ve;
        const float u = lamb_dir(pv[k][e], me, ve, c, eps, wd);
        ap[e] = fmaf(pv[k][e], pv[k][e], ap[e]);
        au[e] = fmaf(u, u, au[e]);
      }
      egv_store<EGV_NT_ADAMW_ST>(m + i + k * 1024, mv[k]);
      egv_store<EGV_NT_ADAMW_ST>(v + i + k * 1024, vv[k]);
    }
  }
  for (; i < vend; i += 1024) {
    const f32x4_t pv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i), gv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i);
    f32x4_t mv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(m + i), vv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(v + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[e], ve = vv[e];
      lamb_moments(gv[e], grad_scale, b1, b2, me, ve);
      mv[e] = me;
      vv[e] = ve;
      const float u = lamb_dir(pv[e], me, ve, c, eps, wd);
      ap[e] = fmaf(pv[e], pv[e], ap[e]);
      au[e] = fmaf(u, u, au[e]);
    }
    egv_store<EGV_NT_ADAMW_ST>(m + i, mv);
    egv_store<EGV_NT_ADAMW_ST>(v + i, vv);
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) {
    const float pe = p[j];
    float me = m[j], ve = v[j];
    lamb_moments(g[j], grad_scale, b1, b2, me, ve);
    const float u = lamb_dir(pe, me, ve, c, eps, wd);
    ap[0] = fmaf(pe, pe, ap[0]);
    au[0] = fmaf(u, u, au[0]);
    m[j] = me;
    v[j] = ve;
  }
  // the fixed order of grad_sqnorm_kernel: lane accumulators, the wave's butterfly, the four waves through LDS
  const float sp = wave_sum((ap[0] + ap[1]) + (ap[2] + ap[3]));
  const float su = wave_sum((au[0] + au[1]) + (au[2] + au[3]));
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = sp;
    sh[4 + (threadIdx.x >> 6)] = su;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = partials + 2 * ((long)first + (long)blockIdx.x);
    out[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    out[1] = (sh[4] + sh[5]) + (sh[6] + sh[7]);
  }
}

// One workgroup per tensor of the caller's list (an empty one included: no partials, both norms 0, r = 1).
__global__ __launch_bounds__(256) void lamb_ratio_kernel(const RatioTable t, const float* __restrict__ partials, int adapt, int trust_clip,
                                                         const float* __restrict__ hyper, float* __restrict__ ratios) {
  __shared__ double sh[8];
  if (hyper && hyper[3] != 0.f) return;          // skipped step: the ratios of the last applied step stay
  const int k = blockIdx.x;                      // one block per item: blk_start[k] == k
  const float* __restrict__ part = partials + 2 * (long)t.start[k];
  const int parts = t.parts[k];
  // the pairs in a fixed order, in double: lane-strided, the wave's butterfly, the four waves
  double sp = 0.0, su = 0.0;
  for (int i = threadIdx.x; i < parts; i += 256) {
    sp += (double)part[2 * i];
    su += (double)part[2 * i + 1];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sp += __shfl_xor(sp, o, 64);
    su += __shfl_xor(su, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6] = sp;
    sh[4 + (threadIdx.x >> 6)] = su;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double pn = sqrt((sh[0] + sh[1]) + (sh[2] + sh[3]));
  const double un = sqrt((sh[4] + sh[5]) + (sh[6] + sh[7]));
  float r = 1.0f;
  if (adapt && pn > 0.0 && un > 0.0) r = (float)(pn / un);
  if (trust_clip) r = fminf(r, 1.0f);
  ratios[t.slot[k]] = r;
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(const LambTable t, float lr, float eps, float wd, float c,
                                                          const float* __restrict__ hyper, const float* __restrict__ ratios) {
  float unused_scale = 1.0f;
  if (!lamb_hyper(hyper, lr, c, unused_scale)) return;
  if (lr == 0.f) return;                         // p stays bit-identical (the moments advanced in stage 1)
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ m = t.m[ti];
  const float* __restrict__ v = t.v[ti];
  const float neg = -(lr * ratios[t.slot[ti]]);
  const long end = min(n, base + CHUNK);
  const bool vec = (((((size_t)p) | ((size_t)m) | ((size_t)v)) & 15) == 0);
  const long vend = vec ? min(end, n & ~3L) : base;
  long i = base + threadIdx.x * 4;
  for (; i + 1024 < vend; i += 2 * 1024) {
    f32x4_t pv[2], mv[2], vv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      pv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i + k * 1024);
      mv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(m + i + k * 1024);
      vv[k] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(v + i + k * 1024);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) pv[k][e] = fmaf(neg, lamb_dir(pv[k][e], mv[k][e], vv[k][e], c, eps, wd), pv[k][e]);
      egv_store<EGV_NT_ADAMW_ST>(p + i + k * 1024, pv[k]);
    }
  }
  for (; i < vend; i += 1024) {
    f32x4_t pv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i);
    const f32x4_t mv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(m + i), vv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(v + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) pv[e] = fmaf(neg, lamb_dir(pv[e], mv[e], vv[e], c, eps, wd), pv[e]);
    egv_store<EGV_NT_ADAMW_ST>(p + i, pv);
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) p[j] = fmaf(neg, lamb_dir(p[j], m[j], v[j], c, eps, wd), p[j]);
}

// sqrt(1 - b2^t) / (1 - b1^t) in double on the fp32 betas, as egv_adamw_multi forms its step size; 1 without the correction
float lamb_correction(float beta1, float beta2, int step, int correct_bias) {
  if (!correct_bias) return 1.0f;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  return (float)(sqrt(bc2) / bc1);
}

// pieces (= partial pairs) of a list, or -1 for a list no launch sequence can take
int64_t lamb_parts(int32_t count, const int64_t* numel) {
  if (count < 0 || (count > 0 && !numel)) return -1;
  int64_t parts = 0;
  for (int i = 0; i < count; ++i) {
    const int64_t b = pieces(numel[i], CHUNK);
    if (b < 0) return -1;
    parts += b;
    if (parts > 0x7fffffff) return -1;
  }
  return parts;
}

}  // namespace

extern "C" int egv_lamb_parts(int32_t count, const int64_t* numel) { return (int)lamb_parts(count, numel); }

extern "C" int egv_lamb_stage1_multi(int32_t count, const float* const* p, const float* const* g, float* const* m, float* const* v,
                                     const int64_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                                     int32_t correct_bias, float grad_scale, const float* hyper_dev, float* partials,
                                     int32_t parts_capacity, void* stream) {
  const int64_t parts = lamb_parts(count, numel);
  if (parts < 0 || step < 1 || parts_capacity < parts || (parts > 0 && (!p || !g || !m || !v || !partials))) return EGV_ERR_ARG;
  const float c = lamb_correction(beta1, beta2, step, correct_bias);
  hipStream_t s = (hipStream_t)stream;
  int first = 0;
  return mt_for_each_launch<LambTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] == 0) return 0;
        return (p[i] && g[i] && m[i] && v[i]) ? pieces(numel[i], CHUNK) : -1;
      },
      [&](LambTable& t, int k, int i) {
        t.p[k] = (float*)p[i]; t.g[k] = g[i]; t.m[k] = m[i]; t.v[k] = v[i];
        t.numel[k] = numel[i];
        t.slot[k] = i;
      },
      [&](const LambTable& t, int nb) -> int {
        EGV_LAUNCH(lamb_stage1_kernel, dim3(nb), dim3(256), 0, s, t, lr, beta1, beta2, eps, weight_decay, c, grad_scale, hyper_dev,
                   partials, first);
        first += nb;
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}

extern "C" int egv_lamb_ratio(int32_t count, const int64_t* numel, const float* partials, int32_t parts, int32_t adapt,
                              int32_t trust_clip, const float* hyper_dev, float* ratios, void* stream) {
  const int64_t want = lamb_parts(count, numel);
  if (want < 0 || parts != want || (want > 0 && !partials) || (count > 0 && !ratios)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int64_t run = 0;
  return mt_for_each_launch<RatioTable>(
      count, [&](int) -> int64_t { return 1; },              // every tensor keeps its slot, an empty one too
      [&](RatioTable& t, int k, int i) {
        const int64_t b = pieces(numel[i], CHUNK);
        t.start[k] = (int)run;
        t.parts[k] = (int)b;
        t.slot[k] = i;
        run += b;
      },
      [&](const RatioTable& t, int nb) -> int {
        EGV_LAUNCH(lamb_ratio_kernel, dim3(nb), dim3(256), 0, s, t, partials, (int)adapt, (int)trust_clip, hyper_dev, ratios);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}

extern "C" int egv_lamb_stage2_multi(int32_t count, float* const* p, const float* const* m, const float* const* v, const int64_t* numel,
                                     float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                                     int32_t correct_bias, const float* hyper_dev, const float* ratios, void* stream) {
  const int64_t parts = lamb_parts(count, numel);
  if (parts < 0 || step < 1 || (parts > 0 && (!p || !m || !v || !ratios))) return EGV_ERR_ARG;
  const float c = lamb_correction(beta1, beta2, step, correct_bias);
  hipStream_t s = (hipStream_t)stream;
  return mt_for_each_launch<LambTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] == 0) return 0;
        return (p[i] && m[i] && v[i]) ? pieces(numel[i], CHUNK) : -1;
      },
      [&](LambTable& t, int k, int i) {
        t.p[k] = p[i]; t.g[k] = nullptr; t.m[k] = (float*)m[i]; t.v[k] = (float*)v[i];
        t.numel[k] = numel[i];
        t.slot[k] = i;
      },
      [&](const LambTable& t, int nb) -> int {
        EGV_LAUNCH(lamb_stage2_kernel, dim3(nb), dim3(256), 0, s, t, lr, eps, weight_decay, c, hyper_dev, ratios);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}
