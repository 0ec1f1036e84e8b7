// Fused multi-tensor AdamW, transformers==4.2.1 semantics (the optimizer configs/pt/egoclip.json:49-54
// + run/train_egoclip.py:73 instantiate):  m,v EMA -> denom = sqrt(v) + eps (eps OUTSIDE the bias
// correction) -> p -= lr*sqrt(1-b2^t)/(1-b1^t) * m/denom -> decoupled weight decay p -= lr*wd*p.
// The reference loops over 327 tensors with ~8 ATen launches each; here the 180.9 M parameters are one
// pass of ~10 launches (pointer tables travel in the kernel arguments), 16 B/lane accesses: the step is
// pure HBM traffic, 16 B read + 12 B written per parameter (+4 B when the bf16 planes are refreshed).
#include "common.h"
#include "egovlp_hip.h"
#include "multi_tensor.h"

namespace {

constexpr int MAX_T = 48;        // tensors per launch
constexpr int CHUNK = 16384;     // elements per block

struct AdamTable {
  float* p[MAX_T];
  const float* g[MAX_T];
  float* m[MAX_T];
  float* v[MAX_T];
  bf16_t* wh[MAX_T];
  bf16_t* wl[MAX_T];
  long numel[MAX_T];
  MtIndex<MAX_T> ix;
};
static_assert(sizeof(AdamTable) <= 4096, "the table travels in the kernel arguments");

__global__ __launch_bounds__(256) void adamw_kernel(const AdamTable t, float lr, float b1, float b2, float eps, float wd,
                                                    float step_size, float grad_scale, const float* __restrict__ hyper) {
  // hyper (optional, device): {lr, step_size, grad_scale, skip} of THIS step, written by egv_loss_scale_update on the same stream:
  // whether the step happens at all (an overflow of the fp16 backward skips it), the 1 / S that un-scales the gradients and the bias
  // correction at the number of steps actually APPLIED are decided on the device -- the host never waits for a found-inf flag
  if (hyper) {
    if (hyper[3] != 0.f) return;       // skipped step: parameters and moments stay as they are
    lr = hyper[0];
    step_size = hyper[1];
    grad_scale = hyper[2];
  }
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  float* __restrict__ p = t.p[ti];
  const float* __restrict__ g = t.g[ti];
  float* __restrict__ m = t.m[ti];
  float* __restrict__ v = t.v[ti];
  bf16_t* wh = t.wh[ti];
  bf16_t* wl = t.wl[ti];
  const long end = min(n, base + CHUNK);
  // 16-byte accesses only where all four streams allow them (bucket views / odd offsets fall back to the scalar loop)
  const bool vec = ((n & 3) == 0) && (((((size_t)p) | ((size_t)g) | ((size_t)m) | ((size_t)v)) & 15) == 0) &&
                   (!wh || (((size_t)wh) & 7) == 0) && (!wl || (((size_t)wl) & 7) == 0);
  if (vec) {
    for (long i = base + threadIdx.x * 4; i < end; i += 256 * 4) {
      f32x4_t pv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i), gv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i),
               mv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(m + i), vv = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(v + i);
      bf16_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ge = gv[e] * grad_scale;
        mv[e] = mv[e] * b1 + (1.0f - b1) * ge;
        vv[e] = vv[e] * b2 + (1.0f - b2) * ge * ge;
        const float denom = sqrtf(vv[e]) + eps;
        pv[e] = pv[e] - step_size * (mv[e] / denom);
        if (wd > 0.f) pv[e] = pv[e] - lr * wd * pv[e];
        split_bf16(pv[e], h[e], l[e]);
      }
      egv_store<EGV_NT_ADAMW_ST>(p + i, pv);
      egv_store<EGV_NT_ADAMW_ST>(m + i, mv);
      egv_store<EGV_NT_ADAMW_ST>(v + i, vv);
      if (wh) *(u32x2_t*)(wh + i) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
      if (wl) *(u32x2_t*)(wl + i) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
    }
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) {
      const float ge = g[i] * grad_scale;
      const float me = m[i] * b1 + (1.0f - b1) * ge;
      const float ve = v[i] * b2 + (1.0f - b2) * ge * ge;
      float pe = p[i] - step_size * (me / (sqrtf(ve) + eps));
      if (wd > 0.f) pe = pe - lr * wd * pe;
      p[i] = pe;
      m[i] = me;
      v[i] = ve;
      bf16_t h, l;
      split_bf16(pe, h, l);
      if (wh) wh[i] = h;
      if (wl) wl[i] = l;
    }
  }
}

// ---- dynamic loss scale of the fp16 backward ---------------------------------------------------------------------------------------
// (1) any non-finite value in any gradient -> state.found_inf
constexpr int NF_MAX_T = 96;
struct NonfiniteTable {
  const float* g[NF_MAX_T];
  long numel[NF_MAX_T];
  MtIndex<NF_MAX_T> ix;
};
static_assert(sizeof(NonfiniteTable) <= 4096, "the table travels in the kernel arguments");
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const NonfiniteTable t, int* __restrict__ state) {
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * (4 * CHUNK);
  const long n = t.numel[ti];
  const float* __restrict__ g = t.g[ti];
  const long end = min(n, base + 4 * CHUNK);
  // the OR of the "bad" bits (egv_nonfinite) of all elements
  unsigned bad = 0u;
  if (((n & 3) == 0) && ((((size_t)g) & 15) == 0)) {
    // four independent 16-byte loads per lane in flight (a pure read stream: 724 MB per step, HBM-bound)
    long i = base + threadIdx.x * 4;
    for (; i + 3 * 1024 < end; i += 4 * 1024) {
      u32x4_t w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = __builtin_bit_cast(u32x4_t, egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i + u * 1024));
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= egv_nonfinite(w[u][e]) ? 1u : 0u;
    }
    for (; i < end; i += 1024) {
      const u32x4_t w = __builtin_bit_cast(u32x4_t, egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i));
#pragma unroll
      for (int e = 0; e < 4; ++e) bad |= egv_nonfinite(w[e]) ? 1u : 0u;
    }
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) bad |= egv_nonfinite(__float_as_uint(g[i])) ? 1u : 0u;
  }
  if (__any(bad != 0u) && (threadIdx.x & 63) == 0) atomicOr(state + 2, 1);      // one atomic per wave that saw one; normally none
}

// (2) the per-step decision, one thread.  state (8 x 32 bits, DEVICE): [0] float scale S; [1] int good steps since the last change of
// S; [2] int found_inf (set by (1), cleared here); [3] int steps skipped so far; [4..7] float {lr, step_size, 1 / S, skip} = the hyper
// block egv_adamw_multi reads (hyper_out may also point to a caller's own 4 floats: one block per parameter group).
__global__ void loss_scale_update_kernel(int* __restrict__ state, float* __restrict__ hyper_out, float lr, float beta1, float beta2,
                                         int step, int correct_bias, float growth, float backoff, int interval, float max_scale, int advance) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float* fs = (float*)state;
  float skip = fs[7], inv = fs[6];
  if (advance) {
    const float S = fs[0];
    inv = 1.0f / S;                              // the scale the gradients of THIS step carry
    if (state[2] != 0) {
      skip = 1.0f;
      state[3] += 1;
      state[1] = 0;
      fs[0] = fmaxf(S * backoff, 1.0f);
    } else {
      skip = 0.0f;
      const int good = state[1] + 1;
      if (good >= interval) {
        fs[0] = fminf(S * growth, max_scale);
        state[1] = 0;
      } else {
        state[1] = good;
      }
    }
    state[2] = 0;
    fs[6] = inv;
    fs[7] = skip;
  }
  // bias correction at the number of steps actually applied (a skipped step does not count): t = step - skipped
  const int t = max(step - state[3], 1);
  float step_size = lr;
  if (correct_bias) {
    const double bc1 = 1.0 - pow((double)beta1, (double)t);
    const double bc2 = 1.0 - pow((double)beta2, (double)t);
    step_size = (float)((double)lr * sqrt(bc2) / bc1);
  }
  hyper_out[0] = lr;
  hyper_out[1] = step_size;
  hyper_out[2] = inv;
  hyper_out[3] = skip;
}

// ---- gradient accumulation of the embedding-cache step ------------------------------------------------------------------------------
// dst[i][j] += src[i][j]: the chunk gradients of a step that re-encodes its batch in chunks are summed into one accumulator per
// parameter.  Pure HBM traffic (8 B read + 4 B written per element).  Work list: (tensor, CHUNK-element piece) per block, 16-byte
// pieces inside it; every element has exactly one writer (no atomics: the sum does not depend on the grid).  120 tensors per launch
// keep the pointer table inside the 4 KB of kernel arguments.
constexpr int ACC_MAX_T = 120;
struct AccumTable {
  float* d[ACC_MAX_T];
  const float* s[ACC_MAX_T];
  long numel[ACC_MAX_T];
  MtIndex<ACC_MAX_T> ix;
};
static_assert(sizeof(AccumTable) <= 4096, "the table travels in the kernel arguments");

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const AccumTable t) {
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  float* __restrict__ d = t.d[ti];
  const float* __restrict__ s = t.s[ti];
  const long end = min(n, base + CHUNK);
  // 16-byte pieces where both bases allow them (a view at an odd offset takes the scalar loop), then the tensor's last n % 4 elements
  const bool vec = (((((size_t)d) | ((size_t)s)) & 15) == 0);
  const long vend = vec ? min(end, n & ~3L) : base;
  long i = base + threadIdx.x * 4;
  for (; i + 3 * 1024 < vend; i += 4 * 1024) {       // four independent 16-byte load pairs per lane in flight
    f32x4_t a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(d + i + u * 1024);
      b[u] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(s + i + u * 1024);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) egv_store<EGV_NT_ADAMW_ST>(d + i + u * 1024, a[u] + b[u]);
  }
  for (; i < vend; i += 1024) {
    const f32x4_t a = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(d + i), b = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(s + i);
    egv_store<EGV_NT_ADAMW_ST>(d + i, a + b);
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) d[j] = d[j] + s[j];
}

// ---- gradient clipping by global norm --------------------------------------------------------------------------------------------------
// (1) the scan above and sum(g * g) in ONE read of the gradients.  Work list of grad_nonfinite_kernel (tensor, 4 * CHUNK-element piece
// per block); 16-byte loads, four in flight, where the base is 16-byte aligned, a scalar loop otherwise and for the tensor's last
// n % 4 elements.  fp32 throughout: four accumulators per lane (<= 64 adds each; one accumulator with <= 256 adds on the scalar path),
// combined, the wave's butterfly (6 levels), the block's four waves through LDS in a fixed order -> ONE partial per block, stored at
// partials[first + blockIdx.x].  No floating-point atomics: a partial depends on its 65 536 elements alone, never on the schedule.
// All terms are >= 0, so the relative error of a partial is <= (256 + 8) * 2^-24 = 1.6e-5, half that on the root.
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const NonfiniteTable t, float* __restrict__ partials, int first,
                                                          int* __restrict__ state) {
  __shared__ float sh[4];
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * (4 * CHUNK);
  const long n = t.numel[ti];
  const float* __restrict__ g = t.g[ti];
  const long end = min(n, base + 4 * CHUNK);
  const long vend = ((((size_t)g) & 15) == 0) ? min(end, n & ~3L) : base;
  unsigned bad = 0u;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  long i = base + threadIdx.x * 4;
  for (; i + 3 * 1024 < vend; i += 4 * 1024) {
    f32x4_t w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i + u * 1024);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bad |= egv_nonfinite(__float_as_uint(w[u][e])) ? 1u : 0u;
        acc[e] = fmaf(w[u][e], w[u][e], acc[e]);
      }
  }
  for (; i < vend; i += 1024) {
    const f32x4_t w = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(g + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bad |= egv_nonfinite(__float_as_uint(w[e])) ? 1u : 0u;
      acc[e] = fmaf(w[e], w[e], acc[e]);
    }
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) {
    const float x = g[j];
    bad |= egv_nonfinite(__float_as_uint(x)) ? 1u : 0u;
    acc[0] = fmaf(x, x, acc[0]);
  }
  if (state && __any(bad != 0u) && (threadIdx.x & 63) == 0) atomicOr(state + 2, 1);      // as the scan: an integer OR, normally none
  const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[first + (int)blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// (2) the clip decision, one workgroup.  norm block (8 x 32 bits, DEVICE): [0] float norm of the UN-scaled gradients before clipping;
// [1] float coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), 0 in a step that is not applied; [2] int this
// step's norm was not finite; [3] int steps clipped so far (coef < 1); [4] int steps not applied for a non-finite norm; [5..7] unused.
constexpr int CLIP_MAX_H = 64;   // hyper blocks (parameter groups / launch groups) one decision serves
struct ClipTable {
  float* hyper[CLIP_MAX_H];
  float lr[CLIP_MAX_H];
  float step_size[CLIP_MAX_H];
  int count;
};
__global__ __launch_bounds__(256) void grad_clip_update_kernel(const float* __restrict__ partials, int parts, const int* state,
                                                               float grad_scale, float max_norm, const ClipTable t, int fill,
                                                               int* norm_block) {
  __shared__ double sh[4];
  // the partials in a fixed order, in double: lane-strided, the wave's butterfly, the four waves
  double s = 0.0;
  for (int i = threadIdx.x; i < parts; i += 256) s += (double)partials[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double total = (sh[0] + sh[1]) + (sh[2] + sh[3]);            // norm^2 of the gradients as they are (scaled by S)
  // with a scaler: 1 / S and the skip of THIS step, as egv_loss_scale_update (advance) left them; both are read before any hyper
  // block is written (the first group's block IS state + 4)
  const float* fs = (const float*)state;
  const float inv = state ? fs[6] : grad_scale;
  const bool skipped = state ? (fs[7] != 0.f) : false;
  const float norm = (float)(sqrt(total) * (double)inv);
  const bool nonfinite = skipped || egv_nonfinite(__float_as_uint(norm));
  float coef = 0.f;
  if (nonfinite) {
    norm_block[4] += 1;
  } else {
    coef = fminf(1.0f, max_norm / (norm + 1e-6f));
    if (coef < 1.0f) norm_block[3] += 1;
  }
  ((float*)norm_block)[0] = norm;
  ((float*)norm_block)[1] = coef;
  norm_block[2] = nonfinite ? 1 : 0;
  for (int k = 0; k < t.count; ++k) {
    float* h = t.hyper[k];
    if (fill) {
      h[0] = t.lr[k];
      h[1] = t.step_size[k];
    }
    h[2] = inv * coef;
    h[3] = nonfinite ? 1.0f : 0.0f;
  }
}

}  // namespace

extern "C" int egv_grad_accumulate_multi(int32_t count, float* const* dst, const float* const* src, const int64_t* numel, void* stream) {
  if (count < 0 || (count > 0 && (!dst || !src || !numel))) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return mt_for_each_launch<AccumTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] <= 0) return numel[i];                                               // 0 is skipped, a negative size is invalid
        if (!dst[i] || !src[i]) return -1;
        if (dst[i] < src[i] + numel[i] && src[i] < dst[i] + numel[i]) return -1;          // overlapping ranges
        return pieces(numel[i], CHUNK);
      },
      [&](AccumTable& t, int k, int i) { t.d[k] = dst[i]; t.s[k] = src[i]; t.numel[k] = numel[i]; },
      [&](const AccumTable& t, int nb) -> int {
        EGV_LAUNCH(grad_accumulate_kernel, dim3(nb), dim3(256), 0, s, t);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}

// The work list of the two gradient scans: (tensor, 4 * CHUNK-element piece) per block.  launch(t, nb, first): `first` = the blocks of
// the launches before this one.  A NULL pointer of a non-empty tensor is invalid; a negative size is invalid or skipped, as the caller says.
template <typename Launch>
static int for_each_scan_launch(int32_t count, const float* const* g, const int64_t* numel, bool negative_is_invalid, Launch launch) {
  int first = 0;
  return mt_for_each_launch<NonfiniteTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] <= 0) return negative_is_invalid ? numel[i] : 0;
        return g[i] ? pieces(numel[i], 4 * CHUNK) : -1;
      },
      [&](NonfiniteTable& t, int k, int i) { t.g[k] = g[i]; t.numel[k] = numel[i]; },
      [&](const NonfiniteTable& t, int nb) -> int {
        const int rc = launch(t, nb, first);
        first += nb;
        return rc;
      });
}

extern "C" int egv_grad_nonfinite_multi(int32_t count, const float* const* g, const int64_t* numel, int32_t* state, void* stream) {
  if (count < 0 || !g || !numel || !state) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return for_each_scan_launch(count, g, numel, false, [&](const NonfiniteTable& t, int nb, int) -> int {
    EGV_LAUNCH(grad_nonfinite_kernel, dim3(nb), dim3(256), 0, s, t, state);
    EGV_CHECK_LAUNCH();
    return EGV_OK;
  });
}

// blocks (= partials) of a gradient list, or -1 for a list no launch sequence can take
static int64_t sqnorm_parts(int32_t count, const int64_t* numel) {
  if (count < 0 || (count > 0 && !numel)) return -1;
  int64_t parts = 0;
  for (int i = 0; i < count; ++i) {
    const int64_t b = pieces(numel[i], 4 * CHUNK);
    if (b < 0) return -1;
    parts += b;
    if (parts > 0x7fffffff) return -1;
  }
  return parts;
}

extern "C" int egv_grad_sqnorm_parts(int32_t count, const int64_t* numel) { return (int)sqnorm_parts(count, numel); }

extern "C" int egv_grad_sqnorm_multi(int32_t count, const float* const* g, const int64_t* numel, float* partials,
                                     int32_t parts_capacity, int32_t* state, void* stream) {
  const int64_t parts = sqnorm_parts(count, numel);
  if (parts < 0 || parts_capacity < parts || (parts > 0 && (!g || !partials))) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return for_each_scan_launch(count, g, numel, true, [&](const NonfiniteTable& t, int nb, int first) -> int {
    EGV_LAUNCH(grad_sqnorm_kernel, dim3(nb), dim3(256), 0, s, t, partials, first, state);
    EGV_CHECK_LAUNCH();
    return EGV_OK;
  });
}

extern "C" int egv_grad_clip_update(const float* partials, int32_t parts, const int32_t* state, float grad_scale, float max_norm,
                                    int32_t n_hyper, float* const* hyper, const float* lr, const float* step_size,
                                    int32_t* norm_block, void* stream) {
  if (parts < 0 || (parts > 0 && !partials) || !(max_norm > 0.f) || n_hyper < 1 || n_hyper > CLIP_MAX_H || !hyper || !norm_block)
    return EGV_ERR_ARG;
  if (!state && (!lr || !step_size)) return EGV_ERR_ARG;      // no scaler: the blocks are filled here, from the host's scalars
  ClipTable t;
  for (int k = 0; k < n_hyper; ++k) {
    if (!hyper[k]) return EGV_ERR_ARG;
    t.hyper[k] = hyper[k];
    t.lr[k] = state ? 0.f : lr[k];
    t.step_size[k] = state ? 0.f : step_size[k];
  }
  t.count = n_hyper;
  EGV_LAUNCH(grad_clip_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, parts, (const int*)state, grad_scale,
             max_norm, t, state ? 0 : 1, (int*)norm_block);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_loss_scale_update(int32_t* state, float* hyper_out, float lr, float beta1, float beta2, int32_t step,
                                     int32_t correct_bias, float growth_factor, float backoff_factor, int32_t growth_interval,
                                     float max_scale, int32_t advance, void* stream) {
  if (!state || step < 1 || !(growth_factor >= 1.0f) || !(backoff_factor > 0.f && backoff_factor <= 1.0f) || growth_interval < 1 ||
      !(max_scale >= 1.0f))
    return EGV_ERR_ARG;
  EGV_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, hyper_out ? hyper_out : (float*)state + 4, lr,
             beta1, beta2, step, correct_bias, growth_factor, backoff_factor, growth_interval, max_scale, advance);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_adamw_multi(int32_t count, float* const* p, const float* const* g, float* const* m, float* const* v,
                               egv_bf16* const* w_hi, egv_bf16* const* w_lo, const int64_t* numel, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int32_t step,
                               int32_t correct_bias, float grad_scale, const float* hyper_dev, void* stream) {
  if (count < 0 || !p || !g || !m || !v || !numel || step < 1) return EGV_ERR_ARG;
  float step_size = lr;
  if (correct_bias) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    step_size = (float)((double)lr * sqrt(bc2) / bc1);
  }
  hipStream_t s = (hipStream_t)stream;
  return mt_for_each_launch<AdamTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] <= 0) return 0;
        return (p[i] && g[i] && m[i] && v[i]) ? pieces(numel[i], CHUNK) : -1;
      },
      [&](AdamTable& t, int k, int i) {
        t.p[k] = p[i]; t.g[k] = g[i]; t.m[k] = m[i]; t.v[k] = v[i];
        t.wh[k] = w_hi ? w_hi[i] : nullptr;
        t.wl[k] = w_lo ? w_lo[i] : nullptr;
        t.numel[k] = numel[i];
      },
      [&](const AdamTable& t, int nb) -> int {
        EGV_LAUNCH(adamw_kernel, dim3(nb), dim3(256), 0, s, t, lr, beta1, beta2, eps, weight_decay, step_size, grad_scale, hyper_dev);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}
