// Exponential moving average (EMA) of the model weights, kept on the device, and the in-place exchange of two weight sets.
//   egv_ema_decide        one thread: is this update applied (the optimizer's skip flag), with which weight w = 1 - decay
//   egv_ema_update_multi  e += w * (p - e) over a list of tensors, w read from the state block on the device
//   egv_swap_multi        a[i] <-> b[i] over a list of tensors (evaluation under the averaged weights: no second model, no backup copy)
// Both passes are pure HBM traffic (update: 8 B read + 4 B written per element; swap: 8 B + 8 B) on the work list of
// grad_accumulate_kernel (csrc/adamw.hip): (tensor, CHUNK-element piece) per block, 16-byte pieces inside it where both bases are
// 16-byte aligned, a scalar loop otherwise and for the tensor's last n % 4 elements.  Every element has exactly one writer: no atomics,
// no LDS, the result does not depend on the grid.
#include "common.h"
#include "egovlp_hip.h"
#include "multi_tensor.h"

namespace {

constexpr int EMA_MAX_T = 120;   // tensors per launch: the pointer table stays inside the 4 KB of kernel arguments
constexpr int CHUNK = 16384;     // elements per block

struct PairTable {
  float* a[EMA_MAX_T];
  float* b[EMA_MAX_T];
  long numel[EMA_MAX_T];
  MtIndex<EMA_MAX_T> ix;
};
static_assert(sizeof(PairTable) <= 4096, "the table travels in the kernel arguments");

// state (8 x 32 bits, DEVICE): [0] int t, updates applied so far; [1] float w, the weight of THIS update (0: the pass does nothing);
// [2] int updates skipped so far; [3] float the decay in effect (logs); [4..7] zero, reserved.
__global__ void ema_decide_kernel(int* __restrict__ state, const float* __restrict__ skip_flag, float decay, int warmup) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float* fs = (float*)state;
  if (skip_flag && *skip_flag != 0.f) {        // the optimizer step was not applied: the average stays, the warm-up count too
    fs[1] = 0.f;
    state[2] += 1;
    return;
  }
  const int t = state[0];
  double d = (double)decay;
  if (warmup) d = fmin(d, (1.0 + (double)t) / (10.0 + (double)t));
  fs[1] = (float)(1.0 - d);
  fs[3] = (float)d;
  state[0] = t + 1;
}

__global__ __launch_bounds__(256) void ema_update_kernel(const PairTable t, const int* __restrict__ state) {
  const float wgt = ((const float*)state)[1];
  if (wgt == 0.f) return;                       // a skipped update: nothing is read, nothing is written
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  float* __restrict__ e = t.a[ti];
  const float* __restrict__ p = t.b[ti];
  const long end = min(n, base + CHUNK);
  const bool vec = (((((size_t)e) | ((size_t)p)) & 15) == 0);
  const long vend = vec ? min(end, n & ~3L) : base;
  long i = base + threadIdx.x * 4;
  for (; i + 3 * 1024 < vend; i += 4 * 1024) {       // four independent 16-byte load pairs per lane in flight
    f32x4_t a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(e + i + u * 1024);
      b[u] = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i + u * 1024);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[u][k] = fmaf(wgt, b[u][k] - a[u][k], a[u][k]);
      egv_store<EGV_NT_ADAMW_ST>(e + i + u * 1024, a[u]);
    }
  }
  for (; i < vend; i += 1024) {
    f32x4_t a = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(e + i);
    const f32x4_t b = egv_load<EGV_NT_ADAMW_LD, f32x4_t>(p + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = fmaf(wgt, b[k] - a[k], a[k]);
    egv_store<EGV_NT_ADAMW_ST>(e + i, a);
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) e[j] = fmaf(wgt, p[j] - e[j], e[j]);
}

// bit for bit: the values travel as 32-bit integers (a float move may quieten a signalling NaN)
__global__ __launch_bounds__(256) void swap_kernel(const PairTable t) {
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  uint32_t* __restrict__ a = (uint32_t*)t.a[ti];
  uint32_t* __restrict__ b = (uint32_t*)t.b[ti];
  const long end = min(n, base + CHUNK);
  const bool vec = (((((size_t)a) | ((size_t)b)) & 15) == 0);
  const long vend = vec ? min(end, n & ~3L) : base;
  long i = base + threadIdx.x * 4;
  for (; i + 3 * 1024 < vend; i += 4 * 1024) {
    u32x4_t x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = egv_load<EGV_NT_ADAMW_LD, u32x4_t>(a + i + u * 1024);
      y[u] = egv_load<EGV_NT_ADAMW_LD, u32x4_t>(b + i + u * 1024);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      egv_store<EGV_NT_ADAMW_ST>(a + i + u * 1024, y[u]);
      egv_store<EGV_NT_ADAMW_ST>(b + i + u * 1024, x[u]);
    }
  }
  for (; i < vend; i += 1024) {
    const u32x4_t x = egv_load<EGV_NT_ADAMW_LD, u32x4_t>(a + i), y = egv_load<EGV_NT_ADAMW_LD, u32x4_t>(b + i);
    egv_store<EGV_NT_ADAMW_ST>(a + i, y);
    egv_store<EGV_NT_ADAMW_ST>(b + i, x);
  }
  for (long j = max(base, vend) + threadIdx.x; j < end; j += 256) {
    const uint32_t x = a[j], y = b[j];
    a[j] = y;
    b[j] = x;
  }
}

// The list of (a[i], b[i], numel[i]) pairs both passes take, validated as egv_grad_accumulate_multi validates its list: a size of 0
// is skipped; a negative size, a NULL pointer of a non-empty pair or overlapping ranges are invalid, and then nothing is enqueued.
template <typename Launch>
int for_each_pair_launch(int32_t count, float* const* a, float* const* b, const int64_t* numel, Launch launch) {
  if (count < 0 || (count > 0 && (!a || !b || !numel))) return EGV_ERR_ARG;
  return mt_for_each_launch<PairTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] <= 0) return numel[i];
        if (!a[i] || !b[i]) return -1;
        if (a[i] < b[i] + numel[i] && b[i] < a[i] + numel[i]) return -1;
        return pieces(numel[i], CHUNK);
      },
      [&](PairTable& t, int k, int i) { t.a[k] = a[i]; t.b[k] = b[i]; t.numel[k] = numel[i]; }, launch);
}

}  // namespace

extern "C" int egv_ema_decide(int32_t* state, const float* skip_flag, float decay, int32_t warmup, void* stream) {
  if (!state || !(decay >= 0.f && decay < 1.f)) return EGV_ERR_ARG;
  EGV_LAUNCH(ema_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)state, skip_flag, decay, (int)warmup);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_ema_update_multi(int32_t count, float* const* ema, const float* const* p, const int64_t* numel,
                                    const int32_t* state, void* stream) {
  if (!state) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return for_each_pair_launch(count, ema, (float* const*)p, numel, [&](const PairTable& t, int nb) -> int {
    EGV_LAUNCH(ema_update_kernel, dim3(nb), dim3(256), 0, s, t, (const int*)state);
    EGV_CHECK_LAUNCH();
    return EGV_OK;
  });
}

extern "C" int egv_swap_multi(int32_t count, float* const* a, float* const* b, const int64_t* numel, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  return for_each_pair_launch(count, a, b, numel, [&](const PairTable& t, int nb) -> int {
    EGV_LAUNCH(swap_kernel, dim3(nb), dim3(256), 0, s, t);
    EGV_CHECK_LAUNCH();
    return EGV_OK;
  });
}
