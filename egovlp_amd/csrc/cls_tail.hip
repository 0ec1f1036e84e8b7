// The CLS tail of the last SpaceTimeBlock (include/egovlp_hip.h, "the CLS tail"): forward_features reads only the B CLS rows of the last
// block's output (model/video_transformer.py:330), so everything behind that block's k / v projection runs on R = B rows.  Here are the
// R-row pieces: Linears in plain fp32 from the fp32 master weights (forward, dgrad, rank-R wgrad) and the attention of one query row per
// (clip, head) with its backward.  All of them are latency-sized (W is streamed once, 9.4 MB at most; K / V once): plain VALU kernels,
// sums in a fixed order (wave / LDS reductions, a two-stage dgrad), no float atomics.
#include <hip/hip_runtime.h>

#include "egovlp_hip.h"
#include "f16x2.h"

namespace {

constexpr int LIN_CT = 4;       // output columns per workgroup of the forward
constexpr int LIN_RT = 8;       // rows per workgroup
constexpr int DG_NS = 64;       // rows of W (contraction indices) per dgrad slab
constexpr int DG_RT = 8;        // rows per dgrad workgroup

// y[r, n] for LIN_RT rows x LIN_CT columns per workgroup: the 256 threads split K, a wave reduction and one LDS step finish the sums
__global__ __launch_bounds__(256) void cls_linear_fwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ W, long ldw,
                                                             const float* __restrict__ bias, int R, int N, int K, int act,
                                                             float* __restrict__ z_out, const float* __restrict__ res, long ldr,
                                                             float* __restrict__ y, long ldy) {
  __shared__ float red[4][LIN_CT * LIN_RT];
  const int n0 = blockIdx.x * LIN_CT, r0 = blockIdx.y * LIN_RT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[LIN_CT][LIN_RT];
#pragma unroll
  for (int c = 0; c < LIN_CT; ++c)
#pragma unroll
    for (int r = 0; r < LIN_RT; ++r) acc[c][r] = 0.f;
  const int nr = min(LIN_RT, R - r0);
  for (int k4 = threadIdx.x; k4 < K / 4; k4 += 256) {
    f32x4_t w[LIN_CT];
#pragma unroll
    for (int c = 0; c < LIN_CT; ++c) w[c] = *(const f32x4_t*)(W + (long)(n0 + c) * ldw + k4 * 4);      // N % 4 == 0: n0 + c < N
#pragma unroll
    for (int r = 0; r < LIN_RT; ++r) {
      if (r < nr) {
        const f32x4_t xv = *(const f32x4_t*)(x + (long)(r0 + r) * ldx + k4 * 4);
#pragma unroll
        for (int c = 0; c < LIN_CT; ++c) acc[c][r] += w[c][0] * xv[0] + w[c][1] * xv[1] + w[c][2] * xv[2] + w[c][3] * xv[3];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < LIN_CT; ++c)
#pragma unroll
    for (int r = 0; r < LIN_RT; ++r) {
      const float s = wave_sum(acc[c][r]);
      if (lane == 0) red[wave][c * LIN_RT + r] = s;
    }
  __syncthreads();
  if (threadIdx.x < LIN_CT * LIN_RT) {
    const int c = threadIdx.x / LIN_RT, r = threadIdx.x % LIN_RT;
    if (r < nr) {
      const int n = n0 + c;
      const long row = r0 + r;
      float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      if (bias) v += bias[n];
      if (z_out) z_out[row * N + n] = v;
      if (act == EGV_ACT_GELU) v = gelu_f(v);
      if (res) v += res[row * ldr + n];
      y[row * ldy + n] = v;
    }
  }
}

// dgrad, stage 1: partial[slab][r][k] = sum over the slab's DG_NS rows n of dY[r, n] W[n, k]; a thread owns 4 consecutive k
__global__ __launch_bounds__(256) void cls_linear_dgrad_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ W, long ldw,
                                                               int R, int N, int K, float* __restrict__ partial) {
  __shared__ float dys[DG_RT][DG_NS];
  const int n0 = blockIdx.x * DG_NS, r0 = blockIdx.y * DG_RT;
  const int nn = min(DG_NS, N - n0), nr = min(DG_RT, R - r0);
  for (int i = threadIdx.x; i < DG_RT * DG_NS; i += 256) {
    const int r = i / DG_NS, n = i % DG_NS;
    dys[r][n] = (r < nr && n < nn) ? dy[(long)(r0 + r) * lddy + n0 + n] : 0.f;
  }
  __syncthreads();
  for (int k4 = blockIdx.z * 256 + threadIdx.x; k4 < K / 4; k4 += gridDim.z * 256) {
    f32x4_t acc[DG_RT];
#pragma unroll
    for (int r = 0; r < DG_RT; ++r) acc[r] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < nn; ++n) {
      const f32x4_t w = *(const f32x4_t*)(W + (long)(n0 + n) * ldw + k4 * 4);
#pragma unroll
      for (int r = 0; r < DG_RT; ++r) acc[r] += dys[r][n] * w;
    }
#pragma unroll
    for (int r = 0; r < DG_RT; ++r)
      if (r < nr) *(f32x4_t*)(partial + ((long)blockIdx.x * R + r0 + r) * K + k4 * 4) = acc[r];
  }
}

// dgrad, stage 2: the slabs summed in order, x gelu'(z), then stored / added to the destination
__global__ __launch_bounds__(256) void cls_linear_dgrad_finish_kernel(const float* __restrict__ partial, int slabs, int R, int K,
                                                                      const float* __restrict__ z, void* __restrict__ dx, long lddx, int mode) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)R * K) return;
  const int r = (int)(i / K), k = (int)(i % K);
  float v = 0.f;
  for (int s = 0; s < slabs; ++s) v += partial[(long)s * R * K + i];
  if (z) v *= gelu_grad_f(z[i]);
  if (mode == EGV_CLS_DX_ADD_F16) {
    _Float16* p = (_Float16*)dx + (long)r * lddx + k;
    *p = (_Float16)((float)*p + v);          // un-clamped: a scaled gradient beyond fp16's range becomes inf (a skipped step)
  } else {
    float* p = (float*)dx + (long)r * lddx + k;
    *p = mode == EGV_CLS_DX_ADD_F32 ? *p + v : v;
  }
}

// rank-R weight gradient: a workgroup owns 4 rows n of dW and 256 float4 columns; the bias gradient rides with the first column chunk
__global__ __launch_bounds__(256) void cls_linear_wgrad_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ x, long ldx,
                                                               int R, int N, int K, float* __restrict__ dW, long lddw, float* __restrict__ db) {
  const int n0 = blockIdx.x * 4;
  const int k4 = blockIdx.y * 256 + threadIdx.x;
  if (db && blockIdx.y == 0 && threadIdx.x < 4) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += dy[(long)r * lddy + n0 + threadIdx.x];
    db[n0 + threadIdx.x] = s;
  }
  if (k4 >= K / 4) return;
  f32x4_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    const f32x4_t xv = *(const f32x4_t*)(x + (long)r * ldx + k4 * 4);
    const f32x4_t g = *(const f32x4_t*)(dy + (long)r * lddy + n0);       // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += g[j] * xv;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) *(f32x4_t*)(dW + (long)(n0 + j) * lddw + k4 * 4) = acc[j];
}

__global__ __launch_bounds__(256) void cls_rows_add_kernel(float* __restrict__ dst, long lddst, const float* __restrict__ src, long ldsrc, int R,
                                                           int cols) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)R * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  dst[(long)r * lddst + c] += src[(long)r * ldsrc + c];
}

// ---- attention of the CLS query ------------------------------------------------------------------------------------------------
// A workgroup per (clip, head).  Eight lanes share a key (8 head dims = one 16-byte plane piece each), so a wave reads eight whole key
// rows per step and the workgroup 32; every lane group keeps its own online softmax, merged once at the end.

// eight consecutive plane elements (hi [+ lo]) -> fp32
template <int FMT>
__device__ __forceinline__ void load8(const uint16_t* hi, const uint16_t* lo, long off, float (&v)[8]) {
  const u32x4_t a = *(const u32x4_t*)(hi + off);
  u32x4_t b = (u32x4_t){0u, 0u, 0u, 0u};
  if (lo) b = *(const u32x4_t*)(lo + off);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a0, a1, b0, b1;
    if (FMT == 1) {
      f16x2_unpack(a[e], a0, a1);
      f16x2_unpack(b[e], b0, b1);
    } else {
      a0 = __uint_as_float(a[e] << 16); a1 = __uint_as_float(a[e] & 0xffff0000u);
      b0 = __uint_as_float(b[e] << 16); b1 = __uint_as_float(b[e] & 0xffff0000u);
    }
    v[2 * e] = a0 + b0;
    v[2 * e + 1] = a1 + b1;
  }
}

__device__ __forceinline__ float group8_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

constexpr float ATTN_SCALE = 0.125f;       // 64^-0.5

template <int FMT>
__global__ __launch_bounds__(256) void cls_attn_fwd_kernel(const float* __restrict__ q, long ldq, const uint16_t* __restrict__ k_hi,
                                                           const uint16_t* __restrict__ k_lo, const uint16_t* __restrict__ v_hi,
                                                           const uint16_t* __restrict__ v_lo, long ldkv, int S, int H,
                                                           float* __restrict__ out, long ldo, float* __restrict__ lse) {
  __shared__ float sm[32], sl[32], sacc[32][64];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int sub = threadIdx.x & 7, grp = threadIdx.x >> 3;       // 32 key groups
  float qv[8], acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    qv[e] = q[(long)b * ldq + h * 64 + sub * 8 + e] * ATTN_SCALE;
    acc[e] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int j = grp; j < S; j += 32) {
    const long off = ((long)b * S + j) * ldkv + h * 64 + sub * 8;
    float kv[8], vv[8];
    load8<FMT>(k_hi, k_lo, off, kv);
    load8<FMT>(v_hi, v_lo, off, vv);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += qv[e] * kv[e];
    s = group8_sum(s);
    const float mn = fmaxf(m, s);
    const float c = __expf(m - mn), p = __expf(s - mn);          // m = -inf at the first key: c = 0
    l = l * c + p;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] * c + p * vv[e];
    m = mn;
  }
  if (sub == 0) { sm[grp] = m; sl[grp] = l; }
#pragma unroll
  for (int e = 0; e < 8; ++e) sacc[grp][sub * 8 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 64) {
    float mx = -INFINITY;
    for (int g = 0; g < 32; ++g) mx = fmaxf(mx, sm[g]);
    float lt = 0.f, o = 0.f;
    for (int g = 0; g < 32; ++g) {
      if (sm[g] == -INFINITY) continue;                         // a group that saw no key (S < 32)
      const float w = __expf(sm[g] - mx);
      lt += sl[g] * w;
      o += sacc[g][threadIdx.x] * w;
    }
    out[(long)b * ldo + h * 64 + threadIdx.x] = o / lt;
    if (threadIdx.x == 0) lse[b * H + h] = mx + __logf(lt);
  }
}

template <int FMT, int DFMT>
__global__ __launch_bounds__(256) void cls_attn_bwd_kernel(const float* __restrict__ q, long ldq, const uint16_t* __restrict__ k_hi,
                                                           const uint16_t* __restrict__ k_lo, const uint16_t* __restrict__ v_hi,
                                                           const uint16_t* __restrict__ v_lo, long ldkv, const float* __restrict__ out,
                                                           const float* __restrict__ d_out, const float* __restrict__ lse, int S, int H,
                                                           float* __restrict__ dq, uint16_t* __restrict__ dk_hi, uint16_t* __restrict__ dk_lo,
                                                           uint16_t* __restrict__ dv_hi, uint16_t* __restrict__ dv_lo, long lddkv) {
  __shared__ float sdq[32][64];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int sub = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const long D = (long)H * 64;
  float qv[8], dov[8], dqa[8];
  float dl = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const long c = (long)b * D + h * 64 + sub * 8 + e;
    qv[e] = q[(long)b * ldq + h * 64 + sub * 8 + e] * ATTN_SCALE;
    dov[e] = d_out[c];
    dl += dov[e] * out[c];
    dqa[e] = 0.f;
  }
  const float delta = group8_sum(dl);        // rowsum(dO o O) of this head
  const float L = lse[b * H + h];
  for (int j = grp; j < S; j += 32) {
    const long off = ((long)b * S + j) * ldkv + h * 64 + sub * 8;
    float kv[8], vv[8];
    load8<FMT>(k_hi, k_lo, off, kv);
    load8<FMT>(v_hi, v_lo, off, vv);
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s += qv[e] * kv[e];
      dp += dov[e] * vv[e];
    }
    s = group8_sum(s);
    dp = group8_sum(dp);
    const float p = __expf(s - L);
    const float ds = p * (dp - delta);
    float dk[8], dv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      dk[e] = ds * qv[e];                    // qv carries the 64^-0.5
      dv[e] = p * dov[e];
      dqa[e] += ds * kv[e];
    }
    const long doff = ((long)b * S + j) * lddkv + h * 64 + sub * 8;
    if (DFMT == 1) {
      *(u32x4_t*)(dk_hi + doff) = f16_grad_piece8(dk);
      *(u32x4_t*)(dv_hi + doff) = f16_grad_piece8(dv);
    } else {
      u32x4_t kh, kl, vh, vl;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t a, b2, c, d;
        split_bf16x2(dk[2 * e], dk[2 * e + 1], a, b2);
        split_bf16x2(dv[2 * e], dv[2 * e + 1], c, d);
        kh[e] = a; kl[e] = b2; vh[e] = c; vl[e] = d;
      }
      *(u32x4_t*)(dk_hi + doff) = kh;
      *(u32x4_t*)(dv_hi + doff) = vh;
      if (dk_lo) *(u32x4_t*)(dk_lo + doff) = kl;
      if (dv_lo) *(u32x4_t*)(dv_lo + doff) = vl;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) sdq[grp][sub * 8 + e] = dqa[e];
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int g = 0; g < 32; ++g) s += sdq[g][threadIdx.x];
    dq[(long)b * D + h * 64 + threadIdx.x] = s * ATTN_SCALE;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int egv_cls_linear_fwd(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int32_t R, int32_t N,
                                  int32_t K, int32_t act, float* z_out, const float* residual, int64_t ldr, float* y, int64_t ldy,
                                  void* stream) {
  if (!x || !W || !y || R <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4 || ldx % 4 || ldw % 4 || ldx < K || ldw < K || ldy < N) return EGV_ERR_ARG;
  if ((act != EGV_ACT_NONE && act != EGV_ACT_GELU) || (residual && ldr < N) || !aligned16(x) || !aligned16(W)) return EGV_ERR_ARG;
  EGV_LAUNCH(cls_linear_fwd_kernel, dim3(N / LIN_CT, (R + LIN_RT - 1) / LIN_RT), dim3(256), 0, (hipStream_t)stream, x, ldx, W, ldw, bias, R, N,
             K, act, z_out, residual, ldr, y, ldy);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int64_t egv_cls_linear_work_floats(int32_t R, int32_t N, int32_t K) {
  if (R <= 0 || N <= 0 || K <= 0) return -1;
  return (int64_t)((N + DG_NS - 1) / DG_NS) * R * K;
}

extern "C" int egv_cls_linear_dgrad(const float* dy, int64_t lddy, const float* W, int64_t ldw, int32_t R, int32_t N, int32_t K, const float* z,
                                    void* dx, int64_t lddx, int32_t dx_mode, float* work, void* stream) {
  if (!dy || !W || !dx || !work || R <= 0 || N <= 0 || K <= 0 || K % 4 || ldw % 4 || ldw < K || lddy < N || lddx < K) return EGV_ERR_ARG;
  if (dx_mode < EGV_CLS_DX_STORE || dx_mode > EGV_CLS_DX_ADD_F16 || !aligned16(W) || !aligned16(work)) return EGV_ERR_ARG;
  const int slabs = (N + DG_NS - 1) / DG_NS;
  const int kz = (K / 4 + 255) / 256;
  EGV_LAUNCH(cls_linear_dgrad_kernel, dim3(slabs, (R + DG_RT - 1) / DG_RT, kz), dim3(256), 0, (hipStream_t)stream, dy, lddy, W, ldw, R, N, K, work);
  EGV_CHECK_LAUNCH();
  const int64_t tot = (int64_t)R * K;
  EGV_LAUNCH(cls_linear_dgrad_finish_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, work, slabs, R, K, z, dx,
             lddx, dx_mode);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_cls_linear_wgrad(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t R, int32_t N, int32_t K, float* dW,
                                    int64_t lddw, float* db, void* stream) {
  if (!dy || !x || !dW || R <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4 || lddy % 4 || ldx % 4 || lddw % 4 || lddy < N || ldx < K || lddw < K)
    return EGV_ERR_ARG;
  if (!aligned16(dy) || !aligned16(x) || !aligned16(dW)) return EGV_ERR_ARG;
  EGV_LAUNCH(cls_linear_wgrad_kernel, dim3(N / 4, (K / 4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, dy, lddy, x, ldx, R, N, K, dW, lddw,
             db);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_cls_rows_add(float* dst, int64_t lddst, const float* src, int64_t ldsrc, int32_t R, int32_t cols, void* stream) {
  if (!dst || !src || R <= 0 || cols <= 0 || lddst < cols || ldsrc < cols) return EGV_ERR_ARG;
  const int64_t tot = (int64_t)R * cols;
  EGV_LAUNCH(cls_rows_add_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, lddst, src, ldsrc, R, cols);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_cls_attn_fwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi,
                                const uint16_t* v_lo, int64_t ldkv, int32_t kv_fmt, int32_t B, int32_t S, int32_t H, float* out, int64_t ldo,
                                float* lse, void* stream) {
  if (!q || !k_hi || !v_hi || !out || !lse || B <= 0 || S <= 0 || H <= 0 || (kv_fmt != EGV_CLS_KV_BF16 && kv_fmt != EGV_CLS_KV_F16)) return EGV_ERR_ARG;
  if (ldkv % 8 || ldkv < (int64_t)H * 64 || ldq < (int64_t)H * 64 || ldo < (int64_t)H * 64 || (k_lo == nullptr) != (v_lo == nullptr))
    return EGV_ERR_ARG;
  if (!aligned16(k_hi) || !aligned16(v_hi) || !aligned16(k_lo) || !aligned16(v_lo)) return EGV_ERR_ARG;
  if (kv_fmt == EGV_CLS_KV_F16)
    EGV_LAUNCH(cls_attn_fwd_kernel<EGV_CLS_KV_F16>, dim3(B * H), dim3(256), 0, (hipStream_t)stream, q, ldq, k_hi, k_lo, v_hi, v_lo, ldkv, S, H, out, ldo, lse);
  else
    EGV_LAUNCH(cls_attn_fwd_kernel<EGV_CLS_KV_BF16>, dim3(B * H), dim3(256), 0, (hipStream_t)stream, q, ldq, k_hi, k_lo, v_hi, v_lo, ldkv, S, H, out, ldo, lse);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_cls_attn_bwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi,
                                const uint16_t* v_lo, int64_t ldkv, int32_t kv_fmt, const float* out, const float* d_out, const float* lse,
                                int32_t B, int32_t S, int32_t H, float* dq, uint16_t* dk_hi, uint16_t* dk_lo, uint16_t* dv_hi, uint16_t* dv_lo,
                                int64_t lddkv, int32_t d_fmt, void* stream) {
  if (!q || !k_hi || !v_hi || !out || !d_out || !lse || !dq || !dk_hi || !dv_hi || B <= 0 || S <= 0 || H <= 0) return EGV_ERR_ARG;
  if ((kv_fmt != EGV_CLS_KV_BF16 && kv_fmt != EGV_CLS_KV_F16) || (d_fmt != EGV_CLS_KV_BF16 && d_fmt != EGV_CLS_KV_F16) || (d_fmt == EGV_CLS_KV_F16 && (dk_lo || dv_lo)))
    return EGV_ERR_ARG;
  if (ldkv % 8 || lddkv % 8 || ldkv < (int64_t)H * 64 || lddkv < (int64_t)H * 64 || ldq < (int64_t)H * 64) return EGV_ERR_ARG;
  if ((k_lo == nullptr) != (v_lo == nullptr) || (dk_lo == nullptr) != (dv_lo == nullptr)) return EGV_ERR_ARG;
  if (!aligned16(k_hi) || !aligned16(v_hi) || !aligned16(k_lo) || !aligned16(v_lo) || !aligned16(dk_hi) || !aligned16(dv_hi) || !aligned16(dk_lo) ||
      !aligned16(dv_lo))
    return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
#define EGV_CLS_BWD(F, DF)                                                                                                              \
  EGV_LAUNCH((cls_attn_bwd_kernel<F, DF>), dim3(B * H), dim3(256), 0, s, q, ldq, k_hi, k_lo, v_hi, v_lo, ldkv, out, d_out, lse, S, H, dq, dk_hi, \
             dk_lo, dv_hi, dv_lo, lddkv)
  if (kv_fmt == EGV_CLS_KV_F16 && d_fmt == EGV_CLS_KV_F16) EGV_CLS_BWD(EGV_CLS_KV_F16, EGV_CLS_KV_F16);
  else if (kv_fmt == EGV_CLS_KV_F16) EGV_CLS_BWD(EGV_CLS_KV_F16, EGV_CLS_KV_BF16);
  else if (d_fmt == EGV_CLS_KV_F16) EGV_CLS_BWD(EGV_CLS_KV_BF16, EGV_CLS_KV_F16);
  else EGV_CLS_BWD(EGV_CLS_KV_BF16, EGV_CLS_KV_BF16);
#undef EGV_CLS_BWD
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
