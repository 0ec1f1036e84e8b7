// Stochastic depth (timm DropPath, scale_by_keep=True) of the SpaceTimeBlock: model/video_transformer.py:155,171,175 of the reference
// drop a whole residual branch per SAMPLE -- sr = x + s1[b] * attn(..), out = sr + s2[b] * mlp(..), s[b] in {0, 1 / (1 - p)}.
// s[b] is the counter-based mask of common.h with the element index set to the sample number: no table, no stored mask, no host
// synchronisation, and the backward regenerates the forward's draws from (p, seed).  All three kernels are HBM-bound: 16-byte accesses,
// at most 2048 workgroups, a grid-stride loop over the pieces.
#include "common.h"
#include "f16x2.h"
#include "egovlp_hip.h"

namespace {

constexpr int DP_MAX_BLOCKS = 2048;     // 256 CUs x 8 workgroups

__global__ __launch_bounds__(256) void drop_path_scales_kernel(int B, EgvDrop d0, float* __restrict__ out) {
  const EgvDrop d = egv_drop_resolve(d0);
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) out[b] = egv_drop_scale(d, (uint64_t)b);
}

// out[m, :] = resid[m, :] + s[m / rps] * y[m, :]; `out` may be `y` (a thread reads its piece before it writes it).  The product and the
// sum are rounded separately (no FMA contraction): the result is what `resid + s * y` gives in fp32 anywhere, and a dropped sample's
// rows are resid's bits whatever y holds.
__global__ __launch_bounds__(256) void drop_path_add_kernel(const float* y, const float* __restrict__ resid, float* out, int rows,
                                                            int cols, int rps, EgvDrop d0) {
  const EgvDrop d = egv_drop_resolve(d0);
  const int c4 = cols >> 2;
  const int total = rows * c4;                        // < 2^31 (checked by the launcher)
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int r = i / c4, c = (i - r * c4) * 4;
    const float s = egv_drop_scale(d, (uint64_t)(r / rps));      // rps = 1 + T n is odd: a true division per row
    const long off = (long)r * cols + c;
    f32x4_t v = *(const f32x4_t*)(resid + off);
    if (s != 0.f) {
      const f32x4_t t = *(const f32x4_t*)(y + off);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(v[e], __fmul_rn(s, t[e]));
    }
    *(f32x4_t*)(out + off) = v;
  }
}

// planes of s[m / rps] * g[m, :], the product rounded to fp32 first (__fmul_rn also keeps it out of an FMA with the split's
// subtraction): bit for bit what split_transpose_kernel (PASSES 1 / 3: hi[, lo]) and f16_cast_kernel (PASSES 4: one plane of
// un-clamped fp16) write from g * s[:, None].  Eight columns per lane: one 16-byte store per plane.
template <int PASSES>
__global__ __launch_bounds__(256) void drop_path_grad_kernel(const float* __restrict__ g, long ldg, int rows, int cols, int rps,
                                                             EgvDrop d0, unsigned short* __restrict__ hi,
                                                             unsigned short* __restrict__ lo, long ldo) {
  const EgvDrop d = egv_drop_resolve(d0);
  const int c8 = cols >> 3;
  const int total = rows * c8;
  const int stride = gridDim.x * 256;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int r = i / c8, c = (i - r * c8) * 8;
    const float s = egv_drop_scale(d, (uint64_t)(r / rps));
    // a dropped sample's rows are multiplied as well: g * 0 keeps g's sign (and inf / NaN, which the loss scaler must see)
    const f32x4_t a = *(const f32x4_t*)(g + (long)r * ldg + c), b = *(const f32x4_t*)(g + (long)r * ldg + c + 4);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = __fmul_rn(a[e], s);
      v[4 + e] = __fmul_rn(b[e], s);
    }
    const long off = (long)r * ldo + c;
    if (PASSES == 4) {
      *(u32x4_t*)(hi + off) = f16_grad_piece8(v);
    } else {
      bf16_t h[8], l[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) split_bf16(v[e], h[e], l[e]);
      *(u32x4_t*)(hi + off) = (u32x4_t){pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7])};
      if (PASSES == 3) *(u32x4_t*)(lo + off) = (u32x4_t){pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7])};
    }
  }
}

inline unsigned dp_grid(long pieces) {
  const long blocks = (pieces + 255) / 256;
  return (unsigned)(blocks < DP_MAX_BLOCKS ? blocks : DP_MAX_BLOCKS);
}

}  // namespace

extern "C" int egv_drop_path_scales(int32_t B, float p, uint64_t seed, const uint64_t* seed_dev, float* out, void* stream) {
  if (!out || B <= 0 || !(p >= 0.f && p < 1.f)) return EGV_ERR_ARG;
  EGV_LAUNCH(drop_path_scales_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
             egv_make_drop(p, seed, seed_dev), out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_drop_path_add(const float* y, const float* resid, float* out, int32_t rows, int32_t cols, int32_t rows_per_sample,
                                 float p, uint64_t seed, const uint64_t* seed_dev, void* stream) {
  if (!y || !resid || !out || rows <= 0 || cols <= 0 || cols % 4 != 0 || rows_per_sample <= 0 || !(p >= 0.f && p < 1.f)) return EGV_ERR_ARG;
  if ((((size_t)y) | ((size_t)resid) | ((size_t)out)) & 15) return EGV_ERR_ARG;
  const long pieces = (long)rows * (cols / 4);
  if (pieces > 0x7fffffffL - DP_MAX_BLOCKS * 256L) return EGV_ERR_ARG;      // the loop index stays an int32
  EGV_LAUNCH(drop_path_add_kernel, dim3(dp_grid(pieces)), dim3(256), 0, (hipStream_t)stream, y, resid, out, rows, cols,
             rows_per_sample, egv_make_drop(p, seed, seed_dev));
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_drop_path_grad(const float* g, int64_t ldg, int32_t rows, int32_t cols, int32_t rows_per_sample, float p,
                                  uint64_t seed, const uint64_t* seed_dev, int32_t passes, uint16_t* hi, uint16_t* lo, int64_t ldo,
                                  void* stream) {
  if (!g || !hi || rows <= 0 || cols <= 0 || cols % 8 != 0 || rows_per_sample <= 0 || !(p >= 0.f && p < 1.f)) return EGV_ERR_ARG;
  if ((passes != 1 && passes != 3 && passes != 4) || (passes == 3 && !lo)) return EGV_ERR_ARG;
  if (ldg < cols || ldg % 4 != 0 || ldo < cols || ldo % 8 != 0) return EGV_ERR_ARG;
  if ((((size_t)g) | ((size_t)hi) | ((size_t)lo)) & 15) return EGV_ERR_ARG;
  const long pieces = (long)rows * (cols / 8);
  if (pieces > 0x7fffffffL - DP_MAX_BLOCKS * 256L) return EGV_ERR_ARG;
  const EgvDrop d = egv_make_drop(p, seed, seed_dev);
  const dim3 grid(dp_grid(pieces));
  hipStream_t s = (hipStream_t)stream;
  if (passes == 4)
    EGV_LAUNCH(drop_path_grad_kernel<4>, grid, dim3(256), 0, s, g, (long)ldg, rows, cols, rows_per_sample, d, hi, lo, (long)ldo);
  else if (passes == 3)
    EGV_LAUNCH(drop_path_grad_kernel<3>, grid, dim3(256), 0, s, g, (long)ldg, rows, cols, rows_per_sample, d, hi, lo, (long)ldo);
  else
    EGV_LAUNCH(drop_path_grad_kernel<1>, grid, dim3(256), 0, s, g, (long)ldg, rows, cols, rows_per_sample, d, hi, lo, (long)ldo);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
