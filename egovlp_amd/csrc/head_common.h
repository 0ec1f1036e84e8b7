// Pieces shared by the contrastive and ranking heads (egonce.hip, egonce_long.hip, sigmoid_head.hip through egonce_tile.h,
// maxmargin_head.hip): the 256-thread block reductions, the backward of the row normalisation and the scale-gradient kernel.
#pragma once
#include "common.h"

namespace {

// 256 threads, fixed order: a lane-xor tree inside each wave, then waves 0..3 through LDS.  sh: [4] floats
__device__ __forceinline__ float egv_block_sum_256(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ __forceinline__ float egv_block_max_256(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// through t / max(|t|, eps): (g - a <a, g>) / |t| above the clamp, g / eps below it.  g: the gradient w.r.t. the normalised row,
// a: the normalised row, proj = <a, g> over the whole row, nrm = |t| unclamped.  T: float or f32x4_t
template <typename T>
__device__ __forceinline__ T egv_norm_bwd(T g, T a, float proj, float nrm, float eps) {
  return nrm > eps ? (g - a * proj) / nrm : g / eps;
}

// dL/d(logit scale) = sum of `count` fp32 partials; one workgroup, double, fixed order.  A kernel in a header is emitted into every
// file that includes it, launched or not: only the files that launch it (egonce.hip, egonce_long.hip) define EGV_SCALE_GRAD_KERNEL.
#ifdef EGV_SCALE_GRAD_KERNEL
__global__ __launch_bounds__(256) void egv_scale_grad_kernel(const float* __restrict__ part, int count,
                                                             float* __restrict__ d_logit_scale) {
  __shared__ double red[256];
  const double s = egv_sum_partials_256(part, count, red);
  if (threadIdx.x == 0) d_logit_scale[0] = (float)s;
}
#endif

}  // namespace
