// Shared by the retrieval kernels (retrieval.hip: egv_rank_scores; recall.hip: egv_gt_ranks / egv_topk_rows): the ordered
// 32-bit key of a similarity and the device-side transpose of a row-major matrix.
#pragma once
#include "common.h"

namespace {

// Ascending key order = descending s; -0.0 and +0.0 share a key (they are equal similarities).  A 64-bit key
//     (ordered_desc32(s) << 32) | column
// ranks by descending similarity with ties by ascending column, and is unique inside a row.
__device__ __forceinline__ uint32_t ordered_desc32(float s) {
  s += 0.0f;                                                     // -0.0 -> +0.0: they are equal similarities
  const uint32_t u = __float_as_uint(s);
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}

// out [cols, rows] = in [rows, cols]^T, 32 x 32 tiles through LDS, 256 threads
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ in, long ldi, int rows, int cols, T* __restrict__ out) {
  __shared__ T tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int y = ty; y < 32; y += 8)
    if (r0 + y < rows && c0 + tx < cols) tile[y][tx] = in[(long)(r0 + y) * ldi + c0 + tx];
  __syncthreads();
  for (int y = ty; y < 32; y += 8)
    if (c0 + y < cols && r0 + tx < rows) out[(long)(c0 + y) * rows + r0 + tx] = tile[tx][y];
}

template <typename T>
int launch_transpose(const T* in, long ldi, int rows, int cols, T* out, hipStream_t s) {
  const int gy = (rows + 31) / 32;
  if (gy > 65535) return EGV_ERR_ARG;
  EGV_LAUNCH((transpose_kernel<T>), dim3((cols + 31) / 32, gy), dim3(256), 0, s, in, ldi, rows, cols, out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

}  // namespace
