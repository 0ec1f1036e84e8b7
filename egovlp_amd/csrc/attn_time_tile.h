// Pieces shared by the two time-attention kernels (attn_time_mfma.hip: T <= 16, one 16-row tile per wave; attn_time_long.hip:
// 16 < T <= 64, 2 - 4 tiles per location): the 16-row operand tile and its swizzled LDS image (attn_common.h), the reductions over the
// accumulator layout of a 16x16 tile, the accumulator -> B-operand packing and the staged output rows.
#pragma once
#include "attn_common.h"

namespace {

// ---- one operand tile (16 frame rows of one plane, 128 B each) as two coalesced loads: lane -> (row 8 it + (l >> 3), chunk l & 7)
struct Tile { u32x4_t r[2]; };
__device__ __forceinline__ void put_tile(char* img, const Tile& t, int lane) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = 8 * it + (lane >> 3), chunk = lane & 7;
    *(u32x4_t*)(img + row * ATT_ROW_BYTES + ((chunk ^ (row & 7)) << 4)) = t.r[it];
  }
}

__device__ __forceinline__ float allg_max(float v) {   // over the four lane groups that share a column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float allg_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float row16_sum(float v) {   // over the 16 lanes of a lane group (DPP row)
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
  return v;
}

// row-contraction B operand from a tile pair's accumulator-layout values: elements 0..3 = rows 4g + j of the 16-row tile,
// elements 4..7 = rows 16..19 (the CLS tile: its rows live in lane group 0 only -- the callers pass zeros elsewhere)
template <bool F16 = false>
__device__ __forceinline__ void pack_b(const float (&a)[4], const float (&x)[4], bf16x8_t& hi, bf16x8_t& lo) {
  const float v[8] = {a[0], a[1], a[2], a[3], x[0], x[1], x[2], x[3]};
  att_split8<F16>(v, hi, lo);
}
template <bool F16 = false>
__device__ __forceinline__ void pack_b(const float (&a)[4], float one, bf16x8_t& hi, bf16x8_t& lo) {
  const float x[4] = {one, 0.f, 0.f, 0.f};
  pack_b<F16>(a, x, hi, lo);
}

template <int PASSES, bool F16 = false>
__device__ __forceinline__ f32x4_t mma2(const bf16x8_t (&ah)[2], const bf16x8_t (&al)[2], const bf16x8_t (&bh)[2], const bf16x8_t (&bl)[2]) {
  f32x4_t c = {0.f, 0.f, 0.f, 0.f};
  c = att_mma<PASSES, F16>(ah[0], al[0], bh[0], bl[0], c);
  return att_mma<PASSES, F16>(ah[1], al[1], bh[1], bl[1], c);
}

// ---- output rows through LDS (round 5).  A lane of an output tile owns 4 channels of ONE token row (8 bytes of each plane): stored
// directly, a wave instruction wrote 16 x 32-byte segments of 16 different 128-byte rows, four instructions per row and plane.  The
// 16 x 64 tile of a plane is staged in the wave's own LDS instead (the image layout: 128-B rows, 16-B chunk XOR (row & 7); LDS
// operations of a wave execute in order, so no barrier) and leaves as whole rows: lane -> (row 8 it + (l >> 3), chunk l & 7), one
// 16-byte store per lane, 8 lanes per 128-byte row.  -DEGV_TMF_OLD_STORES: the direct 8-byte stores (A/B builds).
__device__ __forceinline__ void stage4(char* sh, char* sl, int p, int col, const f32x4_t& v, float scale, int fmt = EGV_ATTN_OUT_BF16_SPLIT) {
  uint32_t h0, h1, l0, l1;
  att_out2(v[0] * scale, v[1] * scale, fmt, h0, l0);
  att_out2(v[2] * scale, v[3] * scale, fmt, h1, l1);
  const int off = att_off(p, col);
  *(u32x2_t*)(sh + off) = (u32x2_t){h0, h1};
  if (sl) *(u32x2_t*)(sl + off) = (u32x2_t){l0, l1};
}

}  // namespace
