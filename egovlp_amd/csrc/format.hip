// Format kernels: fp32 <-> split-bf16 planes, transposes (+ column sums = bias gradients) and their multi-tensor table, relu-split,
// the DistilBERT embedding lookup and its backward, elementwise dropout, zero-fill, the ABI check.  All HBM-bound: 16-byte global
// accesses, LDS only for transposes.  The video input path (patch gathers, token assembly, patch dropout) is csrc/video_input.hip.
#include "common.h"
#include "f16x2.h"
#include "egovlp_hip.h"
#include "multi_tensor.h"

namespace {

// ---------------------------------------------------------------------------------------------
// split_f32: one 64x64 tile per block (256 threads).  Reads fp32 rows coalesced (float4), writes the
// row-major planes directly and the transposed planes through a padded LDS tile; column sums are
// block-reduced and accumulated with one atomicAdd per column per block (colsum is zeroed first).
// SRC_PLANES: the source is already a pair of bf16 planes (value = hi + lo) instead of fp32.
template <bool SRC_PLANES>
__device__ __forceinline__ void split_transpose_tile(
    const float* __restrict__ x, const bf16_t* __restrict__ xh, const bf16_t* __restrict__ xl, long ldx, int rows,
    int cols, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, long ldo, bf16_t* __restrict__ thi,
    bf16_t* __restrict__ tlo, long ldt, float* __restrict__ colsum, const int r0, const int c0, const int text,
    unsigned short* __restrict__ t16 = nullptr) {
  // t16 (optional): the transposed matrix as ONE plane of plain fp16 [cols, ldt] -- W^T for the dgrad GEMMs of the fp16 backward
  // text: columns of the transposed planes this tensor owns (>= rows; rows .. text-1 are zero-filled)
  __shared__ float tile[64][65];
  const int tid = threadIdx.x;
  const int tr = tid >> 4;         // 0..15
  const int tc = (tid & 15) * 4;   // 0..60
  float csum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int rr = 0; rr < 64; rr += 16) {
    const int r = r0 + rr + tr, c = c0 + tc;
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (r < rows && c < cols) {  // cols % 4 == 0
      if (SRC_PLANES) {
        const us4_t h = *(const us4_t*)(xh + (long)r * ldx + c);
        us4_t l = {0, 0, 0, 0};
        if (xl) l = *(const us4_t*)(xl + (long)r * ldx + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32(h[e]) + bf16_to_f32(l[e]);
      } else {
        v = *(const f32x4_t*)(x + (long)r * ldx + c);
        if (hi) {
          bf16_t h[4], l[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split_bf16(v[e], h[e], l[e]);
          *(u32x2_t*)(hi + (long)r * ldo + c) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
          if (lo) *(u32x2_t*)(lo + (long)r * ldo + c) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tile[rr + tr][tc + e] = v[e];
      csum[e] += v[e];
    }
  }
  __syncthreads();
  if (colsum) {
    // reduce csum over the 16 row-threads sharing a column group: lanes tid, tid+16, ... (tr varies)
    // use LDS-free approach: every thread adds its partial for its 4 columns via the tile's spare space
    // (simple and cheap: 16-way shuffle-free reduction through atomics on LDS would be slower), so
    // re-read the tile column-wise instead: thread t < 64 sums column t over 64 rows.
    if (tid < 64) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < 64; ++r) s += tile[r][tid];
      if (c0 + tid < cols) atomicAdd(colsum + c0 + tid, s);
    }
  }
  if (t16) {
#pragma unroll
    for (int cc = 0; cc < 64; cc += 16) {
      const int c = c0 + cc + tr, r = r0 + tc;
      if (c < cols && r < text) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (r + e < rows) ? f16x2_clamp(tile[tc + e][cc + tr]) : 0.f;
        *(u32x2_t*)(t16 + (long)c * ldt + r) = (u32x2_t){f16_pk(v[0], v[1]), f16_pk(v[2], v[3])};
      }
    }
  }
  if (thi) {
    // transposed write: output row = column index c, output col = row index r (contiguous over r)
#pragma unroll
    for (int cc = 0; cc < 64; cc += 16) {
      const int c = c0 + cc + tr;   // output row
      const int r = r0 + tc;        // output col start (4 consecutive source rows)
      if (c < cols && r < text) {
        bf16_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = (r + e < rows) ? tile[tc + e][cc + tr] : 0.f;
          split_bf16(v, h[e], l[e]);
        }
        *(u32x2_t*)(thi + (long)c * ldt + r) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
        if (tlo) *(u32x2_t*)(tlo + (long)c * ldt + r) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
      }
    }
  }
}

template <bool SRC_PLANES>
__global__ __launch_bounds__(256) void split_transpose_kernel(
    const float* __restrict__ x, const bf16_t* __restrict__ xh, const bf16_t* __restrict__ xl, long ldx, int rows,
    int cols, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, long ldo, bf16_t* __restrict__ thi,
    bf16_t* __restrict__ tlo, long ldt, float* __restrict__ colsum) {
  split_transpose_tile<SRC_PLANES>(x, xh, xl, ldx, rows, cols, hi, lo, ldo, thi, tlo, ldt, colsum, blockIdx.y * 64,
                                   blockIdx.x * 64, (int)ldt);
}

// The same tile for MANY tensors in one launch (the once-per-optimizer-step refresh of every weight's operand planes:
// ~100 tensors, one ~8 us launch each when done one by one).  Pointer tables travel in the kernel arguments.
constexpr int SPLIT_MAX_T = 40;
struct SplitTable {
  const float* x[SPLIT_MAX_T];
  bf16_t* hi[SPLIT_MAX_T];
  bf16_t* lo[SPLIT_MAX_T];
  bf16_t* thi[SPLIT_MAX_T];
  bf16_t* tlo[SPLIT_MAX_T];
  unsigned short* t16[SPLIT_MAX_T];
  int ldx[SPLIT_MAX_T], ldo[SPLIT_MAX_T], ldt[SPLIT_MAX_T], rows[SPLIT_MAX_T], cols[SPLIT_MAX_T], text[SPLIT_MAX_T];
  int tiles_x[SPLIT_MAX_T];
  MtIndex<SPLIT_MAX_T> ix;
};
static_assert(sizeof(SplitTable) <= 4096, "the table travels in the kernel arguments");

__global__ __launch_bounds__(256) void split_multi_kernel(const SplitTable t) {
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const int ty = w.block / t.tiles_x[ti], tx = w.block - ty * t.tiles_x[ti];
  split_transpose_tile<false>(t.x[ti], nullptr, nullptr, t.ldx[ti], t.rows[ti], t.cols[ti], t.hi[ti], t.lo[ti], t.ldo[ti],
                              t.thi[ti], t.tlo[ti], t.ldt[ti], nullptr, ty * 64, tx * 64, t.text[ti], t.t16[ti]);
}

// relu(x) -> split planes (txt_proj's ReLU, model/model.py:73)
__global__ __launch_bounds__(256) void relu_split_kernel(const float* __restrict__ x, long ldx, int rows, int cols,
                                                         bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, long ldo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c4 = cols / 4;
  if (i >= (long)rows * c4) return;
  const int r = (int)(i / c4), c = (int)(i % c4) * 4;
  f32x4_t v = *(const f32x4_t*)(x + (long)r * ldx + c);
  bf16_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split_bf16(v[e] <= 0.f ? 0.f : v[e], h[e], l[e]);   // not fmaxf: nn.ReLU hands a NaN on, fmaxf(NaN, 0) is 0
  *(u32x2_t*)(hi + (long)r * ldo + c) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
  if (lo) *(u32x2_t*)(lo + (long)r * ldo + c) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
}

__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ word,
                                                        const float* __restrict__ pos, int B, int L, int D,
                                                        float* __restrict__ e) {
  const int D4 = D / 4;
  const long total = (long)B * L * D4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D4) * 4;
  const long t = i / D4;
  const int l = (int)(t % L);
  const long id = ids[t];
  *(f32x4_t*)(e + t * D + d) = *(const f32x4_t*)(word + id * D + d) + *(const f32x4_t*)(pos + (long)l * D + d);
}
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ de,
                                                        int B, int L, int D, long pad_id,
                                                        float* __restrict__ d_word,
                                                        float* __restrict__ d_pos) {
  const long total = (long)B * L * D;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D);
  const long t = i / D;
  const int l = (int)(t % L);
  const float g = de[i];
  if (ids[t] != pad_id) atomicAdd(d_word + ids[t] * D + d, g);  // nn.Embedding(padding_idx): no grad to the pad row
  atomicAdd(d_pos + (long)l * D + d, g);
}

}  // namespace

extern "C" int egv_split_f32(const float* x, int64_t ldx, int32_t rows, int32_t cols, egv_bf16* hi, egv_bf16* lo,
                             int64_t ldo, egv_bf16* t_hi, egv_bf16* t_lo, int64_t ldt, float* colsum, void* stream) {
  if (!x || rows <= 0 || cols <= 0 || cols % 4 != 0) return EGV_ERR_ARG;
  if (t_hi && (ldt < rows || ldt % 4 != 0)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (colsum) {
    if (hipMemsetAsync(colsum, 0, sizeof(float) * cols, s) != hipSuccess) return EGV_ERR_LAUNCH;
  }
  const int row_extent = t_hi ? (int)ldt : rows;  // cover the zero pad of the transposed planes
  dim3 grid((cols + 63) / 64, (row_extent + 63) / 64);
  EGV_LAUNCH(split_transpose_kernel<false>, grid, dim3(256), 0, s, x, nullptr, nullptr, ldx, rows, cols, hi, lo,
                     ldo, t_hi, t_lo, ldt, colsum);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_split_f32_multi_t16(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows,
                                       const int32_t* cols, egv_bf16* const* hi, egv_bf16* const* lo, const int64_t* ldo,
                                       egv_bf16* const* t_hi, egv_bf16* const* t_lo, const int64_t* ldt, const int32_t* t_cols,
                                       uint16_t* const* t16, void* stream);
extern "C" int egv_split_f32_multi(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows,
                                   const int32_t* cols, egv_bf16* const* hi, egv_bf16* const* lo, const int64_t* ldo,
                                   egv_bf16* const* t_hi, egv_bf16* const* t_lo, const int64_t* ldt, const int32_t* t_cols,
                                   void* stream) {
  return egv_split_f32_multi_t16(count, x, ldx, rows, cols, hi, lo, ldo, t_hi, t_lo, ldt, t_cols, nullptr, stream);
}

extern "C" int egv_split_f32_multi_t16(int32_t count, const float* const* x, const int64_t* ldx, const int32_t* rows,
                                       const int32_t* cols, egv_bf16* const* hi, egv_bf16* const* lo, const int64_t* ldo,
                                       egv_bf16* const* t_hi, egv_bf16* const* t_lo, const int64_t* ldt, const int32_t* t_cols,
                                       uint16_t* const* t16, void* stream) {
  if (count < 0 || !x || !ldx || !rows || !cols || !hi || !lo || !ldo || !t_hi || !t_lo || !ldt || !t_cols) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  auto t16_of = [&](int i) -> unsigned short* { return t16 ? t16[i] : nullptr; };
  // rows of the tile grid: with transposed planes, this tensor's share of their zero pad is covered too
  auto row_extent = [&](int i) -> int { return (t_hi[i] || t16_of(i)) ? t_cols[i] : rows[i]; };
  return mt_for_each_launch<SplitTable>(
      count,
      [&](int i) -> int64_t {
        const bool has_t = t_hi[i] || t16_of(i);
        if (!x[i] || rows[i] <= 0 || cols[i] <= 0 || cols[i] % 4 != 0 || (!hi[i] && !has_t)) return -1;
        if (has_t && (ldt[i] < rows[i] || ldt[i] % 4 != 0 || t_cols[i] < rows[i] || t_cols[i] > ldt[i] || t_cols[i] % 4 != 0)) return -1;
        if (ldx[i] > 0x7fffffff || ldo[i] > 0x7fffffff || ldt[i] > 0x7fffffff) return -1;
        return pieces(cols[i], 64) * pieces(row_extent(i), 64);
      },
      [&](SplitTable& t, int k, int i) {
        t.x[k] = x[i]; t.hi[k] = hi[i]; t.lo[k] = lo[i]; t.thi[k] = t_hi[i]; t.tlo[k] = t_lo[i];
        t.ldx[k] = (int)ldx[i]; t.ldo[k] = (int)ldo[i]; t.ldt[k] = (int)ldt[i]; t.rows[k] = rows[i]; t.cols[k] = cols[i]; t.text[k] = row_extent(i);
        t.t16[k] = t16_of(i);
        t.tiles_x[k] = (cols[i] + 63) / 64;
      },
      [&](const SplitTable& t, int nb) -> int {
        EGV_LAUNCH(split_multi_kernel, dim3(nb), dim3(256), 0, s, t);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}

extern "C" int egv_transpose_planes(const egv_bf16* hi, const egv_bf16* lo, int64_t ldx, int32_t rows, int32_t cols,
                                    egv_bf16* t_hi, egv_bf16* t_lo, int64_t ldt, float* colsum, void* stream) {
  if (!hi || rows <= 0 || cols <= 0 || cols % 4 != 0) return EGV_ERR_ARG;
  if (t_hi && (ldt < rows || ldt % 4 != 0)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (colsum) {
    if (hipMemsetAsync(colsum, 0, sizeof(float) * cols, s) != hipSuccess) return EGV_ERR_LAUNCH;
  }
  const int row_extent = t_hi ? (int)ldt : rows;
  dim3 grid((cols + 63) / 64, (row_extent + 63) / 64);
  EGV_LAUNCH(split_transpose_kernel<true>, grid, dim3(256), 0, s, nullptr, hi, lo, ldx, rows, cols, nullptr,
                     nullptr, 0, t_hi, t_lo, ldt, colsum);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_relu_split(const float* x, int64_t ldx, int32_t rows, int32_t cols, egv_bf16* hi, egv_bf16* lo,
                              int64_t ldo, void* stream) {
  if (!x || !hi || cols % 4 != 0) return EGV_ERR_ARG;
  const long total = (long)rows * (cols / 4);
  EGV_LAUNCH(relu_split_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, ldx, rows,
                     cols, hi, lo, ldo);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_embed_fwd(const int64_t* ids, const float* word, const float* pos, int32_t B, int32_t L, int32_t D,
                             float* e, void* stream) {
  if (!ids || !word || !pos || !e || D % 4 != 0) return EGV_ERR_ARG;
  const long total = (long)B * L * (D / 4);
  EGV_LAUNCH(embed_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, word, pos, B,
                     L, D, e);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_embed_bwd(const int64_t* ids, const float* d_e, int32_t B, int32_t L, int32_t D, int64_t pad_id,
                             float* d_word, float* d_pos, void* stream) {
  if (!ids || !d_e || !d_word || !d_pos) return EGV_ERR_ARG;
  const long total = (long)B * L * D;
  EGV_LAUNCH(embed_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, d_e, B, L, D,
                     (long)pad_id, d_word, d_pos);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_version(void) { return EGV_ABI_VERSION; }
extern "C" int egv_abi_check(int32_t abi_version, int64_t sizeof_gemm_desc, int64_t sizeof_block_geom, int64_t sizeof_block_params,
                             int64_t sizeof_block_bwd_io) {
  return (abi_version == EGV_ABI_VERSION && sizeof_gemm_desc == (int64_t)sizeof(egv_gemm_desc) &&
          sizeof_block_geom == (int64_t)sizeof(egv_block_geom) && sizeof_block_params == (int64_t)sizeof(egv_block_params) &&
          sizeof_block_bwd_io == (int64_t)sizeof(egv_block_bwd_io)) ? 0 : 1;
}


// ---- elementwise dropout (DistilBERT embedding / FFN dropout, HF modeling_distilbert.py Embeddings.forward, FFN.ff_chunk) -------
// out[i] = x[i] * M'(i) + (add ? add[i] : 0), M' = keep ? 1 / (1 - p) : 0 from the counter-based mask of common.h.  The SAME
// call with x = dy is the backward (the mask is regenerated from (p, seed)); `add` fuses the residual of `LN(ffn(x) + x)`.
namespace {
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, const float* __restrict__ add,
                                                      float* __restrict__ out, long n, EgvDrop d0) {
  const EgvDrop d = egv_drop_resolve(d0);
  const long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 + 3 < n) {
    f32x4_t v = *(const f32x4_t*)(x + i4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= egv_drop_scale(d, (uint64_t)(i4 + e));
    if (add) v += *(const f32x4_t*)(add + i4);
    *(f32x4_t*)(out + i4) = v;
  } else {
    for (long i = i4; i < n; ++i) out[i] = x[i] * egv_drop_scale(d, (uint64_t)i) + (add ? add[i] : 0.f);
  }
}
}  // namespace

extern "C" int egv_dropout(const float* x, const float* add, float* out, int64_t n, float p, uint64_t seed,
                           const uint64_t* seed_dev, void* stream) {
  if (!x || !out || n <= 0 || !(p >= 0.f && p < 1.f)) return EGV_ERR_ARG;
  if ((((size_t)x) | ((size_t)out) | ((size_t)add)) & 15) return EGV_ERR_ARG;
  const long blocks = (n / 4 + 256) / 256;
  EGV_LAUNCH(dropout_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, add, out, (long)n, egv_make_drop(p, seed, seed_dev));
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// Zero-fill of a freshly allocated buffer (embedding-gradient tables, the dense CLS-only gradient of the final LayerNorm) as a
// memset node of the HIP runtime on the caller's stream -- not an ATen fill kernel.
extern "C" int egv_zero(void* p, int64_t bytes, void* stream) {
  if (!p || bytes < 0) return EGV_ERR_ARG;
  if (bytes == 0) return EGV_OK;
  const hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, (hipStream_t)stream);
  return e == hipSuccess ? EGV_OK : EGV_ERR_LAUNCH + (int)e;
}
