// Format kernels: fp32 <-> split-bf16 planes, transposes (+ column sums = bias gradients),
// patch gather, token assembly, and both over the kept patches of patch dropout (the egv_*_sel entry points and the draw of their
// table, at the end of the file).  All HBM-bound: 16-byte global accesses, LDS only for transposes and the draw's keys.
#include "common.h"
#include "f16x2.h"
#include "egovlp_hip.h"

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
  int blk_start[SPLIT_MAX_T + 1];
  int count;
};

__global__ __launch_bounds__(256) void split_multi_kernel(const SplitTable t) {
  int ti = 0;
  while (ti + 1 < t.count && (int)blockIdx.x >= t.blk_start[ti + 1]) ++ti;
  const int local = (int)blockIdx.x - t.blk_start[ti];
  const int ty = local / t.tiles_x[ti], tx = local - ty * t.tiles_x[ti];
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
  for (int e = 0; e < 4; ++e) split_bf16(fmaxf(v[e], 0.f), h[e], l[e]);
  *(u32x2_t*)(hi + (long)r * ldo + c) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
  if (lo) *(u32x2_t*)(lo + (long)r * ldo + c) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
}

// ---------------------------------------------------------------------------------------------
// patch gather (im2col for a PxP / stride P conv): one thread moves G consecutive pixels of one patch row (G = 4 when
// P % 4 == 0 -- ViT-B/16 -- else 2 -- ViT-L/14).  Source rows are W*4 B contiguous, so a wave reads one image row
// segment: coalesced.  Columns K .. lda-1 of the output planes (K padded to the GEMM's k-tile) are left untouched:
// the caller zero-fills them once.
struct PatchNorm { float mean[4], std[4]; };   // per-channel Normalize constants of the uint8 path (C <= 4)

template <int G, bool U8>
__global__ __launch_bounds__(256) void patch_gather_kernel(const void* __restrict__ video_, int BT, int C, int H, int W,
                                                           int P, bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo,
                                                           long lda, const PatchNorm nrm) {
  // thread -> (image bt, channel c, image row y, G-pixel group xg)
  const int WG = W / G;
  const long total = (long)BT * C * H * WG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xg = (int)(i % WG);
  long t = i / WG;
  const int y = (int)(t % H);
  t /= H;
  const int c = (int)(t % C);
  const int bt = (int)(t / C);
  const long soff = (((long)bt * C + c) * H + y) * W + xg * G;
  float v[G];
  if (U8) {
    // decoded frames as they come off the decoder (uint8): ToTensor's x / 255 and Normalize's (x - mean) / std happen here,
    // in that order and in fp32 with IEEE division = bit-identical to the host transform (data_loader/transforms.py:38-39,
    // base/base_dataset.py read_frames `/ 255`); the H2D copy and the HBM read are 4x smaller
    const unsigned char* src = (const unsigned char*)video_ + soff;
    const float mu = nrm.mean[c], sd = nrm.std[c];
    unsigned bits;
    if (G == 4) bits = *(const unsigned*)src;
    else bits = *(const unsigned short*)src;
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = ((float)((bits >> (8 * e)) & 0xffu) / 255.0f - mu) / sd;
  } else {
    const float* src = (const float*)video_ + soff;
    if (G == 4) {
      const f32x4_t q = *(const f32x4_t*)src;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
      v[0] = src[0]; v[1] = src[1];
    }
  }
  const int gw = W / P, gh = H / P;
  const int py = y / P, iy = y % P;
  const int x = xg * G;
  const int px = x / P, ix = x % P;
  const long row = ((long)bt * gh + py) * gw + px;
  const int col = (c * P + iy) * P + ix;
  bf16_t h[G], l[G];
#pragma unroll
  for (int e = 0; e < G; ++e) split_bf16(v[e], h[e], l[e]);
  if (G == 4) {
    *(u32x2_t*)(ahi + row * lda + col) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
    if (alo) *(u32x2_t*)(alo + row * lda + col) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
  } else {
    *(uint32_t*)(ahi + row * lda + col) = pack2(h[0], h[1]);
    if (alo) *(uint32_t*)(alo + row * lda + col) = pack2(l[0], l[1]);
  }
}

// x[b, s, :] for s = 0: cls + pos[0]; s = 1 + f*n + i: pe[(b*T+f)*n + i] + pos[1+i] + temporal[f]
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                              const float* __restrict__ pos,
                                                              const float* __restrict__ temporal, int B, int T, int n,
                                                              int D, float* __restrict__ x) {
  const int D4 = D / 4;
  const long S = 1 + (long)T * n;
  const long total = (long)B * S * D4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D4) * 4;
  const long tok = i / D4;
  const int s = (int)(tok % S);
  const int b = (int)(tok / S);
  f32x4_t v;
  if (s == 0) {
    v = *(const f32x4_t*)(cls + d) + *(const f32x4_t*)(pos + d);
  } else {
    const int f = (s - 1) / n, ii = (s - 1) % n;
    v = *(const f32x4_t*)(pe + (((long)b * T + f) * n + ii) * D + d) + *(const f32x4_t*)(pos + (long)(1 + ii) * D + d) +
        *(const f32x4_t*)(temporal + (long)f * D + d);
  }
  *(f32x4_t*)(x + tok * D + d) = v;
}

// backward: d_pe gather + reductions for d_cls, d_pos, d_temporal.
// grid.x = D/256-ish column blocks; each thread owns one channel d and loops over tokens it reduces.
// d_pos[1+i, d]  = sum_{b,f} dx[b, 1+f*n+i, d];  d_pos[0,d] = d_cls[d] = sum_b dx[b,0,d]
// d_temporal[f,d] = sum_{b,i} dx[b, 1+f*n+i, d]
__global__ __launch_bounds__(256) void assemble_bwd_pos_kernel(const float* __restrict__ dx, int B, int T, int n, int D,
                                                               float* __restrict__ d_pos, float* __restrict__ d_cls) {
  // grid (n + 1 position rows, SL slices of the (b, f) rows); threads over 4-channel pieces; every block adds its slice's
  // partial sum with one atomicAdd per channel (d_pos / d_cls zeroed by the launcher).  The first version walked all B*T rows
  // of a position in one block with 4-byte loads: 197 blocks, 186 us for 77 MB.
  const int p = blockIdx.x;
  const long S = 1 + (long)T * n;
  const int rows = (p == 0) ? B : B * T;
  auto tok_of = [&](int r) -> long { return (p == 0) ? (long)r * S : (long)(r / T) * S + 1 + (long)(r % T) * n + (p - 1); };
  for (int d4 = threadIdx.x; d4 < D / 4; d4 += blockDim.x) {
    // four independent row streams per thread (the loads of a 3-KiB row are 600 KB apart: latency-bound unless several are in
    // flight), and only gridDim.y = 4 slices per position: the 2.4 M fp32 atomics of the 16-slice version were what the 193 us of
    // this kernel went into (profiles/r02_zz_kernel_stats_timed_mixed.csv)
    f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int r = blockIdx.y;
    const int st = gridDim.y;
    for (; r + 3 * st < rows; r += 4 * st) {
      const f32x4_t a = *(const f32x4_t*)(dx + tok_of(r) * D + d4 * 4);
      const f32x4_t b = *(const f32x4_t*)(dx + tok_of(r + st) * D + d4 * 4);
      const f32x4_t c = *(const f32x4_t*)(dx + tok_of(r + 2 * st) * D + d4 * 4);
      const f32x4_t d = *(const f32x4_t*)(dx + tok_of(r + 3 * st) * D + d4 * 4);
      s0 += a; s1 += b; s2 += c; s3 += d;
    }
    for (; r < rows; r += st) s0 += *(const f32x4_t*)(dx + tok_of(r) * D + d4 * 4);
    const f32x4_t s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      atomicAdd(d_pos + (long)p * D + d4 * 4 + e, s[e]);
      if (p == 0) atomicAdd(d_cls + d4 * 4 + e, s[e]);
    }
  }
}
__global__ __launch_bounds__(256) void assemble_bwd_temporal_kernel(const float* __restrict__ dx, int B, int T, int n,
                                                                    int D, int T_model, float* __restrict__ d_temporal) {
  // grid (T, ceil(D/64), slices); block 256 = 4 row-groups x 64 channels over this slice's (b, i) rows; LDS reduce over
  // the 4 groups, one atomicAdd per channel per block into d_temporal (zeroed by the launcher, rows >= T stay zero).
  __shared__ float red[4][64];
  const int f = blockIdx.x;
  const int d = blockIdx.y * 64 + (threadIdx.x & 63);
  const int g = threadIdx.x >> 6;
  const long S = 1 + (long)T * n;
  float s = 0.f;
  if (d < D) {
    for (int bi = blockIdx.z * 4 + g; bi < B * n; bi += 4 * gridDim.z) {
      const int b = bi / n, i = bi % n;
      s += dx[((long)b * S + 1 + (long)f * n + i) * D + d];
    }
  }
  red[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && d < D)
    atomicAdd(d_temporal + (long)f * D + d, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void assemble_bwd_pe_kernel(const float* __restrict__ dx, int B, int T, int n, int D,
                                                              float* __restrict__ d_pe) {
  const int D4 = D / 4;
  const long total = (long)B * T * n * D4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D4) * 4;
  const long r = i / D4;  // (b*T+f)*n + ii
  const long b = r / ((long)T * n);
  const long rem = r % ((long)T * n);
  const long S = 1 + (long)T * n;
  *(f32x4_t*)(d_pe + r * D + d) = *(const f32x4_t*)(dx + (b * S + 1 + rem) * D + d);
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
  SplitTable t;
  int nt = 0, nb = 0;
  auto flush = [&]() -> int {
    if (nt == 0) return EGV_OK;
    t.blk_start[nt] = nb;
    t.count = nt;
    EGV_LAUNCH(split_multi_kernel, dim3(nb), dim3(256), 0, s, t);
    EGV_CHECK_LAUNCH();
    nt = 0;
    nb = 0;
    return EGV_OK;
  };
  for (int i = 0; i < count; ++i) {
    unsigned short* const tf = t16 ? t16[i] : nullptr;
    const bool has_t = t_hi[i] || tf;
    if (!x[i] || rows[i] <= 0 || cols[i] <= 0 || cols[i] % 4 != 0 || (!hi[i] && !has_t)) return EGV_ERR_ARG;
    if (has_t && (ldt[i] < rows[i] || ldt[i] % 4 != 0 || t_cols[i] < rows[i] || t_cols[i] > ldt[i] || t_cols[i] % 4 != 0)) return EGV_ERR_ARG;
    if (ldx[i] > 0x7fffffff || ldo[i] > 0x7fffffff || ldt[i] > 0x7fffffff) return EGV_ERR_ARG;
    if (nt == SPLIT_MAX_T) {
      const int rc = flush();
      if (rc) return rc;
    }
    const int row_extent = has_t ? t_cols[i] : rows[i];   // cover this tensor's share of the zero pad of the transposed planes
    const int tx = (cols[i] + 63) / 64, ty = (row_extent + 63) / 64;
    t.x[nt] = x[i]; t.hi[nt] = hi[i]; t.lo[nt] = lo[i]; t.thi[nt] = t_hi[i]; t.tlo[nt] = t_lo[i];
    t.ldx[nt] = (int)ldx[i]; t.ldo[nt] = (int)ldo[i]; t.ldt[nt] = (int)ldt[i]; t.rows[nt] = rows[i]; t.cols[nt] = cols[i]; t.text[nt] = has_t ? t_cols[i] : rows[i];
    t.t16[nt] = tf;
    t.tiles_x[nt] = tx;
    t.blk_start[nt] = nb;
    nb += tx * ty;
    ++nt;
  }
  return flush();
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

template <bool U8>
static int patch_gather_launch(const void* video, int BT, int C, int H, int W, int P, egv_bf16* a_hi, egv_bf16* a_lo,
                               int64_t lda, const PatchNorm& nrm, void* stream) {
  if (!video || !a_hi || P % 2 != 0 || W % P != 0 || H % P != 0 || lda % 2 != 0) return EGV_ERR_ARG;
  if (P % 4 == 0) {
    const long total = (long)BT * C * H * (W / 4);
    EGV_LAUNCH((patch_gather_kernel<4, U8>), dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, video, BT, C, H, W,
               P, a_hi, a_lo, lda, nrm);
  } else {
    const long total = (long)BT * C * H * (W / 2);
    EGV_LAUNCH((patch_gather_kernel<2, U8>), dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, video, BT, C, H, W,
               P, a_hi, a_lo, lda, nrm);
  }
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_patch_gather(const float* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                                egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  return patch_gather_launch<false>(video, BT, C, H, W, P, a_hi, a_lo, lda, PatchNorm{}, stream);
}

extern "C" int egv_patch_gather_u8(const uint8_t* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                                   const float* mean, const float* std, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda,
                                   void* stream) {
  if (!mean || !std || C < 1 || C > 4) return EGV_ERR_ARG;
  PatchNorm nrm{};
  for (int c = 0; c < C; ++c) {
    if (!(std[c] > 0.f)) return EGV_ERR_ARG;
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  return patch_gather_launch<true>(video, BT, C, H, W, P, a_hi, a_lo, lda, nrm, stream);
}

extern "C" int egv_assemble_tokens(const float* pe, const float* cls, const float* pos, const float* temporal,
                                   int32_t B, int32_t T, int32_t n, int32_t D, float* x, void* stream) {
  if (!pe || !cls || !pos || !temporal || !x || D % 4 != 0) return EGV_ERR_ARG;
  const long total = (long)B * (1 + (long)T * n) * (D / 4);
  EGV_LAUNCH(assemble_tokens_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, pe, cls,
                     pos, temporal, B, T, n, D, x);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_assemble_tokens_bwd(const float* dx, int32_t B, int32_t T, int32_t n, int32_t D, int32_t T_model,
                                       float* d_pe, float* d_cls, float* d_pos, float* d_temporal, void* stream) {
  if (!dx || D % 4 != 0 || T > T_model) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (d_pos && d_cls) {
    if (hipMemsetAsync(d_pos, 0, sizeof(float) * (size_t)(n + 1) * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    if (hipMemsetAsync(d_cls, 0, sizeof(float) * (size_t)D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    EGV_LAUNCH(assemble_bwd_pos_kernel, dim3(n + 1, 4), dim3(256), 0, s, dx, B, T, n, D, d_pos, d_cls);
    EGV_CHECK_LAUNCH();
  }
  if (d_temporal) {
    if (hipMemsetAsync(d_temporal, 0, sizeof(float) * (size_t)T_model * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    EGV_LAUNCH(assemble_bwd_temporal_kernel, dim3(T, (D + 63) / 64, 32), dim3(256), 0, s, dx, B, T, n, D, T_model,
               d_temporal);
    EGV_CHECK_LAUNCH();
  }
  if (d_pe) {
    const long total = (long)B * T * n * (D / 4);
    EGV_LAUNCH(assemble_bwd_pe_kernel, dim3((total + 255) / 256), dim3(256), 0, s, dx, B, T, n, D, d_pe);
    EGV_CHECK_LAUNCH();
  }
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

// ---- train-time augmentation fused into the patch gather (data_loader/transforms.py:14-19: RandomResizedCrop(
// input_res, scale) -> RandomHorizontalFlip -> ColorJitter(0, 0, 0) = identity -> Normalize) -----------------------------------
// The loader hands over the DECODED uint8 clip [B*T, C, Hs, Ws] and five ints per clip -- the crop box (top, left, h, w) and a
// flip flag, the random draws of the host transform (one box per clip: the reference applies the transform to the [T, C, H, W]
// tensor as a whole).  Every output pixel of the R x R frame is sampled here: x / 255 first (the reference resizes float frames),
// bilinear with align_corners = False semantics (source index (o + 0.5) * size / R - 0.5 clamped at 0, right / bottom neighbour
// clamped to the box), mirrored when flipped, normalised, split and written straight into the im2col planes of the patch-embed
// GEMM.  No resized fp32 clip ever exists in HBM (the host transform writes 4 x 3 x 224 x 224 floats per clip and the H2D
// copy carries them).
namespace {
struct AugBox { int top, left, h, w, flip; };
// Four consecutive pixels (x .. x + 3 of row y, channel c) of output frame bt -> the im2col planes of an R x R frame cut into P x P
// patches: one 8-byte store per plane where the group lies inside one patch (P % 4 == 0: always), element-wise where it straddles
// two (P = 14).
__device__ __forceinline__ void store_patch4(const float (&v)[4], int bt, int c, int y, int x, int R, int P,
                                             bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda) {
  const int gw = R / P;
  const int py = y / P, iy = y % P;
  const int px = x / P, ix = x % P;
  const long row = ((long)bt * gw + py) * gw + px;
  const int col = (c * P + iy) * P + ix;
  if (ix + 3 < P) {
    uint32_t h0, h1, l0, l1;
    split_bf16x2(v[0], v[1], h0, l0);
    split_bf16x2(v[2], v[3], h1, l1);
    if (((row * lda + col) & 3) == 0) {
      *(u32x2_t*)(ahi + row * lda + col) = (u32x2_t){h0, h1};
      if (alo) *(u32x2_t*)(alo + row * lda + col) = (u32x2_t){l0, l1};
    } else {
      *(uint32_t*)(ahi + row * lda + col) = h0;
      *(uint32_t*)(ahi + row * lda + col + 2) = h1;
      if (alo) {
        *(uint32_t*)(alo + row * lda + col) = l0;
        *(uint32_t*)(alo + row * lda + col + 2) = l1;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int xe = x + e;
      const long rw = ((long)bt * gw + py) * gw + xe / P;
      const int cl = (c * P + iy) * P + xe % P;
      bf16_t h, l;
      split_bf16(v[e], h, l);
      ahi[rw * lda + cl] = h;
      if (alo) alo[rw * lda + cl] = l;
    }
  }
}
// One output row of the resized crop of frame bt, channel c: the clamped box, the two source rows behind output row y and the
// Normalize constants.  pixel(ox) is output pixel ox of that row, normalised.
struct AugRow {
  const unsigned char *r0, *r1;
  float ly, sx, mu, sd;
  int bw, flip, R;
  __device__ __forceinline__ AugRow(const unsigned char* __restrict__ video, const int* __restrict__ boxes, int bt, int T, int C, int c,
                                    int Hs, int Ws, int R_, int y, const PatchNorm& nrm) {
    const int* bx = boxes + (long)(bt / T) * 5;
    // a box that leaves the frame is CLAMPED into it (the host validates boxes it can see, model/video_transformer.py
    // set_input_augmentation; a device-resident box cannot be checked without a sync): no read below can leave the clip
    const int top = min(max(bx[0], 0), Hs - 1), left = min(max(bx[1], 0), Ws - 1);
    const int bh = min(max(bx[2], 1), Hs - top);
    bw = min(max(bx[3], 1), Ws - left);
    flip = bx[4];
    R = R_;
    const unsigned char* src = video + ((long)bt * C + c) * Hs * Ws;
    const float sy = (float)bh / (float)R;
    sx = (float)bw / (float)R;
    float fy = ((float)y + 0.5f) * sy - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    const int y0 = (int)fy;
    const int y1 = y0 + (y0 < bh - 1 ? 1 : 0);
    ly = fy - (float)y0;
    r0 = src + (long)(top + y0) * Ws + left;
    r1 = src + (long)(top + y1) * Ws + left;
    mu = nrm.mean[c];
    sd = nrm.std[c];
  }
  __device__ __forceinline__ float pixel(int ox) const {
    const int sxi = flip ? R - 1 - ox : ox;               // RandomHorizontalFlip acts on the resized crop
    float fx = ((float)sxi + 0.5f) * sx - 0.5f;
    fx = fx < 0.f ? 0.f : fx;
    const int x0 = (int)fx;
    const int x1 = x0 + (x0 < bw - 1 ? 1 : 0);
    const float lx = fx - (float)x0;
    const float p00 = (float)r0[x0] / 255.0f, p01 = (float)r0[x1] / 255.0f;
    const float p10 = (float)r1[x0] / 255.0f, p11 = (float)r1[x1] / 255.0f;
    const float val = (1.0f - ly) * ((1.0f - lx) * p00 + lx * p01) + ly * ((1.0f - lx) * p10 + lx * p11);
    return (val - mu) / sd;
  }
};
__global__ __launch_bounds__(256) void patch_gather_aug_kernel(const unsigned char* __restrict__ video, int BT, int T, int C,
                                                               int Hs, int Ws, int R, int P, const int* __restrict__ boxes,
                                                               bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda,
                                                               const PatchNorm nrm) {
  // thread -> (image bt, channel c, output row y, 4-pixel group xg)
  const int WG = R / 4;
  const long total = (long)BT * C * R * WG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xg = (int)(i % WG);
  long t = i / WG;
  const int y = (int)(t % R);
  t /= R;
  const int c = (int)(t % C);
  const int bt = (int)(t / C);
  const AugRow row(video, boxes, bt, T, C, c, Hs, Ws, R, y, nrm);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = row.pixel(xg * 4 + e);
  store_patch4(v, bt, c, y, xg * 4, R, P, ahi, alo, lda);
}
}  // namespace

extern "C" int egv_patch_gather_u8_aug(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                       int32_t R, int32_t P, const int32_t* boxes, const float* mean, const float* std,
                                       egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  if (!video || !boxes || !a_hi || !mean || !std || BT <= 0 || T <= 0 || BT % T != 0 || C <= 0 || C > 4) return EGV_ERR_ARG;
  if (Hs <= 0 || Ws <= 0 || R <= 0 || P <= 0 || R % P != 0 || R % 4 != 0 || P % 2 != 0 || lda % 2 != 0) return EGV_ERR_ARG;
  PatchNorm nrm{};
  for (int c = 0; c < C; ++c) {
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  const long total = (long)BT * C * R * (R / 4);
  EGV_LAUNCH(patch_gather_aug_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, video, BT, T, C, Hs,
             Ws, R, P, boxes, a_hi, a_lo, (long)lda, nrm);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ---- val / test transform fused into the patch gather (data_loader/transforms.py:49-60: Resize(S) -> CenterCrop(S) -> Resize(R) ->
// Normalize, on x / 255; bilinear, align_corners = False, no antialias -- the tensor path of torchvision 0.13) ----------------------
// The decoded uint8 frame bank [F, C, Hs, Ws] stays as it is; output frame bt reads bank frame index[bt] (clamped into the bank), so
// a window of T frames is T entries of a table: overlapping, sub-sampled and ragged batches of windows cost no copy.  Every output
// pixel is a bilinear sample (stage 2, S x S -> R x R) of four pixels of the centre crop of the stage-1 image, and each of those is
// itself a bilinear sample (stage 1, Hs x Ws -> H1 x W1) of four source bytes: 16 byte loads per output pixel, 4 where stage 1 is
// the identity (short side == S, the ego4d_256 frames).  Neither the H1 x W1 nor the R x R fp32 frame ever exists in memory.
// Per 256 x 341 -> 224 frame 197 KB of the 262 KB source are touched once from HBM and 602 KB of planes (two bf16 planes of
// 196 x 768) are written.  Bound: not HBM (1.2 TB/s of that traffic measured) but instruction issue -- the dependent
// byte loads with their address arithmetic and the IEEE divisions that keep x / 255 and / std bit-compatible with the uint8 gather.
namespace {
struct LinTap { int i0, i1; float l; };
// source taps of output index o of a bilinear resize n_in -> n_out (scale = (float)n_in / n_out), align_corners = False
__device__ __forceinline__ LinTap lin_tap(int o, float scale, int n_in) {
  float f = ((float)o + 0.5f) * scale - 0.5f;
  f = f < 0.f ? 0.f : f;
  const int i0 = min((int)f, n_in - 1);            // f < n_in by construction; the clamp makes it independent of rounding
  LinTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  t.l = f - (float)i0;
  return t;
}
__device__ __forceinline__ float bilerp(float ly, float lx, float p00, float p01, float p10, float p11) {
  return (1.0f - ly) * ((1.0f - lx) * p00 + lx * p01) + ly * ((1.0f - lx) * p10 + lx * p11);
}
struct EvalGeom { int F, BT, C, Hs, Ws, H1, W1, top, left, S, R, P; };

template <bool IDENT>   // IDENT: stage 1 is the identity (H1 == Hs, W1 == Ws)
__global__ __launch_bounds__(256) void patch_gather_eval_kernel(const unsigned char* __restrict__ frames,
                                                                const int* __restrict__ index, const EvalGeom g,
                                                                bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda,
                                                                const PatchNorm nrm) {
  // thread -> (output frame bt, channel c, output row y, 4-pixel group xg)
  const int R = g.R, WG = R / 4;
  const long total = (long)g.BT * g.C * R * WG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xg = (int)(i % WG);
  long t = i / WG;
  const int y = (int)(t % R);
  t /= R;
  const int c = (int)(t % g.C);
  const int bt = (int)(t / g.C);
  // a table entry outside the bank is CLAMPED into it (the host validates tables it can see, ops.patch_gather_eval; a
  // device-resident table cannot be checked without a sync): no read below can leave the bank
  const int f = min(max(index ? index[bt] : bt, 0), g.F - 1);
  const int Hs = g.Hs, Ws = g.Ws;
  const unsigned char* src = frames + ((long)f * g.C + c) * Hs * Ws;
  const float s2 = (float)g.S / (float)R;
  const float s1y = (float)Hs / (float)g.H1, s1x = (float)Ws / (float)g.W1;
  const LinTap ty = lin_tap(y, s2, g.S);                       // rows of the S x S crop
  const int Y0 = g.top + ty.i0, Y1 = g.top + ty.i1;            // rows of the H1 x W1 stage-1 image (top + S <= H1)
  LinTap ya, yb;                                               // source rows behind Y0 / Y1
  if (IDENT) {
    ya.i0 = ya.i1 = min(Y0, Hs - 1);
    yb.i0 = yb.i1 = min(Y1, Hs - 1);
    ya.l = yb.l = 0.f;
  } else {
    ya = lin_tap(Y0, s1y, Hs);
    yb = lin_tap(Y1, s1y, Hs);
  }
  const unsigned char* ra0 = src + (long)ya.i0 * Ws;
  const unsigned char* ra1 = src + (long)ya.i1 * Ws;
  const unsigned char* rb0 = src + (long)yb.i0 * Ws;
  const unsigned char* rb1 = src + (long)yb.i1 * Ws;
  const float mu = nrm.mean[c], sd = nrm.std[c];
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const LinTap tx = lin_tap(xg * 4 + e, s2, g.S);
    const int X0 = g.left + tx.i0, X1 = g.left + tx.i1;
    float q00, q01, q10, q11;                                  // the four stage-1 pixels (Y0 | Y1, X0 | X1)
    if (IDENT) {
      const int x0 = min(X0, Ws - 1), x1 = min(X1, Ws - 1);
      q00 = (float)ra0[x0] / 255.0f; q01 = (float)ra0[x1] / 255.0f;
      q10 = (float)rb0[x0] / 255.0f; q11 = (float)rb0[x1] / 255.0f;
    } else {
      const LinTap xa = lin_tap(X0, s1x, Ws), xb = lin_tap(X1, s1x, Ws);
      q00 = bilerp(ya.l, xa.l, (float)ra0[xa.i0] / 255.0f, (float)ra0[xa.i1] / 255.0f, (float)ra1[xa.i0] / 255.0f, (float)ra1[xa.i1] / 255.0f);
      q01 = bilerp(ya.l, xb.l, (float)ra0[xb.i0] / 255.0f, (float)ra0[xb.i1] / 255.0f, (float)ra1[xb.i0] / 255.0f, (float)ra1[xb.i1] / 255.0f);
      q10 = bilerp(yb.l, xa.l, (float)rb0[xa.i0] / 255.0f, (float)rb0[xa.i1] / 255.0f, (float)rb1[xa.i0] / 255.0f, (float)rb1[xa.i1] / 255.0f);
      q11 = bilerp(yb.l, xb.l, (float)rb0[xb.i0] / 255.0f, (float)rb0[xb.i1] / 255.0f, (float)rb1[xb.i0] / 255.0f, (float)rb1[xb.i1] / 255.0f);
    }
    v[e] = (bilerp(ty.l, tx.l, q00, q01, q10, q11) - mu) / sd;
  }
  store_patch4(v, bt, c, y, xg * 4, R, g.P, ahi, alo, lda);
}
}  // namespace

extern "C" int egv_patch_gather_u8_eval(const uint8_t* frames, int32_t F, const int32_t* index, int32_t BT, int32_t C, int32_t Hs,
                                        int32_t Ws, int32_t S, int32_t R, int32_t P, const float* mean, const float* std,
                                        egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  if (!frames || !a_hi || !mean || !std || F <= 0 || BT <= 0 || C <= 0 || C > 4) return EGV_ERR_ARG;
  if (!index && BT > F) return EGV_ERR_ARG;                     // index == NULL: output frame bt IS bank frame bt
  if (Hs <= 0 || Ws <= 0 || S <= 0 || R <= 0 || P <= 0 || R % P != 0 || R % 4 != 0 || P % 2 != 0 || lda % 2 != 0) return EGV_ERR_ARG;
  if (lda < (int64_t)C * P * P) return EGV_ERR_ARG;
  // Resize(S): the short side becomes S, the long side int(S * long / short) (torchvision's rule); sizes are kept below 2^20 so that
  // every pixel coordinate is an exact fp32 integer and the products below cannot overflow
  const int shrt = Hs < Ws ? Hs : Ws, lng = Hs < Ws ? Ws : Hs;
  if (S >= (1 << 20) || R >= (1 << 20) || lng >= (1 << 20)) return EGV_ERR_ARG;
  const double lng1 = (double)((int64_t)S * lng) / (double)shrt;
  if (!(lng1 < (double)(1 << 20))) return EGV_ERR_ARG;
  const int l1 = (int)lng1;                                     // >= S
  EvalGeom g;
  g.F = F; g.BT = BT; g.C = C; g.Hs = Hs; g.Ws = Ws; g.S = S; g.R = R; g.P = P;
  g.H1 = Hs <= Ws ? S : l1;
  g.W1 = Hs <= Ws ? l1 : S;
  // CenterCrop(S): int(round((H1 - S) / 2.0)) with Python's round (halves go to the even neighbour)
  auto centre = [](int d) { const int k = d / 2; return (d % 2 == 0 || k % 2 == 0) ? k : k + 1; };
  g.top = centre(g.H1 - S);
  g.left = centre(g.W1 - S);
  PatchNorm nrm{};
  for (int c = 0; c < C; ++c) {
    if (!(std[c] > 0.f)) return EGV_ERR_ARG;
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  const long total = (long)BT * C * R * (R / 4);
  const long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffL) return EGV_ERR_ARG;
  if (g.H1 == Hs && g.W1 == Ws) {
    EGV_LAUNCH(patch_gather_eval_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, index, g, a_hi, a_lo,
               (long)lda, nrm);
  } else {
    EGV_LAUNCH(patch_gather_eval_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, index, g, a_hi, a_lo,
               (long)lda, nrm);
  }
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ---- patch dropout (timm patch_drop_rate / FLIP masking, as tubes): train on K of the n patch positions of every clip -------------
// egv_patch_keep_draw draws the table keep[B, K] on the device; the *_sel gathers and the *_sel token assembly are the kernels above
// restricted to the kept positions, so the planes, the patch-embed GEMM, its wgrad and every block run over B*T*K rows and a
// dropped patch is never read.  A table entry outside [0, n) is clamped into it wherever it is read: a bad table cannot make a
// kernel leave its buffers.
namespace {
constexpr int KEEP_MAX_N = 1024;    // 448^2 / 14^2

__device__ __forceinline__ int keep_at(const int* __restrict__ keep, long i, int n) { return min(max(keep[i], 0), n - 1); }

// One workgroup per clip.  key(b, j) = the hash egv_drop_scale uses at element index b * n + j; j is kept <=> fewer than K positions
// of the clip have a smaller (key, j) pair.  Keys in LDS, rank by counting (all lanes read the same LDS word: a broadcast), output
// slot = number of kept positions in front of j.  No atomics: the table is a pure function of (seed, b, n, K).
__global__ __launch_bounds__(256) void patch_keep_draw_kernel(int n, int K, EgvDrop d0, int* __restrict__ keep) {
  __shared__ uint32_t key[KEEP_MAX_N];
  __shared__ unsigned char kept[KEEP_MAX_N];
  const EgvDrop d = egv_drop_resolve(d0);
  const int b = blockIdx.x;
  for (int j = threadIdx.x; j < n; j += 256) {
    const uint64_t idx = (uint64_t)b * (uint64_t)n + (uint64_t)j;
    key[j] = egv_mix32(egv_mix32((uint32_t)idx ^ d.s0) ^ (uint32_t)(idx >> 32) ^ d.s1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 256) {
    const uint32_t h = key[j];
    int rank = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t hi = key[i];
      rank += (hi < h || (hi == h && i < j)) ? 1 : 0;
    }
    kept[j] = rank < K ? 1 : 0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 256) {
    if (!kept[j]) continue;
    int slot = 0;
    for (int i = 0; i < j; ++i) slot += kept[i];
    keep[(long)b * K + slot] = j;      // exactly K positions have rank < K: slot < K
  }
}

// The fp32 / uint8 gather over the kept patches: thread -> (output row r = bt * K + j, channel c, patch row iy, G-pixel group xg), xg
// fastest, so a row's K_cols columns are written contiguously and one patch-row segment (P pixels) is read by P / G neighbours.
// Arithmetic and split as patch_gather_kernel: the same bits in row bt * K + j as that kernel leaves in row bt * n + keep[bt / T][j].
template <int G, bool U8>
__global__ __launch_bounds__(256) void patch_gather_sel_kernel(const void* __restrict__ video_, int BT, int T, int C, int H, int W,
                                                               int P, const int* __restrict__ keep, int K,
                                                               bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda,
                                                               const PatchNorm nrm) {
  const int PG = P / G;
  const long total = (long)BT * K * C * P * PG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xg = (int)(i % PG);
  long t = i / PG;
  const int iy = (int)(t % P);
  t /= P;
  const int c = (int)(t % C);
  const long row = t / C;                       // bt * K + j
  const int bt = (int)(row / K);
  const int gw = W / P, gh = H / P;
  const int pos = keep_at(keep, (long)(bt / T) * K + (row - (long)bt * K), gw * gh);
  const int py = pos / gw, px = pos - py * gw;
  const int ix = xg * G;
  const long soff = (((long)bt * C + c) * H + (py * P + iy)) * W + px * P + ix;
  float v[G];
  if (U8) {
    const unsigned char* src = (const unsigned char*)video_ + soff;
    const float mu = nrm.mean[c], sd = nrm.std[c];
    unsigned bits;
    if (G == 4) bits = *(const unsigned*)src;
    else bits = *(const unsigned short*)src;
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = ((float)((bits >> (8 * e)) & 0xffu) / 255.0f - mu) / sd;
  } else {
    const float* src = (const float*)video_ + soff;
    if (G == 4) {
      const f32x4_t q = *(const f32x4_t*)src;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
      v[0] = src[0]; v[1] = src[1];
    }
  }
  const int col = (c * P + iy) * P + ix;
  bf16_t h[G], l[G];
#pragma unroll
  for (int e = 0; e < G; ++e) split_bf16(v[e], h[e], l[e]);
  if (G == 4) {
    *(u32x2_t*)(ahi + row * lda + col) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
    if (alo) *(u32x2_t*)(alo + row * lda + col) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
  } else {
    *(uint32_t*)(ahi + row * lda + col) = pack2(h[0], h[1]);
    if (alo) *(uint32_t*)(alo + row * lda + col) = pack2(l[0], l[1]);
  }
}

// The train-transform gather over the kept patches.  The bilinear arithmetic is contraction-sensitive (which product of a sum the compiler
// fuses into an FMA depends on how it packs the four pixels of a group), so a thread computes the SAME aligned 4-pixel group x4 .. x4 + 3
// of output row y with the SAME code as patch_gather_aug_kernel and stores the pixels of it that lie in its patch: NG = P / 4 groups
// per patch row when P % 4 == 0, (P + 2) / 4 when a patch can start in the middle of a group (P = 14).
__global__ __launch_bounds__(256) void patch_gather_aug_sel_kernel(const unsigned char* __restrict__ video, int BT, int T, int C,
                                                                   int Hs, int Ws, int R, int P, int NG, const int* __restrict__ boxes,
                                                                   const int* __restrict__ keep, int K, bf16_t* __restrict__ ahi,
                                                                   bf16_t* __restrict__ alo, long lda, const PatchNorm nrm) {
  const long total = (long)BT * K * C * P * NG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int g = (int)(i % NG);
  long t = i / NG;
  const int iy = (int)(t % P);
  t /= P;
  const int c = (int)(t % C);
  const long orow = t / C;                      // bt * K + j
  const int bt = (int)(orow / K);
  const int gw = R / P;
  const int pos = keep_at(keep, (long)(bt / T) * K + (orow - (long)bt * K), gw * gw);
  const int py = pos / gw, px = pos - py * gw;
  const int xq = (px * P) / 4 + g;              // the 4-pixel group of the whole output row
  if (xq * 4 >= (px + 1) * P) return;
  const AugRow row(video, boxes, bt, T, C, c, Hs, Ws, R, py * P + iy, nrm);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = row.pixel(xq * 4 + e);
  const int ix = xq * 4 - px * P;               // column of the group's first pixel inside the patch row: -2 .. P - 2
  bf16_t* const dhi = ahi + orow * lda + (c * P + iy) * P;
  bf16_t* const dlo = alo ? alo + orow * lda + (c * P + iy) * P : nullptr;
  if (ix >= 0 && ix + 3 < P && (((orow * lda + (c * P + iy) * P + ix) & 3) == 0)) {
    uint32_t h0, h1, l0, l1;
    split_bf16x2(v[0], v[1], h0, l0);
    split_bf16x2(v[2], v[3], h1, l1);
    *(u32x2_t*)(dhi + ix) = (u32x2_t){h0, h1};
    if (dlo) *(u32x2_t*)(dlo + ix) = (u32x2_t){l0, l1};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (ix + e < 0 || ix + e >= P) continue;
      bf16_t h, l;
      split_bf16(v[e], h, l);
      dhi[ix + e] = h;
      if (dlo) dlo[ix + e] = l;
    }
  }
}

// x[b, 0, :] = cls + pos[0]; x[b, 1 + f*K + j, :] = (pe[(b*T + f)*K + j] + pos[1 + keep[b][j]]) + temporal[f]: the sum order of
// assemble_tokens_kernel
__global__ __launch_bounds__(256) void assemble_tokens_sel_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                                  const float* __restrict__ pos, const float* __restrict__ temporal,
                                                                  const int* __restrict__ keep, int B, int T, int n, int K, int D,
                                                                  float* __restrict__ x) {
  const int D4 = D / 4;
  const long S = 1 + (long)T * K;
  const long total = (long)B * S * D4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d = (int)(i % D4) * 4;
  const long tok = i / D4;
  const int s = (int)(tok % S);
  const int b = (int)(tok / S);
  f32x4_t v;
  if (s == 0) {
    v = *(const f32x4_t*)(cls + d) + *(const f32x4_t*)(pos + d);
  } else {
    const int f = (s - 1) / K, j = (s - 1) % K;
    const int ii = keep_at(keep, (long)b * K + j, n);
    v = *(const f32x4_t*)(pe + (((long)b * T + f) * K + j) * D + d) + *(const f32x4_t*)(pos + (long)(1 + ii) * D + d) +
        *(const f32x4_t*)(temporal + (long)f * D + d);
  }
  *(f32x4_t*)(x + tok * D + d) = v;
}

// d_pos[1 + p] = sum of dx over the frames of the clips that kept p; d_pos[0] = d_cls = sum_b dx[b, 0].  Grid (n + 1 position rows,
// slices of the clips), as assemble_bwd_pos_kernel; a block walks its clips' table rows for its position (K ints, the same for every
// lane) and adds the T rows of a hit.  A position no clip kept is never added to: it stays the launcher's zero.
__global__ __launch_bounds__(256) void assemble_bwd_pos_sel_kernel(const float* __restrict__ dx, const int* __restrict__ keep, int B,
                                                                   int T, int n, int K, int D, float* __restrict__ d_pos,
                                                                   float* __restrict__ d_cls) {
  const int p = blockIdx.x;
  const long S = 1 + (long)T * K;
  for (int d4 = threadIdx.x; d4 < D / 4; d4 += blockDim.x) {
    f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    bool any = false;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
      if (p == 0) {
        s0 += *(const f32x4_t*)(dx + (long)b * S * D + d4 * 4);
        any = true;
        continue;
      }
      for (int j = 0; j < K; ++j) {
        if (keep_at(keep, (long)b * K + j, n) != p - 1) continue;
        any = true;
        const float* src = dx + ((long)b * S + 1 + j) * D + d4 * 4;
        int f = 0;
        for (; f + 1 < T; f += 2) {
          s0 += *(const f32x4_t*)(src + (long)f * K * D);
          s1 += *(const f32x4_t*)(src + (long)(f + 1) * K * D);
        }
        if (f < T) s0 += *(const f32x4_t*)(src + (long)f * K * D);
      }
    }
    if (!any) continue;
    const f32x4_t s = s0 + s1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      atomicAdd(d_pos + (long)p * D + d4 * 4 + e, s[e]);
      if (p == 0) atomicAdd(d_cls + d4 * 4 + e, s[e]);
    }
  }
}
}  // namespace

extern "C" int egv_patch_keep_draw(int32_t B, int32_t n, int32_t K, uint64_t seed, const uint64_t* seed_dev, int32_t* keep,
                                   void* stream) {
  if (!keep || B <= 0 || K < 1 || K > n || n > KEEP_MAX_N) return EGV_ERR_ARG;
  EGV_LAUNCH(patch_keep_draw_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, n, K, egv_make_drop(0.f, seed, seed_dev), keep);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

template <bool U8>
static int patch_gather_sel_launch(const void* video, int BT, int T, int C, int H, int W, int P, const int32_t* keep, int K,
                                   egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, const PatchNorm& nrm, void* stream) {
  if (!video || !a_hi || !keep || BT <= 0 || T <= 0 || BT % T != 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0) return EGV_ERR_ARG;
  if (P % 2 != 0 || W % P != 0 || H % P != 0 || lda % 4 != 0 || lda < (int64_t)C * P * P) return EGV_ERR_ARG;
  if (K < 1 || K > (H / P) * (W / P)) return EGV_ERR_ARG;
  const int G = P % 4 == 0 ? 4 : 2;
  const long blocks = ((long)BT * K * C * P * (P / G) + 255) / 256;
  if (blocks > 0x7fffffffL) return EGV_ERR_ARG;
  if (G == 4) {
    EGV_LAUNCH((patch_gather_sel_kernel<4, U8>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, video, BT, T, C, H, W, P,
               keep, K, a_hi, a_lo, (long)lda, nrm);
  } else {
    EGV_LAUNCH((patch_gather_sel_kernel<2, U8>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, video, BT, T, C, H, W, P,
               keep, K, a_hi, a_lo, (long)lda, nrm);
  }
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_patch_gather_sel(const float* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                                    const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  return patch_gather_sel_launch<false>(video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, lda, PatchNorm{}, stream);
}

extern "C" int egv_patch_gather_u8_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                                       const float* mean, const float* std, const int32_t* keep, int32_t K, egv_bf16* a_hi,
                                       egv_bf16* a_lo, int64_t lda, void* stream) {
  if (!mean || !std || C < 1 || C > 4) return EGV_ERR_ARG;
  PatchNorm nrm{};
  for (int c = 0; c < C; ++c) {
    if (!(std[c] > 0.f)) return EGV_ERR_ARG;
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  return patch_gather_sel_launch<true>(video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, lda, nrm, stream);
}

extern "C" int egv_patch_gather_u8_aug_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                           int32_t R, int32_t P, const int32_t* boxes, const float* mean, const float* std,
                                           const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda,
                                           void* stream) {
  if (!video || !boxes || !keep || !a_hi || !mean || !std || BT <= 0 || T <= 0 || BT % T != 0 || C <= 0 || C > 4) return EGV_ERR_ARG;
  if (Hs <= 0 || Ws <= 0 || R <= 0 || P <= 0 || R % P != 0 || R % 4 != 0 || P % 2 != 0) return EGV_ERR_ARG;
  if (lda % 4 != 0 || lda < (int64_t)C * P * P || K < 1 || K > (R / P) * (R / P)) return EGV_ERR_ARG;
  PatchNorm nrm{};
  for (int c = 0; c < C; ++c) {
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  const int NG = P % 4 == 0 ? P / 4 : (P + 2) / 4;           // 4-pixel groups of the output row that can touch one patch row
  const long blocks = ((long)BT * K * C * P * NG + 255) / 256;
  if (blocks > 0x7fffffffL) return EGV_ERR_ARG;
  EGV_LAUNCH(patch_gather_aug_sel_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, video, BT, T, C, Hs, Ws, R, P, NG,
             boxes, keep, K, a_hi, a_lo, (long)lda, nrm);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_assemble_tokens_sel(const float* pe, const float* cls, const float* pos, const float* temporal,
                                       const int32_t* keep, int32_t B, int32_t T, int32_t n, int32_t K, int32_t D, float* x,
                                       void* stream) {
  if (!pe || !cls || !pos || !temporal || !keep || !x || D <= 0 || D % 4 != 0) return EGV_ERR_ARG;
  if (B <= 0 || T <= 0 || K < 1 || K > n) return EGV_ERR_ARG;
  const long blocks = ((long)B * (1 + (long)T * K) * (D / 4) + 255) / 256;
  if (blocks > 0x7fffffffL) return EGV_ERR_ARG;
  EGV_LAUNCH(assemble_tokens_sel_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pe, cls, pos, temporal, keep, B, T,
             n, K, D, x);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_assemble_tokens_bwd_sel(const float* dx, const int32_t* keep, int32_t B, int32_t T, int32_t n, int32_t K,
                                           int32_t D, int32_t T_model, float* d_pe, float* d_cls, float* d_pos, float* d_temporal,
                                           void* stream) {
  if (!dx || !keep || D <= 0 || D % 4 != 0 || B <= 0 || T <= 0 || T > T_model || K < 1 || K > n) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (d_pos && d_cls) {
    if (hipMemsetAsync(d_pos, 0, sizeof(float) * (size_t)(n + 1) * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    if (hipMemsetAsync(d_cls, 0, sizeof(float) * (size_t)D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    EGV_LAUNCH(assemble_bwd_pos_sel_kernel, dim3(n + 1, 4), dim3(256), 0, s, dx, keep, B, T, n, K, D, d_pos, d_cls);
    EGV_CHECK_LAUNCH();
  }
  // with K patches per frame the tokens ARE a [B, 1 + T*K, D] sequence: d_temporal and d_pe are those of egv_assemble_tokens_bwd at n = K
  if (d_temporal) {
    if (hipMemsetAsync(d_temporal, 0, sizeof(float) * (size_t)T_model * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    EGV_LAUNCH(assemble_bwd_temporal_kernel, dim3(T, (D + 63) / 64, 32), dim3(256), 0, s, dx, B, T, K, D, T_model, d_temporal);
    EGV_CHECK_LAUNCH();
  }
  if (d_pe) {
    const long total = (long)B * T * K * (D / 4);
    EGV_LAUNCH(assemble_bwd_pe_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dx, B, T, K, D, d_pe);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}
