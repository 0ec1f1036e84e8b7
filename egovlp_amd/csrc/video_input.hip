// Video input kernels: decoded frames -> the im2col planes of the patch-embed GEMM (plain, with the train or the val / test transform
// fused in, over all patches or over the kept patches of patch dropout), the draw of the patch-dropout table, and the token assembly
// (patch embeddings + cls + position + temporal rows) with its backward.  One body per operation: the `_sel` entry points run the
// same device code as their full twins behind another thread map or one table lookup.  All HBM- or issue-bound: 16-byte global
// accesses where the layout allows, LDS only for the draw's keys and the temporal reduction.
#include "common.h"
#include "egovlp_hip.h"

namespace {

struct PatchNorm { float mean[4], std[4]; };   // per-channel Normalize constants of the uint8 paths (C <= 4)

// ---- patch dropout (timm patch_drop_rate / FLIP masking, as tubes): train on K of the n patch positions of every clip -------------
// egv_patch_keep_draw draws the table keep[B, K] on the device; the *_sel gathers and the *_sel token assembly are the kernels below
// restricted to the kept positions, so the planes, the patch-embed GEMM, its wgrad and every block run over B*T*K rows and a
// dropped patch is never read.  A table entry outside [0, n) is clamped into it wherever it is read: a bad table cannot make a
// kernel leave its buffers.
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

// ---------------------------------------------------------------------------------------------
// direct patch gather (im2col for a PxP / stride P conv): one thread moves G consecutive pixels of one patch row (G = 4 when
// P % 4 == 0 -- ViT-B/16 -- else 2 -- ViT-L/14).  Columns K .. lda-1 of the output planes (K padded to the GEMM's k-tile) are left
// untouched: the caller zero-fills them once.

// G pixels of channel c at element offset soff of the clip, as the patch-embed GEMM sees them
template <int G, bool U8>
__device__ __forceinline__ void load_pixels(const void* video_, long soff, int c, const PatchNorm& nrm, float (&v)[G]) {
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
}

// split a G-group and store it at (row, col) of the planes.  The two widths address the planes differently on purpose: with the
// pointers formed first the 2-pixel kernels schedule better and the 4-pixel uint8 kernel worse (DESIGN 4.8 has the figures).
template <int G>
__device__ __forceinline__ void store_group(const float (&v)[G], long row, int col, bf16_t* ahi, bf16_t* alo, long lda) {
  if (G == 2) {
    ahi += row * lda + col;
    if (alo) alo += row * lda + col;
    row = col = 0;
  }
  bf16_t h[G], l[G];
#pragma unroll
  for (int e = 0; e < G; ++e) split_bf16(v[e], h[e], l[e]);
  if (G == 4) {
    *(u32x2_t*)(ahi + row * lda + col) = (u32x2_t){pack2(h[0], h[1]), pack2(h[2], h[3])};
    if (alo) *(u32x2_t*)(alo + row * lda + col) = (u32x2_t){pack2(l[0], l[1]), pack2(l[2], l[3])};
  } else {
    *(uint32_t*)ahi = pack2(h[0], h[1]);
    if (alo) *(uint32_t*)alo = pack2(l[0], l[1]);
  }
}

template <int G, bool U8>
__global__ __launch_bounds__(256) void patch_gather_kernel(const void* __restrict__ video_, int BT, int C, int H, int W,
                                                           int P, bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo,
                                                           long lda, const PatchNorm nrm) {
  // own map: thread -> (image bt, channel c, image row y, G-pixel group xg), so that a wave reads one contiguous image row segment
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
  float v[G];
  load_pixels<G, U8>(video_, (((long)bt * C + c) * H + y) * W + xg * G, c, nrm, v);
  const int gw = W / P, gh = H / P;
  const int py = y / P, iy = y % P;
  const int x = xg * G;
  const int px = x / P, ix = x % P;
  store_group<G>(v, ((long)bt * gh + py) * gw + px, (c * P + iy) * P + ix, ahi, alo, lda);
}

// The same over the kept patches: the same bits in row bt * K + j as patch_gather_kernel leaves in row bt * n + keep[bt / T][j].
template <int G, bool U8>
__global__ __launch_bounds__(256) void patch_gather_sel_kernel(const void* __restrict__ video_, int BT, int T, int C, int H, int W,
                                                               int P, const int* __restrict__ keep, int K,
                                                               bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda,
                                                               const PatchNorm nrm) {
  // own map: thread -> (output row bt * K + j, channel c, patch row iy, G-pixel group xg), so that a dropped patch is never read
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
  float v[G];
  load_pixels<G, U8>(video_, (((long)bt * C + c) * H + (py * P + iy)) * W + px * P + ix, c, nrm, v);
  store_group<G>(v, row, (c * P + iy) * P + ix, ahi, alo, lda);
}

// ---- train-time augmentation fused into the patch gather (data_loader/transforms.py:14-19: RandomResizedCrop(
// input_res, scale) -> RandomHorizontalFlip -> ColorJitter(brightness, saturation, hue) -> Normalize; the jitter is the identity in
// the pre-training config and lives in the *_color kernels further down) ---------------------------------------------------------
// The loader hands over the DECODED uint8 clip [B*T, C, Hs, Ws] and five ints per clip -- the crop box (top, left, h, w) and a
// flip flag, the random draws of the host transform (one box per clip: the reference applies the transform to the [T, C, H, W]
// tensor as a whole).  Every output pixel of the R x R frame is sampled here: x / 255 first (the reference resizes float frames),
// bilinear with align_corners = False semantics (source index (o + 0.5) * size / R - 0.5 clamped at 0, right / bottom neighbour
// clamped to the box), mirrored when flipped, normalised, split and written straight into the im2col planes of the patch-embed
// GEMM.  No resized fp32 clip ever exists in HBM (the host transform writes 4 x 3 x 224 x 224 floats per clip and the H2D
// copy carries them).
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
// The same group into row orow of the planes of a gather over kept patches: the pixels of it that lie in the patch.  ix = column of the
// group's first pixel inside the patch row, -2 .. P - 2.
__device__ __forceinline__ void store_patch4_sel(const float (&v)[4], long orow, int c, int iy, int ix, int P, bf16_t* ahi, bf16_t* alo,
                                                 long lda) {
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
// One output row of the resized crop of frame bt, channel c: the clamped box, the two source rows behind output row y and the
// Normalize constants.  sample(ox) is output pixel ox of that row in [0, 1], pixel(ox) the same normalised.
// The arithmetic is PINNED: contraction off and every fused multiply-add written out.  Left to the compiler, which product of a
// sum became an FMA depended on how it packed the pixels of a group, and that on everything around the group -- two kernels gave
// the same bits only while their bodies happened to be alike (measured: 1 % of the lo-plane elements of a kernel that computed two
// groups differed in the last place).  Written out, every kernel that samples a pixel computes the same bits whatever else it does,
// which is what the kept-patch and the Mixup / CutMix kernels below promise.
struct AugRow {
  const unsigned char *r0, *r1;
  float ly, sx, mu, sd;
  int bw, flip, R;
  __device__ __forceinline__ AugRow(const unsigned char* __restrict__ video, const int* __restrict__ boxes, int bt, int T, int C, int c,
                                    int Hs, int Ws, int R_, int y, const PatchNorm& nrm) {
#pragma clang fp contract(off)
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
    float fy = fmaf((float)y + 0.5f, sy, -0.5f);
    fy = fy < 0.f ? 0.f : fy;
    const int y0 = (int)fy;
    const int y1 = y0 + (y0 < bh - 1 ? 1 : 0);
    ly = fy - (float)y0;
    r0 = src + (long)(top + y0) * Ws + left;
    r1 = src + (long)(top + y1) * Ws + left;
    mu = nrm.mean[c];
    sd = nrm.std[c];
  }
  __device__ __forceinline__ float sample(int ox) const {
#pragma clang fp contract(off)
    const int sxi = flip ? R - 1 - ox : ox;               // RandomHorizontalFlip acts on the resized crop
    float fx = fmaf((float)sxi + 0.5f, sx, -0.5f);
    fx = fx < 0.f ? 0.f : fx;
    const int x0 = (int)fx;
    const int x1 = x0 + (x0 < bw - 1 ? 1 : 0);
    const float lx = fx - (float)x0;
    const float p00 = (float)r0[x0] / 255.0f, p01 = (float)r0[x1] / 255.0f;
    const float p10 = (float)r1[x0] / 255.0f, p11 = (float)r1[x1] / 255.0f;
    const float top = fmaf(lx, p01, (1.0f - lx) * p00), bot = fmaf(lx, p11, (1.0f - lx) * p10);
    return fmaf(ly, bot, (1.0f - ly) * top);
  }
  __device__ __forceinline__ float pixel(int ox) const { return (sample(ox) - mu) / sd; }
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

// The train-transform gather over the kept patches.  The bilinear arithmetic is contraction-sensitive (which product of a sum the compiler
// fuses into an FMA depends on how it packs the four pixels of a group; AugRow pins it), so a thread computes the SAME aligned 4-pixel
// group x4 .. x4 + 3 of output row y with the SAME code as patch_gather_aug_kernel and stores the pixels of it that lie in its patch:
// NG = P / 4 groups per patch row when P % 4 == 0, (P + 2) / 4 when a patch can start in the middle of a group (P = 14).
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
  store_patch4_sel(v, orow, c, iy, xq * 4 - px * P, P, ahi, alo, lda);
}

// ---- ColorJitter(brightness, saturation, hue) of the train transform (torchvision 0.13's tensor path, restated; contrast cannot be
// set by the reference's configs) ---------------------------------------------------------------------------------------------------
// The host draws, per clip, color[b] = (brightness factor, saturation factor, hue shift, code): code holds three base-4 digits, the
// first applied op lowest (0 nothing, 1 brightness, 2 saturation, 3 hue), i.e. which ops run and in torchvision's random order.  The
// ops act on RGB in [0, 1] after crop / resize / flip and before Normalize, and saturation and hue mix the channels: a thread owns
// an aligned 4-pixel group of an output row for ALL THREE channels.  The arithmetic follows the fp32 restatement operation for
// operation with contraction OFF: no product is fused into a neighbouring sum, whichever way the compiler packs the twelve values,
// so the kept-patch twin computes the bits of the full kernel (and the jitter's own error is that of the fp32 host transform).
// No table value addresses anything: (int)code & 63 only selects among the three bodies; a non-finite factor gives NaN pixels (the
// clamps are comparisons, which let a NaN through) in the frames of that clip only.
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// blend(x, 0, f)
__device__ __forceinline__ void jitter_brightness(float& r, float& g, float& b, float f) {
#pragma clang fp contract(off)
  r = clamp01(f * r);
  g = clamp01(f * g);
  b = clamp01(f * b);
}
// blend(x, gray, f)
__device__ __forceinline__ void jitter_saturation(float& r, float& g, float& b, float f) {
#pragma clang fp contract(off)
  const float gray = (1.0f - f) * (0.2989f * r + 0.587f * g + 0.114f * b);
  r = clamp01(f * r + gray);
  g = clamp01(f * g + gray);
  b = clamp01(f * b + gray);
}
// rgb -> hsv, h -> (h + d) mod 1, hsv -> rgb.  Selects only: every lane runs the same instructions whatever its pixel's sector.
__device__ __forceinline__ void jitter_hue(float& r, float& g, float& b, float d) {
#pragma clang fp contract(off)
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.0f : maxc);
  const float dv = eq ? 1.0f : cr;
  const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
  const float hp = maxc == r ? bc - gc : (maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc);
  float h = hp / 6.0f + 1.0f;
  h -= floorf(h);                                 // fmod(., 1) of a positive number: exact
  h += d;
  h -= floorf(h);                                 // Python's %: the sign of the divisor
  const float v = maxc;
  const float h6 = h * 6.0f;
  const float fl = floorf(h6);
  const float f = h6 - fl;
  int i = (int)fl;                                // 0 .. 6 (h may round up to 1); NaN -> 0
  i = i >= 6 ? i - 6 : i;
  const float p = clamp01(v * (1.0f - s));
  const float q = clamp01(v * (1.0f - s * f));
  const float t = clamp01(v * (1.0f - s * (1.0f - f)));
  r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// Pixels x4 .. x4 + 3 of output row y of frame bt, the three channels: sampled by AugRow, jittered as the clip's code says, normalised.
// The code is the same for every thread of a frame, so the dispatch is a branch the whole wave takes together (bar the one wave in
// which one clip ends and the next begins).
__device__ __forceinline__ void aug_color_group(const unsigned char* __restrict__ video, const int* __restrict__ boxes,
                                                const float* __restrict__ color, int bt, int T, int Hs, int Ws, int R, int y, int x4,
                                                const PatchNorm& nrm, float (&v)[3][4]) {
  const AugRow rows[3] = {AugRow(video, boxes, bt, T, 3, 0, Hs, Ws, R, y, nrm), AugRow(video, boxes, bt, T, 3, 1, Hs, Ws, R, y, nrm),
                          AugRow(video, boxes, bt, T, 3, 2, Hs, Ws, R, y, nrm)};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[c][e] = rows[c].sample(x4 + e);
  const float* cj = color + (long)(bt / T) * 4;
  const float fb = cj[0], fs = cj[1], fh = cj[2];
  int code = (int)cj[3] & 63;
#pragma unroll
  for (int k = 0; k < 3; ++k, code >>= 2) {
    const int op = code & 3;
    if (op == 1) {
#pragma unroll
      for (int e = 0; e < 4; ++e) jitter_brightness(v[0][e], v[1][e], v[2][e], fb);
    } else if (op == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) jitter_saturation(v[0][e], v[1][e], v[2][e], fs);
    } else if (op == 3) {
#pragma unroll
      for (int e = 0; e < 4; ++e) jitter_hue(v[0][e], v[1][e], v[2][e], fh);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[c][e] = (v[c][e] - rows[c].mu) / rows[c].sd;
}

__global__ __launch_bounds__(256) void patch_gather_aug_color_kernel(const unsigned char* __restrict__ video, int BT, int T, int Hs,
                                                                     int Ws, int R, int P, const int* __restrict__ boxes,
                                                                     const float* __restrict__ color, bf16_t* __restrict__ ahi,
                                                                     bf16_t* __restrict__ alo, long lda, const PatchNorm nrm) {
  // thread -> (image bt, output row y, 4-pixel group xg), all three channels
  const int WG = R / 4;
  const long total = (long)BT * R * WG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int xg = (int)(i % WG);
  const long t = i / WG;
  const int y = (int)(t % R);
  const int bt = (int)(t / R);
  float v[3][4];
  aug_color_group(video, boxes, color, bt, T, Hs, Ws, R, y, xg * 4, nrm, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) store_patch4(v[c], bt, c, y, xg * 4, R, P, ahi, alo, lda);
}

// The same over the kept patches: thread -> (output row bt * K + j, patch row iy, group g), the straddling rule of
// patch_gather_aug_sel_kernel.
__global__ __launch_bounds__(256) void patch_gather_aug_color_sel_kernel(const unsigned char* __restrict__ video, int BT, int T, int Hs,
                                                                         int Ws, int R, int P, int NG, const int* __restrict__ boxes,
                                                                         const float* __restrict__ color, const int* __restrict__ keep,
                                                                         int K, bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo,
                                                                         long lda, const PatchNorm nrm) {
  const long total = (long)BT * K * P * NG;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int g = (int)(i % NG);
  const long t = i / NG;
  const int iy = (int)(t % P);
  const long orow = t / P;                      // bt * K + j
  const int bt = (int)(orow / K);
  const int gw = R / P;
  const int pos = keep_at(keep, (long)(bt / T) * K + (orow - (long)bt * K), gw * gw);
  const int py = pos / gw, px = pos - py * gw;
  const int xq = (px * P) / 4 + g;              // the 4-pixel group of the whole output row
  if (xq * 4 >= (px + 1) * P) return;
  float v[3][4];
  aug_color_group(video, boxes, color, bt, T, Hs, Ws, R, py * P + iy, xq * 4, nrm, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) store_patch4_sel(v[c], orow, c, iy, xq * 4 - px * P, P, ahi, alo, lda);
}

// ---- Mixup / CutMix inside the gather (extension; timm's Mixup restated, the reference has neither) -----------------------------------
// The host draws, per clip b, mix_idx[b] = (partner, op, y0, y1, x0, x1) and mix_lam[b] (data_loader/transforms.py mix_params).  With
// A_x the fully transformed clip x (its own crop box, flip, colour row and Normalize) and p = partner, the output of clip b is
//   op 1 (mixup):   lam * A_b + (1 - lam) * A_p     two products and one sum, (1 - lam) formed in fp32, nothing contracted
//   op 2 (cutmix):  A_p in rows [y0, y1) x columns [x0, x1) of the output frame (every frame of the clip: a tube), A_b elsewhere
//   op 0 and 3:     A_b
// The partner enters unmixed: no chains.  A thread computes the partner's G-pixel group with the code of the unmixed kernels (the
// contraction rule above patch_gather_aug_sel_kernel) and selects per pixel, so a cutmix output is the unmixed gathers' bits; a
// group wholly outside the box never reads the partner, one wholly inside never reads its own clip.  Both tables are read
// defensively: partner clamped into [0, B), the box into the frame, op & 3 -- no table value addresses anything unclamped.  One
// body per source kind; `keep` (NULL: all patches) only picks the thread map, and under it clip b's kept positions select the
// output rows and the partner is read at those positions.
struct MixRow { int bp, op, y0, y1, x0, x1; float lam; };
__device__ __forceinline__ MixRow mix_row(const int* __restrict__ mix_idx, const float* __restrict__ mix_lam, int b, int B, int H, int W) {
  const int* m = mix_idx + (long)b * 6;
  MixRow r;
  r.bp = min(max(m[0], 0), B - 1);
  r.op = m[1] & 3;
  r.y0 = min(max(m[2], 0), H);
  r.y1 = min(max(m[3], 0), H);
  r.x0 = min(max(m[4], 0), W);
  r.x1 = min(max(m[5], 0), W);
  r.lam = mix_lam[b];
  return r;
}
__device__ __forceinline__ bool mix_in_box(const MixRow& r, int y, int x) {
  return r.op == 2 && y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1;
}
// which of the two clips the N pixels x .. x + N - 1 of output row y need
template <int N>
__device__ __forceinline__ void mix_needs(const MixRow& r, int y, int x, bool& own, bool& partner) {
  int inside = 0;
#pragma unroll
  for (int e = 0; e < N; ++e) inside += mix_in_box(r, y, x + e) ? 1 : 0;
  own = inside < N;
  partner = r.op == 1 || inside > 0;
}
template <int N>
__device__ __forceinline__ void mix_select(const MixRow& r, int y, int x, const float (&a)[N], const float (&p)[N], float (&v)[N]) {
#pragma clang fp contract(off)
  const float om = 1.0f - r.lam;
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = r.op == 1 ? r.lam * a[e] + om * p[e] : (mix_in_box(r, y, x + e) ? p[e] : a[e]);
}

// the same in two steps, for a kernel that walks the clip (w = 0) and then its partner (w = 1): out = lam * a, then out + (1 - lam) * p
template <int N>
__device__ __forceinline__ void mix_take(const MixRow& r, int y, int x, int w, const float (&v)[N], float (&out)[N]) {
#pragma clang fp contract(off)
  const float f = w ? 1.0f - r.lam : r.lam;
#pragma unroll
  for (int e = 0; e < N; ++e) {
    if (r.op == 1) out[e] = w ? out[e] + f * v[e] : f * v[e];
    else if (mix_in_box(r, y, x + e) == (w != 0)) out[e] = v[e];
  }
}

// fp32 and plain uint8 clips (no resampling): the thread maps, loads and stores of patch_gather_kernel / patch_gather_sel_kernel
template <int G, bool U8>
__global__ __launch_bounds__(256) void patch_gather_mix_kernel(const void* __restrict__ video_, int BT, int T, int C, int H, int W, int P,
                                                               const int* __restrict__ mix_idx, const float* __restrict__ mix_lam,
                                                               const int* __restrict__ keep, int K, bf16_t* __restrict__ ahi,
                                                               bf16_t* __restrict__ alo, long lda, const PatchNorm nrm) {
  const int gw = W / P, gh = H / P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int bt, c, y, x;
  long row;
  if (keep) {
    const int PG = P / G;
    if (i >= (long)BT * K * C * P * PG) return;
    const int xg = (int)(i % PG);
    long t = i / PG;
    const int iy = (int)(t % P);
    t /= P;
    c = (int)(t % C);
    row = t / C;                                // bt * K + j
    bt = (int)(row / K);
    const int pos = keep_at(keep, (long)(bt / T) * K + (row - (long)bt * K), gw * gh);
    const int py = pos / gw, px = pos - py * gw;
    y = py * P + iy;
    x = px * P + xg * G;
  } else {
    const int WG = W / G;
    if (i >= (long)BT * C * H * WG) return;
    x = (int)(i % WG) * G;
    long t = i / WG;
    y = (int)(t % H);
    t /= H;
    c = (int)(t % C);
    bt = (int)(t / C);
    row = ((long)bt * gh + y / P) * gw + x / P;
  }
  const MixRow m = mix_row(mix_idx, mix_lam, bt / T, BT / T, H, W);
  const int btp = m.bp * T + bt % T;
  bool own, partner;
  mix_needs<G>(m, y, x, own, partner);
  float a[G] = {}, p[G] = {}, v[G];
  if (own) load_pixels<G, U8>(video_, (((long)bt * C + c) * H + y) * W + x, c, nrm, a);
  if (partner) load_pixels<G, U8>(video_, (((long)btp * C + c) * H + y) * W + x, c, nrm, p);
  mix_select<G>(m, y, x, a, p, v);
  store_group<G>(v, row, (c * P + y % P) * P + x % P, ahi, alo, lda);
}

// The aligned 4-pixel group x4 .. x4 + 3 of output row y of frame bt as the unmixed train-transform kernels compute it: channel c
// into v[0] (plain), or the three jittered channels (COLOR)
template <bool COLOR>
__device__ __forceinline__ void aug_group(const unsigned char* __restrict__ video, const int* __restrict__ boxes,
                                          const float* __restrict__ color, int bt, int T, int C, int c, int Hs, int Ws, int R, int y,
                                          int x4, const PatchNorm& nrm, float (&v)[3][4]) {
  if (COLOR) {
    aug_color_group(video, boxes, color, bt, T, Hs, Ws, R, y, x4, nrm, v);
  } else {
    const AugRow row(video, boxes, bt, T, C, c, Hs, Ws, R, y, nrm);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[0][e] = row.pixel(x4 + e);
  }
}

// the fused train transform: the thread maps and stores of the four patch_gather_aug*_kernel
template <bool COLOR>
__global__ __launch_bounds__(256) void patch_gather_aug_mix_kernel(const unsigned char* __restrict__ video, int BT, int T, int C, int Hs,
                                                                   int Ws, int R, int P, int NG, const int* __restrict__ boxes,
                                                                   const float* __restrict__ color, const int* __restrict__ mix_idx,
                                                                   const float* __restrict__ mix_lam, const int* __restrict__ keep,
                                                                   int K, bf16_t* __restrict__ ahi, bf16_t* __restrict__ alo, long lda,
                                                                   const PatchNorm nrm) {
  const int CT = COLOR ? 1 : C;                 // channels walked by the thread map
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int bt, c = 0, y, x4, iy = 0, ix = 0;
  long orow = 0;
  if (keep) {
    if (i >= (long)BT * K * CT * P * NG) return;
    const int g = (int)(i % NG);
    long t = i / NG;
    iy = (int)(t % P);
    t /= P;
    if (!COLOR) {
      c = (int)(t % C);
      t /= C;
    }
    orow = t;                                   // bt * K + j
    bt = (int)(orow / K);
    const int gw = R / P;
    const int pos = keep_at(keep, (long)(bt / T) * K + (orow - (long)bt * K), gw * gw);
    const int py = pos / gw, px = pos - py * gw;
    const int xq = (px * P) / 4 + g;            // the 4-pixel group of the whole output row
    if (xq * 4 >= (px + 1) * P) return;
    y = py * P + iy;
    x4 = xq * 4;
    ix = x4 - px * P;
  } else {
    const int WG = R / 4;
    if (i >= (long)BT * CT * R * WG) return;
    x4 = (int)(i % WG) * 4;
    long t = i / WG;
    y = (int)(t % R);
    t /= R;
    if (!COLOR) {
      c = (int)(t % C);
      t /= C;
    }
    bt = (int)t;
  }
  const MixRow m = mix_row(mix_idx, mix_lam, bt / T, BT / T, R, R);
  const int btp = m.bp * T + bt % T;
  bool need[2];
  mix_needs<4>(m, y, x4, need[0], need[1]);
  // ONE copy of the group's code, walked for the clip and then for its partner: the loop body is the body of the unmixed kernels
  float out[3][4] = {};
#pragma unroll 1
  for (int w = 0; w < 2; ++w) {
    if (!need[w]) continue;
    float v[3][4];
    aug_group<COLOR>(video, boxes, color, w ? btp : bt, T, C, c, Hs, Ws, R, y, x4, nrm, v);
#pragma unroll
    for (int k = 0; k < (COLOR ? 3 : 1); ++k) mix_take<4>(m, y, x4, w, v[k], out[k]);
  }
#pragma unroll
  for (int k = 0; k < (COLOR ? 3 : 1); ++k) {
    if (keep) store_patch4_sel(out[k], orow, COLOR ? k : c, iy, ix, P, ahi, alo, lda);
    else store_patch4(out[k], bt, COLOR ? k : c, y, x4, R, P, ahi, alo, lda);
  }
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

// ---------------------------------------------------------------------------------------------
// token assembly, K tokens per frame: x[b, 0, :] = cls + pos[0]; x[b, 1 + f*K + j, :] = (pe[(b*T + f)*K + j] + pos[1 + p]) + temporal[f]
// with p = j over all patches (K = n), p = keep[b][j] over the kept ones (SEL): one sum order, so the rows of the two agree in every bit
// (argument order: B, T, n, D are one aligned 16-byte scalar load -- all the full kernel reads of them; the table and its K come last)
template <bool SEL>
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, const float* __restrict__ temporal, int B,
                                                              int T, int n, int D, float* __restrict__ x,
                                                              const int* __restrict__ keep, int K_sel) {
  const int K = SEL ? K_sel : n;
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
    const int ii = SEL ? keep_at(keep, (long)b * K + j, n) : j;
    v = *(const f32x4_t*)(pe + (((long)b * T + f) * K + j) * D + d) + *(const f32x4_t*)(pos + (long)(1 + ii) * D + d) +
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

// The same sums over the kept tokens -- another algorithm, not a twin: d_pos[1 + p] = sum of dx over the frames of the clips that kept
// p; d_pos[0] = d_cls = sum_b dx[b, 0].  Grid (n + 1 position rows, slices of the clips), as assemble_bwd_pos_kernel; a block walks its
// clips' table rows for its position (K ints, the same for every lane) and adds the T rows of a hit.  A position no clip kept is
// never added to: it stays the launcher's zero.
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

// ---------------------------------------------------------------------------------------------
// launcher helpers: every refusal is EGV_ERR_ARG before anything is launched

// mean / std (HOST arrays of C <= 4 floats) -> the kernels' constants; a std that is not positive would write inf / nan planes
bool fill_norm(PatchNorm& nrm, const float* mean, const float* std, int C) {
  if (!mean || !std || C < 1 || C > 4) return false;
  for (int c = 0; c < C; ++c) {
    if (!(std[c] > 0.f)) return false;
    nrm.mean[c] = mean[c];
    nrm.std[c] = std[c];
  }
  return true;
}

// BT frames in clips of T, C channels, H x W cut into P x P patches, planes of lda columns; keep (NULL: all patches): a table of K
// of the patch positions of a frame
bool gather_geom_ok(const void* video, const void* a_hi, int BT, int T, int C, int H, int W, int P, int64_t lda, int lda_align,
                    const void* keep = nullptr, int K = 0) {
  if (!video || !a_hi || BT <= 0 || T <= 0 || BT % T != 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0) return false;
  if (P % 2 != 0 || W % P != 0 || H % P != 0 || lda % lda_align != 0 || lda < (int64_t)C * P * P) return false;
  return !keep || (K >= 1 && K <= (H / P) * (W / P));
}

// one thread per work item in blocks of 256 -> the grid, refused past the 2^31 - 1 blocks of grid.x
bool grid_of(long items, dim3& grid) {
  const long blocks = (items + 255) / 256;
  if (items <= 0 || blocks > 0x7fffffffL) return false;
  grid = dim3((unsigned)blocks);
  return true;
}

// the direct gathers, over all patches (keep == NULL; T plays no part) or over the kept ones
template <bool U8>
int patch_gather_launch(const void* video, int BT, int T, int C, int H, int W, int P, const int32_t* keep, int K,
                        egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, const PatchNorm& nrm, void* stream) {
  if (!gather_geom_ok(video, a_hi, BT, T, C, H, W, P, lda, keep ? 4 : 2, keep, K)) return EGV_ERR_ARG;
  const int G = P % 4 == 0 ? 4 : 2;
  dim3 grid;
  if (!grid_of(keep ? (long)BT * K * C * P * (P / G) : (long)BT * C * H * (W / G), grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (keep) {
    if (G == 4) EGV_LAUNCH((patch_gather_sel_kernel<4, U8>), grid, dim3(256), 0, s, video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, (long)lda, nrm);
    else EGV_LAUNCH((patch_gather_sel_kernel<2, U8>), grid, dim3(256), 0, s, video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, (long)lda, nrm);
  } else {
    if (G == 4) EGV_LAUNCH((patch_gather_kernel<4, U8>), grid, dim3(256), 0, s, video, BT, C, H, W, P, a_hi, a_lo, (long)lda, nrm);
    else EGV_LAUNCH((patch_gather_kernel<2, U8>), grid, dim3(256), 0, s, video, BT, C, H, W, P, a_hi, a_lo, (long)lda, nrm);
  }
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// the train-transform gathers: the R x R output frame is the gather's geometry, the Hs x Ws source only has to exist
// color (NULL: no jitter): the jitter table of the *_color entry points, which have checked it and C == 3 -- one thread then owns a
// group of all three channels
int patch_gather_aug_launch(const uint8_t* video, int BT, int T, int C, int Hs, int Ws, int R, int P, const int32_t* boxes,
                            const float* color, const float* mean, const float* std, const int32_t* keep, int K, egv_bf16* a_hi,
                            egv_bf16* a_lo, int64_t lda, void* stream) {
  PatchNorm nrm{};
  if (!boxes || Hs <= 0 || Ws <= 0 || R % 4 != 0 || !fill_norm(nrm, mean, std, C)) return EGV_ERR_ARG;
  if (!gather_geom_ok(video, a_hi, BT, T, C, R, R, P, lda, keep ? 4 : 2, keep, K)) return EGV_ERR_ARG;
  const int NG = P % 4 == 0 ? P / 4 : (P + 2) / 4;           // 4-pixel groups of the output row that can touch one patch row
  const int CT = color ? 1 : C;                              // channels walked by the thread map
  dim3 grid;
  if (!grid_of(keep ? (long)BT * K * CT * P * NG : (long)BT * CT * R * (R / 4), grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (color && keep) EGV_LAUNCH(patch_gather_aug_color_sel_kernel, grid, dim3(256), 0, s, video, BT, T, Hs, Ws, R, P, NG, boxes, color, keep, K, a_hi, a_lo, (long)lda, nrm);
  else if (color) EGV_LAUNCH(patch_gather_aug_color_kernel, grid, dim3(256), 0, s, video, BT, T, Hs, Ws, R, P, boxes, color, a_hi, a_lo, (long)lda, nrm);
  else if (keep) EGV_LAUNCH(patch_gather_aug_sel_kernel, grid, dim3(256), 0, s, video, BT, T, C, Hs, Ws, R, P, NG, boxes, keep, K, a_hi, a_lo, (long)lda, nrm);
  else EGV_LAUNCH(patch_gather_aug_kernel, grid, dim3(256), 0, s, video, BT, T, C, Hs, Ws, R, P, boxes, a_hi, a_lo, (long)lda, nrm);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// the mixed gathers: the refusals and grids of the two launchers above, plus the two mix tables
template <bool U8>
int patch_gather_mix_launch(const void* video, int BT, int T, int C, int H, int W, int P, const int32_t* mix_idx, const float* mix_lam,
                            const int32_t* keep, int K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, const PatchNorm& nrm, void* stream) {
  if (!mix_idx || !mix_lam || !gather_geom_ok(video, a_hi, BT, T, C, H, W, P, lda, keep ? 4 : 2, keep, K)) return EGV_ERR_ARG;
  const int G = P % 4 == 0 ? 4 : 2;
  dim3 grid;
  if (!grid_of(keep ? (long)BT * K * C * P * (P / G) : (long)BT * C * H * (W / G), grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (G == 4) EGV_LAUNCH((patch_gather_mix_kernel<4, U8>), grid, dim3(256), 0, s, video, BT, T, C, H, W, P, mix_idx, mix_lam, keep, K, a_hi, a_lo, (long)lda, nrm);
  else EGV_LAUNCH((patch_gather_mix_kernel<2, U8>), grid, dim3(256), 0, s, video, BT, T, C, H, W, P, mix_idx, mix_lam, keep, K, a_hi, a_lo, (long)lda, nrm);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

int patch_gather_aug_mix_launch(const uint8_t* video, int BT, int T, int C, int Hs, int Ws, int R, int P, const int32_t* boxes,
                                const float* color, const float* mean, const float* std, const int32_t* mix_idx, const float* mix_lam,
                                const int32_t* keep, int K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  PatchNorm nrm{};
  if (!boxes || !mix_idx || !mix_lam || Hs <= 0 || Ws <= 0 || R % 4 != 0 || (color && C != 3) || !fill_norm(nrm, mean, std, C))
    return EGV_ERR_ARG;
  if (!gather_geom_ok(video, a_hi, BT, T, C, R, R, P, lda, keep ? 4 : 2, keep, K)) return EGV_ERR_ARG;
  const int NG = P % 4 == 0 ? P / 4 : (P + 2) / 4;
  const int CT = color ? 1 : C;
  dim3 grid;
  if (!grid_of(keep ? (long)BT * K * CT * P * NG : (long)BT * CT * R * (R / 4), grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (color) EGV_LAUNCH(patch_gather_aug_mix_kernel<true>, grid, dim3(256), 0, s, video, BT, T, C, Hs, Ws, R, P, NG, boxes, color, mix_idx, mix_lam, keep, K, a_hi, a_lo, (long)lda, nrm);
  else EGV_LAUNCH(patch_gather_aug_mix_kernel<false>, grid, dim3(256), 0, s, video, BT, T, C, Hs, Ws, R, P, NG, boxes, color, mix_idx, mix_lam, keep, K, a_hi, a_lo, (long)lda, nrm);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// token assembly over K tokens per frame; keep == NULL: all patches, K == n
int assemble_launch(const float* pe, const float* cls, const float* pos, const float* temporal, const int32_t* keep, int B, int T, int n,
                    int K, int D, float* x, void* stream) {
  if (!pe || !cls || !pos || !temporal || !x || D <= 0 || D % 4 != 0) return EGV_ERR_ARG;
  if (B <= 0 || T <= 0 || K < 1 || K > n) return EGV_ERR_ARG;
  dim3 grid;
  if (!grid_of((long)B * (1 + (long)T * K) * (D / 4), grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (keep) EGV_LAUNCH(assemble_tokens_kernel<true>, grid, dim3(256), 0, s, pe, cls, pos, temporal, B, T, n, D, x, keep, K);
  else EGV_LAUNCH(assemble_tokens_kernel<false>, grid, dim3(256), 0, s, pe, cls, pos, temporal, B, T, n, D, x, keep, K);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// its backward.  With K tokens per frame the tokens ARE a [B, 1 + T*K, D] sequence: d_temporal and d_pe do not know about the table;
// only the position sums do (d_pos has n + 1 rows either way).
int assemble_bwd_launch(const float* dx, const int32_t* keep, int B, int T, int n, int K, int D, int T_model, float* d_pe,
                        float* d_cls, float* d_pos, float* d_temporal, void* stream) {
  if (!dx || D <= 0 || D % 4 != 0 || B <= 0 || T <= 0 || T > T_model || K < 1 || K > n) return EGV_ERR_ARG;
  dim3 pe_grid;
  if (!grid_of((long)B * T * K * (D / 4), pe_grid)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (d_pos && d_cls) {
    if (hipMemsetAsync(d_pos, 0, sizeof(float) * (size_t)(n + 1) * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    if (hipMemsetAsync(d_cls, 0, sizeof(float) * (size_t)D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    if (keep) EGV_LAUNCH(assemble_bwd_pos_sel_kernel, dim3(n + 1, 4), dim3(256), 0, s, dx, keep, B, T, n, K, D, d_pos, d_cls);
    else EGV_LAUNCH(assemble_bwd_pos_kernel, dim3(n + 1, 4), dim3(256), 0, s, dx, B, T, n, D, d_pos, d_cls);
    EGV_CHECK_LAUNCH();
  }
  if (d_temporal) {
    if (hipMemsetAsync(d_temporal, 0, sizeof(float) * (size_t)T_model * D, s) != hipSuccess) return EGV_ERR_LAUNCH;
    EGV_LAUNCH(assemble_bwd_temporal_kernel, dim3(T, (D + 63) / 64, 32), dim3(256), 0, s, dx, B, T, K, D, T_model, d_temporal);
    EGV_CHECK_LAUNCH();
  }
  if (d_pe) {
    EGV_LAUNCH(assemble_bwd_pe_kernel, pe_grid, dim3(256), 0, s, dx, B, T, K, D, d_pe);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

}  // namespace

extern "C" int egv_patch_keep_draw(int32_t B, int32_t n, int32_t K, uint64_t seed, const uint64_t* seed_dev, int32_t* keep,
                                   void* stream) {
  if (!keep || B <= 0 || K < 1 || K > n || n > KEEP_MAX_N) return EGV_ERR_ARG;
  EGV_LAUNCH(patch_keep_draw_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, n, K, egv_make_drop(0.f, seed, seed_dev), keep);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_patch_gather(const float* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                                egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  return patch_gather_launch<false>(video, BT, 1, C, H, W, P, nullptr, 0, a_hi, a_lo, lda, PatchNorm{}, stream);
}

extern "C" int egv_patch_gather_sel(const float* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                                    const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  if (!keep) return EGV_ERR_ARG;
  return patch_gather_launch<false>(video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, lda, PatchNorm{}, stream);
}

extern "C" int egv_patch_gather_u8(const uint8_t* video, int32_t BT, int32_t C, int32_t H, int32_t W, int32_t P,
                                   const float* mean, const float* std, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda,
                                   void* stream) {
  PatchNorm nrm{};
  if (!fill_norm(nrm, mean, std, C)) return EGV_ERR_ARG;
  return patch_gather_launch<true>(video, BT, 1, C, H, W, P, nullptr, 0, a_hi, a_lo, lda, nrm, stream);
}

extern "C" int egv_patch_gather_u8_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                                       const float* mean, const float* std, const int32_t* keep, int32_t K, egv_bf16* a_hi,
                                       egv_bf16* a_lo, int64_t lda, void* stream) {
  PatchNorm nrm{};
  if (!keep || !fill_norm(nrm, mean, std, C)) return EGV_ERR_ARG;
  return patch_gather_launch<true>(video, BT, T, C, H, W, P, keep, K, a_hi, a_lo, lda, nrm, stream);
}

extern "C" int egv_patch_gather_u8_aug(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                       int32_t R, int32_t P, const int32_t* boxes, const float* mean, const float* std,
                                       egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  return patch_gather_aug_launch(video, BT, T, C, Hs, Ws, R, P, boxes, nullptr, mean, std, nullptr, 0, a_hi, a_lo, lda, stream);
}

extern "C" int egv_patch_gather_u8_aug_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                           int32_t R, int32_t P, const int32_t* boxes, const float* mean, const float* std,
                                           const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda,
                                           void* stream) {
  if (!keep) return EGV_ERR_ARG;
  return patch_gather_aug_launch(video, BT, T, C, Hs, Ws, R, P, boxes, nullptr, mean, std, keep, K, a_hi, a_lo, lda, stream);
}

extern "C" int egv_patch_gather_u8_aug_color(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                             int32_t R, int32_t P, const int32_t* boxes, const float* color, const float* mean,
                                             const float* std, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  if (!color || C != 3) return EGV_ERR_ARG;
  return patch_gather_aug_launch(video, BT, T, C, Hs, Ws, R, P, boxes, color, mean, std, nullptr, 0, a_hi, a_lo, lda, stream);
}

extern "C" int egv_patch_gather_u8_aug_color_sel(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws,
                                                 int32_t R, int32_t P, const int32_t* boxes, const float* color, const float* mean,
                                                 const float* std, const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo,
                                                 int64_t lda, void* stream) {
  if (!color || C != 3 || !keep) return EGV_ERR_ARG;
  return patch_gather_aug_launch(video, BT, T, C, Hs, Ws, R, P, boxes, color, mean, std, keep, K, a_hi, a_lo, lda, stream);
}

extern "C" int egv_patch_gather_mix(const void* video, int32_t u8, int32_t BT, int32_t T, int32_t C, int32_t H, int32_t W, int32_t P,
                                    const float* mean, const float* std, const int32_t* mix_idx, const float* mix_lam,
                                    const int32_t* keep, int32_t K, egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  PatchNorm nrm{};
  if (!u8) return patch_gather_mix_launch<false>(video, BT, T, C, H, W, P, mix_idx, mix_lam, keep, K, a_hi, a_lo, lda, nrm, stream);
  if (!fill_norm(nrm, mean, std, C)) return EGV_ERR_ARG;
  return patch_gather_mix_launch<true>(video, BT, T, C, H, W, P, mix_idx, mix_lam, keep, K, a_hi, a_lo, lda, nrm, stream);
}

extern "C" int egv_patch_gather_u8_aug_mix(const uint8_t* video, int32_t BT, int32_t T, int32_t C, int32_t Hs, int32_t Ws, int32_t R,
                                           int32_t P, const int32_t* boxes, const float* color, const float* mean, const float* std,
                                           const int32_t* mix_idx, const float* mix_lam, const int32_t* keep, int32_t K,
                                           egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  return patch_gather_aug_mix_launch(video, BT, T, C, Hs, Ws, R, P, boxes, color, mean, std, mix_idx, mix_lam, keep, K, a_hi, a_lo, lda,
                                     stream);
}

extern "C" int egv_patch_gather_u8_eval(const uint8_t* frames, int32_t F, const int32_t* index, int32_t BT, int32_t C, int32_t Hs,
                                        int32_t Ws, int32_t S, int32_t R, int32_t P, const float* mean, const float* std,
                                        egv_bf16* a_hi, egv_bf16* a_lo, int64_t lda, void* stream) {
  PatchNorm nrm{};
  if (F <= 0 || Hs <= 0 || Ws <= 0 || S <= 0 || R % 4 != 0 || !fill_norm(nrm, mean, std, C)) return EGV_ERR_ARG;
  if (!index && BT > F) return EGV_ERR_ARG;                     // index == NULL: output frame bt IS bank frame bt
  if (!gather_geom_ok(frames, a_hi, BT, 1, C, R, R, P, lda, 2)) return EGV_ERR_ARG;
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
  dim3 grid;
  if (!grid_of((long)BT * C * R * (R / 4), grid)) return EGV_ERR_ARG;
  if (g.H1 == Hs && g.W1 == Ws) {
    EGV_LAUNCH(patch_gather_eval_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, frames, index, g, a_hi, a_lo, (long)lda, nrm);
  } else {
    EGV_LAUNCH(patch_gather_eval_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, frames, index, g, a_hi, a_lo, (long)lda, nrm);
  }
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_assemble_tokens(const float* pe, const float* cls, const float* pos, const float* temporal,
                                   int32_t B, int32_t T, int32_t n, int32_t D, float* x, void* stream) {
  return assemble_launch(pe, cls, pos, temporal, nullptr, B, T, n, n, D, x, stream);
}

extern "C" int egv_assemble_tokens_sel(const float* pe, const float* cls, const float* pos, const float* temporal,
                                       const int32_t* keep, int32_t B, int32_t T, int32_t n, int32_t K, int32_t D, float* x,
                                       void* stream) {
  if (!keep) return EGV_ERR_ARG;
  return assemble_launch(pe, cls, pos, temporal, keep, B, T, n, K, D, x, stream);
}

extern "C" int egv_assemble_tokens_bwd(const float* dx, int32_t B, int32_t T, int32_t n, int32_t D, int32_t T_model,
                                       float* d_pe, float* d_cls, float* d_pos, float* d_temporal, void* stream) {
  return assemble_bwd_launch(dx, nullptr, B, T, n, n, D, T_model, d_pe, d_cls, d_pos, d_temporal, stream);
}

extern "C" int egv_assemble_tokens_bwd_sel(const float* dx, const int32_t* keep, int32_t B, int32_t T, int32_t n, int32_t K,
                                           int32_t D, int32_t T_model, float* d_pe, float* d_cls, float* d_pos, float* d_temporal,
                                           void* stream) {
  if (!keep) return EGV_ERR_ARG;
  return assemble_bwd_launch(dx, keep, B, T, n, K, D, T_model, d_pe, d_cls, d_pos, d_temporal, stream);
}
