// Tile pieces shared by the contrastive heads that walk the similarity in 64 x 64 tiles without storing it (egonce_long.hip: the long
// and the queue head; sigmoid_head.hip): the prep kernel and its outputs, the column-range split, and the steps of a walk -- the
// prologue (lane coordinates, A operand), the LDS tile, the bit-packed noun / verb mask tile, the X^T fragment product on the
// fp32-input MFMA, the second product dA += G . B with its store -- and the finish kernel (sum of the partials + the backward of the
// row normalisation).
//
// The walk.  Workgroup = (64 rows of A, a range of 64-row column tiles); a wave owns 16 rows and keeps their operand in registers
// (EGL_WALK_LDS, EGL_WALK_BEGIN).  Per tile: barrier, the tile's rows and the mask tile go to LDS (egl_stage_tile, egl_mask_tile; a
// head may stage more), barrier, X^T fragments (egl_xt) and the lane's mask words, row 16 wave + li of the mask tile (bit 4 g + r of
// word jf belongs to x[jf][r]); the head's own arithmetic on the 16 pairs of the lane; then, in a gradient walk, G -- formed in the
// registers of the X^T fragment, which IS the operand layout of the next product (lane = row i, lane group = k) -- goes through
// EGL_SECOND_PRODUCT on the same MFMA with B_J read from the LDS tile, and EGL_STORE_GPART writes the raw partials of the column
// range at the end.
//
// The prologue, the second product and the store are macros over the names of the kernel's scope, not functions: the same
// statements behind a call boundary come out of the compiler as other machine code for the walk instances ("One walk").
//
// k order.  The 16x16x4 MFMA takes k = lane >> 4 from each lane.  A lane reads FOUR consecutive floats (one 16-byte LDS read)
// and feeds element t to MFMA t, so MFMA t of chunk c sums k = 16 c + 4 (lane >> 4) + t; both operands use the same map, which
// only permutes the order of the fma chain.  The second product uses the same trick on the OUTPUT column: MFMA t of a 64-wide
// chunk produces d = 64 c + 4 (lane & 15) + t, so a lane ends with four consecutive d and stores 16 bytes.
#pragma once
#include "head_common.h"

namespace {

constexpr int EGL_TILE = 64;          // rows per tile (A rows per workgroup, B rows per LDS tile)
constexpr int EGL_GRAD_WGS = 256;     // the gradient walks aim at this many workgroups: their partials cost memory and a pass

// `rtiles` row tiles against `ctiles` column tiles, about `target` workgroups -> tiles per column range and ranges
inline void egl_split(int rtiles, int ctiles, int target, int& tps, int& ns) {
  int want = (target + rtiles - 1) / rtiles;
  if (want > ctiles) want = ctiles;
  tps = (ctiles + want - 1) / want;
  ns = (ctiles + tps - 1) / tps;       // no empty range
}

// ------------------------------------------------------------------------------------------------ prep
// What the prep kernel writes, at the front of a tiled head's workspace; the head's own partial buffers follow from `total` on.
struct EglPrepLayout {
  int np, Dp, wn, W, ntiles;
  long tn, vn, words, norms, flags, total;   // offsets in floats
};

inline EglPrepLayout egl_prep_layout(int n, int D, int dn, int dv) {
  EglPrepLayout L;
  L.np = (n + EGL_TILE - 1) / EGL_TILE * EGL_TILE;
  L.Dp = D <= 64 ? 64 : 256;                         // the two widths the tile kernels are compiled for
  L.wn = ((dn + 31) / 32 + 3) / 4 * 4;
  L.W = L.wn + ((dv + 31) / 32 + 3) / 4 * 4;
  L.ntiles = L.np / EGL_TILE;
  const long np = L.np;
  long o = 0;
  L.tn = o;     o += np * L.Dp;
  L.vn = o;     o += np * L.Dp;
  L.words = o;  o += np * L.W;
  L.norms = o;  o += 2 * np;
  L.flags = o;  o += np;
  L.total = o;
  return L;
}

// the kernel of a launcher template fn<DP>, by the layout L in scope
#define EGL_BY_DP(fn, ...) (L.Dp == 64 ? fn<64>(__VA_ARGS__) : fn<256>(__VA_ARGS__))

// the mask mode of egl_mask_tile, as egonce_rows_kernel picks it: noun and verb, noun only, else verb (the reference's else-branch)
inline int egl_mask_mode(const float* noun, int use_noun, int use_verb) {
  return !noun ? 0 : (use_noun && use_verb) ? 1 : use_noun ? 2 : 3;
}

__global__ __launch_bounds__(256) void egl_prep_kernel(const float* __restrict__ text, const float* __restrict__ video,
                                                       const float* __restrict__ noun, const float* __restrict__ verb, int n,
                                                       int np, int D, int Dp, int dn, int dv, int wn, int W, float eps,
                                                       float* __restrict__ tn, float* __restrict__ vn,
                                                       uint32_t* __restrict__ words, float* __restrict__ norms,
                                                       float* __restrict__ flags) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (i >= n) {                                       // the padding rows of the last tile
    for (int d = threadIdx.x; d < Dp; d += 256) {
      tn[(long)i * Dp + d] = 0.f;
      vn[(long)i * Dp + d] = 0.f;
    }
    for (int w = threadIdx.x; w < W; w += 256) words[(long)i * W + w] = 0u;
    if (threadIdx.x == 0) {
      norms[i] = 0.f;
      norms[np + i] = 0.f;
      flags[i] = 0.f;
    }
    return;
  }
  float st = 0.f, sv = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    const float a = text[(long)i * D + d], b = video[(long)i * D + d];
    st += a * a;
    sv += b * b;
  }
  const float nt = sqrtf(egv_block_sum_256(st, sh));
  const float nv = sqrtf(egv_block_sum_256(sv, sh));
  const float ct = fmaxf(nt, eps), cv = fmaxf(nv, eps);
  for (int d = threadIdx.x; d < Dp; d += 256) {
    tn[(long)i * Dp + d] = d < D ? text[(long)i * D + d] / ct : 0.f;
    vn[(long)i * Dp + d] = d < D ? video[(long)i * D + d] / cv : 0.f;
  }
  int bad = 0;
  if (noun) {
    // 64 entries per wave and step: the ballot of (entry > 0) is two of the row's words
    for (int base = wave * 64; base < wn * 32; base += 256) {
      const int c = base + lane;
      const float e = c < dn ? noun[(long)i * dn + c] : 0.f;
      bad |= !(e >= 0.f);
      const unsigned long long b = __ballot(e > 0.f);
      if (lane == 0) {
        words[(long)i * W + base / 32] = (uint32_t)b;
        words[(long)i * W + base / 32 + 1] = (uint32_t)(b >> 32);
      }
    }
    for (int base = wave * 64; base < (W - wn) * 32; base += 256) {
      const int c = base + lane;
      const float e = c < dv ? verb[(long)i * dv + c] : 0.f;
      bad |= !(e >= 0.f);
      const unsigned long long b = __ballot(e > 0.f);
      if (lane == 0) {
        words[(long)i * W + wn + base / 32] = (uint32_t)b;
        words[(long)i * W + wn + base / 32 + 1] = (uint32_t)(b >> 32);
      }
    }
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    norms[i] = nt;
    norms[np + i] = nv;
    flags[i] = bad ? 1.f : 0.f;
  }
}

inline int egl_launch_prep(const EglPrepLayout& L, const float* text, const float* video, const float* noun, const float* verb,
                           int n, int D, int dn, int dv, float eps, float* work, hipStream_t s) {
  EGV_LAUNCH(egl_prep_kernel, dim3(L.np), dim3(256), 0, s, text, video, noun, verb, n, L.np, D, L.Dp, dn, dv, L.wn, L.W, eps,
             work + L.tn, work + L.vn, (uint32_t*)(work + L.words), work + L.norms, work + L.flags);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ------------------------------------------------------------------------------------------------ tile pieces
// B rows j0 .. j0 + 63 -> LDS image [64][DP + 4] (the 4 floats of padding spread the rows over the banks).  ZERO_TAIL: the rows
// from `valid` on are written as zeros and not read (an unused queue slot may hold anything).
template <int DP, bool ZERO_TAIL = false>
__device__ __forceinline__ void egl_stage_tile(float* bt, const float* __restrict__ B, int j0, int valid = EGL_TILE) {
  constexpr int LD = DP + 4, C4 = DP / 4;
  for (int idx = threadIdx.x; idx < EGL_TILE * C4; idx += 256) {
    const int r = idx / C4, c4 = idx % C4;
    f32x4_t v = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if (!ZERO_TAIL || r < valid) v = *(const f32x4_t*)(B + (long)(j0 + r) * DP + 4 * c4);
    *(f32x4_t*)(bt + r * LD + 4 * c4) = v;
  }
}

// The 64 x 64 mask tile between the words of the A rows (wa, rows i0 ..) and those of the tile's rows (wb, rows j0 ..; the same
// array, or a queue's), 16 bits per thread: thread (row i0 + (tid & 63), wave q) covers columns j0 + 16 q .. + 15; the words of a
// column row are wave-uniform.  mode 0: nothing; 1: noun AND verb; 2: noun; 3: verb.  diag: add i == j.  mb: [64][4] words.
__device__ __forceinline__ void egl_mask_tile(const uint32_t* __restrict__ wa, const uint32_t* __restrict__ wb, int W, int wn,
                                              int mode, int i0, int j0, int diag, uint32_t* mb) {
  const int il = threadIdx.x & 63;
  const int jq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + il, jb = j0 + jq * 16;
  uint32_t bits = 0u;
  if (mode != 0) {
    uint32_t hn[16], hv[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) hn[jj] = hv[jj] = 0u;
    const u32x4_t* wi = (const u32x4_t*)(wa + (long)gi * W);
    const int qn = wn >> 2, qa = W >> 2;
    if (mode != 3)
      for (int q = 0; q < qn; ++q) {
        const u32x4_t a = wi[q];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const u32x4_t b = ((const u32x4_t*)(wb + (long)(jb + jj) * W))[q];         // wave-uniform: scalar loads
          hn[jj] |= (a[0] & b[0]) | (a[1] & b[1]) | (a[2] & b[2]) | (a[3] & b[3]);
        }
      }
    if (mode != 2)
      for (int q = qn; q < qa; ++q) {
        const u32x4_t a = wi[q];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const u32x4_t b = ((const u32x4_t*)(wb + (long)(jb + jj) * W))[q];
          hv[jj] |= (a[0] & b[0]) | (a[1] & b[1]) | (a[2] & b[2]) | (a[3] & b[3]);
        }
      }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const bool m = mode == 1 ? (hn[jj] != 0u && hv[jj] != 0u) : (mode == 2 ? hn[jj] != 0u : hv[jj] != 0u);
      bits |= (m ? 1u : 0u) << jj;
    }
  }
  const int dj = gi - jb;
  if (diag && dj >= 0 && dj < 16) bits |= 1u << dj;
  mb[il * 4 + jq] = bits;
}

// X^T fragments of the wave's 16 rows against the LDS tile: x[jf][r] = <A row (lane & 15), B row 16 jf + 4 (lane >> 4) + r>
template <int DP>
__device__ __forceinline__ void egl_xt(const float* bt, const f32x4_t (&a)[DP / 16], int li, int g, f32x4_t (&x)[4]) {
  constexpr int LD = DP + 4;
#pragma unroll
  for (int jf = 0; jf < 4; ++jf) x[jf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < DP / 16; ++c) {
    f32x4_t b[4];
#pragma unroll
    for (int jf = 0; jf < 4; ++jf) b[jf] = *(const f32x4_t*)(bt + (jf * 16 + li) * LD + 16 * c + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int jf = 0; jf < 4; ++jf) x[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[jf][t], a[c][t], x[jf], 0, 0, 0);
  }
}

// What a walk kernel starts with, declared in the kernel's own scope: the two LDS images at the front of its dynamic LDS `smem`
// (bt [64][DP + 4]: the column tile; mb [64][4]: the mask tile; a head's own staging follows from mb + 4 * EGL_TILE on), the lane's
// coordinates (wave: uniform; li = lane & 15, g = lane >> 4; i0: first row of the workgroup, gi: this lane's row), ntiles = np / 64,
// the column tiles t0 .. t1 - 1 of the workgroup out of `tiles` (an expression, which may use ntiles), and row gi of A as the
// operand of egl_xt (the floats 16 c + 4 g .. + 3 of every chunk c).
#define EGL_WALK_LDS(DP)                                      \
  float* bt = (float*)smem;                                   \
  uint32_t* mb = (uint32_t*)(bt + EGL_TILE * ((DP) + 4))
#define EGL_WALK_BEGIN(DP, A, np, tiles, tps)                                                    \
  const int lane = threadIdx.x & 63;                                                             \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                             \
  const int li = lane & 15, g = lane >> 4;                                                       \
  const int i0 = blockIdx.x * EGL_TILE;                                                          \
  const int ntiles = (np) / EGL_TILE;                                                            \
  const int t0 = blockIdx.y * (tps), t1 = min((tiles), t0 + (tps));                              \
  const int gi = i0 + wave * 16 + li;                                                            \
  f32x4_t a[(DP) / 16];                                                                          \
  _Pragma("unroll") for (int c = 0; c < (DP) / 16; ++c) a[c] = *(const f32x4_t*)((A) + (long)gi * (DP) + 16 * c + 4 * g)

// the accumulators of the second product
template <int DP>
__device__ __forceinline__ void egl_acc_zero(f32x4_t (&acc)[DP / 64][4]) {
#pragma unroll
  for (int c = 0; c < DP / 64; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[c][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
}

// dA[i][d] += sum_j G[i][j] B[j][d] on the prologue's names: x[jf][r] holds G and is the A operand of k-step (jf, r) as it stands
// (k = j = 16 jf + 4 g + r), B_J is read from the LDS tile bt, acc[DP / 64][4] are the accumulators.
#define EGL_SECOND_PRODUCT(DP)                                                                           \
  _Pragma("unroll") for (int jf = 0; jf < 4; ++jf)                                                       \
  _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                          \
  _Pragma("unroll") for (int c = 0; c < (DP) / 64; ++c) {                                                \
    const f32x4_t bv = *(const f32x4_t*)(bt + (jf * 16 + 4 * g + r) * ((DP) + 4) + 64 * c + 4 * li);     \
    _Pragma("unroll") for (int tt = 0; tt < 4; ++tt)                                                     \
      acc[c][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[jf][r], bv[tt], acc[c][tt], 0, 0, 0);          \
  }

// acc[c][tt][rr]: row i0 + 16 wave + 4 g + rr, column 64 c + 4 li + tt -> gpart [ranges][np][DP]; a walk with no tile stores zeros
#define EGL_STORE_GPART(DP, gpart, np)                                                                   \
  {                                                                                                      \
    float* out = (gpart) + ((long)blockIdx.y * (np) + i0 + wave * 16 + 4 * g) * (DP) + 4 * li;           \
    _Pragma("unroll") for (int c = 0; c < (DP) / 64; ++c)                                                \
    _Pragma("unroll") for (int rr = 0; rr < 4; ++rr)                                                     \
      *(f32x4_t*)(out + (long)rr * (DP) + 64 * c) =                                                      \
          (f32x4_t){acc[c][0][rr], acc[c][1][rr], acc[c][2][rr], acc[c][3][rr]};                         \
  }

// sum of the column-range partials in a fixed order + the backward of the row normalisation (egv_norm_bwd)
__global__ __launch_bounds__(256) void egl_finish_kernel(const float* __restrict__ gpart, int ns, const float* __restrict__ an,
                                                         const float* __restrict__ norms, int np, int D, int Dp, float eps,
                                                         float* __restrict__ out) {
  __shared__ float sh[4];
  const int i = blockIdx.x, d = threadIdx.x;
  float gsum = 0.f, th = 0.f;
  if (d < Dp) {
    for (int r = 0; r < ns; ++r) gsum += gpart[((long)r * np + i) * Dp + d];
    th = an[(long)i * Dp + d];
  }
  const float proj = egv_block_sum_256(th * gsum, sh);
  const float nrm = norms[i];
  if (d < D) out[(long)i * D + d] = egv_norm_bwd(gsum, th, proj, nrm, eps);
}

inline bool egl_args_ok(int n, int D, int dn, int dv) {
  return n >= 1 && n <= 65536 && D >= 4 && D <= 256 && D % 4 == 0 && dn >= 0 && dv >= 0 && dn <= 65536 && dv <= 65536;
}

}  // namespace
