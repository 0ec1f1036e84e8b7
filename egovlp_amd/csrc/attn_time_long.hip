// Time attention for 16 < T <= 64 frames on the matrix cores.  The semantics are those of attn_time_mfma.hip (its header is the
// specification: per (clip b, location i, head h) the T frame queries attend to the CLS key + the T frame keys of that location, the
// clip's CLS query rides along as one more query, forward as an un-normalised partial (o[64], m, l) per location in cls_ws, backward
// with the global lse / delta); what changes is the tiling.  The frames of one location are NT = ceil(T / 16) 16-row tiles, and ONE
// WORKGROUP of NT waves owns one (b, location, h):
//   * the K, V (backward: K, Q, dO, V) images of all NT tiles are SHARED in LDS: rows 0 .. 16 NT - 1 = the frames (frames >= T repeat
//     frame T - 1 and are masked), row 16 NT = the CLS token's row, rows 16 NT + 1 .. + 4 zero.  Wave w fetches tile w of every
//     operand with the same two coalesced 16-B-per-lane loads as the short kernel; one barrier publishes the images;
//   * forward: wave w owns query tile w.  Its NT score tiles S' = K Q^T (rows = keys, columns = queries) stay in accumulators
//     (4 VGPRs each), so the softmax is one pass over registers -- no online rescaling --, and P feeds O^T = V^T P without leaving its
//     lane.  The contraction of an MFMA covers TWO 16-row "slots" (elements 0..3 / 4..7 of a row fragment): the frame tiles pair up,
//     and the CLS key is one more slot (its row in lane group 0, zero rows elsewhere), so T = 32 costs 2 products per output tile,
//     T = 48 2, T = 64 3.  Wave 0 also carries the clip's CLS query (column 0 of a second B operand against the same A fragments);
//   * backward: wave w owns query tile w for dQ (orientation 1: rows = keys of ALL tiles, columns = its queries) and key tile w for
//     dK / dV (orientation 2: rows = queries of ALL tiles + the CLS query, columns = its keys); scores and dP are recomputed with
//     the operands swapped instead of being transposed through LDS, as in the short kernel.  The only values that cross waves are
//     the 16 NT row sums delta_q = sum_k P dP (computed in orientation 1, read in orientation 2: 64 floats of LDS and one barrier),
//     the queries' lse (64 more floats, published with the images)
//     and the CLS token's dq / dk / dv partials (LDS adds, then 192 atomics per workgroup into dcls).  Every dQ / dK / dV row leaves
//     complete and is written once, as whole 128-byte rows through a staging tile (the wave's own rows of the Q image in the forward,
//     of the V image in the backward: nobody else reads them any more by then).
// LDS per workgroup, (16 NT + 5) rows x 128 B per image and plane: forward 3 images, backward 4 -- one product: 14.2 / 18.9 KB
// (NT = 2), 26.5 / 35.3 KB (NT = 4); three products: twice that (70.7 KB for the NT = 4 backward: two workgroups per CU).  Accumulators:
// NT score tiles (+ NT dP tiles in the backward) of 4 VGPRs, doubled in wave 0 for the CLS query.
// What bounds it.  The expectation was HBM, like the short kernel: every q / k / v / dO row is read exactly once and every output row
// written once, in the same whole-row accesses.  Measured at ViT-B geometry in the benchmarked pairing: the forward runs
// at 0.52 - 0.53 of HBM peak at T = 32 and T = 64 (the short kernel: 0.70 in the same run), the one-product backward at 0.44 (T = 32)
// and 0.29 (T = 64; 0.59 at T = 16).  Per token the matrix work grows with T + 1 while the bytes do not: a wave of the T = 64
// backward fetches the bytes of a T = 16 wave but issues 124 MFMAs (56 there) among 3 600 static instructions (2 250 there), at 3 waves
// per SIMD (157 VGPRs), and every load of a workgroup sits in front of its first barrier -- at NT = 4 the backward is bound by
// instruction issue and latency (little of a workgroup's compute overlaps loads), not by HBM.
#include "attn_common.h"
#include "attn_time_tile.h"
#include "egovlp_hip.h"

namespace {

constexpr int HD64 = 64;

template <int NT>
struct Img {
  static constexpr int CLS = 16 * NT;                             // the CLS token's row; the three rows behind it are zero
  static constexpr int ZERO = 16 * NT + 4;                        // a zero row of its own (what lane groups 1..3 read for the CLS slot)
  static constexpr int BYTES = (16 * NT + 5) * ATT_ROW_BYTES;
};

// frame f of location i -> token of the clip; frames >= T repeat the last one (masked by the callers)
__device__ __forceinline__ long frame_token(int f, int T, int n, int i) { return 1 + (long)(f < T ? f : T - 1) * n + i; }

__device__ __forceinline__ Tile load_frames(const bf16_t* __restrict__ plane, long part_base, int f0, int T, int n, int i, long ts, int lane) {
  Tile t;
#pragma unroll
  for (int it = 0; it < 2; ++it)
    t.r[it] = *(const u32x4_t*)(plane + part_base + frame_token(f0 + 8 * it + (lane >> 3), T, n, i) * ts + (lane & 7) * 8);
  return t;
}
// rows cls_row .. cls_row + 4 of an image: the CLS token's row (64 elements at `src`), then four zero rows
__device__ __forceinline__ void put_cls(char* img, int cls_row, const bf16_t* __restrict__ src, int lane) {
  if (lane < 40) {
    const int row = cls_row + (lane >> 3), chunk = lane & 7;
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (lane < 8) v = *(const u32x4_t*)(src + chunk * 8);
    *(u32x4_t*)(img + row * ATT_ROW_BYTES + ((chunk ^ (row & 7)) << 4)) = v;
  }
}
// column-contraction fragment of the CLS slot: the CLS row in lane p = 0 (row 0 of an A operand, column 0 of a B operand), zero elsewhere
__device__ __forceinline__ bf16x8_t frag_cls(const char* img, int cls_row, int ks, int lane) {
  const bf16x8_t z = __builtin_bit_cast(bf16x8_t, (u32x4_t){0u, 0u, 0u, 0u});
  const int chunk = (lane >> 4) + 4 * ks;
  const bf16x8_t v = *(const bf16x8_t*)(img + cls_row * ATT_ROW_BYTES + ((chunk ^ (cls_row & 7)) << 4));
  return (lane & 15) == 0 ? v : z;
}
// the image row a lane addresses for the transpose read of slot s: s < NT the frame tile s (rows 16 s + 4g + j), s == NT the CLS slot
// (rows CLS + j in lane group 0, the zero row in the others), s > NT nothing (the zero row)
template <int NT>
__device__ __forceinline__ int slot_row(int s, int g, int p) {
  if (s < NT) return 16 * s + 4 * g + (p >> 2);
  return (s == NT && g == 0) ? Img<NT>::CLS + (p >> 2) : Img<NT>::ZERO;
}
// row-contraction fragment over the slots (sa, sb): elements 0..3 = rows 4g + j of slot sa, elements 4..7 = of slot sb
template <int NT>
__device__ __forceinline__ bf16x8_t frag_slots(const char* img, int sa, int sb, int col0, int lane) {
  const int g = lane >> 4, p = lane & 15;
  const int col = col0 + ((p & 3) << 2);
  const s16x4_t x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(img + att_off(slot_row<NT>(sa, g, p), col)));
  const s16x4_t y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(img + att_off(slot_row<NT>(sb, g, p), col)));
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  const s16x8_t z = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
  return __builtin_bit_cast(bf16x8_t, z);
}
// accumulator-layout values of the NT frame tiles + the CLS slot's value (lane group 0, element 0; the callers pass 0 elsewhere)
// -> the B operands of the (NT + 2) / 2 slot pairs
template <int NT, bool F16>
__device__ __forceinline__ void pack_slots(const float (&v)[NT][4], float cls, bf16x8_t (&hi)[(NT + 2) / 2], bf16x8_t (&lo)[(NT + 2) / 2]) {
  constexpr int NP = (NT + 2) / 2;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f}, c[4] = {cls, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    if (2 * u + 1 < NT) pack_b<F16>(v[2 * u], v[2 * u + 1 < NT ? 2 * u + 1 : 0], hi[u], lo[u]);
    else if (2 * u + 1 == NT) pack_b<F16>(v[2 * u < NT ? 2 * u : 0], c, hi[u], lo[u]);
    else pack_b<F16>(c, zero, hi[u], lo[u]);
  }
}
// sum over the slot pairs: A = the image's row fragments of channel tile c, B = the packed slots
template <int PASSES, int NT, bool F16>
__device__ __forceinline__ f32x4_t mma_slots(const char* ih, const char* il, int c, int lane, const bf16x8_t (&bh)[(NT + 2) / 2],
                                             const bf16x8_t (&bl)[(NT + 2) / 2], f32x4_t acc) {
#pragma unroll
  for (int u = 0; u < (NT + 2) / 2; ++u) {
    const bf16x8_t ah = frag_slots<NT>(ih, 2 * u, 2 * u + 1, 16 * c, lane);
    const bf16x8_t al = PASSES == 3 ? frag_slots<NT>(il, 2 * u, 2 * u + 1, 16 * c, lane) : ah;
    acc = att_mma<PASSES, F16>(ah, al, bh[u], bl[u], acc);
  }
  return acc;
}

// rows of the staged tile (frames f0 .. f0 + 15 of location i) -> plane rows, whole 128-byte rows (attn_time_tile.h stage4)
template <int SITE>
__device__ __forceinline__ void flush_frames(const char* sh, const char* sl, bf16_t* __restrict__ ph, bf16_t* __restrict__ pl, long tok0, long ts,
                                             long col0, int f0, int T, int n, int i, int lane) {
  // the tile was written by other lanes of this wave: a wave barrier pins the order the hardware already keeps (see flush_rows of
  // attn_time_mfma.hip)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = 8 * it + (lane >> 3), chunk = lane & 7;
    if (f0 + row >= T) continue;
    const long o = (tok0 + 1 + (long)(f0 + row) * n + i) * ts + col0 + chunk * 8;
    const int lo = row * ATT_ROW_BYTES + ((chunk ^ (row & 7)) << 4);
    egv_store<SITE>(ph + o, *(const u32x4_t*)(sh + lo));
    if (pl) egv_store<SITE>(pl + o, *(const u32x4_t*)(sl + lo));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();           // ... and the staging rows may be overwritten only behind these reads
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NPL>
__device__ __forceinline__ void frags_cols(char* const (&img)[NPL], int r0, int lane, bf16x8_t (&f)[NPL][2]) {
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f[pl][ks] = att_frag_cols(img[pl], r0, ks, lane);
}
template <int NPL>
__device__ __forceinline__ void frags_cls(char* const (&img)[NPL], int cls_row, int lane, bf16x8_t (&f)[NPL][2]) {
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) f[pl][ks] = frag_cls(img[pl], cls_row, ks, lane);
}

// ------------------------------------------------------------------------------------------------------------ forward
template <int PASSES, int NT, bool F16 = false>
__global__ __launch_bounds__(64 * NT) void attn_time_long_fwd_kernel(const bf16_t* __restrict__ qh, const bf16_t* __restrict__ ql, int B, int T,
                                                                     int n, int H, bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo,
                                                                     float* __restrict__ lse, float* __restrict__ cls_ws, int out_fmt) {
  constexpr int NPL = PASSES == 3 ? 2 : 1, LO = NPL - 1, NP = (NT + 2) / 2;
  using I = Img<NT>;
  __shared__ __attribute__((aligned(128))) char smem[3 * NPL * I::BYTES];      // the Q, K and V images of every plane
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, p = lane & 15;
  const int h = (int)(blockIdx.x % H);
  const long r = blockIdx.x / H;
  const int i = (int)(r % n), b = (int)(r / n);
  const long S = 1 + (long)T * n, HD = (long)H * HD64, ts = 3 * HD;
  const long cbase = (long)b * S * ts + (long)h * HD64;          // the clip's CLS token, q part
  const int f0 = 16 * w;                                         // this wave's tile: frames f0 .. f0 + 15
  const bf16_t* planes[2] = {qh, ql};
  char *qim[NPL], *kim[NPL], *vim[NPL];
  {
    Tile qt[NPL], kt[NPL], vt[NPL];
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      qt[pl] = load_frames(planes[pl], cbase, f0, T, n, i, ts, lane);
      kt[pl] = load_frames(planes[pl], cbase + HD, f0, T, n, i, ts, lane);
      vt[pl] = load_frames(planes[pl], cbase + 2 * HD, f0, T, n, i, ts, lane);
    }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      qim[pl] = smem + (3 * pl) * I::BYTES;
      kim[pl] = smem + (3 * pl + 1) * I::BYTES;
      vim[pl] = smem + (3 * pl + 2) * I::BYTES;
      put_tile(qim[pl] + f0 * ATT_ROW_BYTES, qt[pl], lane);
      put_tile(kim[pl] + f0 * ATT_ROW_BYTES, kt[pl], lane);
      put_tile(vim[pl] + f0 * ATT_ROW_BYTES, vt[pl], lane);
      if (w == 0) {
        put_cls(qim[pl], I::CLS, planes[pl] + cbase, lane);
        put_cls(kim[pl], I::CLS, planes[pl] + cbase + HD, lane);
        put_cls(vim[pl], I::CLS, planes[pl] + cbase + 2 * HD, lane);
      }
    }
  }
  __syncthreads();

  // S' = K Q^T: rows = keys (16 kt + 4g + j), columns = this wave's queries (f0 + p); wave 0: a second set of columns whose column 0
  // is the clip's CLS query
  bf16x8_t q0[NPL][2], qc[NPL][2], kc[NPL][2];
  frags_cols<NPL>(qim, f0, lane, q0);
  frags_cls<NPL>(qim, I::CLS, lane, qc);
  frags_cls<NPL>(kim, I::CLS, lane, kc);
  f32x4_t s0[NT], s1[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    bf16x8_t k0[NPL][2];
    frags_cols<NPL>(kim, 16 * kt, lane, k0);
    s0[kt] = mma2<PASSES, F16>(k0[0], k0[LO], q0[0], q0[LO]);
    s1[kt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if (w == 0) s1[kt] = mma2<PASSES, F16>(k0[0], k0[LO], qc[0], qc[LO]);
  }
  const f32x4_t sc0 = mma2<PASSES, F16>(kc[0], kc[LO], q0[0], q0[LO]);      // CLS key (row 0: group 0, j = 0) x frame queries
  const f32x4_t sc1 = mma2<PASSES, F16>(kc[0], kc[LO], qc[0], qc[LO]);      // CLS key x CLS query

  const bool qv = f0 + p < T;                        // this lane's query column
  bf16x8_t b0h[NP], b0l[NP], b1h[NP], b1l[NP];
  float m0, l0, m1 = -3e38f, l1 = 0.f;
  {   // frame queries: softmax over the CLS key + the T frame keys
    float e[NT][4];
    float mx = (g == 0) ? sc0[0] * 0.125f : -3e38f;
    const float c = mx;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[kt][j] = (16 * kt + 4 * g + j < T) ? s0[kt][j] * 0.125f : -3e38f;
        mx = fmaxf(mx, e[kt][j]);
      }
    m0 = allg_max(mx);
    const float ec = (g == 0) ? __expf(c - m0) : 0.f;
    float sum = ec;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[kt][j] = (16 * kt + 4 * g + j < T) ? __expf(e[kt][j] - m0) : 0.f;
        sum += e[kt][j];
      }
    l0 = allg_sum(sum);
    pack_slots<NT, F16>(e, ec, b0h, b0l);
  }
  if (w == 0) {   // the clip's CLS query (column 0) against this location's keys (+ the CLS key, counted in location 0 only): un-normalised partial
    float e[NT][4];
    const bool own = g == 0 && p == 0 && i == 0;
    const float c = own ? sc1[0] * 0.125f : -3e38f;
    float mx = c;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[kt][j] = (p == 0 && 16 * kt + 4 * g + j < T) ? s1[kt][j] * 0.125f : -3e38f;
        mx = fmaxf(mx, e[kt][j]);
      }
    m1 = allg_max(mx);
    const float ec = own ? __expf(c - m1) : 0.f;
    float sum = ec;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[kt][j] = (p == 0 && 16 * kt + 4 * g + j < T) ? __expf(e[kt][j] - m1) : 0.f;
        sum += e[kt][j];
      }
    l1 = allg_sum(sum);
    pack_slots<NT, F16>(e, ec, b1h, b1l);
  }
  const float inv0 = 1.0f / l0;
  float* ws = cls_ws + (((long)b * H + h) * n + i) * 68;
  // the wave's own rows of the Q images are the staging tile: their fragments are in registers and no other wave reads them
  char* const sth = qim[0] + f0 * ATT_ROW_BYTES;
  char* const stl = PASSES == 3 ? qim[LO] + f0 * ATT_ROW_BYTES : nullptr;
  const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    // O^T tile c: rows = channels 16c + 4g + j, columns = queries; contraction over the key slots
    const f32x4_t o0 = mma_slots<PASSES, NT, F16>(vim[0], vim[LO], c, lane, b0h, b0l, z);
    stage4(sth, stl, p, 16 * c + 4 * g, o0, inv0, out_fmt);
    if (w == 0) {
      const f32x4_t o1 = mma_slots<PASSES, NT, F16>(vim[0], vim[LO], c, lane, b1h, b1l, z);
      if (p == 0) *(f32x4_t*)(ws + 16 * c + 4 * g) = o1;
    }
  }
  flush_frames<EGV_NT_ATTN_OUT>(sth, stl, out_hi, PASSES == 3 ? out_lo : nullptr, (long)b * S, HD, (long)h * HD64, f0, T, n, i, lane);
  if (g == 0 && qv && lse) lse[((long)b * H + h) * S + frame_token(f0 + p, T, n, i)] = m0 + __logf(l0);
  if (w == 0 && lane == 0) {
    ws[64] = m1;
    ws[65] = l1;
  }
}

// ------------------------------------------------------------------------------------------------------------ backward
template <int PASSES, int NT, bool F16 = false>
__global__ __launch_bounds__(64 * NT) void attn_time_long_bwd_kernel(const bf16_t* __restrict__ qh, const bf16_t* __restrict__ ql,
                                                                     const bf16_t* __restrict__ doh, const bf16_t* __restrict__ dol,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta, int B, int T,
                                                                     int n, int H, bf16_t* __restrict__ gh, bf16_t* __restrict__ gl,
                                                                     float* __restrict__ dcls, int gfmt) {
  constexpr int NPL = PASSES == 3 ? 2 : 1, LO = NPL - 1, NP = (NT + 2) / 2;
  using I = Img<NT>;
  __shared__ __attribute__((aligned(128))) char smem[4 * NPL * I::BYTES];      // the K, Q, dO and V images of every plane
  __shared__ __attribute__((aligned(16))) float red[192];                      // the CLS token's raw dq | dk | dv partials of this location
  __shared__ float dls[16 * NT];                                               // delta of the frame queries (sum_k P dP)
  __shared__ float lss[16 * NT];                                               // their log-sum-exp
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, p = lane & 15;
  const int h = (int)(blockIdx.x % H);
  const long r = blockIdx.x / H;
  const int i = (int)(r % n), b = (int)(r / n);
  const long S = 1 + (long)T * n, HD = (long)H * HD64, ts = 3 * HD;
  const long cbase = (long)b * S * ts + (long)h * HD64;
  const long cob = (long)b * S * HD + (long)h * HD64;            // dO of the CLS token
  const float* lb = lse + ((long)b * H + h) * S;
  const int f0 = 16 * w;
  const bf16_t* planes[2] = {qh, ql};
  const bf16_t* gplanes[2] = {doh, dol};
  for (int x = threadIdx.x; x < 192; x += 64 * NT) red[x] = 0.f;
  // every global value the wave needs is requested here, in front of the first barrier: the CLS row's lse and delta and the
  // log-sum-exp of the wave's 16 queries, which orientation 2 of the other waves reads as rows (lss, shared like the images)
  const float Lc = lb[0], dlc = delta[((long)b * H + h) * S];
  const float Lq = lb[frame_token(f0 + p, T, n, i)];
  char *kim[NPL], *qim[NPL], *gim[NPL], *vim[NPL];
  {
    Tile qt[NPL], kt[NPL], vt[NPL], gt[NPL];
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      qt[pl] = load_frames(planes[pl], cbase, f0, T, n, i, ts, lane);
      kt[pl] = load_frames(planes[pl], cbase + HD, f0, T, n, i, ts, lane);
      vt[pl] = load_frames(planes[pl], cbase + 2 * HD, f0, T, n, i, ts, lane);
      gt[pl] = load_frames(gplanes[pl], cob, f0, T, n, i, HD, lane);
    }
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
      kim[pl] = smem + (4 * pl) * I::BYTES;
      qim[pl] = smem + (4 * pl + 1) * I::BYTES;
      gim[pl] = smem + (4 * pl + 2) * I::BYTES;
      vim[pl] = smem + (4 * pl + 3) * I::BYTES;
      put_tile(qim[pl] + f0 * ATT_ROW_BYTES, qt[pl], lane);
      put_tile(kim[pl] + f0 * ATT_ROW_BYTES, kt[pl], lane);
      put_tile(vim[pl] + f0 * ATT_ROW_BYTES, vt[pl], lane);
      put_tile(gim[pl] + f0 * ATT_ROW_BYTES, gt[pl], lane);
      if (w == 0) {
        put_cls(qim[pl], I::CLS, planes[pl] + cbase, lane);
        put_cls(kim[pl], I::CLS, planes[pl] + cbase + HD, lane);
        put_cls(vim[pl], I::CLS, planes[pl] + cbase + 2 * HD, lane);
        put_cls(gim[pl], I::CLS, gplanes[pl] + cob, lane);
      }
    }
  }
  if (g == 0) lss[f0 + p] = Lq;
  __syncthreads();

  const bool pv_ = f0 + p < T;                                   // this lane's column as a frame of the wave's tile
  // column fragments of the wave's own tile (B operands of orientation 1 / of orientation 2) and of the CLS slot (lane p = 0: row 0
  // as an A operand, column 0 as a B operand)
  // q0 / g0 serve both orientations and v0's rows become the staging tile, so these are held; the others are read where they are used
  bf16x8_t q0[NPL][2], g0[NPL][2], v0[NPL][2];
  frags_cols<NPL>(qim, f0, lane, q0);
  frags_cols<NPL>(gim, f0, lane, g0);
  frags_cols<NPL>(vim, f0, lane, v0);

  // ---- orientation 1: rows = keys (16 kt + 4g + j), columns = the wave's queries (f0 + p)  ->  dQ (contraction over keys)
  bf16x8_t dq0h[NP], dq0l[NP], dq1h[NP], dq1l[NP];
  {
    bf16x8_t qc[NPL][2], gc[NPL][2], kc[NPL][2], vc[NPL][2];
    frags_cls<NPL>(kim, I::CLS, lane, kc);
    frags_cls<NPL>(vim, I::CLS, lane, vc);
    if (w == 0) {
      frags_cls<NPL>(qim, I::CLS, lane, qc);
      frags_cls<NPL>(gim, I::CLS, lane, gc);
    }
    float pr[NT][4], dp[NT][4], c1[NT][4];
    float acc = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      bf16x8_t kf[NPL][2], vf[NPL][2];
      frags_cols<NPL>(kim, 16 * kt, lane, kf);
      frags_cols<NPL>(vim, 16 * kt, lane, vf);
      const f32x4_t s = mma2<PASSES, F16>(kf[0], kf[LO], q0[0], q0[LO]), d = mma2<PASSES, F16>(vf[0], vf[LO], g0[0], g0[LO]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pr[kt][j] = (pv_ && 16 * kt + 4 * g + j < T) ? __expf(s[j] * 0.125f - Lq) : 0.f;
        dp[kt][j] = d[j];
        acc += pr[kt][j] * d[j];
        c1[kt][j] = 0.f;
      }
      if (w == 0) {   // the clip's CLS query (column 0) against the frame keys
        const f32x4_t s1 = mma2<PASSES, F16>(kf[0], kf[LO], qc[0], qc[LO]), d1 = mma2<PASSES, F16>(vf[0], vf[LO], gc[0], gc[LO]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pj = (p == 0 && 16 * kt + 4 * g + j < T) ? __expf(s1[j] * 0.125f - Lc) : 0.f;
          c1[kt][j] = pj * (d1[j] - dlc);
        }
      }
    }
    const f32x4_t s10 = mma2<PASSES, F16>(kc[0], kc[LO], q0[0], q0[LO]), d10 = mma2<PASSES, F16>(vc[0], vc[LO], g0[0], g0[LO]);
    const float pc = (g == 0 && pv_) ? __expf(s10[0] * 0.125f - Lq) : 0.f;
    const float dl = allg_sum(acc + pc * d10[0]);
    if (g == 0) dls[f0 + p] = dl;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int j = 0; j < 4; ++j) pr[kt][j] *= dp[kt][j] - dl;
    pack_slots<NT, F16>(pr, pc * (d10[0] - dl), dq0h, dq0l);
    if (w == 0) {
      const f32x4_t s11 = mma2<PASSES, F16>(kc[0], kc[LO], qc[0], qc[LO]), d11 = mma2<PASSES, F16>(vc[0], vc[LO], gc[0], gc[LO]);
      const float pcc = (g == 0 && p == 0 && i == 0) ? __expf(s11[0] * 0.125f - Lc) : 0.f;
      pack_slots<NT, F16>(c1, pcc * (d11[0] - dlc), dq1h, dq1l);
    }
  }
  __syncthreads();      // dls complete; from here on nobody but wave w reads the rows f0 .. f0 + 15 of the V images: its staging tile
  char* const sth = vim[0] + f0 * ATT_ROW_BYTES;
  char* const stl = PASSES == 3 ? vim[LO] + f0 * ATT_ROW_BYTES : nullptr;
  bf16_t* const glo = PASSES == 3 ? gl : nullptr;
  const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4_t dq = mma_slots<PASSES, NT, F16>(kim[0], kim[LO], c, lane, dq0h, dq0l, z);      // rows = channels 16c + 4g + j, columns = queries
    stage4(sth, stl, p, 16 * c + 4 * g, dq, 0.125f, gfmt);
    if (w == 0) {
      const f32x4_t dqc = mma_slots<PASSES, NT, F16>(kim[0], kim[LO], c, lane, dq1h, dq1l, z);   // column 0: the CLS query's partial of this location
      if (p == 0) *(f32x4_t*)&red[16 * c + 4 * g] = dqc;
    }
  }
  flush_frames<EGV_NT_TIME_BWD>(sth, stl, gh, glo, (long)b * S, ts, (long)h * HD64, f0, T, n, i, lane);

  // ---- orientation 2: rows = queries (16 qt + 4g + j; the CLS query: row 0 of the CLS slot), columns = the wave's keys (f0 + p)  ->  dK, dV
  bf16x8_t dk0h[NP], dk0l[NP], pv0h[NP], pv0l[NP], dk1h, dk1l, pv1h, pv1l;
  {
    bf16x8_t k0[NPL][2], qc[NPL][2], gc[NPL][2], kc[NPL][2], vc[NPL][2];
    frags_cols<NPL>(kim, f0, lane, k0);
    frags_cls<NPL>(qim, I::CLS, lane, qc);
    frags_cls<NPL>(gim, I::CLS, lane, gc);
    frags_cls<NPL>(kim, I::CLS, lane, kc);
    frags_cls<NPL>(vim, I::CLS, lane, vc);
    float p0[NT][4], d0[NT][4];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
      bf16x8_t qf[NPL][2], gf[NPL][2];
      frags_cols<NPL>(qim, 16 * qt, lane, qf);
      frags_cols<NPL>(gim, 16 * qt, lane, gf);
      const f32x4_t t = mma2<PASSES, F16>(qf[0], qf[LO], k0[0], k0[LO]), e = mma2<PASSES, F16>(gf[0], gf[LO], v0[0], v0[LO]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int fr = 16 * qt + 4 * g + j;
        p0[qt][j] = (pv_ && fr < T) ? __expf(t[j] * 0.125f - lss[fr]) : 0.f;
        d0[qt][j] = p0[qt][j] * (e[j] - dls[fr]);
      }
    }
    const f32x4_t t10 = mma2<PASSES, F16>(qc[0], qc[LO], k0[0], k0[LO]), e10 = mma2<PASSES, F16>(gc[0], gc[LO], v0[0], v0[LO]);
    const float p10 = (g == 0 && pv_) ? __expf(t10[0] * 0.125f - Lc) : 0.f;      // the CLS query x the wave's keys
    pack_slots<NT, F16>(d0, p10 * (e10[0] - dlc), dk0h, dk0l);
    pack_slots<NT, F16>(p0, p10, pv0h, pv0l);
    // the CLS key (column 0) against the wave's OWN query tile (+ the CLS query, wave 0 of location 0): its dk / dv partial
    const f32x4_t t01 = mma2<PASSES, F16>(q0[0], q0[LO], kc[0], kc[LO]), e01 = mma2<PASSES, F16>(g0[0], g0[LO], vc[0], vc[LO]);
    const f32x4_t t11 = mma2<PASSES, F16>(qc[0], qc[LO], kc[0], kc[LO]), e11 = mma2<PASSES, F16>(gc[0], gc[LO], vc[0], vc[LO]);
    float p01[4], d01[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int fr = f0 + 4 * g + j;
      p01[j] = (p == 0 && fr < T) ? __expf(t01[j] * 0.125f - lss[fr]) : 0.f;
      d01[j] = p01[j] * (e01[j] - dls[fr]);
    }
    const float p11 = (w == 0 && g == 0 && p == 0 && i == 0) ? __expf(t11[0] * 0.125f - Lc) : 0.f;
    pack_b<F16>(d01, p11 * (e11[0] - dlc), dk1h, dk1l);
    pack_b<F16>(p01, p11, pv1h, pv1l);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4_t dk = mma_slots<PASSES, NT, F16>(qim[0], qim[LO], c, lane, dk0h, dk0l, z);      // columns = the wave's keys
    const bf16x8_t ah = frag_slots<NT>(qim[0], w, NT, 16 * c, lane);
    const bf16x8_t al = PASSES == 3 ? frag_slots<NT>(qim[LO], w, NT, 16 * c, lane) : ah;
    const f32x4_t dkc = att_mma<PASSES, F16>(ah, al, dk1h, dk1l, z);                              // column 0: the CLS key's partial
    stage4(sth, stl, p, 16 * c + 4 * g, dk, 0.125f, gfmt);
    if (p == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&red[64 + 16 * c + 4 * g + j], dkc[j]);
    }
  }
  flush_frames<EGV_NT_TIME_BWD>(sth, stl, gh, glo, (long)b * S, ts, (long)h * HD64 + HD, f0, T, n, i, lane);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4_t dv = mma_slots<PASSES, NT, F16>(gim[0], gim[LO], c, lane, pv0h, pv0l, z);
    const bf16x8_t ah = frag_slots<NT>(gim[0], w, NT, 16 * c, lane);
    const bf16x8_t al = PASSES == 3 ? frag_slots<NT>(gim[LO], w, NT, 16 * c, lane) : ah;
    const f32x4_t dvc = att_mma<PASSES, F16>(ah, al, pv1h, pv1l, z);
    stage4(sth, stl, p, 16 * c + 4 * g, dv, 1.0f, gfmt);
    if (p == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&red[128 + 16 * c + 4 * g + j], dvc[j]);
    }
  }
  flush_frames<EGV_NT_TIME_BWD>(sth, stl, gh, glo, (long)b * S, ts, (long)h * HD64 + 2 * HD, f0, T, n, i, lane);
  __syncthreads();
  for (int x = threadIdx.x; x < 192; x += 64 * NT) atomicAdd(dcls + ((long)b * H + h) * 192 + x, red[x]);
}

}  // namespace

// A pick (attn_dispatch.h att_pick_time: NT = ceil(T / 16) tiles per location, one workgroup of NT waves per (clip, location, head)) to
// its instance.  fp16 operands: three-product forward, one-product backward.
int egv_attn_time_long_fwd(const AttPick& p, const AttTimeFwd& a, hipStream_t s) {
  return att_instance<2, 3, 4>(p, [&](auto nt, auto passes, auto f16) -> int {
    constexpr int NT = nt, PASSES = passes;
    constexpr bool F16 = f16;
    if constexpr (!F16 || PASSES == 3)
      return att_launch(attn_time_long_fwd_kernel<PASSES, NT, F16>, p, s, a.qh, a.ql, a.B, a.T, a.n, a.H, a.oh, a.ol, a.lse, a.ws, a.out_fmt);
    else
      return EGV_ERR_ARG;
  });
}

int egv_attn_time_long_bwd(const AttPick& p, const AttTimeBwd& a, hipStream_t s) {
  return att_instance<2, 3, 4>(p, [&](auto nt, auto passes, auto f16) -> int {
    constexpr int NT = nt, PASSES = passes;
    constexpr bool F16 = f16;
    if constexpr (!F16 || PASSES == 1)
      return att_launch(attn_time_long_bwd_kernel<PASSES, NT, F16>, p, s, a.qh, a.ql, a.doh, a.dol, a.lse, a.delta, a.B, a.T, a.n, a.H, a.gh,
                        a.gl, a.dcls, a.gfmt);
    else
      return EGV_ERR_ARG;
  });
}
