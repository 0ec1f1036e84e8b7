// EgoNCE / NormSoftmaxLoss with a queue of past embeddings (MoCo, ALBEF, cross-batch memory): the normalised rows of earlier steps
// are extra CONSTANT columns of both softmaxes.  With t_i, v_j the n normalised batch rows, tq_q, vq_q the K valid queue rows
// (K = `filled`, read from the device), m_ij the mask of the long head (diagonal included) and m_iq the same sharing rule between
// batch row i and queue row q WITHOUT a diagonal (0 when there are no noun / verb vectors):
//   a_ij = exp(t_i . v_j / tau)    a_iq = exp(t_i . vq_q / tau)    b_jq = exp(v_j . tq_q / tau)
//   Z_i = sum_j a_ij + sum_q a_iq          P_i = sum_j m_ij a_ij + sum_q m_iq a_iq
//   C_j = sum_i a_ij + sum_q b_jq          Q_j = sum_i m_ij a_ij + sum_q m_jq b_jq
//   L   = -(1 / n) sum_i (log P_i - log Z_i) - (1 / n) sum_j (log Q_j - log C_j)
// On a batch x batch tile G_ij is the expression at the top of egonce_long.hip with these statistics; on a queue tile only the
// walking direction's own term exists, Gt_iq = -(1 / (n tau)) a_iq (m_iq / P_i - 1 / Z_i) (Gv_jq: the same with b, Q_j, C_j), so
//   d t_i = sum_j G_ij v_j + sum_q Gt_iq vq_q,    d v_j = sum_i G_ij t_i + sum_q Gv_jq tq_q,    queue rows get no gradient,
//   dL/ds = sum G_ij x_ij + sum Gt_iq x_iq + sum Gv_jq x_jq       (s = log(1 / tau), the learnable scale).
// K = 0 is the long head's loss.  The problem is RECTANGULAR: 64 batch rows against the batch tiles of the other modality followed
// by the queue tiles of that modality, 2 n (n + K) pairs where the long head on the concatenated rows would spend (n + K)^2 and
// add queue x queue terms that are no part of this loss.  The tile pieces (prep, X^T product, finish) and the k order are those of
// egonce_tile.h / egonce_long.hip; all arithmetic fp32, every reduction in a fixed order (no float atomics): two calls on the same
// inputs and the same queue state give the same bits.
//
//   prep    egonce_tile.h, on the batch rows.
//   stats   workgroup = (64 batch rows of A, a range of column tiles); tile t < ntiles is batch tile t of B (valid: j < n), tile
//           ntiles + u is queue tile u (valid: slot < filled).  The launch is sized by the capacity Q; `filled` is read from the
//           device and a workgroup ends its range at the last tile that holds a valid slot (a wave-uniform bound, no host read).
//           Slots >= filled are staged as zeros, so what an unused slot holds never reaches a product.
//   loss    one workgroup: merges the range partials of both directions in a fixed order, sums the n terms in double, turns any
//           bad noun / verb flag into a NaN loss.
//   grad    the walk again, both terms on batch tiles and the own term on queue tiles, dA_I += G . B_J on the same MFMA.  The
//           (tn, ..) walk sums G X over all its tiles, the (vn, ..) walk over its queue tiles only (the batch x batch sum would be
//           the same number twice); one partial per workgroup, added by egv_scale_grad_kernel in double.
//   finish  egonce_tile.h.
//   push    egv_egonce_queue_push, after the head on the same stream: one workgroup per batch row copies the prep outputs (tn, vn,
//           the packed words) into slot (head + i) mod Q; a launch of its own then advances head and filled -- after every copying
//           workgroup has read head.  A loss that is not finite pushes nothing and leaves the state alone: one NaN row in the queue
//           would make every loss NaN until it is overwritten, Q / n steps later.
#define EGV_SCALE_GRAD_KERNEL
#include "egonce_tile.h"
#include "egovlp_hip.h"

namespace {

constexpr int EGQ_STAT_WGS = 512;     // as the long head: column ranges sized for about two workgroups per CU
constexpr float EGQ_NEG = -3e38f;
constexpr float EGQ_POS = 3e38f;

// egl_split for a rectangle: `rtiles` row tiles, `ctiles` column tiles -> tiles per range and ranges (no empty range)
inline void egq_split(int rtiles, int ctiles, int target, int& tps, int& ns) {
  int want = (target + rtiles - 1) / rtiles;
  if (want > ctiles) want = ctiles;
  tps = (ctiles + want - 1) / want;
  ns = (ctiles + tps - 1) / tps;
}

struct EgqLayout : EglPrepLayout {
  int qtiles, ctiles, tps_s, ns_s, tps_g, ns_g;
  long spart, stat, gpart, lpart;   // offsets in floats, behind the prep outputs
};

inline EgqLayout egq_layout(int n, int D, int dn, int dv, int Q) {
  EgqLayout L{egl_prep_layout(n, D, dn, dv)};
  L.qtiles = Q / EGL_TILE;
  L.ctiles = L.ntiles + L.qtiles;
  egq_split(L.ntiles, L.ctiles, EGQ_STAT_WGS, L.tps_s, L.ns_s);
  egq_split(L.ntiles, L.ctiles, EGL_GRAD_WGS, L.tps_g, L.ns_g);
  const long np = L.np;
  long o = L.total;
  L.spart = o;  o += 2L * L.ns_s * 3 * np;
  L.stat = o;   o += 6 * np;
  L.gpart = o;  o += (long)L.ns_g * np * L.Dp;
  L.lpart = o;  o += 2L * L.ns_g * L.ntiles;           // sum G X: one partial per workgroup of each of the two grad walks
  L.total = o;
  return L;
}

inline bool egq_args_ok(int n, int D, int dn, int dv, int Q) {
  return egl_args_ok(n, D, dn, dv) && Q >= EGL_TILE && Q <= 65536 && Q % EGL_TILE == 0 && n <= Q;
}

// ------------------------------------------------------------------------------------------------ tile pieces
// The column tile `t` of a walk: which rows it reads and how many of its 64 columns count.
struct EgqTile {
  const float* B;          // the rows behind the tile: the other modality's batch rows, or that modality's queue
  const uint32_t* wb;      // the packed words of those rows
  int r0, valid, queue;    // first row, valid columns (0 .. 64), 1 on a queue tile (no diagonal, own term only)
};

__device__ __forceinline__ EgqTile egq_tile(int t, int ntiles, int n, int filled, const float* Bb, const float* Bq,
                                            const uint32_t* words, const uint32_t* q_words) {
  EgqTile T;
  T.queue = t >= ntiles;
  T.r0 = (T.queue ? t - ntiles : t) * EGL_TILE;
  T.B = T.queue ? Bq : Bb;
  T.wb = T.queue ? q_words : words;
  T.valid = min(EGL_TILE, (T.queue ? filled : n) - T.r0);
  return T;
}

// `filled` as the kernels use it: wave-uniform and inside [0, Q] whatever the word holds
__device__ __forceinline__ int egq_filled(const int32_t* __restrict__ q_state, int Q) {
  return __builtin_amdgcn_readfirstlane(min(max(q_state[1], 0), Q));
}

// egl_stage_tile with the rows from `valid` on written as zeros (an unused queue slot may hold anything)
template <int DP>
__device__ __forceinline__ void egq_stage_tile(float* bt, const float* __restrict__ B, int r0, int valid) {
  constexpr int LD = DP + 4, C4 = DP / 4;
  for (int idx = threadIdx.x; idx < EGL_TILE * C4; idx += 256) {
    const int r = idx / C4, c4 = idx % C4;
    f32x4_t v = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if (r < valid) v = *(const f32x4_t*)(B + (long)(r0 + r) * DP + 4 * c4);
    *(f32x4_t*)(bt + r * LD + 4 * c4) = v;
  }
}

// egl_mask_tile between the words of the A rows (wa, rows i0 ..) and those of the tile's rows (wb, rows r0 ..), which may belong
// to the queue; `diag`: add i == j (batch tiles only).  Same thread map: thread (row tid & 63, wave q) covers columns 16 q .. + 15.
__device__ __forceinline__ void egq_mask_tile(const uint32_t* __restrict__ wa, const uint32_t* __restrict__ wb, int W, int wn,
                                              int mode, int i0, int r0, int diag, uint32_t* mb) {
  const int il = threadIdx.x & 63;
  const int jq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = i0 + il, jb = r0 + jq * 16;
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

// ------------------------------------------------------------------------------------------------ statistics
template <int DP>
__global__ __launch_bounds__(256, 2) void egq_stats_kernel(const float* __restrict__ A, const float* __restrict__ Bb,
                                                           const float* __restrict__ Bq, const uint32_t* __restrict__ words,
                                                           const uint32_t* __restrict__ q_words,
                                                           const int32_t* __restrict__ q_state, int Q, int n, int np, int W,
                                                           int wn, int mode, float inv_tau,
                                                           const float* __restrict__ logit_scale, int tps,
                                                           float* __restrict__ part /* [ranges][3][np] */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LD = DP + 4;
  float* bt = (float*)smem;
  uint32_t* mb = (uint32_t*)(bt + EGL_TILE * LD);
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  const int filled = egq_filled(q_state, Q);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * EGL_TILE;
  const int ntiles = np / EGL_TILE;
  const int live_tiles = ntiles + (filled + EGL_TILE - 1) / EGL_TILE;      // tiles past it hold no valid slot
  const int t0 = blockIdx.y * tps, t1 = min(live_tiles, t0 + tps);
  const int gi = i0 + wave * 16 + li;

  f32x4_t a[DP / 16];
#pragma unroll
  for (int c = 0; c < DP / 16; ++c) a[c] = *(const f32x4_t*)(A + (long)gi * DP + 16 * c + 4 * g);

  float m = EGQ_NEG, Z = 0.f, P = 0.f;                // this lane's share of row gi: the columns 16 jf + 4 g + r of every tile
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const EgqTile T = egq_tile(t, ntiles, n, filled, Bb, Bq, words, q_words);
    __syncthreads();                                  // every wave is done with the previous tile
    egq_stage_tile<DP>(bt, T.B, T.r0, T.valid);
    egq_mask_tile(words, T.wb, W, wn, mode, i0, T.r0, !T.queue, mb);
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    float cm = EGQ_NEG;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (jf * 16 + 4 * g + r < T.valid) cm = fmaxf(cm, x[jf][r]);
    const float mn = fmaxf(m, cm);
    const float alpha = __expf((m - mn) * inv_tau);   // first tile: exp(-inf) = 0 and Z, P are 0 anyway
    float zs = 0.f, ps = 0.f;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (jf * 16 + 4 * g + r < T.valid) ? __expf((x[jf][r] - mn) * inv_tau) : 0.f;
        zs += e;
        ps += ((mbits[jf] >> (4 * g + r)) & 1u) ? e : 0.f;
      }
    Z = Z * alpha + zs;
    P = P * alpha + ps;
    m = mn;
  }
  // the four lane groups of a row
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float mo = __shfl_xor(m, off, 64), Zo = __shfl_xor(Z, off, 64), Po = __shfl_xor(P, off, 64);
    const float M = fmaxf(m, mo);
    const float s1 = __expf((m - M) * inv_tau), s2 = __expf((mo - M) * inv_tau);
    Z = Z * s1 + Zo * s2;
    P = P * s1 + Po * s2;
    m = M;
  }
  if (g == 0 && gi < n) {                             // a range with no live tile writes (EGQ_NEG, 0, 0): weight 0 in the merge
    float* p = part + (long)blockIdx.y * 3 * np;
    p[gi] = m;
    p[np + gi] = Z;
    p[2 * np + gi] = P;
  }
}

// ------------------------------------------------------------------------------------------------ loss
__global__ __launch_bounds__(1024) void egq_loss_kernel(const float* __restrict__ spart /* [2][ranges][3][np] */, int ns, int n,
                                                        int np, float inv_tau, const float* __restrict__ logit_scale,
                                                        const float* __restrict__ flags,
                                                        float* __restrict__ stat /* [2][3][np] */, float* __restrict__ loss) {
  __shared__ double red[1024];
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  double s = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    float term = 0.f;
    for (int dir = 0; dir < 2; ++dir) {
      const float* p = spart + (long)dir * ns * 3 * np;
      float M = EGQ_NEG;
      for (int r = 0; r < ns; ++r) M = fmaxf(M, p[(long)r * 3 * np + i]);
      float Z = 0.f, P = 0.f;
      for (int r = 0; r < ns; ++r) {
        const float w = __expf((p[(long)r * 3 * np + i] - M) * inv_tau);
        Z += p[((long)r * 3 + 1) * np + i] * w;
        P += p[((long)r * 3 + 2) * np + i] * w;
      }
      float* o = stat + (long)dir * 3 * np;
      o[i] = M;
      o[np + i] = Z;
      o[2 * np + i] = P;
      term += __logf(P) - __logf(Z);
    }
    s += (double)term;
    bad |= flags[i] != 0.f;
  }
  red[threadIdx.x] = s;
  bad = __syncthreads_or(bad);
  for (int h = 512; h >= 1; h >>= 1) {                // pairwise, fixed order
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = bad ? __builtin_nanf("") : (float)(-red[0] / (double)n);
}

// ------------------------------------------------------------------------------------------------ gradient
template <int DP>
__global__ __launch_bounds__(256, 2) void egq_grad_kernel(const float* __restrict__ A, const float* __restrict__ Bb,
                                                          const float* __restrict__ Bq, const uint32_t* __restrict__ words,
                                                          const uint32_t* __restrict__ q_words,
                                                          const int32_t* __restrict__ q_state, int Q,
                                                          const float* __restrict__ own /* [3][np]: statistics of A's rows */,
                                                          const float* __restrict__ oth /* [3][np]: of Bb's rows */, int n, int np,
                                                          int W, int wn, int mode, float inv_tau, float sc,
                                                          const float* __restrict__ logit_scale, int tps, int gx_batch,
                                                          float* __restrict__ gpart /* [ranges][np][DP] */,
                                                          float* __restrict__ lpart /* [ranges][tiles] or NULL */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LD = DP + 4;
  float* bt = (float*)smem;
  uint32_t* mb = (uint32_t*)(bt + EGL_TILE * LD);
  float* cs = (float*)(mb + EGL_TILE * 4);            // [3][64]: max, 1 / Z, 1 / P of the tile's rows (queue tile: no such term)
  float* sh = cs + 3 * EGL_TILE;                      // [4]
  if (logit_scale) {                                  // uniform
    inv_tau = expf(logit_scale[0]);
    sc = -inv_tau / (float)n;
  }
  const int filled = egq_filled(q_state, Q);
  float gx = 0.f;                                     // this lane's share of sum G X
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * EGL_TILE;
  const int ntiles = np / EGL_TILE;
  const int live_tiles = ntiles + (filled + EGL_TILE - 1) / EGL_TILE;
  const int t0 = blockIdx.y * tps, t1 = min(live_tiles, t0 + tps);
  const int gi = i0 + wave * 16 + li;

  f32x4_t a[DP / 16];
#pragma unroll
  for (int c = 0; c < DP / 16; ++c) a[c] = *(const f32x4_t*)(A + (long)gi * DP + 16 * c + 4 * g);
  const bool live = gi < n;
  const float mo = live ? own[gi] : 0.f;
  const float izo = live ? 1.0f / own[np + gi] : 0.f;
  const float ipo = live ? 1.0f / own[2 * np + gi] : 0.f;

  f32x4_t acc[DP / 64][4];
#pragma unroll
  for (int c = 0; c < DP / 64; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[c][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const EgqTile T = egq_tile(t, ntiles, n, filled, Bb, Bq, words, q_words);
    __syncthreads();
    egq_stage_tile<DP>(bt, T.B, T.r0, T.valid);
    egq_mask_tile(words, T.wb, W, wn, mode, i0, T.r0, !T.queue, mb);
    if (threadIdx.x < EGL_TILE) {
      // a queue row has no statistics of its own: maximum +3e38 makes its exponential exactly 0, and 0 * (0 - 0) adds nothing
      const int gj = T.r0 + threadIdx.x;
      const bool ok = !T.queue && gj < n;
      cs[threadIdx.x] = ok ? oth[gj] : EGQ_POS;
      cs[64 + threadIdx.x] = ok ? 1.0f / oth[np + gj] : 0.f;
      cs[128 + threadIdx.x] = ok ? 1.0f / oth[2 * np + gj] : 0.f;
    }
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    float tgx = 0.f;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf) {
      const f32x4_t cm4 = *(const f32x4_t*)(cs + jf * 16 + 4 * g);
      const f32x4_t iz4 = *(const f32x4_t*)(cs + 64 + jf * 16 + 4 * g);
      const f32x4_t ip4 = *(const f32x4_t*)(cs + 128 + jf * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xv = x[jf][r];
        const float eo = __expf((xv - mo) * inv_tau);         // under the maximum of A's row
        const float ec = __expf((xv - cm4[r]) * inv_tau);     // under the maximum of B's row; 0 on a queue tile
        const float mm = ((mbits[jf] >> (4 * g + r)) & 1u) ? 1.f : 0.f;
        const float gv = sc * (eo * (mm * ipo - izo) + ec * (mm * ip4[r] - iz4[r]));
        const float gm = (live && jf * 16 + 4 * g + r < T.valid) ? gv : 0.f;
        tgx += gm * xv;
        x[jf][r] = gm;
      }
    }
    if (gx_batch || T.queue) gx += tgx;               // uniform
    // dA[i][d] += sum_j G[i][j] B[j][d]: x[jf][r] is the A operand of k-step (jf, r) as it stands (k = j = 16 jf + 4 g + r)
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < DP / 64; ++c) {
          const f32x4_t bv = *(const f32x4_t*)(bt + (jf * 16 + 4 * g + r) * LD + 64 * c + 4 * li);
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) acc[c][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[jf][r], bv[tt], acc[c][tt], 0, 0, 0);
        }
  }
  // acc[c][tt][rr]: row i0 + 16 wave + 4 g + rr, column 64 c + 4 li + tt; a range with no live tile stores zeros
  float* out = gpart + ((long)blockIdx.y * np + i0 + wave * 16 + 4 * g) * DP + 4 * li;
#pragma unroll
  for (int c = 0; c < DP / 64; ++c)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      *(f32x4_t*)(out + (long)rr * DP + 64 * c) = (f32x4_t){acc[c][0][rr], acc[c][1][rr], acc[c][2][rr], acc[c][3][rr]};
  if (lpart) {                                        // uniform over the workgroup
    gx = egv_block_sum_256(gx, sh);
    if (threadIdx.x == 0) lpart[(long)blockIdx.y * ntiles + blockIdx.x] = gx;
  }
}

template <int DP>
int egq_launch_stats(const EgqLayout& L, const float* A, const float* Bb, const float* Bq, const uint32_t* words,
                     const uint32_t* q_words, const int32_t* q_state, int Q, int n, int mode, float inv_tau,
                     const float* logit_scale, float* part, hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4;
  auto k = egq_stats_kernel<DP>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_s), dim3(256), lds, s, A, Bb, Bq, words, q_words, q_state, Q, n, L.np, L.W, L.wn, mode,
             inv_tau, logit_scale, L.tps_s, part);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

template <int DP>
int egq_launch_grad(const EgqLayout& L, const float* A, const float* Bb, const float* Bq, const uint32_t* words,
                    const uint32_t* q_words, const int32_t* q_state, int Q, const float* own, const float* oth, int n, int mode,
                    float inv_tau, const float* logit_scale, int gx_batch, float* gpart, float* lpart, hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4 + 3 * EGL_TILE * 4 + 16;
  auto k = egq_grad_kernel<DP>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_g), dim3(256), lds, s, A, Bb, Bq, words, q_words, q_state, Q, own, oth, n, L.np, L.W, L.wn,
             mode, inv_tau, -inv_tau / (float)n, logit_scale, L.tps_g, gx_batch, gpart, lpart);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ------------------------------------------------------------------------------------------------ push
// one workgroup per batch row: the row's prep outputs -> slot (head + i) mod Q.  Nothing moves after a loss that is not finite.
__global__ __launch_bounds__(256) void egq_push_kernel(const float* __restrict__ tn, const float* __restrict__ vn,
                                                       const uint32_t* __restrict__ words, const float* __restrict__ loss, int Dp,
                                                       int W, int Q, const int32_t* __restrict__ q_state,
                                                       float* __restrict__ q_text, float* __restrict__ q_video,
                                                       uint32_t* __restrict__ q_words) {
  if (!isfinite(loss[0])) return;
  const int i = blockIdx.x;
  const int head = min(max(q_state[0], 0), Q - 1);
  const long slot = (head + i) % Q;
  for (int d = threadIdx.x; d < Dp / 4; d += 256) {
    ((f32x4_t*)(q_text + slot * Dp))[d] = ((const f32x4_t*)(tn + (long)i * Dp))[d];
    ((f32x4_t*)(q_video + slot * Dp))[d] = ((const f32x4_t*)(vn + (long)i * Dp))[d];
  }
  for (int w = threadIdx.x; w < W; w += 256) q_words[slot * W + w] = words[(long)i * W + w];
}

// a launch of its own, so that every workgroup of egq_push_kernel has read `head` before it moves
__global__ __launch_bounds__(64) void egq_advance_kernel(const float* __restrict__ loss, int n, int Q, int32_t* __restrict__ q_state) {
  if (threadIdx.x != 0 || !isfinite(loss[0])) return;
  const int head = min(max(q_state[0], 0), Q - 1), filled = min(max(q_state[1], 0), Q);
  q_state[0] = (head + n) % Q;
  q_state[1] = min(Q, filled + n);
}

}  // namespace

extern "C" int64_t egv_egonce_queue_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv, int32_t Q) {
  if (!egq_args_ok(n, D, dn, dv, Q)) return 0;
  return egq_layout(n, D, dn, dv, Q).total;
}

extern "C" int egv_egonce_queue_layout(int32_t D, int32_t dn, int32_t dv, int32_t* Dp, int32_t* W) {
  if (!Dp || !W || !egl_args_ok(1, D, dn, dv)) return EGV_ERR_ARG;
  const EglPrepLayout L = egl_prep_layout(1, D, dn, dv);
  *Dp = L.Dp;
  *W = L.W;
  return EGV_OK;
}

extern "C" int egv_egonce_queue_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                        int32_t D, int32_t dn, int32_t dv, const float* q_text, const float* q_video,
                                        const uint32_t* q_words, int32_t Q, const int32_t* q_state, float temperature,
                                        const float* logit_scale, float eps, int32_t use_noun, int32_t use_verb, float* loss,
                                        float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream) {
  if (!text || !video || !loss || !work || !q_text || !q_video || !q_state) return EGV_ERR_ARG;
  if ((noun != nullptr) != (verb != nullptr)) return EGV_ERR_ARG;
  if (!noun) dn = dv = 0;
  if (!egq_args_ok(n, D, dn, dv, Q)) return EGV_ERR_ARG;
  if (!logit_scale && !(temperature > 0.f)) return EGV_ERR_ARG;
  // both gradients or neither: the scale's gradient takes its queue parts from both walks
  if ((d_text != nullptr) != (d_video != nullptr)) return EGV_ERR_ARG;
  if (d_logit_scale && !(logit_scale && d_text)) return EGV_ERR_ARG;
  if (logit_scale && d_text && !d_logit_scale) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const EgqLayout L = egq_layout(n, D, dn, dv, Q);
  if (L.W > 0 && !q_words) return EGV_ERR_ARG;
  const float inv_tau = logit_scale ? 0.f : 1.0f / temperature;
  float* tn = work + L.tn;
  float* vn = work + L.vn;
  const uint32_t* words = (const uint32_t*)(work + L.words);
  const float* norms = work + L.norms;
  const float* flags = work + L.flags;
  float* spart = work + L.spart;
  float* stat = work + L.stat;
  float* gpart = work + L.gpart;
  float* lpart = d_logit_scale ? work + L.lpart : nullptr;
  const int mode = egl_mask_mode(noun, use_noun, use_verb);
  const long np = L.np;

  int rc = egl_launch_prep(L, text, video, noun, verb, n, D, dn, dv, eps, work, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_DP(egq_launch_stats, L, tn, vn, q_video, words, q_words, q_state, Q, n, mode, inv_tau, logit_scale, spart, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_DP(egq_launch_stats, L, vn, tn, q_text, words, q_words, q_state, Q, n, mode, inv_tau, logit_scale,
                 spart + (long)L.ns_s * 3 * np, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(egq_loss_kernel, dim3(1), dim3(1024), 0, s, spart, L.ns_s, n, L.np, inv_tau, logit_scale, flags, stat, loss);
  EGV_CHECK_LAUNCH();
  if (!d_text) return EGV_OK;
  rc = EGL_BY_DP(egq_launch_grad, L, tn, vn, q_video, words, q_words, q_state, Q, stat, stat + 3 * np, n, mode, inv_tau,
                 logit_scale, 1, gpart, lpart, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, tn, norms, L.np, D, L.Dp, eps, d_text);
  EGV_CHECK_LAUNCH();
  rc = EGL_BY_DP(egq_launch_grad, L, vn, tn, q_text, words, q_words, q_state, Q, stat + 3 * np, stat, n, mode, inv_tau,
                 logit_scale, 0, gpart, lpart ? lpart + (long)L.ns_g * L.ntiles : nullptr, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, vn, norms + np, L.np, D, L.Dp, eps, d_video);
  EGV_CHECK_LAUNCH();
  if (lpart) {
    EGV_LAUNCH(egv_scale_grad_kernel, dim3(1), dim3(256), 0, s, lpart, 2 * L.ns_g * L.ntiles, d_logit_scale);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_egonce_queue_push(const float* work, const float* loss, int32_t n, int32_t D, int32_t dn, int32_t dv,
                                     float* q_text, float* q_video, uint32_t* q_words, int32_t Q, int32_t* q_state,
                                     void* stream) {
  if (!work || !loss || !q_text || !q_video || !q_state) return EGV_ERR_ARG;
  if (!egq_args_ok(n, D, dn, dv, Q)) return EGV_ERR_ARG;
  const EglPrepLayout L = egl_prep_layout(n, D, dn, dv);
  if (L.W > 0 && !q_words) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(egq_push_kernel, dim3(n), dim3(256), 0, s, work + L.tn, work + L.vn, (const uint32_t*)(work + L.words), loss, L.Dp,
             L.W, Q, (const int32_t*)q_state, q_text, q_video, q_words);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(egq_advance_kernel, dim3(1), dim3(64), 0, s, loss, n, Q, q_state);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
