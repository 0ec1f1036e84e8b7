// The softmax contrastive heads that walk the similarity in 64 x 64 tiles without storing it: the LONG head, for global batches
// past the 1 024 rows of egonce.hip, and the QUEUE head, the same loss with the rows of earlier steps as extra columns.  One walk
// (egonce_tile.h: its pieces and the k order) serves both; `QUEUE` is a compile-time parameter of the two walk kernels, so the long
// head's instances are kernels of their own that carry nothing of the queue.  The similarity tile X = A_I . B_J^T is formed on
// the fp32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit an fp32 fma chain, so the numerics are those of the fp32 short head),
// the EgoNCE mask comes from bit-packed noun / verb rows, and the row statistics are kept online while the column tiles stream
// through LDS.  All arithmetic fp32; every reduction runs in a fixed order (no float atomics), so a call is deterministic: two
// calls on the same inputs (and the same queue state) give the same bits.
//
// The long head: the loss and the gradients of egonce.hip (the formulas at its top), with nothing of size n x n in memory.
//
// The queue head (MoCo, ALBEF, cross-batch memory): the normalised rows of earlier steps are extra CONSTANT columns of both
// softmaxes.  With t_i, v_j the n normalised batch rows, tq_q, vq_q the K valid queue rows (K = `filled`, read from the device), m_ij
// the mask of the long head (diagonal included) and m_iq the same sharing rule between batch row i and queue row q WITHOUT a
// diagonal (0 when there are no noun / verb vectors):
//   a_ij = exp(t_i . v_j / tau)    a_iq = exp(t_i . vq_q / tau)    b_jq = exp(v_j . tq_q / tau)
//   Z_i = sum_j a_ij + sum_q a_iq          P_i = sum_j m_ij a_ij + sum_q m_iq a_iq
//   C_j = sum_i a_ij + sum_q b_jq          Q_j = sum_i m_ij a_ij + sum_q m_jq b_jq
//   L   = -(1 / n) sum_i (log P_i - log Z_i) - (1 / n) sum_j (log Q_j - log C_j)
// On a batch x batch tile G_ij is the long head's expression (`grad` below) with these statistics; on a queue tile only the walking
// direction's own term exists, Gt_iq = -(1 / (n tau)) a_iq (m_iq / P_i - 1 / Z_i) (Gv_jq: the same with b, Q_j, C_j), so
//   d t_i = sum_j G_ij v_j + sum_q Gt_iq vq_q,    d v_j = sum_i G_ij t_i + sum_q Gv_jq tq_q,    queue rows get no gradient,
//   dL/ds = sum G_ij x_ij + sum Gt_iq x_iq + sum Gv_jq x_jq       (s = log(1 / tau), the learnable scale).
// K = 0 is the long head's loss.  The problem is RECTANGULAR: 64 batch rows against the batch tiles of the other modality followed
// by the queue tiles of that modality, 2 n (n + K) pairs where the long head on the concatenated rows would spend (n + K)^2 and
// add queue x queue terms that are no part of this loss.  The long head is this problem with no queue tiles.
//
//   prep    egonce_tile.h, on the batch rows.  One workgroup per row: |t|, |v|, the normalised rows tn / vn zero-padded from D to
//           Dp (64 or 256), and the noun / verb rows packed into bit words (bit = entry > 0; each part padded to a multiple of 4
//           words).  Rows n .. np - 1 (np = n rounded up to 64) are written as zeros, so no tile load needs a bound.  A negative or
//           NaN noun / verb entry sets the row's flag; the loss kernel turns any flag into a NaN loss (no host sync).
//   stats   workgroup = (64 batch rows of A, a range of column tiles); tile t < ntiles is batch tile t of B (valid: j < n) and, in
//           the queue head, tile ntiles + u is queue tile u (valid: slot < filled).  Per tile: X^T fragments, the 64 x 64 mask tile
//           from AND / OR of the packed words, and per lane the running maximum, Z = sum a and P = sum m a, rescaled online.
//           Launched twice: (tn, vn) gives the row statistics of the loss; (vn, tn) gives the column statistics, because the mask
//           is symmetric:
//             m_ij = (rows i, j share a noun AND share a verb) OR i == j        (use_noun only: share a noun; else verb)
//           which under the data contract -- noun / verb are non-negative multi-hots -- is sim_v * sim_n + I > 0.
//           The queue head's launch is sized by the capacity Q; `filled` is read from the device and a workgroup ends its range at
//           the last tile that holds a valid slot (a wave-uniform bound, no host read).  Slots >= filled are staged as zeros, so
//           what an unused slot holds never reaches a product.
//   loss    one workgroup: merges the column-range partials of both directions in a fixed order, writes the final statistics,
//           sums the n loss terms in double and turns any bad noun / verb flag into a NaN loss.
//   grad    the stats walk again; G_IJ = -1/(n tau) [m a_r / P_i - a_r / Z_i + m a_c / Q_j - a_c / C_j] (queue tile: the first two
//           terms) is formed in the registers of the X^T fragment and dA_I += G_IJ . B_J runs on the same MFMA (egonce_tile.h).
//           Launched twice with the roles swapped; raw partials per column range go to the workspace.
//   finish  egonce_tile.h: one workgroup per row sums the partials in a fixed order and applies the backward of the normalisation.
//   scale   learnable temperature only (1 / tau = exp(s) read from the device by every kernel above): dL/ds = sum G X.  In the
//           grad walk the X^T fragment and G_IJ sit in the same registers, so each lane accumulates G X (masked exactly like G),
//           the workgroup reduces and stores ONE partial per (row tile, column range); egv_scale_grad_kernel adds the partials in
//           a fixed order in double.  The loss kernel runs BEFORE the walk, so this sum is a launch of its own, of the same shape.
//           Long head: the (tn, vn) walk alone (the swapped walk would give the same number), summed right after it.  Queue head:
//           the (tn, ..) walk over all its tiles and the (vn, ..) walk over its queue tiles only, summed at the end.
//   push    egv_egonce_queue_push, after the queue head on the same stream: one workgroup per batch row copies the prep outputs
//           (tn, vn, the packed words) into slot (head + i) mod Q; a launch of its own then advances head and filled -- after every
//           copying workgroup has read head.  A loss that is not finite pushes nothing and leaves the state alone: one NaN row in
//           the queue would make every loss NaN until it is overwritten, Q / n steps later.
#define EGV_SCALE_GRAD_KERNEL
#include "egonce_tile.h"
#include "egovlp_hip.h"

namespace {

constexpr int EGL_STAT_WGS = 512;     // column ranges are chosen so that a launch has about this many workgroups (2 per CU)
constexpr float EGL_NEG = -3e38f;
constexpr float EGL_POS = 3e38f;

struct EglLayout : EglPrepLayout {
  int tps_s, ns_s, tps_g, ns_g;
  long spart, stat, gpart, lpart;   // offsets in floats, behind the prep outputs
  int nl;                           // partials of sum G X
};

// Q: the queue's capacity; 0 is the long head
inline EglLayout egl_layout(int n, int D, int dn, int dv, int Q) {
  EglLayout L{egl_prep_layout(n, D, dn, dv)};
  const int ctiles = L.ntiles + Q / EGL_TILE;
  egl_split(L.ntiles, ctiles, EGL_STAT_WGS, L.tps_s, L.ns_s);
  egl_split(L.ntiles, ctiles, EGL_GRAD_WGS, L.tps_g, L.ns_g);
  L.nl = (Q ? 2 : 1) * L.ns_g * L.ntiles;              // one per workgroup of the grad walks that sum G X: one walk, with a queue both
  const long np = L.np;
  long o = L.total;
  L.spart = o;  o += 2L * L.ns_s * 3 * np;
  L.stat = o;   o += 6 * np;
  L.gpart = o;  o += (long)L.ns_g * np * L.Dp;
  L.lpart = o;  o += L.nl;
  L.total = o;
  return L;
}

inline bool egq_args_ok(int n, int D, int dn, int dv, int Q) {
  return egl_args_ok(n, D, dn, dv) && Q >= EGL_TILE && Q <= 65536 && Q % EGL_TILE == 0 && n <= Q;
}

// ------------------------------------------------------------------------------------------------ columns
// The column tile `t` of a walk: where its rows start and how many of its 64 columns count.  Which rows those are -- the other
// modality's batch rows B, or on a queue tile that modality's queue Bq, with their packed words -- is chosen where the tile is
// staged.  Without a queue only r0 is read.
struct EglTile {
  int r0, valid, queue;    // first row, valid columns (0 .. 64), 1 on a queue tile (no diagonal, own term only)
};

template <bool QUEUE>
__device__ __forceinline__ EglTile egl_tile(int t, int ntiles, int n, int filled) {
  EglTile T{t * EGL_TILE, EGL_TILE, 0};
  if constexpr (QUEUE) {
    T.queue = t >= ntiles;
    T.r0 = (T.queue ? t - ntiles : t) * EGL_TILE;
    T.valid = min(EGL_TILE, (T.queue ? filled : n) - T.r0);
  }
  return T;
}

// whether column c of the tile counts.  The long head keeps its own form of the bound (against n): written the queue's way it
// costs the instance registers.
template <bool QUEUE>
__device__ __forceinline__ bool egl_col_ok(const EglTile& T, int c, int n) {
  if constexpr (QUEUE) return c < T.valid;
  else return T.r0 + c < n;
}

// `filled` as the kernels use it: wave-uniform and inside [0, Q] whatever the word holds
__device__ __forceinline__ int egq_filled(const int32_t* __restrict__ q_state, int Q) {
  return __builtin_amdgcn_readfirstlane(min(max(q_state[1], 0), Q));
}

// The queue's arguments come last in both walk kernels; the instances without a queue are passed nulls and never read them.
// ------------------------------------------------------------------------------------------------ statistics
template <int DP, bool QUEUE>
__global__ __launch_bounds__(256, 2) void egl_stats_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                           const uint32_t* __restrict__ words, int n, int np, int W, int wn,
                                                           int mode, float inv_tau,
                                                           const float* __restrict__ logit_scale, int tps,
                                                           float* __restrict__ part /* [ranges][3][np] */,
                                                           const float* __restrict__ Bq, const uint32_t* __restrict__ q_words,
                                                           const int32_t* __restrict__ q_state, int Q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  EGL_WALK_LDS(DP);
  inv_tau = egv_inv_tau(inv_tau, logit_scale);
  int filled = 0;
  if constexpr (QUEUE) filled = egq_filled(q_state, Q);
  // with a queue the range ends at the last tile that holds a valid slot
  EGL_WALK_BEGIN(DP, A, np, QUEUE ? ntiles + (filled + EGL_TILE - 1) / EGL_TILE : ntiles, tps);

  float m = EGL_NEG, Z = 0.f, P = 0.f;                // this lane's share of row gi: the columns 16 jf + 4 g + r of every tile
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const EglTile T = egl_tile<QUEUE>(t, ntiles, n, filled);
    __syncthreads();                                  // every wave is done with the previous tile
    egl_stage_tile<DP, QUEUE>(bt, QUEUE && T.queue ? Bq : B, T.r0, T.valid);
    egl_mask_tile(words, QUEUE && T.queue ? q_words : words, W, wn, mode, i0, T.r0, !T.queue, mb);
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    float cm = EGL_NEG;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (egl_col_ok<QUEUE>(T, jf * 16 + 4 * g + r, n)) cm = fmaxf(cm, x[jf][r]);
    const float mn = fmaxf(m, cm);
    const float alpha = __expf((m - mn) * inv_tau);   // first tile: exp(-inf) = 0 and Z, P are 0 anyway
    float zs = 0.f, ps = 0.f;
#pragma unroll
    for (int jf = 0; jf < 4; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = egl_col_ok<QUEUE>(T, jf * 16 + 4 * g + r, n) ? __expf((x[jf][r] - mn) * inv_tau) : 0.f;
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
  if (g == 0 && gi < n) {                             // a range with no live tile writes (EGL_NEG, 0, 0): weight 0 in the merge
    float* p = part + (long)blockIdx.y * 3 * np;
    p[gi] = m;
    p[np + gi] = Z;
    p[2 * np + gi] = P;
  }
}

// ------------------------------------------------------------------------------------------------ loss
__global__ __launch_bounds__(1024) void egl_loss_kernel(const float* __restrict__ spart /* [2][ranges][3][np] */, int ns, int n,
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
      float M = EGL_NEG;
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
template <int DP, bool QUEUE>
__global__ __launch_bounds__(256, 2) void egl_grad_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const uint32_t* __restrict__ words,
                                                          const float* __restrict__ own /* [3][np]: statistics of A's rows */,
                                                          const float* __restrict__ oth /* [3][np]: of B's rows */, int n,
                                                          int np, int W, int wn, int mode, float inv_tau, float sc,
                                                          const float* __restrict__ logit_scale, int tps,
                                                          float* __restrict__ gpart /* [ranges][np][DP] */,
                                                          float* __restrict__ lpart /* [ranges][tiles] or NULL */,
                                                          const float* __restrict__ Bq, const uint32_t* __restrict__ q_words,
                                                          const int32_t* __restrict__ q_state, int Q,
                                                          int gx_batch /* the batch tiles count in sum G X (queue tiles always do) */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  EGL_WALK_LDS(DP);
  float* cs = (float*)(mb + EGL_TILE * 4);            // [3][64]: max, 1 / Z, 1 / P of the tile's rows (queue tile: no such term)
  float* sh;                                          // [4], for the block sum: static in the long head, behind cs with a queue
  if constexpr (QUEUE) {
    sh = cs + 3 * EGL_TILE;
  } else {
    __shared__ float sh_static[4];
    sh = sh_static;
  }
  if (logit_scale) {                                  // uniform
    inv_tau = expf(logit_scale[0]);
    sc = -inv_tau / (float)n;
  }
  int filled = 0;
  if constexpr (QUEUE) filled = egq_filled(q_state, Q);
  float gx = 0.f;                                     // this lane's share of sum G X
  EGL_WALK_BEGIN(DP, A, np, QUEUE ? ntiles + (filled + EGL_TILE - 1) / EGL_TILE : ntiles, tps);
  const bool live = gi < n;
  const float mo = live ? own[gi] : 0.f;
  const float izo = live ? 1.0f / own[np + gi] : 0.f;
  const float ipo = live ? 1.0f / own[2 * np + gi] : 0.f;

  f32x4_t acc[DP / 64][4];
  egl_acc_zero<DP>(acc);

#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    const EglTile T = egl_tile<QUEUE>(t, ntiles, n, filled);
    __syncthreads();
    egl_stage_tile<DP, QUEUE>(bt, QUEUE && T.queue ? Bq : B, T.r0, T.valid);
    egl_mask_tile(words, QUEUE && T.queue ? q_words : words, W, wn, mode, i0, T.r0, !T.queue, mb);
    if (threadIdx.x < EGL_TILE) {
      // a queue row has no statistics of its own: maximum +3e38 makes its exponential exactly 0, and 0 * (0 - 0) adds nothing
      const int gj = T.r0 + threadIdx.x;
      const bool ok = !T.queue && gj < n;
      cs[threadIdx.x] = ok ? oth[gj] : (QUEUE ? EGL_POS : 0.f);
      cs[64 + threadIdx.x] = ok ? 1.0f / oth[np + gj] : 0.f;
      cs[128 + threadIdx.x] = ok ? 1.0f / oth[2 * np + gj] : 0.f;
    }
    __syncthreads();
    f32x4_t x[4];
    egl_xt<DP>(bt, a, li, g, x);
    const u32x4_t mbits = *(const u32x4_t*)(mb + (wave * 16 + li) * 4);
    // sum G X: the long head adds every term to the running sum, the queue head the tile's 16 terms first (it may drop the tile)
    float tgx = 0.f;
    float& sgx = QUEUE ? tgx : gx;
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
        const float gm = (live && egl_col_ok<QUEUE>(T, jf * 16 + 4 * g + r, n)) ? gv : 0.f;
        sgx += gm * xv;
        x[jf][r] = gm;
      }
    }
    if constexpr (QUEUE)
      if (gx_batch || T.queue) gx += tgx;             // uniform
    EGL_SECOND_PRODUCT(DP);
  }
  EGL_STORE_GPART(DP, gpart, np);
  if (lpart) {                                        // uniform over the workgroup
    gx = egv_block_sum_256(gx, sh);
    if (threadIdx.x == 0) lpart[(long)blockIdx.y * ntiles + blockIdx.x] = gx;
  }
}

// what the launchers take of a queue; all null / 0 without one
struct EglQueue {
  const float *text, *video;
  const uint32_t* words;
  const int32_t* state;
  int Q;
};

template <int DP, bool QUEUE>
int egl_launch_stats(const EglLayout& L, const float* A, const float* B, const float* Bq, const uint32_t* words, const EglQueue& q,
                     int n, int mode, float inv_tau, const float* logit_scale, float* part, hipStream_t s) {
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4;
  auto k = egl_stats_kernel<DP, QUEUE>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_s), dim3(256), lds, s, A, B, words, n, L.np, L.W, L.wn, mode, inv_tau, logit_scale, L.tps_s,
             part, Bq, q.words, q.state, q.Q);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

template <int DP, bool QUEUE>
int egl_launch_grad(const EglLayout& L, const float* A, const float* B, const float* Bq, const uint32_t* words, const EglQueue& q,
                    const float* own, const float* oth, int n, int mode, float inv_tau, const float* logit_scale, int gx_batch,
                    float* gpart, float* lpart, hipStream_t s) {
  // the tile, the mask tile, cs; the queue instance keeps the 4 floats of its block sum there as well
  constexpr int lds = EGL_TILE * (DP + 4) * 4 + EGL_TILE * 4 * 4 + 3 * EGL_TILE * 4 + (QUEUE ? 16 : 0);
  auto k = egl_grad_kernel<DP, QUEUE>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  EGV_LAUNCH(k, dim3(L.ntiles, L.ns_g), dim3(256), lds, s, A, B, words, own, oth, n, L.np, L.W, L.wn, mode, inv_tau,
             -inv_tau / (float)n, logit_scale, L.tps_g, gpart, lpart, Bq, q.words, q.state, q.Q, gx_batch);
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

// ------------------------------------------------------------------------------------------------ host sequence
// the kernel of a launcher template fn<DP, QUEUE>, by the layout L and the QUEUE in scope
#define EGL_BY_Q(fn, ...) (L.Dp == 64 ? fn<64, QUEUE>(__VA_ARGS__) : fn<256, QUEUE>(__VA_ARGS__))

// prep, stats x 2, loss, then per wanted gradient grad + finish, and the sum of the scale partials.  The arguments are checked by
// the entry points.  logit_scale != NULL: 1 / tau = exp(*logit_scale) on the device (inv_tau unused); d_logit_scale needs d_text.
template <bool QUEUE>
int egl_head(const float* text, const float* video, const float* noun, const float* verb, int n, int D, int dn, int dv,
             const EglQueue& q, float inv_tau, const float* logit_scale, float eps, int use_noun, int use_verb, float* loss,
             float* d_text, float* d_video, float* d_logit_scale, float* work, hipStream_t s) {
  const EglLayout L = egl_layout(n, D, dn, dv, q.Q);
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
  rc = EGL_BY_Q(egl_launch_stats, L, tn, vn, q.video, words, q, n, mode, inv_tau, logit_scale, spart, s);
  if (rc != EGV_OK) return rc;
  rc = EGL_BY_Q(egl_launch_stats, L, vn, tn, q.text, words, q, n, mode, inv_tau, logit_scale, spart + (long)L.ns_s * 3 * np, s);
  if (rc != EGV_OK) return rc;
  EGV_LAUNCH(egl_loss_kernel, dim3(1), dim3(1024), 0, s, spart, L.ns_s, n, L.np, inv_tau, logit_scale, flags, stat, loss);
  EGV_CHECK_LAUNCH();
  if (d_text) {
    rc = EGL_BY_Q(egl_launch_grad, L, tn, vn, q.video, words, q, stat, stat + 3 * np, n, mode, inv_tau, logit_scale, 1, gpart, lpart,
                  s);
    if (rc != EGV_OK) return rc;
    if (!QUEUE && lpart) {                              // the long head's sum is complete after this walk
      EGV_LAUNCH(egv_scale_grad_kernel, dim3(1), dim3(256), 0, s, lpart, L.nl, d_logit_scale);
      EGV_CHECK_LAUNCH();
    }
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, tn, norms, L.np, D, L.Dp, eps, d_text);
    EGV_CHECK_LAUNCH();
  }
  if (d_video) {
    rc = EGL_BY_Q(egl_launch_grad, L, vn, tn, q.text, words, q, stat + 3 * np, stat, n, mode, inv_tau, logit_scale, 0, gpart,
                  QUEUE && lpart ? lpart + L.nl / 2 : nullptr, s);
    if (rc != EGV_OK) return rc;
    EGV_LAUNCH(egl_finish_kernel, dim3(n), dim3(256), 0, s, gpart, L.ns_g, vn, norms + np, L.np, D, L.Dp, eps, d_video);
    EGV_CHECK_LAUNCH();
  }
  if (QUEUE && lpart) {                                 // the queue head's sum takes its queue parts from both walks
    EGV_LAUNCH(egv_scale_grad_kernel, dim3(1), dim3(256), 0, s, lpart, L.nl, d_logit_scale);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

// what the three heads ask of the batch; -> false: EGV_ERR_ARG.  Without noun / verb vectors dn = dv = 0.
inline bool egl_batch_ok(const float* text, const float* video, const float* noun, const float* verb, const float* loss,
                         const float* work, int32_t& dn, int32_t& dv) {
  if (!text || !video || !loss || !work) return false;
  if ((noun != nullptr) != (verb != nullptr)) return false;
  if (!noun) dn = dv = 0;
  return true;
}

}  // namespace

extern "C" int64_t egv_egonce_long_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv) {
  if (!egl_args_ok(n, D, dn, dv)) return 0;
  return egl_layout(n, D, dn, dv, 0).total;
}

extern "C" int64_t egv_egonce_queue_work_floats(int32_t n, int32_t D, int32_t dn, int32_t dv, int32_t Q) {
  if (!egq_args_ok(n, D, dn, dv, Q)) return 0;
  return egl_layout(n, D, dn, dv, Q).total;
}

extern "C" int egv_egonce_queue_layout(int32_t D, int32_t dn, int32_t dv, int32_t* Dp, int32_t* W) {
  if (!Dp || !W || !egl_args_ok(1, D, dn, dv)) return EGV_ERR_ARG;
  const EglPrepLayout L = egl_prep_layout(1, D, dn, dv);
  *Dp = L.Dp;
  *W = L.W;
  return EGV_OK;
}

// the long head allows either gradient alone
extern "C" int egv_egonce_long_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                       int32_t D, int32_t dn, int32_t dv, float temperature, float eps, int32_t use_noun,
                                       int32_t use_verb, float* loss, float* d_text, float* d_video, float* work,
                                       void* stream) {
  if (!(temperature > 0.f)) return EGV_ERR_ARG;
  if (!egl_batch_ok(text, video, noun, verb, loss, work, dn, dv) || !egl_args_ok(n, D, dn, dv)) return EGV_ERR_ARG;
  return egl_head<false>(text, video, noun, verb, n, D, dn, dv, EglQueue{}, 1.0f / temperature, nullptr, eps, use_noun, use_verb,
                         loss, d_text, d_video, nullptr, work, (hipStream_t)stream);
}

extern "C" int egv_egonce_long_fwd_bwd_ls(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                          int32_t D, int32_t dn, int32_t dv, const float* logit_scale, float eps,
                                          int32_t use_noun, int32_t use_verb, float* loss, float* d_text, float* d_video,
                                          float* d_logit_scale, float* work, void* stream) {
  if (!logit_scale) return EGV_ERR_ARG;
  // the scale's gradient comes out of the (tn, vn) walk: it needs d_text
  if ((d_text || d_video) && !(d_text && d_logit_scale)) return EGV_ERR_ARG;
  if (!egl_batch_ok(text, video, noun, verb, loss, work, dn, dv) || !egl_args_ok(n, D, dn, dv)) return EGV_ERR_ARG;
  return egl_head<false>(text, video, noun, verb, n, D, dn, dv, EglQueue{}, 0.f, logit_scale, eps, use_noun, use_verb, loss, d_text,
                         d_video, d_text ? d_logit_scale : nullptr, work, (hipStream_t)stream);
}

extern "C" int egv_egonce_queue_fwd_bwd(const float* text, const float* video, const float* noun, const float* verb, int32_t n,
                                        int32_t D, int32_t dn, int32_t dv, const float* q_text, const float* q_video,
                                        const uint32_t* q_words, int32_t Q, const int32_t* q_state, float temperature,
                                        const float* logit_scale, float eps, int32_t use_noun, int32_t use_verb, float* loss,
                                        float* d_text, float* d_video, float* d_logit_scale, float* work, void* stream) {
  if (!q_text || !q_video || !q_state) return EGV_ERR_ARG;
  if (!egl_batch_ok(text, video, noun, verb, loss, work, dn, dv) || !egq_args_ok(n, D, dn, dv, Q)) return EGV_ERR_ARG;
  if (!logit_scale && !(temperature > 0.f)) return EGV_ERR_ARG;
  // both gradients or neither: the scale's gradient takes its queue parts from both walks
  if ((d_text != nullptr) != (d_video != nullptr)) return EGV_ERR_ARG;
  if (d_logit_scale && !(logit_scale && d_text)) return EGV_ERR_ARG;
  if (logit_scale && d_text && !d_logit_scale) return EGV_ERR_ARG;
  if (egl_prep_layout(n, D, dn, dv).W > 0 && !q_words) return EGV_ERR_ARG;
  return egl_head<true>(text, video, noun, verb, n, D, dn, dv, EglQueue{q_text, q_video, q_words, q_state, Q},
                        logit_scale ? 0.f : 1.0f / temperature, logit_scale, eps, use_noun, use_verb, loss, d_text, d_video,
                        d_logit_scale, work, (hipStream_t)stream);
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
