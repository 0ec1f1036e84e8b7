// Ranking-loss head of the retrieval fine-tunes in ONE call: sim_matrix + MaxMarginRankingLoss / AdaptiveMaxMarginRankingLoss,
// forward AND analytic backward down to the embeddings.
//   model/model.py:189-197 (sim_matrix), model/loss.py:55-133 (the two ranking losses), trainer/trainer_epic.py:123-130.
//   x_ij  = <t_i / max(|t_i|, eps), v_j / max(|v_j|, eps)>
//   loss  = mean over the kept (i, j) of  relu(w_i m - x_ii + x_ij) + relu(w_i m - x_ii + x_ji)      (fix_norm drops i == j)
//   G_ab  = d loss / d x_ab = ([w_a m - x_aa + x_ab > 0] + [w_b m - x_bb + x_ab > 0]) / count          (a != b)
//   G_aa  = - sum_{j != a} ([w_a m - x_aa + x_aj > 0] + [w_a m - x_aa + x_ja > 0]) / count
//   d_tn[a] = sum_j G_aj vn_j,   d_vn[a] = sum_j G_ja tn_j,   then back through the row normalisation.
// Neither x nor G ever exists in memory (x only when the caller asks for `sim`): the workgroup that owns row a forms row a AND
// column a of x from the normalised rows, and the only foreign values its indicators need are the diagonal x_jj and the margins
// w_j m.  Three launches:
//   A  mmh_norm_kernel   one workgroup per row: norms, normalised rows, the diagonal x_ii                     -> work
//   B  mmh_rows_kernel   one workgroup per row a: a wave per j streams tn_j / vn_j ONCE (16 bytes per lane, the whole row in
//                        one wave for D <= 256), reduces x_aj and x_ja over the wave, turns them into G_aj / G_ja on the spot
//                        and accumulates both gradient rows in registers; the four waves' partial rows meet in LDS in a fixed
//                        order.  (Four rows per workgroup, to stream tn / vn from L2 a quarter as often, was measured at
//                        n = 1024: 497 us against 196 us -- the wave reductions, not L2, are what this kernel waits for.)
//   C  mmh_loss_kernel   the per-row partial losses, summed in a fixed order.
// Deterministic: no floating-point atomics, every sum has a fixed order (lane-xor trees inside a wave, waves 0..3 in LDS, rows by
// index).  fp32 throughout, wave64, launch arguments only (capture-safe), no host synchronisation.
// The same losses on a GIVEN similarity matrix (egv_maxmargin_fwd_bwd, the API-compatible path) are at the end of the file.
#include "head_common.h"
#include "egovlp_hip.h"

namespace {

__device__ __forceinline__ float dot4(const f32x4_t a, const f32x4_t b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

// A: stats = [3][n]: |t_i|, |v_i| (unclamped, for the backward's eps branch), x_ii
__global__ __launch_bounds__(256) void mmh_norm_kernel(const float* __restrict__ text, const float* __restrict__ video, int n, int D,
                                                       float eps, float* __restrict__ tn, float* __restrict__ vn,
                                                       float* __restrict__ stats) {
  __shared__ float sh[4];
  const int i = blockIdx.x;
  const int d = threadIdx.x;                  // D <= 256: one feature per thread
  const float a = d < D ? text[(long)i * D + d] : 0.f;
  const float b = d < D ? video[(long)i * D + d] : 0.f;
  const float nt = sqrtf(egv_block_sum_256(a * a, sh));
  const float nv = sqrtf(egv_block_sum_256(b * b, sh));
  const float ta = a / fmaxf(nt, eps), vb = b / fmaxf(nv, eps);
  if (d < D) {
    tn[(long)i * D + d] = ta;
    vn[(long)i * D + d] = vb;
  }
  const float xii = egv_block_sum_256(ta * vb, sh);
  if (threadIdx.x == 0) {
    stats[i] = nt;
    stats[n + i] = nv;
    stats[2 * n + i] = xii;
  }
}

// B: workgroup = row a.  Lane l of every wave owns features 4l .. 4l + 3; wave w takes j = w, w + 4, ...
__global__ __launch_bounds__(256) void mmh_rows_kernel(const float* __restrict__ tn, const float* __restrict__ vn,
                                                       const float* __restrict__ stats, const float* __restrict__ w, int n, int D,
                                                       float margin, int fix_norm, float inv_count, float eps,
                                                       float* __restrict__ sim, float* __restrict__ d_text,
                                                       float* __restrict__ d_video, float* __restrict__ rowloss) {
  __shared__ f32x4_t red[4][2][64];           // [wave][text / video gradient][lane]
  __shared__ float sred[4][2];                // [wave][loss sum, indicator count]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x;
  const int d = lane * 4;
  const bool on = d < D;
  const float* __restrict__ diag = stats + 2 * (long)n;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4_t ta = on ? *(const f32x4_t*)(tn + (long)a * D + d) : zero;
  const f32x4_t va = on ? *(const f32x4_t*)(vn + (long)a * D + d) : zero;
  const float xaa = diag[a];
  const float ma = (w ? w[a] : 1.0f) * margin;
  f32x4_t gt = zero, gv = zero;
  float ls = 0.f, ds = 0.f;
  for (int j = wave; j < n; j += 4) {
    const f32x4_t tj = on ? *(const f32x4_t*)(tn + (long)j * D + d) : zero;
    const f32x4_t vj = on ? *(const f32x4_t*)(vn + (long)j * D + d) : zero;
    const float xaj = wave_sum(dot4(ta, vj));            // every lane holds the sum
    const float xja = wave_sum(dot4(tj, va));
    if (sim && lane == 0) sim[(long)a * n + j] = xaj;
    if (j == a) continue;                                // the diagonal pair: constant (or dropped), no gradient (wave-uniform)
    const float xjj = diag[j];
    const float mj = (w ? w[j] : 1.0f) * margin;
    const float t1 = ma - xaa + xaj, t2 = ma - xaa + xja;
    const float i1 = t1 > 0.f ? 1.f : 0.f, i2 = t2 > 0.f ? 1.f : 0.f;
    ls += fmaxf(t1, 0.f) + fmaxf(t2, 0.f);
    ds += i1 + i2;
    // x_aj also sits in row j's column-direction hinge, x_ja in row j's row-direction hinge
    const float gr = (i1 + ((mj - xjj + xaj) > 0.f ? 1.f : 0.f)) * inv_count;   // G[a, j]
    const float gc = (i2 + ((mj - xjj + xja) > 0.f ? 1.f : 0.f)) * inv_count;   // G[j, a]
    gt += gr * vj;
    gv += gc * tj;
  }
  red[wave][0][lane] = gt;
  red[wave][1][lane] = gv;
  if (lane == 0) {
    sred[wave][0] = ls;
    sred[wave][1] = ds;
  }
  __syncthreads();
  if (wave != 0) return;
  // epilogue on wave 0: the four waves' partial rows, summed in the order 0, 1, 2, 3
  f32x4_t g_t = ((red[0][0][lane] + red[1][0][lane]) + red[2][0][lane]) + red[3][0][lane];
  f32x4_t g_v = ((red[0][1][lane] + red[1][1][lane]) + red[2][1][lane]) + red[3][1][lane];
  const float lsum = ((sred[0][0] + sred[1][0]) + sred[2][0]) + sred[3][0];
  const float dsum = ((sred[0][1] + sred[1][1]) + sred[2][1]) + sred[3][1];
  const float gaa = -dsum * inv_count;                   // G[a, a]
  g_t += gaa * va;
  g_v += gaa * ta;
  // through t / max(|t|, eps)
  const float pt = wave_sum(dot4(ta, g_t));
  const float pv = wave_sum(dot4(va, g_v));
  const float nt = stats[a], nv = stats[n + a];
  if (on) {
    if (d_text) *(f32x4_t*)(d_text + (long)a * D + d) = egv_norm_bwd(g_t, ta, pt, nt, eps);
    if (d_video) *(f32x4_t*)(d_video + (long)a * D + d) = egv_norm_bwd(g_v, va, pv, nv, eps);
  }
  if (lane == 0) rowloss[a] = (lsum + (fix_norm ? 0.f : 2.f * fmaxf(ma, 0.f))) * inv_count;
}

// C: loss = sum_a rowloss[a], thread t takes a = t, t + 256, ...; then the fixed-order block sum
__global__ __launch_bounds__(256) void mmh_loss_kernel(const float* __restrict__ rowloss, int n, float* __restrict__ loss) {
  __shared__ float sh[4];
  float s = 0.f;
  for (int a = threadIdx.x; a < n; a += 256) s += rowloss[a];
  s = egv_block_sum_256(s, sh);
  if (threadIdx.x == 0) loss[0] = s;
}

}  // namespace

extern "C" int64_t egv_maxmargin_head_work_floats(int32_t n, int32_t D) {
  if (n <= 0 || D <= 0) return 0;
  return 2LL * n * D + 4LL * n;   // tn, vn, |t|, |v|, diagonal, per-row losses
}

extern "C" int egv_maxmargin_head_fwd_bwd(const float* text, const float* video, const float* weight, int32_t n, int32_t D,
                                          float margin, int32_t fix_norm, float eps, float* loss, float* sim, float* d_text,
                                          float* d_video, float* work, void* stream) {
  if (!text || !video || !loss || !work || n <= 0 || n > 1024 || D <= 0 || D > 256 || D % 4 != 0) return EGV_ERR_ARG;
  if (fix_norm && n < 2) return EGV_ERR_ARG;             // no kept pair: the reference's mean is 0 / 0
  hipStream_t s = (hipStream_t)stream;
  float* tn = work;
  float* vn = tn + (long)n * D;
  float* stats = vn + (long)n * D;    // 3n
  float* rowloss = stats + 3 * n;     // n
  const double count = fix_norm ? 2.0 * n * (n - 1.0) : 2.0 * n * (double)n;
  const float inv_count = (float)(1.0 / count);
  EGV_LAUNCH(mmh_norm_kernel, dim3(n), dim3(256), 0, s, text, video, n, D, eps, tn, vn, stats);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(mmh_rows_kernel, dim3(n), dim3(256), 0, s, tn, vn, stats, weight, n, D, margin, fix_norm, inv_count, eps, sim, d_text,
             d_video, rowloss);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(mmh_loss_kernel, dim3(1), dim3(256), 0, s, rowloss, n, loss);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ---- max-margin ranking losses (model/loss.py:55-133; the EPIC-MIR / Charades fine-tuning heads on the same similarity
// matrix) ----------------------------------------------------------------------------------------------------------------
//   loss = mean over the kept (i, j) of  relu(w_i m - x_ii + x_ij) + relu(w_i m - x_ii + x_ji)
// (w_i = 1: MaxMarginRankingLoss; w_i = weight[i]: AdaptiveMaxMarginRankingLoss); fix_norm drops the diagonal pairs, so the
// mean runs over 2 n (n - 1) terms instead of 2 n^2.  The gradient is local in x:
//   d x_ab (a != b) = ( [w_a m - x_aa + x_ab > 0] + [w_b m - x_bb + x_ab > 0] ) / count
//   d x_aa          = - sum_{j != a} ( [w_a m - x_aa + x_aj > 0] + [w_a m - x_aa + x_ja > 0] ) / count
// One workgroup per row a; the loss is accumulated with one atomicAdd per row into a zeroed scalar.
namespace {
__global__ __launch_bounds__(256) void maxmargin_kernel(const float* __restrict__ x, const float* __restrict__ w, int n,
                                                        float margin, int fix_norm, float inv_count,
                                                        float* __restrict__ loss, float* __restrict__ dx) {
  const int a = blockIdx.x;
  const float xaa = x[(long)a * n + a];
  const float ma = (w ? w[a] : 1.0f) * margin;
  float lsum = 0.f, dsum = 0.f;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const float xaj = x[(long)a * n + j], xja = x[(long)j * n + a];
    const float t1 = ma - xaa + xaj, t2 = ma - xaa + xja;
    if (j != a) {
      lsum += fmaxf(t1, 0.f) + fmaxf(t2, 0.f);
      const float i1 = t1 > 0.f ? 1.f : 0.f, i2 = t2 > 0.f ? 1.f : 0.f;
      dsum += i1 + i2;
      if (dx) {
        const float mj = (w ? w[j] : 1.0f) * margin;
        const float t3 = mj - x[(long)j * n + j] + xaj;        // the column-direction term of row j that contains x_aj
        dx[(long)a * n + j] = (i1 + (t3 > 0.f ? 1.f : 0.f)) * inv_count;
      }
    } else if (!fix_norm) {
      lsum += 2.f * fmaxf(ma, 0.f);                             // x_aa cancels: constant terms, no gradient
    }
  }
  __shared__ float red[2][4];
  lsum = wave_sum(lsum);
  dsum = wave_sum(dsum);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = lsum;
    red[1][threadIdx.x >> 6] = dsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(loss, (red[0][0] + red[0][1] + red[0][2] + red[0][3]) * inv_count);
    if (dx) dx[(long)a * n + a] = -(red[1][0] + red[1][1] + red[1][2] + red[1][3]) * inv_count;
  }
}
}  // namespace

extern "C" int egv_maxmargin_fwd_bwd(const float* x, const float* weight, int32_t n, float margin, int32_t fix_norm,
                                     float* loss, float* dx, void* stream) {
  if (!x || !loss || n <= 0 || n > 4096 || (fix_norm && n < 2)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(loss, 0, sizeof(float), s) != hipSuccess) return EGV_ERR_LAUNCH;
  const double count = fix_norm ? 2.0 * n * (n - 1.0) : 2.0 * n * (double)n;
  EGV_LAUNCH(maxmargin_kernel, dim3(n), dim3(256), 0, s, x, weight, n, margin, fix_norm, (float)(1.0 / count), loss, dx);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
