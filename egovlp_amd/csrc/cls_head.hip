// Classification head of the Ego4D hands-and-objects fine-tunes (OSCC: object-state-change classification, PNR: point-of-no-return
// keyframe localisation) -- the narrow Linear behind the video tower, its loss, its backward and the validation scores.
//   model/model.py:76 (vid_proj = Linear(768, projection_dim)), model/loss.py:135-141 (CrossEntropy),
//   trainer/trainer_oscc.py:335-338  loss = CE(allgather(scores), allgather(state))
//   trainer/trainer_pnr.py:341-350   loss = mean(state.T * CE(allgather(scores), argmax(allgather(labels).long(), 1)))
//                                         = mean(state) * CE, target 0 for the all-zero label rows of clips without a state change
//   trainer/trainer_oscc.py:40-45    AllGather_multi.backward: every rank keeps the LOCAL rows of the global gradient
//   model/metric.py:342-397          oscc_metrics / pnr_metrics
// The projection has 2 (OSCC) or 16 / 17 (PNR) output columns and 4 rows per rank: far too narrow for the MFMA GEMMs, which ran it
// padded to 32 columns in about fifteen launches.  Here:
//   egv_cls_head_fwd       1 launch   a workgroup per row, a wave per class, 16-byte loads along K, one wave reduction per score;
//                                     the scores land in the first C columns of the row block the collective sends
//   egv_cls_head_loss_bwd  2 launches cls_loss_kernel (one workgroup): per row logsumexp, argmax, the loss and the scale s / n;
//                                     cls_grad_kernel (B + C workgroups): workgroup r < B writes dfeats[r] = g_r W, workgroup B + c
//                                     writes dW[c] = sum_r g_rc feats_r and db[c], with g = s (softmax - onehot) / n recomputed
//                                     from the stored logsumexp for the local rows only
//   egv_cls_head_loss_bwd_soft        the same two launches on soft targets (label smoothing, the partner's class and lam of a
//                                     Mixup / CutMix step in two more columns of the block): cls_loss_soft_kernel, cls_grad_soft_kernel
//   egv_cls_eval_update    1 launch   hits / keyframe errors of a gathered validation block added to four doubles on the device
//   egv_cross_entropy_fwd_bwd         the API-compatible loss on given scores and int64 labels, fp32: at the end of the file,
//   egv_cross_entropy_soft_fwd_bwd    with its soft-target form behind it
// Values are fp32 in memory; the sums (over K, over the classes, over the rows) are carried in fp64 registers -- at most a few
// thousand terms per output, so the cost is nothing and every output is the correctly rounded fp32 of an essentially exact sum.
// Deterministic: no atomics, every sum has a fixed order (a thread's terms by index, lane-xor trees, waves 0..3, rows ascending).
// wave64, launch arguments only (capture-safe), no host synchronisation.
#include "common.h"
#include "egovlp_hip.h"

namespace {

constexpr int CLS_MAX_C = 64, CLS_MAX_K = 1024, CLS_MAX_B = 256, CLS_MAX_N = 4096;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// workgroup = row r; wave w takes the classes w, w + 4, ...; lane l the features 4l .. 4l + 3 (+ 256 i)
__global__ __launch_bounds__(256) void cls_fwd_kernel(const float* __restrict__ feats, long ldf, const float* __restrict__ W,
                                                      const float* __restrict__ bias, int K, int C, float* __restrict__ scores,
                                                      long ld) {
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ x = feats + (long)r * ldf;
  for (int c = wave; c < C; c += 4) {                      // wave-uniform
    const float* __restrict__ w = W + (long)c * K;
    double acc = 0.0;
    for (int k = lane * 4; k < K; k += 256) {
      const f32x4_t a = *(const f32x4_t*)(x + k);
      const f32x4_t b = *(const f32x4_t*)(w + k);
      acc += (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2] + (double)a[3] * b[3];
    }
    acc = wave_sum_d(acc);
    if (lane == 0) scores[(long)r * ld + c] = (float)(acc + (bias ? (double)bias[c] : 0.0));
  }
}

__device__ __forceinline__ int row_argmax(const float* __restrict__ x, int C, float& m) {   // lowest index on ties
  m = x[0];
  int am = 0;
  for (int c = 1; c < C; ++c)
    if (x[c] > m) {
      m = x[c];
      am = c;
    }
  return am;
}

// one workgroup; thread t takes the rows t, t + 256, ...   work: [n] logsumexp of every row, work[n] = s / n (NaN: a bad target)
__global__ __launch_bounds__(256) void cls_loss_kernel(const float* __restrict__ packed, long ld, int n, int C, int col_t, int col_s,
                                                       float* __restrict__ loss, int* __restrict__ pred, double* __restrict__ work) {
  __shared__ double sh[2][4];
  double ls = 0.0, ss = 0.0;
  int bad = 0;
  for (int r = threadIdx.x; r < n; r += 256) {
    const float* __restrict__ x = packed + (long)r * ld;
    float m;
    const int am = row_argmax(x, C, m);
    double e = 0.0;
    for (int c = 0; c < C; ++c) e += exp((double)x[c] - (double)m);
    const double lse = (double)m + log(e);
    const float tf = x[col_t];
    const bool ok = tf >= 0.f && tf < (float)C && tf == floorf(tf);
    if (ok) ls += lse - (double)x[(int)tf];
    else bad = 1;
    ss += col_s >= 0 ? (double)x[col_s] : 1.0;
    work[r] = lse;
    if (pred) pred[r] = am;
  }
  bad = __syncthreads_or(bad);
  ls = wave_sum_d(ls);
  ss = wave_sum_d(ss);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = ls;
    sh[1][threadIdx.x >> 6] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double lsum = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    const double s = (((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3]) / (double)n;
    loss[0] = bad ? __int_as_float(0x7fc00000) : (float)(s * (lsum / (double)n));
    work[n] = bad ? nan : s / (double)n;
  }
}

// g_rc = (s / n) (softmax(x_r)_c - [c == t_r]) for a local row r (global row row0 + r), from the stored logsumexp
__device__ __forceinline__ double cls_g(const float* __restrict__ packed, long ld, int col_t, const double* __restrict__ work,
                                        double sc, int row, int c) {
  const float* __restrict__ x = packed + (long)row * ld;
  return sc * (exp((double)x[c] - work[row]) - ((float)c == x[col_t] ? 1.0 : 0.0));
}

// The soft-target form of the head (label smoothing, Mixup / CutMix): the target distribution of row r is
//   q_r = (1 - eps) (lam_r e(t_r) + (1 - lam_r) e(t2_r)) + eps / C
// with t2 = column col_t2 (-1: t2 = t) and lam = column col_lam (-1: lam = 1) of the block.
struct ClsSoft { int col_t2, col_lam; float eps; };

__device__ __forceinline__ bool cls_target_ok(float tf, int C) { return tf >= 0.f && tf < (float)C && tf == floorf(tf); }

// g_rc = (s / n) (softmax(x_r)_c - q_rc) for a local row r, from the stored logsumexp
__device__ __forceinline__ double cls_g_soft(const float* __restrict__ packed, long ld, int col_t, const ClsSoft& sf, int C,
                                             const double* __restrict__ work, double sc, int row, int c) {
  const float* __restrict__ x = packed + (long)row * ld;
  const float t = x[col_t], t2 = sf.col_t2 >= 0 ? x[sf.col_t2] : t;
  const double lam = sf.col_lam >= 0 ? (double)x[sf.col_lam] : 1.0;
  const double q = (1.0 - (double)sf.eps) * (lam * ((float)c == t ? 1.0 : 0.0) + (1.0 - lam) * ((float)c == t2 ? 1.0 : 0.0)) +
                   (double)sf.eps / (double)C;
  return sc * (exp((double)x[c] - work[row]) - q);
}

// workgroups [0, B): dfeats rows;  workgroups [B, B + C): one class each, dW row and db entry
template <bool SOFT>
__device__ __forceinline__ void cls_grad_body(const float* __restrict__ packed, long ld, int n, int C, int col_t, const ClsSoft& sf,
                                              int row0, int B, const float* __restrict__ feats, long ldf, const float* __restrict__ W,
                                              int K, const double* __restrict__ work, float* __restrict__ dW, float* __restrict__ db,
                                              float* __restrict__ dfeats, long ldd) {
  __shared__ double g[CLS_MAX_B];
  const double sc = work[n];
  const int tid = threadIdx.x;
  auto g_of = [&](int row, int c) {
    return SOFT ? cls_g_soft(packed, ld, col_t, sf, C, work, sc, row, c) : cls_g(packed, ld, col_t, work, sc, row, c);
  };
  if ((int)blockIdx.x < B) {
    if (!dfeats) return;
    const int r = blockIdx.x;
    if (tid < C) g[tid] = g_of(row0 + r, tid);
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
      double a = 0.0;
      for (int c = 0; c < C; ++c) a += g[c] * (double)W[(long)c * K + k];
      dfeats[(long)r * ldd + k] = (float)a;
    }
  } else {
    const int c = blockIdx.x - B;
    if (tid < B) g[tid] = g_of(row0 + tid, c);
    __syncthreads();
    if (dW) {
      for (int k = tid; k < K; k += 256) {
        double a = 0.0;
        for (int r = 0; r < B; ++r) a += g[r] * (double)feats[(long)r * ldf + k];
        dW[(long)c * K + k] = (float)a;
      }
    }
    if (db && tid == 0) {
      double a = 0.0;
      for (int r = 0; r < B; ++r) a += g[r];
      db[c] = (float)a;
    }
  }
}

__global__ __launch_bounds__(256) void cls_grad_kernel(const float* __restrict__ packed, long ld, int n, int C, int col_t, int row0,
                                                       int B, const float* __restrict__ feats, long ldf,
                                                       const float* __restrict__ W, int K, const double* __restrict__ work,
                                                       float* __restrict__ dW, float* __restrict__ db, float* __restrict__ dfeats,
                                                       long ldd) {
  cls_grad_body<false>(packed, ld, n, C, col_t, ClsSoft{-1, -1, 0.f}, row0, B, feats, ldf, W, K, work, dW, db, dfeats, ldd);
}

__global__ __launch_bounds__(256) void cls_grad_soft_kernel(const float* __restrict__ packed, long ld, int n, int C, int col_t,
                                                            const ClsSoft sf, int row0, int B, const float* __restrict__ feats, long ldf,
                                                            const float* __restrict__ W, int K, const double* __restrict__ work,
                                                            float* __restrict__ dW, float* __restrict__ db,
                                                            float* __restrict__ dfeats, long ldd) {
  cls_grad_body<true>(packed, ld, n, C, col_t, sf, row0, B, feats, ldf, W, K, work, dW, db, dfeats, ldd);
}

// cls_loss_kernel on soft targets: the row term is logsumexp(x_r) - sum_c q_rc x_rc
//   = logsumexp(x_r) - (1 - eps) (lam x_r[t] + (1 - lam) x_r[t2]) - (eps / C) sum_c x_rc;  a bad t OR t2 voids the loss
__global__ __launch_bounds__(256) void cls_loss_soft_kernel(const float* __restrict__ packed, long ld, int n, int C, int col_t, int col_s,
                                                            const ClsSoft sf, float* __restrict__ loss, int* __restrict__ pred,
                                                            double* __restrict__ work) {
  __shared__ double sh[2][4];
  double ls = 0.0, ss = 0.0;
  int bad = 0;
  for (int r = threadIdx.x; r < n; r += 256) {
    const float* __restrict__ x = packed + (long)r * ld;
    float m;
    const int am = row_argmax(x, C, m);
    double e = 0.0, sx = 0.0;
    for (int c = 0; c < C; ++c) {
      e += exp((double)x[c] - (double)m);
      sx += (double)x[c];
    }
    const double lse = (double)m + log(e);
    const float tf = x[col_t], t2f = sf.col_t2 >= 0 ? x[sf.col_t2] : tf;
    const double lam = sf.col_lam >= 0 ? (double)x[sf.col_lam] : 1.0;
    if (cls_target_ok(tf, C) && cls_target_ok(t2f, C))
      ls += lse - ((1.0 - (double)sf.eps) * (lam * (double)x[(int)tf] + (1.0 - lam) * (double)x[(int)t2f]) +
                   (double)sf.eps / (double)C * sx);
    else bad = 1;
    ss += col_s >= 0 ? (double)x[col_s] : 1.0;
    work[r] = lse;
    if (pred) pred[r] = am;
  }
  bad = __syncthreads_or(bad);
  ls = wave_sum_d(ls);
  ss = wave_sum_d(ss);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = ls;
    sh[1][threadIdx.x >> 6] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double lsum = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    const double s = (((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3]) / (double)n;
    loss[0] = bad ? __int_as_float(0x7fc00000) : (float)(s * (lsum / (double)n));
    work[n] = bad ? nan : s / (double)n;
  }
}

// one workgroup; 256 rows at a time are scored in parallel, then thread 0 adds them to the accumulators in ascending row order
__global__ __launch_bounds__(256) void cls_eval_kernel(const float* __restrict__ packed, long ld, int n, int C, int col_t, int col_s,
                                                       int col_fps, int col_start, int col_end, int col_pnr,
                                                       double* __restrict__ accum) {
  __shared__ double val[256];
  __shared__ int take[256];
  const int tid = threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  if (tid == 0) {
    sum = col_s < 0 ? accum[0] : accum[2];
    cnt = col_s < 0 ? accum[1] : accum[3];
  }
  for (int base = 0; base < n; base += 256) {
    const int r = base + tid;
    double v = 0.0;
    int tk = 0;
    if (r < n) {
      const float* __restrict__ x = packed + (long)r * ld;
      float m;
      const int am = row_argmax(x, C, m);
      if (col_s < 0) {                                                       // model/metric.py:346-350
        v = (float)am == x[col_t] ? 1.0 : 0.0;
        tk = 1;
      } else if (x[col_s] == 1.0f) {                                         // :378-387
        const float start = x[col_start];
        const float mapped = (x[col_end] - start) / 16.0f * (float)am;       // fp32 tensor arithmetic, the literal 16 of :381
        const double fps = (double)x[col_fps] + (double)x[col_fps + 1];
        v = fabs((double)mapped - (double)(x[col_pnr] - start)) / fps;
        tk = 1;
      }
    }
    val[tid] = v;
    take[tid] = tk;
    __syncthreads();
    if (tid == 0) {
      const int m = n - base < 256 ? n - base : 256;
      for (int i = 0; i < m; ++i)
        if (take[i]) {
          sum += val[i];
          cnt += 1.0;
        }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (col_s < 0) {
      accum[0] = sum;
      accum[1] = cnt;
    } else {
      accum[1] += (double)n;
      accum[2] = sum;
      accum[3] = cnt;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool col_ok(int col, int C, int64_t ld) { return col >= C && col < ld; }

}  // namespace

extern "C" int egv_cls_head_fwd(const float* feats, int64_t ldf, const float* W, const float* bias, int32_t B, int32_t K, int32_t C,
                                float* scores, int64_t ld, void* stream) {
  if (!feats || !W || !scores || B <= 0 || B > CLS_MAX_B || K <= 0 || K > CLS_MAX_K || K % 4 != 0 || C <= 0 || C > CLS_MAX_C)
    return EGV_ERR_ARG;
  if (ldf < K || ldf % 4 != 0 || ld < C || !aligned16(feats) || !aligned16(W)) return EGV_ERR_ARG;
  EGV_LAUNCH(cls_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, feats, (long)ldf, W, bias, K, C, scores, (long)ld);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_cls_head_loss_bwd(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                                     int32_t row0, int32_t B, const float* feats, int64_t ldf, const float* W, int32_t K,
                                     float* loss, float* dW, float* db, float* dfeats, int64_t ldd, int32_t* pred, double* work,
                                     void* stream) {
  if (!packed || !loss || !work || n <= 0 || n > CLS_MAX_N || C <= 0 || C > CLS_MAX_C) return EGV_ERR_ARG;
  if (!col_ok(col_target, C, ld) || (col_state >= 0 && (!col_ok(col_state, C, ld) || col_state == col_target))) return EGV_ERR_ARG;
  if (B <= 0 || B > CLS_MAX_B || row0 < 0 || (int64_t)row0 + B > n || K <= 0 || K > CLS_MAX_K || K % 4 != 0) return EGV_ERR_ARG;
  const bool grads = dW || db || dfeats;
  if (grads && ((dW && (!feats || ldf < K)) || (dfeats && (!W || ldd < K)))) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(cls_loss_kernel, dim3(1), dim3(256), 0, s, packed, (long)ld, n, C, col_target, col_state, loss, pred, work);
  EGV_CHECK_LAUNCH();
  if (grads) {
    EGV_LAUNCH(cls_grad_kernel, dim3(B + C), dim3(256), 0, s, packed, (long)ld, n, C, col_target, row0, B, feats, (long)ldf, W, K,
               (const double*)work, dW, db, dfeats, (long)ldd);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_cls_head_loss_bwd_soft(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                                          int32_t col_target2, int32_t col_lam, float label_smoothing, int32_t row0, int32_t B,
                                          const float* feats, int64_t ldf, const float* W, int32_t K, float* loss, float* dW, float* db,
                                          float* dfeats, int64_t ldd, int32_t* pred, double* work, void* stream) {
  if (!packed || !loss || !work || n <= 0 || n > CLS_MAX_N || C <= 0 || C > CLS_MAX_C) return EGV_ERR_ARG;
  if (!col_ok(col_target, C, ld) || (col_state >= 0 && (!col_ok(col_state, C, ld) || col_state == col_target))) return EGV_ERR_ARG;
  if (col_target2 >= 0 && (!col_ok(col_target2, C, ld) || col_target2 == col_target || col_target2 == col_state)) return EGV_ERR_ARG;
  if (col_lam >= 0 && (!col_ok(col_lam, C, ld) || col_lam == col_target || col_lam == col_state || col_lam == col_target2))
    return EGV_ERR_ARG;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return EGV_ERR_ARG;
  if (B <= 0 || B > CLS_MAX_B || row0 < 0 || (int64_t)row0 + B > n || K <= 0 || K > CLS_MAX_K || K % 4 != 0) return EGV_ERR_ARG;
  const bool grads = dW || db || dfeats;
  if (grads && ((dW && (!feats || ldf < K)) || (dfeats && (!W || ldd < K)))) return EGV_ERR_ARG;
  const ClsSoft sf{col_target2 >= 0 ? col_target2 : -1, col_lam >= 0 ? col_lam : -1, label_smoothing};
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(cls_loss_soft_kernel, dim3(1), dim3(256), 0, s, packed, (long)ld, n, C, col_target, col_state, sf, loss, pred, work);
  EGV_CHECK_LAUNCH();
  if (grads) {
    EGV_LAUNCH(cls_grad_soft_kernel, dim3(B + C), dim3(256), 0, s, packed, (long)ld, n, C, col_target, sf, row0, B, feats, (long)ldf, W,
               K, (const double*)work, dW, db, dfeats, (long)ldd);
    EGV_CHECK_LAUNCH();
  }
  return EGV_OK;
}

extern "C" int egv_cls_eval_update(const float* packed, int64_t ld, int32_t n, int32_t C, int32_t col_target, int32_t col_state,
                                   int32_t col_fps, int32_t col_start, int32_t col_end, int32_t col_pnr, double* accum,
                                   void* stream) {
  if (!packed || !accum || n <= 0 || n > CLS_MAX_N || C <= 0 || C > CLS_MAX_C) return EGV_ERR_ARG;
  if (col_state < 0) {
    if (!col_ok(col_target, C, ld)) return EGV_ERR_ARG;
  } else if (!col_ok(col_state, C, ld) || !col_ok(col_fps, C, ld) || !col_ok(col_fps + 1, C, ld) || !col_ok(col_start, C, ld) ||
             !col_ok(col_end, C, ld) || !col_ok(col_pnr, C, ld)) {
    return EGV_ERR_ARG;
  }
  EGV_LAUNCH(cls_eval_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, packed, (long)ld, n, C, col_target, col_state, col_fps,
             col_start, col_end, col_pnr, accum);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ---- softmax cross-entropy of the classification fine-tunes (OSCC / PNR: model/loss.py:135-141 = nn.CrossEntropyLoss with its
// defaults, mean over the targets != ignore_index; trainer/trainer_oscc.py:335-338 feeds it the [B, 2] / [B, 17] scores of
// FrozenInTime(video_only=True) and int64 labels).  One workgroup: a wave per row (log-sum-exp by wave shuffles), the row losses
// are summed in a fixed order through LDS, so the result is deterministic; d_logits = (softmax - onehot) / #valid.
namespace {
__global__ __launch_bounds__(256) void cross_entropy_kernel(const float* __restrict__ logits, long ld, const long long* __restrict__ target,
                                                            int rows, int cols, long long ignore_index, float* __restrict__ loss,
                                                            float* __restrict__ dlogits, long ldd) {
  __shared__ float part[4];
  __shared__ int cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // pass 1: number of valid rows (the gradient scale), then pass 2: losses and gradients
  // A label outside [0, cols) that is not ignore_index is an ERROR (torch raises a device assert): it must neither be skipped
  // silently nor inflate the mean's denominator -- the loss comes back NaN (and the gradient of every row with it).
  __shared__ int bad[4];
  int nvalid = 0, nbad = 0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const long long t = target[r];
    nvalid += (t != ignore_index);
    nbad += (t != ignore_index && (t < 0 || t >= cols));
  }
  nvalid = (int)wave_sum((float)nvalid);
  nbad = (int)wave_sum((float)nbad);
  if (lane == 0) { cnt[wave] = nvalid; bad[wave] = nbad; }
  __syncthreads();
  const int valid = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  const bool any_bad = (bad[0] + bad[1] + bad[2] + bad[3]) > 0;
  const float inv = valid > 0 ? 1.0f / (float)valid : 0.f;
  float acc = 0.f;
  for (int r = wave; r < rows; r += 4) {
    const float* x = logits + (long)r * ld;
    const long long t = target[r];
    const bool on = t != ignore_index && t >= 0 && t < cols;
    float m = -3.0e38f;
    for (int c = lane; c < cols; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < cols; c += 64) se += __expf(x[c] - m);
    se = wave_sum(se);
    const float lse = m + __logf(se);
    if (on) acc += lse - x[t];
    if (dlogits) {
      float* d = dlogits + (long)r * ldd;
      for (int c = lane; c < cols; c += 64)
        d[c] = any_bad ? __builtin_nanf("") : (on ? (__expf(x[c] - lse) - (c == (int)t ? 1.f : 0.f)) * inv : 0.f);
    }
  }
  if (lane == 0) part[wave] = acc;      // every lane of a wave holds the same acc
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (valid > 0 && !any_bad) ? (part[0] + part[1] + part[2] + part[3]) * inv : __builtin_nanf("");
}
}  // namespace

extern "C" int egv_cross_entropy_fwd_bwd(const float* logits, int64_t ld, const int64_t* target, int32_t rows, int32_t cols,
                                         int64_t ignore_index, float* loss, float* dlogits, int64_t ldd, void* stream) {
  if (!logits || !target || !loss || rows <= 0 || cols <= 0 || rows > (1 << 20) || cols > 65536 || ld < cols) return EGV_ERR_ARG;
  if (dlogits && ldd < cols) return EGV_ERR_ARG;
  EGV_LAUNCH(cross_entropy_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, (const long long*)target, rows, cols,
             (long long)ignore_index, loss, dlogits, (long)ldd);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

// ---- the same loss on soft targets (label smoothing, Mixup / CutMix; torch's label_smoothing rule = timm's mixup_target):
//   q_r = (1 - eps) (lam_r e(t_r) + (1 - lam_r) e(t2_r)) + eps / cols,  target2 NULL: t2 = t,  lam NULL: lam = 1
//   loss = mean over the rows with t != ignore_index of (logsumexp(x_r) - sum_c q_rc x_rc),  d_logits = (softmax - q) / #valid
// One workgroup, a wave per row as above; the sums over the classes and over the rows are carried in fp64 (the head's rule).
namespace {
__global__ __launch_bounds__(256) void cross_entropy_soft_kernel(const float* __restrict__ logits, long ld, const long long* __restrict__ target,
                                                                 const long long* __restrict__ target2, const float* __restrict__ lam,
                                                                 float eps, int rows, int cols, long long ignore_index,
                                                                 float* __restrict__ loss, float* __restrict__ dlogits, long ldd) {
  __shared__ double part[4];
  __shared__ int cnt[4], bad[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a valid row's t AND t2 lie in [0, cols): anything else voids the loss and every gradient (the rule of cross_entropy_kernel)
  int nvalid = 0, nbad = 0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const long long t = target[r], t2 = target2 ? target2[r] : t;
    nvalid += (t != ignore_index);
    nbad += (t != ignore_index && (t < 0 || t >= cols || t2 < 0 || t2 >= cols));
  }
  nvalid = (int)wave_sum((float)nvalid);
  nbad = (int)wave_sum((float)nbad);
  if (lane == 0) { cnt[wave] = nvalid; bad[wave] = nbad; }
  __syncthreads();
  const int valid = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  const bool any_bad = (bad[0] + bad[1] + bad[2] + bad[3]) > 0;
  const double inv = valid > 0 ? 1.0 / (double)valid : 0.0;
  const double qs = (double)eps / (double)cols, keep1 = 1.0 - (double)eps;
  double acc = 0.0;
  for (int r = wave; r < rows; r += 4) {
    const float* x = logits + (long)r * ld;
    const long long t = target[r], t2 = target2 ? target2[r] : t;
    const bool on = t != ignore_index && t >= 0 && t < cols && t2 >= 0 && t2 < cols;
    const double l = lam ? (double)lam[r] : 1.0;
    float m = -3.0e38f;
    for (int c = lane; c < cols; c += 64) m = fmaxf(m, x[c]);
    m = wave_max(m);
    double se = 0.0, sx = 0.0;
    for (int c = lane; c < cols; c += 64) {
      se += exp((double)x[c] - (double)m);
      sx += (double)x[c];
    }
    se = wave_sum_d(se);
    sx = wave_sum_d(sx);
    const double lse = (double)m + log(se);
    if (on) acc += lse - (keep1 * (l * (double)x[t] + (1.0 - l) * (double)x[t2]) + qs * sx);
    if (dlogits) {
      float* d = dlogits + (long)r * ldd;
      for (int c = lane; c < cols; c += 64) {
        const double q = keep1 * (l * (c == (int)t ? 1.0 : 0.0) + (1.0 - l) * (c == (int)t2 ? 1.0 : 0.0)) + qs;
        d[c] = any_bad ? __builtin_nanf("") : (on ? (float)((exp((double)x[c] - lse) - q) * inv) : 0.f);
      }
    }
  }
  if (lane == 0) part[wave] = acc;      // every lane of a wave holds the same acc
  __syncthreads();
  if (threadIdx.x == 0)
    loss[0] = (valid > 0 && !any_bad) ? (float)((((part[0] + part[1]) + part[2]) + part[3]) * inv) : __builtin_nanf("");
}
}  // namespace

extern "C" int egv_cross_entropy_soft_fwd_bwd(const float* logits, int64_t ld, const int64_t* target, const int64_t* target2,
                                              const float* lam, float label_smoothing, int32_t rows, int32_t cols, int64_t ignore_index,
                                              float* loss, float* dlogits, int64_t ldd, void* stream) {
  if (!logits || !target || !loss || rows <= 0 || cols <= 0 || rows > (1 << 20) || cols > 65536 || ld < cols) return EGV_ERR_ARG;
  if ((dlogits && ldd < cols) || !(label_smoothing >= 0.f && label_smoothing <= 1.f)) return EGV_ERR_ARG;
  EGV_LAUNCH(cross_entropy_soft_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, (long)ld, (const long long*)target,
             (const long long*)target2, lam, label_smoothing, rows, cols, (long long)ignore_index, loss, dlogits, (long)ldd);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
