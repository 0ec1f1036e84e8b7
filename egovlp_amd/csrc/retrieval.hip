// Retrieval scoring on the device: per query row the DCG (utils/nDCG.py calculate_DCG with calculate_k_counts) and the
// average precision (utils/mAP.py calculate_mAP; model/metric.py map for binary labels) of the row's ranking.
//
// One workgroup per query row.  The row becomes 64-bit keys in LDS
//     key = (~ordered(s) << 32) | column            ("rank" mode: ascending key order = descending s, ties by ascending column)
//     key = ~ordered(r as fp64)                      ("ideal" mode, S == NULL: the relevancy row sorted by itself, calculate_IDCG;
//                                                     the value is its own payload, so fp64 relevancies never pass through fp32)
// padded with ~0 to a power of two, sorted by a bitonic network in LDS (keys are unique, so the network's instability
// cannot show), and then ONE pass over the sorted positions p, every thread on a contiguous chunk:
//     r      = R[row, column(p)]                                   (gather; the row was just streamed, it sits in L2)
//     DCG   += r / log2(p + 2)              for p < K,  K = #{r > 0} counted while the row was loaded
//     A     += (local prefix of r) / (p+1),  B += 1 / (p+1)         for the positions with r == 1
// and after a workgroup scan of the chunks' sums of r (base = sum of r over all earlier chunks)
//     AP     = sum over threads (A + base * B) / #{r == 1}          (0 / 0 = NaN for a row without a positive, as the reference)
// c(p) is the running SUM of the relevancies as in calculate_mAP's cumsum (= the count of positives when R is binary).
// All sums, the discount and the division are fp64.  No atomics: results do not depend on scheduling.
// The dual-softmax rescaling of a retrieval similarity matrix (egv_dual_softmax, fp32) is at the end of the file.
#include "common.h"
#include "rank_keys.h"                                           // ordered_desc32, launch_transpose
#include "egovlp_hip.h"

namespace {

constexpr int RANK_MAX_THREADS = 1024;

__device__ __forceinline__ uint64_t ordered_desc64(double r) {
  r += 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(r);
  return ~(u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull));
}
__device__ __forceinline__ double from_ordered_desc64(uint64_t k) {
  k = ~k;
  const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
  return __longlong_as_double((long long)u);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// blockDim.x = max(64, npad / 2) capped at 1024; npad = power of two >= max(128, n).  Dynamic LDS: npad * 8 bytes.
template <typename RT>
__global__ __launch_bounds__(RANK_MAX_THREADS) void rank_scores_kernel(const float* __restrict__ S, long lds_, const RT* __restrict__ R,
                                                                     long ldr, int n, int npad, int affine_half,
                                                                     double* __restrict__ dcg_out, double* __restrict__ ap_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* keys = (uint64_t*)smem;
  __shared__ double red_d[3][16];
  __shared__ int red_i[2][16];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const long row = xcd_remap(blockIdx.x, gridDim.x);
  const RT* Rr = R + row * ldr;
  const bool ideal = (S == nullptr);
  const float* Sr = ideal ? nullptr : S + row * lds_;

  // ---- load: keys into LDS, K = #{r > 0}, n_pos = #{r == 1}
  int k_cnt = 0, pos_cnt = 0;
  for (int j = tid; j < npad; j += nt) {
    uint64_t key = ~0ull;
    if (j < n) {
      const double r = (double)Rr[j];
      k_cnt += (r > 0.0);
      pos_cnt += (r == 1.0);
      if (ideal) {
        key = ordered_desc64(r);
      } else {
        float s = Sr[j];
        if (affine_half) s = (s + 1.0f) * 0.5f;                 // (s + 1) / 2 in fp32, two roundings as numpy's float32 arithmetic
        key = ((uint64_t)ordered_desc32(s) << 32) | (uint32_t)j;
      }
    }
    keys[j] = key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    k_cnt += __shfl_xor(k_cnt, o, 64);
    pos_cnt += __shfl_xor(pos_cnt, o, 64);
  }
  if (lane == 0) { red_i[0][wave] = k_cnt; red_i[1][wave] = pos_cnt; }
  __syncthreads();
  int K = 0, n_pos = 0;
  for (int w = 0; w < nw; ++w) { K += red_i[0][w]; n_pos += red_i[1][w]; }

  // ---- bitonic sort, ascending
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += nt) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }

  // ---- one pass over this thread's contiguous chunk of positions
  const int per = npad / nt;
  double dcg = 0.0, A = 0.0, B = 0.0, L = 0.0;
  for (int q = 0; q < per; ++q) {
    const int p = tid * per + q;
    if (p >= n) break;                                           // the padding sorted behind every real entry
    const uint64_t key = keys[p];
    const double r = ideal ? from_ordered_desc64(key) : (double)Rr[(uint32_t)key];
    L += r;
    if (p < K && r != 0.0) dcg += r / log2((double)(p + 2));
    if (r == 1.0) {
      const double inv = 1.0 / (double)(p + 1);
      A += L * inv;
      B += inv;
    }
  }
  // exclusive scan of L over the threads: inside the wave by shuffles, across the waves through LDS
  double incl = L;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) red_d[0][wave] = incl;
  __syncthreads();
  double base = incl - L;
  for (int w = 0; w < wave; ++w) base += red_d[0][w];
  double ap = A + base * B;
  dcg = wave_sum_f64(dcg);
  ap = wave_sum_f64(ap);
  if (lane == 0) { red_d[1][wave] = dcg; red_d[2][wave] = ap; }
  __syncthreads();
  if (tid == 0) {
    double d = 0.0, a = 0.0;
    for (int w = 0; w < nw; ++w) { d += red_d[1][w]; a += red_d[2][w]; }
    if (dcg_out) dcg_out[row] = d;
    if (ap_out) ap_out[row] = a / (double)n_pos;
  }
}

template <typename RT>
int launch_rank(const float* S, long lds_, const RT* R, long ldr, int rows, int n, int affine_half, double* dcg, double* ap,
                hipStream_t s) {
  int npad = 128;
  while (npad < n) npad <<= 1;
  const int nt = npad / 2 < RANK_MAX_THREADS ? npad / 2 : RANK_MAX_THREADS;
  const size_t lds_bytes = (size_t)npad * 8;
  if (lds_bytes > 65536)                                         // above 64 KB of dynamic LDS the runtime wants to be told
    (void)hipFuncSetAttribute((const void*)rank_scores_kernel<RT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  EGV_LAUNCH((rank_scores_kernel<RT>), dim3(rows), dim3(nt), lds_bytes, s, S, lds_, R, ldr, n, npad, affine_half, dcg, ap);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

}  // namespace

extern "C" int64_t egv_rank_scores_work_bytes(int32_t n1, int32_t n2) {
  if (n1 < 0 || n2 < 0) return 0;
  const int64_t e = (int64_t)n1 * n2;
  return ((e * (int64_t)sizeof(float) + 7) & ~(int64_t)7) + e * (int64_t)sizeof(double);
}

extern "C" int egv_rank_scores(const float* S, int64_t lds_, int32_t transposed, const void* R, int32_t r_is_f64, int64_t ldr,
                               int32_t n1, int32_t n2, int32_t affine_half, double* dcg_out, double* ap_out, void* work,
                               void* stream) {
  const int rows = transposed ? n2 : n1, len = transposed ? n1 : n2;
  if (!R || n1 < 1 || n2 < 1 || len > EGV_RANK_MAX_ROW || ldr < n2 || (S && lds_ < n2) || (!dcg_out && !ap_out) ||
      (transposed && !work))
    return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (transposed) {
    // work = [ S^T fp32 | R^T in R's type ], both [n2, n1] dense; the R plane starts 8-byte aligned
    float* St = (float*)work;
    char* Rt = (char*)work + (((size_t)n1 * n2 * sizeof(float) + 7) & ~(size_t)7);
    int rc;
    if (S && (rc = launch_transpose<float>(S, (long)lds_, n1, n2, St, s)) != EGV_OK) return rc;
    rc = r_is_f64 ? launch_transpose<double>((const double*)R, (long)ldr, n1, n2, (double*)Rt, s)
                  : launch_transpose<float>((const float*)R, (long)ldr, n1, n2, (float*)Rt, s);
    if (rc != EGV_OK) return rc;
    S = S ? St : nullptr;
    R = Rt;
    lds_ = ldr = n1;
  }
  return r_is_f64 ? launch_rank<double>(S, (long)lds_, (const double*)R, (long)ldr, rows, len, affine_half, dcg_out, ap_out, s)
                  : launch_rank<float>(S, (long)lds_, (const float*)R, (long)ldr, rows, len, affine_half, dcg_out, ap_out, s);
}

// ---- dual-softmax re-scaling of a retrieval similarity matrix (run/test_epic.py:137-143) ------------------------------------
//   y = softmax(x / temp, dim = 1) * x        (row-wise prior: one wave per row, the row is streamed three times from L2)
//   z = softmax(y, dim = 0)                   (column-wise: a workgroup owns 64 columns; lanes walk the rows coalesced)
namespace {
__global__ __launch_bounds__(256) void dual_softmax_rows_kernel(const float* __restrict__ x, int n, int m, float inv_temp,
                                                                float* __restrict__ y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* xr = x + (long)row * m;
  float mx = -3.0e38f;
  for (int j = lane; j < m; j += 64) mx = fmaxf(mx, xr[j] * inv_temp);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < m; j += 64) sum += __expf(xr[j] * inv_temp - mx);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  float* yr = y + (long)row * m;
  for (int j = lane; j < m; j += 64) yr[j] = __expf(xr[j] * inv_temp - mx) * inv * xr[j];
}

__global__ __launch_bounds__(256) void dual_softmax_cols_kernel(const float* __restrict__ y, int n, int m, float* __restrict__ z) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
  const bool live = col < m;
  float mx = -3.0e38f;
  for (int i = part; i < n; i += 4) if (live) mx = fmaxf(mx, y[(long)i * m + col]);
  red[part][threadIdx.x & 63] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][threadIdx.x & 63], red[1][threadIdx.x & 63]), fmaxf(red[2][threadIdx.x & 63], red[3][threadIdx.x & 63]));
  __syncthreads();
  float sum = 0.f;
  for (int i = part; i < n; i += 4) if (live) sum += __expf(y[(long)i * m + col] - mx);
  red[part][threadIdx.x & 63] = sum;
  __syncthreads();
  sum = red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63] + red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63];
  const float inv = 1.0f / sum;
  for (int i = part; i < n; i += 4) if (live) z[(long)i * m + col] = __expf(y[(long)i * m + col] - mx) * inv;
}
}  // namespace

extern "C" int egv_dual_softmax(const float* x, int32_t n, int32_t m, float temp, float* work, float* out, void* stream) {
  if (!x || !work || !out || n <= 0 || m <= 0 || !(temp > 0.f)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  EGV_LAUNCH(dual_softmax_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x, n, m, 1.0f / temp, work);
  EGV_CHECK_LAUNCH();
  EGV_LAUNCH(dual_softmax_cols_kernel, dim3((m + 63) / 64), dim3(256), 0, s, work, n, m, out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
