// Recall@K on the device: the rank of the ground truth as a count, the top-k list of a row, row normalisation.
//
// egv_gt_ranks -- model/metric.py t2v_metrics (:20-124) and v2t_metrics (:127-216).  The reference sorts the row and looks the
// ground-truth distance up in the sorted row; the position it finds is a count,
//     optimistic (t2v, :66, :71-73):   rank = #{j : s_j > g}
//     averaging  (v2t, :157, :187):    rank = #{j : s_j > g} + (#{j : s_j == g} - 1) / 2
// over the valid columns j of the row, with g the LARGEST similarity among the valid columns of the row's ground-truth segment
// (v2t keeps the minimum of the averaged ranks of a video's captions, :188-189, which is the rank of its best caption; an
// invalid caption is pushed to MISSING_VAL and skipped, :167, :177-179).  One workgroup of 256 threads per row streams it once:
// up to three scalar columns to the first 16-byte boundary, then 16-byte loads (four in flight per thread in the main loop,
// RC_TILE columns per trip), then a scalar tail.  The counters are integers, so no result depends on an order.
//
// egv_topk_rows -- the k <= 64 best (value, column) pairs of a row, descending value, ties by ascending column (the documented
// rule of egv_rank_scores, same 64-bit keys).  One workgroup per row keeps a candidate buffer of TK_CAP keys in LDS: a column
// whose key beats the current k-th best is appended (LDS integer atomic on the fill count; the order of the appends cannot
// show, the keys are unique and the buffer is sorted before it is read); when a tile of TK_TILE columns could overflow the
// buffer it is sorted by a bitonic network, cut to its k best, and the k-th becomes the new bar.  The first bar comes from a
// sample, the row's first TK_SAMPLE columns.  On rows in random order about k * ln(n / TK_SAMPLE) columns pass a bar in all;
// a row in ascending order sorts once per tile (slow, still correct).
//
// egv_row_normalize -- x / max(|x|, eps), the rule of sim_matrix (model/model.py:189-197), the twin of egonce.hip's
// rownorm_kernel with leading dimensions.
#include "common.h"
#include "rank_keys.h"
#include "egovlp_hip.h"

namespace {

constexpr int RC_THREADS = 256;                                  // workgroup: four waves
constexpr int RC_VEC = 4;                                        // floats per 16-byte load
constexpr int RC_TRIP = RC_THREADS * RC_VEC;                     // 1 024 columns: one 16-byte load per thread
constexpr int RC_UNROLL = 4;
constexpr int RC_TILE = RC_TRIP * RC_UNROLL;                     // 4 096 columns: one trip of the rank kernel's main loop
constexpr int TK_UNROLL = 2;
constexpr int TK_TILE = RC_TRIP * TK_UNROLL;                     // 2 048 columns between two looks at the candidate count
constexpr int TK_SAMPLE = RC_THREADS;                           // columns behind the head that set the first bar (keeps the 16-byte alignment)
constexpr int TK_CAP = 4096;                                     // candidate keys in LDS (32 KB) >= k + 3 + TK_TILE
static_assert(EGV_TOPK_MAX + TK_TILE <= TK_CAP && 3 + TK_SAMPLE <= TK_CAP, "a tile must fit behind the kept candidates");

// number of leading floats before the first 16-byte boundary of a 4-byte-aligned row (0..3), at most n
__device__ __forceinline__ int head_len(const float* p, long n) {
  const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  return (long)h < n ? h : (int)n;
}

// validity bytes of four consecutive columns as one word (byte q = column q); all ones without a vector
template <bool HAS_CV>
__device__ __forceinline__ uint32_t load_cv4(const uint8_t* __restrict__ cv, long j, bool aligned4) {
  if constexpr (!HAS_CV) return 0x01010101u;
  if (aligned4) return *(const uint32_t*)(cv + j);
  return (uint32_t)cv[j] | ((uint32_t)cv[j + 1] << 8) | ((uint32_t)cv[j + 2] << 16) | ((uint32_t)cv[j + 3] << 24);
}

__device__ __forceinline__ unsigned block_sum_u32(unsigned v, unsigned* sh) {   // 256 threads
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// ------------------------------------------------------------------------------------------------ ranks
struct RankCount {
  float g;
  unsigned gt, eq;
  __device__ __forceinline__ void one(float s, bool valid) {
    gt += (unsigned)(valid && s > g);
    eq += (unsigned)(valid && s == g);
  }
  __device__ __forceinline__ void four(f32x4_t v, uint32_t w) {
    one(v.x, (w & 0x000000ffu) != 0);
    one(v.y, (w & 0x0000ff00u) != 0);
    one(v.z, (w & 0x00ff0000u) != 0);
    one(v.w, (w & 0xff000000u) != 0);
  }
};

// S: rows of n columns, leading dimension ld.  Row r (global row row0 + r) has the ground-truth segment
//   seg_wide == 0: the single column (row0 + r) / qpv          seg_wide != 0: the qpv columns from (row0 + r) * qpv
// (the host checked that every segment lies inside [0, n)).
template <bool HAS_CV>
__global__ __launch_bounds__(RC_THREADS) void gt_rank_kernel(const float* __restrict__ S, long ld, long n, long row0, int qpv,
                                                             int seg_wide, const uint8_t* __restrict__ cv, int tie_avg,
                                                             double* __restrict__ out) {
  __shared__ float sh_f[4];
  __shared__ unsigned sh_u[3][4];
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const float* Sr = S + row * ld;

  // ---- the bar: the best valid similarity of the ground-truth segment
  const long grow = row0 + row;
  const long seg0 = seg_wide ? grow * qpv : grow / qpv;
  const int seg_n = seg_wide ? qpv : 1;
  float g = -INFINITY;
  unsigned have = 0;
  for (int q = tid; q < seg_n; q += RC_THREADS) {
    const long c = seg0 + q;
    if (!HAS_CV || cv[c]) {
      g = fmaxf(g, Sr[c]);
      have = 1;
    }
  }
  g = wave_max(g);
  if ((tid & 63) == 0) sh_f[tid >> 6] = g;
  have = block_sum_u32(have, sh_u[2]);                          // its two barriers also publish sh_f
  g = fmaxf(fmaxf(sh_f[0], sh_f[1]), fmaxf(sh_f[2], sh_f[3]));

  // ---- one pass over the row
  RankCount c{g, 0u, 0u};
  const int head = head_len(Sr, n);
  if (tid < head) c.one(Sr[tid], !HAS_CV || cv[tid]);
  const float* B = Sr + head;                                    // 16-byte aligned from here
  const uint8_t* cb = HAS_CV ? cv + head : nullptr;
  const bool cva = HAS_CV && (((uintptr_t)cb & 3u) == 0);
  const long nb = n - head, nvec = nb >> 2;
  const f32x4_t* B4 = (const f32x4_t*)B;
  long v = tid;
  for (; v + (RC_UNROLL - 1) * RC_THREADS < nvec; v += RC_UNROLL * RC_THREADS) {
    f32x4_t a[RC_UNROLL];
    uint32_t w[RC_UNROLL];
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) a[u] = __builtin_nontemporal_load(B4 + v + u * RC_THREADS);
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) w[u] = load_cv4<HAS_CV>(cb, (v + u * RC_THREADS) << 2, cva);
#pragma unroll
    for (int u = 0; u < RC_UNROLL; ++u) c.four(a[u], w[u]);
  }
  for (; v < nvec; v += RC_THREADS) c.four(__builtin_nontemporal_load(B4 + v), load_cv4<HAS_CV>(cb, v << 2, cva));
  const long t0 = nvec << 2;
  if (tid < (int)(nb - t0)) c.one(B[t0 + tid], !HAS_CV || cb[t0 + tid]);

  const unsigned gt = block_sum_u32(c.gt, sh_u[0]);
  const unsigned eq = block_sum_u32(c.eq, sh_u[1]);
  if (tid == 0) {
    double r = INFINITY;                                         // no valid column in the segment (model/metric.py:175)
    if (have) r = (double)gt + (tie_avg ? ((double)eq - 1.0) * 0.5 : 0.0);
    out[row] = r;
  }
}

// ------------------------------------------------------------------------------------------------ top-k
// sorts keys[0 .. npad) ascending, npad a power of two; ends with a barrier
__device__ __forceinline__ void bitonic_sort_lds(uint64_t* keys, int npad, int tid, int nt) {
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
}

template <bool HAS_CV>
__global__ __launch_bounds__(RC_THREADS) void topk_kernel(const float* __restrict__ S, long ld, long n,
                                                          const uint8_t* __restrict__ cv, int k, float* __restrict__ vals,
                                                          long long* __restrict__ idx) {
  __shared__ uint64_t buf[TK_CAP];
  __shared__ int cnt;
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const float* Sr = S + row * ld;
  uint64_t bar = ~0ull;                                          // a candidate's key is below the bar; no real key is ~0 (column < 2^31)
  if (tid == 0) cnt = 0;
  __syncthreads();

  auto push = [&](float s, bool valid, long col) {
    const uint64_t key = ((uint64_t)ordered_desc32(s) << 32) | (uint32_t)col;
    if (valid && key < bar) buf[atomicAdd(&cnt, 1)] = key;
  };
  // sort the candidates, keep the k best, lower the bar to the k-th; every thread calls it (barriers inside)
  auto cut = [&]() {
    const int c = cnt;                                           // the same for all: read between two barriers without a writer
    int npad = 64;
    while (npad < c) npad <<= 1;
    __syncthreads();
    for (int t = c + tid; t < npad; t += RC_THREADS) buf[t] = ~0ull;
    __syncthreads();
    bitonic_sort_lds(buf, npad, tid, RC_THREADS);
    if (c >= k) bar = buf[k - 1];
    if (tid == 0) cnt = c < k ? c : k;
    __syncthreads();
  };

  // the head (to the first 16-byte boundary) and a sample of TK_SAMPLE columns set a first bar: without it the whole first
  // tile would be appended and sorted
  const int head = head_len(Sr, n);
  const long pre = n >= (long)head + TK_SAMPLE ? (long)head + TK_SAMPLE : n;
  for (long c = tid; c < pre; c += RC_THREADS) push(Sr[c], !HAS_CV || cv[c], c);
  __syncthreads();
  cut();
  const float* B = Sr + pre;                                     // 16-byte aligned (or nothing is left)
  const uint8_t* cb = HAS_CV ? cv + pre : nullptr;
  const bool cva = HAS_CV && (((uintptr_t)cb & 3u) == 0);
  const long nb = n - pre;
  for (long base = 0; base < nb; base += TK_TILE) {
    f32x4_t a[TK_UNROLL];
    uint32_t w[TK_UNROLL];
    long j[TK_UNROLL];
#pragma unroll
    for (int u = 0; u < TK_UNROLL; ++u) {
      j[u] = base + ((long)u * RC_THREADS + tid) * RC_VEC;
      if (j[u] + RC_VEC <= nb) {
        a[u] = __builtin_nontemporal_load((const f32x4_t*)(B + j[u]));
        w[u] = load_cv4<HAS_CV>(cb, j[u], cva);
      }
    }
#pragma unroll
    for (int u = 0; u < TK_UNROLL; ++u) {
      if (j[u] + RC_VEC <= nb) {
        push(a[u].x, (w[u] & 0x000000ffu) != 0, pre + j[u]);
        push(a[u].y, (w[u] & 0x0000ff00u) != 0, pre + j[u] + 1);
        push(a[u].z, (w[u] & 0x00ff0000u) != 0, pre + j[u] + 2);
        push(a[u].w, (w[u] & 0xff000000u) != 0, pre + j[u] + 3);
      } else {
        for (long q = j[u]; q < nb; ++q) push(B[q], !HAS_CV || cb[q], pre + q);      // at most three columns, one thread
      }
    }
    __syncthreads();
    if (cnt > TK_CAP - TK_TILE) cut();                           // uniform: nobody appends between this barrier and the next
    __syncthreads();
  }
  cut();
  if (tid < k) {
    const bool have = tid < cnt;
    const uint32_t col = (uint32_t)buf[tid];
    vals[row * k + tid] = have ? Sr[col] : -INFINITY;            // the entry itself: a -0.0 stays a -0.0
    idx[row * k + tid] = have ? (long long)col : -1ll;
  }
}

// ------------------------------------------------------------------------------------------------ row normalisation
__global__ __launch_bounds__(RC_THREADS) void row_normalize_kernel(const float* __restrict__ x, long ldx, int D, float eps,
                                                                   float* __restrict__ out, long ldo) {
  __shared__ float sh[4];
  const long i = blockIdx.x;
  const float* xr = x + i * ldx;
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += RC_THREADS) {
    const float v = xr[d];
    s += v * v;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  const float c = fmaxf(sqrtf(sh[0] + sh[1] + sh[2] + sh[3]), eps);
  for (int d = threadIdx.x; d < D; d += RC_THREADS) out[i * ldo + d] = xr[d] / c;
}

}  // namespace

extern "C" int64_t egv_gt_ranks_work_bytes(int32_t n1, int32_t n2) {
  if (n1 < 0 || n2 < 0) return 0;
  return (int64_t)n1 * n2 * (int64_t)sizeof(float);
}

extern "C" int egv_gt_ranks(const float* S, int64_t lds_, int32_t transposed, int32_t n1, int32_t n2, int64_t row0, int32_t qpv,
                            int32_t seg_wide, const uint8_t* col_valid, int32_t tie_avg, double* rank_out, void* work,
                            void* stream) {
  if (!S || !rank_out || n1 < 1 || n2 < 1 || lds_ < n2 || row0 < 0 || qpv < 1 || (transposed && !work)) return EGV_ERR_ARG;
  const int64_t rows = transposed ? n2 : n1, len = transposed ? n1 : n2;
  // every ground-truth segment inside the row: the kernel reads it without a further check
  if (row0 > INT64_MAX / 4 - rows) return EGV_ERR_ARG;
  const int64_t last = row0 + rows - 1;
  if (seg_wide ? (last + 1 > len / qpv) : (last / qpv >= len)) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (transposed) {
    const int rc = launch_transpose<float>(S, (long)lds_, n1, n2, (float*)work, s);
    if (rc != EGV_OK) return rc;
    S = (const float*)work;
    lds_ = n1;
  }
  if (col_valid)
    EGV_LAUNCH((gt_rank_kernel<true>), dim3((unsigned)rows), dim3(RC_THREADS), 0, s, S, (long)lds_, (long)len, (long)row0, qpv,
               seg_wide, col_valid, tie_avg, rank_out);
  else
    EGV_LAUNCH((gt_rank_kernel<false>), dim3((unsigned)rows), dim3(RC_THREADS), 0, s, S, (long)lds_, (long)len, (long)row0, qpv,
               seg_wide, col_valid, tie_avg, rank_out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_topk_rows(const float* S, int64_t lds_, int32_t rows, int32_t cols, const uint8_t* col_valid, int32_t k,
                             float* vals, int64_t* idx, void* stream) {
  if (!S || !vals || !idx || rows < 1 || cols < 1 || lds_ < cols || k < 1 || k > EGV_TOPK_MAX) return EGV_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (col_valid)
    EGV_LAUNCH((topk_kernel<true>), dim3((unsigned)rows), dim3(RC_THREADS), 0, s, S, (long)lds_, (long)cols, col_valid, k, vals,
               (long long*)idx);
  else
    EGV_LAUNCH((topk_kernel<false>), dim3((unsigned)rows), dim3(RC_THREADS), 0, s, S, (long)lds_, (long)cols, col_valid, k, vals,
               (long long*)idx);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_row_normalize(const float* x, int64_t ldx, int32_t rows, int32_t D, float eps, float* out, int64_t ldo,
                                 void* stream) {
  if (!x || !out || rows < 1 || D < 1 || ldx < D || ldo < D) return EGV_ERR_ARG;
  EGV_LAUNCH(row_normalize_kernel, dim3((unsigned)rows), dim3(RC_THREADS), 0, (hipStream_t)stream, x, (long)ldx, D, eps, out,
             (long)ldo);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}
