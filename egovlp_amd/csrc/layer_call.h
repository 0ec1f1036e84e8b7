// Host-side scaffolding of the one-C-call-per-layer entry points (block.hip: egv_block_fwd / _bwd, text_layer.hip: egv_text_layer_fwd /
// _bwd): the workspace-arena allocator, pointers into an arena, the early return on a failed launch, and the GEMM descriptors every
// such call fills the same way, the layout of the one gradient buffer.  Internal to csrc/; plain C++ (block_plan.h builds on it and is
// compiled on its own by tests/test_block_plan_cpu.py).
#pragma once
#include <stdint.h>

#include "egovlp_hip.h"

#ifndef EGV_OK
#define EGV_OK 0
#define EGV_ERR_ARG 1
#endif

// bump allocator over one arena: byte offsets, every allocation 256-byte aligned
struct Bump {
  static constexpr int64_t ALIGN = 256;
  int64_t off = 0;
  int64_t take(int64_t bytes) {
    const int64_t o = off;
    off += (bytes + ALIGN - 1) / ALIGN * ALIGN;
    return o;
  }
};

// arena base + byte offset (-1: absent -> null)
template <class T>
T* at(void* base, int64_t off) { return off < 0 ? nullptr : (T*)((char*)base + off); }
template <class T>
const T* at(const void* base, int64_t off) { return off < 0 ? nullptr : (const T*)((const char*)base + off); }

#define EGV_TRY(call)                \
  do {                               \
    const int rc__ = (call);         \
    if (rc__ != EGV_OK) return rc__; \
  } while (0)

// gradient buffer of a layer with `nw` weights W[N,K] (nk[i] = {N, K}) and `nln` LayerNorm vectors of D floats: [dW x nw][db x nw]
// [the (dgamma, dbeta) vectors] back to back, offsets in floats (every size is a multiple of 4 floats: D % 32 == 0)
static inline void layer_grad_layout(const int64_t (*nk)[2], int nw, int64_t D, int nln, int64_t* off, int64_t& total) {
  int64_t p = 0;
  auto take = [&](int64_t n) { const int64_t q = p; p += n; return q; };
  for (int i = 0; i < nw; ++i) off[i] = take(nk[i][0] * nk[i][1]);
  for (int i = 0; i < nw; ++i) off[nw + i] = take(nk[i][0]);
  for (int i = 0; i < nln; ++i) off[2 * nw + i] = take(D);
  total = p;
}

// an operand the forward saved in its arena, as the backward reads it: the hi plane, the lo plane only in a three-product backward
static inline void saved_planes(const void* fwd_arena, int bwd_passes, int64_t hi, int64_t lo, const egv_bf16*& ph, const egv_bf16*& pl) {
  ph = at<egv_bf16>(fwd_arena, hi);
  pl = bwd_passes == 3 ? at<egv_bf16>(fwd_arena, lo) : nullptr;
}

// C[M,N] = A[M,K] . B[N,K]^T (forward Linears, dgrads); the caller adds the epilogue fields
static inline egv_gemm_desc nt_desc(const egv_bf16* a_hi, const egv_bf16* a_lo, int64_t lda, const egv_bf16* b_hi, const egv_bf16* b_lo,
                                    int64_t ldb, int64_t M, int64_t N, int64_t K, int passes, int grid_cap, int ksplit = 1,
                                    float* partial = nullptr) {
  egv_gemm_desc d = {};
  d.a_hi = a_hi; d.a_lo = a_lo; d.lda = lda;
  d.b_hi = b_hi; d.b_lo = b_lo; d.ldb = ldb;
  d.M = (int32_t)M; d.N = (int32_t)N; d.K = (int32_t)K; d.passes = passes;
  d.alpha = 1.0f;
  d.ksplit = ksplit;
  d.partial = ksplit > 1 ? partial : nullptr;
  d.grid_cap = grid_cap;
  return d;
}

// the weight gradient dW[N,K] = dY[M,N]^T X[M,K] (TN kernel), the bias gradient (column sums of dY) from the same pass; the caller
// sets alpha / accumulate where they differ from 1 / 0 and chooses the stream
static inline egv_gemm_desc tn_desc(const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy, const egv_bf16* x_hi, const egv_bf16* x_lo,
                                    int64_t ldx, int64_t N, int64_t K, int64_t M, int passes, float* out, float* colsum, int ksplit,
                                    float* partial, int grid_cap) {
  egv_gemm_desc d = nt_desc(dy_hi, dy_lo, lddy, x_hi, x_lo, ldx, N, K, M, passes, grid_cap, ksplit > 1 ? ksplit : 1, partial);
  d.out_f32 = out; d.ldo = K;
  d.trans = 1;
  d.colsum = colsum;
  return d;
}
