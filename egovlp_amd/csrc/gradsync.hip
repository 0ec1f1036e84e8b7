// Gradient exchange format of the data-parallel step (replaces DDP's fp32 buckets, base/base_trainer.py:258):
// the fp32 gradients of a bucket of parameters are scaled by 1/W, rounded to bf16 and packed back to back into ONE flat
// buffer that RCCL all-reduces over xGMI (half the bytes of the reference's fp32 all-reduce: 362 MB instead of 724 MB per
// step for the 180.9 M parameters), then unpacked into the fp32 .grad tensors the optimizer reads.  Both directions are one
// multi-tensor launch per bucket (pointer tables travel in the kernel arguments), 16-byte accesses, pure HBM traffic:
// 4 B read + 2 B written per element packing, 2 B + 4 B unpacking.
#include "common.h"
#include "egovlp_hip.h"
#include "multi_tensor.h"

namespace {

constexpr int MAX_T = 96;        // tensors per launch
constexpr int CHUNK = 16384;     // elements per block

struct PackTable {
  float* f32[MAX_T];             // the fp32 side (source when packing, destination when unpacking)
  long off[MAX_T];               // element offset of the tensor inside the flat bf16 buffer
  long numel[MAX_T];
  MtIndex<MAX_T> ix;
};
static_assert(sizeof(PackTable) <= 4096, "the table travels in the kernel arguments");

template <bool PACK>
__global__ __launch_bounds__(256) void grad_pack_kernel(const PackTable t, bf16_t* __restrict__ flat, float scale) {
  const MtWork w = mt_locate(t.ix);
  const int ti = w.item;
  const long base = (long)w.block * CHUNK;
  const long n = t.numel[ti];
  float* __restrict__ f = t.f32[ti];
  bf16_t* __restrict__ b = flat + t.off[ti];
  const long end = min(n, base + CHUNK);
  const bool vec = ((n & 3) == 0) && ((((size_t)f) & 15) == 0) && ((((size_t)b) & 7) == 0);
  if (vec) {
    for (long i = base + threadIdx.x * 4; i < end; i += 256 * 4) {
      if (PACK) {
        const f32x4_t v = *(const f32x4_t*)(f + i) * scale;
        *(u32x2_t*)(b + i) = (u32x2_t){pack2(f32_to_bf16(v[0]), f32_to_bf16(v[1])), pack2(f32_to_bf16(v[2]), f32_to_bf16(v[3]))};
      } else {
        const u32x2_t w = *(const u32x2_t*)(b + i);
        *(f32x4_t*)(f + i) = (f32x4_t){__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u),
                                       __uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xffff0000u)};
      }
    }
  } else {
    for (long i = base + threadIdx.x; i < end; i += 256) {
      if (PACK) b[i] = f32_to_bf16(f[i] * scale);
      else f[i] = bf16_to_f32(b[i]);
    }
  }
}

template <bool PACK>
int run(int32_t count, float* const* f32, const int64_t* numel, bf16_t* flat, const int64_t* off, float scale, hipStream_t s) {
  if (count < 0 || !f32 || !numel || !flat || !off) return EGV_ERR_ARG;
  return mt_for_each_launch<PackTable>(
      count,
      [&](int i) -> int64_t {
        if (numel[i] <= 0) return 0;
        return (f32[i] && off[i] >= 0) ? pieces(numel[i], CHUNK) : -1;
      },
      [&](PackTable& t, int k, int i) { t.f32[k] = f32[i]; t.off[k] = off[i]; t.numel[k] = numel[i]; },
      [&](const PackTable& t, int nb) -> int {
        EGV_LAUNCH(grad_pack_kernel<PACK>, dim3(nb), dim3(256), 0, s, t, flat, scale);
        EGV_CHECK_LAUNCH();
        return EGV_OK;
      });
}

// The local step of the DIRECT exchange (egovlp_amd.dist.Bf16GradSync, exchange = "direct"): after the all-to-all every rank holds
// `world` slices -- its own slice of every peer's bucket, back to back -- and sums them in FP32 (one rounding to bf16 at the end,
// where a bf16 all-reduce rounds after every one of its world - 1 additions); the reduced slice is then all-gathered.
// 16-byte accesses (8 bf16 per lane), world <= 64.
__global__ __launch_bounds__(256) void slice_sum_kernel(const bf16_t* __restrict__ recv, int world, long slice, bf16_t* __restrict__ out) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= slice) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < world; ++p) {
    const u32x4_t w = *(const u32x4_t*)(recv + (long)p * slice + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[2 * e] += __uint_as_float(w[e] << 16);
      acc[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
    }
  }
  *(u32x4_t*)(out + i) = (u32x4_t){f32x2_to_bf16x2(acc[0], acc[1]), f32x2_to_bf16x2(acc[2], acc[3]), f32x2_to_bf16x2(acc[4], acc[5]),
                                   f32x2_to_bf16x2(acc[6], acc[7])};
}

}  // namespace

extern "C" int egv_slice_sum_bf16(const egv_bf16* recv, int32_t world, int64_t slice_elems, egv_bf16* out, void* stream) {
  if (!recv || !out || world < 1 || world > 64 || slice_elems <= 0 || slice_elems % 8 != 0) return EGV_ERR_ARG;
  if ((((size_t)recv) & 15) || (((size_t)out) & 15)) return EGV_ERR_ARG;
  const long lanes = slice_elems / 8;
  EGV_LAUNCH(slice_sum_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, recv, world, (long)slice_elems,
             (bf16_t*)out);
  EGV_CHECK_LAUNCH();
  return EGV_OK;
}

extern "C" int egv_grad_pack_bf16(int32_t count, const float* const* grads, const int64_t* numel, egv_bf16* flat,
                                  const int64_t* offsets, float scale, void* stream) {
  return run<true>(count, (float* const*)grads, numel, flat, offsets, scale, (hipStream_t)stream);
}

extern "C" int egv_grad_unpack_bf16(int32_t count, float* const* grads, const int64_t* numel, const egv_bf16* flat,
                                    const int64_t* offsets, void* stream) {
  return run<false>(count, grads, numel, (bf16_t*)flat, offsets, 1.0f, (hipStream_t)stream);
}
