// C-ABI entry points of divided space-time attention (VarAttention core, model/video_transformer.py:104-133).
// Patch queries run in the space kernels (attn_mfma_fwd / _bwd.hip: groups of up to 288 keys, K / V of a group in LDS; attn_long.hip:
// more than 288 keys -- input resolutions above 224^2 --, keys and queries walked in 64-row tiles) or the time kernels
// (attn_time_mfma.hip: T <= 16 frames; attn_time_long.hip: 16 < T <= 64) -- all on the matrix cores --; the clip's CLS query row (:109-112) rides along in every
// group of those kernels (see attn_small.hip) and is finished by tiny combine / delta / finish kernels.
// Every call is checked and every launch of it picked (attn_dispatch.h) before the first kernel is enqueued: a refused call writes nothing.
#include "attn_dispatch.h"
#include "egovlp_hip.h"

extern "C" int64_t egv_divided_attn_fwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode) {
  return (int64_t)B * H * (mode == 0 ? T : n) * 68;
}

extern "C" int64_t egv_divided_attn_bwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H) {
  return (int64_t)B * H * (1 + (int64_t)T * n) + (int64_t)B * H * 192;
}

extern "C" int egv_divided_attn_fwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, int32_t B, int32_t T, int32_t n,
                                    int32_t H, int32_t mode, int32_t passes, egv_bf16* out_hi, egv_bf16* out_lo,
                                    float* lse, float* work, void* stream) {
  AttDividedFwd d;
  AttPick p;
  if (att_check_divided_fwd(B, T, n, H, mode, passes, qkv_hi && out_hi && lse && work, qkv_lo != nullptr, out_lo != nullptr, &d))
    return EGV_ERR_ARG;
  if (d.time ? att_pick_time(false, B, T, n, H, passes, d.f16, &p)
             : att_pick_fwd(true, att_space_groups(B, T, H), n + 1, n + 1, passes, d.f16, &p))
    return EGV_ERR_ARG;
  if (!d.qkv_lo) qkv_lo = nullptr;
  if (!d.out_lo) out_lo = nullptr;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (d.time) {
    const AttTimeFwd a = {qkv_hi, qkv_lo, B, T, n, H, out_hi, out_lo, lse, work, d.out_fmt};
    rc = p.family == ATT_TIME_LONG ? egv_attn_time_long_fwd(p, a, s) : egv_attn_time_tile_fwd(p, a, s);
  } else {
    rc = egv_attn_space_fwd_impl(p, qkv_hi, qkv_lo, B, T, n, H, out_hi, out_lo, lse, work, d.out_fmt, s);
  }
  if (rc) return rc;
  return egv_attn_cls_combine_impl(work, B, d.time ? n : T, 1 + T * n, H, out_hi, out_lo, lse, d.out_fmt, s);
}

extern "C" int egv_divided_attn_bwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, const egv_bf16* out_hi,
                                    const egv_bf16* out_lo, const egv_bf16* dout_hi, const egv_bf16* dout_lo,
                                    const float* lse, int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode,
                                    int32_t passes, egv_bf16* dqkv_hi, egv_bf16* dqkv_lo, float* work, void* stream) {
  AttDividedBwd d;
  AttPick p, pkv;
  if (att_check_divided_bwd(B, T, n, H, mode, passes, qkv_hi && out_hi && dout_hi && lse && dqkv_hi && work, qkv_lo != nullptr,
                            out_lo != nullptr, dout_lo != nullptr, dqkv_lo != nullptr, &d))
    return EGV_ERR_ARG;
  const int64_t groups = att_space_groups(B, T, H);
  if (d.time ? att_pick_time(true, B, T, n, H, passes, d.f16, &p)
             : (att_pick_dq(true, groups, n + 1, n + 1, passes, d.f16, &p) || att_pick_dkv(true, groups, n + 1, n + 1, passes, d.f16, &pkv)))
    return EGV_ERR_ARG;
  if (!d.qkv_lo) qkv_lo = nullptr;
  if (!d.out_lo) out_lo = nullptr;
  if (!d.dout_lo) dout_lo = nullptr;
  if (!d.dqkv_lo) dqkv_lo = nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int S = 1 + T * n;
  float* delta = work;                          // [B, H, S]
  float* dcls = work + (long)B * H * S;         // [B, H, 3, 64] raw fp32 accumulators of the CLS token
  int rc = egv_attn_cls_delta_impl(out_hi, out_lo, dout_hi, dout_lo, B, S, H, delta, dcls, d.o_fmt, d.f16, s);   // also zeroes dcls
  if (rc) return rc;
  if (d.time) {
    const AttTimeBwd a = {qkv_hi, qkv_lo, dout_hi, dout_lo, lse, delta, B, T, n, H, dqkv_hi, dqkv_lo, dcls, d.g_fmt};
    rc = p.family == ATT_TIME_LONG ? egv_attn_time_long_bwd(p, a, s) : egv_attn_time_tile_bwd(p, a, s);
  } else {
    rc = egv_attn_space_bwd_impl(p, pkv, qkv_hi, qkv_lo, out_hi, out_lo, dout_hi, dout_lo, lse, delta, dcls, B, T, n, H, dqkv_hi, dqkv_lo,
                                 d.o_fmt, d.g_fmt, s);
  }
  if (rc) return rc;
  return egv_attn_cls_finish_impl(dcls, B, S, H, dqkv_hi, dqkv_lo, d.g_fmt, s);
}
