// The recording stub and the sweep of tools/block_call_census.py: linked against the host-only objects of csrc/block.hip and
// csrc/text_layer.hip in place of the library, it answers every entry point those two files call by printing the call -- every scalar,
// every field of every egv_gemm_desc, every pointer as region+byte offset -- so that two trees can be compared call by call without
// a GPU.  No memory stands behind the pointers: every region is a 2^40-byte address range of its own, nothing is dereferenced except
// the host arrays of egv_splitk_reduce_multi / egv_layernorm_bwd_reduce.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "egovlp_hip.h"

namespace {

const char* const REGIONS[] = {"x", "out", "fwd_arena", "bwd_arena", "grads", "g_out", "g_hi", "g_lo", "d_x", "dx_hi", "dx_lo", "mask", "seed_dev",
                               "stream", "side_a", "side_b", "ln0", "ln1", "ln2", "ln3", "ln4", "ln5",
                               "bias0", "bias1", "bias2", "bias3", "bias4", "bias5", "w_hi0", "w_hi1", "w_hi2", "w_hi3", "w_hi4", "w_hi5",
                               "w_lo0", "w_lo1", "w_lo2", "w_lo3", "w_lo4", "w_lo5", "wt_hi0", "wt_hi1", "wt_hi2", "wt_hi3", "wt_hi4", "wt_hi5",
                               "wt_lo0", "wt_lo1", "wt_lo2", "wt_lo3", "wt_lo4", "wt_lo5", "event0", "event1", "event2", "event3", "event4", "event5"};
constexpr int NREG = sizeof(REGIONS) / sizeof(REGIONS[0]);

template <class T = void>
T* region(const char* name, int idx = -1) {
  char buf[32];
  if (idx >= 0) snprintf(buf, sizeof buf, "%s%d", name, idx); else snprintf(buf, sizeof buf, "%s", name);
  for (int i = 0; i < NREG; ++i)
    if (!strcmp(REGIONS[i], buf)) return (T*)((uint64_t)(i + 1) << 40);
  fprintf(stderr, "no region %s\n", buf);
  abort();
}

int calls = 0;      // of the current case

void P(const char* name, const void* p) {
  const uint64_t a = (uint64_t)p;
  if (!a) { printf(" %s=0", name); return; }
  const uint64_t r = a >> 40;
  if (r < 1 || r > (uint64_t)NREG) printf(" %s=?%llx", name, (unsigned long long)a);
  else printf(" %s=%s+%llu", name, REGIONS[r - 1], (unsigned long long)(a & ((1ull << 40) - 1)));
}
void I(const char* name, long long v) { printf(" %s=%lld", name, v); }
void F(const char* name, double v) { printf(" %s=%.9g", name, v); }
void call(const char* name) { ++calls; printf("  %s", name); }
int done() { printf("\n"); return 0; }      // EGV_OK

}  // namespace

#define PP(x) P(#x, x)
#define II(x) I(#x, (long long)(x))
#define FF(x) F(#x, (double)(x))

// ---- fixed stand-ins for the workspace formulas (any function of the arguments: the layouts only add them up)
extern "C" int64_t egv_divided_attn_fwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode) {
  return (int64_t)B * H * (1 + (int64_t)T * n) * (mode ? 3 : 5) + 7;
}
extern "C" int64_t egv_divided_attn_bwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H) { return (int64_t)B * H * (1 + (int64_t)T * n) * 2 + 64 * H; }
extern "C" int egv_layernorm_bwd_parts(int32_t rows) { return rows < 64 * 256 ? (rows + 63) / 64 : 256; }
extern "C" int64_t egv_cls_linear_work_floats(int32_t R, int32_t N, int32_t K) { return (int64_t)R * K * 8 + N; }

extern "C" hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) { call("hipEventRecord"); PP(event); PP(stream); done(); return hipSuccess; }
extern "C" hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int flags) {
  call("hipStreamWaitEvent"); PP(stream); PP(event); II(flags); done(); return hipSuccess;
}

extern "C" int egv_gemm_nt(const egv_gemm_desc* d, void* stream) {
  call("egv_gemm_nt");
  P("a_hi", d->a_hi); P("a_lo", d->a_lo); I("lda", d->lda); P("b_hi", d->b_hi); P("b_lo", d->b_lo); I("ldb", d->ldb);
  I("M", d->M); I("N", d->N); I("K", d->K); I("passes", d->passes); F("alpha", d->alpha); I("act", d->act); P("bias", d->bias);
  P("residual", d->residual); I("ldr", d->ldr); P("aux_in", d->aux_in); P("aux_out", d->aux_out); I("ldaux", d->ldaux);
  P("out_f32", d->out_f32); I("ldo", d->ldo); P("out_hi", d->out_hi); P("out_lo", d->out_lo); I("ldoh", d->ldoh); I("ksplit", d->ksplit);
  I("accumulate", d->accumulate); P("partial", d->partial); I("trans", d->trans); I("aux_bf16", d->aux_bf16); P("colsum", d->colsum);
  I("grid_cap", d->grid_cap); I("out_fmt", d->out_fmt); P("out_bf", d->out_bf); PP(stream);
  return done();
}
extern "C" int egv_splitk_reduce_multi(int32_t count, const float* const* partial, float* const* out, const int64_t* mn, const int32_t* ksplit,
                                       float* const* colsum, const int32_t* m, void* stream) {
  call("egv_splitk_reduce_multi"); II(count);
  for (int i = 0; i < count; ++i) { PP(partial[i]); PP(out[i]); II(mn[i]); II(ksplit[i]); PP(colsum[i]); II(m[i]); }
  PP(stream);
  return done();
}
extern "C" int egv_split_f32(const float* x, int64_t ldx, int32_t rows, int32_t cols, egv_bf16* hi, egv_bf16* lo, int64_t ldo, egv_bf16* t_hi,
                             egv_bf16* t_lo, int64_t ldt, float* colsum, void* stream) {
  call("egv_split_f32"); PP(x); II(ldx); II(rows); II(cols); PP(hi); PP(lo); II(ldo); PP(t_hi); PP(t_lo); II(ldt); PP(colsum); PP(stream);
  return done();
}
extern "C" int egv_f16x2_encode(const float* x, int64_t ldx, int32_t rows, int32_t cols, uint16_t* p1, uint16_t* p2, egv_bf16* bf, int64_t ldo,
                                int32_t role, void* stream) {
  call("egv_f16x2_encode"); PP(x); II(ldx); II(rows); II(cols); PP(p1); PP(p2); PP(bf); II(ldo); II(role); PP(stream);
  return done();
}
extern "C" int egv_layernorm_fwd_f16x2(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, int32_t rows, int32_t cols,
                                       uint16_t* y1, uint16_t* y2, egv_bf16* ybf, int64_t ldy, float* mean, float* rstd, void* stream) {
  call("egv_layernorm_fwd_f16x2"); PP(x); II(ldx); PP(gamma); PP(beta); FF(eps); II(rows); II(cols); PP(y1); PP(y2); PP(ybf); II(ldy); PP(mean);
  PP(rstd); PP(stream);
  return done();
}
extern "C" int egv_layernorm_fwd(const float* x, const float* x_add, int64_t ldx, const float* gamma, const float* beta, float eps, int32_t rows,
                                 int32_t cols, float* sum_out, egv_bf16* y_hi, egv_bf16* y_lo, float* y_f32, int64_t ldy, float* mean, float* rstd,
                                 void* stream) {
  call("egv_layernorm_fwd"); PP(x); PP(x_add); II(ldx); PP(gamma); PP(beta); FF(eps); II(rows); II(cols); PP(sum_out); PP(y_hi); PP(y_lo); PP(y_f32);
  II(ldy); PP(mean); PP(rstd); PP(stream);
  return done();
}
static int ln_bwd(const char* name, const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy, const float* x, int64_t ldx,
                  const float* gamma, const float* mean, const float* rstd, int32_t rows, int32_t cols, const float* add1, const float* add2,
                  float* dx, int64_t lddx, egv_bf16* dx_hi, egv_bf16* dx_lo, int32_t dx_fmt, float* dgamma, float* dbeta, float* work, void* stream) {
  call(name); PP(dy); PP(dy_hi); PP(dy_lo); II(lddy); PP(x); II(ldx); PP(gamma); PP(mean); PP(rstd); II(rows); II(cols); PP(add1); PP(add2); PP(dx);
  II(lddx); PP(dx_hi); PP(dx_lo); II(dx_fmt); PP(dgamma); PP(dbeta); PP(work); PP(stream);
  return done();
}
extern "C" int egv_layernorm_bwd(const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy, const float* x, int64_t ldx,
                                 const float* gamma, const float* mean, const float* rstd, int32_t rows, int32_t cols, const float* add1,
                                 const float* add2, float* dx, int64_t lddx, egv_bf16* dx_hi, egv_bf16* dx_lo, float* dgamma, float* dbeta, float* work,
                                 void* stream) {
  return ln_bwd("egv_layernorm_bwd", dy, dy_hi, dy_lo, lddy, x, ldx, gamma, mean, rstd, rows, cols, add1, add2, dx, lddx, dx_hi, dx_lo, -1, dgamma,
                dbeta, work, stream);
}
extern "C" int egv_layernorm_bwd_partial(const float* dy, const egv_bf16* dy_hi, const egv_bf16* dy_lo, int64_t lddy, const float* x, int64_t ldx,
                                         const float* gamma, const float* mean, const float* rstd, int32_t rows, int32_t cols, const float* add1,
                                         const float* add2, float* dx, int64_t lddx, egv_bf16* dx_hi, egv_bf16* dx_lo, int32_t dx_fmt, float* dgamma,
                                         float* dbeta, float* work, void* stream) {
  return ln_bwd("egv_layernorm_bwd_partial", dy, dy_hi, dy_lo, lddy, x, ldx, gamma, mean, rstd, rows, cols, add1, add2, dx, lddx, dx_hi, dx_lo, dx_fmt,
                dgamma, dbeta, work, stream);
}
extern "C" int egv_layernorm_bwd_reduce(int32_t count, const float* const* work, int32_t rows, int32_t cols, float* const* dgamma,
                                        float* const* dbeta, void* stream) {
  call("egv_layernorm_bwd_reduce"); II(count);
  for (int i = 0; i < count; ++i) { PP(work[i]); PP(dgamma[i]); PP(dbeta[i]); }
  II(rows); II(cols); PP(stream);
  return done();
}
extern "C" int egv_divided_attn_fwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode,
                                    int32_t passes, egv_bf16* out_hi, egv_bf16* out_lo, float* lse, float* work, void* stream) {
  call("egv_divided_attn_fwd"); PP(qkv_hi); PP(qkv_lo); II(B); II(T); II(n); II(H); II(mode); II(passes); PP(out_hi); PP(out_lo); PP(lse); PP(work);
  PP(stream);
  return done();
}
extern "C" int egv_divided_attn_bwd(const egv_bf16* qkv_hi, const egv_bf16* qkv_lo, const egv_bf16* out_hi, const egv_bf16* out_lo,
                                    const egv_bf16* dout_hi, const egv_bf16* dout_lo, const float* lse, int32_t B, int32_t T, int32_t n, int32_t H,
                                    int32_t mode, int32_t passes, egv_bf16* dqkv_hi, egv_bf16* dqkv_lo, float* work, void* stream) {
  call("egv_divided_attn_bwd"); PP(qkv_hi); PP(qkv_lo); PP(out_hi); PP(out_lo); PP(dout_hi); PP(dout_lo); PP(lse); II(B); II(T); II(n); II(H); II(mode);
  II(passes); PP(dqkv_hi); PP(dqkv_lo); PP(work); PP(stream);
  return done();
}
extern "C" int egv_cls_linear_fwd(const float* x, int64_t ldx, const float* W, int64_t ldw, const float* bias, int32_t R, int32_t N, int32_t K,
                                  int32_t act, float* z_out, const float* residual, int64_t ldr, float* y, int64_t ldy, void* stream) {
  call("egv_cls_linear_fwd"); PP(x); II(ldx); PP(W); II(ldw); PP(bias); II(R); II(N); II(K); II(act); PP(z_out); PP(residual); II(ldr); PP(y); II(ldy);
  PP(stream);
  return done();
}
extern "C" int egv_cls_linear_dgrad(const float* dy, int64_t lddy, const float* W, int64_t ldw, int32_t R, int32_t N, int32_t K, const float* z,
                                    void* dx, int64_t lddx, int32_t dx_mode, float* work, void* stream) {
  call("egv_cls_linear_dgrad"); PP(dy); II(lddy); PP(W); II(ldw); II(R); II(N); II(K); PP(z); PP(dx); II(lddx); II(dx_mode); PP(work); PP(stream);
  return done();
}
extern "C" int egv_cls_linear_wgrad(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t R, int32_t N, int32_t K, float* dW,
                                    int64_t lddw, float* db, void* stream) {
  call("egv_cls_linear_wgrad"); PP(dy); II(lddy); PP(x); II(ldx); II(R); II(N); II(K); PP(dW); II(lddw); PP(db); PP(stream);
  return done();
}
extern "C" int egv_cls_rows_add(float* dst, int64_t lddst, const float* src, int64_t ldsrc, int32_t R, int32_t cols, void* stream) {
  call("egv_cls_rows_add"); PP(dst); II(lddst); PP(src); II(ldsrc); II(R); II(cols); PP(stream);
  return done();
}
extern "C" int egv_cls_attn_fwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi, const uint16_t* v_lo,
                                int64_t ldkv, int32_t kv_fmt, int32_t B, int32_t S, int32_t H, float* out, int64_t ldo, float* lse, void* stream) {
  call("egv_cls_attn_fwd"); PP(q); II(ldq); PP(k_hi); PP(k_lo); PP(v_hi); PP(v_lo); II(ldkv); II(kv_fmt); II(B); II(S); II(H); PP(out); II(ldo); PP(lse);
  PP(stream);
  return done();
}
extern "C" int egv_cls_attn_bwd(const float* q, int64_t ldq, const uint16_t* k_hi, const uint16_t* k_lo, const uint16_t* v_hi, const uint16_t* v_lo,
                                int64_t ldkv, int32_t kv_fmt, const float* out, const float* d_out, const float* lse, int32_t B, int32_t S, int32_t H,
                                float* dq, uint16_t* dk_hi, uint16_t* dk_lo, uint16_t* dv_hi, uint16_t* dv_lo, int64_t lddkv, int32_t d_fmt,
                                void* stream) {
  call("egv_cls_attn_bwd"); PP(q); II(ldq); PP(k_hi); PP(k_lo); PP(v_hi); PP(v_lo); II(ldkv); II(kv_fmt); PP(out); PP(d_out); PP(lse); II(B); II(S); II(H);
  PP(dq); PP(dk_hi); PP(dk_lo); PP(dv_hi); PP(dv_lo); II(lddkv); II(d_fmt); PP(stream);
  return done();
}
extern "C" int egv_text_attn_fwd(const float* q, const float* k, const float* v, int64_t ldqkv, const int64_t* mask, int32_t B, int32_t L, int32_t H,
                                 int32_t passes, float dropout_p, uint64_t seed, const uint64_t* seed_dev, egv_bf16* out_hi, egv_bf16* out_lo, float* lse,
                                 void* stream) {
  call("egv_text_attn_fwd"); PP(q); PP(k); PP(v); II(ldqkv); PP(mask); II(B); II(L); II(H); II(passes); FF(dropout_p); II(seed); PP(seed_dev); PP(out_hi);
  PP(out_lo); PP(lse); PP(stream);
  return done();
}
extern "C" int egv_text_attn_bwd(const float* q, const float* k, const float* v, int64_t ldqkv, const int64_t* mask, const float* d_out, const float* lse,
                                 int32_t B, int32_t L, int32_t H, int32_t passes, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* dq,
                                 float* dk, float* dv, int64_t lddqkv, float* delta_work, void* stream) {
  call("egv_text_attn_bwd"); PP(q); PP(k); PP(v); II(ldqkv); PP(mask); PP(d_out); PP(lse); II(B); II(L); II(H); II(passes); FF(dropout_p); II(seed);
  PP(seed_dev); PP(dq); PP(dk); PP(dv); II(lddqkv); PP(delta_work); PP(stream);
  return done();
}
extern "C" int egv_dropout(const float* x, const float* add, float* out, int64_t n, float p, uint64_t seed, const uint64_t* seed_dev, void* stream) {
  call("egv_dropout"); PP(x); PP(add); PP(out); II(n); FF(p); II(seed); PP(seed_dev); PP(stream);
  return done();
}

// ---------------------------------------------------------------------------------------------------------------- the sweep
namespace {

egv_block_params block_params(int64_t D, int64_t Hd) {
  egv_block_params p = {};
  const int64_t NK[6][2] = {{3 * D, D}, {D, D}, {3 * D, D}, {D, D}, {Hd, D}, {D, Hd}};
  const float** ln[6] = {&p.n3w, &p.n3b, &p.n1w, &p.n1b, &p.n2w, &p.n2b};
  for (int i = 0; i < 6; ++i) {
    *ln[i] = region<float>("ln", i);
    p.bias[i] = region<float>("bias", i);
    p.w_hi[i] = region<egv_bf16>("w_hi", i); p.w_lo[i] = region<egv_bf16>("w_lo", i);
    p.wt_hi[i] = region<egv_bf16>("wt_hi", i); p.wt_lo[i] = region<egv_bf16>("wt_lo", i);
    p.ldw[i] = NK[i][1]; p.ldwt[i] = NK[i][0];
  }
  return p;
}

const int32_t KSPLITS[3][6] = {{1, 1, 1, 1, 1, 1}, {1, 2, 4, 1, 3, 2}, {8, 8, 8, 8, 8, 8}};

// "@ <group> | <case>": the group is what tests/golden/block_call_census.sha256 keeps one digest of
void head(const char* entry, const egv_block_geom& g, bool accepted, int geo, const char* variant) {
  if (accepted) printf("@ %s P%d Pb%d train%d", entry, g.fwd_passes, g.bwd_passes, g.train);
  else printf("@ %s refused", entry);
  printf(" | geo%d P=%d Pb=%d train=%d z_bf16=%d single=%d %s\n", geo, g.fwd_passes, g.bwd_passes, g.train, g.z_bf16, g.f16_single, variant);
  calls = 0;
}
void tail_line(int rc) { printf("  -> rc %d after %d calls\n", rc, calls); }

void block_sizes(const egv_block_geom& g, bool ok, int geo) {
  head("egv_block_sizes", g, ok, geo, "");
  printf("  fwd_arena_bytes %lld\n", (long long)egv_block_fwd_arena_bytes(&g));
  int64_t off[18] = {}, tot = 0;
  int rc = egv_block_fwd_offsets(&g, off);
  printf("  fwd_offsets rc %d:", rc);
  for (int i = 0; i < 11; ++i) printf(" %lld", (long long)off[i]);
  memset(off, 0, sizeof off);
  rc = egv_block_grad_layout(&g, off, &tot);
  printf("\n  grad_layout rc %d:", rc);
  for (int i = 0; i < 18; ++i) printf(" %lld", (long long)off[i]);
  printf(" total %lld\n", (long long)tot);
  printf("  bwd_arena_bytes null %lld", (long long)egv_block_bwd_arena_bytes(&g, nullptr));
  for (int k = 0; k < 3; ++k) printf(" ks%d %lld", k, (long long)egv_block_bwd_arena_bytes(&g, KSPLITS[k]));
  printf("\n");
}

void block_fwd(const egv_block_geom& g, bool ok, int geo, const char* variant, const egv_block_params& p) {
  head("egv_block_fwd", g, ok, geo, variant);
  tail_line(egv_block_fwd(&g, &p, region<float>("x"), region<float>("out"), region("fwd_arena"), region("stream")));
}

egv_block_bwd_io block_io(bool planes, int ks, int streams) {
  egv_block_bwd_io io = {};
  io.g_out = region<float>("g_out");
  if (planes) { io.g_hi = region<egv_bf16>("g_hi"); io.g_lo = region<egv_bf16>("g_lo"); }
  io.x = region<float>("x"); io.fwd_arena = region("fwd_arena"); io.bwd_arena = region("bwd_arena");
  io.d_x = region<float>("d_x"); io.dx_hi = region<egv_bf16>("dx_hi"); io.dx_lo = region<egv_bf16>("dx_lo");
  io.grads = region<float>("grads");
  for (int i = 0; i < 6; ++i) {
    io.side_stream[i] = streams == 0 ? nullptr : region(streams == 2 && (i & 1) ? "side_b" : "side_a");
    io.side_event[i] = streams == 0 ? nullptr : region("event", i);
    io.wgrad_ksplit[i] = KSPLITS[ks][i];
  }
  return io;
}

void block_bwd(const egv_block_geom& g, bool ok, int geo, const char* variant, const egv_block_params& p, const egv_block_bwd_io& io) {
  head("egv_block_bwd", g, ok, geo, variant);
  tail_line(egv_block_bwd(&g, &p, &io, region("stream")));
}

void block_sweep() {
  const int32_t GEO[3][5] = {{2, 2, 4, 4, 1024}, {32, 4, 196, 12, 3072}, {64, 16, 196, 12, 3072}};   // B, T, n, H, Hd
  for (int geo = 0; geo < 3; ++geo) {
    const egv_block_params full = block_params(64 * GEO[geo][3], GEO[geo][4]);
    for (int P = 0; P <= 4; ++P)
      for (int Pb = 0; Pb <= 5; ++Pb)
        for (int train = -1; train <= 4; ++train)
          for (int z = 0; z <= 1; ++z)
            for (int single = -1; single <= 16; ++single) {
              egv_block_geom g = {};
              g.B = GEO[geo][0]; g.T = GEO[geo][1]; g.n = GEO[geo][2]; g.H = GEO[geo][3]; g.D = 64 * g.H; g.Hd = GEO[geo][4];
              g.fwd_passes = P; g.bwd_passes = Pb; g.train = train; g.z_bf16 = z; g.eps = 1e-6f; g.grid_cap = geo == 1 ? 248 : 0; g.f16_single = single;
              const bool ok = egv_block_fwd_arena_bytes(&g) >= 0;
              block_sizes(g, ok, geo);
              if (!ok) {
                if ((P * 31 + Pb * 17 + train * 7 + z * 3 + single) % 11 == 0) {      // a sample of the refused ones: nothing is enqueued
                  block_fwd(g, ok, geo, "", full);
                  block_bwd(g, ok, geo, "", full, block_io(true, 0, 0));
                }
                continue;
              }
              block_fwd(g, ok, geo, "", full);
              {   // refusals by a missing pointer: a weight's lo plane, the tail's master weights
                egv_block_params p = full;
                p.w_lo[2] = nullptr;
                block_fwd(g, ok, geo, "w_lo[2]=0", p);
                p = full;
                p.wt_hi[4] = nullptr;
                block_fwd(g, ok, geo, "wt_hi[4]=0", p);
              }
              if (!(train & 1)) {
                block_bwd(g, ok, geo, "eval", full, block_io(false, 0, 0));
                continue;
              }
              for (int planes = 0; planes <= 1; ++planes)
                for (int ks = 0; ks < 3; ++ks)
                  for (int streams = 0; streams < 3; ++streams) {
                    char v[64];
                    snprintf(v, sizeof v, "g_hi=%d ks%d streams%d", planes, ks, streams);
                    block_bwd(g, ok, geo, v, full, block_io(planes && !(train & 2), ks, streams));
                  }
              {
                egv_block_bwd_io io = block_io(true, 1, 1);
                block_bwd(g, ok, geo, "g_hi=1 (tail: refused)", full, io);
                io = block_io(false, 1, 1); io.dx_lo = nullptr;
                block_bwd(g, ok, geo, "dx_lo=0", full, io);
                io = block_io(true, 1, 1); io.g_lo = nullptr;
                block_bwd(g, ok, geo, "g_lo=0", full, io);
                egv_block_params p = full;
                p.wt_lo[1] = nullptr;
                block_bwd(g, ok, geo, "wt_lo[1]=0", p, block_io(false, 1, 2));
                p = full;
                p.w_hi[3] = nullptr;
                block_bwd(g, ok, geo, "w_hi[3]=0", p, block_io(false, 0, 1));
              }
            }
  }
}

void text_sweep() {
  const int PASSES[3][2] = {{1, 1}, {3, 1}, {3, 3}};
  egv_text_params p = {};
  const float** ln[4] = {&p.ln1w, &p.ln1b, &p.ln2w, &p.ln2b};
  for (int i = 0; i < 4; ++i) {
    *ln[i] = region<float>("ln", i);
    p.bias[i] = region<float>("bias", i);
    p.w_hi[i] = region<egv_bf16>("w_hi", i); p.w_lo[i] = region<egv_bf16>("w_lo", i);
    p.wt_hi[i] = region<egv_bf16>("wt_hi", i); p.wt_lo[i] = region<egv_bf16>("wt_lo", i);
    p.ldw[i] = i == 3 ? 3072 : 768; p.ldwt[i] = i == 0 ? 2304 : (i == 2 ? 3072 : 768);
  }
  for (int pi = 0; pi < 4; ++pi)
    for (int train = 0; train <= 1; ++train)
      for (int drop = 0; drop <= 1; ++drop)
        for (int split = 0; split <= 1; ++split) {
          egv_text_geom g = {};
          g.B = 32; g.L = 32; g.H = 12; g.D = 768; g.Hd = 3072;
          g.fwd_passes = pi < 3 ? PASSES[pi][0] : 1; g.bwd_passes = pi < 3 ? PASSES[pi][1] : 3;      // the fourth pair is refused
          g.train = train; g.eps = 1e-12f; g.attn_p = drop ? 0.1f : 0.0f; g.ffn_p = drop ? 0.1f : 0.0f; g.grid_cap = 248;
          g.attn_seed = 0x1234567ull; g.ffn_seed = 0x7654321ull; g.seed_dev = drop ? region<uint64_t>("seed_dev") : nullptr;
          const int32_t KS[3][4] = {{2, 3, 1, 4}, {1, 2, 4, 3}, {4, 1, 3, 2}};
          for (int i = 0; i < 4; ++i) { g.nt_ksplit_fwd[i] = split ? KS[0][i] : 1; g.nt_ksplit_bwd[i] = split ? KS[1][i] : 1; g.wgrad_ksplit[i] = split ? KS[2][i] : 1; }
          for (int what = 0; what < 3; ++what) {
            const char* entry = what == 0 ? "egv_text_layer_sizes" : what == 1 ? "egv_text_layer_fwd" : "egv_text_layer_bwd";
            printf("@ %s P%d Pb%d train%d | drop=%d split=%d\n", entry, g.fwd_passes, g.bwd_passes, train, drop, split);
            calls = 0;
            if (what == 0) {
              int64_t off[12] = {}, tot = 0;
              const int rc = egv_text_layer_grad_layout(&g, off, &tot);
              printf("  fwd_arena_bytes %lld bwd_arena_bytes %lld grad_layout rc %d:", (long long)egv_text_layer_fwd_arena_bytes(&g),
                     (long long)egv_text_layer_bwd_arena_bytes(&g), rc);
              for (int i = 0; i < 12; ++i) printf(" %lld", (long long)off[i]);
              printf(" total %lld\n", (long long)tot);
            } else if (what == 1) {
              tail_line(egv_text_layer_fwd(&g, &p, region<float>("x"), region<int64_t>("mask"), region<float>("out"), region("fwd_arena"), region("stream")));
            } else {
              tail_line(egv_text_layer_bwd(&g, &p, region<float>("g_out"), region<int64_t>("mask"), region("fwd_arena"), region("bwd_arena"),
                                           region<float>("d_x"), region<float>("grads"), region("stream")));
            }
          }
        }
}

}  // namespace

int main() {
  block_sweep();
  text_sweep();
  return 0;
}
