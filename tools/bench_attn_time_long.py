"""What the time attention past 16 frames (csrc/attn_time_long.hip) costs per call on one GPU, against its own HBM-traffic floor and
against the one-tile kernel of csrc/attn_time_mfma.hip at the same number of tokens:

    python tools/bench_attn_time_long.py [--tokens-of 16] [--iters 20] [--warmup 5]

ViT-B/16 geometry (n = 196 locations, H = 12 heads) at T = 32 and T = 64 in the benchmarked pairing (fp16-split qkv, three-product
forward into 'f16x2' planes; fp16 one-product backward into one fp16 dqkv plane).  `--tokens-of B16`: every shape holds the tokens of B16
clips of 16 frames -- B16 / 2 clips of 32 frames, B16 / 4 of 64 -- and the T = 16 kernel is measured on B16 clips in the same run.
There is no reference GPU path to compare with, so every time is set against the bytes the call cannot avoid:

    forward  : the qkv planes read once + the output planes and lse written once
    backward : the q, k, v plane + the dO plane + lse read once, the dqkv plane written once

(plane = one 16-bit value per element; the forward reads and writes two planes per tensor, the backward one.)  The whole calls
(egv_divided_attn_fwd / _bwd: the CLS combine / delta / finish helpers included) are timed with HIP events over `--iters` calls after
`--warmup`; the time kernels alone come from the profiler's device times of the same calls, and `per_token_vs_T16` is the ratio of
those kernel times (the token counts are equal).  One JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_TBPS = 8.0            # MI355X


def floors(B, T, n, H):
    """bytes (forward, backward) for B clips of T frames of n locations (B (T n + 1) tokens) in the benchmarked pairing"""
    tok, HD = B * (T * n + 1), H * 64
    vec = tok * H * 4                                   # lse
    fwd = tok * 3 * HD * 2 * 2 + tok * HD * 2 * 2 + vec
    bwd = tok * 3 * HD * 2 + tok * HD * 2 + vec + tok * 3 * HD * 2
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens-of", type=int, default=16, help="clips of 16 frames whose tokens every shape holds (a multiple of 4)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.tokens_of < 4 or args.tokens_of % 4:
        raise SystemExit("bench_attn_time_long: --tokens-of is a positive multiple of 4")
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_time_long: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import ops

    def events(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)                    # us

    def kernel_time(fn, pat):
        """median device time (us) of the kernels whose name contains `pat` over `--iters` calls, from the profiler"""
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
        got = [ev.device_time for ev in prof.events() if pat in ev.name and ev.device_time > 0]
        if not got:
            raise SystemExit("bench_attn_time_long: the profiler reported no %s -- is this shape on that path?" % pat)
        return statistics.median(got)

    n, H = 196, 12
    D = H * 64
    rows = args.tokens_of * (1 + 16 * n)
    g = torch.Generator(device="cuda").manual_seed(n + H)
    x = torch.randn(rows, 3 * D, generator=g, device="cuda")
    dy = torch.randn(rows, D, generator=g, device="cuda") * 50.0
    out = {"tokens_of": args.tokens_of, "iters": args.iters, "warmup": args.warmup, "n": n, "H": H, "mode": "f16mix/f16",
           "hbm_peak_TBps": HBM_PEAK_TBPS, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for T in (16, 32, 64):
        B = args.tokens_of * 16 // T
        S = 1 + T * n
        xs = x[:B * S]
        hi = xs.to(torch.float16)
        qkv = ops.Planes(hi, (xs - hi.float()).to(torch.float16), B * S, 3 * D, "f16s")
        dO = ops.f16_cast(dy[:B * S].contiguous())
        fwd = lambda: ops.divided_attn_fwd(qkv, B, T, n, H, 1, 3, out_fmt="f16x2")
        o, lse = fwd()
        bwd = lambda: ops.divided_attn_bwd(qkv, o, dO, lse, B, T, n, H, 1, 1, grad_f16=True)
        kern = "attn_time_mfma_" if T <= 16 else "attn_time_long_"
        t_f, t_b = events(fwd), events(bwd)
        k_f, k_b = kernel_time(fwd, kern + "fwd_kernel"), kernel_time(bwd, kern + "bwd_kernel")
        fl = floors(B, T, n, H)
        row = {"B": B, "tokens": B * S, "fwd_call_us": round(t_f, 1), "bwd_call_us": round(t_b, 1), "fwd_kernel_us": round(k_f, 1),
               "bwd_kernel_us": round(k_b, 1)}
        for key, t, byt in (("fwd", k_f, fl[0]), ("bwd", k_b, fl[1])):
            row[key + "_floor_MB"] = round(byt / 1e6, 1)
            row[key + "_TBps"] = round(byt / t / 1e6, 3)          # bytes / us = MB/s; / 1e6 -> TB/s
            row[key + "_of_peak"] = round(byt / t / 1e6 / HBM_PEAK_TBPS, 3)
        out["shapes"]["T%d" % T] = row
        del qkv, dO, o, lse, hi
        torch.cuda.empty_cache()
    base = out["shapes"]["T16"]
    for T in (32, 64):
        row = out["shapes"]["T%d" % T]
        row["per_token_vs_T16"] = {k: round((row[k + "_kernel_us"] / row["tokens"]) / (base[k + "_kernel_us"] / base["tokens"]), 3)
                                   for k in ("fwd", "bwd")}
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
