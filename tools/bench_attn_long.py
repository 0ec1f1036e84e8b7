"""What the key-tiled space attention (csrc/attn_long.hip) costs per call on one GPU, against its own HBM-traffic floor:

    python tools/bench_attn_long.py [--groups 64] [--iters 20] [--warmup 5]

Two shapes: ViT-B/16 at 384^2 (B.T = 64 frame groups x 12 heads, n = 576 patches, 577 keys) and ViT-L/14 at 336^2 (64 x 16 heads, n = 576),
each in the benchmarked pairing (fp16-split qkv, three-product forward into 'f16x2' planes; fp16 one-product backward) and in 'bf16x3'.
There is no reference GPU path to compare with, so every time is set against the bytes the call cannot avoid:

    forward : the qkv planes read once + the output planes and lse written once
    dQ      : q, k, v planes + dO + O + lse read once, dq + delta written once
    dK / dV : q, k, v planes + dO + lse + delta read once, dk + dv written once

(plane = one 16-bit value per element; the three-product modes have two planes per tensor.)  The whole forward / backward calls
(egv_divided_attn_fwd / _bwd: the CLS combine / delta / finish helpers included) are timed with HIP events over `--iters` calls after
`--warmup`; the split of the backward into its dQ and dK/dV kernels comes from the profiler's device times of the same calls.  One JSON
line."""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def floors(B, T, n, H, planes_qkv, planes_out, planes_do, planes_g):
    """bytes (forward, dQ, dK/dV) for B clips of T frames of n patches (B (T n + 1) tokens)."""
    tok, HD = B * (T * n + 1), H * 64
    qkv = tok * 3 * HD * 2 * planes_qkv
    out = tok * HD * 2 * planes_out
    do = tok * HD * 2 * planes_do
    vec = tok * H * 4                                   # lse or delta
    fwd = qkv + out + vec
    dq = qkv + do + out + vec + tok * HD * 2 * planes_g + vec
    dkv = qkv + do + 2 * vec + tok * 2 * HD * 2 * planes_g
    return fwd, dq, dkv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=64, help="B.T frame groups (clips of 4 frames)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_long: needs an MI355X (there is no CPU measurement path)")
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

    def kernel_split(fn):
        """median device time (us) of the dQ and dK/dV kernels of one backward call, from the profiler"""
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
        got = {"dq": [], "dkv": []}
        for ev in prof.events():
            for key, pat in (("dq", "attn_long_dq_kernel"), ("dkv", "attn_long_dkv_kernel")):
                dt = ev.device_time
                if pat in ev.name and dt > 0:
                    got[key].append(dt)
        if not got["dq"] or not got["dkv"]:
            raise SystemExit("bench_attn_long: the profiler reported no attn_long kernels -- is this shape on the long path?")
        return statistics.median(got["dq"]), statistics.median(got["dkv"])

    out = {"groups": args.groups, "iters": args.iters, "warmup": args.warmup, "shapes": {}}
    T, B = 4, max(1, args.groups // 4)
    for name, n, H in (("vit_b16_384", 576, 12), ("vit_l14_336", 576, 16)):
        S, D = 1 + T * n, H * 64
        g = torch.Generator().manual_seed(n + H)
        x = torch.randn(B * S, 3 * D, generator=g)
        dy = torch.randn(B * S, D, generator=g) * 50.0
        res = {}
        for mode in ("f16mix/f16", "bf16x3"):
            if mode == "bf16x3":
                qkv = ops.split_f32(x.cuda(), 3)[0]
                dO = ops.split_f32(dy.cuda(), 3)[0]
                fwd = lambda: ops.divided_attn_fwd(qkv, B, T, n, H, 0, 3)
                o, lse = fwd()
                bwd = lambda: ops.divided_attn_bwd(qkv, o, dO, lse, B, T, n, H, 0, 3)
                fl = floors(B, T, n, H, 2, 2, 2, 2)
            else:
                hi = x.to(torch.float16)
                qkv = ops.Planes(hi.cuda(), (x - hi.float()).to(torch.float16).cuda(), B * S, 3 * D, "f16s")
                dO = ops.f16_cast(dy.cuda())
                fwd = lambda: ops.divided_attn_fwd(qkv, B, T, n, H, 0, 3, out_fmt="f16x2")
                o, lse = fwd()
                bwd = lambda: ops.divided_attn_bwd(qkv, o, dO, lse, B, T, n, H, 0, 1, grad_f16=True)
                f3 = floors(B, T, n, H, 2, 2, 1, 1)
                f1 = floors(B, T, n, H, 1, 1, 1, 1)          # the backward reads the hi plane of qkv and the first plane of O
                fl = (f3[0], f1[1], f1[2])
            t_f, t_b = events(fwd), events(bwd)
            t_dq, t_dkv = kernel_split(bwd)
            row = {"fwd_us": round(t_f, 1), "bwd_us": round(t_b, 1), "dq_us": round(t_dq, 1), "dkv_us": round(t_dkv, 1)}
            for key, t, byt in (("fwd", t_f, fl[0]), ("dq", t_dq, fl[1]), ("dkv", t_dkv, fl[2])):
                row[key + "_floor_MB"] = round(byt / 1e6, 1)
                row[key + "_TBps"] = round(byt / t / 1e6, 3)          # bytes / us = MB/s; / 1e6 -> TB/s
            res[mode] = row
            del qkv, dO, o, lse
            torch.cuda.empty_cache()
        out["shapes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
