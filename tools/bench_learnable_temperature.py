"""What the gradient of the learnable logit scale adds to a call of the contrastive head, on one GPU:

    python tools/bench_learnable_temperature.py [--iters 200] [--warmup 20] [--rounds 5]

The short head at n = 256 and the long head at n = 4 096 (D = 256, 582 nouns / 118 verbs, temperature 0.05, the inputs of
tools/bench_egonce_long.py, whose `long_us` / `short_us` the fixed-temperature figures here can be compared with), each as the
fixed-temperature call (egv_egonce_fwd_bwd / egv_egonce_long_fwd_bwd) and as the learnable one (the *_ls entry points: 1 / tau =
exp(s) read on the device, d_logit_scale next to the embedding gradients).  The two variants ALTERNATE round by round in the same
process; a round times `--iters` back-to-back calls between two HIP events and reports the time per call.  Reported: the median
over the rounds, the spread (min .. max) of each variant, and learnable / fixed.

What the learnable call adds: one FMA per element of a matrix the gradient kernels already walk, a workgroup reduction per row
(short) or per workgroup (long), and one single-workgroup launch.  One JSON line."""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--short-n", type=int, default=256)
    ap.add_argument("--long-n", type=int, default=4096)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_learnable_temperature: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import loss_ops

    def per_call_us(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    D = 256
    scale = torch.tensor([math.log(1.0 / 0.05)], dtype=torch.float32, device="cuda")
    out = {"D": D, "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "heads": {}}
    for name, n, call, iters in (("short", args.short_n, loss_ops.egonce_fwd_bwd, args.iters),
                                 ("long", args.long_n, loss_ops.egonce_long_fwd_bwd, max(args.iters // 4, 1))):
        g = torch.Generator().manual_seed(n)
        text, video = torch.randn(n, D, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
        noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
        noun[:, :8] = (torch.rand(n, 8, generator=g) < 0.19).float()
        verb[:, :4] = (torch.rand(n, 4, generator=g) < 0.25).float()
        noun, verb = noun.cuda(), verb.cuda()
        fixed = lambda: call(text, video, noun, verb, 0.05)
        learn = lambda: call(text, video, noun, verb, None, logit_scale=scale)
        for _ in range(args.warmup):
            fixed()
            learn()
        torch.cuda.synchronize()
        tf, tl = [], []
        for _ in range(args.rounds):                    # alternate: what else runs on the host hits both alike
            tf.append(per_call_us(fixed, iters))
            tl.append(per_call_us(learn, iters))
        lf, ll = fixed(), learn()
        row = {"n": n, "calls_per_round": iters,
               "fixed_us": round(statistics.median(tf), 2), "fixed_min_max_us": [round(min(tf), 2), round(max(tf), 2)],
               "learnable_us": round(statistics.median(tl), 2), "learnable_min_max_us": [round(min(tl), 2), round(max(tl), 2)],
               "learnable_over_fixed": round(statistics.median(tl) / statistics.median(tf), 4),
               "loss_fixed": float(lf[0]), "loss_learnable": float(ll[0]), "d_logit_scale": float(ll[-1])}
        out["heads"][name] = row
        del text, video, noun, verb
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
