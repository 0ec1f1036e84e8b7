"""What the EgoNCE head costs per call past the short head's 1 024 rows, on one GPU:

    python tools/bench_egonce_long.py [--sizes 1024,2048,4096,8192,16384] [--iters 10] [--warmup 3]

At every n (D = 256, 582 nouns / 118 verbs, temperature 0.05) the long head (egv_egonce_long_fwd_bwd: loss and both gradients) is
timed with HIP events over `--iters` calls after `--warmup`; at n = 1 024 the short head (egv_egonce_fwd_bwd) next to it, and up to
n = 4 096 the reference's decomposition (egoclip_head_loss(..., fused_head=False) forward AND backward: three sim_matrix calls,
egv_egonce_from_sim, the sim_matrix backward -- the route every n > 1 024 took before the long head).

The floor: the long head forms the n x n x D similarity product six times (two statistics walks, two gradient walks that recompute it
and each multiply G by the other side's rows), 6 . 2 n^2 D FLOP, on the fp32-input MFMA whose peak is 155 TFLOP/s on an MI355X
(64 FLOP / clk / SIMD x 4 SIMD x 256 CU x 2.4 GHz); `floor_frac` is that time over the measured one.  One JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_F32_MFMA = 155e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048,4096,8192,16384")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_egonce_long: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import loss_ops
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.trainer.common import egoclip_head_loss

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

    D = 256
    out = {"D": D, "iters": args.iters, "warmup": args.warmup, "peak_f32_mfma_TFLOPs": PEAK_F32_MFMA / 1e12, "sizes": {}}
    for n in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(n)
        text, video = torch.randn(n, D, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
        # 0-3 of the first 8 nouns and 0-2 of the first 4 verbs per row, as in the tests
        noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
        noun[:, :8] = (torch.rand(n, 8, generator=g) < 0.19).float()
        verb[:, :4] = (torch.rand(n, 4, generator=g) < 0.25).float()
        noun, verb = noun.cuda(), verb.cuda()
        row = {}
        t_long = events(lambda: loss_ops.egonce_long_fwd_bwd(text, video, noun, verb, 0.05))
        flop = 6.0 * 2.0 * n * n * D
        row["long_us"] = round(t_long, 1)
        row["floor_us"] = round(flop / PEAK_F32_MFMA * 1e6, 1)
        row["floor_frac"] = round(flop / PEAK_F32_MFMA * 1e6 / t_long, 3)
        row["loss"] = float(loss_ops.egonce_long_fwd_bwd(text, video, noun, verb, 0.05)[0])
        if n <= loss_ops.EGONCE_SHORT_MAX:
            row["short_us"] = round(events(lambda: loss_ops.egonce_fwd_bwd(text, video, noun, verb, 0.05)), 1)
        if n <= 4096:
            loss_fn = EgoNCE()

            def decomposed():
                tc, vc = text.detach().requires_grad_(True), video.detach().requires_grad_(True)
                egoclip_head_loss(loss_fn, tc, vc, noun, verb, fused_head=False).backward()
            row["decomposed_us"] = round(events(decomposed), 1)
            row["decomposed_over_long"] = round(row["decomposed_us"] / t_long, 2)
        out["sizes"][str(n)] = row
        del text, video, noun, verb
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
