"""What patch dropout in the video tower buys on one GPU:

    python tools/bench_patch_drop.py [--batch 32] [--frames 4] [--rates 0,0.25,0.5,0.75] [--steps 6] [--rounds 3]

In ONE process, alternating round by round (legs measured minutes apart do not compare), at bench.py's headline shape and setup: the
whole step `egoclip_step` of ONE model whose rate is set per leg (`set_patch_drop_rate`), in the benchmarked 'f16mix' / 'f16' mode and
in 'bf16x3' / 'bf16'.  Every leg's shapes are warmed up first; the device is synchronised on both sides of a leg.  At rate r the video
tower runs 1 + T * K token rows per clip, K = max(1, int(n * (1 - r))), instead of 1 + T * n: `rows_ratio` is that arithmetic,
`ms_ratio` what the step does.  The text tower, the loss head and the optimizer do not shrink.

The three gathers are also timed alone (device events, median of --gather-reps launches) at rate 0 (the full gather) and at 0.5 (the
*_sel gather over half the patches, which reads one patch-row segment per thread group instead of a stretch of a whole image row): us,
bytes moved (source bytes read + plane bytes written) and GB/s.  One JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(precision, text_dropout):
    sys.path.insert(0, HERE)
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.synth import synth_state_dict
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16, "pretrained": True,
                                   "time_init": "rand", "patch_drop_rate": 0.0},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"}, projection="minimal",
                     load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0))
    m.text_model.set_dropout(text_dropout, text_dropout)
    m = m.cuda().train()
    m.exec_ctx.set_precision(*precision)
    m.exec_ctx.set(gemm_grid=256, wgrad_side_stream=True, text_side_stream=True)
    return m


def timed(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def gather_timings(torch, B, T, reps):
    """us / bytes / GB/s of the three gathers alone, full (rate 0) and over half the patches (rate 0.5), three-product planes."""
    from egovlp_amd import ops
    P, R, n = 16, 224, 196
    K = max(1, int(n * 0.5))
    g = torch.Generator().manual_seed(0)
    f32 = torch.randn(B, T, 3, R, R, generator=g).cuda()
    u8 = torch.randint(0, 256, (B, T, 3, R, R), generator=g, dtype=torch.uint8).cuda()
    src = torch.randint(0, 256, (B, T, 3, 256, 341), generator=g, dtype=torch.uint8).cuda()      # the ego4d_256 frames
    boxes = torch.tensor([[16, 40, 200, 260, b & 1] for b in range(B)], dtype=torch.int32).cuda()
    keep = ops.patch_keep_draw(B, n, K, 0x0123456789ABCDEF)
    cases = {"fp32": (f32, {}, 4), "uint8": (u8, {}, 1), "uint8_aug": (src, {"aug": (boxes, R)}, 1)}
    out = {}
    for name, (video, kw, elt) in cases.items():
        for tag, kp, per_frame in (("rate_0", None, n), ("rate_0.5", keep, K)):
            for _ in range(3):
                ops.patch_gather(video, P, 3, keep=kp, **kw)
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.patch_gather(video, P, 3, keep=kp, **kw)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            rows = B * T * per_frame
            # source bytes: the pixels of the gathered patches (the augmented gather reads up to four source bytes per output pixel out of
            # the crop box, counted once here: an estimate); planes: two bf16 planes of 768 columns
            nbytes = rows * 768 * elt + rows * 768 * 2 * 2
            med = statistics.median(us)
            out.setdefault(name, {})[tag] = {"us": round(med, 2), "rows": rows, "bytes": nbytes, "GBps": round(nbytes / med / 1e3, 1)}
        out[name]["us_ratio"] = round(out[name]["rate_0.5"]["us"] / out[name]["rate_0"]["us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rates", type=str, default="0,0.25,0.5,0.75")
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--text-dropout", type=float, default=0.1)
    ap.add_argument("--gather-reps", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_drop: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    rates = [float(r) for r in args.rates.split(",")]
    if rates[0] != 0.0:
        raise SystemExit("bench_patch_drop: the first rate is 0 (every ratio is to that leg)")
    h = synth_batch(args.batch, T=args.frames, L=32, seed=1234)
    dev = {"video": h["video"].cuda(), "text": {k: v.cuda() for k, v in h["text"].items()}, "noun_vec": h["noun_vec"].cuda(),
           "verb_vec": h["verb_vec"].cuda()}
    out = {"batch": args.batch, "frames": args.frames, "rates": rates, "rounds": args.rounds, "timed_steps_per_round": args.steps}
    loss_fn = EgoNCE()
    tags = ["rate_%g" % r for r in rates]
    for precision in (("f16mix", "f16"), ("bf16x3", "bf16")):
        m = build(precision, args.text_dropout)
        vm = m.video_model
        n = vm.patches_per_frame
        opt = AdamW(m.parameters(), lr=0.0)       # lr = 0: the weights stay where they are; the update kernels run all the same

        def leg(rate):
            vm.set_patch_drop_rate(rate)
            return lambda: egoclip_step(m, loss_fn, opt, dev)
        rows = {}
        for tag, rate in zip(tags, rates):        # every leg's shapes first: allocator pools, workspace sizes, weight planes
            fn = leg(rate)
            for _ in range(3):
                fn()
            rows[tag] = args.batch * (1 + args.frames * vm.patch_keep_count(n))
        times = {k: [] for k in tags}
        for _ in range(args.rounds):
            for tag, rate in zip(tags, rates):
                times[tag].append(timed(torch, leg(rate), args.steps))
        med = {k: statistics.median(v) * 1e3 for k, v in times.items()}
        out["/".join(precision)] = {"ms": {k: round(v, 3) for k, v in med.items()},
                                    "ms_rounds": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
                                    "token_rows": rows,
                                    "rows_ratio": {k: round(rows[k] / rows[tags[0]], 4) for k in tags},
                                    "ms_ratio": {k: round(med[k] / med[tags[0]], 4) for k in tags},
                                    "pairs_per_s": {k: round(args.batch / med[k] * 1e3, 1) for k in tags}}
        del m, opt, vm
        torch.cuda.empty_cache()
    out["gathers"] = gather_timings(torch, args.batch, args.frames, args.gather_reps)
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
