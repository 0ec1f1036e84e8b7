"""What stochastic depth in the video tower costs on one GPU:

    python tools/bench_drop_path.py [--batch 32] [--frames 4] [--rate 0.1] [--steps 6] [--rounds 3]

In ONE process, alternating round by round (legs measured minutes apart do not compare), at bench.py's headline shape and setup: the
whole step `egoclip_step` of two models with the same weights, one built with drop_path_rate 0 and one with `--rate`, in the
benchmarked 'f16mix' / 'f16' mode and in 'bf16x3' / 'bf16'.  At rate 0 every block runs the C block calls; at a rate > 0 the eleven
blocks with p > 0 run the per-kernel path with two egv_drop_path_add passes in the forward and two egv_drop_path_grad passes in place
of two format passes in the backward -- the difference between the legs is the cost of both.  One JSON line: median ms per leg, all
rounds, and the difference."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(precision, rate, text_dropout):
    sys.path.insert(0, HERE)
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.synth import synth_state_dict
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16, "pretrained": True,
                                   "time_init": "rand", "drop_path_rate": rate},
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--text-dropout", type=float, default=0.1)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_path: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    h = synth_batch(args.batch, T=args.frames, L=32, seed=1234)
    dev = {"video": h["video"].cuda(), "text": {k: v.cuda() for k, v in h["text"].items()}, "noun_vec": h["noun_vec"].cuda(),
           "verb_vec": h["verb_vec"].cuda()}
    out = {"batch": args.batch, "frames": args.frames, "rate": args.rate, "rounds": args.rounds, "timed_steps_per_round": args.steps}
    loss_fn = EgoNCE()
    for precision in (("f16mix", "f16"), ("bf16x3", "bf16")):
        legs = {}
        for tag, rate in (("rate_0", 0.0), ("rate_on", args.rate)):
            m = build(precision, rate, args.text_dropout)
            opt = AdamW(m.parameters(), lr=0.0)       # lr = 0: the weights stay where they are; the update kernels run all the same
            legs[tag] = lambda m=m, opt=opt: egoclip_step(m, loss_fn, opt, dev)
        for fn in legs.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(torch, fn, args.steps))
        med = {k: statistics.median(v) * 1e3 for k, v in times.items()}
        out["/".join(precision)] = {"ms": {k: round(v, 3) for k, v in med.items()},
                                    "ms_rounds": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
                                    "cost_ms": round(med["rate_on"] - med["rate_0"], 3),
                                    "cost_percent": round(100.0 * (med["rate_on"] - med["rate_0"]) / med["rate_0"], 2)}
        del legs, m, opt
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
