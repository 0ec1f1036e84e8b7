"""What the embedding-cache step costs on one GPU: python tools/bench_cached_step.py [--batch 32] [--chunks 4] [--steps 6] [--rounds 3]

In ONE process, alternating round by round (the box's clock and its neighbours drift: legs measured minutes apart do not compare):
  (a) the plain step, `egoclip_step`, at B = batch                    -- bench.py's flagship figure
  (b) one train-mode forward under no_grad at B = batch               -- what pass 1 adds per chunk
  (c) the cached step, `egoclip_step_cached`, at B = chunks x batch, chunk = batch
and prints one JSON line: clip-pairs/s of each (median over the rounds), the model `chunks x batch / (chunks x (t_a + t_b))` next to
(c), and peak memory of (a) and (c).  The model setup (synthetic weights, text dropout 0.1, 'f16mix' forward with the fp16 backward,
wgrad and text side streams) is bench.py's."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egovlp_amd.model.loss import EgoNCE                       # noqa: E402
from egovlp_amd.model.model import FrozenInTime                # noqa: E402
from egovlp_amd.optim import AdamW                             # noqa: E402
from egovlp_amd.synth import synth_batch, synth_state_dict     # noqa: E402
from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32, help="rows of the plain step = rows per chunk of the cached step")
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6, help="timed repetitions per leg and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="f16mix")
    ap.add_argument("--text-dropout", type=float, default=0.1)
    ap.add_argument("--only", default="", help="diagnostics (profiler runs): time one leg only, 'a', 'b' or 'c'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cached_step: needs an MI355X (there is no CPU measurement path)")
    b, K, T = args.batch, args.chunks, args.frames
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16, "pretrained": True,
                                   "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"}, projection="minimal",
                     load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0))
    m.text_model.set_dropout(args.text_dropout, args.text_dropout)
    m = m.cuda().train()
    ec = m.exec_ctx
    if args.precision == "mixed":
        ec.set_precision("bf16x3", "bf16")
    else:
        ec.set_precision(args.precision)
    ec.set(gemm_grid=256, wgrad_side_stream=True, text_side_stream=True)
    opt = AdamW(m.parameters(), lr=3e-5)
    loss_fn = EgoNCE()

    def dev(n, seed):
        h = synth_batch(n, T=T, L=32, seed=seed)
        return {"video": h["video"].cuda(), "text": {k: v.cuda() for k, v in h["text"].items()}, "noun_vec": h["noun_vec"].cuda(),
                "verb_vec": h["verb_vec"].cuda()}
    small, big = dev(b, 1234), dev(K * b, 4321)

    def leg_a():
        egoclip_step(m, loss_fn, opt, small)

    def leg_b():
        with torch.no_grad(), ec.train_kernels_without_grad():
            m(small)

    def leg_c():
        egoclip_step_cached(m, loss_fn, opt, big, b)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    if args.only:
        legs = {args.only: legs[args.only]}
    peak = {}
    for name, fn in legs.items():              # warm-up: every shape of the timed window, and the peak memory of each leg on its own
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
    times = {name: [] for name in legs}
    reps = {name: (args.steps if name != "c" else max(2, args.steps // 2)) for name in legs}     # a (c) step is `chunks` steps of work
    for _ in range(args.rounds):
        for name, fn in legs.items():
            times[name].append(timed(fn, reps[name]))
    t = {name: statistics.median(v) for name, v in times.items()}
    out = {"batch": b, "chunks": K, "frames": T, "precision": "/".join(ec.precision_name()), "rounds": args.rounds,
           "timed_calls_per_round": reps,
           "ms": {k: round(v * 1e3, 3) for k, v in t.items()}, "ms_rounds": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
           "peak_alloc_GB": {k: round(v / 2 ** 30, 3) for k, v in peak.items()}}
    if "a" in t:
        out["plain_step_clip_pairs_per_s"] = round(b / t["a"], 2)
    if "b" in t:
        out["nograd_train_forward_clip_pairs_per_s"] = round(b / t["b"], 2)
    if "c" in t:
        out["cached_step_clip_pairs_per_s"] = round(K * b / t["c"], 2)
    if len(t) == 3:
        model = K * b / (K * (t["a"] + t["b"]))
        out["model_clip_pairs_per_s"] = round(model, 2)
        out["cached_vs_model"] = round((K * b / t["c"]) / model, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
