"""What gradient clipping by global norm costs on one GPU:

    python tools/bench_grad_clip.py [--batch 32] [--steps 6] [--rounds 3]                  (b) clipping on against off
    python tools/bench_grad_clip.py --against /path/to/a/built/checkout/of/the/parent      (a) clipping off against the parent commit

(b) In ONE process, alternating round by round (legs measured minutes apart do not compare), at bench.py's headline shape and setup:
the whole step `egoclip_step` and the optimizer alone (`optimizer.step` on the gradients the last backward left), each with
max_grad_norm off and on, in the benchmarked 'f16mix' / 'f16' mode (the model's loss scaler: the reduction rides on the scan) and in
'bf16x3' / 'bf16' (no scaler: the reduction is one more read of the gradients).  One JSON line: median ms per leg, all rounds.
(a) One child process per measurement, alternating parent, this tree, parent, ... (`rounds` times): the step rate with clipping off
of both trees and the optimizer alone (`optimizer.step` with the model's loss scaler, on the gradients the last backward left), and
the spread between the parent's own runs -- the difference between the trees means something only beyond it."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(root, precision, batch, frames, text_dropout):
    sys.path.insert(0, root)
    import torch
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.synth import synth_batch, synth_state_dict
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16, "pretrained": True,
                                   "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"}, projection="minimal",
                     load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0))
    m.text_model.set_dropout(text_dropout, text_dropout)
    m = m.cuda().train()
    ec = m.exec_ctx
    ec.set_precision(*precision)
    ec.set(gemm_grid=256, wgrad_side_stream=True, text_side_stream=True)
    h = synth_batch(batch, T=frames, L=32, seed=1234)
    dev = {"video": h["video"].cuda(), "text": {k: v.cuda() for k, v in h["text"].items()}, "noun_vec": h["noun_vec"].cuda(),
           "verb_vec": h["verb_vec"].cuda()}
    return torch, m, ec, dev


def timed(torch, fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def child(args):
    """One tree, clipping off, the benchmarked mode: ms per step and per optimizer step alone (medians of `rounds` windows of `steps`
    steps / 40 x `steps` optimizer steps: ~1 ms each, so that its window is no shorter)."""
    torch, m, ec, dev = build(args.root, ("f16mix", "f16"), args.batch, args.frames, args.text_dropout)
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    opt, loss_fn = AdamW(m.parameters(), lr=3e-5), EgoNCE()
    step = lambda: egoclip_step(m, loss_fn, opt, dev)
    for _ in range(3):
        step()
    ms = [timed(torch, step, args.steps) * 1e3 for _ in range(args.rounds)]
    scaler = ec.loss_scaler(device="cuda") if ec.bwd_passes == 4 else None
    opt_step = (lambda: opt.step(scaler=scaler)) if scaler is not None else opt.step
    opt_ms = [timed(torch, opt_step, 40 * args.steps) * 1e3 for _ in range(args.rounds)]
    print(json.dumps({"root": args.root, "ms": round(statistics.median(ms), 3), "ms_rounds": [round(x, 3) for x in ms],
                      "optimizer_ms": round(statistics.median(opt_ms), 4), "optimizer_ms_rounds": [round(x, 4) for x in opt_ms]}))


def against(args):
    runs = {"parent": [], "this": []}
    opt = {"parent": [], "this": []}
    order = (["parent", "this"] * args.rounds) + ["parent"]
    for who in order:
        root = args.against if who == "parent" else HERE
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--batch", str(args.batch), "--frames",
                              str(args.frames), "--steps", str(args.steps), "--rounds", str(args.rounds), "--text-dropout",
                              str(args.text_dropout)], check=True, capture_output=True, text=True, timeout=600).stdout
        line = json.loads(out.strip().splitlines()[-1])
        runs[who].append(line["ms"])
        opt[who].append(line["optimizer_ms"])
    p, t = runs["parent"], runs["this"]
    print(json.dumps({"batch": args.batch, "frames": args.frames, "precision": "f16mix/f16", "order": order, "parent_ms": p, "this_off_ms": t,
                      "parent_spread_ms": round(max(p) - min(p), 3), "this_minus_parent_ms": round(statistics.median(t) - statistics.median(p), 3),
                      "parent_optimizer_ms": opt["parent"], "this_optimizer_ms": opt["this"],
                      "parent_optimizer_spread_ms": round(max(opt["parent"]) - min(opt["parent"]), 4),
                      "this_minus_parent_optimizer_ms": round(statistics.median(opt["this"]) - statistics.median(opt["parent"]), 4),
                      "parent_clip_pairs_per_s": round(args.batch / statistics.median(p) * 1e3, 2),
                      "this_off_clip_pairs_per_s": round(args.batch / statistics.median(t) * 1e3, 2)}))


def on_off(args):
    out = {"batch": args.batch, "frames": args.frames, "rounds": args.rounds, "timed_calls_per_round": args.steps, "max_grad_norm": args.max_grad_norm}
    for precision in (("f16mix", "f16"), ("bf16x3", "bf16")):
        torch, m, ec, dev = build(HERE, precision, args.batch, args.frames, args.text_dropout)
        from egovlp_amd.model.loss import EgoNCE
        from egovlp_amd.optim import AdamW
        from egovlp_amd.trainer.trainer_egoclip import egoclip_step
        loss_fn = EgoNCE()
        # lr = 0: the four legs share one model and the weights stay where they are; the update kernels run all the same
        opts = {"off": AdamW(m.parameters(), lr=0.0), "on": AdamW(m.parameters(), lr=0.0, max_grad_norm=args.max_grad_norm)}
        scaler = ec.loss_scaler(device="cuda") if ec.bwd_passes == 4 else None
        legs = {}
        for k, opt in opts.items():
            legs["step_" + k] = lambda opt=opt: egoclip_step(m, loss_fn, opt, dev)
            legs["optimizer_" + k] = (lambda opt=opt: opt.step(scaler=scaler)) if scaler is not None else (lambda opt=opt: opt.step())
        for fn in legs.values():
            for _ in range(2):
                fn()
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(timed(torch, fn, args.steps if k.startswith("step") else 4 * args.steps))
        tag = "/".join(precision)
        out[tag] = {"ms": {k: round(statistics.median(v) * 1e3, 3) for k, v in times.items()},
                    "ms_rounds": {k: [round(x * 1e3, 3) for x in v] for k, v in times.items()},
                    "scaler": scaler is not None, "last_grad_norm": opts["on"].grad_norm(), "last_clip_coef": opts["on"].clip_coef(),
                    "clipped_steps": opts["on"].clipped_steps(), "nonfinite_steps": opts["on"].nonfinite_steps()}
        del m, opts, legs
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg and round (the optimizer-only legs run 4 x as many)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--text-dropout", type=float, default=0.1)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--against", default="", help="a built checkout of the parent commit: measure clipping OFF against it")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.against:
        return against(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip: needs an MI355X (there is no CPU measurement path)")
    on_off(args)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
