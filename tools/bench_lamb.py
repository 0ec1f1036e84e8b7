"""What LAMB (egovlp_amd.optim.LAMB, csrc/lamb.hip) costs on one GPU, against AdamW in the same run:

    python tools/bench_lamb.py [--batch 32] [--steps 6] [--rounds 5]

In ONE process, the legs alternating round by round (legs measured minutes apart do not compare), at bench.py's headline shape and
setup, the benchmarked 'f16mix' / 'f16' mode:
  * over the model's real tensor list (327 tensors, 180.9 M parameters) on buffers of their own: the AdamW pass (egv_adamw_multi, 28 B
    per parameter), the LAMB pass (stage 1, ratio, stage 2: 40 B per parameter) and each of its three stages alone (24 B, ~0 B, 16 B
    per parameter): median ms, TB/s, and each as a share of the AdamW pass's bandwidth;
  * `egoclip_step` with AdamW, with LAMB, and with LAMB at its default max_grad_norm = 1 (the clip's norm replaces the plain scan).
The learning rates are 0 (AdamW) and 1e-30 (LAMB: at exactly 0 stage 2 would return without touching p): the legs share one model and
the weights stay where they are; every kernel moves the bytes it always moves.  One JSON line: median ms per leg, all rounds."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_LR = 1e-30


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
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg and round (the pass-only legs run 40 x as many)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--text-dropout", type=float, default=0.1)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lamb: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import ops
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.optim import LAMB, AdamW
    from egovlp_amd.synth import synth_batch, synth_state_dict
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16, "pretrained": True,
                                   "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"}, projection="minimal",
                     load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0))
    m.text_model.set_dropout(args.text_dropout, args.text_dropout)
    m = m.cuda().train()
    ec = m.exec_ctx
    ec.set_precision("f16mix", "f16")
    ec.set(gemm_grid=256, wgrad_side_stream=True, text_side_stream=True)
    h = synth_batch(args.batch, T=args.frames, L=32, seed=1234)
    dev = {"video": h["video"].cuda(), "text": {k: v.cuda() for k, v in h["text"].items()}, "noun_vec": h["noun_vec"].cuda(),
           "verb_vec": h["verb_vec"].cuda()}
    loss_fn = EgoNCE()
    params = [p for p in m.parameters() if p.requires_grad]
    n_params = sum(p.numel() for p in params)
    opts = {"step_adamw": AdamW(params, lr=0.0), "step_lamb": LAMB(params, lr=TINY_LR, max_grad_norm=None),
            "step_lamb_clip": LAMB(params, lr=TINY_LR)}
    # the passes alone: the same tensor list (sizes, one allocation per tensor) on buffers of their own with finite gradients, so that
    # they need no scaler and no scan and never touch the model
    twins = [torch.nn.Parameter(torch.full_like(p, 0.02)) for p in params]
    for q in twins:
        q.grad = torch.full_like(q, 1e-3)
    twin_adamw, twin_lamb = AdamW(twins, lr=0.0), LAMB(twins, lr=TINY_LR, max_grad_norm=None)
    twin_lamb.step()
    ms, vs = [twin_lamb.state[q]["exp_avg"] for q in twins], [twin_lamb.state[q]["exp_avg_sq"] for q in twins]
    gs = [q.grad for q in twins]
    tables = ops.lamb_tables(twins, ms, vs)
    partials, ratios = twin_lamb._lamb_partials, twin_lamb._lamb_ratios
    hp = (TINY_LR, 0.9, 0.999, 1e-6, 0.01, 2, True)
    legs = {k: (lambda o=o: egoclip_step(m, loss_fn, o, dev)) for k, o in opts.items()}
    legs.update({
        "adamw_pass": lambda: twin_adamw.step(), "lamb_pass": lambda: twin_lamb.step(),
        "lamb_stage1": lambda: ops.lamb_stage1_multi(twins, gs, ms, vs, *hp, 1.0, partials, tables=tables),
        "lamb_ratio": lambda: ops.lamb_ratio(twins, partials, ratios, True, False, tables=tables),
        "lamb_stage2": lambda: ops.lamb_stage2_multi(twins, ms, vs, *hp, ratios, tables=tables)})
    for fn in legs.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(torch, fn, args.steps if k.startswith("step") else 40 * args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    bytes_per = {"adamw_pass": 28, "lamb_pass": 40, "lamb_stage1": 24, "lamb_stage2": 16}
    tbs = {k: b * n_params / med[k] / 1e12 for k, b in bytes_per.items()}
    print(json.dumps({
        "batch": args.batch, "frames": args.frames, "precision": "f16mix/f16", "rounds": args.rounds, "timed_calls_per_round": args.steps,
        "tensors": len(params), "parameters": n_params, "pieces": tables[4],
        "ms": {k: round(v * 1e3, 4) for k, v in med.items()}, "ms_rounds": {k: [round(x * 1e3, 4) for x in v] for k, v in times.items()},
        "TBps": {k: round(v, 3) for k, v in tbs.items()},
        "share_of_adamw_bandwidth": {k: round(v / tbs["adamw_pass"], 3) for k, v in tbs.items()},
        "lamb_pass_over_adamw_pass": round(med["lamb_pass"] / med["adamw_pass"], 3),
        "step_lamb_minus_adamw_ms": round((med["step_lamb"] - med["step_adamw"]) * 1e3, 3),
        "step_lamb_clip_minus_adamw_ms": round((med["step_lamb_clip"] - med["step_adamw"]) * 1e3, 3),
        "step_lamb_over_adamw": round(med["step_lamb"] / med["step_adamw"], 4)}))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
