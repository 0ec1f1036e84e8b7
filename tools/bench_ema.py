"""What the weight average (egovlp_amd/ema.py, csrc/ema.hip) costs on one GPU:

    python tools/bench_ema.py [--batch 32] [--steps 6] [--rounds 5]

In ONE process, the legs alternating round by round (legs measured minutes apart do not compare), at bench.py's headline shape and
setup, the benchmarked 'f16mix' / 'f16' mode:
  * the update pass alone over the model's real tensor list (egv_ema_update_multi, 12 B per parameter), `ModelEMA.update()` as the
    trainer calls it (decision + pass), and the AdamW pass alone (egv_adamw_multi without a scaler, 28 B per parameter) timed the same
    way in the same rounds: median ms, GB/s, and the update's GB/s as a share of the AdamW pass's;
  * `egoclip_step` with the average off and on;
  * `ModelEMA.swap()` (16 B per parameter).
One JSON line: median ms per leg, all rounds."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        raise SystemExit("bench_ema: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import ops
    from egovlp_amd.ema import ModelEMA
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.optim import AdamW
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
    # lr = 0: the legs share one model and the weights stay where they are; every kernel moves the bytes it always moves
    opt = AdamW(m.parameters(), lr=0.0)
    ema = ModelEMA(m, decay=0.9999, warmup=True)
    n_params = sum(p.numel() for p in ema._params)
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    state.view(torch.float32)[1] = 1e-4                       # the pass alone: a fixed non-zero weight, no decision kernel
    tables = [None]
    # the AdamW pass alone: the same tensor list (sizes, one allocation per tensor) on buffers of its own with finite gradients, so that
    # it needs no scaler and no scan and never touches the model
    twins = [torch.nn.Parameter(torch.zeros_like(p)) for p in ema._params]
    for q in twins:
        q.grad = torch.full_like(q, 1e-3)
    twin_opt = AdamW(twins, lr=0.0)

    def pass_only():
        tables[0] = ops.ema_update_multi(ema._views, ema._params, state, tables[0])

    def step_on():
        egoclip_step(m, loss_fn, opt, dev)
        ema.update(opt)

    def swap_twice():
        ema.swap()
        ema.swap()
    legs = {"step_off": lambda: egoclip_step(m, loss_fn, opt, dev), "step_on": step_on, "ema_pass": pass_only,
            "ema_update": lambda: ema.update(opt), "adamw_pass": lambda: twin_opt.step(), "swap_x2": swap_twice}
    for fn in legs.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(timed(torch, fn, args.steps if k.startswith("step") else 40 * args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    gbs = {"ema_pass": 12 * n_params / med["ema_pass"] / 1e9, "ema_update": 12 * n_params / med["ema_update"] / 1e9,
           "adamw_pass": 28 * n_params / med["adamw_pass"] / 1e9, "swap": 16 * n_params / (med["swap_x2"] / 2) / 1e9}
    print(json.dumps({
        "batch": args.batch, "frames": args.frames, "precision": "f16mix/f16", "rounds": args.rounds, "timed_calls_per_round": args.steps,
        "tensors": len(ema._params), "parameters": n_params, "arena_bytes": ema.arena_bytes(),
        "ms": {k: round(v * 1e3, 4) for k, v in med.items()}, "ms_rounds": {k: [round(x * 1e3, 4) for x in v] for k, v in times.items()},
        "swap_ms": round(med["swap_x2"] / 2 * 1e3, 4), "GBps": {k: round(v, 1) for k, v in gbs.items()},
        "ema_pass_share_of_adamw_bandwidth": round(gbs["ema_pass"] / gbs["adamw_pass"], 3),
        "step_on_minus_off_ms": round((med["step_on"] - med["step_off"]) * 1e3, 3),
        "ema_share_of_step": round((med["step_on"] - med["step_off"]) / med["step_off"], 4),
        "ema_update_share_of_step_off": round(med["ema_update"] / med["step_off"], 4),
        "num_updates": ema.num_updates(), "skipped_updates": ema.skipped_updates(), "decay_in_effect": ema.current_decay()}))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
