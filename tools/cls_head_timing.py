"""Time the classification head of the OSCC / PNR fine-tunes at the configs' local batch: from the video tower's features [4, 768]
to the loss, dfeats, dW and db at world size 1, for C = 2 (OSCC) and C = 16 (PNR, with the mean(state) weighting).

    python tools/cls_head_timing.py [--reps 200] [--step-reps 20] [--out profiles/cls_head_timing.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/cls_head_timing.py --count fused|padded --classes 2 --iters N

Two routes, interleaved repetition by repetition in one process after a warm-up:
  padded  the projection node of model(data, video_only=True) (_ProjFn: output width padded to 32 for the MFMA GEMMs) + CrossEntropy
          + their backward -- the route of `classification_step(fused_head=False)`;
  fused   CrossEntropy.fused: egv_cls_head_fwd, egv_cls_head_loss_bwd on one autograd node.
Each repetition is timed by a pair of HIP events around forward + backward (the device is idle-waited before, so this is the
latency of the tail behind a step: launch overheads included, which is what the tail consists of).  Medians, 10th and 90th
percentiles.  The whole step (`classification_step`, B = 4, T = 16, f16mix / f16 as bench.py runs) is timed the same way.
`--count` runs `--iters` repetitions of one route and nothing else, for a profiler run that counts its launches: two runs with
different --iters give the launches per repetition as a difference (set-up launches cancel)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def routes(C):
    from egovlp_amd import ops
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.model.model import _ProjFn
    g = torch.Generator().manual_seed(C)
    feats = torch.randn(4, 768, generator=g).cuda().requires_grad_(True)
    W = (torch.randn(C, 768, generator=g) / 768 ** 0.5).cuda().requires_grad_(True)
    b = torch.zeros(C).cuda().requires_grad_(True)
    target = torch.randint(0, C, (4,), generator=g).cuda()
    state = torch.tensor([1, 0, 1, 1]).cuda() if C > 2 else None
    ce, ec = CrossEntropy(), ops.new_context()

    def padded():
        feats.grad = W.grad = b.grad = None
        ec.begin_step()
        loss = ce(_ProjFn.apply(feats, W, b, False, ec), target)
        if state is not None:
            loss = torch.mean(state * loss)
        loss.backward()
        ec.join_side_stream()
        return loss

    def fused():
        feats.grad = W.grad = b.grad = None
        loss = ce.fused(feats, W, b, target, state, 1, 0, ec)
        loss.backward()
        return loss
    return {"padded": padded, "fused": fused}, (feats, W, b)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[(9 * len(v)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--count", default=None, choices=["fused", "padded"])
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_head_timing needs an MI355X: no HIP device is visible")
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    if a.count:
        fn = routes(a.classes)[0][a.count]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    lines = ["classification head, features [4, 768] -> loss, dfeats, dW, db, world size 1, %s" % torch.cuda.get_device_name(0),
             "HIP events around one forward + backward on an idle device, %d repetitions per route, routes interleaved" % a.reps,
             "%4s  %-7s  %30s" % ("C", "route", "us: median (p10 .. p90)")]
    for C in (2, 16):
        fns, (feats, W, b) = routes(C)
        for _ in range(30):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        grads = {}
        for k, fn in fns.items():
            grads[k] = (float(fn().detach()), feats.grad.clone(), W.grad.clone(), b.grad.clone())
        la, lb = grads["fused"][0], grads["padded"][0]
        assert abs(la - lb) < 1e-4 * abs(lb), (la, lb)
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        med = {}
        for k in ("padded", "fused"):
            med[k], lo, hi = stats(t[k])
            lines.append("%4d  %-7s  %12.1f (%.1f .. %.1f)" % (C, k, med[k], lo, hi))
        lines.append("%4s  fused is %.1f us (%.0f %%) below padded; loss fused %.8f, padded %.8f" % (
            "", med["padded"] - med["fused"], 100.0 * (med["padded"] - med["fused"]) / med["padded"], la, lb))
    # the whole step
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.trainer.trainer_oscc import classification_step
    Precision.set("f16mix", "f16")
    lines.append("whole step: classification_step, B = 4, T = 16, ViT-B/16, f16mix / f16, %d repetitions per route, interleaved" % a.step_reps)
    for task, C in (("oscc", 2), ("pnr", 16)):
        m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16,
                                       "pretrained": True, "time_init": "rand"},
                         text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                         projection="minimal", projection_dim=C, load_checkpoint="")
        m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=21))
        m = m.cuda().train()
        opt = AdamW(m.parameters(), lr=1e-6)
        g = torch.Generator().manual_seed(5)
        data = {"video": torch.randn(4, 16, 3, 224, 224, generator=g).cuda(), "state": torch.tensor([1, 0, 1, 1]).cuda()}
        if task == "pnr":
            lab = torch.zeros(4, 16, dtype=torch.long)
            lab[torch.arange(4), torch.tensor([3, 0, 9, 15])] = 1
            lab[1] = 0
            data["labels"] = lab.cuda()
        fns = {"padded": lambda: classification_step(m, CrossEntropy(), opt, data, task=task, fused_head=False),
               "fused": lambda: classification_step(m, CrossEntropy(), opt, data, task=task, fused_head=True)}
        for _ in range(3):
            for fn in fns.values():
                fn()
        t = {k: [] for k in fns}
        for _ in range(a.step_reps):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        med = {}
        for k in ("padded", "fused"):
            med[k], lo, hi = stats(t[k])
            lines.append("%4s  %-7s  %12.1f (%.1f .. %.1f)" % (task, k, med[k], lo, hi))
        spread = max(stats(t["padded"])[2] - stats(t["padded"])[1], stats(t["fused"])[2] - stats(t["fused"])[1])
        lines.append("%4s  difference of the medians %.1f us; p10 .. p90 spread of a route %.1f us: %s" % (
            "", med["padded"] - med["fused"], spread,
            "inside the run-to-run spread" if abs(med["padded"] - med["fused"]) < spread else "outside the run-to-run spread"))
        del m, opt
        torch.cuda.empty_cache()
    Precision.set("bf16x3")
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
