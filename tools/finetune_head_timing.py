"""Time the ranking-loss head of the retrieval fine-tunes: the one-call head (loss.fused -> egv_maxmargin_head_fwd_bwd) against
the three-call path it replaces in the step (sim_matrix -> loss -> backward: egv_sim_matrix_fwd, egv_maxmargin_fwd_bwd,
egv_sim_matrix_bwd with their autograd nodes), which is unchanged code.

    python tools/finetune_head_timing.py [--reps 200] [--rounds 5] [--sizes 32,256,1024] [--out profiles/finetune_head_timing.txt]

At n = 32, 256 and 1024 rows of D = 256 (MaxMarginRankingLoss, fix_norm), forward + backward down to the embedding gradients:
  device  time between two events around `reps` back-to-back iterations, per iteration (the stream never runs dry: the queue is
          primed before the first event); min / median over `rounds` rounds, the two paths alternating round by round;
  host    wall clock of enqueueing one iteration (no synchronisation inside the window; the device is idle-waited before).
Kernel times proper come from a profiler run of this tool at one size (`--sizes 1024` under rocprofv3 --kernel-trace --stats).
Also prints the C calls and kernel launches per iteration of each path (counted from the source: 3 kernels in one call vs
3 + memset + 1 + 2 in three calls) and checks that both paths return the same loss."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="32,256,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_head_timing needs an MI355X: no HIP device is visible")
    from egovlp_amd.model.loss import MaxMarginRankingLoss
    from egovlp_amd.model.model import sim_matrix
    loss_fn = MaxMarginRankingLoss()
    lines = ["ranking-loss head, forward + backward to the embedding gradients, D = 256, %s" % torch.cuda.get_device_name(0),
             "one call: 1 C call, 3 kernels, 1 autograd node;  three calls: 3 C calls, 6 kernels + 1 memset, 2 autograd nodes",
             "%6s  %-11s  %22s  %22s" % ("n", "path", "device us (min / med)", "host us (min / med)")]
    for n in [int(x) for x in a.sizes.split(",")]:
        g = torch.Generator().manual_seed(n)
        text = torch.randn(n, 256, generator=g)
        video = (0.25 * text + torch.randn(n, 256, generator=g)).cuda().requires_grad_(True)
        text = text.cuda().requires_grad_(True)

        def one_call():
            text.grad = video.grad = None
            loss = loss_fn.fused(text, video)
            loss.backward()
            return loss

        def three_calls():
            text.grad = video.grad = None
            loss = loss_fn(sim_matrix(text, video))
            loss.backward()
            return loss
        paths = (("one call", one_call), ("three calls", three_calls))
        for _, fn in paths:
            for _ in range(20):
                last = fn()
        torch.cuda.synchronize()
        la, lb = float(one_call().detach()), float(three_calls().detach())
        assert abs(la - lb) < 1e-5 * abs(lb), (la, lb)
        dev = {k: [] for k, _ in paths}
        host = {k: [] for k, _ in paths}
        for _ in range(a.rounds):
            for name, fn in paths:
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                dev[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
                hs = []
                for _ in range(30):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    hs.append((time.perf_counter() - t0) * 1e6)
                host[name].append(statistics.median(hs))
        for name, _ in paths:
            lines.append("%6d  %-11s  %10.1f / %9.1f  %10.1f / %9.1f" % (n, name, min(dev[name]), statistics.median(dev[name]),
                                                                        min(host[name]), statistics.median(host[name])))
        lines.append("%6s  loss one call %.8f, three calls %.8f" % ("", la, lb))
    lines.append("device = events around %d back-to-back iterations (when the host enqueues more slowly than the device runs, this is the "
                 "host's rate); host = enqueue of one iteration on an idle device" % a.reps)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
