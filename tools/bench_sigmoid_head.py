"""The pairwise sigmoid head against the EgoNCE head with a learnable temperature, on one GPU and the same inputs:

    python tools/bench_sigmoid_head.py [--iters 200] [--warmup 10] [--rounds 5] [--sizes 256,1024,4096,16384]

n = 256, 1 024, 4 096 and 16 384 rows of D = 256 (582 nouns / 118 verbs, the inputs of tools/bench_learnable_temperature.py).  Per
size: `loss_ops.sigmoid_head_fwd_bwd` (s = ln 10, b = -10: loss, both embedding gradients, d_scale, d_bias; ONE tile walk per direction at
every n) and `loss_ops.egonce_fwd_bwd` with `logit_scale` (up to 1 024 rows the SHORT head of csrc/egonce.hip, latency-sized kernels over an
n x n buffer; past it the LONG head of csrc/egonce_long.hip, which walks the tile grid for statistics and again for gradients), and
the sigmoid head's loss-only call.  The variants ALTERNATE round by round in the same process; a round times back-to-back calls
between two HIP events and reports the time per call.  Reported: the median over the rounds, the spread (min .. max) of each variant,
and sigmoid / EgoNCE.  Up to 4 096 rows the head's five outputs are also compared with the from-sim path (`EgoSigmoidLoss.forward`
on materialised similarity matrices: other kernels, the same loss), so the sizes that are timed are sizes that are checked.  One
JSON line."""
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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", type=str, default="256,1024,4096,16384")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sigmoid_head: needs an MI355X (there is no CPU measurement path)")
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
    temp_scale = torch.tensor([math.log(1.0 / 0.05)], dtype=torch.float32, device="cuda")
    s = torch.tensor([math.log(10.0)], dtype=torch.float32, device="cuda")
    b = torch.tensor([-10.0], dtype=torch.float32, device="cuda")
    out = {"D": D, "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds, "sizes": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        # the work grows with n^2: windows of 0.1 s and more (2 000 / 2 000 / 200 / 32 calls at the default sizes and --iters)
        iters = max(32, min(10 * args.iters, args.iters * 4096 * 4096 // (n * n)))
        g = torch.Generator().manual_seed(n)
        text, video = torch.randn(n, D, generator=g).cuda(), torch.randn(n, D, generator=g).cuda()
        noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
        noun[:, :8] = (torch.rand(n, 8, generator=g) < 0.19).float()
        verb[:, :4] = (torch.rand(n, 4, generator=g) < 0.25).float()
        noun, verb = noun.cuda(), verb.cuda()
        sig = lambda: loss_ops.sigmoid_head_fwd_bwd(text, video, noun, verb, s, b)
        sig_loss = lambda: loss_ops.sigmoid_head_fwd_bwd(text, video, noun, verb, s, b, want_grads=False)
        ego = lambda: loss_ops.egonce_fwd_bwd(text, video, noun, verb, None, logit_scale=temp_scale)
        for _ in range(min(args.warmup, iters)):
            sig()
            sig_loss()
            ego()
        torch.cuda.synchronize()
        ts, tl, te = [], [], []
        for _ in range(args.rounds):                    # alternate: what else runs on the host hits all alike
            ts.append(per_call_us(sig, iters))
            te.append(per_call_us(ego, iters))
            tl.append(per_call_us(sig_loss, iters))
        rs, re_ = sig(), ego()
        agree = None
        if n <= 4096:                                   # the element-wise path on a materialised similarity matrix: other kernels, same loss
            from egovlp_amd.model.loss import EgoSigmoidLoss
            from egovlp_amd.model.model import sim_matrix
            loss_fn = EgoSigmoidLoss().cuda()
            tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
            ref = loss_fn(sim_matrix(tc, vc), sim_matrix(verb, verb), sim_matrix(noun, noun))
            ref.backward()
            rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
            agree = {"loss": rel(rs[0], ref.detach().reshape(1)), "d_text": rel(rs[1], tc.grad), "d_video": rel(rs[2], vc.grad),
                     "d_scale": rel(rs[3], loss_fn.logit_scale.grad), "d_bias": rel(rs[4], loss_fn.logit_bias.grad)}
            agree = {k: float("%.2e" % v) for k, v in agree.items()}
            del loss_fn, tc, vc, ref
        med = statistics.median
        out["sizes"].append({
            "n": n, "calls_per_round": iters, "egonce_head": "short" if n <= loss_ops.EGONCE_SHORT_MAX else "long",
            "sigmoid_us": round(med(ts), 2), "sigmoid_min_max_us": [round(min(ts), 2), round(max(ts), 2)],
            "egonce_us": round(med(te), 2), "egonce_min_max_us": [round(min(te), 2), round(max(te), 2)],
            "sigmoid_over_egonce": round(med(ts) / med(te), 4),
            "sigmoid_loss_only_us": round(med(tl), 2), "sigmoid_loss_only_min_max_us": [round(min(tl), 2), round(max(tl), 2)],
            "loss_sigmoid": float(rs[0]), "d_scale": float(rs[3]), "d_bias": float(rs[4]), "loss_egonce": float(re_[0]),
            "rel_diff_to_from_sim_path": agree})
        del text, video, noun, verb
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
