"""What the EgoNCE head with a queue of past embeddings costs per call, on one GPU:

    python tools/bench_egonce_queue.py [--batches 256,1024] [--queues 4096,16384,65536] [--rounds 5] [--window-ms 150]

At every (n, Q) (D = 256, 582 nouns / 118 verbs, temperature 0.05, the queue FULL) three calls are timed in one process:
  queue   egv_egonce_queue_fwd_bwd on n batch rows against the Q queued rows (loss and both gradients); `queue_push_us` is the same
          call followed by egv_egonce_queue_push, which is what a training step pays;
  long    egv_egonce_long_fwd_bwd on n + Q rows -- the only way to see these columns without a queue (rows capped at the long head's
          65 536: at Q = 65 536 it runs on FEWER rows than n + Q, which favours it; `long_rows` says how many);
  plain   the head a queue-less step runs on its n rows (egv_egonce_fwd_bwd up to 1 024 rows): what the queue adds to a step.
The variants ALTERNATE round by round; a round times back-to-back calls between two HIP events over a window of about --window-ms
(the call count comes from one timed call after the warm-up) and reports the time per call.  Reported: the median over the rounds
and the spread of each variant, `queue_over_long` next to the pair-count expectation 2 n / (n + Q) (arithmetic, not a measurement:
the queue head forms 2 n (n + Q) similarity pairs where the long head forms (n + Q)^2), and `queue_over_plain`.  One JSON line."""
import argparse
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--queues", default="4096,16384,65536")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=150.0)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_egonce_queue: needs an MI355X (there is no CPU measurement path)")
    from egovlp_amd import loss_ops

    def per_call_us(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    def calls_for(fn):
        "two warm-up calls, then as many calls as fill the window (2 .. 1000)"
        fn()
        fn()
        torch.cuda.synchronize()
        return max(2, min(1000, int(args.window_ms * 1e3 / per_call_us(fn, 1))))

    def rows(n, seed):
        g = torch.Generator().manual_seed(seed)
        text, video = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
        # 0-3 of the first 8 nouns and 0-2 of the first 4 verbs per row, as in the tests
        noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
        noun[:, :8] = (torch.rand(n, 8, generator=g) < 0.19).float()
        verb[:, :4] = (torch.rand(n, 4, generator=g) < 0.25).float()
        return [t.cuda() for t in (text, video, noun, verb)]

    D = 256
    out = {"D": D, "rounds": args.rounds, "window_ms": args.window_ms, "sizes": []}
    for Q in [int(x) for x in args.queues.split(",")]:
        queued = rows(Q, Q)
        queue = loss_ops.EgonceQueue(Q, D, 582, 118, "cuda")
        step = min(Q, 1024)
        for lo in range(0, Q, step):                    # fill the ring through the product's own calls
            block = [t[lo:lo + step] for t in queued]
            loss, _, _, work = loss_ops.egonce_queue_fwd_bwd(*block, 0.05, queue, want_grads=False)
            loss_ops.egonce_queue_push(work, loss, block[0].shape[0], queue)
        assert queue.filled() == Q
        for n in [int(x) for x in args.batches.split(",")]:
            if n > Q:
                continue
            batch = rows(n, n + Q)
            long_rows = min(n + Q, loss_ops.EGONCE_LONG_MAX)
            both = [torch.cat([b, q])[:long_rows].contiguous() for b, q in zip(batch, queued)]
            state = queue.state.clone()

            def with_push():
                loss, _, _, work = loss_ops.egonce_queue_fwd_bwd(*batch, 0.05, queue)
                loss_ops.egonce_queue_push(work, loss, n, queue)
            fns = {"queue": lambda: loss_ops.egonce_queue_fwd_bwd(*batch, 0.05, queue),
                   "queue_push": with_push,
                   "long": lambda: loss_ops.egonce_long_fwd_bwd(*both, 0.05),
                   "plain": lambda: loss_ops.egonce_fwd_bwd(*batch, 0.05)}
            losses = {"loss_queue": float(fns["queue"]()[0]), "loss_plain": float(fns["plain"]()[0])}
            iters = {k: calls_for(fn) for k, fn in fns.items()}
            ts = {k: [] for k in fns}
            for _ in range(args.rounds):                # alternate: what else runs on the host hits all alike
                for k, fn in fns.items():
                    ts[k].append(per_call_us(fn, iters[k]))
            # the pushes overwrote slots with copies of the batch (no timing depends on what a slot holds); head goes back, so that
            # every n starts at the same place
            queue.state.copy_(state)
            torch.cuda.synchronize()
            med = {k: statistics.median(v) for k, v in ts.items()}
            row = {"n": n, "Q": Q, "long_rows": long_rows, "calls_per_round": iters}
            for k in fns:
                row[k + "_us"] = round(med[k], 2)
                row[k + "_min_max_us"] = [round(min(ts[k]), 2), round(max(ts[k]), 2)]
            row["queue_over_long"] = round(med["queue"] / med["long"], 4)
            row["pairs_expectation"] = round(2.0 * n / (n + Q), 4)
            row["queue_over_plain"] = round(med["queue"] / med["plain"], 2)
            row.update(losses)
            out["sizes"].append(row)
            del batch, both
        del queued, queue
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main()
