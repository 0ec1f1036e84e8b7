"""Time the Recall@K kernels and the chunked RecallEvaluator on one GPU.

    python tools/bench_recall.py [--sizes 3842x9668,16384x16384,8192x262144] [--eval 16384,65536] [--out FILE]

Part 1, per matrix size (a random fp32 matrix that already lives in HBM; HIP events, median of 10 calls after 3):
  egv_gt_ranks (t2v form, row form) and egv_topk_rows (k = 10), with the fraction of 5 TB/s each reaches counted as ONE read of
  the matrix; the same ranks as the torch expression (s > g).sum(1) on the device; tests/recall_ref.py on the host, once
  (skipped above --host-limit elements).
Part 2, per gallery size n (n captions against n videos, D = 256): RecallEvaluator.compute() from the embeddings, the time split
  into the GEMM and the rank kernel by HIP events around every chunk's two calls, and the peak extra memory
  (torch.cuda.max_memory_allocated above what was allocated before the call) next to the one-chunk model."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM = 5e12


def timed(fn, reps=10, warm=3):
    """Median milliseconds of fn() by HIP events."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def kernels(rows, cols, host_limit, lines):
    import recall_ref as RF
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    s = torch.randn(rows, cols, device="cuda", generator=torch.Generator("cuda").manual_seed(rows + cols))
    nbytes = 4.0 * rows * cols
    ar = torch.arange(rows, device="cuda")
    t_rank = timed(lambda: gt_ranks(s, 1, "t2v", n_videos=cols))
    t_topk = timed(lambda: topk_rows(s, 10))
    t_torch = timed(lambda: (s > s[ar, ar][:, None]).sum(1))
    got = gt_ranks(s, 1, "t2v", n_videos=cols)
    assert torch.equal(got, (s > s[ar, ar][:, None]).sum(1).double())
    lines.append("%6d x %6d (%.2f GB): ranks %8.3f ms (%4.1f %% of 5 TB/s)   top-10 %8.3f ms (%4.1f %%)   torch (s > g).sum(1) %8.3f ms"
                 % (rows, cols, nbytes / 1e9, t_rank, 100 * nbytes / (t_rank * 1e-3) / HBM, t_topk,
                    100 * nbytes / (t_topk * 1e-3) / HBM, t_torch))
    if rows * cols <= host_limit:
        h = s.cpu().numpy()
        t0 = time.perf_counter()
        want = RF.t2v_ranks(h, 1)
        t_host = time.perf_counter() - t0
        assert np.array_equal(got.cpu().numpy(), want)
        lines.append("%s host numpy recall_ref.t2v_ranks %.3f s (once)" % (" " * 26, t_host))
    del s
    torch.cuda.empty_cache()


def evaluator(n, D, chunk_bytes, lines):
    from egovlp_amd import retrieval_ops
    from egovlp_amd.model.model import sim_matrix_mm
    from egovlp_amd.trainer.retrieval_eval import RecallEvaluator, chunk_plan
    g = torch.Generator("cuda").manual_seed(n)
    t = torch.randn(n, D, device="cuda", generator=g)
    v = t + 0.5 * torch.randn(n, D, device="cuda", generator=g)
    ev = RecallEvaluator(chunk_bytes=chunk_bytes)
    ev.update(t, v)
    ev.compute()                                                  # warm-up
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ev.update(t, v)
    t0 = time.perf_counter()
    res = ev.compute()[0]
    total = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    # the same walk with events around each chunk's GEMM and rank call
    tn, vn = retrieval_ops.row_normalize(t), retrieval_ops.row_normalize(v)
    pairs = []
    for rows, cols, kw in ((tn, vn, dict(direction="t2v")), (vn, tn, dict(direction="v2t", transposed=False))):
        plan = chunk_plan(n, n, chunk_bytes)
        for c0, c1 in zip(plan[:-1], plan[1:]):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            s = sim_matrix_mm(rows[c0:c1], cols)
            e[1].record()
            retrieval_ops.gt_ranks(s, 1, row0=c0, n_videos=n, **kw)
            e[2].record()
            pairs.append(e)
            del s
    torch.cuda.synchronize()
    t_gemm = sum(e[0].elapsed_time(e[1]) for e in pairs)
    t_rank = sum(e[1].elapsed_time(e[2]) for e in pairs)
    rows_per = chunk_plan(n, n, chunk_bytes)[1]
    lines.append("%6d^2, D = %d, %d chunks of %d rows per direction: compute() %.3f s; by events GEMM (split + bf16x3) %.1f ms, rank kernel "
                 "%.1f ms; peak extra memory %.1f MB, one chunk %.1f MB, embeddings normalised %.1f MB; R1 t2v %.2f v2t %.2f"
                 % (n, D, len(chunk_plan(n, n, chunk_bytes)) - 1, rows_per, total, t_gemm, t_rank, peak / 1e6, 4.0 * rows_per * n / 1e6,
                    2 * 4.0 * n * D / 1e6, res["t2v_metrics"]["R1"], res["v2t_metrics"]["R1"]))
    del t, v, tn, vn
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3842x9668,16384x16384,8192x262144")
    ap.add_argument("--eval", default="16384,65536")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30)
    ap.add_argument("--host-limit", type=int, default=16384 * 16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Recall@K kernels and RecallEvaluator on %s" % torch.cuda.get_device_name(0)]
    for sz in filter(None, a.sizes.split(",")):
        r, c = (int(x) for x in sz.split("x"))
        kernels(r, c, a.host_limit, lines)
        print(lines[-1], flush=True)
    for n in filter(None, a.eval.split(",")):
        evaluator(int(n), a.dim, a.chunk_bytes, lines)
        print(lines[-1], flush=True)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
