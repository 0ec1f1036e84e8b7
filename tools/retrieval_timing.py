"""Time the EPIC-sized retrieval scoring (9 668 clips x 3 842 sentences) on the device against the same arithmetic on the host.

    python tools/retrieval_timing.py [--reps 10] [--host-reps 2] [--out profiles/retrieval_metrics_timing.txt]

Device: egovlp_amd.model.metric.mir_metrics on a similarity matrix that already lives in HBM, timed with a host clock around
calls that end in the metric's own host copy of the scalars (a synchronisation), after a warm-up; with the IDCG cached (every
call but the first of a validation run) and not cached (a fresh annotations object per call; includes the upload of the fp64
relevancy matrix, as a first call does).  Host: tests/retrieval_ref.py (numpy: a full stable argsort of every row in both
directions, a gather of the float64 relevancy, cumulative sums -- the arithmetic of the reference's utils/nDCG.py + utils/mAP.py)
on the same matrix, IDCG included / excluded.  Prints min / median / max of each."""
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


def stats(ts):
    return "min %.4f  median %.4f  max %.4f s  (n = %d)" % (min(ts), statistics.median(ts), max(ts), len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import retrieval_ref as RR
    from egovlp_amd.model.metric import RetrievalAnnotations, mir_metrics
    from egovlp_amd.model.model import sim_matrix
    from egovlp_amd.synth import synth_tensor
    nv, ns, D = 9668, 3842, 256
    rng = np.random.default_rng(100)
    text = synth_tensor("retrieval.text_embed", (nv, D), seed=5).cuda()
    vid = synth_tensor("retrieval.video_embed", (nv, D), seed=6).cuda()
    idx = rng.permutation(nv)
    text_rows = np.sort(rng.permutation(nv)[:ns])
    rel = np.zeros((nv, ns))
    sentence_of = rng.integers(0, ns, size=nv)
    sentence_of[rng.permutation(nv)[:ns]] = np.arange(ns)
    rel[np.arange(nv), sentence_of] = 1.0
    frac = (rng.random((nv, ns)) < 0.002) & (rel == 0)
    rel[frac] = (rng.integers(1, 8, size=(nv, ns)) / 8.0)[frac]
    with torch.no_grad():
        sims = sim_matrix(text, vid)
    idx_d = torch.from_numpy(idx).cuda()
    ann = RetrievalAnnotations(np.arange(nv), text_rows, rel)
    lines = ["mir_metrics at %d clips x %d sentences, %s" % (nv, ns, torch.cuda.get_device_name(0))]
    for _ in range(3):
        res = mir_metrics(sims, idx_d, ann)
    cached, fresh = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mir_metrics(sims, idx_d, ann)
        cached.append(time.perf_counter() - t0)
    for _ in range(max(2, a.reps // 3)):
        ann2 = RetrievalAnnotations(ann.video_id, ann.text_id, rel)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mir_metrics(sims, idx_d, ann2)
        fresh.append(time.perf_counter() - t0)
    lines.append("device, IDCG cached:      " + stats(cached))
    lines.append("device, IDCG not cached:  " + stats(fresh) + "   (fresh annotations: 297 MB relevancy upload + index build included)")
    M = RR.prepare_mir_fast(sims.cpu().numpy(), np.argsort(idx), text_rows)
    host_all, host_rank = [], []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        scal, _ = RR.mir(M, rel, affine_half=True)
        host_all.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        RR.rank_scores(M, rel, True)
        RR.rank_scores(np.ascontiguousarray(M.T), np.ascontiguousarray(rel.T), True)
        host_rank.append(time.perf_counter() - t0)
    lines.append("host numpy, IDCG included: " + stats(host_all))
    lines.append("host numpy, IDCG excluded: " + stats(host_rank) + "   (torch.get_num_threads() = %d; numpy's sort is one thread)" % torch.get_num_threads())
    lines.append("ratio host / device, IDCG cached / excluded: %.0f x;  not cached / included: %.0f x"
                 % (statistics.median(host_rank) / statistics.median(cached), statistics.median(host_all) / statistics.median(fresh)))
    lines.append("scores: device %s" % {k: round(v, 6) for k, v in res.items()})
    lines.append("        host   %s" % {k: round(float(v), 6) for k, v in scal.items()})
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
