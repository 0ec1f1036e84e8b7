"""Generate the retrieval-metric goldens by RUNNING THE REFERENCE ITSELF (model/metric.py mir_metrics, map, charades_metrics,
oscc_metrics; utils/nDCG.py; utils/mAP.py).  Run once where the reference is available:
    python tests/golden/make_golden_retrieval.py
Writes, next to this file,
  retrieval_metrics.npz            mir_<tag>_* for (videos, sentences) = (96, 40) and (410, 300), mirtie_*, oscc_*
  retrieval_metrics_charades.npz   charades_*   (a file of its own: the two together would pass the 1 MiB cap on a committed file)

mir_<tag>: fp32 similarities [videos, videos] in [-1, 1] as the trainer hands them over (one caption per clip, rows / columns in
  data-loader order), the permuted idx_arr, video_id, text_id (a subset of video_id), a float64 relevancy [videos, sentences]
  stored sparse (flat indices + values) in which every row and every column holds an exact 1.0 and about 2 % of the entries are
  fractions.  Expected: the six scalars of the reference's mir_metrics, run in a temporary working directory that holds the two
  csv files and the pickle under the paths it hard-codes, and the per-query nDCG (calculate_nDCG(..., reduction=None)) and AP
  (calculate_mAP on one row at a time) of both directions.
mirtie: a prepared [videos, sentences] matrix WITH ties, all of them among zero-relevancy entries; same expected vectors.
charades: [500, 157] fp32 scores, 3 % positives, 20 videos without a label; variant b additionally has a class without a
  positive (NaN).  Expected: charades_metrics and map of the reference.  The reference writes np.NINF, which numpy 2 dropped:
  np.NINF = -np.inf is set before the call.
oscc: [64, 2] scores and labels.

TIES: the reference's order among equal similarities is whatever numpy's unstable sort leaves.  It changes a score only when
the tied items differ in relevancy, so every fixture is re-drawn (the offending entries only) until no row and no column of the
matrix that is ranked -- after the fp32 (s + 1) / 2 -- holds two equal values with different relevancies.  This is asserted."""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))

import retrieval_ref as RR  # noqa: E402
from oracle import ref_import  # noqa: E402

EPIC_DIR = "dataset/epic-kitchens/epic-kitchens-100-annotations-master/retrieval_annotations"


def draw_relevancy(rng, nv, ns):
    rel = np.zeros((nv, ns), dtype=np.float64)
    sentence_of = rng.integers(0, ns, size=nv)
    sentence_of[rng.permutation(nv)[:ns]] = np.arange(ns)         # every sentence is some clip's own caption; several clips share one
    rel[np.arange(nv), sentence_of] = 1.0
    frac = (rng.random((nv, ns)) < 0.02) & (rel == 0)
    den = rng.integers(2, 9, size=(nv, ns))
    num = np.minimum(rng.integers(1, 8, size=(nv, ns)), den - 1)
    rel[frac] = (num / den)[frac]                                 # IoU-like fractions in (0, 1)
    assert (rel == 1).any(axis=1).all() and (rel == 1).any(axis=0).all()
    return rel


def no_conflicts(M, rel):
    return not RR.tie_conflicts(M, rel).any() and not RR.tie_conflicts(M.T, rel.T).any()


def per_query(nDCG, mAP, M, rel, prefix, out):
    out[prefix + "_q_nDCG_V2T"] = nDCG.calculate_nDCG(M, rel, reduction=None)
    out[prefix + "_q_nDCG_T2V"] = nDCG.calculate_nDCG(M.T, rel.T, reduction=None)
    out[prefix + "_q_AP_V2T"] = np.array([mAP.calculate_mAP(M[i:i + 1], rel[i:i + 1]) for i in range(M.shape[0])])
    out[prefix + "_q_AP_T2V"] = np.array([mAP.calculate_mAP(M.T[j:j + 1], rel.T[j:j + 1]) for j in range(M.shape[1])])


def make_mir(metric_mod, nDCG, mAP, rng, nv, ns, tag, out):
    video_id = 1000 + 7 * rng.permutation(nv)
    text_id = video_id[np.sort(rng.permutation(nv)[:ns])]
    rel = draw_relevancy(rng, nv, ns)
    idx_arr = rng.permutation(nv)
    sims = rng.uniform(-1, 1, size=(nv, nv)).astype(np.float32)
    where = RR.prepare_mir(np.arange(nv * nv).reshape(nv, nv), idx_arr, video_id, text_id)   # which entry of sims lands where
    redrawn = 0
    while True:
        M = RR.transform(RR.prepare_mir(sims, idx_arr, video_id, text_id), affine_half=True)
        i1, j1 = RR.tie_conflict_entries(M, rel)
        j2, i2 = RR.tie_conflict_entries(M.T, rel.T)
        bad = where[np.concatenate([i1, i2]), np.concatenate([j1, j2])]
        if bad.size == 0:
            break
        sims.reshape(-1)[bad] = rng.uniform(-1, 1, size=bad.size).astype(np.float32)
        redrawn += bad.size
    assert no_conflicts(M, rel)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, EPIC_DIR, "relevancy"))
        with open(os.path.join(tmp, EPIC_DIR, "EPIC_100_retrieval_test.csv"), "w") as f:
            f.write("narration_id,narration\n" + "".join("%d,clip %d\n" % (v, v) for v in video_id))
        with open(os.path.join(tmp, EPIC_DIR, "EPIC_100_retrieval_test_sentence.csv"), "w") as f:
            f.write("narration_id,narration\n" + "".join("%d,clip %d\n" % (v, v) for v in text_id))
        with open(os.path.join(tmp, EPIC_DIR, "relevancy", "caption_relevancy_EPIC_100_retrieval_test.pkl"), "wb") as f:
            pickle.dump(rel, f)
        os.chdir(tmp)
        try:
            res = metric_mod.mir_metrics(sims.copy(), idx_arr.copy())
        finally:
            os.chdir(cwd)
    nz = np.flatnonzero(rel)
    out.update({f"mir_{tag}_sims": sims, f"mir_{tag}_idx_arr": idx_arr.astype(np.int64), f"mir_{tag}_video_id": video_id.astype(np.int64),
                f"mir_{tag}_text_id": text_id.astype(np.int64), f"mir_{tag}_rel_shape": np.array(rel.shape, dtype=np.int64),
                f"mir_{tag}_rel_index": nz.astype(np.int32), f"mir_{tag}_rel_value": rel.reshape(-1)[nz]})
    for k, v in res.items():
        out[f"mir_{tag}_{k}"] = np.float64(v)
    per_query(nDCG, mAP, M, rel, f"mir_{tag}", out)
    print(f"mir_{tag}: {redrawn} entries re-drawn for the tie condition;", {k: round(float(v), 4) for k, v in res.items()})


def make_mirtie(nDCG, mAP, rng, out):
    nv, ns = 24, 16
    rel = draw_relevancy(rng, nv, ns)
    M = (rng.integers(-8, 9, size=(nv, ns)) / 8.0).astype(np.float32)          # 17 levels: every row and column is full of ties
    nz = np.nonzero(rel)
    M[nz] = (0.0371 + 0.0023 * rng.permutation(nz[0].size)).astype(np.float32)   # relevant entries: distinct, off the grid
    assert no_conflicts(M, rel)
    assert (np.sort(M, axis=1)[:, 1:] == np.sort(M, axis=1)[:, :-1]).any(axis=1).all()
    flat = np.flatnonzero(rel)
    out.update({"mirtie_M": M, "mirtie_rel_shape": np.array(rel.shape, dtype=np.int64), "mirtie_rel_index": flat.astype(np.int32),
                "mirtie_rel_value": rel.reshape(-1)[flat]})
    per_query(nDCG, mAP, M, rel, "mirtie", out)


def make_charades(metric_mod, rng, out):
    nv, nc = 500, 157
    gt = (rng.random((nv, nc)) < 0.03).astype(np.float64)
    gt[rng.permutation(nv)[:20]] = 0
    for c in np.flatnonzero(gt.sum(axis=0) == 0):
        gt[np.flatnonzero(gt.sum(axis=1) > 0)[c], c] = 1
    sub = rng.standard_normal((nv, nc)).astype(np.float32)
    while True:
        j, i = RR.tie_conflict_entries(sub.T, gt.T)
        if i.size == 0:
            break
        sub[i, j] = rng.standard_normal(i.size).astype(np.float32)
    np.NINF = -np.inf                                             # numpy 2 dropped the alias the reference uses
    out["charades_sub"] = sub
    for tag, g in (("a", gt), ("b", gt * (np.arange(nc) != 5))):
        assert not RR.tie_conflicts(sub.T, g.T).any()
        out[f"charades_{tag}_gt_index"] = np.flatnonzero(g).astype(np.int32)
        out[f"charades_{tag}_mAP"] = np.float64(metric_mod.charades_metrics(sub.copy(), g.copy())["mAP"])
        m_ap, w_ap, m_aps = metric_mod.map(sub.copy(), g.copy())
        out[f"charades_{tag}_map_m_ap"], out[f"charades_{tag}_map_w_ap"], out[f"charades_{tag}_map_m_aps"] = np.float64(m_ap), w_ap, m_aps
        print(f"charades_{tag}: mAP {out[f'charades_{tag}_mAP']}, map() {m_ap}, NaN classes {int(np.isnan(m_aps).sum())}")
    out["charades_gt_shape"] = np.array([nv, nc], dtype=np.int64)


def make_oscc(metric_mod, rng, out):
    preds = rng.standard_normal((64, 2)).astype(np.float32)
    labels = rng.integers(0, 2, size=64).astype(np.int64)
    out["oscc_preds"], out["oscc_labels"] = preds, labels
    out["oscc_accuracy"] = np.float64(metric_mod.oscc_metrics(torch.from_numpy(preds), torch.from_numpy(labels))["accuracy"])


def main():
    ref_import.load_reference()                                   # stubs what the reference imports and this machine lacks
    import model.metric as metric_mod
    from utils import mAP, nDCG
    rng = np.random.default_rng(20240607)
    out = {}
    make_mir(metric_mod, nDCG, mAP, rng, 96, 40, "s", out)
    make_mir(metric_mod, nDCG, mAP, rng, 410, 300, "m", out)
    make_mirtie(nDCG, mAP, rng, out)
    make_oscc(metric_mod, rng, out)
    np.savez(os.path.join(HERE, "retrieval_metrics.npz"), **out)
    out = {}
    make_charades(metric_mod, rng, out)
    np.savez(os.path.join(HERE, "retrieval_metrics_charades.npz"), **out)
    for n in ("retrieval_metrics.npz", "retrieval_metrics_charades.npz"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()
