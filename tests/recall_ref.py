"""TEST INFRASTRUCTURE: numpy restatement of the Recall@K rule (reference model/metric.py t2v_metrics :20-124, v2t_metrics
:127-216) in its count form, of `cols2metrics` and of the top-k rule.  tests/test_recall_cpu.py pins it to the ranks the
reference itself produced (tests/golden/recall_ranks.npz), which makes it a trustworthy stand-in at sizes without a golden.

sims [Nq, Nv], sims[i, j] = <text i, video j>; qpv = Nq // Nv; caption i belongs to video i // qpv.
  t2v: rank_i = #{j : sims[i, j] > sims[i, i // qpv]}; masks do not enter the ranks, the masked queries are dropped afterwards.
  v2t: only valid captions count; g_v = max over the valid captions c of video v of sims[c, v];
       rank_v = #{valid c : sims[c, v] > g_v} + (#{valid c : sims[c, v] == g_v} - 1) / 2; +inf for a video without one.
Comparisons are numpy float32 comparisons (IEEE: -0.0 == +0.0)."""
import numpy as np


def t2v_ranks(sims, qpv=None, row0=0):
    """Ranks of the rows of sims [rows, Nv], global caption row0 + r (unfiltered)."""
    sims = np.asarray(sims, dtype=np.float32)
    qpv = sims.shape[0] // sims.shape[1] if qpv is None else qpv
    gt = (row0 + np.arange(sims.shape[0])) // qpv
    g = sims[np.arange(sims.shape[0]), gt][:, None]
    return (sims > g).sum(axis=1).astype(np.float64)


def v2t_ranks_rows(rows, qpv, valid=None, row0=0, tie="averaging"):
    """Row form: rows [videos, captions], the captions of global video row0 + r are the columns (row0 + r) * qpv ...; valid:
    one flag per caption."""
    rows = np.asarray(rows, dtype=np.float32)
    valid = np.ones(rows.shape[1], dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    out = np.full(rows.shape[0], np.inf)
    for r in range(rows.shape[0]):
        seg = np.arange((row0 + r) * qpv, (row0 + r + 1) * qpv)
        seg = seg[valid[seg]]
        if seg.size == 0:
            continue
        g = rows[r, seg].max()
        gt, eq = (rows[r, valid] > g).sum(), (rows[r, valid] == g).sum()
        out[r] = gt + ((eq - 1) / 2 if tie == "averaging" else 0.0)
    return out


def v2t_ranks(sims, query_masks=None):
    """Ranks of the videos from sims [Nq, Nv]."""
    sims = np.asarray(sims, dtype=np.float32)
    return v2t_ranks_rows(sims.T, sims.shape[0] // sims.shape[1], query_masks)


def cols2metrics(cols, num_queries):
    """The function the reference calls at model/metric.py:124 / :216 and does not define; the definition of the public code
    those call sites were written for (frozen-in-time / collaborative-experts model/metric.py)."""
    cols = np.asarray(cols, dtype=np.float64)
    metrics = {}
    metrics["R1"] = 100 * float(np.sum(cols == 0)) / num_queries
    metrics["R5"] = 100 * float(np.sum(cols < 5)) / num_queries
    metrics["R10"] = 100 * float(np.sum(cols < 10)) / num_queries
    metrics["R50"] = 100 * float(np.sum(cols < 50)) / num_queries
    metrics["MedR"] = np.median(cols) + 1
    metrics["MeanR"] = np.mean(cols) + 1
    stats = np.array([metrics[x] for x in ("R1", "R5", "R10")], dtype=np.float64)
    with np.errstate(divide="ignore"):
        metrics["geometric_mean_R1-R5-R10"] = float(np.exp(np.mean(np.log(stats))))
    return metrics


def t2v_metrics(sims, query_masks=None):
    cols = t2v_ranks(sims)
    n = cols.size
    if query_masks is not None:
        keep = np.asarray(query_masks).reshape(-1) != 0
        cols, n = cols[keep], keep.sum()
    return cols2metrics(cols, n), cols


def v2t_metrics(sims, query_masks=None):
    cols = v2t_ranks(sims, query_masks)
    return cols2metrics(cols, cols.size), cols


def topk_rows(rows, k, valid=None):
    """(values [rows, k] fp32, indices [rows, k] int64): descending value, ties by ascending column, among the valid columns;
    -inf / -1 behind the last valid one."""
    rows = np.asarray(rows, dtype=np.float32)
    valid = np.ones(rows.shape[1], dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    cols = np.flatnonzero(valid)
    vals = np.full((rows.shape[0], k), -np.inf, dtype=np.float32)
    idx = np.full((rows.shape[0], k), -1, dtype=np.int64)
    for r in range(rows.shape[0]):
        v = rows[r, cols] + np.float32(0.0)                      # -0.0 -> +0.0: equal similarities
        order = np.lexsort((cols, -v))[:k]
        vals[r, :order.size] = rows[r, cols[order]]
        idx[r, :order.size] = cols[order]
    return vals, idx
