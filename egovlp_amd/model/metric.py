"""EgoMCQ accuracy -- drop-in for the one metric the EgoClip validation pass uses (reference model/metric.py:218-234,
named by configs/pt/egoclip.json `metrics: ["egomcq_accuracy_metrics"]`).

preds [Q, 5] (text-to-video similarities of the five candidate clips), labels [Q] (index of the correct clip), types [Q]
(1 = inter-video, 2 = intra-video in the EgoMCQ json).  The reference pairs the SORTED unique type ids with the fixed name
list ["Intra-video", "Inter-video"] (its zip, :221-223) -- reproduced literally, including the fact that the names follow
the sort order of the ids present, not their meaning.  Vectorised: no Python loop over the questions.

Retrieval scores -- drop-ins for `mir_metrics` (EPIC-Kitchens-100 multi-instance retrieval, reference model/metric.py:257-299,
configs/ft/epic.json, configs/eval/epic.json), `map` / `charades_metrics` (:301-340, configs/ft/charades.json,
configs/eval/charades.json) and `oscc_metrics` (:342-353).  The per-query nDCG / average precision of both directions run on
the device (retrieval_ops.rank_scores -> egv_rank_scores): the similarity matrix is never copied to the host, only the final
scalars are.  Equal similarities are ranked by ascending index (the reference's order among ties is whatever numpy's unstable
sort leaves); similarities are ranked as fp32.

Recall@K -- drop-ins for `t2v_metrics` / `v2t_metrics` (reference model/metric.py:20-216, named by configs/eval/nlq.json and
configs/eval/mq.json, resolved by run/test_nlq.py:37 and run/test_mq.py:36) and for the `cols2metrics` they call (:124, :216).
The reference defines no `cols2metrics`: the EgoVLP copy of the file dropped the function.  The definition here is the one of
the public code those two functions were written for (frozen-in-time / collaborative-experts model/metric.py): R1, R5, R10, R50,
MedR, MeanR and the geometric mean of R1, R5, R10.  The ranks are counts (retrieval_ops.gt_ranks -> egv_gt_ranks), equal to the
positions the reference's sort-and-subtract finds; their summary is torch on the device, read by the host once."""
import csv
import os
import pickle

import numpy as np
import torch

from .. import retrieval_ops


def egomcq_accuracy_metrics(preds, labels, types):
    metrics = {}
    preds, labels, types = torch.as_tensor(preds), torch.as_tensor(labels).reshape(-1), torch.as_tensor(types).reshape(-1)
    hit = (preds.reshape(labels.shape[0], -1).argmax(dim=1) == labels.to(preds.device)).double()
    group_list = ["Intra-video", "Inter-video"]
    for type_i, group_i in zip(torch.unique(types), group_list):
        sel = (types == type_i).to(hit.device)
        metrics[group_i] = float(hit[sel].sum() / sel.sum()) * 100
    return metrics


# ------------------------------------------------------------------------------------------------ EPIC-Kitchens-100 MIR
EPIC_RETRIEVAL_DIR = "dataset/epic-kitchens/epic-kitchens-100-annotations-master/retrieval_annotations"   # model/metric.py:261, :282


class RetrievalAnnotations:
    """What mir_metrics needs besides the similarities: `video_id` (first column of EPIC_100_retrieval_test.csv), `text_id`
    (first column of EPIC_100_retrieval_test_sentence.csv) and `relevancy` [videos, sentences] (the caption-relevancy pickle).
    Any object with these three attributes serves; the per-device relevancy, IDCG vectors and column selection are cached on it
    (attribute `_egv_cache`), so a relevancy matrix costs its two IDCG launches once."""

    def __init__(self, video_id, text_id, relevancy):
        self.video_id, self.text_id, self.relevancy = video_id, text_id, relevancy

    @classmethod
    def from_epic_files(cls, root=EPIC_RETRIEVAL_DIR):
        def first_column(name):
            with open(os.path.join(root, name), newline="") as f:
                rows = list(csv.reader(f))
            return [r[0] for r in rows[1:] if r]                # the header line names the columns, as pandas.read_csv takes it

        with open(os.path.join(root, "relevancy", "caption_relevancy_EPIC_100_retrieval_test.pkl"), "rb") as f:
            relevancy = pickle.load(f)
        return cls(first_column("EPIC_100_retrieval_test.csv"), first_column("EPIC_100_retrieval_test_sentence.csv"), relevancy)


_DEFAULT_ANNOTATIONS = {}


def _default_annotations():
    key = os.path.abspath(EPIC_RETRIEVAL_DIR)
    if key not in _DEFAULT_ANNOTATIONS:
        _DEFAULT_ANNOTATIONS[key] = RetrievalAnnotations.from_epic_files()
    return _DEFAULT_ANNOTATIONS[key]


def _to_device(x, dtype=None):
    """A CUDA tensor stays where it is; a numpy array / CPU tensor is uploaded once to the current device."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))
    if not t.is_cuda and torch.cuda.is_available():
        t = t.cuda()
    return t if dtype is None else t.to(dtype)


def _annotation_cache(annotations, device):
    cache = annotations.__dict__.setdefault("_egv_cache", {})
    c = cache.get(device)
    if c is None:
        rel = annotations.relevancy
        rel = rel if torch.is_tensor(rel) else torch.as_tensor(np.ascontiguousarray(rel))
        if rel.dtype != torch.float32:
            rel = rel.double()                                   # the EPIC pickle is float64: the == 1 / > 0 tests see the original
        rel = rel.to(device)
        video_id = [v.item() if hasattr(v, "item") else v for v in annotations.video_id]
        first = {}
        for i, v in enumerate(video_id):
            first.setdefault(v, i)
        indexes = []
        for elem in annotations.text_id:
            elem = elem.item() if hasattr(elem, "item") else elem
            if elem in first:
                indexes.append(first[elem])
            else:
                print(f"error happened when index of {elem}.")  # model/metric.py:270
        c = cache[device] = {"rel": rel, "n_video": len(video_id), "indexes": torch.as_tensor(indexes, dtype=torch.int64, device=device)}
    return c


def _idcg(c):
    if "idcg_v" not in c:
        c["idcg_v"] = retrieval_ops.rank_scores(None, c["rel"], want_ap=False)[0]
        c["idcg_t"] = retrieval_ops.rank_scores(None, c["rel"], transposed=True, want_ap=False)[0]
    return c["idcg_v"], c["idcg_t"]


def _mir_results(dcg_v, ap_v, dcg_t, ap_t, idcg_v, idcg_t, per_query):
    vals = torch.stack([(dcg_v / idcg_v).mean(), (dcg_t / idcg_t).mean(), ap_v.mean(), ap_t.mean()]).tolist()   # the one host copy
    vis_nDCG, txt_nDCG, vis_mAP, txt_mAP = vals
    metrics = {"nDCG_V2T": vis_nDCG * 100, "nDCG_T2V": txt_nDCG * 100, "nDCG_AVG": 100 * (vis_nDCG + txt_nDCG) / 2,
               "mAP_V2T": vis_mAP * 100, "mAP_T2V": txt_mAP * 100, "mAP_AVG": 100 * (vis_mAP + txt_mAP) / 2}
    if per_query:
        return metrics, {"nDCG_V2T": dcg_v / idcg_v, "nDCG_T2V": dcg_t / idcg_t, "AP_V2T": ap_v, "AP_T2V": ap_t}
    return metrics


def mir_metrics(similarity_matrix, idx_arr, annotations=None, per_query=False):
    """nDCG / mAP of both retrieval directions from the trainer's [texts, videos] similarity matrix (one caption per clip, in
    data-loader order) and the clip indices `idx_arr` of its rows: re-ordered to the csv's order, the sentences' columns
    selected, (s + 1) / 2 applied in fp32, scored against the relevancy matrix -- model/metric.py:257-299.
    per_query=True additionally returns the per-query vectors (device tensors)."""
    if annotations is None:
        annotations = _default_annotations()
    sims = _to_device(similarity_matrix, torch.float32)
    c = _annotation_cache(annotations, sims.device)
    idx = (idx_arr if torch.is_tensor(idx_arr) else torch.as_tensor(np.asarray(idx_arr))).reshape(-1).to(sims.device, torch.int64)
    # order[i] = first position of i in idx_arr (the reference's list.index)
    sorted_idx, perm = torch.sort(idx, stable=True)
    want = torch.arange(c["n_video"], device=sims.device)
    pos = torch.searchsorted(sorted_idx, want).clamp_(max=idx.numel() - 1)
    if not bool((sorted_idx[pos] == want).all()):
        raise ValueError("mir_metrics: idx_arr does not name every clip of the retrieval csv")
    order = perm[pos]
    # similarity_matrix[order][:, order].T[:, indexes]: [videos, sentences]
    m = sims.index_select(0, order.index_select(0, c["indexes"])).index_select(1, order).t().contiguous()
    idcg_v, idcg_t = _idcg(c)
    dcg_v, ap_v = retrieval_ops.rank_scores(m, c["rel"], affine_half=True)
    dcg_t, ap_t = retrieval_ops.rank_scores(m, c["rel"], transposed=True, affine_half=True)
    return _mir_results(dcg_v, ap_v, dcg_t, ap_t, idcg_v, idcg_t, per_query)


def mir_scores(similarity_matrix, annotations, per_query=False):
    """The scoring of run/test_epic.py: an already prepared [sentences, videos] matrix (plain or dual-softmax), no re-ordering
    and no (s + 1) / 2 -- that script applies its own.  Same six keys as mir_metrics."""
    sims = _to_device(similarity_matrix, torch.float32)
    c = _annotation_cache(annotations, sims.device)
    if "rel_t" not in c:
        c["rel_t"] = c["rel"].t().contiguous()                   # [sentences, videos], the layout of the matrix handed over
    idcg_v, idcg_t = _idcg(c)
    dcg_v, ap_v = retrieval_ops.rank_scores(sims, c["rel_t"], transposed=True)
    dcg_t, ap_t = retrieval_ops.rank_scores(sims, c["rel_t"])
    return _mir_results(dcg_v, ap_v, dcg_t, ap_t, idcg_v, idcg_t, per_query)


# ------------------------------------------------------------------------------------------------ Recall@K
RECALL_KEYS = ("R1", "R5", "R10", "R50", "MedR", "MeanR", "geometric_mean_R1-R5-R10")


def _recall_summary(cols, num_queries, keep=None):
    """The seven numbers of cols2metrics from a rank vector on its device.  keep (bool, same length): only these entries count
    (t2v's query mask, model/metric.py:109-115), without compacting the vector.  num_queries: a number or a 0-dim tensor."""
    cols = cols.reshape(-1).double()
    dev = cols.device
    if keep is None:
        n = torch.tensor(cols.numel(), dtype=torch.int64, device=dev)
        live, srt = cols, torch.sort(cols).values
        total = cols.sum()
    else:
        n = keep.sum()
        live = torch.where(keep, cols, torch.full_like(cols, float("inf")))     # dropped entries count for no recall ...
        srt = torch.sort(live).values                                           # ... and sort behind the n kept ones
        total = torch.where(keep, cols, torch.zeros_like(cols)).sum()
    if cols.numel() == 0:
        med = mean = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    else:
        lo, hi = ((n - 1) // 2).clamp(min=0), (n // 2).clamp(max=cols.numel() - 1)
        med = torch.where(n > 0, (srt[lo] + srt[hi]) / 2, torch.full_like(total, float("nan")))   # numpy's median
        mean = total / n
    nq = torch.as_tensor(num_queries).to(device=dev, dtype=torch.float64).reshape(())
    hits = [(live == 0).sum()] + [(live < k).sum() for k in (5, 10, 50)]
    vals = torch.stack([h.double() for h in hits] + [med, mean, nq]).tolist()           # the one host copy
    nq = vals[6]
    metrics = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, hit in zip(("R1", "R5", "R10", "R50"), vals[:4]):
            metrics[name] = float(100 * np.float64(hit) / np.float64(nq))
        metrics["MedR"] = vals[4] + 1
        metrics["MeanR"] = vals[5] + 1
        stats = np.array([metrics[x] for x in ("R1", "R5", "R10")])
        metrics["geometric_mean_R1-R5-R10"] = float(np.exp(np.mean(np.log(stats))))      # 0 when one of them is 0
    return metrics


def cols2metrics(cols, num_queries):
    """Recall summary of a vector of ranks (0 = the ground truth came first): R1 = 100 * #{cols == 0} / n, R5 / R10 / R50 =
    100 * #{cols < k} / n, MedR = median + 1, MeanR = mean + 1 and the geometric mean of R1, R5, R10 -- the function the
    reference calls at model/metric.py:124 and :216 and does not define (see the module docstring for its origin)."""
    return _recall_summary(_to_device(cols, torch.float64), num_queries)


def _recall_inputs(name, sims, query_masks):
    s = _to_device(sims, torch.float32)
    if s.dim() != 2:
        raise ValueError(f"{name}: expected a [texts, videos] matrix")
    nq, nv = s.shape
    if nq < 1 or nv < 1:
        raise ValueError(f"{name}: empty matrix {tuple(s.shape)}")
    if nq % nv != 0:
        raise ValueError(f"{name}: {nq} texts for {nv} videos: Nq must be a multiple of Nv (caption i belongs to video i // (Nq // Nv))")
    mask = None
    if query_masks is not None:
        mask = _to_device(query_masks).to(s.device).reshape(-1)
        if mask.numel() != nq:
            raise ValueError(f"{name}: invalid query mask shape: {mask.numel()} elements for {nq} texts")
        mask = mask != 0
    return s, nq // nv, mask


def t2v_metrics(sims, query_masks=None, per_query=False):
    """Text-to-video recall from sims [texts, videos], sims[i, j] = <text i, video j> (model/metric.py:20-124): rank_i =
    #{j : sims[i, j] > sims[i, i // qpv]}, ties "optimistically"; the queries query_masks marks as missing are dropped afterwards
    and num_queries = query_masks.sum().  per_query=True additionally returns the kept ranks (device tensor)."""
    s, qpv, mask = _recall_inputs("t2v_metrics", sims, query_masks)
    ranks = retrieval_ops.gt_ranks(s, qpv, "t2v", query_masks=mask)
    metrics = _recall_summary(ranks, ranks.numel() if mask is None else mask.sum(), keep=mask)
    if per_query:
        return metrics, (ranks if mask is None else ranks[mask])
    return metrics


def v2t_metrics(sims, query_masks=None, per_query=False):
    """Video-to-text recall from the same [texts, videos] matrix (model/metric.py:127-216): per video the rank of its closest
    existing caption among the existing captions, ties "averaging"; a video without a caption ranks +inf; num_queries = videos.
    per_query=True additionally returns the ranks (device tensor)."""
    s, qpv, mask = _recall_inputs("v2t_metrics", sims, query_masks)
    ranks = retrieval_ops.gt_ranks(s, qpv, "v2t", query_masks=mask)
    metrics = _recall_summary(ranks, ranks.numel())
    if per_query:
        return metrics, ranks
    return metrics


# ------------------------------------------------------------------------------------------------ Charades
def _map_device(sub, gt):
    m_aps = retrieval_ops.rank_scores(sub, gt, transposed=True, want_dcg=False)[1]     # per class column, over the videos
    col = gt.sum(dim=0)
    return m_aps.mean(), m_aps * col / col.sum(), m_aps


def map(submission_array, gt_array):
    """Returns mAP, weighted mAP, and AP array (model/metric.py:301-325): per class column the average precision of the videos
    ranked by descending score (as fp32) against gt == 1; NaN for a class without positives, hence a NaN mean."""
    sub = _to_device(submission_array, torch.float32)
    gt = _to_device(gt_array).to(sub.device)
    gt = gt if gt.dtype == torch.float64 else gt.float()
    m_ap, w_ap, m_aps = _map_device(sub, gt)
    return float(m_ap), w_ap.cpu().numpy(), m_aps.cpu().numpy()


def charades_metrics(submission_array, gt_array):
    """Approximate version of the charades evaluation function (model/metric.py:327-340): videos without a label score -inf."""
    sub = _to_device(submission_array, torch.float32)
    gt = _to_device(gt_array).to(sub.device)
    gt = gt if gt.dtype == torch.float64 else gt.float()
    empty = gt.sum(dim=1) == 0
    fix = sub.masked_fill(empty[:, None], float("-inf"))
    return {"mAP": float(_map_device(fix, gt)[0])}


# ------------------------------------------------------------------------------------------------ OSCC
def oscc_metrics(preds, labels):
    preds, labels = torch.as_tensor(preds), torch.as_tensor(labels).reshape(-1)
    hit = preds.reshape(labels.shape[0], -1).argmax(dim=1) == labels.to(preds.device)
    return {"accuracy": float(hit.double().mean()) * 100}


def pnr_metrics(preds, labels, sc_labels, fps, parent_start_frames, parent_end_frames, parent_pnr_frames):
    """model/metric.py:355-397: mean distance in seconds between the predicted and the annotated point-of-no-return frame over the
    clips with a state change (sc_label == 1).  The predicted frame is `(end - start) / 16 * argmax(pred)` in the tensors' own
    arithmetic (fp32 for integer frame numbers; the 16 is the reference's literal), the error is taken in fp64 and divided by the
    clip's fps.  NaN when no clip has a state change: the reference's `if len(distance_list) == 0` branch is overwritten by the
    line after it (:393-394), so `np.mean([])` is what it returns.  `labels` is not read (as in the reference)."""
    preds = torch.as_tensor(preds).detach().cpu()
    n = preds.shape[0]
    am = preds.reshape(n, -1).argmax(dim=1)

    def col(t):
        return torch.as_tensor(t).detach().cpu().reshape(-1)
    sc, start, end, pnr, fps = col(sc_labels), col(parent_start_frames), col(parent_end_frames), col(parent_pnr_frames), col(fps)
    mapped = ((end - start) / 16 * am).double()                                  # :381-382
    err_sec = (mapped - (pnr - start).double()).abs() / fps.double()             # :383-385
    sel = sc == 1
    if not bool(sel.any()):
        return {"keyframe_distance": float("nan")}
    return {"keyframe_distance": float(np.mean(err_sec[sel].numpy()))}


def oscc_metrics_from_counts(accum):
    """oscc_metrics from the device accumulator of egv_cls_eval_update (hits, rows, -, -)."""
    hits, rows = float(accum[0]), float(accum[1])
    return {"accuracy": hits / rows * 100 if rows > 0 else float("nan")}      # no row seen: the reference divides by zero


def pnr_metrics_from_counts(accum):
    """pnr_metrics from the device accumulator of egv_cls_eval_update (-, rows, sum of err_sec, positives); NaN without positives."""
    err, pos = float(accum[2]), float(accum[3])
    return {"keyframe_distance": err / pos if pos > 0 else float("nan")}
