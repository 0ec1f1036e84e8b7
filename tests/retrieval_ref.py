"""TEST INFRASTRUCTURE: the two retrieval scores in plain numpy, with the device kernel's tie rule, for sizes where no golden
output of the reference is stored.  tests/test_retrieval_metrics_cpu.py pins this file to every stored golden.

Per query row i of similarities S [n1, n2] and relevancies R [n1, n2], with pi_i = the columns of row i by descending
similarity, EQUAL SIMILARITIES BY ASCENDING COLUMN INDEX:
    DCG_i = sum_p R[i, pi_i(p)] * [p < K_i] / log2(p + 2),            K_i = #{j : R[i, j] > 0}
    AP_i  = (1 / n_i) sum_{p : R[i, pi_i(p)] == 1} c_i(p) / (p + 1),   n_i = #{j : R[i, j] == 1}  (0 / 0 = NaN)
    c_i(p) = sum_{q <= p} R[i, pi_i(q)]: the running sum of the relevancies, which is the number of positions <= p with
             relevancy 1 when R holds only 0 and 1, and what the EPIC evaluation computes when R also holds fractions.
Everything after the ranking is float64.  Never imported by the product."""
import numpy as np


def transform(S, affine_half=False):
    S = np.asarray(S, dtype=np.float32)
    if affine_half:
        S = (S + np.float32(1)) / np.float32(2)                 # float32 arithmetic, as the EPIC scoring applies it
    return S


def ranking(S):
    """[n1, n2] column indices by descending similarity, ties by ascending index (a stable sort of the negated values)."""
    return np.argsort(-np.asarray(S), axis=1, kind="stable")


def rank_scores(S, R, affine_half=False, chunk=512):
    """-> (dcg [n1], ap [n1]) float64.  S None: the ideal ranking, S := R (IDCG)."""
    R = np.asarray(R)
    n1, n2 = R.shape
    pos = np.arange(n2)
    disc = 1.0 / np.log2(pos + 2.0)
    dcg = np.empty(n1)
    ap = np.empty(n1)
    for a in range(0, n1, chunk):
        r = R[a:a + chunk].astype(np.float64)
        s = r if S is None else transform(S[a:a + chunk], affine_half)
        rr = np.take_along_axis(r, ranking(s), axis=1)
        K = (r > 0).sum(axis=1)
        dcg[a:a + chunk] = (rr * (pos[None, :] < K[:, None]) * disc).sum(axis=1)
        hit = rr == 1
        with np.errstate(invalid="ignore", divide="ignore"):
            ap[a:a + chunk] = (np.where(hit, np.cumsum(rr, axis=1), 0.0) / (pos + 1.0)).sum(axis=1) / hit.sum(axis=1)
    return dcg, ap


def mir(M, R, affine_half=False):
    """The six EPIC scores (percent) and the per-query vectors from a prepared [videos, sentences] matrix."""
    R = np.asarray(R)
    Mt, Rt = np.ascontiguousarray(np.asarray(M).T), np.ascontiguousarray(R.T)
    dcg_v, ap_v = rank_scores(M, R, affine_half)
    dcg_t, ap_t = rank_scores(Mt, Rt, affine_half)
    nd_v, nd_t = dcg_v / rank_scores(None, R)[0], dcg_t / rank_scores(None, Rt)[0]
    v, t, av, at = nd_v.mean(), nd_t.mean(), ap_v.mean(), ap_t.mean()
    scal = {"nDCG_V2T": v * 100, "nDCG_T2V": t * 100, "nDCG_AVG": 100 * (v + t) / 2,
            "mAP_V2T": av * 100, "mAP_T2V": at * 100, "mAP_AVG": 100 * (av + at) / 2}
    return scal, {"nDCG_V2T": nd_v, "nDCG_T2V": nd_t, "AP_V2T": ap_v, "AP_T2V": ap_t}


def prepare_mir(sims, idx_arr, video_id, text_id):
    """The re-ordering of mir_metrics: [texts, videos] in loader order -> [videos, sentences] in the csv's order."""
    video_id = list(video_id)
    indexes = [video_id.index(e) for e in text_id]
    idx = list(np.asarray(idx_arr).tolist())
    order = [idx.index(i) for i in range(len(video_id))]
    sims = np.asarray(sims)
    return sims[order, :][:, order].T[:, indexes]


def prepare_mir_fast(sims, order, indexes):
    """prepare_mir with the two index lists already known: sims[order][:, order].T[:, indexes] without the big temporaries."""
    order, indexes = np.asarray(order), np.asarray(indexes)
    return np.ascontiguousarray(np.asarray(sims)[order[indexes]][:, order].T)


def tie_conflicts(S, R):
    """Boolean [n1]: rows in which two EQUAL similarities carry DIFFERENT relevancies -- the only case in which the order among
    ties changes a score.  (In a group of equal values with non-uniform relevancy some neighbouring pair differs.)"""
    S, R = np.asarray(S), np.asarray(R)
    order = np.argsort(S, axis=1, kind="stable")
    ss = np.take_along_axis(S, order, axis=1)
    rr = np.take_along_axis(R, order, axis=1)
    return ((ss[:, 1:] == ss[:, :-1]) & (rr[:, 1:] != rr[:, :-1])).any(axis=1)


def tie_conflict_entries(S, R):
    """(rows, cols) of the entries that take part in such a conflict (for re-drawing them)."""
    S, R = np.asarray(S), np.asarray(R)
    order = np.argsort(S, axis=1, kind="stable")
    ss = np.take_along_axis(S, order, axis=1)
    rr = np.take_along_axis(R, order, axis=1)
    i, p = np.nonzero((ss[:, 1:] == ss[:, :-1]) & (rr[:, 1:] != rr[:, :-1]))
    return i, order[i, p]


def sparse_to_dense(shape, flat_index, values):
    R = np.zeros(int(shape[0]) * int(shape[1]), dtype=np.float64)
    R[np.asarray(flat_index, dtype=np.int64)] = values
    return R.reshape(int(shape[0]), int(shape[1]))
