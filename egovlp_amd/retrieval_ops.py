"""Tensor-level wrappers of the retrieval kernels (include/egovlp_hip.h: egv_rank_scores; egv_gt_ranks, egv_topk_rows,
egv_row_normalize)."""
import torch

from . import _lib, ops
from ._lib import check
from .ops import _p

MAX_ROW = 16384      # EGV_RANK_MAX_ROW: longest query row the kernel sorts in LDS
TOPK_MAX = 64        # EGV_TOPK_MAX: longest top-k list of egv_topk_rows
MAX_LEN = 2 ** 31 - 1                # rows / columns of a matrix handed to egv_gt_ranks / egv_topk_rows (int32 in the C ABI)
MAX_TRANSPOSED_ROWS = 65535 * 32     # egv_gt_ranks, transposed form: rows of the matrix the device-side transpose takes


def rank_scores(sims, relevancy, transposed=False, affine_half=False, want_dcg=True, want_ap=True):
    """Per query: DCG (first K_i = #{relevancy > 0} positions, discount 1 / log2(p + 2)) and average precision (relevancy == 1)
    of the ranking by descending similarity, ties by ascending index -> (dcg, ap), fp64 vectors (None where not wanted).

    sims [n1, n2] fp32 and relevancy [n1, n2] fp32 or fp64 on the device.  The queries are the rows, or the columns when
    `transposed` (sims^T scored against relevancy^T, transposed on the device).  sims None: the ideal ranking, sims := relevancy
    (IDCG).  affine_half: rank by (s + 1) / 2 evaluated in fp32.  A query row longer than MAX_ROW raises."""
    ops._need_cuda(sims, relevancy)
    if relevancy.dim() != 2 or (sims is not None and (sims.dim() != 2 or sims.shape != relevancy.shape)):
        raise ValueError("rank_scores: sims and relevancy must be [n1, n2] matrices of one shape")
    if relevancy.dtype not in (torch.float32, torch.float64):
        raise ValueError("rank_scores: relevancy must be float32 or float64")
    if not (want_dcg or want_ap):
        raise ValueError("rank_scores: nothing asked for")
    n1, n2 = relevancy.shape
    if n1 < 1 or n2 < 1:
        raise ValueError("rank_scores: empty matrix")
    def rows_dense(t):                                           # unit stride inside a row; a one-row matrix has no leading dimension
        return t.stride(1) == 1 and (n1 == 1 or t.stride(0) >= n2)

    def ld(t):
        return n2 if n1 == 1 else t.stride(0)

    r = relevancy if rows_dense(relevancy) else relevancy.contiguous()
    s = None
    if sims is not None:
        s = sims.float()
        if not rows_dense(s):
            s = s.contiguous()
    dev = r.device
    nq = n2 if transposed else n1
    dcg = torch.empty(nq, dtype=torch.float64, device=dev) if want_dcg else None
    ap = torch.empty(nq, dtype=torch.float64, device=dev) if want_ap else None
    lib = _lib.lib()
    work = None
    if transposed:
        work = torch.empty(max(int(lib.egv_rank_scores_work_bytes(n1, n2)), 8) // 8, dtype=torch.float64, device=dev)
    check(lib.egv_rank_scores(_p(s), 0 if s is None else ld(s), int(bool(transposed)), _p(r), int(r.dtype == torch.float64),
                              ld(r), n1, n2, int(bool(affine_half)), _p(dcg), _p(ap), _p(work), ops._stream(r)),
          "egv_rank_scores")
    return dcg, ap


def _rows_dense(t):
    """[n1, n2] fp32 with unit stride inside a row -> (tensor, leading dimension); copied only when the layout does not fit."""
    t = t if t.dtype == torch.float32 else t.float()
    n1, n2 = t.shape
    if t.stride(1) != 1 or (n1 > 1 and t.stride(0) < n2):
        t = t.contiguous()
    return t, (n2 if n1 == 1 else t.stride(0))


def _matrix_check(name, sims):
    if not torch.is_tensor(sims) or sims.dim() != 2:
        raise ValueError(f"{name}: sims must be a [rows, columns] matrix")
    n1, n2 = sims.shape
    if n1 < 1 or n2 < 1:
        raise ValueError(f"{name}: empty matrix {tuple(sims.shape)}: at least one row and one column are needed")
    if n1 > MAX_LEN or n2 > MAX_LEN:
        raise ValueError(f"{name}: a matrix has at most {MAX_LEN} rows and {MAX_LEN} columns")
    return n1, n2


def _valid_vector(name, mask, n, device):
    """query_masks / col_valid in any shape with n elements -> uint8 [n] on the device (nonzero = exists), or None."""
    if mask is None:
        return None
    m = mask if torch.is_tensor(mask) else torch.as_tensor(mask)
    if m.numel() != n:
        raise ValueError(f"{name}: the mask has {m.numel()} elements, {n} are needed (one per caption)")
    return (m.reshape(-1) != 0).to(device=device, dtype=torch.uint8).contiguous()


def gt_ranks(sims, qpv, direction, query_masks=None, row0=0, n_videos=None, transposed=None, tie=None):
    """Rank of the ground truth of every query, as the count the reference's sort-and-subtract finds (model/metric.py:20-216)
    -> fp64 vector on the device, one entry per query.  Caption i belongs to video i // qpv.

    direction "t2v": sims [captions, videos]; the queries are the rows, global caption row0 + r.  rank = #{j : s_j > g},
      g = sims[r, (row0 + r) // qpv] (ties "optimistically").  query_masks does not enter the ranks (the caller drops the
      masked queries afterwards, :109-115); only its size is checked.
    direction "v2t": the queries are the videos and the captions are what is ranked; only the captions query_masks leaves count.
      g = the best valid caption of the video, rank = #{s > g} + (#{s == g} - 1) / 2 (ties "averaging"), +inf without one.
      transposed=True (the default): sims is the [captions, videos] matrix the metric functions receive, ranked column-wise.
      transposed=False: sims is [videos, captions], rows row0 + r of a larger problem (the chunked form of RecallEvaluator).
    n_videos: the number of videos of the whole problem when sims is a chunk of its rows (default: what sims itself shows).
    tie: "optimistic" / "averaging" to override the direction's rule."""
    if direction not in ("t2v", "v2t"):
        raise ValueError(f"gt_ranks: direction must be 't2v' or 'v2t', not {direction!r}")
    if tie not in (None, "optimistic", "averaging"):
        raise ValueError(f"gt_ranks: tie must be 'optimistic' or 'averaging', not {tie!r}")
    n1, n2 = _matrix_check("gt_ranks", sims)
    qpv, row0 = int(qpv), int(row0)
    if qpv < 1 or row0 < 0:
        raise ValueError("gt_ranks: qpv >= 1 and row0 >= 0 are needed")
    wide = direction == "v2t"
    transposed = (wide if transposed is None else bool(transposed))
    if transposed and not wide:
        raise ValueError("gt_ranks: the transposed form belongs to direction 'v2t'")
    if transposed and row0 != 0:
        raise ValueError("gt_ranks: row0 belongs to the row form (transposed=False)")
    if transposed and n1 > MAX_TRANSPOSED_ROWS:
        raise ValueError(f"gt_ranks: the transposed form takes at most {MAX_TRANSPOSED_ROWS} captions; rank sims.T in row form")
    if not wide:                                                 # [captions chunk, videos]
        nv = n2 if n_videos is None else int(n_videos)
        nq, rows, n_caps = qpv * nv, n1, None
        if nv != n2:
            raise ValueError(f"gt_ranks: sims has {n2} columns but n_videos = {nv}")
        if row0 + rows > nq:
            raise ValueError(f"gt_ranks: captions {row0}..{row0 + rows - 1} of {nq} = qpv * Nv: Nq must be a multiple of Nv "
                             f"(Nq == {qpv} * {nv})")
    else:
        n_caps, rows = (n1, n2) if transposed else (n2, n1)
        nv = (rows if transposed else n_caps // qpv) if n_videos is None else int(n_videos)
        if n_caps != qpv * nv:
            raise ValueError(f"gt_ranks: {n_caps} captions for {nv} videos: Nq must be a multiple of Nv (Nq == {qpv} * Nv)")
        if row0 + rows > nv:
            raise ValueError(f"gt_ranks: videos {row0}..{row0 + rows - 1} of {nv}")
        nq = n_caps
    cv = _valid_vector("gt_ranks", query_masks, nq, sims.device)
    ops._need_cuda(sims)
    s, ld = _rows_dense(sims)
    out = torch.empty(rows, dtype=torch.float64, device=s.device)
    lib = _lib.lib()
    work = None
    if transposed:
        work = torch.empty(max(int(lib.egv_gt_ranks_work_bytes(n1, n2)), 4) // 4, dtype=torch.float32, device=s.device)
    avg = (tie == "averaging") if tie is not None else wide
    check(lib.egv_gt_ranks(_p(s), ld, int(transposed), n1, n2, row0, qpv, int(wide), _p(cv) if wide else None, int(avg), _p(out),
                           _p(work), ops._stream(s)), "egv_gt_ranks")
    return out


def topk_rows(sims, k, col_valid=None):
    """Per row of sims [rows, columns] the k <= TOPK_MAX largest entries among the columns col_valid leaves (uint8 / bool, one
    per column, nonzero = exists) -> (values fp32 [rows, k], indices int64 [rows, k]), descending, ties by ascending column
    (the rule of rank_scores).  With fewer than k valid columns the tail is -inf / -1."""
    n1, n2 = _matrix_check("topk_rows", sims)
    k = int(k)
    if k < 1 or k > TOPK_MAX:
        raise ValueError(f"topk_rows: k = {k}, 1 <= k <= {TOPK_MAX} is needed")
    cv = _valid_vector("topk_rows", col_valid, n2, sims.device)
    ops._need_cuda(sims)
    s, ld = _rows_dense(sims)
    vals = torch.empty((n1, k), dtype=torch.float32, device=s.device)
    idx = torch.empty((n1, k), dtype=torch.int64, device=s.device)
    check(_lib.lib().egv_topk_rows(_p(s), ld, n1, n2, _p(cv), k, _p(vals), _p(idx), ops._stream(s)), "egv_topk_rows")
    return vals, idx


def row_normalize(x, eps=1e-8):
    """x / max(|x|_2, eps) per row of x [rows, D] -- sim_matrix's normalisation (model/model.py:189-197) as an op of its own."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("row_normalize: x must be a non-empty [rows, D] matrix")
    if x.shape[0] > MAX_LEN or x.shape[1] > MAX_LEN:
        raise ValueError(f"row_normalize: at most {MAX_LEN} rows and columns")
    ops._need_cuda(x)
    xs, ld = _rows_dense(x.detach())
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=xs.device)
    check(_lib.lib().egv_row_normalize(_p(xs), ld, x.shape[0], x.shape[1], float(eps), _p(out), x.shape[1], ops._stream(xs)),
          "egv_row_normalize")
    return out
