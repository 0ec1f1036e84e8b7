"""Tensor-level wrapper of the retrieval-scoring kernel (include/egovlp_hip.h: egv_rank_scores)."""
import torch

from . import _lib, ops
from ._lib import check
from .ops import _p

MAX_ROW = 16384      # EGV_RANK_MAX_ROW: longest query row the kernel sorts in LDS


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
