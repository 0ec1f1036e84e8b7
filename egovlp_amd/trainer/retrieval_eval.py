"""Validation glue of the retrieval fine-tuning tasks: what trainer/trainer_epic.py:_valid_epoch does between the forward pass
and the logging, with everything kept on the device.

The reference appends `text_embed.cpu()` / `vid_embed.cpu()` of every batch, concatenates on the host, computes
`sim_matrix(...).cpu().numpy()` and hands that to the metric functions (:216-243).  Here the gathered per-batch embeddings stay
where they are, the similarity matrix comes from model.sim_matrix (egv_sim_matrix_fwd) and the metric functions of
egovlp_amd.model.metric rank it on the device; only the final scalars reach the host.

RecallEvaluator scores Recall@K (t2v_metrics / v2t_metrics) straight from the embeddings without ever holding the
[texts, videos] matrix: a chunk of its rows comes from the bf16x3 GEMM, is ranked by the streaming kernels and is dropped."""
import torch

from .. import retrieval_ops
from ..model import metric as module_metric
from ..model.model import sim_matrix, sim_matrix_mm


class RetrievalEvaluator:
    """evaluator = RetrievalEvaluator(["mir_metrics"], annotations); per validation batch evaluator.update(text_embed, vid_embed,
    idx, dl_idx) with the embeddings already gathered over the ranks; evaluator.compute() -> {dl_idx: {metric name: results}}
    (the reference's `nested_val_metrics`) and forgets the batches.

    metrics: names in egovlp_amd.model.metric (as the configs give them) or callables `metric(sims, idx_arr)`.
    annotations: passed on as `annotations=` when given (mir_metrics reads the EPIC files at the reference's paths otherwise)."""

    def __init__(self, metrics, annotations=None, n_loaders=1):
        self.metrics = [getattr(module_metric, m) if isinstance(m, str) else m for m in metrics]
        self.annotations = annotations
        self.n_loaders = n_loaders
        self.reset()

    def reset(self):
        self._text = [[] for _ in range(self.n_loaders)]
        self._vid = [[] for _ in range(self.n_loaders)]
        self._idx = [[] for _ in range(self.n_loaders)]

    def update(self, text_embed, vid_embed, idx, dl_idx=0):
        self._text[dl_idx].append(text_embed.detach())
        self._vid[dl_idx].append(vid_embed.detach())
        self._idx[dl_idx].append(torch.as_tensor(idx).reshape(-1).to(text_embed.device))

    def similarity(self, dl_idx=0):
        """[texts, videos] similarity matrix of everything seen so far, on the embeddings' device."""
        with torch.no_grad():
            return sim_matrix(torch.cat(self._text[dl_idx]), torch.cat(self._vid[dl_idx]))

    def compute(self):
        nested_metrics = {x: {} for x in range(self.n_loaders)}
        kw = {} if self.annotations is None else {"annotations": self.annotations}
        for dl_idx in range(self.n_loaders):
            if not self._text[dl_idx]:
                continue
            sims = self.similarity(dl_idx)
            arr_embeds = torch.cat(self._idx[dl_idx])
            for metric in self.metrics:
                nested_metrics[dl_idx][metric.__name__] = metric(sims, arr_embeds, **kw)
        self.reset()
        return nested_metrics


def chunk_plan(n_rows, n_cols, chunk_bytes):
    """Row boundaries [0, ..., n_rows] of the chunks in which an [n_rows, n_cols] fp32 score matrix is walked: as many whole rows
    as fit into chunk_bytes, one row at least.  A pure function of its arguments."""
    n_rows, n_cols, chunk_bytes = int(n_rows), int(n_cols), int(chunk_bytes)
    if n_rows < 1 or n_cols < 1:
        raise ValueError("chunk_plan: at least one row and one column are needed")
    per = max(1, chunk_bytes // (4 * n_cols))
    return list(range(0, n_rows, per)) + [n_rows]


class RecallEvaluator:
    """evaluator = RecallEvaluator(queries_per_video); per validation batch evaluator.update(text_embed, vid_embed, query_mask,
    dl_idx) with the embeddings already gathered over the ranks: vid_embed [b, D], text_embed [b * queries_per_video, D] with the
    captions of a video next to each other, query_mask (optional, one entry per caption, nonzero = the caption exists);
    evaluator.compute() -> {dl_idx: {"t2v_metrics": {...}, "v2t_metrics": {...}}} and forgets the batches.

    Both sets are normalised once (normalize=True: x / max(|x|, eps), sim_matrix's rule; False: plain inner products).  t2v walks
    the captions in chunks of rows, sim_matrix_mm(text[c0:c1], video); v2t walks the videos, sim_matrix_mm(video[c0:c1], text),
    where the ground truth of a row is a segment of queries_per_video columns and the mask is the column validity.  A chunk holds
    at most chunk_bytes of scores (whole rows, one at least), is ranked and dropped: the ranks are those of the scores the GEMM
    wrote, the bar of a row is read from the chunk it is compared with."""

    def __init__(self, queries_per_video=1, normalize=True, eps=1e-8, chunk_bytes=1 << 30, n_loaders=1):
        if int(queries_per_video) < 1:
            raise ValueError("RecallEvaluator: queries_per_video >= 1 is needed")
        if int(chunk_bytes) < 1:
            raise ValueError("RecallEvaluator: chunk_bytes >= 1 is needed")
        self.qpv, self.normalize, self.eps, self.chunk_bytes = int(queries_per_video), bool(normalize), float(eps), int(chunk_bytes)
        self.n_loaders = n_loaders
        self.reset()

    def reset(self):
        self._text = [[] for _ in range(self.n_loaders)]
        self._vid = [[] for _ in range(self.n_loaders)]
        self._mask = [[] for _ in range(self.n_loaders)]

    def update(self, text_embed, vid_embed, query_mask=None, dl_idx=0):
        if text_embed.dim() != 2 or vid_embed.dim() != 2 or text_embed.shape[1] != vid_embed.shape[1]:
            raise ValueError("RecallEvaluator.update: text_embed [captions, D] and vid_embed [videos, D] of one width are needed")
        if text_embed.shape[0] != self.qpv * vid_embed.shape[0]:
            raise ValueError(f"RecallEvaluator.update: {text_embed.shape[0]} captions for {vid_embed.shape[0]} videos: Nq must be "
                             f"queries_per_video = {self.qpv} times Nv")
        if query_mask is None:
            mask = None
        else:
            mask = torch.as_tensor(query_mask).reshape(-1)
            if mask.numel() != text_embed.shape[0]:
                raise ValueError(f"RecallEvaluator.update: the mask has {mask.numel()} elements, {text_embed.shape[0]} are needed")
            mask = (mask != 0).to(text_embed.device)
        self._text[dl_idx].append(text_embed.detach())
        self._vid[dl_idx].append(vid_embed.detach())
        self._mask[dl_idx].append(mask)

    def _gathered(self, dl_idx):
        """(text [Nq, D], video [Nv, D], mask bool [Nq] or None), normalised when asked for."""
        if not self._text[dl_idx]:
            raise ValueError(f"RecallEvaluator: no batch seen for loader {dl_idx}")
        t, v = torch.cat(self._text[dl_idx]).float(), torch.cat(self._vid[dl_idx]).float()
        mask = None
        if any(m is not None for m in self._mask[dl_idx]):
            mask = torch.cat([torch.ones(x.shape[0], dtype=torch.bool, device=x.device) if m is None else m
                              for m, x in zip(self._mask[dl_idx], self._text[dl_idx])])
        if self.normalize:
            t, v = retrieval_ops.row_normalize(t, self.eps), retrieval_ops.row_normalize(v, self.eps)
        pad = -t.shape[1] % 32                                   # the GEMM walks k in steps of 32: zero columns add exact zeros
        if pad:
            t, v = torch.nn.functional.pad(t, (0, pad)), torch.nn.functional.pad(v, (0, pad))
        return t, v, mask

    def _walk(self, rows, cols, per_chunk):
        """per_chunk(scores [c1 - c0, n_cols], c0) for every chunk of sim_matrix_mm(rows, cols); the results concatenated."""
        out = []
        plan = chunk_plan(rows.shape[0], cols.shape[0], self.chunk_bytes)
        for c0, c1 in zip(plan[:-1], plan[1:]):
            out.append(per_chunk(sim_matrix_mm(rows[c0:c1], cols), c0))
        return out

    def ranks(self, dl_idx=0):
        """(t2v ranks [Nq], v2t ranks [Nv], mask or None): fp64 device vectors, the t2v ones unfiltered."""
        with torch.no_grad():
            t, v, mask = self._gathered(dl_idx)
            nv = v.shape[0]
            r_t = torch.cat(self._walk(t, v, lambda s, c0: retrieval_ops.gt_ranks(s, self.qpv, "t2v", row0=c0, n_videos=nv)))
            r_v = torch.cat(self._walk(v, t, lambda s, c0: retrieval_ops.gt_ranks(s, self.qpv, "v2t", query_masks=mask, row0=c0,
                                                                               n_videos=nv, transposed=False)))
        return r_t, r_v, mask

    def topk(self, k, direction="t2v", dl_idx=0):
        """(values [queries, k], indices [queries, k]) of the k best videos of every caption ("t2v") or the k best existing
        captions of every video ("v2t"); ties by ascending index, -inf / -1 where fewer than k exist."""
        if direction not in ("t2v", "v2t"):
            raise ValueError(f"RecallEvaluator.topk: direction must be 't2v' or 'v2t', not {direction!r}")
        if not 1 <= int(k) <= retrieval_ops.TOPK_MAX:
            raise ValueError(f"RecallEvaluator.topk: k = {k}, 1 <= k <= {retrieval_ops.TOPK_MAX} is needed")
        with torch.no_grad():
            t, v, mask = self._gathered(dl_idx)
            if direction == "t2v":
                parts = self._walk(t, v, lambda s, c0: retrieval_ops.topk_rows(s, k))
            else:
                parts = self._walk(v, t, lambda s, c0: retrieval_ops.topk_rows(s, k, col_valid=mask))
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def compute(self):
        nested_metrics = {x: {} for x in range(self.n_loaders)}
        for dl_idx in range(self.n_loaders):
            if not self._text[dl_idx]:
                continue
            r_t, r_v, mask = self.ranks(dl_idx)
            nested_metrics[dl_idx]["t2v_metrics"] = module_metric._recall_summary(r_t, r_t.numel() if mask is None else mask.sum(),
                                                                                 keep=mask)
            nested_metrics[dl_idx]["v2t_metrics"] = module_metric._recall_summary(r_v, r_v.numel())
        self.reset()
        return nested_metrics
