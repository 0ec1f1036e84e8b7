"""Validation glue of the classification fine-tunes (OSCC / PNR): what trainer/trainer_oscc.py:_valid_epoch and
trainer/trainer_pnr.py:_valid_epoch do between the forward pass and the logging, kept on the device.

The reference gathers scores, labels (and for PNR state, fps and three frame numbers: seven collectives) per batch, copies every
one of them to the host and scores them in Python loops with an `.item()` per clip (model/metric.py:342-397).  Here each
validation batch is ONE gathered row block (egovlp_amd.loss_ops.ClsLayout) and ONE egv_cls_eval_update call that adds its hits or
keyframe errors to four doubles on the device; the validation loss is summed on the device as well.  Only `compute()` reads them."""
import torch

from .. import loss_ops
from ..model import metric as module_metric

_FROM_COUNTS = {"oscc_metrics": module_metric.oscc_metrics_from_counts, "pnr_metrics": module_metric.pnr_metrics_from_counts}


class ClassificationEvaluator:
    """evaluator = ClassificationEvaluator(["oscc_metrics"]); per validation batch evaluator.update(block, layout, dl_idx) with the
    row block already gathered over the ranks and evaluator.add_loss(loss, dl_idx) with the rank-local loss;
    evaluator.compute() -> ({dl_idx: {metric name: results}}, [sum of the losses per loader]) and starts over.

    metrics: 'oscc_metrics' / 'pnr_metrics' as the configs name them, or the functions of egovlp_amd.model.metric of those names
    (their results are formed from the device accumulators).  keep_blocks: also keep every gathered block (`.blocks[dl_idx]`, on
    the device) -- for checks against the host metric functions, not for training."""

    def __init__(self, metrics, n_loaders=1, keep_blocks=False):
        self.names = [m if isinstance(m, str) else m.__name__ for m in metrics]
        for name in self.names:
            if name not in _FROM_COUNTS:
                raise ValueError(f"{name}: the classification evaluator scores oscc_metrics and pnr_metrics")
        self.n_loaders, self.keep_blocks = n_loaders, keep_blocks
        self.accum = [None] * n_loaders
        self.loss = [None] * n_loaders
        self.reset()

    def reset(self):
        for a in self.accum + self.loss:
            if a is not None:
                a.zero_()
        self.blocks = [[] for _ in range(self.n_loaders)]

    def update(self, block, layout, dl_idx=0):
        if self.accum[dl_idx] is None:
            self.accum[dl_idx] = torch.zeros(4, dtype=torch.float64, device=block.device)
        loss_ops.cls_eval_update(block, layout, self.accum[dl_idx])
        if self.keep_blocks:
            self.blocks[dl_idx].append(block.detach().clone())

    def add_loss(self, loss, dl_idx=0):
        if self.loss[dl_idx] is None:
            self.loss[dl_idx] = torch.zeros((), dtype=torch.float32, device=loss.device)
        self.loss[dl_idx] += loss.detach().reshape(())

    def compute(self):
        nested_metrics = {x: {} for x in range(self.n_loaders)}
        losses = []
        for dl_idx in range(self.n_loaders):
            losses.append(0.0 if self.loss[dl_idx] is None else float(self.loss[dl_idx]))
            if self.accum[dl_idx] is None:
                continue
            accum = self.accum[dl_idx].cpu().tolist()             # the one copy to the host
            for name in self.names:
                nested_metrics[dl_idx][name] = _FROM_COUNTS[name](accum)
        self.reset()
        return nested_metrics, losses
