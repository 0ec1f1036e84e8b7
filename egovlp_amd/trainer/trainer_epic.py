"""EPIC-Kitchens-100 multi-instance-retrieval fine-tuning -- drop-in for the reference's trainer/trainer_epic.py.

`retrieval_step` is the optimisation step of the two retrieval fine-tunes (trainer/trainer_epic.py:118-132,
trainer/trainer_charades.py the same lines): zero_grad, forward, gather over the ranks, similarity + ranking loss, backward,
optimizer.step.  What differs from the reference, as in the EgoClip step: the embeddings (and, for
AdaptiveMaxMarginRankingLoss, the per-row weight `data['relation']` the reference has commented out at :116,124,128) cross the
ranks in ONE collective, and similarity + loss + both embedding gradients are ONE C call (`loss.fused`,
egv_maxmargin_head_fwd_bwd: deterministic, nothing n x n in memory) instead of sim_matrix, the loss and their two autograd nodes.

`Multi_Trainer_dist_MIR` keeps the reference's constructor and `train()` flow (egovlp_amd.base.Multi_BaseTrainer_dist), feeds
the step through the prefetching loader of TrainerBase (trainer/common.py) and validates with `RetrievalEvaluator` on the device
(trainer/trainer_epic.py:173-262).  `RetrievalTrainerBase` is what it shares with the Charades-Ego trainer.
"""
from __future__ import annotations

import torch

from ..gather import AllGatherRows, _gather_rows, _world
from ..loss_ops import maxmargin_head_ok
from ..model.model import sim_matrix
from .common import TrainerBase, step_epilogue, step_prologue
from .retrieval_eval import RetrievalEvaluator


def retrieval_step(model, loss_fn, optimizer, data, world_size=1, rank=0, fused_head=True, grad_sync=None, scaler=None):
    """One fine-tuning step on a batch {'video', 'text'[, 'relation']} already on the device.  Returns the (device) loss tensor;
    no host sync.  `grad_sync` / `scaler`: as egoclip_step (the fp16 backward runs on the loss times the model's device-side
    loss scale and the optimizer un-scales or skips).  The per-row margin weight of AdaptiveMaxMarginRankingLoss is
    `data['relation']` [B]; MaxMarginRankingLoss ignores it, as in the reference."""
    _, ec, scaler = step_prologue(model, optimizer, scaler)
    text_embeds, video_embeds = model(data)                                     # :121
    adaptive = type(loss_fn).__name__ == 'AdaptiveMaxMarginRankingLoss'
    weight = None
    if adaptive:
        if 'relation' not in data:
            raise KeyError("AdaptiveMaxMarginRankingLoss needs the per-row weight data['relation']")
        w = data['relation'].to(video_embeds.device, torch.float32).reshape(-1, 1)
        video_embeds, text_embeds, w = AllGatherRows.apply(world_size, rank, video_embeds, text_embeds, w)   # :123-125
        weight = w.reshape(-1)
    else:
        video_embeds, text_embeds = AllGatherRows.apply(world_size, rank, video_embeds, text_embeds)        # :123-124
    n, D = text_embeds.shape
    # the one-call ranking head covers n <= 1024, D <= 256, D % 4 == 0 (the fine-tunes run small batches; only the EgoNCE head goes
    # further); beyond that the reference's own decomposition takes over (n <= 4096)
    if fused_head and hasattr(loss_fn, 'fused') and maxmargin_head_ok(n, D):
        loss = loss_fn.fused(text_embeds, video_embeds, weight) if adaptive else loss_fn.fused(text_embeds, video_embeds)
    else:
        output = sim_matrix(text_embeds, video_embeds)                          # :126
        loss = loss_fn(output, weight) if adaptive else loss_fn(output)         # :127-128
    return step_epilogue(loss, ec, optimizer, grad_sync, scaler)                # :129-131


class RetrievalTrainerBase(TrainerBase):
    """The step and the validation helpers shared by the EPIC-MIR and Charades-Ego trainers (the classification trainers put
    their own step in `_step` and reuse the helpers); everything else is TrainerBase's."""

    def _step(self, data):
        return retrieval_step(self.model, self.loss, self.optimizer, data, self.n_gpu, self.args.rank,
                              fused_head=self.fused_head, grad_sync=self.grad_sync)

    def _val_batch_to_device(self, data):
        if self.tokenizer is not None:
            data['text'] = self.tokenizer(data['text'], return_tensors='pt', padding=True, truncation=True)
        data['text'] = {key: val.to(self.device) for key, val in data['text'].items()}
        data['video'] = data['video'].to(self.device)
        return data

    def _report(self, epoch, dl_idx, metric_name, res, verbose_fn):
        """Log line and writer scalars of one validation metric (:236-249)."""
        if self.args.rank != 0:
            return
        name = getattr(self.valid_data_loader[dl_idx], 'dataset_name', 'TEST')
        self.logger.info(verbose_fn(epoch=epoch, metrics=res, name=name, mode=metric_name))
        if self.writer is not None:
            for key, val in format_nested_metrics_for_writer(res, mode=metric_name, name=name).items():
                key = key.replace('[', '_').replace(']', '_')
                self.writer.add_scalar(f'Val_metrics_{dl_idx}/{key}', val, epoch - 1)

    def _val_result(self, nested_metrics, val_loss=None):
        """`val_loss`: one value per validation loader; None = the reference never accumulates one (:176), so
        `monitor: "min val_loss_0"` sees 0.0 there as here."""
        res_dict = {}
        if self.args.rank == 0:
            res_dict = {f'val_loss_{dl_idx}': 0.0 if val_loss is None else val_loss[dl_idx]
                        for dl_idx in range(len(self.valid_data_loader))}
            res_dict['nested_val_metrics'] = nested_metrics
        return res_dict


class Multi_Trainer_dist_MIR(RetrievalTrainerBase):
    """Drop-in for trainer/trainer_epic.py:29-275.  `annotations` (attribute; egovlp_amd.model.metric.RetrievalAnnotations or
    None = the EPIC files at the reference's paths) is what mir_metrics scores against."""

    annotations = None

    def _valid_epoch(self, epoch):
        """:173-262 with everything on the device: per batch the embeddings and clip indices (`data['meta']['paths']`) are
        gathered over the ranks and handed to a RetrievalEvaluator; its compute() (one similarity matrix, nDCG / mAP kernels)
        is the `nested_val_metrics`.  Only the final scalars reach the host."""
        self.model.eval()
        n_loaders = len(self.valid_data_loader)
        evaluator = RetrievalEvaluator(self.metrics, annotations=self.annotations, n_loaders=n_loaders)
        world = _world()
        with torch.no_grad():
            for dl_idx, dl in enumerate(self.valid_data_loader):
                for data in dl:
                    idx_embed = data['meta']['paths'].to(self.device)
                    data = self._val_batch_to_device(data)
                    text_embed, vid_embed = self.model(data, return_embeds=True)                 # :196
                    vid_embed, text_embed = AllGatherRows.apply(world, 0, vid_embed, text_embed)   # :205-211, one collective
                    evaluator.update(text_embed, vid_embed, _gather_rows(idx_embed, world), dl_idx)   # :216-219
        nested_metrics = evaluator.compute()
        for dl_idx in range(n_loaders):
            for metric_name, res in nested_metrics[dl_idx].items():
                self._report(epoch, dl_idx, metric_name, res, verbose)
        return self._val_result(nested_metrics)


def verbose(epoch, metrics, mode, name="TEST"):
    """The validation log line of trainer/trainer_epic.py:264-271."""
    keys = ("nDCG_V2T", "nDCG_T2V", "nDCG_AVG")
    msg = f"[{mode}]{name:s} epoch {epoch}, " + ", ".join(f"{k}: {metrics[k]:.3f}" for k in keys) + ",, "
    msg += ", ".join(f"{k}: {metrics[k]:.3f}" for k in ("mAP_V2T", "mAP_T2V", "mAP_AVG"))
    print(msg)
    return msg


def format_nested_metrics_for_writer(metrics, mode, name="TEST"):
    """{'[mode]name_key': value}: the writer keys of trainer/trainer_epic.py:273-278."""
    return {f"[{mode}]{name}_{key}": val for key, val in metrics.items()}
