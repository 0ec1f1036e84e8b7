"""EPIC-Kitchens-100 multi-instance-retrieval fine-tuning -- drop-in for the reference's trainer/trainer_epic.py.

`retrieval_step` is the optimisation step of the two retrieval fine-tunes (trainer/trainer_epic.py:118-132,
trainer/trainer_charades.py the same lines): zero_grad, forward, gather over the ranks, similarity + ranking loss, backward,
optimizer.step.  What differs from the reference, as in the EgoClip step: the embeddings (and, for
AdaptiveMaxMarginRankingLoss, the per-row weight `data['relation']` the reference has commented out at :116,124,128) cross the
ranks in ONE collective, and similarity + loss + both embedding gradients are ONE C call (`loss.fused`,
egv_maxmargin_head_fwd_bwd: deterministic, nothing n x n in memory) instead of sim_matrix, the loss and their two autograd nodes.

`Multi_Trainer_dist_MIR` keeps the reference's constructor and `train()` flow (egovlp_amd.base.Multi_BaseTrainer_dist), feeds
the step through the prefetching loader of the EgoClip trainer and validates with `RetrievalEvaluator` on the device
(trainer/trainer_epic.py:173-262).  `RetrievalTrainerBase` is what it shares with the Charades-Ego trainer.
"""
from __future__ import annotations

import numpy as np
import torch

from ..base.base_trainer import Multi_BaseTrainer_dist
from ..loss_ops import maxmargin_head_ok
from ..model.model import sim_matrix
from .retrieval_eval import RetrievalEvaluator
from .trainer_egoclip import AllGather_multi, AllGatherRows, _gather_rows, _prefetched, _world


def retrieval_step(model, loss_fn, optimizer, data, world_size=1, rank=0, fused_head=True, grad_sync=None, scaler=None):
    """One fine-tuning step on a batch {'video', 'text'[, 'relation']} already on the device.  Returns the (device) loss tensor;
    no host sync.  `grad_sync` / `scaler`: as egoclip_step (the fp16 backward runs on the loss times the model's device-side
    loss scale and the optimizer un-scales or skips).  The per-row margin weight of AdaptiveMaxMarginRankingLoss is
    `data['relation']` [B]; MaxMarginRankingLoss ignores it, as in the reference."""
    core = getattr(model, 'module', model)
    ec = getattr(core, 'exec_ctx', None)
    if scaler is None and ec is not None and ec.bwd_passes == 4:
        scaler = ec.loss_scaler(device=next(core.parameters()).device)
    optimizer.zero_grad(set_to_none=True)
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
    # the one-call head covers what the EgoNCE head covers (n <= 1024, D <= 256, D % 4 == 0); beyond that the reference's own
    # decomposition takes over (n <= 4096)
    if fused_head and hasattr(loss_fn, 'fused') and maxmargin_head_ok(n, D):
        loss = loss_fn.fused(text_embeds, video_embeds, weight) if adaptive else loss_fn.fused(text_embeds, video_embeds)
    else:
        output = sim_matrix(text_embeds, video_embeds)                          # :126
        loss = loss_fn(output, weight) if adaptive else loss_fn(output)         # :127-128
    (loss if scaler is None else scaler.scale(loss)).backward()                 # :129
    if ec is not None:
        ec.join_side_stream()
    if grad_sync is not None:
        grad_sync.finish()
    if scaler is None:
        optimizer.step()                                                        # :131
    else:
        optimizer.step(scaler=scaler)
    return loss.detach()


class RetrievalTrainerBase(Multi_BaseTrainer_dist):
    """Constructor, batch feed, LR rule and training epoch shared by the EPIC-MIR and Charades-Ego trainers (the two reference
    files repeat them line for line: trainer/trainer_epic.py:38-171 == trainer/trainer_charades.py:40-173)."""

    def __init__(self, args, model, loss, metrics, optimizer, config, data_loader, valid_data_loader=None,
                 lr_scheduler=None, len_epoch=None, writer=None, visualizer=None, tokenizer=None,
                 max_samples_per_epoch=50000):
        super().__init__(args, model, loss, metrics, optimizer, config, writer)
        self.config = config
        self.args = args
        self.data_loader = data_loader
        self.len_epoch = min(len(x) for x in data_loader) if len_epoch is None else len_epoch    # :44-51
        self.valid_data_loader = valid_data_loader
        self.do_validation = self.valid_data_loader is not None
        self.lr_scheduler = lr_scheduler
        self.visualizer = visualizer
        self.val_chunking = True
        self.metrics = metrics if metrics is not None else []
        self.batch_size = self.data_loader[0].batch_size
        self.log_step = int(np.sqrt(self.batch_size))
        self.total_batch_sum = sum(x.batch_size for x in self.data_loader)
        self.tokenizer = tokenizer
        self.max_samples_per_epoch = max_samples_per_epoch
        self.n_gpu = self.args.world_size
        self.allgather = AllGather_multi.apply
        self.fused_head = True

    def _host_batches(self):
        """(batch_idx, dl_idx, data on the HOST) in the reference's order and with its stopping rules (:104-106,149-150)."""
        for batch_idx, data_li in enumerate(zip(*self.data_loader)):
            if (batch_idx + 1) * self.total_batch_sum > self.max_samples_per_epoch:
                break
            for dl_idx, data in enumerate(data_li):
                if self.tokenizer is not None:
                    data['text'] = self.tokenizer(data['text'], return_tensors='pt', padding=True, truncation=True)
                yield batch_idx, dl_idx, data
            if batch_idx == self.len_epoch:
                break

    def _adjust_learning_rate(self, optimizer, epoch, args):
        lr = args.learning_rate1                                                # :73-78
        for milestone in args.schedule:
            lr *= 0.1 if epoch >= milestone else 1.
        for param_group in optimizer.param_groups:
            param_group['lr'] = lr

    _guard = None

    def _step(self, data):
        """The optimisation step of one device batch -> its (device) loss; the classification trainers put their own here."""
        return retrieval_step(self.model, self.loss, self.optimizer, data, self.n_gpu, self.args.rank,
                              fused_head=self.fused_head, grad_sync=self.grad_sync)

    def _train_epoch(self, epoch):
        self.model.train()
        total_loss = [torch.zeros((), device=self.device) for _ in self.data_loader]
        for loader in self.data_loader:
            if hasattr(loader, 'train_sampler'):
                loader.train_sampler.set_epoch(epoch)                           # :101-102
        # as Multi_Trainer_dist._train_epoch: the next batch is tokenised, staged and copied on a copy stream under the current step
        feed = _prefetched(self._host_batches(), self.device)
        for batch_idx, dl_idx, data in feed:
            if batch_idx is None:
                break
            if self._guard is None:
                from ..guard import PrecisionGuard
                self._guard = PrecisionGuard(self.model, interval=int(getattr(self.args, 'precision_guard_interval', 1000)))
            self._guard.maybe_check(data)
            loss = self._step(data)
            total_loss[dl_idx] += loss          # stays on the device: no per-step .item() sync (reference :141,143)
            if self.writer is not None and self.args.rank == 0 and batch_idx % self.log_step == 0:
                total = int(self.data_loader[dl_idx].n_samples / self.n_gpu) if hasattr(self.data_loader[dl_idx], 'n_samples') else 0
                current = batch_idx * self.data_loader[dl_idx].batch_size
                self.writer.add_scalar(f'Loss_training/loss_{dl_idx}', float(loss), (epoch - 1) * total + current)   # :136-141
        log = {f'loss_{dl_idx}': float(total_loss[dl_idx]) / self.len_epoch for dl_idx in range(len(self.data_loader))}   # :153-155
        if self.writer is not None and self.args.rank == 0:
            for dl_idx in range(len(self.data_loader)):
                self.writer.add_scalar(f'Loss_training/loss_total_{dl_idx}', log[f'loss_{dl_idx}'], epoch - 1)
        if self.do_validation:                                                  # :162-165
            val_log = self._valid_epoch(epoch)
            if self.args.rank == 0:
                log.update(val_log)
        self._adjust_learning_rate(self.optimizer, epoch, self.args)            # :167
        return log

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

    def _val_result(self, nested_metrics):
        res_dict = {}
        if self.args.rank == 0:
            # the reference never accumulates a validation loss (:176), so `monitor: "min val_loss_0"` sees 0.0 there as here
            res_dict = {f'val_loss_{dl_idx}': 0.0 for dl_idx in range(len(self.valid_data_loader))}
            res_dict['nested_val_metrics'] = nested_metrics
        return res_dict

    def _progress(self, batch_idx, dl_idx):
        if hasattr(self.data_loader[dl_idx], 'n_samples'):
            current = batch_idx * self.data_loader[dl_idx].batch_size
            total = int(self.data_loader[dl_idx].n_samples / self.n_gpu)
        else:
            current, total = batch_idx, self.len_epoch
        return '[{}/{} ({:.0f}%)]'.format(current, total, 100.0 * current / total)


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
