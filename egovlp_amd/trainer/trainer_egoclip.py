"""EgoClip pre-training step -- drop-in for the reference's trainer/trainer_egoclip.py.

`egoclip_step` is the optimisation step (:123-141); `Multi_Trainer_dist` is the reference's trainer class on the shared
`TrainerBase` (trainer/common.py: constructor, prefetching batch feed, LR rule, epoch loop) with the scene-aware negatives
of the EgoClip batches and the EgoMCQ validation.  The gathers (`AllGather_multi`, `AllGatherFused`: egovlp_amd/gather.py) and
the batch feed (`_prefetched`) are importable from here as they are in the reference's file.
"""
from __future__ import annotations

import torch

from ..gather import AllGather_multi  # noqa: F401  (re-exported, as the reference file has it)
from ..gather import AllGatherFused, _gather_rows, _world
from ..model.model import sim_matrix
from .common import _prefetched  # noqa: F401  (re-exported: the feed of the epoch loop, timed on its own by bench.py)
from .cached_step import egoclip_step_cached  # noqa: F401  (re-exported: the same step over a batch larger than memory)
from .common import TrainerBase, clamp_loss_scale, egoclip_head_loss, step_epilogue, step_prologue
from .common import register_loss_parameters  # noqa: F401  (re-exported: the optimizer group of a loss with parameters)


def _pad_tokens(text, multiple):
    """Right-pad input_ids (0 = [PAD]) and attention_mask (0 = masked) to a multiple of `multiple` tokens."""
    L = text['input_ids'].shape[1]
    Lp = (L + multiple - 1) // multiple * multiple
    if Lp == L:
        return text
    return {k: torch.nn.functional.pad(v, (0, Lp - L), value=0) for k, v in text.items()}


def egoclip_step(model, loss_fn, optimizer, data, world_size=1, rank=0, fused_head=True, grad_sync=None, scaler=None):
    """One optimisation step = trainer/trainer_egoclip.py:123-141 (zero_grad, forward, gathers,
    similarity + loss, backward, optimizer.step).  Returns the (device) loss tensor; no host sync.
    `grad_sync` (egovlp_amd.dist.Bf16GradSync, world size > 1) averages the gradients over the ranks -- its all-reduces
    are launched by grad-ready hooks during backward; `finish()` waits for them before the optimizer reads p.grad.
    `scaler` (egovlp_amd.optim.LossScaler; default when the model's backward precision is 'f16': exec_ctx.loss_scaler()): the loss is multiplied by the device-side
    loss scale before backward() and the optimizer un-scales, or skips the step after an overflow -- no host synchronisation.
    A `loss_fn` with a learnable temperature (its `logit_scale` must be in the optimizer: `register_loss_parameters`) gets that
    parameter's gradient from the head's own node, and its clamp runs after optimizer.step."""
    _, ec, scaler = step_prologue(model, optimizer, scaler)
    text_embeds, video_embeds = model(data)
    n_embeds, v_embeds = data['noun_vec'], data['verb_vec']
    video_embeds, text_embeds, n_embeds, v_embeds = AllGatherFused.apply(
        video_embeds, text_embeds, n_embeds, v_embeds, world_size, rank)
    loss = egoclip_head_loss(loss_fn, text_embeds, video_embeds, n_embeds, v_embeds, fused_head)   # :130-137
    loss = step_epilogue(loss, ec, optimizer, grad_sync, scaler)            # :139-141
    clamp_loss_scale(loss_fn)               # a learnable temperature: clamp the logit scale the optimizer has just moved
    return loss


class Multi_Trainer_dist(TrainerBase):
    """Drop-in for the reference's trainer class (trainer/trainer_egoclip.py:29-275): same constructor, `train()` /
    checkpointing from the base class (egovlp_amd.base.Multi_BaseTrainer_dist == base/base_trainer.py:239-480), the
    training hot loop `_train_epoch` (:82-180; TrainerBase) and the EgoMCQ validation `_valid_epoch` (:182-275)."""

    def _host_batch(self, data):
        if 'video_neg' in data.keys():                                      # :109-113, scene-aware negatives: B -> 2B
            data['text'] = data['text'] + data['text_neg']
            data['video'] = torch.cat((data['video'], data['video_neg']), axis=0)
            data['noun_vec'] = torch.cat((data['noun_vec'], data['noun_vec_neg']), axis=0)
            data['verb_vec'] = torch.cat((data['verb_vec'], data['verb_vec_neg']), axis=0)
            for k in ('text_neg', 'video_neg', 'noun_vec_neg', 'verb_vec_neg'):
                data.pop(k, None)        # concatenated above: not staged / copied to the device a second time
        return super()._host_batch(data)

    def _embed_cache_chunk(self):
        """`args.embed_cache_chunk` > 0: the step re-encodes its batch in chunks of that many rows (egoclip_step_cached) -- the
        contrastive batch is then no longer bounded by the activations that fit in memory."""
        return int(getattr(self.args, 'embed_cache_chunk', 0) or 0)

    def _guard_batch(self, data):
        chunk = self._embed_cache_chunk()
        return {'video': data['video'][:chunk]} if chunk > 0 else data       # the guard's forwards must fit where a chunk fits

    def _step(self, data):
        chunk = self._embed_cache_chunk()
        if chunk > 0:
            return egoclip_step_cached(self.model, self.loss, self.optimizer, data, chunk, self.n_gpu, self.args.rank,
                                       grad_sync=self.grad_sync, fused_head=self.fused_head)
        return egoclip_step(self.model, self.loss, self.optimizer, data, self.n_gpu, self.args.rank,
                            fused_head=self.fused_head, grad_sync=self.grad_sync)

    def _valid_epoch(self, epoch):
        """EgoMCQ validation = reference trainer/trainer_egoclip.py:182-275: for every question the text query and its five
        candidate clips go through the same encoders in eval mode (`model(data, return_embeds=True)`, :211), the prediction
        is `sim_matrix(text, video)` [1, 5] (:214), predictions / answers / types are all-gathered over the ranks (:225-235)
        and scored by the configured metrics (model/metric.py:218-234).  Differences: the gathers are one collective each
        (`all_gather_into_tensor`) and are skipped without a process group; results stay on the device until the end."""
        self.model.eval()
        # one query + five clips per question is ~330 launches for ~3 ms of GPU work: with `args.graph_eval` the forward is
        # captured once per input shape into a HIP graph and replayed (egovlp_amd/graph.py); queries are padded to a multiple
        # of 8 tokens (masked keys contribute exact zeros) so that a handful of graphs covers every caption length
        fwd = None
        if getattr(self.args, 'graph_eval', False):
            from ..graph import GraphedForward
            fwd = GraphedForward(self.model)
            self.last_graphed_forward = fwd
        n_loaders = len(self.valid_data_loader)
        gt_arr = {x: [] for x in range(n_loaders)}
        pred_arr = {x: [] for x in range(n_loaders)}
        type_arr = {x: [] for x in range(n_loaders)}
        world = _world()
        with torch.no_grad():
            for dl_idx, dl in enumerate(self.valid_data_loader):
                for data in dl:
                    data['video'] = data['video'][0]                                    # remove batch (:205)
                    if self.tokenizer is not None:
                        data['text'] = self.tokenizer(data['text'], return_tensors='pt', padding=True, truncation=True)
                    data['text'] = {key: val.to(self.device) for key, val in data['text'].items()}
                    data['video'] = data['video'].to(self.device)
                    if fwd is not None:
                        data['text'] = _pad_tokens(data['text'], 8)
                        text_embed, vid_embed = fwd(data)
                        text_embed, vid_embed = text_embed.clone(), vid_embed.clone()  # the graph's static outputs
                    else:
                        text_embed, vid_embed = self.model(data, return_embeds=True)   # :211
                    data_gt = data['correct'][0].to(self.device).unsqueeze(0)
                    data_pred = sim_matrix(text_embed, vid_embed)                        # :214
                    data_type = data['type'][0].to(self.device).unsqueeze(0)
                    gt_arr[dl_idx].append(_gather_rows(data_gt, world))
                    pred_arr[dl_idx].append(_gather_rows(data_pred, world))
                    type_arr[dl_idx].append(_gather_rows(data_type, world))
        nested_metrics = {x: {} for x in range(n_loaders)}
        for dl_idx in range(n_loaders):
            gt_cat = torch.cat(gt_arr[dl_idx]).cpu()
            pred_cat = torch.cat(pred_arr[dl_idx]).cpu()
            type_cat = torch.cat(type_arr[dl_idx]).cpu()
            for metric in self.metrics:
                nested_metrics[dl_idx][metric.__name__] = metric(pred_cat, gt_cat, type_cat)
        res_dict = {}
        if self.args.rank == 0:
            res_dict = {f'val_loss_{dl_idx}': 0.0 for dl_idx in range(n_loaders)}       # the reference never accumulates it (:192)
            res_dict['nested_val_metrics'] = nested_metrics
        self.last_val_predictions = {x: torch.cat(pred_arr[x]).cpu() for x in range(n_loaders)}
        return res_dict
