"""Ego4D object-state-change classification (OSCC) fine-tuning -- drop-in for the reference's trainer/trainer_oscc.py -- and what
it shares with the point-of-no-return trainer (trainer_pnr.py).

`classification_step` is the optimisation step of both (trainer/trainer_oscc.py:330-341, trainer/trainer_pnr.py:331-354):
zero_grad, video tower, the narrow head (vid_proj = Linear(768, 2 | 16 | 17)), gather over the ranks, CrossEntropy (PNR: times
the mean of `state`, target = argmax of the one-hot `labels`, 0 for the all-zero rows of clips without a state change), backward,
optimizer.step.  What differs from the reference: the head is ONE autograd node (`CrossEntropy.fused`: egv_cls_head_fwd, one packed
collective instead of two or three, egv_cls_head_loss_bwd) where the padded-GEMM projection node + gathers + loss node took about
fifteen launches for a [4, 768] x [768, 2] product.  `fused_head=False` (or a shape outside `cls_head_ok`) is that earlier route.

`Multi_Trainer_dist_OSCC` keeps the reference's constructor and `train()` flow; constructor, batch feed, LR rule, precision guard
and epoch loop are TrainerBase's (trainer/common.py).  Validation (:382-467) runs on the device: one forward, one gathered block and one
egv_cls_eval_update per batch, the rank-local validation loss (:428) summed there too (`monitor: "min val_loss_0"`).
"""
from __future__ import annotations

import torch

from .. import loss_ops
from ..gather import AllGatherRows, _gather_rows, _world
from ..data_loader.transforms import mix_params
from ..loss_ops import ClsLayout, cls_head_ok
from .classification_eval import ClassificationEvaluator
from .common import step_epilogue, step_prologue
from .trainer_epic import RetrievalTrainerBase, format_nested_metrics_for_writer  # noqa: F401  (re-exported, as the reference file has it)


def _targets(data, task, device):
    """-> (target [B] int64, state [B] or None): OSCC classifies `state`; PNR localises argmax(labels) and weighs by `state`.
    The argmax is taken locally: it commutes with the gather (trainer/trainer_pnr.py:346,350)."""
    state = data['state'].to(device).reshape(-1)
    if task == 'oscc':
        return state.long(), None
    if task != 'pnr':
        raise ValueError("task is 'oscc' or 'pnr'")
    return torch.argmax(data['labels'].to(device).long(), dim=1), state


def _head(core):
    lin = core.vid_proj[0] if isinstance(core.vid_proj, torch.nn.Sequential) else None
    return lin if isinstance(lin, torch.nn.Linear) else None


def classification_step(model, loss_fn, optimizer, data, world_size=1, rank=0, task='oscc', fused_head=True, grad_sync=None,
                        scaler=None, mix=None):
    """One fine-tuning step on a batch {'video', 'state'[, 'labels']} already on the device.  Returns the (device) loss tensor; no
    host sync.  `grad_sync` / `scaler`: as egoclip_step.
    mix = (mix_idx, mix_lam) (an extension; data_loader.transforms.mix_params): Mixup / CutMix of every clip with its partner inside
    the patch gather (`set_input_mix`), the target lam * target + (1 - lam) * target[partner] -- partners are rank-local, so the
    partner's class is formed here, before the gather, and rides with lam in the step's one collective.  OSCC only: a blended clip
    has no keyframe.  None: the calls made without it."""
    if mix is not None and task == 'pnr':
        raise ValueError("classification_step: Mixup / CutMix does not combine with task='pnr' (a blended clip has no keyframe); "
                         "PNR takes label smoothing only")
    core, ec, scaler = step_prologue(model, optimizer, scaler)                  # trainer_oscc.py:333
    video = data['video']
    target, state = _targets(data, task, video.device)
    lin, B = _head(core), video.shape[0]
    soft = ()
    if mix is not None:
        mix_idx, mix_lam = mix
        core.video_model.set_input_mix(mix_idx, mix_lam)                        # consumed by the forward below, on either route
        partner = mix_idx[:, 0].to(device=video.device, dtype=torch.long).clamp(0, B - 1)   # the clamp of the kernels
        soft = (target[partner], mix_lam.to(device=video.device, dtype=torch.float32))
    if fused_head and hasattr(loss_fn, 'fused') and lin is not None and cls_head_ok(world_size * B, B, lin.in_features, lin.out_features):
        ec.begin_step()
        feats = core.video_model(video)                                         # model/model.py:114, without the projection
        if soft:
            loss = loss_fn.fused(feats, lin.weight, lin.bias, target, state, world_size, rank, ec, target2=soft[0], lam=soft[1])
        else:
            loss = loss_fn.fused(feats, lin.weight, lin.bias, target, state, world_size, rank, ec)   # :335-338 / pnr :341-350
    else:
        scores = model(data, video_only=True)                                   # :335
        if soft:
            scores, target, target2, lam = AllGatherRows.apply(world_size, rank, scores, target, *soft)
            loss = loss_fn(scores, target, target2, lam)
        elif state is None:
            scores, target = AllGatherRows.apply(world_size, rank, scores, target)             # :336-337
            loss = loss_fn(scores, target)                                      # :338
        else:
            scores, target, state = AllGatherRows.apply(world_size, rank, scores, target, state)   # pnr :345-347
            loss = torch.mean(state * loss_fn(scores, target))                  # pnr :350
    return step_epilogue(loss, ec, optimizer, grad_sync, scaler)                # :339-341


class ClassificationTrainerBase(RetrievalTrainerBase):
    """What the OSCC and PNR trainers share: the step, the host batch order without a tokenizer call (the reference's loops make
    none: trainer_oscc.py:328-331) and the validation loop."""

    task = 'oscc'
    keep_val_blocks = False         # checks only: keep every gathered validation block in `last_val_blocks`

    def _host_batch(self, data):
        return data

    MIX_ARGS = ('mixup_alpha', 'cutmix_alpha')      # `args` attributes that switch Mixup / CutMix on (absent or 0: off)
    last_mix_lambda = None                           # mean lam of the step's draw, for the log; None: nothing was drawn

    def _mix_on(self):
        return any(float(getattr(self.args, k, 0) or 0) > 0 for k in self.MIX_ARGS)

    def _draw_mix(self, data):
        """The step's Mixup / CutMix tables from args.mixup_alpha, cutmix_alpha, mix_prob, mix_switch_prob, mix_mode; None when off."""
        return None

    def _step(self, data):
        mix = self._draw_mix(data)
        if mix is None:
            return classification_step(self.model, self.loss, self.optimizer, data, self.n_gpu, self.args.rank, task=self.task,
                                       fused_head=self.fused_head, grad_sync=self.grad_sync)
        return classification_step(self.model, self.loss, self.optimizer, data, self.n_gpu, self.args.rank, task=self.task,
                                   fused_head=self.fused_head, grad_sync=self.grad_sync, mix=mix)

    def _val_columns(self, data):
        """Everything of a validation batch that rides in the row block besides the scores (ClsLayout.fill's arguments)."""
        target, state = _targets(data, self.task, self.device)
        return {'target': target, 'state': state}

    def _valid_epoch(self, epoch):
        self.model.eval()
        n_loaders = len(self.valid_data_loader)
        evaluator = ClassificationEvaluator(self.metrics, n_loaders=n_loaders, keep_blocks=self.keep_val_blocks)
        core = getattr(self.model, 'module', self.model)
        lin, world = _head(core), _world()
        with torch.no_grad():
            for dl_idx, dl in enumerate(self.valid_data_loader):
                for data in dl:
                    video = data['video'].to(self.device)                                        # :403
                    cols = self._val_columns(data)
                    B = video.shape[0]
                    C = lin.out_features if lin is not None else 0
                    if lin is not None and cls_head_ok(world * B, B, lin.in_features, C):
                        lay = ClsLayout(C, self.task, evaluate=True)
                        block = torch.empty((B, lay.ld), dtype=torch.float32, device=self.device)
                        core.exec_ctx.begin_step()
                        loss_ops.cls_head_fwd(core.video_model(video), lin.weight, lin.bias, out=block)      # :406
                        lay.fill(block, **cols)
                        # the rank-local loss on the un-gathered batch (:428, pnr :473)
                        loss = loss_ops.cls_head_loss_bwd(block, C, lay.target, lay.state, want_grad=False)[0]
                    else:
                        scores = self.model({'video': video}, video_only=True)
                        C = scores.shape[1]
                        lay = ClsLayout(C, self.task, evaluate=True)
                        block = torch.empty((B, lay.ld), dtype=torch.float32, device=self.device)
                        block[:, :C] = scores
                        lay.fill(block, **cols)
                        loss = getattr(self.loss, 'hard', self.loss)(scores, cols['target'])     # no smoothing in validation
                        if cols['state'] is not None:
                            loss = torch.mean(cols['state'] * loss)
                    evaluator.add_loss(loss, dl_idx)
                    evaluator.update(_gather_rows(block, world), lay, dl_idx)                    # :415-426, one collective
        self.last_val_blocks = evaluator.blocks
        nested_metrics, losses = evaluator.compute()
        val_loss = [losses[dl_idx] / len(self.valid_data_loader[dl_idx]) for dl_idx in range(n_loaders)]
        for dl_idx in range(n_loaders):
            if self.writer is not None and self.args.rank == 0:
                self.writer.add_scalar(f'Loss_val/loss_total_{dl_idx}', val_loss[dl_idx], epoch - 1)         # :431-434
            for metric_name, res in nested_metrics[dl_idx].items():
                # :449-459; the reference's verbose() of these two trainers takes no `mode`
                self._report(epoch, dl_idx, metric_name, res, lambda mode, **kw: self._verbose(**kw))
        return self._val_result(nested_metrics, val_loss)                                        # :461-465


def verbose(epoch, metrics, name="TEST"):
    """The validation log line of trainer/trainer_oscc.py:479-483."""
    msg = f"{name:s} epoch {epoch}, Acc: {metrics['accuracy']:.1f}"
    print(msg)
    return msg


class Multi_Trainer_dist_OSCC(ClassificationTrainerBase):
    """Drop-in for trainer/trainer_oscc.py:237-477 (configs/ft/oscc.json: projection_dim 2, CrossEntropy, oscc_metrics)."""

    task = 'oscc'
    _verbose = staticmethod(verbose)
    _mix_generator = None

    def _draw_mix(self, data):
        a = self.args
        if not self._mix_on():
            return None
        if self._mix_generator is None:             # a stream of its own per rank: the draws disturb no other random state
            self._mix_generator = torch.Generator().manual_seed(int(getattr(a, 'seed', 0) or 0) * 1000003 + int(getattr(a, 'rank', 0)))
        video = data['video']
        prob = getattr(a, 'mix_prob', None)
        switch = getattr(a, 'mix_switch_prob', None)
        mix = mix_params(video.shape[0], video.shape[-2], video.shape[-1], float(getattr(a, 'mixup_alpha', 0) or 0),
                         float(getattr(a, 'cutmix_alpha', 0) or 0), 1.0 if prob is None else float(prob),
                         0.5 if switch is None else float(switch), getattr(a, 'mix_mode', None) or 'batch', self._mix_generator)
        self.last_mix_lambda = None if mix[0] is None else float(mix[1].mean())         # host tables: no sync
        return None if mix[0] is None else mix
