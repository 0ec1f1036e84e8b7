"""What the five trainers share: the two ends of an optimisation step, the prefetching host-to-device feed and `TrainerBase`
(constructor, LR rule, precision guard, host batch order and the training epoch of the reference's trainer files, which repeat
them line for line: trainer/trainer_egoclip.py:29-180 == trainer_epic.py:29-171 == trainer_oscc.py:237-380 ...)."""
from __future__ import annotations

import numpy as np
import torch

from ..base.base_trainer import Multi_BaseTrainer_dist
from ..gather import AllGather_multi


def step_prologue(model, optimizer, scaler):
    """Opens egoclip_step / retrieval_step / classification_step -> (the unwrapped model, its execution context, the scaler):
    `scaler` defaults to the model's own when its backward precision is 'f16'; then zero_grad."""
    core = getattr(model, 'module', model)
    ec = getattr(core, 'exec_ctx', None)
    if scaler is None and ec is not None and ec.bwd_passes == 4:
        # fp16 gradient planes flush un-scaled gradients of 1e-6 to zero: the model's own scaler (on the device its parameters live on)
        scaler = ec.loss_scaler(device=next(core.parameters()).device)
    optimizer.zero_grad(set_to_none=True)
    return core, ec, scaler


def step_epilogue(loss, ec, optimizer, grad_sync, scaler):
    """Closes the three steps: (scaled) backward, wait for the side stream and the gradient exchange, optimizer.step.
    -> the detached (device) loss; no host sync."""
    (loss if scaler is None else scaler.scale(loss)).backward()
    if ec is not None:
        ec.join_side_stream()       # idempotent; covers a backward whose end-of-pass callback did not run
    if grad_sync is not None:
        grad_sync.finish()
    if scaler is None:
        optimizer.step()
    else:
        optimizer.step(scaler=scaler)
    return loss.detach()


def clamp_loss_scale(loss_fn):
    """After optimizer.step of the EgoClip steps: a loss with a learnable temperature (EgoNCE / NormSoftmaxLoss with
    `learnable_temperature=True`; SigmoidLoss / EgoSigmoidLoss with `learnable=True`, which set the same attribute) clamps its logit
    scale (one tiny device op, no synchronisation); any other loss: nothing is called."""
    if getattr(loss_fn, 'learnable_temperature', False):
        loss_fn.clamp_logit_scale_()


def register_loss_parameters(optimizer, loss_fn, lr=None):
    """The reference builds its optimizer from `model.parameters()` only (run/train_egoclip.py:72-73); a loss with parameters of its
    own (EgoNCE / NormSoftmaxLoss with `learnable_temperature=True`: the logit scale; SigmoidLoss / EgoSigmoidLoss: the logit scale and
    the logit bias, both in the one group) gets ONE more parameter group here:
    weight_decay 0, `lr` defaulting to the first group's.  Parameters the optimizer already holds are left where they are (calling
    this twice adds nothing).  -> the new group, or None when there was nothing to add."""
    if not hasattr(loss_fn, 'parameters'):
        return None
    held = {id(p) for g in optimizer.param_groups for p in g['params']}
    params = [p for p in loss_fn.parameters() if p.requires_grad and id(p) not in held]
    if not params:
        return None
    own_lr = lr is not None
    optimizer.add_param_group({'params': params, 'weight_decay': 0.0, 'lr': float(lr) if own_lr else optimizer.param_groups[0]['lr'],
                               'loss_parameters': True, 'base_lr': float(lr) if own_lr else None})
    return optimizer.param_groups[-1]


def egoclip_head_loss(loss_fn, text_embeds, video_embeds, n_embeds, v_embeds, fused_head=True):
    """Similarity + loss of the EgoClip step on the (gathered) global batch, trainer/trainer_egoclip.py:130-137 -- shared by
    `egoclip_step` and `egoclip_step_cached`."""
    from ..model.model import sim_matrix
    # EgoNCE, and any loss that says so (EgoSigmoidLoss), takes the noun / verb vectors; the others the embeddings alone
    is_ego = type(loss_fn).__name__ == 'EgoNCE' or bool(getattr(loss_fn, 'takes_noun_verb', False))
    n, D = text_embeds.shape
    # the one-call head covers global batches up to 65 536 rows of <= 256 features: the latency-bound kernels up to 1 024 rows, the
    # tiled fp32-MFMA ones beyond (loss_ops.egonce_fwd_bwd switches); anything else, or fused_head=False, takes the API-compatible
    # sim_matrix + loss.forward path (n <= 4096)
    if fused_head and hasattr(loss_fn, 'fused') and n <= 65536 and D <= 256 and D % 4 == 0:
        return loss_fn.fused(text_embeds, video_embeds, n_embeds, v_embeds) if is_ego \
            else loss_fn.fused(text_embeds, video_embeds)
    if getattr(loss_fn, 'queue_size', 0):
        loss_fn._refuse_matrix_path()           # a queue in train() mode lives in `fused` only: a ValueError that says so
    output = sim_matrix(text_embeds, video_embeds)                          # :130
    if is_ego:
        sim_v = sim_matrix(v_embeds, v_embeds)                              # :133
        sim_n = sim_matrix(n_embeds, n_embeds)                              # :134
        return loss_fn(output, sim_v, sim_n)                                # :135
    return loss_fn(output)


def _to_device_async(data, device, stream):
    """Host batch -> device on `stream`: tensors go through pinned staging copies (a pageable source makes the copy synchronous);
    -> (device batch, event of the last copy).  Keys that are not tensors are passed through."""
    out = {}

    def put(t):
        if not torch.is_tensor(t) or t.device.type != 'cpu' or torch.device(device).type != 'cuda':
            return t.to(device) if torch.is_tensor(t) else t
        src = t if t.is_pinned() else t.contiguous().pin_memory()
        return src.to(device, non_blocking=True)
    if torch.device(device).type == 'cuda':
        with torch.cuda.stream(stream):
            for k, v in data.items():
                out[k] = {kk: put(vv) for kk, vv in v.items()} if isinstance(v, dict) or hasattr(v, 'items') else put(v)
            ev = torch.cuda.Event()
            ev.record(stream)
        return out, ev
    for k, v in data.items():
        out[k] = {kk: put(vv) for kk, vv in v.items()} if isinstance(v, dict) or hasattr(v, 'items') else put(v)
    return out, None


def _prefetched(host_iter, device):
    """Yield (batch_idx, dl_idx, device batch) with the copy of batch i + 1 in flight on a copy stream while batch i is consumed;
    ends with (None, None, None)."""
    cuda = torch.device(device).type == 'cuda'
    stream = torch.cuda.Stream() if cuda else None
    it = iter(host_iter)

    def start():
        try:
            bi, di, data = next(it)
        except StopIteration:
            return None
        dev, ev = _to_device_async(data, device, stream)
        return bi, di, dev, ev
    nxt = start()
    while nxt is not None:
        bi, di, dev, ev = nxt
        nxt = start()                    # the next batch's host work + copy start BEFORE this batch's step is enqueued
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)
            for v in dev.values():       # the tensors were allocated on the copy stream: tell the allocator who uses them
                for t in (v.values() if isinstance(v, dict) else [v]):
                    if torch.is_tensor(t) and t.is_cuda:
                        t.record_stream(torch.cuda.current_stream())
        yield bi, di, dev
    yield None, None, None


class TrainerBase(Multi_BaseTrainer_dist):
    """The reference's trainer constructor and training hot loop (trainer/trainer_egoclip.py:29-180); `train()` / checkpointing
    come from egovlp_amd.base.Multi_BaseTrainer_dist.  A trainer adds `_step` (its optimisation step), `_valid_epoch` and, where
    its batches need other host work than tokenising, `_host_batch`."""

    fused_head = True               # False: the steps take the reference's own decomposition (sim_matrix + loss / projection + loss)
    _guard = None

    def __init__(self, args, model, loss, metrics, optimizer, config, data_loader, valid_data_loader=None,
                 lr_scheduler=None, len_epoch=None, writer=None, visualizer=None, tokenizer=None,
                 max_samples_per_epoch=50000):
        super().__init__(args, model, loss, metrics, optimizer, config, writer)
        self.config = config
        self.args = args
        self.data_loader = data_loader
        self.len_epoch = min(len(x) for x in data_loader) if len_epoch is None else len_epoch    # epoch-based training (:44-47)
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

    def _host_batch(self, data):
        """Host-side preparation of one loader batch before it is staged for the device: the captions are tokenised."""
        if self.tokenizer is not None:
            data['text'] = self.tokenizer(data['text'], return_tensors='pt', padding=True, truncation=True)
        return data

    def _host_batches(self):
        """(batch_idx, dl_idx, data on the HOST) in the reference's order and with its stopping rules (:104-108,158-159)."""
        for batch_idx, data_li in enumerate(zip(*self.data_loader)):
            if (batch_idx + 1) * self.total_batch_sum > self.max_samples_per_epoch:
                break
            for dl_idx, data in enumerate(data_li):
                yield batch_idx, dl_idx, self._host_batch(data)
            if batch_idx == self.len_epoch:
                break

    def _adjust_learning_rate(self, optimizer, epoch, args):
        lr = args.learning_rate1                                            # :75-80
        decay = 1.
        for milestone in args.schedule:
            lr *= 0.1 if epoch >= milestone else 1.
            decay *= 0.1 if epoch >= milestone else 1.
        for param_group in optimizer.param_groups:
            # the loss's group keeps a learning rate of its own (args.temperature_lr) under the same schedule
            own = param_group.get('base_lr') if param_group.get('loss_parameters') else None
            param_group['lr'] = lr if own is None else own * decay

    def _step(self, data):
        """The optimisation step of one device batch -> its (device) loss."""
        raise NotImplementedError

    def _guard_batch(self, data):
        """What the precision guard measures the policy on: the device batch (a trainer whose step runs the batch in pieces hands
        over one piece)."""
        return data

    def _train_epoch(self, epoch):
        self.model.train()
        total_loss = [torch.zeros((), device=self.device) for _ in self.data_loader]
        for loader in self.data_loader:
            if hasattr(loader, 'train_sampler'):
                loader.train_sampler.set_epoch(epoch)                       # :101-102
        # The reference moves every batch to the device with blocking `.to(device)` calls on the compute stream right before the
        # step (:115-121).  Here the NEXT batch is prepared (negatives concatenated, captions tokenised), staged in pinned host
        # memory and copied on a private copy stream while the current step runs; the step only waits for the copy's event.
        feed = _prefetched(self._host_batches(), self.device)
        # `args.model_ema_decay`: the weight average (egovlp_amd.ema.ModelEMA), built here from the weights on the device before the
        # first step; None when the option is off, and then no line below does anything
        ema = self._model_ema()
        for batch_idx, dl_idx, data in feed:
            if batch_idx is None:
                break
            # the per-block precision policy is measured on the weights at hand: first batch, then every `precision_guard_interval`
            # steps (egovlp_amd.guard.PrecisionGuard; a no-op unless the forward runs fp16 products)
            if self._guard is None:
                from ..guard import PrecisionGuard
                self._guard = PrecisionGuard(self.model, interval=int(getattr(self.args, 'precision_guard_interval', 1000)))
            self._guard.maybe_check(self._guard_batch(data))
            loss = self._step(data)
            if ema is not None:
                ema.update(self.optimizer)  # one decision + one multi-tensor pass per OPTIMIZER step (a cached step's chunks share it)
            total_loss[dl_idx] += loss      # stays on the device: no per-step .item() sync (reference :148,150)
            if self.writer is not None and self.args.rank == 0 and batch_idx % self.log_step == 0:
                total = int(self.data_loader[dl_idx].n_samples / self.n_gpu) if hasattr(self.data_loader[dl_idx], 'n_samples') else 0
                current = batch_idx * self.data_loader[dl_idx].batch_size
                self.writer.add_scalar(f'Loss_training/loss_{dl_idx}', float(loss), (epoch - 1) * total + current)   # :143-148
                if getattr(getattr(self, 'loss', None), 'learnable_temperature', False):   # float(loss) has just synchronised: the read-back is free
                    self.writer.add_scalar(f'Loss_training/temperature_{dl_idx}', self.loss.current_temperature(), (epoch - 1) * total + current)
                if getattr(getattr(self, 'loss', None), 'queue_size', 0):                   # a loss with a queue of past embeddings: its valid rows
                    self.writer.add_scalar(f'Loss_training/queue_filled_{dl_idx}', self.loss.queue_filled(), (epoch - 1) * total + current)
                if hasattr(getattr(self, 'loss', None), 'current_bias'):                    # the sigmoid losses: their second parameter
                    self.writer.add_scalar(f'Loss_training/bias_{dl_idx}', self.loss.current_bias(), (epoch - 1) * total + current)
                if getattr(self, 'last_mix_lambda', None) is not None:                      # Mixup / CutMix on: the mean lam of this step's draw
                    self.writer.add_scalar(f'Loss_training/mix_lambda_{dl_idx}', self.last_mix_lambda, (epoch - 1) * total + current)
                if ema is not None:                                                         # the decay the average has just run with
                    self.writer.add_scalar(f'Loss_training/ema_decay_{dl_idx}', ema.current_decay(), (epoch - 1) * total + current)
                # gradient clipping on: the step's un-scaled pre-clip norm and its coefficient, read back where float(loss) has
                # just synchronised anyway (off: nothing is computed, nothing is read)
                if getattr(self.optimizer, 'max_grad_norm', None) is not None:
                    self.writer.add_scalar(f'Grad_training/grad_norm_{dl_idx}', self.optimizer.grad_norm(), (epoch - 1) * total + current)
                    self.writer.add_scalar(f'Grad_training/clip_coef_{dl_idx}', self.optimizer.clip_coef(), (epoch - 1) * total + current)
                # LAMB: the smallest and the largest trust ratio of the step, next to the norm (the same free read-back)
                ratios = self.optimizer.trust_ratios() if hasattr(self.optimizer, 'trust_ratios') else None
                if ratios is not None and ratios.numel():
                    self.writer.add_scalar(f'Grad_training/trust_ratio_min_{dl_idx}', float(ratios.min()), (epoch - 1) * total + current)
                    self.writer.add_scalar(f'Grad_training/trust_ratio_max_{dl_idx}', float(ratios.max()), (epoch - 1) * total + current)
        log = {f'loss_{dl_idx}': float(total_loss[dl_idx]) / self.len_epoch for dl_idx in range(len(self.data_loader))}   # :162-164
        if self.writer is not None and self.args.rank == 0:
            for dl_idx in range(len(self.data_loader)):
                self.writer.add_scalar(f'Loss_training/loss_total_{dl_idx}', log[f'loss_{dl_idx}'], epoch - 1)
        if self.do_validation:                                              # :172-175
            val_log = self._validate(epoch)             # `_valid_epoch`, under the averaged weights with args.model_ema_eval
            if self.args.rank == 0:
                log.update(val_log)
        self._adjust_learning_rate(self.optimizer, epoch, self.args)        # :178
        return log
