"""Exponential moving average (EMA) of the model weights, kept on the device (csrc/ema.hip).

The reference keeps no average.  The usual emulation -- `copy.deepcopy(model)`, a Python loop over 327 tensors per step, a second
model for validation -- costs ~650 small launches and a host stall per step, and a second copy of the parameters plus a second
operand-plane cache for evaluation.  Here:

  * the shadow weights are ONE flat fp32 arena (every tensor's view starts 16-byte aligned: the kernels' vector path);
  * `update()` enqueues one decision thread (egv_ema_decide) and one multi-tensor pass (egv_ema_update_multi: e += w * (p - e)), with
    no host synchronisation.  Whether the optimizer step was applied at all (an overflow of the fp16 backward, a non-finite gradient
    norm) is read on the device from the optimizer's own hyper block (`AdamW.skip_flag()`): a step that was not applied neither
    moves the average nor advances the warm-up count;
  * for evaluation, `swap()` / `swapped()` exchange the two weight sets IN PLACE (egv_swap_multi) -- parameter addresses never
    change, so there is no second model and no backup copy; the operand planes follow through `weights.bump_epoch()`.

decay in effect: `warmup` ? min(decay, (1 + t) / (10 + t)) : decay, t = the updates applied so far (the rule of timm's ModelEmaV2 /
torch-ema).  Every rank holds the same parameters after the gradient exchange and therefore the same average: nothing is exchanged.
"""
from __future__ import annotations

import contextlib

import torch

from . import ops, weights


class ModelEMA:
    """ema = ModelEMA(model, decay=0.9999, warmup=True): the shadow starts as the current weights.  Covers every floating-point
    parameter of the unwrapped model (`model.module` if present; any nn.Module will do, e.g. a loss with parameters), whatever its
    requires_grad.  Parameters are fp32, dense and on one device (the package has no other kind)."""

    def __init__(self, model, decay=0.9999, warmup=True):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ModelEMA: 0 <= decay < 1")
        self.decay, self.warmup = float(decay), bool(warmup)
        core = getattr(model, "module", model)
        named = [(k, p) for k, p in core.named_parameters() if p.is_floating_point()]
        if not named:
            raise ValueError("ModelEMA: the model has no floating-point parameter")
        dev = named[0][1].device
        for k, p in named:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("ModelEMA: %s is not a dense contiguous fp32 parameter on %s" % (k, dev))
        self._core = core
        self._names = [k for k, _ in named]
        self._params = [p for _, p in named]
        offsets, cur = [], 0
        for p in self._params:
            offsets.append(cur)
            cur += (p.numel() + 3) // 4 * 4             # every view starts at a multiple of 16 bytes
        self._arena = torch.zeros(max(cur, 4), dtype=torch.float32, device=dev)
        self._views = [self._arena[o:o + p.numel()] for o, p in zip(offsets, self._params)]
        self._state = torch.zeros(8, dtype=torch.int32, device=dev)     # {t, w, skipped, decay in effect, 0, 0, 0, 0}: csrc/ema.hip
        self._tables = None         # ops.PairTables of (shadow, parameter), shared by update and swap
        self._swapped = False
        self.reset()

    def reset(self):
        """shadow := the current weights (one multi-tensor copy), counters := 0."""
        if self._swapped:
            raise RuntimeError("ModelEMA.reset while swapped")
        with torch.no_grad():
            torch._foreach_copy_(self._views, [p.detach().reshape(-1) for p in self._params])
        self._state.zero_()

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def update(self, optimizer=None, skip_flag=None):
        """After optimizer.step(): one decision + one multi-tensor pass, no host synchronisation.  `skip_flag`: a one-element fp32 device
        tensor whose non-zero value means "the last optimizer step was not applied"; default `optimizer.skip_flag()` (None -- always
        applied -- for an optimizer without one)."""
        if self._swapped:
            raise RuntimeError("ModelEMA.update while swapped: the model holds the averaged weights (swap back first)")
        if skip_flag is None and optimizer is not None and hasattr(optimizer, "skip_flag"):
            skip_flag = optimizer.skip_flag()
        ops.ema_decide(self._state, skip_flag, self.decay, self.warmup)
        self._tables = ops.ema_update_multi(self._views, self._params, self._state, self._tables)

    # ---- evaluation under the averaged weights --------------------------------------------------------------------------------------
    def swap(self):
        """Exchange parameters and shadow in place.  The parameters were written through raw pointers: weights.bump_epoch()."""
        self._tables = ops.swap_multi(self._views, self._params, self._tables)
        self._swapped = not self._swapped
        weights.bump_epoch()

    @contextlib.contextmanager
    def swapped(self):
        """with ema.swapped(): the model holds the averaged weights; they are swapped back on exit, whatever happens inside."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def is_swapped(self):
        return self._swapped

    def copy_to(self, model=None):
        """Overwrite the parameters of `model` (default: the model this average follows) with the averaged weights."""
        if self._swapped:
            raise RuntimeError("ModelEMA.copy_to while swapped")
        if model is None:
            dst = self._params
        else:
            own = dict(getattr(model, "module", model).named_parameters())
            missing = [k for k, v in zip(self._names, self._views) if k not in own or own[k].numel() != v.numel()]
            if missing:
                raise KeyError("ModelEMA.copy_to: the model lacks (or has another size of) %s" % missing[:4])
            dst = [own[k] for k in self._names]
        with torch.no_grad():
            torch._foreach_copy_([p.detach().reshape(-1) for p in dst], self._views)
        weights.bump_epoch()

    # ---- host readbacks (synchronise: logs, tests, checkpoints) ---------------------------------------------------------------------
    def num_updates(self):
        return int(self._state[0].item())

    def skipped_updates(self):
        return int(self._state[2].item())

    def current_decay(self):
        """The decay the last applied update ran with (0.0 before the first)."""
        return float(self._state.view(torch.float32)[3].item())

    @property
    def shadow(self):
        """{parameter name: fp32 view of the arena, in the parameter's shape}: the averaged weights (the training weights while swapped)."""
        return {k: v.view(p.shape) for k, v, p in zip(self._names, self._views, self._params)}

    def arena_bytes(self):
        return self._arena.numel() * 4

    def state_dict(self):
        """{'shadow': {name: cpu fp32 tensor}, 'num_updates', 'skipped', 'decay', 'warmup'}.  'shadow' loads into the model's own
        `load_state_dict(..., strict=False)` as it is: how the averaged model is shipped.  While swapped the averaged weights are read
        from where they are, the parameters."""
        src = self._params if self._swapped else self._views
        st = self._state.cpu()
        return {"shadow": {k: s.detach().cpu().clone().view(p.shape) for k, s, p in zip(self._names, src, self._params)},
                "num_updates": int(st[0]), "skipped": int(st[2]), "decay": self.decay, "warmup": self.warmup}

    def load_state_dict(self, d):
        """Restores the averaged weights and the two counters; names and shapes are checked strictly.  decay / warmup stay what the
        constructor was given (a resumed run may change them)."""
        if self._swapped:
            raise RuntimeError("ModelEMA.load_state_dict while swapped")
        sh = d["shadow"]
        if set(sh) != set(self._names):
            missing, extra = sorted(set(self._names) - set(sh)), sorted(set(sh) - set(self._names))
            raise KeyError("ModelEMA.load_state_dict: missing %s, unexpected %s" % (missing[:4], extra[:4]))
        for k, p in zip(self._names, self._params):
            if tuple(sh[k].shape) != tuple(p.shape):
                raise ValueError("ModelEMA.load_state_dict: %s has shape %s, the parameter %s" % (k, tuple(sh[k].shape), tuple(p.shape)))
        with torch.no_grad():
            torch._foreach_copy_(self._views, [sh[k].detach().to(torch.float32).reshape(-1) for k in self._names])
        host = torch.zeros(8, dtype=torch.int32)
        host[0], host[2] = int(d.get("num_updates", 0)), int(d.get("skipped", 0))
        self._state.copy_(host)
