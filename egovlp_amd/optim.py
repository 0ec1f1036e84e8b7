"""AdamW with transformers==4.2.1 semantics on the fused multi-tensor kernel (egv_adamw_multi).

The reference builds its optimizer with `config.initialize('optimizer', transformers, params)`
(run/train_egoclip.py:72-73) -> `transformers.AdamW(lr=3e-5)` with that version's defaults
betas (0.9, 0.999), eps 1e-6, weight_decay 0.0, correct_bias True.  transformers 5.x no longer
ships AdamW, so this module is what `optimizer.type == "AdamW"` resolves to.  `LAMB` (no counterpart in the reference) is AdamW's
step with another update: layer-wise adaptive rates for large effective batches, on the three kernels of csrc/lamb.hip.

(An `overlap_backward()` mode -- updates enqueued from grad-ready hooks under the rest of backward -- was built in round 2,
measured 1.8 % SLOWER (the persistent GEMM workgroups own every CU, a 5-GB HBM stream squeezed into their tails only delays
them; profiles/r02_w_*) and removed in round 4.)
"""
import torch

from . import ops, weights


class LossScaler:
    """Dynamic loss scale of the fp16 backward (`exec_ctx.set_precision('f16mix', 'f16')`): torch.cuda.amp.GradScaler's rule, decided
    entirely on the device.  The reference back-propagates in fp32 (trainer/trainer_egoclip.py:139-141) and needs none of this; fp16
    gradient planes need the loss multiplied by S (here: `scaler.scale(loss).backward()`), and

      * S, the found-inf flag, the good-step counter and the number of skipped steps live in ONE 32-byte device block (`state`);
      * `AdamW.step(scaler=...)` enqueues: a scan of every gradient for inf / NaN (egv_grad_nonfinite_multi), the one-thread decision
        kernel (egv_loss_scale_update: overflow -> skip + S *= backoff_factor; growth_interval good steps in a row -> S *= growth_factor)
        and the AdamW kernels, which read {lr, step size, 1 / S, skip} from the block and do NOTHING in a skipped step;
      * the host never reads any of it back during training (no synchronisation per step); `get_scale()` / `skipped_steps()` do, for
        logs and tests.  The bias correction counts APPLIED steps (host step count minus the device's skipped count).
    Overflow is detectable because gradient planes are written UN-clamped (csrc/f16x2.h f16_grad_piece8): a value beyond fp16's range
    becomes inf and poisons every gradient behind it."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, max_scale=2.0 ** 24, device="cuda"):
        if not (init_scale >= 1.0 and growth_factor >= 1.0 and 0.0 < backoff_factor <= 1.0 and growth_interval >= 1 and max_scale >= init_scale):
            raise ValueError("LossScaler: init_scale >= 1, growth_factor >= 1, 0 < backoff_factor <= 1, growth_interval >= 1, max_scale >= init_scale")
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval, self.max_scale = int(growth_interval), float(max_scale)
        host = torch.zeros(8, dtype=torch.int32)
        host.view(torch.float32)[0] = float(init_scale)
        host.view(torch.float32)[6] = 1.0 / float(init_scale)
        self.state = host.to(device)
        self._f = self.state.view(torch.float32)
        self.scale_tensor = self._f[0]          # 0-dim view: `loss * scale_tensor` reads S when the multiplication RUNS on the stream
        self._extra_hyper = {}                  # parameter-group index > 0 -> its own {lr, step_size, 1 / S, skip} block

    def scale(self, loss):
        """loss -> S * loss (a device-side multiply: backward() then carries S through every gradient of the step)."""
        return loss * self.scale_tensor

    def hyper_block(self, group_index):
        if group_index == 0:
            return self._f[4:8]
        blk = self._extra_hyper.get(group_index)
        if blk is None:
            blk = self._extra_hyper[group_index] = torch.zeros(4, dtype=torch.float32, device=self.state.device)
        return blk

    # ---- host readbacks (synchronise: logs, tests, checkpoints) ----
    def get_scale(self):
        return float(self._f[0].item())

    def skipped_steps(self):
        return int(self.state[3].item())

    def state_dict(self):
        st = self.state.cpu()
        return {"scale": float(st.view(torch.float32)[0]), "growth_tracker": int(st[1]), "skipped": int(st[3])}

    def load_state_dict(self, d):
        host = torch.zeros(8, dtype=torch.int32)
        host.view(torch.float32)[0] = float(d["scale"])
        host.view(torch.float32)[6] = 1.0 / float(d["scale"])
        host[1], host[3] = int(d.get("growth_tracker", 0)), int(d.get("skipped", 0))
        self.state.copy_(host)


class AdamW(torch.optim.Optimizer):
    """`max_grad_norm` (None, 0 or inf: off): clip the gradients by their GLOBAL norm over all parameter groups, as
    `torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)` before the step would -- on the device, inside the step:
    the pass that scans the gradients for inf / NaN also reduces sum(g * g) (egv_grad_sqnorm_multi replaces egv_grad_nonfinite_multi:
    the gradients are still read once), one workgroup forms norm = sqrt(sum) / S and coef = min(1, max_grad_norm / (norm + 1e-6))
    (egv_grad_clip_update) and every hyper block of the step carries (1 / S) * coef where it carried 1 / S, the factor the update
    multiplies each gradient by anyway.  No host synchronisation, no extra pass.  Without a scaler the optimizer owns the hyper
    blocks and the kernel fills them with {lr, step size, grad_scale * coef, skip}.
    ONE DEVIATION from clip_grad_norm_ (whose default would scale every gradient by NaN and write NaN into every parameter): a step
    whose norm is not finite is NOT APPLIED, with or without a scaler -- parameters and moments stay, `nonfinite_steps()` counts it;
    with a scaler the scale backs off by its usual rule as well.
    `grad_norm()` (un-scaled, before clipping), `clip_coef()`, `clipped_steps()`, `nonfinite_steps()` read the last step's decision
    back (they synchronise: logs, tests, checkpoints).  It is a property of the step, not of a group: stored on the optimizer and in
    `state_dict()['max_grad_norm']`."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: {}".format(betas))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      correct_bias=correct_bias))
        self._scaler = None     # the LossScaler of the step() in progress (None: un-scaled gradients, host-side hyper-parameters)
        self._scaler_first = False
        self._plans = {}        # id(param group) -> (params, states, exp_avg, exp_avg_sq, argument tables) of the steady-state launch
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)     # None: clipping is off, step() is the step it always was
        self._pending = None    # clipping: the launches of the step in progress, collected before the decision kernel runs
        self._clip_numels = None        # sizes of the gradient list `_clip_partials` was sized for
        self._clip_partials = None      # fp32[parts]: one sum of squares per block of egv_grad_sqnorm_multi
        self._clip_parts = 0
        self._norm_block = None         # int32[8] on the device: {norm, coef, nonfinite, clipped steps, non-finite steps, -, -, -}
        self._clip_hyper = None         # fp32[64, 4]: the hyper blocks of a step without a scaler
        self._skip_hyper = None         # the first hyper block the last step() used (None: it had neither a scaler nor clipping)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, scaler=None):
        """`scaler` (LossScaler): the gradients carry its scale S -- scan them for inf / NaN, let the device decide whether the step is
        applied (and with which S next), un-scale inside the update.  No host synchronisation either way."""
        loss = closure() if closure is not None else None
        self._skip_hyper = None
        groups = [(g, [p for p in g["params"] if p.grad is not None]) for g in self.param_groups]
        if self.max_grad_norm is not None:
            self._step_clipped(groups, grad_scale, scaler)
            weights.bump_epoch()
            return loss
        if scaler is not None:
            grads = [p.grad for _, ps in groups for p in ps]
            if any(g.is_sparse or not g.is_contiguous() for g in grads):
                raise RuntimeError("AdamW (HIP) needs contiguous dense gradients")
            ops.grad_nonfinite_multi(grads, scaler.state)
            self._scaler, self._scaler_first = scaler, True
        try:
            for gi, (group, params) in enumerate(groups):
                self._group_index = gi
                self._update_group(group, params, grad_scale)
        finally:
            self._scaler = None
        weights.bump_epoch()   # parameters were written through raw pointers: invalidate the bf16 planes
        return loss

    def _step_clipped(self, groups, grad_scale, scaler):
        """The step with max_grad_norm: scan + sum of squares (one read of the gradients), the scale decision and every launch's hyper
        block, ONE clip decision for all of them, then the updates."""
        grads = [p.grad for _, ps in groups for p in ps]
        if not grads:
            return
        if any(g.is_sparse or not g.is_contiguous() for g in grads):
            raise RuntimeError("AdamW (HIP) needs contiguous dense gradients")
        numels = [g.numel() for g in grads]
        dev = grads[0].device
        if numels != self._clip_numels or self._clip_partials.device != dev:
            # the parameter set changed (or this is the first step): size the partials for it.  Comparing the sizes themselves catches
            # every change the plans' identity test catches, and a `p.data = ...` of another size as well
            self._clip_parts = ops.grad_sqnorm_parts(grads)
            self._clip_partials = torch.empty(max(self._clip_parts, 1), dtype=torch.float32, device=dev)
            self._clip_numels = numels
        if self._norm_block is None or self._norm_block.device != dev:
            self._norm_block = torch.zeros(8, dtype=torch.int32, device=dev)      # the counters live as long as the optimizer
        ops.grad_sqnorm_multi(grads, self._clip_partials, scaler.state if scaler is not None else None)
        self._pending = []
        try:
            for gi, (group, params) in enumerate(groups):
                self._group_index = gi
                self._update_group(group, params, grad_scale)
            launches = self._pending
        finally:
            self._pending = None
        hypers, lrs, sizes, seen = [], [], [], {}
        for k, (group, gi, ps, gs, ms, vs, step, tables) in enumerate(launches):
            b1, b2 = group["betas"]
            if scaler is not None:
                # a group's first launch takes the scaler's block of that group, as the un-clipped step does; launches of the same
                # group at another step count (rare) get blocks of their own, since all blocks are written BEFORE the first update
                j = seen[gi] = seen.get(gi, -1) + 1
                hyper = scaler.hyper_block(gi if j == 0 else (gi, j))
                ops.loss_scale_update(scaler.state, hyper, group["lr"], b1, b2, step, group["correct_bias"], scaler.growth_factor,
                                      scaler.backoff_factor, scaler.growth_interval, scaler.max_scale, advance=(k == 0))
            else:
                if self._clip_hyper is None or self._clip_hyper.device != dev:
                    self._clip_hyper = torch.zeros((64, 4), dtype=torch.float32, device=dev)
                if k >= 64:
                    raise RuntimeError("AdamW (HIP): max_grad_norm serves at most 64 launch groups (parameter groups x step counts)")
                hyper = self._clip_hyper[k]
                lrs.append(group["lr"])
                sizes.append(_step_size_f32(group["lr"], b1, b2, step, group["correct_bias"]))
            hypers.append(hyper)
        self._skip_hyper = hypers[0] if hypers else None
        ops.grad_clip_update(self._clip_partials, self._clip_parts, self._norm_block, self.max_grad_norm, hypers,
                             state=scaler.state if scaler is not None else None, grad_scale=grad_scale, lrs=lrs, step_sizes=sizes)
        for hyper, (group, gi, ps, gs, ms, vs, step, tables) in zip(hypers, launches):
            self._apply(group, ps, gs, ms, vs, step, grad_scale, hyper, tables)

    def skip_flag(self):
        """Was the last step() applied?  -> a one-element fp32 DEVICE view whose non-zero value means "not applied" (an overflow of the
        fp16 backward, a non-finite gradient norm): the [3] element of the first hyper block that step used -- the scaler's block, or
        the optimizer's own first block when clipping ran without a scaler; all blocks of one step carry the same value.  None when the
        step had neither a scaler nor clipping: such a step is always applied.  An accessor only (no launch, no synchronisation); the
        view is read on the stream, e.g. by `egovlp_amd.ema.ModelEMA.update`."""
        h = self._skip_hyper
        return None if h is None else h[3:4]

    # ---- host readbacks of the clip decision (synchronise: logs, tests, checkpoints); None while clipping is off / before a step ----
    def _norm_host(self):
        return None if self._norm_block is None else self._norm_block.cpu()

    def grad_norm(self):
        """Global norm of the last step's gradients, un-scaled (divided by the loss scale), BEFORE clipping."""
        nb = self._norm_host()
        return None if nb is None else float(nb.view(torch.float32)[0])

    def clip_coef(self):
        """The factor the last step's gradients were multiplied by: min(1, max_grad_norm / (norm + 1e-6)); 0 in a step not applied."""
        nb = self._norm_host()
        return None if nb is None else float(nb.view(torch.float32)[1])

    def clipped_steps(self):
        nb = self._norm_host()
        return 0 if nb is None else int(nb[3])

    def nonfinite_steps(self):
        """Steps not applied because their gradient norm was inf / NaN (with a scaler these are also among its skipped steps)."""
        nb = self._norm_host()
        return 0 if nb is None else int(nb[4])

    def state_dict(self):
        d = super().state_dict()
        d["max_grad_norm"] = self.max_grad_norm
        return d

    def load_state_dict(self, state_dict):
        self._plans.clear()
        if "max_grad_norm" in state_dict:
            self.max_grad_norm = _check_max_grad_norm(state_dict["max_grad_norm"])
        return super().load_state_dict(state_dict)

    def _update_group(self, group, params, grad_scale):
        # steady state: the same parameters with the same moment buffers, all at the same step count -- one launch whose
        # parameter / moment tables were built at the first such step (the gradient table is rebuilt: gradients are new tensors)
        plan = self._plans.get(id(group))
        if plan is not None and len(plan[0]) == len(params) and all(a is b for a, b in zip(plan[0], params)):
            _, states, ms, vs, tables, ptrs = plan
            step = states[0]["step"] + 1
            ok = all(p.data_ptr() == q for p, q in zip(params, ptrs))       # `p.data = ...` / `.to()` since the plan was made
            for p_, st, m, v in zip(params, states, ms, vs):
                # the cached state dicts must still BE the optimizer's state (a caller may have replaced optimizer.state[p] or one of
                # the moment tensors without load_state_dict): otherwise the fast path would keep updating orphaned buffers
                ok = ok and st["step"] + 1 == step and st["exp_avg"] is m and st.get("exp_avg_sq") is v and self.state.get(p_) is st
                st["step"] += 1
            grads = [p.grad for p in params]
            if ok and not any(g.is_sparse or not g.is_contiguous() for g in grads):
                self._launch(group, params, grads, ms, vs, step, grad_scale, tables)
                return
            for st in states:          # something changed under the plan: undo, take the general path
                st["step"] -= 1
            del self._plans[id(group)]
        ps, gs, ms, vs, sts = [], [], [], [], []
        step = None
        uniform = True
        for p in params:
            if p.grad.is_sparse:
                raise RuntimeError("AdamW does not support sparse gradients")
            st = self.state[p]
            if len(st) == 0 or "exp_avg" not in st:
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["step"] += 1
            if step is None:
                step = st["step"]
            elif step != st["step"]:
                # tensors at different step counts get their own launch group
                self._launch(group, ps, gs, ms, vs, step, grad_scale)
                ps, gs, ms, vs, step = [], [], [], [], st["step"]
                uniform = False
            if not (p.is_contiguous() and p.grad.is_contiguous()):
                raise RuntimeError("AdamW (HIP) needs contiguous parameters and gradients")
            ps.append(p); gs.append(p.grad); ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"]); sts.append(st)
        self._launch(group, ps, gs, ms, vs, step, grad_scale)
        if uniform and ps:
            self._plans[id(group)] = (list(ps), sts, list(ms), list(vs), self._tables(ps, ms, vs), [p.data_ptr() for p in ps])

    def _launch(self, group, ps, gs, ms, vs, step, grad_scale, tables=None):
        if not ps:
            return
        if self._pending is not None:       # clipping: the hyper blocks of ALL launches are decided first (_step_clipped)
            self._pending.append((group, getattr(self, "_group_index", 0), ps, gs, ms, vs, step, tables))
            return
        b1, b2 = group["betas"]
        hyper = None
        sc = self._scaler
        if sc is not None:
            # the decision kernel of this step (first launch only: scale logic + found-inf reset), then this group's hyper block
            # {lr, step size at the number of APPLIED steps, 1 / S, skip} -- all on the device, read by the AdamW kernel below
            hyper = sc.hyper_block(getattr(self, "_group_index", 0))
            ops.loss_scale_update(sc.state, hyper, group["lr"], b1, b2, step, group["correct_bias"], sc.growth_factor, sc.backoff_factor,
                                  sc.growth_interval, sc.max_scale, advance=self._scaler_first)
            if self._scaler_first:
                self._skip_hyper = hyper
            self._scaler_first = False
        self._apply(group, ps, gs, ms, vs, step, grad_scale, hyper, tables)

    # ---- the update of one launch group: the one thing a subclass with another rule (LAMB) replaces ----
    def _apply(self, group, ps, gs, ms, vs, step, grad_scale, hyper, tables):
        b1, b2 = group["betas"]
        ops.adamw_multi(ps, gs, ms, vs, group["lr"], b1, b2, group["eps"], group["weight_decay"], step,
                        group["correct_bias"], grad_scale, hyper_dev=hyper, tables=tables)

    def _tables(self, ps, ms, vs):
        return ops.adamw_tables(ps, ms, vs)


class LAMB(AdamW):
    """Layer-wise adaptive moments (You et al. 2020, "Large Batch Optimization for Deep Learning") on three kernels of csrc/lamb.hip.
    Per tensor, with the step's g' = g * (1 / S) * coef (loss scale and global-norm clip, both from the hyper block, as in AdamW):

        m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  c = sqrt(1 - b2^t) / (1 - b1^t)   (t: steps APPLIED; 1 without correct_bias)
        u = c * m / (sqrt(v) + eps) + wd * p
        r = ||p|| / ||u||  if adapt and ||p|| > 0 and ||u|| > 0 else 1;   r = min(r, 1) if trust_clip;   p = p - lr * r * u

    `adapt` is `weight_decay != 0 or always_adapt`, the rule of timm's Lamb and apex's FusedLAMB (use_nvlamb): biases, LayerNorm
    weights and loss parameters in weight_decay = 0 groups take plain Adam steps.  An all-zero tensor (the zero-initialised time
    attention, temporal_embed under 'zeros') has r = 1 and moves at lr.  lr == 0: the moments advance, p stays bit-identical.
    ONE DEVIATION from timm and apex, which bias-correct m and v separately (eps INSIDE the correction): eps stays OUTSIDE, so u is,
    per unit lr, the direction this module's AdamW applies, and c = step_size / lr comes from the hyper block {lr, step_size,
    (1 / S) * coef, skip} that egv_loss_scale_update / egv_grad_clip_update already write.
    Everything before the update is AdamW's, inherited: the non-finite scan, the clip decision, the scaler's hyper blocks, launch
    groups by step count, the steady-state plans, `skip_flag()`, `grad_norm()` and the other readbacks.  A step that is not applied
    leaves parameters, moments and ratios bit-identical.  Defaults are timm's; `trust_clip` and `always_adapt` are group defaults and
    travel in `state_dict()` with the groups.  `trust_ratios()` reads the last step's ratios back (it synchronises)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, correct_bias=True, max_grad_norm=1.0,
                 trust_clip=False, always_adapt=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias,
                         max_grad_norm=max_grad_norm)
        self.defaults.update(trust_clip=bool(trust_clip), always_adapt=bool(always_adapt))
        for group in self.param_groups:
            group.setdefault("trust_clip", bool(trust_clip))
            group.setdefault("always_adapt", bool(always_adapt))
        self._lamb_numels = None        # sizes of the gradient list the two buffers below were sized for
        self._lamb_partials = None      # fp32[2 * pieces]: {sum p^2, sum u^2} of every 16 384-element piece, in list order
        self._lamb_ratios = None        # fp32[tensors]: the trust ratio of every parameter that had a gradient, in list order
        self._lamb_cursor = (0, 0)      # (tensors, pieces) the launch groups of the step in progress have taken

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, scaler=None):
        loss = None
        if closure is not None:         # the buffers are sized from the gradients: the closure runs first
            with torch.enable_grad():
                loss = closure()
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        numels = [g.numel() for g in grads]
        if grads and (numels != self._lamb_numels or self._lamb_ratios.device != grads[0].device):
            # as _clip_partials: sized once, re-sized when the parameter list changes.  The ratios start at 1
            parts = sum((n + ops.LAMB_CHUNK - 1) // ops.LAMB_CHUNK for n in numels)
            self._lamb_partials = torch.zeros(2 * max(parts, 1), dtype=torch.float32, device=grads[0].device)
            self._lamb_ratios = torch.ones(len(numels), dtype=torch.float32, device=grads[0].device)
            self._lamb_numels = numels
        self._lamb_cursor = (0, 0)
        super().step(grad_scale=grad_scale, scaler=scaler)
        return loss

    def _apply(self, group, ps, gs, ms, vs, step, grad_scale, hyper, tables):
        b1, b2 = group["betas"]
        tables = tables if tables is not None else ops.lamb_tables(ps, ms, vs)
        t0, p0 = self._lamb_cursor
        parts = tables[4]
        self._lamb_cursor = (t0 + len(ps), p0 + parts)
        if t0 + len(ps) > self._lamb_ratios.numel() or 2 * (p0 + parts) > self._lamb_partials.numel():
            raise RuntimeError("LAMB (HIP): the launch groups of a step exceed the gradient list it was sized for")
        ops.lamb_multi(ps, gs, ms, vs, group["lr"], b1, b2, group["eps"], group["weight_decay"], step, group["correct_bias"],
                       grad_scale, self._lamb_partials[2 * p0:2 * (p0 + max(parts, 1))], self._lamb_ratios[t0:t0 + len(ps)],
                       adapt=(group["weight_decay"] != 0 or group["always_adapt"]), trust_clip=group["trust_clip"],
                       hyper_dev=hyper, tables=tables)

    def _tables(self, ps, ms, vs):
        return ops.lamb_tables(ps, ms, vs)

    def trust_ratios(self):
        """The trust ratios of the last applied step, one per parameter that had a gradient, in the order of the parameter groups:
        a CPU fp32 tensor (synchronises: logs, tests); None before the first step."""
        return None if self._lamb_ratios is None else self._lamb_ratios.cpu()


def _check_max_grad_norm(v):
    """None, 0 and inf mean "off" (-> None); a negative value or NaN is an error."""
    if v is None:
        return None
    v = float(v)
    if not v >= 0.0:
        raise ValueError("Invalid max_grad_norm: {} - should be >= 0.0 (None, 0 or inf: no clipping)".format(v))
    return None if v == 0.0 or v == float("inf") else v


def clip_coefficient(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s rule, which egv_grad_clip_update applies on the device: gradients are multiplied by this."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def _step_size_f32(lr, beta1, beta2, step, correct_bias):
    """adamw_step_size on the fp32 roundings of lr / betas: what egv_adamw_multi computes from its float arguments."""
    import ctypes
    f = lambda x: ctypes.c_float(x).value
    return adamw_step_size(f(lr), f(beta1), f(beta2), step, correct_bias)


def adamw_step_size(lr, beta1, beta2, step, correct_bias=True):
    """The step-dependent scalar of transformers-4.2.1 AdamW: lr * sqrt(1 - beta2^t) / (1 - beta1^t) (double precision, as the
    C entry point computes it)."""
    if not correct_bias:
        return float(lr)
    import math
    return float(lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step))
