"""EgoNCE / NormSoftmaxLoss -- drop-in for the reference's model/loss.py:7-53.

Two ways in, same kernels underneath (egovlp_amd/csrc/egonce.hip, through the wrappers of egovlp_amd/loss_ops.py):
  * the reference's own call shape  `loss(sim_matrix(text, video), sim_v, sim_n)`  (model/loss.py:34,
    trainer/trainer_egoclip.py:130-137): `forward` below, an autograd node over egv_egonce_from_sim;
  * the fused hot path  `loss.fused(text, video, noun, verb)`: ONE call computes the three similarity
    matrices, the mask, the loss and the gradients w.r.t. both embeddings (egv_egonce_fwd_bwd; past 1 024 rows the tiled
    egv_egonce_long_fwd_bwd of csrc/egonce_long.hip, which forms no n x n matrix).
Both losses take `learnable_temperature=True` (not in the reference): the temperature becomes CLIP's learnable logit scale, read on the
device by the *_ls variants of the same entry points, which also return its gradient (_TemperatureMixin below), and `queue_size=Q`
(not in the reference): the normalised embeddings of the last steps are kept in a ring of Q rows on the device and serve as extra
constant columns of the softmax in `fused` (egv_egonce_queue_fwd_bwd, csrc/egonce_long.hip); the ring is no part of state_dict(),
so a resumed run refills its queue in Q / n steps.
SigmoidLoss / EgoSigmoidLoss (not in the reference) are the pairwise sigmoid (SigLIP) counterparts of the two softmax losses, with a
learnable logit scale AND bias (_SigmoidMixin): `forward` over egv_sigmoid_from_sim, `fused` over egv_sigmoid_head_fwd_bwd
(csrc/sigmoid_head.hip: one tile walk per direction for any n up to 65 536).
MaxMarginRankingLoss (:55-90) and AdaptiveMaxMarginRankingLoss (:92-133), the EPIC-MIR / Charades fine-tuning heads over the
same similarity matrix, run on egv_maxmargin_fwd_bwd; their `fused(text, video[, weight])` is the one-call head
of the fine-tuning step (egv_maxmargin_head_fwd_bwd: similarity, loss and both embedding gradients, deterministic; both in
csrc/maxmargin_head.hip).  CrossEntropy (:135-141), the loss of the OSCC / PNR
classification fine-tunes on the [B, classes] scores of FrozenInTime(video_only=True) (trainer/trainer_oscc.py:335-338), runs on
egv_cross_entropy_fwd_bwd (csrc/cls_head.hip); its `fused(feats, weight, bias, target[, state])` is the whole head of those steps
on an autograd node of its own: the narrow projection (egv_cls_head_fwd), one packed collective, loss and backward
(egv_cls_head_loss_bwd).
Every other loss here runs on ONE generic node, _KernelLossFn: the kernels return the gradients with the loss.
"""
import math

import torch
from torch import nn

from .. import gather, loss_ops


class _KernelLossFn(torch.autograd.Function):
    """The one autograd node of the losses whose kernel returns its own gradients: `call(*tensors)` -> (loss[1], then one gradient
    or None per tensor) runs in forward; backward hands each saved gradient out times the upstream factor, so they carry the loss
    scale of an fp16 backward.  Everything that is not differentiable lives in `call`'s closure."""

    @staticmethod
    def forward(ctx, call, *tensors):
        loss, *grads = call(*tensors)
        ctx.given = [g is not None for g in grads]
        ctx.save_for_backward(*(g for g in grads if g is not None))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        saved = iter(ctx.saved_tensors)
        return (None,) + tuple(next(saved) * g if given else None for given in ctx.given)


def _f32(t):
    return None if t is None else t.contiguous().float()


def _over_world(dls):
    """Every rank runs the head on the same gathered batch with deterministic kernels, so dL/ds is bit-identical everywhere and
    is NOT exchanged (it is no part of Bf16GradSync).  The model's gradients leave the exchange as (1 / W) grad L_global
    (egovlp_amd/gather.py); the scale's is stored with the same factor, so that the optimizer -- and its global-norm clipping -- sees
    one consistent gradient vector.  None (a gradient the kernel was not asked for) stays None."""
    W = gather._world()
    return dls if W == 1 or dls is None else dls / W


class _LogitScaleMixin:
    """What the losses with a logit scale s = log(1 / tau) share: the fp32 clamp bound, the clamp and the read-back."""

    def _init_clamp(self, learnable, max_logit_scale):
        self.learnable_temperature = bool(learnable)     # what the steps' clamp and the trainer's temperature log look at
        self.max_logit_scale = float(max_logit_scale)
        # the clamp runs in fp32: its upper bound is the largest fp32 value <= max_logit_scale (fp32(ln 100) itself rounds UP)
        hi = torch.tensor(self.max_logit_scale, dtype=torch.float32)
        if float(hi) > self.max_logit_scale:
            hi = torch.nextafter(hi, torch.tensor(float("-inf")))
        self._clamp_hi = float(hi)

    def current_temperature(self):
        """tau = exp(-s) read back from the device (synchronises: logs and tests); the fixed value of a module without the parameter."""
        if getattr(self, "logit_scale", None) is None:
            return float(self.temperature)
        return math.exp(-float(self.logit_scale.detach().float().cpu()))

    @torch.no_grad()
    def clamp_logit_scale_(self):
        """s <- clamp(s, 0, max_logit_scale) in place (CLIP: max ln 100): one tiny device op, no synchronisation.  The steps call it
        after optimizer.step.  A logit bias is not clamped."""
        if self.learnable_temperature:
            self.logit_scale.clamp_(0.0, self._clamp_hi)
        return self


class _TemperatureMixin(_LogitScaleMixin):
    """temperature = 0.05 of the reference (model/loss.py:8-11,28-32), fixed -- or, `learnable_temperature=True`, CLIP's learnable
    logit scale: `self.logit_scale` = s = log(1 / tau), one fp32 parameter initialised to log(1 / temperature); the head kernels
    read it on the device and return dL/ds.  Off (the default) the module has no parameter and makes the calls it always made.
    `queue_size=Q` (0: none): a ring of the last Q normalised embeddings as extra columns of `fused` in train() mode -- see _init_queue.
    Its buffers are non-persistent: checkpoints (loss_state_dict) do not carry them and a resumed run refills its queue in Q / n steps."""

    def _init_temperature(self, temperature, learnable_temperature, max_logit_scale, queue_size=0):
        self.temperature = temperature
        self._init_queue(queue_size)
        self._init_clamp(learnable_temperature, max_logit_scale)
        if self.learnable_temperature:
            if not temperature > 0:
                raise ValueError("learnable_temperature: the initial temperature must be positive")
            self.logit_scale = nn.Parameter(torch.full((1,), math.log(1.0 / temperature), dtype=torch.float32))

    def _scale(self):
        return (self.logit_scale,) if self.learnable_temperature else ()

    def _from_sim(self, x, mask_v, mask_n, use_noun, use_verb):
        "an autograd node over egv_egonce_from_sim (learnable: _ls, which also returns dL/d(logit_scale))"
        def call(x, logit_scale=None):
            loss, dx, *dls = loss_ops.egonce_from_sim(x, mask_v, mask_n, self.temperature, use_noun, use_verb, want_grad=True,
                                                      logit_scale=logit_scale)
            return (loss, dx, *map(_over_world, dls))
        return _KernelLossFn.apply(call, x, *self._scale())

    # ---- the queue of past embeddings (`queue_size=Q`, a multiple of 64 in [64, 65 536]; 0: none, the module is what it always was)
    # In train() mode `fused` runs the rectangular head of csrc/egonce_long.hip for EVERY n <= Q: the batch against itself and
    # against the valid slots of the ring -- extra negatives and, for EgoNCE, extra positives (a queued clip that shares a noun and
    # a verb with an anchor), constants that get no gradient -- and then enqueues the batch, unless the loss is not finite.  Every
    # rank runs the head on the same gathered batch, so every rank enqueues the same rows and nothing is exchanged.  In eval() mode
    # `fused` is the plain head and nothing is enqueued.  The ring is allocated by the first such call (it needs D, the noun / verb
    # widths and the device) as NON-PERSISTENT buffers: state_dict() and the checkpoint's loss_state_dict do not change, and a
    # resumed run refills its queue in Q / n steps.
    def _init_queue(self, queue_size):
        if isinstance(queue_size, bool) or not isinstance(queue_size, int) or \
                (queue_size != 0 and not loss_ops.egonce_queue_size_ok(queue_size)):
            raise ValueError("queue_size must be 0 or a multiple of 64 in [%d, %d], got %r"
                             % (loss_ops.EGONCE_QUEUE_MIN, loss_ops.EGONCE_QUEUE_MAX, queue_size))
        self.queue_size = queue_size
        self._queue = None

    _QUEUE_BUFFERS = ("text", "video", "words", "state")

    def _ring(self):
        "the ring, if one is allocated, on the module's current buffers (a module.to(...) replaces them)"
        if self._queue is not None:
            for name in self._QUEUE_BUFFERS:
                setattr(self._queue, name, getattr(self, "queue_" + name))
        return self._queue

    def _queue_for(self, text, noun, verb):
        "the ring, allocated on first use; its tensors are the module's buffers queue_text / _video / _words / _state"
        if self._queue is None:
            dn, dv = loss_ops._nv_widths(noun, verb)
            self._queue = loss_ops.EgonceQueue(self.queue_size, text.shape[1], dn, dv, text.device)
            for name in self._QUEUE_BUFFERS:
                self.register_buffer("queue_" + name, getattr(self._queue, name), persistent=False)
        return self._ring()

    def reset_queue(self):
        "empty the ring (head = filled = 0); the next train-mode `fused` sees the batch alone"
        if self._ring() is not None:
            self._queue.reset()
        return self

    def queue_filled(self):
        "valid rows of the ring, read back from the device (synchronises: logs and tests); 0 before the first train-mode `fused`"
        return 0 if self._ring() is None else self._queue.filled()

    def _refuse_matrix_path(self):
        if self.queue_size and self.training:
            raise ValueError("a loss with queue_size > 0 in train() mode takes the embeddings, not a similarity matrix: call "
                             "`fused` (egoclip_head_loss: fused_head=True, D <= 256, D % 4 == 0)")

    def _fused_queue(self, text, video, noun, verb, use_noun, use_verb):
        "an autograd node over egv_egonce_queue_fwd_bwd, followed by egv_egonce_queue_push on the same stream"
        noun, verb = _f32(noun), _f32(verb)
        queue = self._queue_for(text, noun, verb)

        def call(text, video, logit_scale=None):
            loss, dt, dv, *dls, work = loss_ops.egonce_queue_fwd_bwd(text.contiguous(), video.contiguous(), noun, verb,
                                                                     self.temperature, queue, use_noun=use_noun,
                                                                     use_verb=use_verb, logit_scale=logit_scale)
            loss_ops.egonce_queue_push(work, loss, text.shape[0], queue)
            return (loss, dt, dv, *map(_over_world, dls))
        return _KernelLossFn.apply(call, text, video, *self._scale())

    def _fused(self, text, video, noun, verb, use_noun, use_verb):
        "an autograd node over egv_egonce_fwd_bwd / egv_egonce_long_fwd_bwd (learnable: their _ls variants)"
        if self.queue_size and self.training:
            return self._fused_queue(text, video, noun, verb, use_noun, use_verb)

        def call(text, video, logit_scale=None):
            loss, _, dt, dv, *dls = loss_ops.egonce_fwd_bwd(text.contiguous(), video.contiguous(), _f32(noun), _f32(verb),
                                                            self.temperature, use_noun=use_noun, use_verb=use_verb,
                                                            logit_scale=logit_scale)
            return (loss, dt, dv, *map(_over_world, dls))
        return _KernelLossFn.apply(call, text, video, *self._scale())


class NormSoftmaxLoss(_TemperatureMixin, nn.Module):
    def __init__(self, temperature=0.05, learnable_temperature=False, max_logit_scale=math.log(100), queue_size=0):
        super().__init__()
        self._init_temperature(temperature, learnable_temperature, max_logit_scale, queue_size)

    def forward(self, x):
        "x: similarity matrix N x N in [-1, 1] (model/loss.py:13-25)"
        self._refuse_matrix_path()
        return self._from_sim(x, None, None, True, True)

    def fused(self, text_embeds, video_embeds):
        return self._fused(text_embeds, video_embeds, None, None, True, True)


class EgoNCE(_TemperatureMixin, nn.Module):
    def __init__(self, temperature=0.05, noun=True, verb=True, learnable_temperature=False, max_logit_scale=math.log(100),
                 queue_size=0):
        super().__init__()
        self.noun = noun
        self.verb = verb
        self._init_temperature(temperature, learnable_temperature, max_logit_scale, queue_size)

    def forward(self, x, mask_v, mask_n):
        self._refuse_matrix_path()
        # noun=False, verb=False falls into the reference's else-branch (mask_v), model/loss.py:40-41
        return self._from_sim(x, mask_v, mask_n, self.noun, self.verb or not self.noun)

    def fused(self, text_embeds, video_embeds, noun_vec, verb_vec):
        return self._fused(text_embeds, video_embeds, noun_vec, verb_vec, self.noun, self.verb or not self.noun)


class _SigmoidMixin(_LogitScaleMixin):
    """SigLIP's two parameters (Zhai et al. 2023): `logit_scale` = s (u = exp(s) x + b; initial value ln 10) and `logit_bias` = b
    (initial value -10), fp32 [1] each, read on the device by the head kernels, which return dL/ds and dL/db beside the embedding
    gradients.  learnable=False: both are held with requires_grad=False and the heads are called without the parameter gradients."""

    def _init_sigmoid(self, logit_scale, logit_bias, learnable, max_logit_scale):
        self.learnable = bool(learnable)
        self._init_clamp(learnable, max_logit_scale)
        self.logit_scale = nn.Parameter(torch.full((1,), float(logit_scale), dtype=torch.float32), requires_grad=self.learnable)
        self.logit_bias = nn.Parameter(torch.full((1,), float(logit_bias), dtype=torch.float32), requires_grad=self.learnable)

    def current_bias(self):
        """b read back from the device (synchronises: logs and tests)."""
        return float(self.logit_bias.detach().float().cpu())

    def _from_sim(self, x, mask_v, mask_n, use_noun, use_verb):
        "an autograd node over egv_sigmoid_from_sim: dx, dL/ds and dL/db"
        def call(x, logit_scale, logit_bias):
            loss, dx, dls, dlb = loss_ops.sigmoid_from_sim(x, mask_v, mask_n, logit_scale, logit_bias, use_noun, use_verb,
                                                           want_grad=True, want_param_grads=self.learnable)
            return loss, dx, _over_world(dls), _over_world(dlb)
        return _KernelLossFn.apply(call, x, self.logit_scale, self.logit_bias)

    def _fused(self, text, video, noun, verb, use_noun, use_verb):
        "an autograd node over the one-call sigmoid head (egv_sigmoid_head_fwd_bwd): all four gradients"
        def call(text, video, logit_scale, logit_bias):
            loss, dt, dv, dls, dlb = loss_ops.sigmoid_head_fwd_bwd(text.contiguous(), video.contiguous(), _f32(noun), _f32(verb),
                                                                   logit_scale, logit_bias, use_noun=use_noun, use_verb=use_verb,
                                                                   want_param_grads=self.learnable)
            return loss, dt, dv, _over_world(dls), _over_world(dlb)
        return _KernelLossFn.apply(call, text, video, self.logit_scale, self.logit_bias)


class SigmoidLoss(_SigmoidMixin, nn.Module):
    """Pairwise sigmoid loss (SigLIP) on the diagonal positives: the counterpart of NormSoftmaxLoss (not in the reference).
    L = (1 / n) sum_ij softplus(-z_ij (exp(s) x_ij + b)), z = +1 on the diagonal, -1 elsewhere."""

    takes_noun_verb = False

    def __init__(self, logit_scale=math.log(10), logit_bias=-10.0, learnable=True, max_logit_scale=math.log(100)):
        super().__init__()
        self._init_sigmoid(logit_scale, logit_bias, learnable, max_logit_scale)

    def forward(self, x):
        "x: similarity matrix N x N in [-1, 1]"
        return self._from_sim(x, None, None, True, True)

    def fused(self, text_embeds, video_embeds):
        return self._fused(text_embeds, video_embeds, None, None, True, True)


class EgoSigmoidLoss(_SigmoidMixin, nn.Module):
    """The sigmoid loss with EgoNCE's positives: the counterpart of EgoNCE (not in the reference).  z_ij = +1 where rows i and j
    share a noun and a verb, or i == j (`noun` only: share a noun; neither flag: the reference's else-branch, verb): every pair is
    its own binary decision, so the set of positives of a row needs no normalisation."""

    takes_noun_verb = True          # trainer/common.py egoclip_head_loss: fused(text, video, noun_vec, verb_vec), forward(x, mask_v, mask_n)

    def __init__(self, logit_scale=math.log(10), logit_bias=-10.0, learnable=True, max_logit_scale=math.log(100), noun=True, verb=True):
        super().__init__()
        self.noun = noun
        self.verb = verb
        self._init_sigmoid(logit_scale, logit_bias, learnable, max_logit_scale)

    def forward(self, x, mask_v, mask_n):
        return self._from_sim(x, mask_v, mask_n, self.noun, self.verb or not self.noun)

    def fused(self, text_embeds, video_embeds, noun_vec, verb_vec):
        return self._fused(text_embeds, video_embeds, noun_vec, verb_vec, self.noun, self.verb or not self.noun)


def _maxmargin(x, weight, margin, fix_norm):
    return _KernelLossFn.apply(lambda x: loss_ops.maxmargin(x, weight, margin, fix_norm, want_grad=True), x)


def _maxmargin_fused(text, video, weight, margin, fix_norm):
    def call(text, video):
        loss, _, dt, dv = loss_ops.maxmargin_head(text, video, weight, margin, fix_norm)
        return loss, dt, dv
    return _KernelLossFn.apply(call, text, video)


class MaxMarginRankingLoss(nn.Module):
    """model/loss.py:55-90 (same constructor; `weight` is accepted and ignored, as in the reference)."""

    def __init__(self, margin=0.2, fix_norm=True):
        super().__init__()
        self.fix_norm = fix_norm
        self.margin = margin

    def forward(self, x, weight=None):
        return _maxmargin(x, None, self.margin, self.fix_norm)

    def fused(self, text_embeds, video_embeds, weight=None):
        "loss(sim_matrix(text_embeds, video_embeds)) in one call (`weight` ignored, as in forward)"
        return _maxmargin_fused(text_embeds, video_embeds, None, self.margin, self.fix_norm)


class AdaptiveMaxMarginRankingLoss(nn.Module):
    """model/loss.py:92-133: the margin of row i is weight[i] * margin."""

    def __init__(self, margin=0.4, fix_norm=True):
        super().__init__()
        self.fix_norm = fix_norm
        self.margin = margin

    def forward(self, x, weight=None):
        if weight is None:
            raise TypeError("AdaptiveMaxMarginRankingLoss needs the per-row weight (model/loss.py:109)")
        return _maxmargin(x, weight, self.margin, self.fix_norm)

    def fused(self, text_embeds, video_embeds, weight=None):
        "loss(sim_matrix(text_embeds, video_embeds), weight) in one call"
        if weight is None:
            raise TypeError("AdaptiveMaxMarginRankingLoss needs the per-row weight (model/loss.py:109)")
        return _maxmargin_fused(text_embeds, video_embeds, weight, self.margin, self.fix_norm)


class CrossEntropy(nn.Module):
    """model/loss.py:135-141: `nn.CrossEntropyLoss()(output, target)` (mean reduction, ignore_index -100), the loss of
    configs/ft/oscc.json and pnr.json.  `label_smoothing` (an extension, torch's own argument: `"args": {"label_smoothing": 0.1}`)
    and the `target2` / `lam` of a Mixup / CutMix step make the target of a row (1 - eps) (lam e(t) + (1 - lam) e(t2)) + eps / C;
    with label_smoothing 0 and no target2 every method makes the calls it made before."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError("CrossEntropy: label_smoothing lies in [0, 1]")
        self.label_smoothing = float(label_smoothing)

    def _soft(self, target2, lam):
        if lam is not None and target2 is None:
            raise ValueError("CrossEntropy: lam mixes target with target2")
        return {} if target2 is None and self.label_smoothing == 0.0 else \
            {"target2": target2, "lam": lam, "label_smoothing": self.label_smoothing}

    def forward(self, output, target, target2=None, lam=None):
        soft = self._soft(target2, lam)
        return _KernelLossFn.apply(lambda output: loss_ops.cross_entropy(output, target, want_grad=True, **soft), output)

    def hard(self, output, target):
        "The loss on the hard targets whatever `label_smoothing` says: what validation reports (comparable across recipes)."
        return _KernelLossFn.apply(lambda output: loss_ops.cross_entropy(output, target, want_grad=True), output)

    def fused(self, feats, weight, bias, target, state=None, world_size=1, rank=0, ec=None, target2=None, lam=None):
        """The classification head of the OSCC / PNR step in one node, from the video tower's features [B, K]:
        scores = feats weight^T + bias, gathered over the ranks with target (and state) in one collective, then
          state None:  CrossEntropy(scores, target)                       trainer/trainer_oscc.py:335-338
          state [B]:   mean(state.T * CrossEntropy(scores, target))       trainer/trainer_pnr.py:345-350
        and the local gradients w.r.t. feats, weight and bias (what AllGather_multi.backward leaves to this rank).
        `ec`: the model's execution context (its backward poll runs first in backward, as in the projection node this replaces).
        target2 [B] / lam [B]: the partner's class and the mixing weight of a Mixup / CutMix step; they ride in the same collective."""
        self._soft(target2, lam)
        return _ClsHeadFn.apply(feats, weight, bias, target, state, world_size, rank, ec, target2, lam, self.label_smoothing)[0]


class _ClsHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, weight, bias, target, state, world, rank, ec=None, target2=None, lam=None, label_smoothing=0.0):
        B, C = feats.shape[0], weight.shape[0]
        # hard targets: the layout, the columns and the loss call of always; the two soft columns ride only with a target2
        cols, soft = {}, {}
        if target2 is None:
            lay = loss_ops.ClsLayout(C, 'oscc' if state is None else 'pnr')
        else:
            lay = loss_ops.ClsLayout(C, 'oscc' if state is None else 'pnr', soft=True)
            cols = {"target2": target2, "lam": 1.0 if lam is None else lam}
        packed = torch.empty((B, lay.ld), dtype=torch.float32, device=feats.device)
        loss_ops.cls_head_fwd(feats, weight, bias, out=packed)
        lay.fill(packed, target, state, **cols)
        allp = gather._gather_rows(packed, world)             # the ONE collective of the step; nothing is sent at world size 1
        if target2 is not None or label_smoothing != 0.0:
            soft = {"col_target2": lay.target2, "col_lam": lay.lam, "label_smoothing": label_smoothing}
        loss, dW, db, dx, _ = loss_ops.cls_head_loss_bwd(allp, C, lay.target, lay.state, row0=rank * B, B=B, feats=feats,
                                                         weight=weight, **soft)
        ctx.ec, ctx.has_bias = ec, bias is not None
        ctx.save_for_backward(dx, dW, db)
        ctx.mark_non_differentiable(allp)
        return loss.reshape(()), allp

    @staticmethod
    def backward(ctx, g, _g_block):
        dx, dW, db = ctx.saved_tensors
        if ctx.ec is not None and not ctx.ec.on_text_stream():
            ctx.ec.poll_backward()      # the first node of the video tower's backward on the main stream (as _ProjFn.backward)
        return (dx * g, dW * g, (db * g if ctx.has_bias else None)) + (None,) * 8
