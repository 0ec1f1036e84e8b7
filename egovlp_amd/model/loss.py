"""EgoNCE / NormSoftmaxLoss -- drop-in for the reference's model/loss.py:7-53.

Two ways in, same kernels underneath (egovlp_amd/csrc/egonce.hip):
  * the reference's own call shape  `loss(sim_matrix(text, video), sim_v, sim_n)`  (model/loss.py:34,
    trainer/trainer_egoclip.py:130-137): `forward` below, an autograd node over egv_egonce_from_sim;
  * the fused hot path  `loss.fused(text, video, noun, verb)`: ONE call computes the three similarity
    matrices, the mask, the loss and the gradients w.r.t. both embeddings (egv_egonce_fwd_bwd; past 1 024 rows the tiled
    egv_egonce_long_fwd_bwd of csrc/egonce_long.hip, which forms no n x n matrix).
MaxMarginRankingLoss (:55-90) and AdaptiveMaxMarginRankingLoss (:92-133), the EPIC-MIR / Charades fine-tuning heads over the
same similarity matrix, run on egv_maxmargin_fwd_bwd; their `fused(text, video[, weight])` is the one-call head
of the fine-tuning step (egv_maxmargin_head_fwd_bwd: similarity, loss and both embedding gradients, deterministic).  CrossEntropy (:135-141), the loss of the OSCC / PNR
classification fine-tunes on the [B, classes] scores of FrozenInTime(video_only=True) (trainer/trainer_oscc.py:335-338), runs on
egv_cross_entropy_fwd_bwd; its `fused(feats, weight, bias, target[, state])` is the whole head of those steps on ONE autograd
node: the narrow projection (egv_cls_head_fwd), one packed collective, loss and backward (egv_cls_head_loss_bwd).
"""
import torch
from torch import nn

from .. import gather, loss_ops, ops


class _LossFromSimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask_v, mask_n, temperature, use_noun, use_verb):
        loss, dx = loss_ops.egonce_from_sim(x, mask_v, mask_n, temperature, use_noun, use_verb, want_grad=True)
        ctx.save_for_backward(dx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None, None, None, None


class _FusedHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, text, video, noun, verb, temperature, use_noun, use_verb):
        loss, _, dt, dv = ops.egonce_fwd_bwd(text.contiguous(), video.contiguous(),
                                             None if noun is None else noun.contiguous().float(),
                                             None if verb is None else verb.contiguous().float(),
                                             temperature, use_noun=use_noun, use_verb=use_verb)
        ctx.save_for_backward(dt, dv)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dt, dv = ctx.saved_tensors
        return dt * g, dv * g, None, None, None, None, None


class NormSoftmaxLoss(nn.Module):
    def __init__(self, temperature=0.05):
        super().__init__()
        self.temperature = temperature

    def forward(self, x):
        "x: similarity matrix N x N in [-1, 1] (model/loss.py:13-25)"
        return _LossFromSimFn.apply(x, None, None, self.temperature, True, True)

    def fused(self, text_embeds, video_embeds):
        return _FusedHeadFn.apply(text_embeds, video_embeds, None, None, self.temperature, True, True)


class EgoNCE(nn.Module):
    def __init__(self, temperature=0.05, noun=True, verb=True):
        super().__init__()
        self.noun = noun
        self.verb = verb
        self.temperature = temperature

    def forward(self, x, mask_v, mask_n):
        # noun=False, verb=False falls into the reference's else-branch (mask_v), model/loss.py:40-41
        return _LossFromSimFn.apply(x, mask_v, mask_n, self.temperature, self.noun, self.verb or not self.noun)

    def fused(self, text_embeds, video_embeds, noun_vec, verb_vec):
        return _FusedHeadFn.apply(text_embeds, video_embeds, noun_vec, verb_vec, self.temperature, self.noun,
                                  self.verb or not self.noun)


class _MaxMarginFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, margin, fix_norm):
        loss, dx = loss_ops.maxmargin(x, weight, margin, fix_norm, want_grad=True)
        ctx.save_for_backward(dx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None, None


class _FusedMaxMarginFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, text, video, weight, margin, fix_norm):
        loss, _, dt, dv = loss_ops.maxmargin_head(text, video, weight, margin, fix_norm)
        ctx.save_for_backward(dt, dv)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dt, dv = ctx.saved_tensors
        return dt * g, dv * g, None, None, None


class MaxMarginRankingLoss(nn.Module):
    """model/loss.py:55-90 (same constructor; `weight` is accepted and ignored, as in the reference)."""

    def __init__(self, margin=0.2, fix_norm=True):
        super().__init__()
        self.fix_norm = fix_norm
        self.margin = margin

    def forward(self, x, weight=None):
        return _MaxMarginFn.apply(x, None, self.margin, self.fix_norm)

    def fused(self, text_embeds, video_embeds, weight=None):
        "loss(sim_matrix(text_embeds, video_embeds)) in one call (`weight` ignored, as in forward)"
        return _FusedMaxMarginFn.apply(text_embeds, video_embeds, None, self.margin, self.fix_norm)


class AdaptiveMaxMarginRankingLoss(nn.Module):
    """model/loss.py:92-133: the margin of row i is weight[i] * margin."""

    def __init__(self, margin=0.4, fix_norm=True):
        super().__init__()
        self.fix_norm = fix_norm
        self.margin = margin

    def forward(self, x, weight=None):
        if weight is None:
            raise TypeError("AdaptiveMaxMarginRankingLoss needs the per-row weight (model/loss.py:109)")
        return _MaxMarginFn.apply(x, weight, self.margin, self.fix_norm)

    def fused(self, text_embeds, video_embeds, weight=None):
        "loss(sim_matrix(text_embeds, video_embeds), weight) in one call"
        if weight is None:
            raise TypeError("AdaptiveMaxMarginRankingLoss needs the per-row weight (model/loss.py:109)")
        return _FusedMaxMarginFn.apply(text_embeds, video_embeds, weight, self.margin, self.fix_norm)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target):
        loss, dx = loss_ops.cross_entropy(output, target, want_grad=True)
        ctx.save_for_backward(dx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g, None


class CrossEntropy(nn.Module):
    """model/loss.py:135-141: `nn.CrossEntropyLoss()(output, target)` (mean reduction, ignore_index -100), the loss of
    configs/ft/oscc.json and pnr.json."""

    def __init__(self):
        super().__init__()

    def forward(self, output, target):
        return _CrossEntropyFn.apply(output, target)

    def fused(self, feats, weight, bias, target, state=None, world_size=1, rank=0, ec=None):
        """The classification head of the OSCC / PNR step in one node, from the video tower's features [B, K]:
        scores = feats weight^T + bias, gathered over the ranks with target (and state) in one collective, then
          state None:  CrossEntropy(scores, target)                       trainer/trainer_oscc.py:335-338
          state [B]:   mean(state.T * CrossEntropy(scores, target))       trainer/trainer_pnr.py:345-350
        and the local gradients w.r.t. feats, weight and bias (what AllGather_multi.backward leaves to this rank).
        `ec`: the model's execution context (its backward poll runs first in backward, as in the projection node this replaces)."""
        return _ClsHeadFn.apply(feats, weight, bias, target, state, world_size, rank, ec)[0]


class _ClsHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, weight, bias, target, state, world, rank, ec=None):
        B, C = feats.shape[0], weight.shape[0]
        lay = loss_ops.ClsLayout(C, 'oscc' if state is None else 'pnr')
        packed = torch.empty((B, lay.ld), dtype=torch.float32, device=feats.device)
        loss_ops.cls_head_fwd(feats, weight, bias, out=packed)
        lay.fill(packed, target, state)
        allp = gather._gather_rows(packed, world)             # the ONE collective of the step; nothing is sent at world size 1
        loss, dW, db, dx, _ = loss_ops.cls_head_loss_bwd(allp, C, lay.target, lay.state, row0=rank * B, B=B, feats=feats,
                                                         weight=weight)
        ctx.ec, ctx.has_bias = ec, bias is not None
        ctx.save_for_backward(dx, dW, db)
        ctx.mark_non_differentiable(allp)
        return loss.reshape(()), allp

    @staticmethod
    def backward(ctx, g, _g_block):
        dx, dW, db = ctx.saved_tensors
        if ctx.ec is not None and not ctx.ec.on_text_stream():
            ctx.ec.poll_backward()      # the first node of the video tower's backward on the main stream (as _ProjFn.backward)
        return dx * g, dW * g, (db * g if ctx.has_bias else None), None, None, None, None, None
