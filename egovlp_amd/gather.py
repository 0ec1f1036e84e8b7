"""The embedding all-gathers of every training and validation step.

`AllGather_multi` keeps the reference's autograd contract (trainer/trainer_egoclip.py:11-27): forward =
all-gather + rank-major concatenation, backward = the LOCAL rows of the incoming gradient, no reduction
(every rank computes the identical global loss; DDP's mean over ranks then yields (1/W) dL_global/dtheta,
SURVEY 3.2).  On MI355X the four per-step gathers of the reference (:126-129: video, text, noun, verb =
four latency-bound RCCL launches + 4W allocations + 4 cats) become ONE `all_gather_into_tensor` of a
packed [B, 256+256+582+118] fp32 row block (~152 KiB per rank at B=32) written straight into its final
place -- xGMI is point-to-point, so for a payload this small launch latency, not link bandwidth, is
what there is to save.  `backend='nccl'` on PyTorch-ROCm IS RCCL.

Every collective of the three autograd functions (and of the model's classification head, model/loss.py) goes through the
module global `_gather_rows`.
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _gather_rows(t: torch.Tensor, world: int) -> torch.Tensor:
    if world == 1 and os.environ.get("EGV_FORCE_GATHER") != "1":
        return t
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    from .dist import timed
    timed("embedding_all_gather", lambda: dist.all_gather_into_tensor(out, t.contiguous()))
    return out


class AllGather_multi(torch.autograd.Function):
    """An autograd function that performs allgather on a tensor (reference signature kept:
    `AllGather_multi.apply(tensor, n_gpu, args)` with args.world_size / args.rank)."""

    @staticmethod
    def forward(ctx, tensor, n_gpu, args):
        ctx.rank = args.rank
        ctx.batch_size = tensor.shape[0]
        return _gather_rows(tensor, args.world_size)

    @staticmethod
    def backward(ctx, grad_output):
        return (grad_output[ctx.batch_size * ctx.rank: ctx.batch_size * (ctx.rank + 1)], None, None)


class AllGatherFused(torch.autograd.Function):
    """(video_embeds, text_embeds, noun_vec, verb_vec) -> their global-batch versions with ONE collective."""

    @staticmethod
    def forward(ctx, video, text, noun, verb, world_size, rank):
        ctx.rank, ctx.B = rank, video.shape[0]
        if world_size == 1 and os.environ.get("EGV_FORCE_GATHER") != "1":   # (forced: 1-GPU smoke test of the collective path)
            return video, text, noun, verb
        widths = [video.shape[1], text.shape[1], noun.shape[1], verb.shape[1]]
        packed = torch.cat([video, text, noun.to(video.dtype), verb.to(video.dtype)], dim=1)
        allp = _gather_rows(packed, world_size)
        v, t, n, b = torch.split(allp, widths, dim=1)
        return v.contiguous(), t.contiguous(), n.contiguous(), b.contiguous()

    @staticmethod
    def backward(ctx, gv, gt, gn, gb):
        lo, hi = ctx.B * ctx.rank, ctx.B * (ctx.rank + 1)
        return gv[lo:hi], gt[lo:hi], None, None, None, None


class AllGatherRows(torch.autograd.Function):
    """`AllGatherRows.apply(world_size, rank, *tensors)`: row-aligned [B, ...] tensors -> their global-batch versions with ONE
    collective (packed as columns of one fp32 row block, like AllGatherFused).  Backward hands every input the LOCAL rows of
    its gradient (inputs that do not require one, e.g. per-row loss weights, are ignored by autograd)."""

    @staticmethod
    def forward(ctx, world_size, rank, *tensors):
        ctx.rank, ctx.B = rank, tensors[0].shape[0]
        if world_size == 1 and os.environ.get("EGV_FORCE_GATHER") != "1":
            return tensors if len(tensors) > 1 else tensors[0]
        dtype = tensors[0].dtype
        flat = [t.reshape(ctx.B, -1).to(dtype) for t in tensors]
        allp = _gather_rows(torch.cat(flat, dim=1), world_size)
        parts = torch.split(allp, [f.shape[1] for f in flat], dim=1)
        out = tuple(p.contiguous().reshape((allp.shape[0],) + tuple(t.shape[1:])).to(t.dtype) for p, t in zip(parts, tensors))
        return out if len(out) > 1 else out[0]

    @staticmethod
    def backward(ctx, *grads):
        lo, hi = ctx.B * ctx.rank, ctx.B * (ctx.rank + 1)
        return (None, None) + tuple(None if g is None else g[lo:hi] for g in grads)
