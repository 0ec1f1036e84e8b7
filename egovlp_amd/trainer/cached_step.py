"""The EgoClip step over a batch larger than memory: embedding-cache chunks (the scheme known as GradCache).

`egoclip_step` runs its whole per-GPU batch through one forward and one backward, so the EgoNCE negatives of a step -- world size x B
rows -- are bounded by the saved activations of twelve space-time blocks.  The reference gets its global batch from node count
(configs/pt/egoclip.json: 16 per GPU on many GPUs); on one or two cards that is a different objective from the published one, and plain
gradient accumulation does not repair it: a mean of per-chunk EgoNCE losses is not the loss of the global batch.

The encoders couple the rows of a batch only through the head, so the step splits there:

  1. every chunk is encoded WITHOUT saving activations and its embeddings go into two [B, D] fp32 caches;
  2. the head runs ONCE on the cached (and gathered) embeddings of the whole batch and is back-propagated to the caches only:
     their gradients are S dL/d(embedding) of the local rows;
  3. every chunk is encoded AGAIN, with activations, and back-propagated from its rows of those gradients; the chunk gradients are
     summed into one accumulator per parameter by ONE multi-tensor launch per chunk (egv_grad_accumulate_multi).

By construction memory is that of a step over `chunk` rows (plus two [B, D] caches and a second copy of the gradients while a chunk's
exist) and time that of the plain step plus one forward per chunk; what was measured is in DESIGN 4.10.
"""
from __future__ import annotations

import contextlib

import torch

from .. import ops
from ..gather import AllGatherFused
from .common import clamp_loss_scale, egoclip_head_loss, step_prologue


def _rows(data, lo, hi):
    """Rows [lo, hi) of a device batch: the model's inputs (video, tokenised text) only."""
    return {'video': data['video'][lo:hi], 'text': {k: v[lo:hi] for k, v in data['text'].items()}}


def egoclip_step_cached(model, loss_fn, optimizer, data, chunk, world_size=1, rank=0, grad_sync=None, scaler=None, aug_boxes=None,
                        check_replay=False, fused_head=True, aug_color=None):
    """`egoclip_step` with the per-GPU batch encoded `chunk` rows at a time: the loss and the gradients are those of the whole batch
    of B rows (times the world size), the activations held at any time those of one chunk.  `data`: one device batch as for
    `egoclip_step`; the last chunk may be shorter, `chunk >= B` is a single chunk.  Returns the detached (device) loss; no host sync.

    `aug_boxes` (int [B, 5], SpaceTimeTransformer.set_input_augmentation): the train transform fused into the patch gather -- each
    chunk's slice is set before BOTH of its forwards; `aug_color` (float [B, 4], needs `aug_boxes`): the colour-jitter table that goes
    with them, sliced the same way.  `grad_sync`: its exchange is held while the chunks run (a gradient that exists
    after the first chunk is a partial sum) and leaves from `finish()`, un-overlapped, once per step.  `scaler`: as in `egoclip_step`;
    an inf / NaN in any chunk's gradients survives the fp32 sums, so the optimizer's scan of the accumulators skips the step as ever.

    Replay: the gradient of the head is taken at the embeddings of pass 1 and applied through the graph of pass 3, so the two passes
    must compute the same embeddings.  Pass 1 therefore runs the train-mode kernels under no_grad
    (ExecContext.train_kernels_without_grad) and the call counters of the text tower's dropout and of the video tower's stochastic
    depth are put back before pass 3 re-encodes a chunk, which regenerates the same counter-based masks.  `check_replay=True` (tests, diagnostics) leaves on the unwrapped model
    `last_replay_max_abs_diff` -- a device scalar, max over chunks of |pass-3 embedding - cached row| -- and `last_cached_embeddings`
    (text, video), the two [B, D] caches of the step (kept alive until the next such step; not set without `check_replay`).
    `fused_head=False`: the head takes the reference's own decomposition (sim_matrix + loss.forward), as in `egoclip_step`.

    Dropout: the masks are drawn per chunk forward.  They are other draws of the same distribution than those of a one-shot step over
    the B rows, not the same masks."""
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError("egoclip_step_cached: chunk is a positive number of rows")
    if aug_color is not None and aug_boxes is None:
        raise ValueError("egoclip_step_cached: aug_color is a stage of the fused train transform and needs aug_boxes")
    core, ec, scaler = step_prologue(model, optimizer, scaler)
    B = data['video'].shape[0]
    spans = [(lo, min(lo + chunk, B)) for lo in range(0, B, chunk)]
    video_model, text_model = getattr(core, 'video_model', None), getattr(core, 'text_model', None)

    def encode(lo, hi):
        if aug_color is not None:
            video_model.set_input_augmentation(aug_boxes[lo:hi], color=aug_color[lo:hi])
        elif aug_boxes is not None:
            video_model.set_input_augmentation(aug_boxes[lo:hi])
        return model(_rows(data, lo, hi))

    # ---- pass 1: encode and cache -- the train-mode kernels, nothing saved
    counters = []
    t_cache = v_cache = None
    with torch.no_grad(), (ec.train_kernels_without_grad() if ec is not None else contextlib.nullcontext()):
        for lo, hi in spans:
            counters.append((getattr(text_model, '_drop_calls', None), getattr(video_model, '_drop_calls', None)))
            text_k, video_k = encode(lo, hi)
            if t_cache is None:
                t_cache = torch.empty((B, text_k.shape[1]), dtype=torch.float32, device=text_k.device)
                v_cache = torch.empty((B, video_k.shape[1]), dtype=torch.float32, device=video_k.device)
            t_cache[lo:hi].copy_(text_k)
            v_cache[lo:hi].copy_(video_k)
            del text_k, video_k

    # ---- pass 2: the head, once, on the whole (gathered) batch; back-propagated to the caches only
    t_cache.requires_grad_(True)
    v_cache.requires_grad_(True)
    video_all, text_all, n_all, v_all = AllGatherFused.apply(v_cache, t_cache, data['noun_vec'], data['verb_vec'], world_size, rank)
    loss = egoclip_head_loss(loss_fn, text_all, video_all, n_all, v_all, fused_head)
    params = [p for p in core.parameters() if p.requires_grad]
    acc = None
    diff = torch.zeros((), dtype=torch.float32, device=t_cache.device) if check_replay else None
    # the gradient exchange is held from the head's backward to the end of pass 3: no gradient that exists in between is final
    with (grad_sync.hold() if grad_sync is not None else contextlib.nullcontext()):
        (loss if scaler is None else scaler.scale(loss)).backward()
        g_text, g_video = t_cache.grad, v_cache.grad           # S dL/d(embedding) of the local rows
        del video_all, text_all, n_all, v_all

        # ---- pass 3: re-encode with activations, back-propagate each chunk from its rows of the cached gradients.  Every p.grad is
        # None when a chunk's backward starts, so the wgrad side streams, the gradient planes and AccumulateGrad's steal path behave as
        # in the plain step; the first chunk's gradient tensors become the accumulators.
        for k, (lo, hi) in enumerate(spans):
            for tower, calls in zip((text_model, video_model), counters[k]):
                if calls is not None:
                    tower._drop_calls = calls
            text_k, video_k = encode(lo, hi)
            if check_replay:
                with torch.no_grad():
                    diff = torch.maximum(diff, torch.maximum((text_k - t_cache[lo:hi]).abs().max(), (video_k - v_cache[lo:hi]).abs().max()))
            torch.autograd.backward([text_k, video_k], [g_text[lo:hi], g_video[lo:hi]])
            del text_k, video_k
            if ec is not None:
                ec.join_side_stream()       # idempotent; the accumulate launch below reads weight gradients of the side streams
            grads = [p.grad for p in params]
            if acc is None:
                acc = grads
            else:
                if any((a is None) != (g is None) for a, g in zip(acc, grads)):
                    raise RuntimeError("egoclip_step_cached: a parameter received a gradient in one chunk and none in another")
                ops.grad_accumulate_multi([a for a in acc if a is not None], [g for g in grads if g is not None])
            del grads
            if k + 1 < len(spans):
                for p in params:
                    p.grad = None
        if len(spans) > 1:
            for p, a in zip(params, acc):
                p.grad = a
    if check_replay:
        core.last_replay_max_abs_diff = diff
        core.last_cached_embeddings = (t_cache.detach(), v_cache.detach())

    # ---- the tail of step_epilogue: side streams, the (held) gradient exchange, the optimizer
    if ec is not None:
        ec.join_side_stream()
    if grad_sync is not None:
        grad_sync.finish()
    if scaler is None:
        optimizer.step()
    else:
        optimizer.step(scaler=scaler)
    clamp_loss_scale(loss_fn)       # a learnable temperature: its gradient came from pass 2, the head over the WHOLE batch
    return loss.detach()
