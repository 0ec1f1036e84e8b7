"""SpaceTimeTransformer on MI355X kernels -- drop-in for the reference's model/video_transformer.py.

Same constructor, same parameter names and shapes (state_dict compatible), same
arithmetic (reference lines cited inline), different execution: one autograd node per
SpaceTimeBlock whose forward and hand-written backward are sequences of enqueues of the gfx950
kernels behind include/egovlp_hip.h.  The residual stream is fp32; every GEMM operand is a
split-bf16 plane pair produced by the epilogue of the kernel before it (LayerNorm, attention, GELU),
so no activation is ever re-formatted in a separate pass in forward.

nn.Linear / nn.LayerNorm / nn.Conv2d are used as PARAMETER CONTAINERS only (names + default init
identical to the reference); their own forward is never called.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from functools import partial
from typing import Any, NamedTuple

import torch
from torch import nn

from .. import _lib, ops
from .._lib import EGV, BlockBwdIO, BlockGeom, BlockParams
from ..ops import ACT_GELU, ACT_GELU_BWD, ExecContext
from .layer_common import (PLANE_HANDOFF, _attach_grad_planes, _lin_bwd, _take_grad_planes, bwd_arena_bytes,  # noqa: F401  (PLANE_HANDOFF: tests)
                           block_plan, gelu_grad_16bit, grad_views, layer_sizes, need_fwd_arena, param_struct)


class BlockCall(NamedTuple):      # the `geom` argument of the two block nodes; their .apply takes it or a plain tuple in this order
    B: int
    T: int
    n: int
    H: int
    eps: float
    single: int = 0       # ops.F16_SINGLE_BITS: Linears of THIS block that run ONE fp16 product (f16x2 mode)
    drop: Any = None      # stochastic depth of this forward: (p, seed_space, seed_mlp, seed_dev) or None
    tail: bool = False    # CLS tail (the tower's last block, C calls only): the output is the [B, D] CLS rows


# The `geom` argument of _PatchTokensFn.  P: patch size; mean_std: the loader's Normalize; aug = (boxes, out_res[, colour-jitter table]): the
# train transform inside the gather; eval = (center_crop, out_res, frame table): the val / test transform inside the gather; keep: patch
# dropout, int32 [B, K] kept positions on the device; mix = (mix_idx, mix_lam): Mixup / CutMix inside the gather, tables on the device
PatchCall = namedtuple("PatchCall", "B T n P D T_model mean_std aug eval keep mix",
                       defaults=((ops.IMAGENET_MEAN, ops.IMAGENET_STD), None, None, None, None))


def f16x2_block_ok(M, D, Hd, train):
    """Can a block of this size run its qkv / fc1 / fc2 Linears in the f16x2 format?  (the big-tile kernel for the three products, and
    -- the fc1 epilogue of that format saves gelu' as bf16 -- for the single-pass fc2 dgrad that reads it back; smaller blocks run
    split-bf16 x3)"""
    if not (ops.f16x2_gemm_ok(M, 3 * D, D) and ops.f16x2_gemm_ok(M, Hd, D) and ops.f16x2_gemm_ok(M, D, Hd)):
        return False
    return not train or ops.uses_big_gemm(M, Hd, D, 1)


class _SpaceTimeBlockFn(torch.autograd.Function):
    """SpaceTimeBlock.forward, model/video_transformer.py:163-177:
         t  = timeattn(norm3(x));  tr = x + t
         s  = attn(norm1(tr));     sr = x + s          (residual from x, NOT tr -- :171)
         out = sr + mlp(norm2(sr))
    With stochastic depth (:155,:171,:175; geom.drop = (p, seed_space, seed_mlp, seed_dev), set by a train-mode block with p > 0):
         sr = x + s1[b] * attn(..);  out = sr + s2[b] * mlp(..)       s[b] in {0, 1 / (1 - p)} per sample, ops.drop_path_*
    the proj / fc2 Linears then run without their residual and one egv_drop_path_add merges it; the backward scales the two branch
    gradients while it formats them (egv_drop_path_grad) from the seeds of the forward.
    """

    @staticmethod
    def forward(ctx, x, geom, ec: ExecContext,
                n3w, n3b, tqkv_w, tqkv_b, tproj_w, tproj_b,
                n1w, n1b, sqkv_w, sqkv_b, sproj_w, sproj_b,
                n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b):
        geom = BlockCall(*geom)
        B, T, n, H, eps, single, dp = geom[:7]
        S = 1 + T * n
        D = x.shape[-1]
        M = B * S
        P = ec.fwd_passes
        wc = ec.wc
        dev = x.device
        x2 = x.contiguous().view(M, D)
        save = any(ctx.needs_input_grad)    # grad mode is off inside Function.forward; this is the reliable signal
        train = ec.forward_is_train(ctx)    # = save, or the train-mode kernels were asked for under no_grad (the embedding-cache step)
        Hd = fc1_w.shape[0]
        # 'f16x2': the LayerNorm -> qkv / fc1 and fc1 -> fc2 hand-overs are in the f16x2 operand format (two fp16 products instead of
        # three bf16 ones, big-tile kernel only); attention and the proj Linears keep split-bf16 three-product operands (Pa).  Token
        # counts too small for the big-tile kernel (toy geometries) run the block in bf16x3.
        fx2 = P == 2 and f16x2_block_ok(M, D, Hd, train)
        if not fx2:
            P, single = ec.fwd_passes_split, 0
        # every format below is the plan's (csrc/block_plan.h; the backward of a block that fell back to split-bf16 is no fp16 one)
        pl = block_plan(P, ec.bwd_passes if fx2 else min(ec.bwd_passes_split, P), single, int(train), gelu_grad_16bit(ec, M, Hd, D, P))
        h16, want_bf, Pa, afmt = pl.fp16_bwd, pl.bf, pl.attn_passes, pl.ATTN_FMTS[pl.attn_fmt]
        def lin(i, a, w, **kw):        # forward Linear i of the plan on the planes `a`
            ops.gemm_nt(a, wc.get(w, need_t=False, fmt=pl.W_FMTS[pl.w_fmt[i]])[0], passes=pl.passes[i], ec=ec, **kw)

        def attn_branch(i, time, inp, nw, nb, qkv_w, qkv_b, proj_w, proj_b, residual):
            # LayerNorm -> qkv (Linear i) -> attention -> proj (Linear i + 1) + residual.  qkv never exists in fp32: the attention kernels
            # read planes (split-bf16; an fp16 split when the backward is fp16: the attention then multiplies fp16 in both directions)
            nrm, _, mean, rstd, _ = ops.layernorm_fwd(inp, nw, nb, eps, P, want_bf=want_bf, single=pl.single[i])
            qkv = ops.empty_planes_f16x2(M, 3 * D, dev, split=True) if h16 else ops.empty_planes(M, 3 * D, Pa, dev)
            lin(i, nrm, qkv_w, bias=qkv_b, out_planes=qkv)
            a, lse = ops.divided_attn_fwd(qkv, B, T, n, H, time, Pa, out_fmt=afmt)
            res = torch.empty((M, D), dtype=torch.float32, device=dev)
            lin(i + 1, a, proj_w, bias=proj_b, residual=residual, out_f32=res)
            return nrm, mean, rstd, qkv, a, lse, res

        # ---- temporal (:166-167) and spatial (:168-171) attention branches
        n3, mean3, rstd3, qkv_t, a_t, lse_t, tr = attn_branch(0, 1, x2, n3w, n3b, tqkv_w, tqkv_b, tproj_w, tproj_b, x2)
        n1, mean1, rstd1, qkv_s, a_s, lse_s, sr = attn_branch(2, 0, tr, n1w, n1b, sqkv_w, sqkv_b, sproj_w, sproj_b, None if dp else x2)
        if dp:      # sr = x + s1[b] * attn(..), in place on the branch
            ops.drop_path_add(sr, x2, S, dp[0], dp[1], dp[3])
        # ---- MLP (:175, Mlp.forward :46-52), exact-erf GELU fused into the fc1 epilogue
        n2, _, mean2, rstd2, _ = ops.layernorm_fwd(sr, n2w, n2b, eps, P, want_bf=want_bf, single=pl.single[4])
        h = ops.empty_planes_f16x2(M, Hd, dev, want_bf=want_bf, single=pl.single[5]) if fx2 else ops.empty_planes(M, Hd, P, dev)
        # saved for backward: the fp32 pre-activation z in the all-bf16x3 parity mode; when backward runs single-pass bf16
        # anyway, gelu'(z) itself as bf16 -- the epilogue has Phi(z) and phi(z) in registers, the buffer is half the bytes,
        # and the fc2-dgrad epilogue becomes one multiply instead of a second erf evaluation over 77 M elements
        # (the fp16 backward keeps gelu' as fp16: bf16's 2^-9 on the derivative would cap dZ's accuracy)
        z_dtype = {EGV.AUX_F32: torch.float32, EGV.AUX_DGELU_BF16: torch.bfloat16, EGV.AUX_DGELU_F16: torch.float16}[pl.z_code]
        z = torch.empty((M, Hd), dtype=z_dtype, device=dev) if train else None
        lin(4, n2, fc1_w, bias=fc1_b, act=ACT_GELU, aux_out=z, out_planes=h, aux_is_grad=z is not None and pl.z_code != EGV.AUX_F32)
        out = torch.empty((M, D), dtype=torch.float32, device=dev)
        lin(5, h, fc2_w, bias=fc2_b, residual=None if dp else sr, out_f32=out)
        if dp:      # out = sr + s2[b] * mlp(..)
            ops.drop_path_add(out, sr, S, dp[0], dp[2], dp[3])

        if save:
            ctx.geom, ctx.ec, ctx.P, ctx.h16 = geom, ec, P, h16
            ctx.planes = (n3, a_t, n1, a_s, n2, h, qkv_t, qkv_s)
            ctx.save_for_backward(x2, mean3, rstd3, lse_t, tr, mean1, rstd1, lse_s, sr, mean2, rstd2, z,
                                  n3w, tqkv_w, tproj_w, n1w, sqkv_w, sproj_w, n2w, fc1_w, fc2_w)
        return out.view(B, S, D)

    @staticmethod
    def backward(ctx, g_out):
        (x2, mean3, rstd3, lse_t, tr, mean1, rstd1, lse_s, sr, mean2, rstd2, z,
         n3w, tqkv_w, tproj_w, n1w, sqkv_w, sproj_w, n2w, fc1_w, fc2_w) = ctx.saved_tensors
        n3, a_t, n1, a_s, n2, h, qkv_t, qkv_s = ctx.planes
        B, T, n, H, eps, _, dp = ctx.geom[:7]          # dp: the forward's stochastic-depth draws
        ec = ctx.ec
        wc = ec.wc
        Pb = ec.bwd_passes
        ec.poll_backward()              # gradients of the blocks behind this one are final: the data-parallel exchange may start
        if Pb == 4 and not ctx.h16:
            if ec.fwd_passes == 2 and ctx.P == 2:
                raise RuntimeError("the backward precision changed to 'f16' after this block's forward (which wrote bf16 copies, not fp16 planes)")
            Pb = min(ec.bwd_passes_split, ctx.P)       # a block too small for the fp16 forward format (toy geometries) ran split-bf16
        if Pb == 3 and ctx.P != 3:
            raise RuntimeError("backward precision bf16x3 needs a bf16x3 forward (the saved activation planes carry no lo part)")
        pl = block_plan(ctx.P, Pb, 0, 1)      # (the backward's fields do not depend on which Linears ran one product)
        h16 = pl.fp16_bwd
        M, D = x2.shape
        G = g_out.contiguous().view(M, D)

        def Wt(p):
            return wc.get(p, need_t=True, fmt="f16x2" if h16 else "bf16", t_fmt=pl.wt_fmt)[1]

        S = 1 + T * n
        # ---- MLP backward.  dZ = (G . W2) * gelu'(z) comes out of the fc2-dgrad epilogue already split.
        G_pl = _take_grad_planes(g_out, M, D, Pb)
        if dp:
            # the branch gradient is s2[b] * G: planes handed over by the block behind this one are those of the un-scaled G
            G_pl = ops.drop_path_grad(G, S, dp[0], dp[2], Pb, dp[3])
        elif G_pl is None:
            G_pl = ops.f16_cast(G) if h16 else ops.split_f32(G, Pb)[0]
        Hd = fc1_w.shape[0]
        dZ = ops.empty_planes_f16x2(M, Hd, G.device, single=True) if h16 else ops.empty_planes(M, Hd, Pb, G.device)
        ops.gemm_nt(G_pl, Wt(fc2_w), passes=Pb, act=ACT_GELU_BWD, aux_in=z, out_planes=dZ, K=D,
                    aux_is_grad=z.dtype != torch.float32, ec=ec)
        _, d_fc2_w, d_fc2_b = _lin_bwd(G_pl, h, None, Pb, need_dx=False, params=(fc2_w,), ec=ec)
        ln16 = pl.grad_fmt == EGV.OUT_F16_GRAD          # fp16 backward: the dgrads in front of a LayerNorm backward hand it ONE plane of un-clamped fp16 (no fp32 copy)
        d_n2, d_fc1_w, d_fc1_b = _lin_bwd(dZ, n2, Wt(fc1_w), Pb, dx_planes=ln16, params=(fc1_w,), ec=ec)
        # d_sr = G + LN2'(d_n2)
        if dp:      # the space branch's gradient is s1[b] * d_sr, formatted from the fp32 d_sr
            d_sr, d_n2w, d_n2b = ops.layernorm_bwd(d_n2, sr, n2w, mean2, rstd2, add1=G)
            d_sr_pl = ops.drop_path_grad(d_sr, S, dp[0], dp[1], Pb, dp[3])
        else:
            d_sr, d_n2w, d_n2b, d_sr_pl = ops.layernorm_bwd(d_n2, sr, n2w, mean2, rstd2, add1=G, planes_passes=Pb)
        # ---- spatial attention backward
        d_as, d_sproj_w, d_sproj_b = _lin_bwd(d_sr_pl, a_s, Wt(sproj_w), Pb, dx_planes=True, params=(sproj_w,), ec=ec)
        d_qkv_s = ops.divided_attn_bwd(qkv_s, a_s, d_as, lse_s, B, T, n, H, 0, pl.attn_bwd_passes, grad_f16=h16)
        d_n1, d_sqkv_w, d_sqkv_b = _lin_bwd(d_qkv_s, n1, Wt(sqkv_w), Pb, dx_planes=ln16, params=(sqkv_w,), ec=ec)
        d_tr, d_n1w, d_n1b, d_tr_pl = ops.layernorm_bwd(d_n1, tr, n1w, mean1, rstd1, planes_passes=Pb)
        # ---- temporal attention backward
        d_at, d_tproj_w, d_tproj_b = _lin_bwd(d_tr_pl, a_t, Wt(tproj_w), Pb, dx_planes=True, params=(tproj_w,), ec=ec)
        d_qkv_t = ops.divided_attn_bwd(qkv_t, a_t, d_at, lse_t, B, T, n, H, 1, pl.attn_bwd_passes, grad_f16=h16)
        d_n3, d_tqkv_w, d_tqkv_b = _lin_bwd(d_qkv_t, n3, Wt(tqkv_w), Pb, dx_planes=ln16, params=(tqkv_w,), ec=ec)
        # x feeds norm3, the tr residual and the sr residual: dx = d_tr + d_sr + LN3'(d_n3)
        d_x, d_n3w, d_n3b, d_x_pl = ops.layernorm_bwd(d_n3, x2, n3w, mean3, rstd3, add1=d_tr, add2=d_sr,
                                                       planes_passes=Pb)
        return (_attach_grad_planes(d_x.view(B, S, D), Pb, d_x_pl), None, None,
                d_n3w, d_n3b, d_tqkv_w, d_tqkv_b, d_tproj_w, d_tproj_b,
                d_n1w, d_n1b, d_sqkv_w, d_sqkv_b, d_sproj_w, d_sproj_b,
                d_n2w, d_n2b, d_fc1_w.view_as(fc1_w), d_fc1_b, d_fc2_w.view_as(fc2_w), d_fc2_b)


# ---------------------------------------------------------------------------------------------- one C call per block
# The same block through egv_block_fwd / egv_block_bwd (csrc/block.hip): the C side enqueues the block's kernels with pointers into
# one workspace arena per direction.  What stays in Python is policy: which precision, which stream each weight gradient goes to,
# how many k-slices it gets, the gradient-plane hand-over between blocks, the backward poll of the gradient exchange.


def block_calls_ok(ec: ExecContext, M, D, Hd, drop_path=False):
    """May this block run through the C block calls?  (split-bf16 / bf16 precision, no per-kernel timer attached, every GEMM of
    the block un-split and at least one 256-wide tile: the per-kernel path covers the toy shapes, and every forward that drops
    paths -- `drop_path`: stochastic depth is not in the C calls)"""
    if drop_path or not ec.block_calls or ec.kernel_timer is not None or (ec.bwd_passes == 3 and ec.fwd_passes != 3) or \
            (ec.bwd_passes == 4 and ec.fwd_passes != 2):
        return False
    if ec.fwd_passes == 2 and not f16x2_block_ok(M, D, Hd, True):
        return False
    if D < 256 or Hd < 256 or D % 64 or Hd % 64 or M < 256:
        return False
    return all(ops.auto_ksplit_nt(*sh) == 1 for sh in ((M, 3 * D, D), (M, D, D), (M, Hd, D), (M, D, Hd), (M, D, 3 * D)))


def _block_geom(B, T, n, H, D, Hd, P, Pb, train, z_bf16, single, eps, grid, tail=False):
    # egv_block_geom.train: keep what the backward needs; CLS tail (only the B CLS rows of the output are wanted)
    return BlockGeom(B, T, n, H, D, Hd, P, Pb, (EGV.TRAIN_KEEP if train else 0) | (EGV.TRAIN_CLS_TAIL if tail else 0), int(z_bf16), float(eps), int(grid), int(single))


def cls_tail_ok(ec: ExecContext, M, D):
    """May the LAST block of a tower that runs through the C block calls compute the CLS rows of its output only?  (the setting, and
    the space qkv GEMMs restricted to the k / v rows -- N = 2 D forward, K = 2 D in the dgrad -- un-split like the block's other GEMMs)"""
    if not ec.cls_tail:
        return False
    if ec.fwd_passes == 2 and not ops.f16x2_gemm_ok(M, 2 * D, D):
        return False
    return all(ops.auto_ksplit_nt(*sh) == 1 for sh in ((M, 2 * D, D), (M, D, 2 * D)))


def _tail_params(prm, weights, need_t):
    """egv_block_params of a CLS-tail call: a copy of `prm` in which the fp32 master weights of attn.qkv, attn.proj, fc1, fc2 (read by the
    B-row Linears, csrc/cls_tail.hip) travel in the plane slots of the OTHER direction, which that call does not read -- wt_hi[2..5]
    in the forward, w_hi[2..5] in the backward (contiguous [N, K] fp32)."""
    out = BlockParams.from_buffer_copy(prm)
    slot = out.w_hi if need_t else out.wt_hi
    for i in range(2, 6):
        w = weights[i]
        if w.dtype != torch.float32 or not w.is_contiguous():
            raise ValueError("the CLS tail reads the fp32 master weights: contiguous float32 parameters")
        slot[i] = w.data_ptr()
    return out


def _block_params(wc, ln, biases, weights, need_t, pl=block_plan(3, 3, 0, 1)):
    """egv_block_params from the parameter tensors: LayerNorm affine (n3w, n3b, n1w, n1b, n2w, n2b), the six biases and the
    cached operand planes of the six weights (W^T planes too when `need_t`), kept on the model's weight cache, keyed by the block's
    first weight, the direction and the formats (layer_common.param_struct)."""
    # `pl`: the block's plan -- the format of each weight's forward planes and of the W^T planes (default: split-bf16 everywhere)
    pls = [wc.get(w, need_t=need_t, fmt=pl.W_FMTS[pl.w_fmt[i]], t_fmt=pl.wt_fmt) for i, w in enumerate(weights)]
    return param_struct(wc, BlockParams, (id(weights[0]), need_t, pl.w_fmt, pl.wt_fmt), need_t, ln, biases, pls)


class _SpaceTimeBlockCFn(torch.autograd.Function):
    """SpaceTimeBlock.forward / backward as ONE C-ABI call each (see _SpaceTimeBlockFn for the arithmetic)."""

    @staticmethod
    def forward(ctx, x, geom, ec: ExecContext,
                n3w, n3b, tqkv_w, tqkv_b, tproj_w, tproj_b,
                n1w, n1b, sqkv_w, sqkv_b, sproj_w, sproj_b,
                n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b):
        geom = BlockCall(*geom)
        B, T, n, H, eps = geom[:5]
        S = 1 + T * n
        D = x.shape[-1]
        M = B * S
        Hd = fc1_w.shape[0]
        P, Pb = ec.fwd_passes, ec.bwd_passes
        single = geom.single if P == 2 else 0
        dev = x.device
        x2 = x.contiguous().view(M, D)
        save = any(ctx.needs_input_grad)
        train = ec.forward_is_train(ctx)
        tail = bool(geom.tail)
        key = (B, T, n, H, D, Hd, P, Pb, train, gelu_grad_16bit(ec, M, Hd, D, P), single)
        g = _block_geom(*key, eps, ec.gemm_grid, tail)
        ent = layer_sizes("egv_block", key + (tail,), g, 18)
        arena = torch.empty(ent[0], dtype=torch.uint8, device=dev)
        out = torch.empty((B if tail else M, D), dtype=torch.float32, device=dev)
        ln = (n3w, n3b, n1w, n1b, n2w, n2b)
        biases = (tqkv_b, tproj_b, sqkv_b, sproj_b, fc1_b, fc2_b)
        weights = (tqkv_w, tproj_w, sqkv_w, sproj_w, fc1_w, fc2_w)
        prm = _block_params(ec.wc, ln, biases, weights, False, block_plan(P, Pb, single, int(train)))
        if tail:
            prm = _tail_params(prm, weights, need_t=False)
        _lib.check(_lib.lib().egv_block_fwd(C.byref(g), C.byref(prm), x2.data_ptr(), out.data_ptr(), arena.data_ptr(), ops._stream(x2)),
                   "egv_block_fwd")
        if save:
            ctx.key, ctx.eps, ctx.ec, ctx.arena, ctx.sizes, ctx.tail = key, eps, ec, arena, ent, tail
            ctx.save_for_backward(x2, *ln, *biases, *weights)
        return out if tail else out.view(B, S, D)

    @staticmethod
    def backward(ctx, g_out):
        saved = ctx.saved_tensors
        x2, ln, biases, weights = saved[0], saved[1:7], saved[7:13], saved[13:19]
        need_fwd_arena(ctx.arena, "block")
        B, T, n, H, D, Hd, P, Pb, train, z_bf16, single = ctx.key
        ec = ctx.ec
        pl = block_plan(P, Pb, single, int(train))
        ec.poll_backward()              # gradients of the blocks behind this one are final: the data-parallel exchange may start
        Pb_now = ec.bwd_passes
        if Pb_now != Pb:
            raise RuntimeError("the backward precision changed between this block's forward and its backward")
        S = 1 + T * n
        M = B * S
        dev = x2.device
        tail = ctx.tail
        G = g_out.contiguous().view(B if tail else M, D)
        # the gradient-plane hand-over of the block behind this one (layer_common._attach_grad_planes); without it the C side formats G
        # (the CLS tail takes its [B, D] gradient as fp32)
        g_pl = None if tail else _take_grad_planes(g_out, M, D, Pb)
        g_hi, g_lo = (g_pl.hi.data_ptr(), ops._p(g_pl.lo)) if g_pl is not None else (None, None)
        # weight gradients in the order the C side enqueues them (fc2, fc1, attn.proj, attn.qkv, timeattn.proj, timeattn.qkv): stream,
        # event and k-slices of each -- the policy of _lin_bwd / ops.gemm_tn
        shapes = [(w.shape[0], w[0].numel()) for w in weights]
        order = (5, 4, 3, 2, 1, 0)
        side_ok = ec.wgrad_side_stream and not ec.on_text_stream()
        use = [side_ok and weights[i].grad is None for i in range(6)]
        deal = ec.assign_side_streams([float(M) * shapes[i][0] * shapes[i][1] for i in order if use[i]]) if any(use) else []
        streams, events = [None] * 6, [None] * 6
        it = iter(deal)
        for i in order:
            if use[i]:
                streams[i], events[i] = next(it)
        if tail:        # the big space qkv weight gradient covers the k / v rows; attn.proj / fc1 / fc2 are rank-B updates (no k-slices)
            shapes[2] = (2 * D, D)
        ks = [1 if tail and i > 2 else ops.wgrad_ksplit(shapes[i][0], shapes[i][1], M, ec, use[i]) for i in range(6)]
        g = _block_geom(*ctx.key, ctx.eps, ec.gemm_grid, tail)
        ks6 = (C.c_int32 * 6)(*ks)
        barena = torch.empty(bwd_arena_bytes("egv_block", (ctx.key, tail, tuple(ks)), g, ks6), dtype=torch.uint8, device=dev)
        _, goff, gtot = ctx.sizes
        grads = torch.empty(gtot, dtype=torch.float32, device=dev)
        d_x = torch.empty((M, D), dtype=torch.float32, device=dev)
        dx_pl = ops.empty_planes_f16x2(M, D, dev, single=True) if pl.grad_fmt == EGV.OUT_F16_GRAD else ops.empty_planes(M, D, Pb, dev)
        used = {s_ for s_ in streams if s_ is not None}          # the side streams read / write these allocations of the main stream
        if used:
            # held until the side streams are joined (end of backward) instead of record_stream-ed: the multi-GB arenas (see
            # hold_until_join), the gradient buffer, and the gradient planes handed over by the block behind this one -- BOTH planes (a
            # bf16x3 backward reads the lo plane in the fc2 weight gradient as well).  record_stream leaves an event per block and
            # stream with the caching allocator, which polls every outstanding event on every allocation: with 24 blocks and a host
            # that runs two steps ahead that was ~10 ms of host time per ViT-L/14 step (host_enqueue 26 ms against 16 from idle).
            ec.hold_until_join(ctx.arena, barena, grads, *((g_pl.hi, g_pl.lo) if g_pl is not None else ()))
        prm = _block_params(ec.wc, ln, biases, weights, True, pl)
        if tail:
            prm = _tail_params(prm, weights, need_t=True)
        P6 = C.c_void_p * 6
        io = BlockBwdIO(G.data_ptr(), g_hi, g_lo, x2.data_ptr(), ctx.arena.data_ptr(), barena.data_ptr(),
                        d_x.data_ptr(), dx_pl.hi.data_ptr(), ops._p(dx_pl.lo), grads.data_ptr(),
                        P6(*[s_.cuda_stream if s_ is not None else None for s_ in streams]),
                        P6(*[e.cuda_event if e is not None else None for e in events]), ks6)
        _lib.check(_lib.lib().egv_block_bwd(C.byref(g), C.byref(prm), C.byref(io), ops._stream(x2)), "egv_block_bwd")
        ctx.arena = None

        parts = grad_views(grads, goff, gtot)                 # 18 views of the one buffer
        dW = [parts[i].view(weights[i].shape) for i in range(6)]
        db = parts[6:12]
        dln = parts[12:18]                                  # norm3 g/b, norm1 g/b, norm2 g/b
        return (_attach_grad_planes(d_x.view(B, S, D), Pb, dx_pl), None, None,
                dln[0], dln[1], dW[0], db[0], dW[1], db[1],
                dln[2], dln[3], dW[2], db[2], dW[3], db[3],
                dln[4], dln[5], dW[4], db[4], dW[5], db[5])


class _PatchTokensFn(torch.autograd.Function):
    """VideoPatchEmbed (:72-77) + flatten/CLS/pos/temporal (:305-320): patch gather -> MFMA GEMM (+bias)
    -> token assembly.  No gradient flows to the input frames.  With patch dropout (geom.keep, int32 [B, K] on the device) all of it
    runs over the K kept positions of every frame: B*T*K rows in the gather, the GEMM, its saved operand and its weight gradient."""

    @staticmethod
    def forward(ctx, video, geom, ec, proj_w, proj_b, cls_token, pos_embed, temporal_embed):
        geom = PatchCall(*geom)
        B, T, n, P_, D, T_model, (mean, std), aug, ev, keep, mix = geom
        mixed = {} if mix is None else {"mix": mix}             # no mix: the calls made without the argument
        Pp = ec.fwd_passes_split
        wc = ec.wc
        if ev is not None:
            # the val / test transform inside the gather: `video` is the uint8 frame bank, ev = (center_crop, out_res, frame table)
            a = ops.patch_gather_eval(video.contiguous(), ev[2], T, P_, Pp, ev[0], ev[1], mean, std)
        else:
            # uint8 frames: /255 + Normalize (and, with `aug`, the train transform's crop / resize / flip) inside the gather
            if aug is not None and len(aug) > 2:       # (boxes, out_res, colour-jitter table)
                a = ops.patch_gather(video.contiguous(), P_, Pp, mean, std, aug=aug[:2], keep=keep, color=aug[2], **mixed)
            else:
                a = ops.patch_gather(video.contiguous(), P_, Pp, mean, std, aug=aug, keep=keep, **mixed)
        K = proj_w[0].numel()
        if a.cols == K:
            w_pl = wc.get(proj_w, need_t=False)[0]
        else:   # ViT-L/14: K = 588 is zero-padded to the 64-deep k-tile on both operands
            w_pl = ops.split_f32(torch.nn.functional.pad(proj_w.detach().reshape(D, K), (0, a.cols - K)), Pp)[0]
        pe = torch.empty((a.rows, D), dtype=torch.float32, device=video.device)
        ops.gemm_nt(a, w_pl, passes=Pp, bias=proj_b, out_f32=pe, ec=ec)
        x = ops.assemble_tokens(pe, cls_token, pos_embed, temporal_embed, B, T, n, D, keep=keep)
        ctx.geom, ctx.a, ctx.Pp, ctx.ec = geom._replace(keep=None, mix=None), a, Pp, ec
        ctx.save_for_backward(*(() if keep is None else (keep,)))
        ctx.wshape, ctx.proj_w = proj_w.shape, proj_w
        return x

    @staticmethod
    def backward(ctx, dx):
        B, T, n, P_, D, T_model = ctx.geom[:6]
        ec = ctx.ec
        # next to an fp16 backward of the blocks: ONE bf16 product.  This wgrad is the last GEMM of backward (nothing left to hide it under),
        # its dY carries the blocks' 2.5e-3 already, and three products would cost 0.12 ms on the tail for 3.5e-3 -> 2.5e-3 on this one tensor
        Pb = 1 if ec.bwd_passes == 4 else ec.bwd_passes
        ec.poll_backward()              # every block's gradients are final here
        keep = ctx.saved_tensors[0] if ctx.saved_tensors else None
        d_pe, d_cls, d_pos, d_tmp = ops.assemble_tokens_bwd(dx.contiguous(), B, T, n, D, T_model, keep=keep)
        K = ctx.wshape[1] * ctx.wshape[2] * ctx.wshape[3]
        # a zero-padded K (ViT-L/14: 588 -> 640) is cut off dW right here, on THIS stream: that wgrad must not run on a side stream
        # (bench.py's grad_rel_err had this gradient 100 % off in config 5 with the wgrad side streams on, rounds 3 - 4)
        _, d_w, d_b = _lin_bwd(d_pe, ctx.a, None, Pb, need_dx=False, params=(ctx.proj_w,), ec=ec, allow_side=(ctx.a.cols == K))
        if d_w.shape[1] != K:
            d_w = d_w[:, :K].contiguous()      # drop the zero-padded k columns
        return None, None, None, d_w.view(ctx.wshape), d_b, d_cls, d_pos, d_tmp


class _ClsNormFn(torch.autograd.Function):
    """`self.norm(x)[:, 0]` (:330): LayerNorm is per token, so only the B CLS rows are normalised."""

    @staticmethod
    def forward(ctx, x, w, b, eps, ec):
        xc = x.contiguous()
        if x.dim() == 2:                # the last block ran its CLS tail: x IS the [B, D] CLS rows
            _, y, mean, rstd, _ = ops.layernorm_fwd(xc, w, b, eps, 1, want_f32=True, want_planes=False)
        else:
            B, S, D = x.shape
            _, y, mean, rstd, _ = ops.layernorm_fwd(xc.view(B * S, D), w, b, eps, 1, want_f32=True, want_planes=False,
                                                    rows=B, ldx=S * D)
        ctx.save_for_backward(xc, w, mean, rstd)
        ctx.ec = ec
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, w, mean, rstd = ctx.saved_tensors
        ctx.ec.poll_backward()          # first node of the video tower's backward: what ran before it (the text tower) is final
        if xc.dim() == 2:               # a [B, D] gradient for the CLS tail: no zero fill of [B, S, D]
            dx, dg, db = ops.layernorm_bwd(dy.contiguous(), xc, w, mean, rstd)
            return dx, dg, db, None, None
        B, S, D = xc.shape
        dx = ops.zeros(tuple(xc.shape), device=xc.device)     # only the B CLS rows receive a gradient
        _, dg, db = ops.layernorm_bwd(dy.contiguous(), xc.view(B * S, D), w, mean, rstd, rows=B, ldx=S * D,
                                      dx=dx.view(B * S, D), lddx=S * D)
        return dx, dg, db, None, None


def to_2tuple(x):
    return x if isinstance(x, tuple) else (x, x)


class Mlp(nn.Module):
    """Parameter container for model/video_transformer.py:36-52 (fc1 -> GELU -> fc2)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if drop != 0.:
            raise NotImplementedError("dropout > 0 is not on the EgoClip hot path (video drop rates are all 0)")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)


class VideoPatchEmbed(nn.Module):
    """model/video_transformer.py:55-77."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=8):
        super().__init__()
        img_size = to_2tuple(img_size)
        patch_size = to_2tuple(patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0]) * num_frames
        self.num_frames = num_frames
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class VarAttention(nn.Module):
    """Parameter container for model/video_transformer.py:80-98 (incl. the 'zeros' initialisation :90-96)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.,
                 initialize='random'):
        super().__init__()
        if attn_drop != 0. or proj_drop != 0.:
            raise NotImplementedError("attention dropout is 0 on the EgoClip hot path")
        if dim // num_heads != 64:
            raise NotImplementedError("the gfx950 attention kernels are built for head_dim 64 (ViT-B/16, ViT-L/14)")
        if qk_scale is not None and qk_scale != 64 ** -0.5:
            raise NotImplementedError("qk_scale override is not supported")
        self.num_heads = num_heads
        self.scale = 64 ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        if initialize == 'zeros':
            self.qkv.weight.data.fill_(0)
            self.qkv.bias.data.fill_(0)
            self.proj.weight.data.fill_(1)
            self.proj.bias.data.fill_(0)


class SpaceTimeBlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, time_init='zeros',
                 attention_style='frozen-in-time'):
        super().__init__()
        if not 0. <= drop_path < 1.:
            raise ValueError("drop_path is a probability in [0, 1)")
        self.drop_path = float(drop_path)     # :155 (timm DropPath, scale_by_keep): Identity at 0, as in the reference
        if attention_style != 'frozen-in-time':
            raise NotImplementedError  # model/video_transformer.py:173
        self.norm1 = norm_layer(dim)
        self.attn = VarAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                 attn_drop=attn_drop, proj_drop=drop)
        self.timeattn = VarAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                     attn_drop=attn_drop, proj_drop=drop, initialize=time_init)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.norm3 = norm_layer(dim)
        self.num_heads = num_heads
        self.attention_style = attention_style

    def forward(self, x, B, T, n, ec, drop_seeds=None, cls_only=False):
        """`drop_seeds` = (seed_space, seed_mlp, seed_dev): this forward's stochastic-depth seeds (SpaceTimeTransformer._seed); without
        them, in eval() and at drop_path == 0 the block is the deterministic one.  `cls_only` (the tower's last block): the caller
        reads the CLS rows only -- the block MAY then return them as [B, D] (the CLS tail: C block calls, no dropped paths,
        `ec.cls_tail`) instead of [B, S, D]."""
        # which Linears of THIS block run one fp16 product in the f16x2 mode: the model's precision policy (ops.single_product_policy)
        single = ec.f16_single_mask(getattr(self, "layer_index", None), getattr(self, "depth", None)) if ec.fwd_passes == 2 else 0
        geom = BlockCall(B, T, n, self.num_heads, self.norm1.eps, single)
        if self.training and self.drop_path > 0.:
            if drop_seeds is None:
                raise ValueError("SpaceTimeBlock: a train-mode forward with drop_path > 0 needs its seeds (drop_seeds)")
            geom = geom._replace(drop=(self.drop_path,) + tuple(drop_seeds))
        fn = _SpaceTimeBlockCFn if block_calls_ok(ec, B * (1 + T * n), x.shape[-1], self.mlp.fc1.weight.shape[0], drop_path=geom.drop is not None) \
            else _SpaceTimeBlockFn
        if cls_only and fn is _SpaceTimeBlockCFn and cls_tail_ok(ec, B * (1 + T * n), x.shape[-1]):
            geom = geom._replace(tail=True)
        return fn.apply(
            x, geom, ec,
            self.norm3.weight, self.norm3.bias, self.timeattn.qkv.weight, self.timeattn.qkv.bias,
            self.timeattn.proj.weight, self.timeattn.proj.bias,
            self.norm1.weight, self.norm1.bias, self.attn.qkv.weight, self.attn.qkv.bias,
            self.attn.proj.weight, self.attn.proj.bias,
            self.norm2.weight, self.norm2.bias, self.mlp.fc1.weight, self.mlp.fc1.bias,
            self.mlp.fc2.weight, self.mlp.fc2.bias)


class SpaceTimeTransformer(nn.Module):
    """Drop-in for model/video_transformer.py:180-338 (same ctor signature :196-199)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., hybrid_backbone=None, norm_layer=None,
                 num_frames=8, time_init='rand', attention_style='frozen-in-time', patch_drop_rate=0.):
        super().__init__()
        if hybrid_backbone is not None:
            raise NotImplementedError('hybrid backbone not implemented')       # :231
        if drop_rate != 0. or attn_drop_rate != 0.:
            raise NotImplementedError("element-wise dropout is not in the video tower (stochastic depth is: drop_path_rate)")
        if not 0. <= drop_path_rate < 1.:
            raise ValueError("drop_path_rate is a probability in [0, 1)")
        if representation_size:
            raise NotImplementedError("representation_size (pre_logits) is not on the EgoClip hot path")
        if num_frames > ops.TIME_ATTN_MAX_FRAMES:
            raise ValueError("num_frames = %d: the time attention takes at most %d frames" % (num_frames, ops.TIME_ATTN_MAX_FRAMES))
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.num_frames = num_frames
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)             # :228
        self.patch_embed = VideoPatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans,
                                           embed_dim=embed_dim, num_frames=num_frames)
        num_patches = self.patch_embed.num_patches
        self.patches_per_frame = num_patches // num_frames
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patches_per_frame + 1, embed_dim))
        self.temporal_embed = nn.Parameter(torch.zeros(1, num_frames, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]     # :246, stochastic depth decay rule
        self.drop_path_rate, self.dpr = float(drop_path_rate), dpr
        self.blocks = nn.ModuleList([
            SpaceTimeBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                           qk_scale=qk_scale, drop_path=dpr[i], norm_layer=norm_layer, time_init=time_init,
                           attention_style=attention_style)
            for i in range(depth)])
        for i, blk in enumerate(self.blocks):
            blk.layer_index, blk.depth = i, depth     # the precision policy is per block (ExecContext.f16_single_mask)
        self.norm = norm_layer(embed_dim)
        self.pre_logits = nn.Identity()
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.pos_embed, std=.02, a=-2., b=2.)            # :264-265
        nn.init.trunc_normal_(self.cls_token, std=.02, a=-2., b=2.)
        if num_frames == 1:                                                    # :272-273
            self.apply(self._init_weights)
        # patch dropout (extension; timm's patch_drop_rate, FLIP's masking): a train-mode forward runs the tower on K = max(1, int(n * (1 -
        # rate))) of the n patch positions of every clip, the same positions in all its frames (a tube: the time attention attends over one
        # position across frames, :114); eval() sees all patches.  `last_patch_keep`: the int32 [B, K] device table of the last train-mode
        # forward that dropped (tests, debugging), else None.
        self.set_patch_drop_rate(patch_drop_rate)
        self.last_patch_keep = None
        self.exec_ctx = ops.new_context()     # FrozenInTime replaces it with the dual encoder's shared context
        # stochastic-depth seeds, as the text tower's dropout seeds (text_transformer.DistilBertModel): a call counter advanced by every
        # train-mode forward that drops paths or patches, the data-parallel rank, an optional capture-safe device word XOR-ed in by the kernels
        # (the counter stops while it is set), and a site id per block and branch (and one for the patch-dropout table)
        self._drop_calls = 0
        self.seed_rank = 0
        self.seed_device = None

    def _seed(self, site):
        # 64-bit seed of one drop-path site of one forward call: torch's seed, the call counter, the site id and the rank, mixed
        x = (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._drop_calls * 0xD1B54A32D192ED03 + site * 0x94D049BB133111EB
             + self.seed_rank * 0xA24BAED4963EE407) & (2 ** 64 - 1)
        x ^= x >> 31
        return (x * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)

    def drop_path_seeds(self, layer):
        """(seed_space, seed_mlp, seed_dev) of block `layer` at the CURRENT call counter: what its last train-mode forward drew from."""
        # sites 4096 + ...: apart from the text tower's dropout sites, which share the formula
        return self._seed(4096 + 2 * layer), self._seed(4097 + 2 * layer), self.seed_device

    PATCH_DROP_SITE = 2048      # apart from the text tower's sites (0 ..) and the drop-path sites (4096 + ..)

    def set_patch_drop_rate(self, rate):
        """Change the patch-dropout rate between epochs (FLIP's last, unmasked epochs: set_patch_drop_rate(0.))."""
        rate = float(rate)
        if not 0. <= rate < 1.:
            raise ValueError("patch_drop_rate is a probability in [0, 1)")
        self.patch_drop_rate = rate

    def patch_keep_count(self, n=None):
        """K, the patch positions a train-mode forward keeps of n per frame (timm's rule)."""
        n = self.patches_per_frame if n is None else n
        return max(1, int(n * (1. - self.patch_drop_rate)))

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02, a=-2., b=2.)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def set_input_augmentation(self, boxes, out_res=None, color=None):
        """Fuse the loader's train transform into the NEXT forward: `boxes` int32 [B, 5] (top, left, h, w, flip; see
        egovlp_amd.data_loader.transforms.train_transform_params) select, per clip, the region of the decoded uint8 frames
        that is resized to `out_res` (default: the model's img_size), flipped and normalised inside the patch gather.
        `color` (float [B, 4]: brightness factor, saturation factor, hue shift, op code -- train_transform_params_color): the
        transform's ColorJitter, applied per clip between the flip and Normalize.  A host-resident table is validated here; a
        device table is taken as it is (no sync; the kernel masks the code and a bad factor spoils that clip's pixels only).
        One-shot: consumed by the next forward_features call."""
        if getattr(self, "_input_eval", None) is not None:
            raise ValueError("set_input_augmentation: an eval transform is pending for the next forward (set_input_eval_transform)")
        host = boxes.detach().to(dtype=torch.int64).cpu() if not boxes.is_cuda else None     # checked against the frame size in forward
        if host is not None and (host.dim() != 2 or host.shape[1] != 5 or bool((host[:, :2] < 0).any()) or bool((host[:, 2:4] < 1).any())):
            raise ValueError("set_input_augmentation: boxes are int [B, 5] rows (top >= 0, left >= 0, h >= 1, w >= 1, flip)")
        aug = (boxes.to(device=self.cls_token.device, dtype=torch.int32).contiguous(), int(out_res or self.patch_embed.img_size[0]), host)
        if color is not None:
            if not torch.is_tensor(color) or not color.is_floating_point() or color.dim() != 2 or tuple(color.shape) != (boxes.shape[0], 4):
                raise ValueError("set_input_augmentation: color is a float [B, 4] table (brightness, saturation, hue, op code), one row per box")
            if not color.is_cuda:
                c = color.detach().double()
                code = c[:, 3]
                if not bool(torch.isfinite(c).all()) or bool((c[:, :2] < 0).any()) or bool((c[:, 2].abs() > 0.5).any()) \
                        or bool((code != code.round()).any()) or bool((code < 0).any()) or bool((code > 63).any()):
                    raise ValueError("set_input_augmentation: color rows are finite, brightness and saturation factors >= 0, "
                                     "|hue shift| <= 0.5, op code an integer in 0..63")
            aug = aug + (color.to(device=self.cls_token.device, dtype=torch.float32).contiguous(),)
        self._input_aug = aug

    def set_input_mix(self, mix_idx, mix_lam):
        """Mixup / CutMix inside the patch gather of the NEXT forward (egovlp_amd.data_loader.transforms.mix_params draws the tables):
        `mix_idx` int [B, 6] rows (partner, op, y0, y1, x0, x1) -- op 0 nothing, 1 mixup, 2 cutmix, the box in rows / columns of the
        frame the tower patches -- and `mix_lam` float [B].  Clip b becomes lam * A_b + (1 - lam) * A_partner (mixup) or takes the
        partner's pixels inside the box (cutmix), with A_x the transformed clip x; it combines with fp32 and uint8 input,
        set_input_augmentation and patch dropout, and not with set_input_eval_transform.  Host-resident tables are validated here
        (partner in [0, B), lam finite in [0, 1]); device tables are taken as they are (no sync; the kernels clamp what they read).
        One-shot: consumed by the next forward_features call."""
        if getattr(self, "_input_eval", None) is not None:
            raise ValueError("set_input_mix: an eval transform is pending for the next forward (set_input_eval_transform)")
        if not torch.is_tensor(mix_idx) or mix_idx.is_floating_point() or mix_idx.dtype == torch.bool or mix_idx.dim() != 2 \
                or mix_idx.shape[1] != 6 or mix_idx.shape[0] < 1:
            raise ValueError("set_input_mix: mix_idx is an int [B, 6] table (partner, op, y0, y1, x0, x1)")
        B = mix_idx.shape[0]
        if not torch.is_tensor(mix_lam) or not mix_lam.is_floating_point() or tuple(mix_lam.shape) != (B,):
            raise ValueError(f"set_input_mix: mix_lam is a float [{B}] table, one weight per row of mix_idx")
        if not mix_idx.is_cuda and (bool((mix_idx[:, 0] < 0).any()) or bool((mix_idx[:, 0] >= B).any())):
            raise ValueError(f"set_input_mix: a partner lies outside the batch of {B} clips")
        if not mix_lam.is_cuda:
            lam = mix_lam.detach().double()
            if not bool(torch.isfinite(lam).all()) or bool((lam < 0).any()) or bool((lam > 1).any()):
                raise ValueError("set_input_mix: mix_lam values are finite and lie in [0, 1]")
        dev = self.cls_token.device
        self._input_mix = (mix_idx.to(device=dev, dtype=torch.int32).contiguous(), mix_lam.to(device=dev, dtype=torch.float32).contiguous())

    def set_input_eval_transform(self, center_crop=256, out_res=None, frame_index=None):
        """Fuse the loader's val / test transform (Resize(center_crop) -> CenterCrop(center_crop) -> Resize(out_res) -> Normalize,
        data_loader/transforms.py:49-60) into the NEXT forward: it takes decoded uint8 frames [b, T, C, Hs, Ws] and resizes, crops
        and normalises them inside the patch gather (`out_res` defaults to the model's img_size).  With `frame_index` (int [b, T])
        the next forward takes a uint8 frame BANK [F, C, Hs, Ws] instead and row i of the table names the T bank frames of clip
        i -- the windows of a long clip without a copy of its frames (egovlp_amd.extract).  A host table is validated against the
        bank in forward; a device table is clamped into it by the kernel.  One-shot, and not combinable with
        set_input_augmentation."""
        if getattr(self, "_input_aug", None) is not None:
            raise ValueError("set_input_eval_transform: a train augmentation is pending for the next forward (set_input_augmentation)")
        if getattr(self, "_input_mix", None) is not None:
            raise ValueError("set_input_eval_transform: a Mixup / CutMix table is pending for the next forward (set_input_mix)")
        S, R = int(center_crop), int(out_res or self.patch_embed.img_size[0])
        if S < 1 or R < 1:
            raise ValueError("set_input_eval_transform: center_crop and out_res are positive sizes")
        if frame_index is not None:
            if not torch.is_tensor(frame_index) or frame_index.dim() != 2 or frame_index.numel() == 0 \
                    or frame_index.dtype not in (torch.int32, torch.int64):
                raise ValueError("set_input_eval_transform: frame_index is an int32 / int64 [b, T] table of bank frame numbers")
        self._input_eval = (S, R, frame_index)

    def forward_features(self, x):
        ev = getattr(self, "_input_eval", None)
        self._input_eval = None
        aug = getattr(self, "_input_aug", None)
        self._input_aug = None
        mix = getattr(self, "_input_mix", None)
        self._input_mix = None
        if ev is not None:
            if aug is not None:
                raise ValueError("set_input_eval_transform and set_input_augmentation are mutually exclusive")
            if mix is not None:
                raise ValueError("set_input_eval_transform and set_input_mix are mutually exclusive")
            if x.dtype != torch.uint8:
                raise ValueError("set_input_eval_transform expects decoded uint8 frames")
            if ev[2] is not None:
                if x.dim() != 4:
                    raise ValueError("set_input_eval_transform(frame_index=...): the input is a uint8 frame bank [F, C, Hs, Ws]")
                b, curr_frames = ev[2].shape
                channels = x.shape[1]
            else:
                b, curr_frames, channels = x.shape[:3]
                x = x.reshape(b * curr_frames, channels, *x.shape[3:])        # the batch is its own bank
            Hh = Ww = ev[1]                                                    # the resized crop is what gets patched
        else:
            b, curr_frames, channels, Hh, Ww = x.shape
        assert curr_frames <= self.num_frames                                  # :74
        P_ = self.patch_embed.patch_size[0]
        if aug is not None:
            if x.dtype != torch.uint8:
                raise ValueError("set_input_augmentation expects decoded uint8 frames")
            host = aug[2]
            if host is not None and (host.shape[0] != b or bool((host[:, 0] + host[:, 2] > Hh).any())
                                     or bool((host[:, 1] + host[:, 3] > Ww).any())):
                raise ValueError(f"set_input_augmentation: a crop box leaves the {Hh} x {Ww} frame (or the batch size changed)")
            aug = aug[:2] + aug[3:]                                            # (boxes, out_res[, colour-jitter table])
            Hh = Ww = aug[1]                                                   # the resized crop is what gets patched
        if mix is not None and mix[0].shape[0] != b:
            raise ValueError(f"set_input_mix: the tables have {mix[0].shape[0]} rows, the batch {b} clips")
        n = (Hh // P_) * (Ww // P_)
        if n != self.patches_per_frame:
            raise NotImplementedError("input resolution must match the positional embedding")
        # `input_norm` = (mean, std) of the loader's Normalize (data_loader/transforms.py:34-39); only used when the frames
        # arrive as decoded uint8 (then x / 255 and the normalisation are fused into the patch gather on the device)
        geom = PatchCall(b, curr_frames, n, P_, self.embed_dim, self.num_frames,
                         getattr(self, "input_norm", (ops.IMAGENET_MEAN, ops.IMAGENET_STD)), aug, ev, None, mix)
        ec = self.exec_ctx
        drops = self.training and any(blk.drop_path > 0. for blk in self.blocks)
        patch_drop = self.training and self.patch_drop_rate > 0.
        if patch_drop and ev is not None:
            raise ValueError("patch dropout (patch_drop_rate > 0 in train mode) does not combine with set_input_eval_transform: "
                             "that gather is the extraction path; call eval() or set_patch_drop_rate(0.)")
        if (drops or patch_drop) and self.seed_device is None:
            self._drop_calls += 1                                              # fresh draws in every train-mode forward: once
        kept = n                                                               # patch positions per frame the blocks see
        self.last_patch_keep = None
        if patch_drop:
            kept = self.patch_keep_count(n)
            self.last_patch_keep = ops.patch_keep_draw(b, n, kept, self._seed(self.PATCH_DROP_SITE), self.seed_device,
                                                       device=self.cls_token.device)
            geom = geom._replace(keep=self.last_patch_keep)
        x = _PatchTokensFn.apply(x, geom, ec, self.patch_embed.proj.weight, self.patch_embed.proj.bias,
                                 self.cls_token, self.pos_embed, self.temporal_embed)
        last = len(self.blocks) - 1
        for li, blk in enumerate(self.blocks):                                 # :325-328
            # only the CLS rows of the last block's output are read below (:330): it may return just those, [b, D]
            x = blk(x, b, curr_frames, kept, ec, self.drop_path_seeds(li) if drops and blk.drop_path > 0. else None, cls_only=li == last)
        x = _ClsNormFn.apply(x, self.norm.weight, self.norm.bias, self.norm.eps, ec)   # :330
        return self.pre_logits(x)

    def forward(self, x):
        x = self.forward_features(x)
        if not isinstance(self.head, nn.Identity):
            raise NotImplementedError("classification head: FrozenInTime replaces it with Identity (model/model.py:55)")
        return x
