"""What the two towers' autograd functions share: the backward of a Linear, the gradient-plane hand-off between consecutive
backward nodes, and the host-side scaffolding of the one-C-call-per-layer paths (video_transformer._SpaceTimeBlockCFn on
egv_block_fwd / _bwd, text_transformer._TextLayerCFn on egv_text_layer_fwd / _bwd): the cached parameter struct, the geometry-keyed
workspace sizes and gradient layout, the views of the one gradient buffer.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple

import torch

from .. import _lib, ops
from .._lib import EGV as E
from ..ops import ExecContext, Planes


# The dgrad GEMMs that feed LayerNorm-backward write fp32: handing dy over as bf16 planes instead halves those bytes but measured
# 0.5 ms/step SLOWER in round 2 and within noise in round 3 (the split epilogue's VALU work and 8-byte stores / loads cost what the
# bytes save; profiles/r03_stream_ab.txt) -- the switch is gone, egv_layernorm_bwd still accepts planes (tests).


def _lin_bwd(dy, x_pl: Planes, wt: Planes, Pb, need_dx=True, dx_planes=False, params=(), ec: ExecContext = None, allow_side=True):
    """Backward of y = x W^T + b.  `dy` is fp32 [M,N] (split to bf16 planes here, one pass, no transpose) or
    already-split row-major Planes.  The SAME row-major planes feed both gradients: dgrad contracts over N
    (dy . W, weights cached transposed) and wgrad contracts over the M token rows with the TN kernel
    (dy^T x via the CDNA4 transpose read, bias gradient from the same pass).
    `params`: the parameters (weight, bias) the returned dW / db will be accumulated into by autograd; `ec`: the model's
    execution context (side stream, grid cap); `allow_side=False`: the caller reads dW / db right away on ITS stream (slices of a
    padded head), so the weight gradient stays on the current stream.
    -> (dx fp32 [M,K] | None, dW fp32 [N,K], db [N])."""
    ec = ops.DEFAULT if ec is None else ec
    alpha = 1.0
    if Pb == 4:
        # the fp16 backward: dy = ONE plane of un-clamped fp16 (a scaled gradient), X = plane 1 of the forward's own fp16 operand (the
        # weight gradient is rescaled when that plane is a1 = fp16((1 - 2^-6) x) of an f16x2 encoding), W^T an fp16 plane
        if not isinstance(dy, Planes):
            dy = ops.f16_cast(dy)
        x_pl, alpha = x_pl.bwd16()
    else:
        if not isinstance(dy, Planes):
            dy = ops.split_f32(dy, Pb)[0]
        x_pl = x_pl.bwd()              # an f16x2 forward operand hands over its bf16 plane
    M, K = x_pl.rows, x_pl.cols
    N = dy.cols
    dev = x_pl.hi.device
    # off the critical path: fills the CUs the dgrad chain leaves idle (ops.side_stream); the text tower's own backward is
    # already off the video tower's stream (ops.TEXT_SIDE_STREAM) and keeps its small wgrads where they are.
    # The side stream is only safe while autograd's AccumulateGrad STEALS dW (parameter.grad is None: zero_grad(set_to_none=True),
    # one backward per step): with a gradient already in place it enqueues `grad += dW` on the node's stream, which is not
    # ordered behind the side stream -- such wgrads (gradient accumulation, set_to_none=False) stay on the main stream.
    accumulating = any(p_ is not None and p_.grad is not None for p_ in params)
    if allow_side and ec.wgrad_side_stream and not ec.on_text_stream() and not accumulating:
        with ec.side_stream(dy.hi, dy.lo, x_pl.hi, x_pl.lo, cost=float(M) * N * K):
            dW = torch.empty((N, K), dtype=torch.float32, device=dev)
            db = ops.gemm_tn(dy, x_pl, passes=Pb, out_f32=dW, want_colsum=True, ec=ec, alpha=alpha)
    else:
        dW = torch.empty((N, K), dtype=torch.float32, device=dev)
        db = ops.gemm_tn(dy, x_pl, passes=Pb, out_f32=dW, want_colsum=True, ec=ec, alpha=alpha)
    dx = None
    if need_dx and dx_planes:      # dx feeds a kernel that consumes planes (attention backward): no fp32 copy at all
        if Pb == 4:                # dO of the fp16 attention backward: one plane of un-clamped fp16
            dx = ops.empty_planes_f16x2(M, K, dev, single=True)
            ops.gemm_nt(dy, wt, passes=4, out_planes=dx, K=N, ec=ec, grad_out=True)
        else:
            dx = ops.empty_planes(M, K, Pb, dev)
            ops.gemm_nt(dy, wt, passes=Pb, out_planes=dx, K=N, ec=ec)
    elif need_dx:
        dx = torch.empty((M, K), dtype=torch.float32, device=dev)
        ops.gemm_nt(dy, wt, passes=Pb, out_f32=dx, K=N, ec=ec)
    return dx, dW, db


# Gradient hand-off between consecutive blocks' backward passes: the LayerNorm-backward kernel that produces a block's
# input gradient d_x also emits it as split-bf16 planes (the format the previous block's GEMMs consume).  autograd only
# carries the fp32 tensor, so the planes ride along ON that tensor object (`_egv_planes`: PyTorch preserves a tensor's Python
# object, attributes included, across the engine), stamped with the tensor's version counter.  Anything that replaces the
# tensor (gradient accumulation from a second consumer, hooks that return a new tensor) drops the attribute; anything that
# modifies it in place bumps the version -- either way the consumer gets None and formats the real values itself.
PLANE_HANDOFF = {"hit": 0, "miss": 0}     # diagnostics / tests


def _attach_grad_planes(g, Pb, planes):
    g._egv_planes = (Pb, planes, g._version)
    return g


def _take_grad_planes(g_out, rows, cols, Pb):
    """-> the planes handed over with `g_out` if they are still those of its [rows, cols] values in the format of a `Pb` backward,
    else None."""
    ent = getattr(g_out, "_egv_planes", None)
    if ent is not None:
        try:
            del g_out._egv_planes
        except AttributeError:
            pass
        if ent[0] == Pb and ent[2] == g_out._version and ent[1].rows == rows and ent[1].cols == cols:
            PLANE_HANDOFF["hit"] += 1
            return ent[1]
    PLANE_HANDOFF["miss"] += 1
    return None


def gelu_grad_16bit(ec: ExecContext, M, Hd, D, P):
    """Does the fc1 epilogue of a video block save gelu'(z) in 16 bits (bf16; fp16 for the fp16 backward) instead of the fp32
    pre-activation?  When the backward runs a single product anyway and fc1 is on the big-tile kernel, whose epilogue writes it."""
    return ec.bwd_passes in (1, 4) and ops.uses_big_gemm(M, Hd, D, P)


# The operand-format plan of a video block: csrc/block_plan.h's BlockPlan, field by field and in its order (tests/test_block_plan_cpu.py
# pins this to the header, where each field is described).  Tuples of six are per Linear in the order timeattn.qkv, timeattn.proj,
# attn.qkv, attn.proj, fc1, fc2: `passes` as ops.gemm_nt takes them, `operand` 0 both planes / 1 the first alone / 2 the second alone,
# `w_fmt` an index into W_FMTS; `attn_fmt` is an index into ATTN_FMTS; `bf`: bf16 copies of the LayerNorm outputs and of h (want_bf).
class BlockPlan(namedtuple("BlockPlan", "train tail passes operand w_fmt walpha w_lo ln_f16 lnq_lo ln2_lo qkv_lo attn_lo h_lo bf qkv_fmt attn_passes "
                           "attn_fmt attn_mode_fwd attn_mode_bwd kv_fmt h_fmt z_code z_bytes bwd_passes bwd_lo saved_bf grad_fmt ln_fmt "
                           "attn_bwd_passes attn_bwd_o_lo cls_dx_mode")):
    __slots__ = ()
    W_FMTS = ("bf16", "f16x2")                               # weight-cache format names
    ATTN_FMTS = ("bf16", "bf16+f16", "f16x2", "f16")         # ops.divided_attn_fwd out_fmt names
    fp16_bwd = property(lambda self: self.bwd_passes == 4)
    wt_fmt = property(lambda self: "f16" if self.bwd_passes == 4 else "bf16")      # W^T planes of the backward
    single = property(lambda self: tuple(p == 4 for p in self.passes))           # Linears whose first operand is ONE plain fp16 plane


A1_INV = 1.0 / (1.0 - 2.0 ** -6)          # csrc/f16x2.h: a1 = fp16((1 - 2^-6) x)


@functools.lru_cache(maxsize=None)
def block_plan(P, Pb, single, train, z_bf16=False):
    """csrc/block_plan.h::block_plan for an accepted (fwd_passes, bwd_passes, f16_single, egv_block_geom.train, z_bf16)."""
    x2, h16, lo = P == 2, Pb == 4, P != 1
    one = tuple(bool(single & b) for b in (E.SINGLE_QKV, E.SINGLE_PROJ, E.SINGLE_QKV, E.SINGLE_PROJ, E.SINGLE_FC1, E.SINGLE_FC2))
    keep, tail = bool(train & E.TRAIN_KEEP), bool(train & E.TRAIN_CLS_TAIL)
    attn_passes = 3 if x2 else P
    attn_fmt = (E.ATTN_OUT_F16 if one[1] else E.ATTN_OUT_F16X2) if h16 else (E.ATTN_OUT_BF16_F16 if one[1] else E.ATTN_OUT_BF16_SPLIT)
    # (passes, operand, w_fmt) per Linear; the proj Linears by attention format
    proj = {E.ATTN_OUT_BF16_SPLIT: (attn_passes, 0, 0), E.ATTN_OUT_BF16_F16: (4, 2, 1), E.ATTN_OUT_F16X2: (2, 0, 1), E.ATTN_OUT_F16: (4, 1, 1)}[attn_fmt]
    passes, operand, w_fmt = zip(*(proj if i in (1, 3) else (4 if one[i] else P, int(one[i]), int(x2)) for i in range(6)))
    attn_mode = attn_fmt << E.ATTN_OUT_SHIFT
    return BlockPlan(
        train=keep, tail=tail, passes=passes, operand=operand, w_fmt=w_fmt,
        walpha=tuple(A1_INV if h16 and not one[i] else 1.0 for i in range(6)),
        w_lo=lo, ln_f16=x2, lnq_lo=lo and not one[0], ln2_lo=lo and not one[4], qkv_lo=lo, attn_lo=lo and attn_fmt != E.ATTN_OUT_F16,
        h_lo=lo and not one[5], bf=x2 and keep and not h16, qkv_fmt=E.OUT_F16_SPLIT if h16 else E.OUT_BF16_SPLIT, attn_passes=attn_passes,
        attn_fmt=attn_fmt, attn_mode_fwd=attn_mode | (E.ATTN_FWD_QKV_F16 if h16 else 0),
        attn_mode_bwd=attn_mode | (E.ATTN_BWD_GRAD_F16 | E.ATTN_BWD_QKV_F16 if h16 else 0), kv_fmt=E.CLS_KV_F16 if h16 else E.CLS_KV_BF16,
        h_fmt=(E.OUT_F16 if one[5] else E.OUT_F16X2) if x2 else E.OUT_BF16_SPLIT,
        z_code=(E.AUX_DGELU_F16 if h16 else E.AUX_DGELU_BF16) if z_bf16 else E.AUX_F32, z_bytes=(2 if z_bf16 else 4) if keep else 0,
        bwd_passes=Pb, bwd_lo=Pb == 3, saved_bf=x2 and not h16, grad_fmt=E.OUT_F16_GRAD if h16 else E.OUT_BF16_SPLIT,
        ln_fmt=E.LN_DX_F16 | E.LN_DY_F16 if h16 else 0, attn_bwd_passes=1 if h16 else Pb, attn_bwd_o_lo=attn_fmt == E.ATTN_OUT_BF16_SPLIT,
        cls_dx_mode=E.CLS_DX_ADD_F16 if h16 else E.CLS_DX_ADD_F32)


# ---------------------------------------------------------------------------------------------- one C call per layer
def param_struct(wc, cls, key, need_t, ln, biases, pls):
    """The parameter struct of a C layer call (`cls`: _lib.BlockParams / _lib.TextParams) from the LayerNorm affine tensors `ln`,
    the `biases` and `pls` = the (operand planes, W^T planes) pair of every weight as the weight cache `wc` hands them out; the W^T
    tables are filled only when `need_t` (the backward).  The planes are refreshed IN PLACE after an optimizer step, so the struct
    stays the same from step to step: it is kept on the model's weight cache under `key` and reused while the cache still holds
    the very same plane objects and the small parameters have not moved."""
    small = tuple(t.data_ptr() for t in ln) + tuple(b.data_ptr() for b in biases)
    hit = wc.param_structs.get(key)
    if hit is not None and hit[1] == small and all(a[0] is b[0] and a[1] is b[1] for a, b in zip(hit[0], pls)):
        return hit[2]
    n = len(pls)
    Pn, Ln = C.c_void_p * n, C.c_int64 * n

    def tables(planes):            # hi, lo (a plane set without one: null) and leading dimension of every weight
        return Pn(*[p.hi.data_ptr() for p in planes]), Pn(*[ops._p(p.lo) for p in planes]), Ln(*[p.ld for p in planes])
    prm = cls(*[t.data_ptr() for t in ln], Pn(*[b.data_ptr() for b in biases]), *tables([p for p, _ in pls]),
              *(tables([t for _, t in pls]) if need_t else (Pn(), Pn(), Ln())))
    wc.param_structs[key] = (pls, small, prm)
    return prm


# Sizes and layouts are pure functions of the geometry: the library is asked once per geometry, the answers live in ops._SIZE_CACHE
# under (entry points' prefix, ..., geometry key) next to the other workspace sizes.


def _geometry_error(name):
    return _lib.EgovlpHipError(f"{name}: unsupported geometry")


def layer_sizes(kind, key, g, n_grads):
    """-> (forward arena bytes, offsets of the `n_grads` gradients in the one gradient buffer, its floats) of the geometry struct
    `g`; `kind`: "egv_block" / "egv_text_layer", `key`: what `g` was built from."""
    ent = ops._SIZE_CACHE.get((kind, key))
    if ent is None:
        lib = _lib.lib()
        off, tot = (C.c_int64 * n_grads)(), C.c_int64()
        nb = int(getattr(lib, kind + "_fwd_arena_bytes")(C.byref(g)))
        _lib.check(getattr(lib, kind + "_grad_layout")(C.byref(g), off, C.byref(tot)), kind + "_grad_layout")
        if nb <= 0:
            raise _geometry_error(kind + "_fwd_arena_bytes")
        ent = ops._SIZE_CACHE[(kind, key)] = (nb, tuple(int(o) for o in off), int(tot.value))
    return ent


def bwd_arena_bytes(kind, key, g, *extra):
    """-> backward arena bytes of geometry `g` (`key` covers `extra`: the block's per-weight k-slices)."""
    nb = ops._SIZE_CACHE.get((kind, "bwd", key))
    if nb is None:
        nb = int(getattr(_lib.lib(), kind + "_bwd_arena_bytes")(C.byref(g), *extra))
        if nb <= 0:
            raise _geometry_error(kind + "_bwd_arena_bytes")
        ops._SIZE_CACHE[(kind, "bwd", key)] = nb
    return nb


def grad_views(grads, offsets, total):
    """The gradients of one layer as views of its one buffer (the layout is back to back)."""
    return grads.split_with_sizes([b - a for a, b in zip(offsets, offsets[1:] + (total,))])


def need_fwd_arena(arena, what):
    if arena is None:
        raise RuntimeError(f"the C {what} calls release their forward workspace after the first backward: a second backward through "
                           "the same graph (retain_graph=True) needs the per-kernel path (exec_ctx.set(block_calls=False))")
