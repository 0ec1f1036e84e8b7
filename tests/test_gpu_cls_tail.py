"""The CLS tail of the video tower's last block (egv_block_geom.train bit 1, csrc/cls_tail.hip): forward_features reads only the B CLS
rows of the last SpaceTimeBlock's output (model/video_transformer.py:330), so that block's space-attention output, space proj, norm2, fc1 /
GELU and fc2 run on B rows -- fp32 Linears from the master weights and the attention of one query row per (clip, head).

Yardsticks: fp64 torch for the pieces, the fp32 CPU oracle block (oracle/egovlp_oracle.py) for the block, the same tower with the tail
switched off for the model.  Bars: those the full path is held to in the same mode (tests/test_gpu_model.py: PARITY = 1e-3 forward and
3e-3 on gradients in 'bf16x3'; MIX_BAR = 7e-4 forward and F16_GRAD = 1e-2 on gradients in 'f16mix' with the fp16 backward)."""
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

BARS = {"bf16x3": (1e-3, 3e-3), "f16mix": (7e-4, 1e-2)}      # (forward, gradients): tests/test_gpu_model.py PARITY / 3 PARITY, MIX_BAR / F16_GRAD


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ B-row Linears
@pytest.mark.parametrize("R", [1, 3, 32, 40])
@pytest.mark.parametrize("NK", [(768, 256), (256, 1024), (1024, 256)])
def test_cls_linears_match_fp64(R, NK):
    """Forward (plain, GELU + saved pre-activation, residual; strided input rows), dgrad (plain, x gelu', accumulating into fp32 and into
    an un-clamped fp16 plane) and the rank-R wgrad with its bias gradient.  fp32 sums over K <= 1 024 (N <= 1 024, R <= 40) terms:
    rel-L2 <= 1e-5."""
    from egovlp_amd import ops
    N, K = NK
    S = 5                                     # the R rows are rows 0, S, 2 S, ... of a [R S, K] tensor, as the CLS rows of [B, S, D] are
    g = torch.Generator().manual_seed(100 * R + N + K)
    xs = torch.randn(R * S, K, generator=g)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    res = torch.randn(R * S, N, generator=g)
    dy = torch.randn(R, N, generator=g)
    x = xs[::S]
    xd, Wd, bd = x.double(), W.double(), b.double()
    z_ref = xd @ Wd.t() + bd
    xs_c, W_c, b_c, res_c, dy_c = xs.cuda(), W.cuda(), b.cuda(), res.cuda(), dy.cuda()

    y = ops.cls_linear_fwd(xs_c, W_c, b_c, rows=R, ldx=S * K)
    assert rel(y, z_ref) <= 1e-5
    y, z = ops.cls_linear_fwd(xs_c, W_c, b_c, rows=R, ldx=S * K, gelu=True, want_z=True)
    assert rel(z, z_ref) <= 1e-5 and rel(y, torch.nn.functional.gelu(z_ref)) <= 1e-5
    y = ops.cls_linear_fwd(xs_c, W_c, b_c, rows=R, ldx=S * K, residual=res_c, ldr=S * N)
    assert rel(y, z_ref + res[::S].double()) <= 1e-5
    y = ops.cls_linear_fwd(xs_c, W_c, None, rows=R, ldx=S * K)
    assert rel(y, xd @ Wd.t()) <= 1e-5

    dx_ref = dy.double() @ Wd
    assert rel(ops.cls_linear_dgrad(dy_c, W_c), dx_ref) <= 1e-5
    zk = torch.randn(R, K, generator=g)
    zkd = zk.double().requires_grad_(True)
    torch.nn.functional.gelu(zkd).sum().backward()
    assert rel(ops.cls_linear_dgrad(dy_c, W_c, z=zk.cuda()), dx_ref * zkd.grad) <= 1e-5
    base = torch.randn(R * S, K, generator=g)
    acc = base.cuda()
    ops.cls_linear_dgrad(dy_c, W_c, out=acc, ldo=S * K, add=True)
    want = base.double().clone()
    want[::S] += dx_ref
    assert rel(acc, want) <= 1e-5
    acc16 = base.half().cuda()
    ops.cls_linear_dgrad(dy_c, W_c, out=acc16, ldo=S * K, add=True)
    want16 = base.half().double()
    want16[::S] += dx_ref
    assert rel(acc16, want16) <= 2.0 ** -11                     # one fp16 rounding of the sum
    assert torch.equal(acc16.view(R, S, K)[:, 1:], base.half().cuda().view(R, S, K)[:, 1:])     # the other rows are untouched

    dW, db = ops.cls_linear_wgrad(dy_c, xs_c, ldx=S * K)
    assert rel(dW, dy.double().t() @ xd) <= 1e-5 and rel(db, dy.double().sum(0)) <= 1e-5


# ------------------------------------------------------------------------------------------------ CLS-query attention
def _kv_planes(kv, fmt):
    from egovlp_amd import ops
    rows, cols = kv.shape
    if fmt == "f16s":
        hi = kv.half()
        lo = (kv - hi.float()).half()
        return ops.Planes(hi.cuda(), lo.cuda(), rows, cols, "f16s"), hi.double() + lo.double()
    hi = kv.bfloat16()
    lo = (kv - hi.float()).bfloat16()
    return ops.Planes(hi.cuda(), lo.cuda(), rows, cols), hi.double() + lo.double()


@pytest.mark.parametrize("fmt,passes", [("bf16", 3), ("f16s", 4)])
@pytest.mark.parametrize("Tn", [(1, 1), (2, 49), (4, 196), (16, 196), (1, 324)])
def test_cls_attention_matches_fp64(Tn, fmt, passes):
    """One query row per (clip, head) over all 1 + T n keys, B = 2, H = 2, against fp64 torch on the values the planes hold (hi + lo).
    Bars of the existing attention tests for the same formats (tests/test_gpu_attn_long.py): the forward row of fp32-grade operands 2e-5,
    lse 1e-5; dq is fp32 (2e-5); dK / dV (the CLS key row included) as split-bf16 planes 2e-5 (hi + lo = value to 2^-17), as ONE plane
    of fp16 4e-4 (the bar of a value stored as one fp16 plane)."""
    from egovlp_amd import ops
    T, n = Tn
    B, H = 2, 2
    S, D = 1 + T * n, 128
    g = torch.Generator().manual_seed(S)
    q = torch.randn(B, D, generator=g)
    kv = torch.randn(B * S, 2 * D, generator=g)
    do = torch.randn(B, D, generator=g)
    pl, kvd = _kv_planes(kv, fmt)
    qd = q.double().requires_grad_(True)
    kvd = kvd.requires_grad_(True)
    k = kvd[:, :D].reshape(B, S, H, 64).permute(0, 2, 1, 3)
    v = kvd[:, D:].reshape(B, S, H, 64).permute(0, 2, 1, 3)
    s = torch.einsum("bhd,bhjd->bhj", qd.view(B, H, 64) * 0.125, k)
    ref = torch.einsum("bhj,bhjd->bhd", s.softmax(-1), v).reshape(B, D)
    lse_ref = torch.logsumexp(s, -1)
    ref.backward(do.double())

    out, lse = ops.cls_attn_fwd(q.cuda(), pl, B, S, H)
    r_o, r_l = rel(out, ref), rel(lse, lse_ref)
    dq, dkv = ops.cls_attn_bwd(q.cuda(), pl, out, do.cuda(), lse, B, S, H, passes)
    got = dkv.hi.double() + (dkv.lo.double() if dkv.lo is not None else 0)
    r_q, r_k, r_v = rel(dq, qd.grad), rel(got[:, :D], kvd.grad[:, :D]), rel(got[:, D:], kvd.grad[:, D:])
    r_cls = rel(got.view(B, S, 2 * D)[:, 0], kvd.grad.view(B, S, 2 * D)[:, 0])
    print("cls attention %s S=%d: out %.1e lse %.1e dq %.1e dk %.1e dv %.1e (cls key row %.1e)" % (fmt, S, r_o, r_l, r_q, r_k, r_v, r_cls))
    bar = 4e-4 if passes == 4 else 2e-5
    assert r_o <= 2e-5 and r_l <= 1e-5 and r_q <= 2e-5
    assert r_k <= bar and r_v <= bar and r_cls <= bar


# ------------------------------------------------------------------------------------------------ the block
D_, H_ = 256, 4            # Hd = 4 D = 1 024
_NAMES = ("norm3.weight", "norm3.bias", "timeattn.qkv.weight", "timeattn.qkv.bias", "timeattn.proj.weight", "timeattn.proj.bias",
          "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
          "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _block(seed=0):
    from torch import nn
    from egovlp_amd.model.video_transformer import SpaceTimeBlock
    torch.manual_seed(seed)
    blk = SpaceTimeBlock(dim=D_, num_heads=H_, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), time_init='rand')
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return blk


_ORACLE = {}


def _oracle(geom):
    """The fp32 CPU oracle block on this geometry, once: input, CLS-row gradient, CLS rows of the output, dx and the 18 parameter gradients."""
    if geom not in _ORACLE:
        from oracle import egovlp_oracle as O
        B, T, n = geom
        S = 1 + T * n
        blk = _block()
        sd = {"b." + k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
        gen = torch.Generator().manual_seed(7)
        x = torch.randn(B, S, D_, generator=gen)
        g = torch.randn(B, D_, generator=gen) * 0.1
        xin = x.clone().requires_grad_(True)
        cfg = O.VideoCfg(embed_dim=D_, num_heads=H_, ln_eps=1e-6)
        out = O.space_time_block(xin, sd, "b.", cfg, n, T)
        out[:, 0].backward(g)
        _ORACLE[geom] = (blk, x, g, out[:, 0].detach(), xin.grad, {k: sd["b." + k].grad for k in _NAMES})
    return _ORACLE[geom]


def _run_block(blk, ec, x, g, geom, tail, side):
    """The C block calls on (x, g): tail -> g is the [B, D] gradient of the [B, D] output; else the full path with g on the CLS rows."""
    from egovlp_amd.model import video_transformer as vt
    B, T, n = geom
    ec.set(wgrad_side_stream=side)
    for p in blk.parameters():
        p.grad = None
    prm = dict(blk.named_parameters())
    single = 15 if ec.fwd_passes == 2 else 0       # 'f16mix': ONE fp16 product in every Linear, as in the last block of the benchmarked policy
    gm = (B, T, n, H_, 1e-6, single) + ((None, True) if tail else ())
    xin = x.clone().requires_grad_(True)
    ec.begin_step()
    y = vt._SpaceTimeBlockCFn.apply(xin, gm, ec, *[prm[k] for k in _NAMES])
    if tail:
        assert tuple(y.shape) == (B, D_)
        y.backward(g)
        cls = y.detach()
    else:
        gf = torch.zeros_like(y)
        gf[:, 0] = g
        y.backward(gf)
        cls = y.detach()[:, 0]
    ec.join_side_stream()
    torch.cuda.synchronize()
    return cls.clone(), xin.grad.clone(), {k: prm[k].grad.detach().clone() for k in _NAMES}


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix"])
@pytest.mark.parametrize("geom,side", [((3, 2, 49), False), ((2, 4, 196), True)])
def test_block_tail_matches_the_oracle(mode, geom, side):
    """egv_block_fwd / _bwd in tail mode at D = 256, Hd = 1024 (M = 297, and S = 785: the real group size; the second on the wgrad side
    stream) against the fp32 oracle block: CLS rows of the output, d_x on ALL rows and the 18 parameter gradients from a gradient on the
    CLS rows.  The distance to the full path on the same inputs is printed, not asserted."""
    from egovlp_amd import ops
    blk, x, g, y_ref, dx_ref, g_ref = _oracle(geom)
    blk = blk.cuda().train()
    ec = ops.new_context()
    if mode == "f16mix":
        ec.set_precision("f16mix", "f16")
    else:
        ec.set_precision("bf16x3")
    xc, gc = x.cuda(), g.cuda()
    y_t, dx_t, gr_t = _run_block(blk, ec, xc, gc, geom, True, side)
    y_f, dx_f, gr_f = _run_block(blk, ec, xc, gc, geom, False, side)
    fbar, gbar = BARS[mode]
    errs = {"out": rel(y_t, y_ref), "dx": rel(dx_t, dx_ref), **{k: rel(gr_t[k], g_ref[k]) for k in _NAMES}}
    full = {"out": rel(y_f, y_ref), "dx": rel(dx_f, dx_ref), **{k: rel(gr_f[k], g_ref[k]) for k in _NAMES}}
    dist = {"out": rel(y_t, y_f), "dx": rel(dx_t, dx_f), **{k: rel(gr_t[k], gr_f[k]) for k in _NAMES}}
    for k in errs:
        print("block tail %s %s %-22s vs oracle %.2e (full path %.2e)  tail vs full %.2e" % (mode, geom, k, errs[k], full[k], dist[k]))
    assert errs["out"] <= fbar, errs["out"]
    bad = {k: v for k, v in errs.items() if k != "out" and not v <= gbar}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the tower
def _tower(**kw):
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    torch.manual_seed(3)
    m = SpaceTimeTransformer(img_size=224, patch_size=16, num_classes=0, embed_dim=D_, depth=2, num_heads=H_, num_frames=4, **kw)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    m.exec_ctx.set_precision("bf16x3")
    return m.cuda().train()


def _tower_step(m, video, gout, cls_tail):
    from egovlp_amd.model import video_transformer as vt
    m.exec_ctx.set(cls_tail=cls_tail)
    for p in m.parameters():
        p.grad = None
    taps = {}
    h = m.blocks[-1].register_forward_hook(lambda _m, _a, out: taps.__setitem__("last", out))
    try:
        m.exec_ctx.begin_step()
        e = m(video)
        e.backward(gout)
        m.exec_ctx.join_side_stream()
        torch.cuda.synchronize()
    finally:
        h.remove()
    c_path = isinstance(taps["last"].grad_fn, vt._SpaceTimeBlockCFn._backward_cls)
    return e.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, taps["last"].dim() == 2, c_path


@pytest.mark.parametrize("case", ["plain", "patch_drop", "drop_path"])
def test_tower_with_the_tail_matches_the_tower_without(case):
    """A depth-2 D = 256 tower (12 clips x 4 frames: enough token rows for the C block calls) in 'bf16x3', cls_tail on against off:
    embedding inside 1e-3, every gradient inside 3e-3.  'patch_drop': patch_drop_rate = 0.5 with a fixed device seed (both runs keep
    the same tubes).  'drop_path': the last block drops paths in train mode, so it keeps the full per-kernel path."""
    kw = {"patch_drop": {"patch_drop_rate": 0.5}, "drop_path": {"drop_path_rate": 0.2}}.get(case, {})
    m = _tower(**kw)
    if case != "plain":
        m.seed_device = torch.zeros(1, dtype=torch.int64, device="cuda")     # the same draws in both runs
    gen = torch.Generator().manual_seed(11)
    video = torch.randn(12, 4, 3, 224, 224, generator=gen).cuda()
    gout = torch.randn(12, D_, generator=gen).cuda()
    e1, g1, tail1, c1 = _tower_step(m, video, gout, True)
    e0, g0, tail0, c0 = _tower_step(m, video, gout, False)
    assert not tail0
    if case == "drop_path":
        assert not tail1 and not c1              # the full path, per kernel
    else:
        assert tail1 and c1 and c0
    r = rel(e1, e0)
    errs = {k: rel(g1[k], g0[k]) for k in g0}
    print("tower %s: embedding %.2e, worst gradient %.2e (%s)" % (case, r, max(errs.values()), max(errs, key=errs.get)))
    assert r <= 1e-3
    bad = {k: v for k, v in errs.items() if not v <= 3e-3}
    assert not bad, bad
