"""Stochastic depth in the video tower on a real MI355X (`pytest -m gpu`): the three kernels of csrc/drop_path.hip against the numpy
mirror of the mask / torch / the existing formatters, a SpaceTimeBlock with dropped paths in all three backward precisions and a
depth-3 tower against the fp64 helper of tests/drop_path_ref.py (the scales are read back from the device and handed to it), and the
embedding-cache step's replay.

Bars: those the rate-0 model is held to in tests/test_gpu_model.py (forward PARITY = 1e-3, 2e-4 for the f16x2 forward; gradients 3e-3
in 'bf16x3', MIXED_GRAD = 5e-2 with the single-pass bf16 backward, F16_GRAD = 1e-2 with the fp16 backward) times 1 / (1 - p): a kept
branch is amplified by exactly that factor, and so is its rounding error.  The rate-0 error of the same block is measured in the same
run against the un-scaled bar and printed next to it.

Measured on MI355X (rel-L2 against fp64; out, worst of the 19 gradients), p = 0.5, and the rate-0 block in the same run:
  bf16x3 / bf16x3, M = 72:    out 2.2e-06 (rate 0: 1.8e-06)   timeattn.qkv.weight 1.1e-05 (rate 0: 1.0e-05)
  bf16x3 / bf16,   M = 72:    out 2.2e-06 (rate 0: 1.8e-06)   norm3.weight 6.0e-03 (rate 0: 5.1e-03)
  f16x2  / f16,    M = 7992:  out 2.0e-06 (rate 0: 1.5e-06)   timeattn.qkv.weight 5.5e-04 (rate 0: norm3.weight 5.9e-04)
  tower (depth 3, rate 0.3, 'bf16x3'): embedding 1.0e-05, worst gradient 1.8e-05; egv_drop_path_add: 0 ulp from torch on kept rows.
"""
import numpy as np
import pytest
import torch

import drop_path_ref as R

pytestmark = pytest.mark.gpu

PARITY, X2_BAR, MIXED_GRAD, F16_GRAD = 1e-3, 2e-4, 5e-2, 1e-2        # tests/test_gpu_model.py
RPS = 9                                                               # rows per sample of the toy geometry: 1 + T n, T = 2, n = 4


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int16).cpu() if t.element_size() == 2 else t.contiguous().view(torch.int32).cpu()


def dev_scales(B, p, seed, seed_dev=None):
    from egovlp_amd import ops
    s = ops.drop_path_scales(B, p, seed, seed_dev)
    torch.cuda.synchronize()
    return s.cpu()


# ------------------------------------------------------------------------------------------------ 1. scales
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed,word", [(0x0123456789ABCDEF, None), (0xF00DFACE12345678, 0x5DEECE66D1234567)])
def test_scales_equal_the_numpy_mirror(p, seed, word):
    B = 4096
    sdev = None if word is None else torch.tensor([word], dtype=torch.int64, device="cuda")
    got = dev_scales(B, p, seed, sdev).numpy()
    want = R.drop_path_scales(B, p, seed, 0 if word is None else word)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    keep = float((got != 0).mean())
    sigma = (p * (1 - p) / B) ** 0.5
    print("p = %.1f: kept %.4f (1 - p = %.1f, 4 sigma = %.4f)" % (p, keep, 1 - p, 4 * sigma))
    assert abs(keep - (1 - p)) < 4 * sigma
    if word is not None:                                     # the device word is part of the seed
        assert not np.array_equal(got, dev_scales(B, p, seed).numpy())


def test_scales_at_p_zero_are_ones():
    assert torch.equal(dev_scales(4096, 0.0, 0x0123456789ABCDEF), torch.ones(4096))


# ------------------------------------------------------------------------------------------------ 2. egv_drop_path_add
# rows: 45 = 5 samples of 9 rows (a workgroup covers 8 rows of 128 columns: 45 is no multiple), 41 = a last sample cut short,
# 17 100 = 547 200 pieces: more than the 2048 x 256 threads of the capped grid, so the grid-stride loop goes round
@pytest.mark.parametrize("rows", [45, 41, 9 * 1900])
@pytest.mark.parametrize("inplace", [False, True])
def test_drop_path_add(rows, inplace):
    from egovlp_amd import ops
    cols, p, seed = 128, 0.5, 0x0BADC0DE5EED0001
    B = (rows + RPS - 1) // RPS
    g = torch.Generator().manual_seed(rows)
    y, resid = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    s = dev_scales(B, p, seed)
    assert 0 < int((s == 0).sum()) < B
    s_row = s.repeat_interleave(RPS)[:rows]
    want = resid + s_row[:, None] * y                         # fp32 on the host: one rounding of the product, one of the sum
    yd, rd = y.cuda(), resid.cuda()
    if inplace:
        out = ops.drop_path_add(yd, rd, RPS, p, seed)
        assert out.data_ptr() == yd.data_ptr()
    else:
        out = ops.drop_path_add(yd, rd, RPS, p, seed, out=torch.full((rows, cols), float("nan"), device="cuda"))
        assert torch.equal(yd.cpu(), y)                       # the inputs are left alone
    torch.cuda.synchronize()
    assert torch.equal(rd.cpu(), resid)
    got = out.cpu()
    dropped = s_row == 0
    assert torch.equal(bits(got[dropped]), bits(resid[dropped]))                    # bitwise: out == resid
    ulp = (bits(got[~dropped]).long() - bits(want[~dropped]).long()).abs().max()
    print("rows %d: kept rows differ from torch by at most %d ulp" % (rows, int(ulp)))
    assert int(ulp) <= 1


def test_drop_path_add_does_not_read_a_dropped_branch():
    """inf / NaN in the rows of a dropped sample's branch stay out of the residual stream."""
    from egovlp_amd import ops
    p, seed = 0.5, 0x0BADC0DE5EED0001
    s = dev_scales(5, p, seed)
    b = int((s == 0).nonzero()[0])
    y = torch.randn(45, 128)
    y[b * RPS:(b + 1) * RPS] = float("nan")
    resid = torch.randn(45, 128)
    out = ops.drop_path_add(y.cuda(), resid.cuda(), RPS, p, seed).cpu()
    assert torch.equal(out[b * RPS:(b + 1) * RPS], resid[b * RPS:(b + 1) * RPS]) and bool(torch.isfinite(out).all())


def test_bad_arguments_launch_nothing():
    from egovlp_amd import _lib
    h = _lib.lib()
    a = torch.zeros(45, 128, device="cuda")
    pl = torch.zeros(45, 128, dtype=torch.int16, device="cuda")
    P = a.data_ptr()
    assert h.egv_drop_path_scales(0, 0.5, 1, None, P, None) == 1 and h.egv_drop_path_scales(4, 1.0, 1, None, P, None) == 1
    assert h.egv_drop_path_add(P, P, P, 45, 126, 9, 0.5, 1, None, None) == 1          # cols % 4
    assert h.egv_drop_path_add(P + 4, P, P, 44, 128, 9, 0.5, 1, None, None) == 1      # alignment
    assert h.egv_drop_path_add(P, P, P, 45, 128, 0, 0.5, 1, None, None) == 1
    assert h.egv_drop_path_add(P, None, P, 45, 128, 9, 0.5, 1, None, None) == 1
    assert h.egv_drop_path_grad(P, 128, 45, 128, 9, 0.5, 1, None, 2, pl.data_ptr(), None, 128, None) == 1     # passes
    assert h.egv_drop_path_grad(P, 128, 45, 128, 9, 0.5, 1, None, 3, pl.data_ptr(), None, 128, None) == 1     # no lo plane
    assert h.egv_drop_path_grad(P, 64, 45, 128, 9, 0.5, 1, None, 1, pl.data_ptr(), None, 128, None) == 1      # ldg < cols
    assert h.egv_drop_path_grad(P, 128, 45, 124, 9, 0.5, 1, None, 1, pl.data_ptr(), None, 128, None) == 1     # cols % 8
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. egv_drop_path_grad
@pytest.mark.parametrize("rows", [45, 41, 9 * 3700])          # 33 300 rows = 532 800 8-column pieces: the grid-stride loop goes round
@pytest.mark.parametrize("pad", [0, 8])                      # ldg = cols + pad
@pytest.mark.parametrize("passes", [1, 3, 4])
def test_drop_path_grad_planes_are_the_formatters_planes(rows, pad, passes):
    from egovlp_amd import ops
    cols, p, seed = 128, 0.5, 0x0BADC0DE5EED0002
    B = (rows + RPS - 1) // RPS
    g = torch.Generator().manual_seed(rows + pad)
    big = (torch.randn(rows, cols + pad, generator=g) * 0.1).cuda()
    gv = big[:, :cols]
    assert gv.stride(0) == cols + pad
    s = ops.drop_path_scales(B, p, seed)
    assert 0 < int((s == 0).sum()) < B
    scaled = (gv * s.repeat_interleave(RPS)[:rows, None]).contiguous()        # one fp32 rounding per element
    got = ops.drop_path_grad(gv, RPS, p, seed, passes)
    want = ops.f16_cast(scaled) if passes == 4 else ops.split_f32(scaled, passes)[0]
    torch.cuda.synchronize()
    assert got.fmt == want.fmt and got.rows == rows and got.cols == cols and (got.lo is None) == (want.lo is None)
    assert torch.equal(bits(got.hi), bits(want.hi))
    if passes == 3:
        assert torch.equal(bits(got.lo), bits(want.lo))


# ------------------------------------------------------------------------------------------------ 4. one block
P_BLOCK = 0.5
# (forward, backward) -> geometry (B, T, n, D, H, Hd), (seed_space, seed_mlp) chosen with drop_path_ref.find_seeds so that the cases
# asserted below occur, forward bar, gradient bar.  'f16': the smallest block at which f16x2_block_ok(M, D, Hd, True) holds -- one
# 256-wide tile of D = 256, fc1 on the big-tile kernel from ceil(M / 256) * 4 >= 128 tiles, i.e. M > 7936: 54 x (1 + 3 x 49) = 7992
BLOCK_CASES = {
    "bf16x3": (("bf16x3", "bf16x3"), (8, 2, 4, 128, 2, 256), (0x51ED270B0001, 0x56811977D8C46918), PARITY, 3 * PARITY),
    "bf16": (("bf16x3", "bf16"), (8, 2, 4, 128, 2, 256), (0x51ED270B0001, 0x56811977D8C46918), PARITY, MIXED_GRAD),
    "f16": (("f16x2", "f16"), (54, 3, 49, 256, 4, 1024), (0x2545F4914F6C0001, 0x9A93BF8824B96918), X2_BAR, F16_GRAD),
}


def _make_block(D, H, Hd, p):
    from functools import partial
    from torch import nn
    from egovlp_amd.model.video_transformer import SpaceTimeBlock
    torch.manual_seed(0)
    blk = SpaceTimeBlock(dim=D, num_heads=H, mlp_ratio=Hd / D, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                         time_init='rand', drop_path=p)
    with torch.no_grad():
        for prm in blk.parameters():                            # affine / biases away from their 1 / 0 initial values
            if prm.dim() == 1:
                prm.add_(0.1 * torch.randn_like(prm))
    return blk


def _run_block(blk, ec, x, g, geom, seeds):
    B, T, n = geom[:3]
    for prm in blk.parameters():
        prm.grad = None
    xin = x.clone().requires_grad_(True)
    ec.begin_step()
    y = blk(xin, B, T, n, ec, seeds)
    y.backward(g)
    ec.join_side_stream()
    torch.cuda.synchronize()
    grads = {"d_x": xin.grad.detach().clone(), **{k: prm.grad.detach().clone() for k, prm in blk.named_parameters()}}
    return y.detach().clone(), grads, y.grad_fn


def _ref_block(blk, x, g, geom, s1, s2):
    from oracle import egovlp_oracle as O
    B, T, n, D, H, Hd = geom
    cfg = O.VideoCfg(embed_dim=D, num_heads=H, ln_eps=1e-6)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = R.block(x64, sd, "", cfg, n, T, None if s1 is None else s1.double(), None if s2 is None else s2.double())
    (y * g.detach().cpu().double()).sum().backward()
    return y.detach(), {"d_x": x64.grad, **{k: v.grad for k, v in sd.items()}}


@pytest.mark.parametrize("mode", ["bf16x3", "bf16", "f16"])
def test_block_with_dropped_paths_matches_the_fp64_reference(mode):
    from egovlp_amd import ops
    from egovlp_amd.model import video_transformer as vt
    prec, geom, (seed_s, seed_m), fbar, gbar = BLOCK_CASES[mode]
    B, T, n, D, H, Hd = geom
    S = 1 + T * n
    p = P_BLOCK
    if mode == "f16":
        assert vt.f16x2_block_ok(B * S, D, Hd, True) and not vt.f16x2_block_ok(7936, D, Hd, True)
    torch.set_num_threads(16)
    blk = _make_block(D, H, Hd, p).cuda().train()
    assert len([1 for _ in blk.parameters()]) == 18
    ec = ops.new_context()
    ec.set_precision(*prec)
    ec.set(block_calls=False, wgrad_side_stream=False)          # both measurements on the per-kernel path: the same kernels but for the drop
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, S, D, generator=gen).cuda()
    g = (torch.randn(B, S, D, generator=gen) * 0.1).cuda()      # O(0.1): "already scaled" for the fp16 backward

    # the draws, read back from the device; the cases this test needs (conditions, not tolerances)
    s1, s2 = dev_scales(B, p, seed_s), dev_scales(B, p, seed_m)
    assert np.array_equal(s1.numpy(), R.drop_path_scales(B, p, seed_s)) and np.array_equal(s2.numpy(), R.drop_path_scales(B, p, seed_m))
    for s in (s1, s2):
        assert 0 < int((s == 0).sum()) < B                      # every branch has a kept and a dropped sample
        assert set(s.tolist()) == {0.0, 2.0}
    both = ((s1 == 0) & (s2 == 0)).nonzero().flatten().tolist()
    assert both                                                 # a sample dropped on both branches

    y, grads, fn = _run_block(blk, ec, x, g, geom, (seed_s, seed_m, None))
    assert isinstance(fn, vt._SpaceTimeBlockFn._backward_cls)
    assert len(grads) == 19
    for b in both:                                              # that sample passes through, and so does its gradient: exactly
        assert torch.equal(y[b], x[b]) and torch.equal(grads["d_x"][b], g[b])
    y_ref, g_ref = _ref_block(blk, x, g, geom, s1, s2)
    e_out = rel(y, y_ref)
    e_g = {k: rel(grads[k], g_ref[k]) for k in grads}

    # the same seeds again: bit-equal output (the forward is a pure function of its inputs) and the same draws in the backward
    y2, grads2, _ = _run_block(blk, ec, x, g, geom, (seed_s, seed_m, None))
    assert torch.equal(y, y2) and torch.equal(grads["mlp.fc2.weight"], grads2["mlp.fc2.weight"])
    # a device seed word is XOR-ed into both seeds: zero changes nothing, another word draws other paths
    w0 = torch.zeros(1, dtype=torch.int64, device="cuda")
    y3, _, _ = _run_block(blk, ec, x, g, geom, (seed_s, seed_m, w0))
    assert torch.equal(y, y3)
    y4, _, _ = _run_block(blk, ec, x, g, geom, (seed_s, seed_m, torch.full((1,), 0x1357_9BDF_0246_8ACE, dtype=torch.int64, device="cuda")))
    assert not torch.equal(y, y4)

    # rate 0 in the same run: the same block, nothing dropped, against the un-scaled bars
    blk.drop_path = 0.0
    y0, grads0, fn0 = _run_block(blk, ec, x, g, geom, None)
    assert isinstance(fn0, vt._SpaceTimeBlockFn._backward_cls)
    y0_ref, g0_ref = _ref_block(blk, x, g, geom, None, None)
    e0_out = rel(y0, y0_ref)
    e0_g = {k: rel(grads0[k], g0_ref[k]) for k in grads0}
    blk.eval()
    blk.drop_path = p                                           # eval(): the identity, whatever the rate
    with torch.no_grad():
        assert torch.equal(blk(x, B, T, n, ec, (seed_s, seed_m, None)), blk(x, B, T, n, ec))

    wk, w0k = max(e_g, key=e_g.get), max(e0_g, key=e0_g.get)
    print("block %s/%s M = %d, p = %.1f: out %.2e (rate 0: %.2e; bar %.1e / %.1e)  worst grad %s %.2e (rate 0: %s %.2e; bar %.1e / %.1e)" % (
        prec[0], prec[1], B * S, p, e_out, e0_out, fbar / (1 - p), fbar, wk, e_g[wk], w0k, e0_g[w0k], gbar / (1 - p), gbar))
    for k in e_g:
        print("   grad %-22s %.2e   (rate 0: %.2e)" % (k, e_g[k], e0_g[k]))
    assert e0_out < fbar and all(v < gbar for v in e0_g.values()), (e0_out, e0_g)
    assert e_out < fbar / (1 - p), e_out
    assert all(v < gbar / (1 - p) for v in e_g.values()), e_g


# ------------------------------------------------------------------------------------------------ 5. the tower
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
RATE = 0.3


def _tiny(rate):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2)}
    if rate:
        vp["drop_path_rate"] = rate
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    m.text_model.set_dropout(0.0, 0.0)
    return m


@pytest.fixture(scope="module")
def towers():
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    Precision.set("bf16x3")
    m, m0 = _tiny(RATE), _tiny(0.0)
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=7)
    m.load_state_dict(sd, strict=True)
    m0.load_state_dict(sd, strict=True)
    yield m.cuda(), m0.cuda(), sd
    Precision.set("bf16x3")


def test_tower_block0_and_eval_equal_the_rate_zero_model(towers):
    from egovlp_amd.model import video_transformer as vt
    from egovlp_amd.synth import synth_batch
    m, m0, _ = towers
    video = synth_batch(8, T=2, L=16, seed=21, res=32)["video"].cuda()
    m.eval()
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m.video_model(video), m0.video_model(video))
    m.train()
    m0.train()
    taps = {}
    hooks = [mod.video_model.blocks[i].register_forward_hook(lambda _m, _a, out, key=(tag, i): taps.__setitem__(key, out))
             for tag, mod in (("r", m), ("0", m0)) for i in range(3)]
    try:
        c0 = m.video_model._drop_calls
        e, e0 = m.video_model(video), m0.video_model(video)
        torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    assert m.video_model._drop_calls == c0 + 1 and m0.video_model._drop_calls == 0
    assert torch.equal(taps[("r", 0)], taps[("0", 0)])                       # block 0 has p = 0
    assert not torch.equal(taps[("r", 2)], taps[("0", 2)]) and not torch.equal(e, e0)
    for i in (1, 2):                                                        # the blocks with p > 0 ran the per-kernel path
        assert isinstance(taps[("r", i)].grad_fn, vt._SpaceTimeBlockFn._backward_cls)
    # the next call counter draws other scales
    vm = m.video_model
    before = [dev_scales(64, vm.dpr[2], sd_) for sd_ in vm.drop_path_seeds(2)[:2]]
    vm(video)
    after = [dev_scales(64, vm.dpr[2], sd_) for sd_ in vm.drop_path_seeds(2)[:2]]
    assert vm._drop_calls == c0 + 2 and all(not torch.equal(a, b) for a, b in zip(before, after))


def test_tower_matches_the_fp64_reference(towers):
    """Embedding and every gradient of the video tower at drop_path_rate = 0.3 (dpr = 0, 0.15, 0.3) in 'bf16x3', against the fp64
    helper fed with the scales the device drew; bars: 1e-3 / 3e-3 (tests/test_gpu_model.py, 'bf16x3') times 1 / (1 - 0.3)."""
    from egovlp_amd.synth import synth_batch
    from oracle import egovlp_oracle as O
    m, _, sd = towers
    B, T = 8, 2
    video = synth_batch(B, T=T, L=16, seed=22, res=32)["video"]
    gen = torch.Generator().manual_seed(3)
    gout = torch.randn(B, 128, generator=gen)
    m.train()
    vm = m.video_model
    for prm in vm.parameters():
        prm.grad = None
    m.exec_ctx.begin_step()
    emb = vm(video.cuda())
    emb.backward(gout.cuda())
    m.exec_ctx.join_side_stream()
    torch.cuda.synchronize()
    scales = [None] + [tuple(dev_scales(B, vm.dpr[i], s_).double() for s_ in vm.drop_path_seeds(i)[:2]) for i in (1, 2)]
    drawn = torch.stack([s_ for pair in scales[1:] for s_ in pair])
    print("tower: dropped (sample, branch) pairs: %d of %d" % (int((drawn == 0).sum()), drawn.numel()))
    assert bool((drawn == 0).any()) and bool((drawn != 0).any())              # this call dropped some paths and kept some
    cfg = O.VideoCfg(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_frames=4)
    sdo = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith("video_model.")}
    ref = R.tower(video.double(), sdo, cfg, scales)
    (ref * gout.double()).sum().backward()
    k = 1.0 / (1.0 - RATE)
    e = rel(emb, ref)
    errs = {name: rel(prm.grad, sdo["video_model." + name].grad) for name, prm in vm.named_parameters()}
    worst = max(errs, key=errs.get)
    print("tower rate %.1f: embedding %.2e (bar %.1e), worst gradient %s %.2e (bar %.1e)" % (RATE, e, PARITY * k, worst, errs[worst], 3 * PARITY * k))
    assert e < PARITY * k
    assert all(v < 3 * PARITY * k for v in errs.values()), {n_: v for n_, v in errs.items() if v >= 3 * PARITY * k}


# ------------------------------------------------------------------------------------------------ 6. the embedding-cache step
def test_cached_step_replays_its_own_drop_path_draws(towers):
    """B = 8 in chunks of 4 at rate 0.3: pass 3 re-computes, bit for bit, the embeddings pass 1 cached (the video tower's call counter
    is put back per chunk); a second step draws other paths."""
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    m, _, sd = towers
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    torch.manual_seed(0)
    b = synth_batch(8, T=2, L=16, seed=23, res=32)
    dev = {"video": b["video"].cuda(), "text": {k: v.cuda() for k, v in b["text"].items()}, "noun_vec": b["noun_vec"].cuda(),
           "verb_vec": b["verb_vec"].cuda()}
    opt = AdamW(m.parameters(), lr=0.0)
    vm = m.video_model
    c0 = vm._drop_calls
    caches, diffs = [], []
    for _ in range(2):
        egoclip_step_cached(m, EgoNCE(), opt, dev, 4, check_replay=True)
        torch.cuda.synchronize()
        diffs.append(float(m.last_replay_max_abs_diff))
        caches.append(tuple(t.clone() for t in m.last_cached_embeddings))
    print("cached step at rate %.1f: max |pass-3 - cached| %.3e, %.3e" % (RATE, diffs[0], diffs[1]))
    assert diffs == [0.0, 0.0]
    assert vm._drop_calls == c0 + 4                                          # once per chunk and step, not twice
    assert torch.equal(caches[0][0], caches[1][0])                           # the text tower draws nothing here
    assert not torch.equal(caches[0][1], caches[1][1])                       # the video tower drew other paths in the second step
