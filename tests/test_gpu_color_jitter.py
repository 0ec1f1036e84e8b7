"""Colour jitter in the fused train transform on a real MI355X (`pytest -m gpu`): egv_patch_gather_u8_aug_color and its `_sel` twin
against the fp64 restatement of torchvision's ops (tests/color_jitter_ref.py), against the host pipeline with a real resize, bit for
bit against each other, against the plain train gather with an all-zero code, through the model and the cached step, and the C-level
refusals.

Bars.  (a) 2e-5 + 4 e32: 2e-5 is the rounding step of the two bf16 planes at |value| <= 2.7 (tests/test_gpu_ops.py), e32 the largest
fp32-against-fp64 difference of the restatement on the test's own inputs, computed in the test; the factor 4 was set before any device
run to cover FMA contraction.  (b) 2e-3: an indexing test (an error there is of order 1), above the 3e-4 interpolation tail of the
plain transform's test times the jitter's gain.  (e) the project's 1e-3.

Measured on MI355X.  (a) device max |error| against fp64 1.68e-5 at P = 16, R = 32 and 1.58e-5 at P = 14, R = 28, every clip within
1.5 - 1.7e-5; e32 4.7e-6 (1.3 % of elements above 2e-6); bar 3.9e-5.  The kernel's jitter arithmetic is compiled without contraction,
so its error is e32 plus the plane step.  (b) max 1.5e-5, no element above 2e-5.  (d) 7.6e-6 at P = 16, 1.5e-5 at P = 14.  (e) embeddings
rel-L2 4.1e-6 (0.58 without the jitter); cached step, chunk 2 against chunk 4: the same loss in every digit.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import color_jitter_ref as CJ

pytestmark = pytest.mark.gpu

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
ARCH = dict(img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2)        # the tiny tower of tests/test_gpu_patch_drop.py
ORDERS = [(1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int16)


def code_of(order):
    return float(sum(d << (2 * k) for k, d in enumerate(order)))


def norm_consts(dtype):
    from egovlp_amd import ops
    return (torch.tensor(ops.IMAGENET_MEAN, dtype=dtype).view(1, 3, 1, 1), torch.tensor(ops.IMAGENET_STD, dtype=dtype).view(1, 3, 1, 1))


def host_transform(u8, boxes, color, R, dtype=torch.float32):
    """The train transform on the host, per clip: crop, x / 255, bilinear resize, flip, the restated jitter (color None: none),
    Normalize.  -> [B, T, 3, R, R]"""
    mean, std = norm_consts(dtype)
    out = []
    for b in range(u8.shape[0]):
        i, j, h, w, flip = [int(v) for v in boxes[b]]
        clip = u8[b, :, :, i:i + h, j:j + w].to(dtype) / 255
        if (h, w) != (R, R):
            clip = F.interpolate(clip, size=(R, R), mode="bilinear", align_corners=False)
        if flip:
            clip = clip.flip(-1)
        if color is not None:
            clip = CJ.apply(clip, color[b])
        out.append((clip - mean) / std)
    return torch.stack(out).contiguous()         # the restated hue op leaves permuted strides; ops.patch_gather takes the memory as it is


def im2col(img, P):
    """[B, T, C, R, R] -> the rows of the patch planes: [(bt * gh + py) * gw + px, (c * P + iy) * P + ix]"""
    B, T, Cc, R, _ = img.shape
    g = R // P
    return img.reshape(B * T, Cc, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * T * g * g, Cc * P * P)


def _planted_clips(B, T, Hs, Ws, seed):
    """Random bytes with, in every frame, a block of grey / black / white / primary / secondary pixels, and frame (1, 0) quantised to
    four levels (many channel ties: the hue op's max == r / max == g selects)."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, T, 3, Hs, Ws), generator=g, dtype=torch.uint8)
    u8[1, 0] = (u8[1, 0] // 64) * 85
    special = torch.tensor([[128, 128, 128], [0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0],
                            [0, 255, 255], [255, 0, 255], [77, 77, 77], [1, 1, 1], [254, 254, 254], [200, 200, 10], [10, 200, 200]],
                           dtype=torch.uint8)
    for k in range(special.shape[0]):
        u8[:, :, :, 14 + k // 7, 20 + k % 7] = special[k]                 # inside every box used below
    return u8


@pytest.mark.parametrize("P,R", [(16, 32), (14, 28)])
def test_a_precision_against_the_fp64_restatement(P, R):
    from egovlp_amd import ops
    B, T, Hs, Ws = 6, 2, 40, 48
    u8 = _planted_clips(B, T, Hs, Ws, seed=21)
    # h = w = R: the source coordinate (o + 0.5) * 1 - 0.5 is an exact integer, the pre-jitter pixel exactly u8 / 255
    boxes = torch.tensor([[0, 0, R, R, 0], [8, 16, R, R, 1], [3, 5, R, R, 0], [Hs - R, Ws - R, R, R, 0], [1, 2, R, R, 0], [5, 11, R, R, 0]],
                         dtype=torch.int32)
    factors = [(0.6, 0.6, 0.1), (1.4, 1.4, -0.1), (0.6, 0.0, 0.5), (1.4, 2.0, -0.5), (1.4, 0.0, -0.1), (0.6, 2.0, 0.5)]
    color = torch.tensor([list(f) + [code_of(o)] for f, o in zip(factors, ORDERS)], dtype=torch.float32)
    assert [CJ.ops_of(c) for c in color[:, 3].tolist()] == [list(o) for o in ORDERS]
    want64 = im2col(host_transform(u8, boxes, color, R, torch.float64), P)
    want32 = im2col(host_transform(u8, boxes, color, R, torch.float32), P)
    diff32 = (want32.double() - want64).abs()
    e32 = float(diff32.max())
    bar = 2e-5 + 4 * e32
    pl = ops.patch_gather(u8.cuda(), P, 3, aug=(boxes.cuda(), R), color=color.cuda())
    torch.cuda.synchronize()
    K = 3 * P * P
    got = (pl.hi[:, :K].double() + pl.lo[:, :K].double()).cpu()
    assert got.shape == want64.shape and bool(torch.isfinite(got).all())
    err = (got - want64).abs()
    per_clip = err.view(B, -1).max(1).values.tolist()
    print("colour gather P=%d R=%d: device max |err| vs fp64 %.3e (per clip %s), e32 %.3e (%.2f %% of elements above 2e-6), bar %.3e" % (
        P, R, float(err.max()), " ".join("%.1e" % v for v in per_clip), e32, 100.0 * float((diff32 > 2e-6).double().mean()), bar))
    assert float(err.max()) < bar
    if pl.cols > K:
        assert float(pl.hi[:, K:].float().abs().max()) == 0.0 and float(pl.lo[:, K:].float().abs().max()) == 0.0
    # one plane: bf16 rounding of the same values
    pl1 = ops.patch_gather(u8.cuda(), P, 1, aug=(boxes.cuda(), R), color=color.cuda())
    assert pl1.lo is None and float((pl1.hi[:, :K].double().cpu() - want64).abs().max()) < 2e-2


def test_b_real_resize_against_the_host_pipeline():
    from egovlp_amd import ops
    from egovlp_amd.data_loader.transforms import train_transform_params_color
    B, T, Hs, Ws, R, P = 3, 2, 64, 80, 32, 16
    g = torch.Generator().manual_seed(22)
    u8 = torch.randint(0, 256, (B, T, 3, Hs, Ws), generator=g, dtype=torch.uint8)
    boxes, color = train_transform_params_color(B, Hs, Ws, (0.5, 1.0), (0.4, 0.4, 0.1), generator=g)
    boxes[1, 4] = 1
    boxes[0, 4] = 0
    assert len({tuple(r) for r in color.tolist()}) == B and all(len(CJ.ops_of(c)) == 3 for c in color[:, 3].tolist())
    want = ops.patch_gather(host_transform(u8, boxes, color, R).cuda(), P, 3).float().cpu()
    got = ops.patch_gather(u8.cuda(), P, 3, aug=(boxes.cuda(), R), color=color.cuda()).float().cpu()
    err = (got - want).abs()
    print("colour gather with a real resize: max |err| %.3e, %d of %d elements above 2e-5" % (float(err.max()), int((err > 2e-5).sum()), err.numel()))
    assert got.shape == want.shape and float(err.max()) < 2e-3
    # the jitter is there at all: the plain train gather differs by far more
    plain = ops.patch_gather(u8.cuda(), P, 3, aug=(boxes.cuda(), R)).float().cpu()
    assert float((plain - want).abs().max()) > 0.1


@pytest.mark.parametrize("P,R", [(16, 32), (14, 28)])
def test_c_gather_over_kept_patches_is_the_full_colour_gathers_rows(P, R):
    from egovlp_amd import ops
    B, T, Hs, Ws, n, K = 6, 2, 40, 48, 4, 2
    u8 = _planted_clips(B, T, Hs, Ws, seed=23).cuda()
    boxes = torch.tensor([[0, 0, Hs, Ws, 0], [3, 5, 30, 37, 1], [8, 16, R, R, 1], [2, 1, 37, 29, 0], [0, 7, 33, 41, 1], [5, 11, 35, 35, 0]],
                         dtype=torch.int32).cuda()
    factors = [(0.6, 0.6, 0.1), (1.4, 1.4, -0.1), (0.6, 0.0, 0.5), (1.4, 2.0, -0.5), (1.4, 0.0, -0.1), (0.6, 2.0, 0.5)]
    color = torch.tensor([list(f) + [code_of(o)] for f, o in zip(factors, ORDERS)], dtype=torch.float32).cuda()
    keep = torch.tensor([[0, 3], [1, 2], [0, 1], [2, 3], [1, 3], [0, 2]], dtype=torch.int32).cuda()
    bt = torch.arange(B * T, device="cuda")
    rows = (bt[:, None] * n + keep.long()[bt // T]).reshape(-1)
    for passes in (1, 3):
        full = ops.patch_gather(u8, P, passes, aug=(boxes, R), color=color)
        sel = ops.patch_gather(u8, P, passes, aug=(boxes, R), color=color, keep=keep)
        torch.cuda.synchronize()
        assert full.rows == B * T * n and sel.rows == B * T * K and sel.cols == full.cols and sel.ld == full.ld
        assert torch.equal(bits(sel.hi), bits(full.hi.index_select(0, rows)))
        assert (sel.lo is None) == (passes == 1)
        if passes == 3:
            assert torch.equal(bits(sel.lo), bits(full.lo.index_select(0, rows)))


@pytest.mark.parametrize("P,R", [(16, 32), (14, 28)])
def test_d_a_table_of_zero_codes_is_the_plain_train_gather(P, R):
    """One plane step, not bit equality: the bilinear sum is contraction-sensitive (csrc/video_input.hip) and the two kernels pack
    their pixels differently."""
    from egovlp_amd import ops
    B, T, Hs, Ws = 3, 2, 40, 48
    u8 = _planted_clips(B, T, Hs, Ws, seed=24).cuda()
    boxes = torch.tensor([[0, 0, Hs, Ws, 0], [3, 5, 30, 37, 1], [8, 16, R, R, 1]], dtype=torch.int32).cuda()
    color = torch.tensor([[0.5, 0.5, 0.3, 0.0], [1.0, 1.0, 0.0, 0.0], [2.0, 0.0, -0.5, 0.0]], dtype=torch.float32).cuda()
    a = ops.patch_gather(u8, P, 3, aug=(boxes, R), color=color).float()
    b = ops.patch_gather(u8, P, 3, aug=(boxes, R)).float()
    e = float((a - b).abs().max())
    print("all codes 0 against egv_patch_gather_u8_aug, P=%d: max |diff| %.3e" % (P, e))
    assert e <= 2e-5


def _tiny(**keys):
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.synth import synth_state_dict
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(ARCH)}
    vp.update(keys)
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=7), strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    m.cuda()
    m.exec_ctx.set_precision("bf16x3", "bf16x3")
    return m


def _model_inputs(B, seed):
    from egovlp_amd.data_loader.transforms import train_transform_params_color
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, 2, 3, 80, 100), generator=g, dtype=torch.uint8)
    # smooth frames under the noise, so that the embedding is not that of white noise alone
    ramp = torch.linspace(0, 1, 100).view(1, 1, 1, 1, 100) * torch.tensor([200.0, 120.0, 60.0]).view(1, 1, 3, 1, 1)
    u8 = (u8.float() * 0.25 + ramp).clamp(0, 255).to(torch.uint8)
    boxes, color = train_transform_params_color(B, 80, 100, (0.5, 1.0), (0.4, 0.4, 0.1), generator=g)
    return u8, boxes, color


def test_e_model_level_embeddings_patch_dropout_and_the_cached_step():
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    B = 4
    u8, boxes, color = _model_inputs(B, 25)
    host = host_transform(u8, boxes, color, 64)
    m = _tiny()
    vm = m.video_model
    m.eval()
    with torch.no_grad():
        vm.set_input_augmentation(boxes, 64, color)                         # host tables: validated, then moved
        e_dev = vm(u8.cuda())
        e_host = vm(host.cuda())
        vm.set_input_augmentation(boxes, 64)
        e_plain = vm(u8.cuda())
    r = rel(e_dev, e_host)
    print("model: fused transform with jitter against the host-transformed frames: embedding rel %.2e; without the jitter %.2e" % (
        r, rel(e_plain, e_host)))
    assert r < 1e-3 and rel(e_plain, e_host) > 1e-3                        # the bar tells a forward without the jitter apart
    # train mode with patch dropout: the _sel twin runs, the backward gives finite gradients
    md = _tiny(patch_drop_rate=0.5)
    md.train()
    vd = md.video_model
    vd.set_input_augmentation(boxes.cuda(), 64, color.cuda())               # device tables
    out = vd(u8.cuda())
    out.sum().backward()
    md.exec_ctx.join_side_stream()
    torch.cuda.synchronize()
    assert tuple(vd.last_patch_keep.shape) == (B, 8) and bool(torch.isfinite(out).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in vd.parameters())
    assert float(vd.patch_embed.proj.weight.grad.abs().max()) > 0.0
    # the cached step: chunks of 2 give the loss of one chunk of 4
    m.train()
    sb = synth_batch(B, T=2, L=16, seed=26, res=64)
    data = {"video": u8.cuda(), "text": {k: v.cuda() for k, v in sb["text"].items()}, "noun_vec": sb["noun_vec"].cuda(),
            "verb_vec": sb["verb_vec"].cuda()}
    opt = AdamW(m.parameters(), lr=0.0)
    losses = []
    for chunk in (2, 4):
        for p in m.parameters():
            p.grad = None
        losses.append(float(egoclip_step_cached(m, EgoNCE(), opt, data, chunk, aug_boxes=boxes.cuda(), aug_color=color.cuda())))
    plain = float(egoclip_step_cached(m, EgoNCE(), opt, data, 4, aug_boxes=boxes.cuda()))
    torch.cuda.synchronize()
    print("cached step with aug_color: loss chunk 2 %.7f chunk 4 %.7f (rel %.2e); without the jitter %.7f" % (
        losses[0], losses[1], abs(losses[0] - losses[1]) / abs(losses[1]), plain))
    assert abs(losses[0] - losses[1]) < 1e-3 * abs(losses[1])               # PARITY of tests/test_gpu_cached_step.py
    assert plain != losses[1]


def test_f_bad_arguments_launch_nothing():
    from egovlp_amd import _lib
    h = _lib.lib()
    BT, T, H, P, n, K = 2, 2, 32, 16, 4, 2
    lda = 3 * P * P
    u8 = torch.zeros(BT, 4, 40, 40, dtype=torch.uint8, device="cuda")
    hi, lo = (torch.full((BT * n, lda + 256), -7, dtype=torch.int16, device="cuda") for _ in range(2))
    keep = torch.tensor([[0, 3]], dtype=torch.int32, device="cuda")
    boxes = torch.tensor([[0, 0, 40, 40, 0]], dtype=torch.int32, device="cuda")
    color = torch.tensor([[1.2, 0.8, 0.1, code_of((1, 2, 3))]], dtype=torch.float32, device="cuda")
    mean, std = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5), (C.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    p = lambda t: t.data_ptr()
    full = dict(video=p(u8), BT=BT, T=T, C=3, Hs=40, Ws=40, R=H, P=P, boxes=p(boxes), color=p(color), mean=mean, std=std,
                a_hi=p(hi), a_lo=p(lo), lda=lda + 256, stream=None)
    sel = dict(full)
    del sel["a_hi"], sel["a_lo"], sel["lda"], sel["stream"]
    sel.update(keep=p(keep), K=K, a_hi=p(hi), a_lo=p(lo), lda=lda + 256, stream=None)
    shared = [dict(color=None), dict(C=4), dict(C=1), dict(boxes=None), dict(video=None), dict(a_hi=None), dict(R=30), dict(P=15), dict(BT=3),
              dict(lda=lda - 4), dict(std=(C.c_float * 4)(0.25, 0.0, 0.25, 0.25)), dict(BT=1 << 30, R=4096)]
    for case in shared:
        assert h.egv_patch_gather_u8_aug_color(*{**full, **case}.values()) == 1, case
    for case in shared[:-1] + [dict(keep=None), dict(K=0), dict(K=n + 1), dict(BT=1 << 30, R=4096, K=65536)]:
        assert h.egv_patch_gather_u8_aug_color_sel(*{**sel, **case}.values()) == 1, case
    torch.cuda.synchronize()
    assert bool((hi == -7).all()) and bool((lo == -7).all())
