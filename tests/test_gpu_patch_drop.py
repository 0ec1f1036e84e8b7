"""Patch dropout in the video tower on a real MI355X (`pytest -m gpu`): the draw against its numpy mirror (tests/patch_drop_ref.py), the
three *_sel gathers and the *_sel token assembly bit for bit against the rows of the full kernels, the assembly's backward against fp64
autograd, a depth-3 tower (alone and with stochastic depth) against the fp64 reference fed with the table the device drew, the
workload's kernels at the sizes rate 0.5 gives them (99 keys, M = 786), and identity / replay: eval() and rate 0 are the model without
the key, the embedding-cache step replays its tables.

Bars: those the full-sequence model is held to in tests/test_gpu_model.py -- 1e-3 on embeddings and 3e-3 on gradients in 'bf16x3' (times
1 / (1 - p) with stochastic depth at rate p, as tests/test_gpu_drop_path.py), _fbar / F16_GRAD for 'f16mix' / 'f16' -- with no extra
factor: nothing is rescaled by patch dropout, the tower simply runs a shorter sequence.

Measured on MI355X (rel-L2): tower (depth 3, B = 6, T = 2, K = 8 of 16, 'bf16x3') against fp64: embedding 1.0e-5, worst gradient
blocks.0.timeattn.qkv.weight 1.6e-5; with drop_path 0.3 on top: 1.1e-5 / 1.7e-5.  Assembly backward against fp64 autograd: d_pe 0,
d_cls 3.0e-8, d_pos 3.9e-8, d_temporal 4.8e-8.  ViT-B width at K = 98 (M = 786), 'f16mix' / 'f16' against 'bf16x3' / 'bf16x3': embedding
0 (786 rows are too few for the fp16 big-tile format, f16x2_block_ok: the forward of both runs is split-bf16), worst gradient
patch_embed.proj.weight 2.3e-3.  Draw, gathers and assembly forward: bit-equal.  Cached step: max |pass 3 - cache| = 0.  Identity table
(K = n) against the full kernels: gathers and assembly forward bit-equal, assembly backward d_pe 0, d_cls 0, d_pos 6.3e-8, d_temporal 5.6e-8.
"""
import numpy as np
import pytest
import torch

import drop_path_ref as DR
import patch_drop_ref as R

pytestmark = pytest.mark.gpu

SEEDS = (0x0123456789ABCDEF, 0xF00DFACE12345678)
WORD = 0x5DEECE66D1234567
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the draw
@pytest.mark.parametrize("B,n,K", [(3, 4, 1), (2, 37, 18), (5, 196, 98), (2, 257, 64), (1, 1024, 256), (2, 16, 16)])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("word", [None, WORD])
def test_draw_equals_the_numpy_mirror(B, n, K, seed, word):
    from egovlp_amd import ops
    sdev = None if word is None else torch.tensor([word], dtype=torch.int64, device="cuda")
    got = ops.patch_keep_draw(B, n, K, seed, sdev)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (B, K)
    want = R.patch_keep(B, n, K, seed, 0 if word is None else word)
    assert np.array_equal(got.cpu().numpy(), want)
    if K == n:
        assert torch.equal(got.cpu(), torch.arange(n, dtype=torch.int32).expand(B, n))
    if word is not None and K < n and n >= 37:                # the device word is part of the seed
        assert not torch.equal(got, ops.patch_keep_draw(B, n, K, seed))


def test_draw_with_bad_arguments_launches_nothing():
    from egovlp_amd import _lib
    h = _lib.lib()
    buf = torch.full((4, 1025), -7, dtype=torch.int32, device="cuda")
    P = buf.data_ptr()
    assert h.egv_patch_keep_draw(4, 16, 0, 1, None, P, None) == 1            # K = 0
    assert h.egv_patch_keep_draw(4, 16, 17, 1, None, P, None) == 1           # K > n
    assert h.egv_patch_keep_draw(4, 1025, 8, 1, None, P, None) == 1          # n > 1024
    assert h.egv_patch_keep_draw(4, 16, 8, 1, None, None, None) == 1         # no table
    assert h.egv_patch_keep_draw(0, 16, 8, 1, None, P, None) == 1
    torch.cuda.synchronize()
    assert bool((buf == -7).all())


# ------------------------------------------------------------------------------------------------ 2. the gathers
def _tables(B, n, K, hand):
    from egovlp_amd import ops
    drawn = [ops.patch_keep_draw(B, n, K, s) for s in SEEDS]
    hand = torch.tensor(hand, dtype=torch.int32, device="cuda")
    assert tuple(hand.shape) == (B, K) and int(hand.min()) == 0 and int(hand.max()) == n - 1
    return drawn + [hand]


def _rows(keep, T, n):
    """rows of the full gather's planes that make the planes of the gather over `keep`: bt * n + keep[bt // T][j]"""
    B, K = keep.shape
    bt = torch.arange(B * T, device=keep.device)
    return (bt[:, None] * n + keep.long()[bt // T]).reshape(-1)


def _check_gather(video, P, n, T, keep, **kw):
    from egovlp_amd import ops
    B, K = keep.shape
    for passes in (1, 3):
        full = ops.patch_gather(video, P, passes, **kw)
        sel = ops.patch_gather(video, P, passes, keep=keep, **kw)
        torch.cuda.synchronize()
        assert full.rows == B * T * n and sel.rows == B * T * K and sel.cols == full.cols and sel.ld == full.ld
        assert (sel.lo is None) == (passes == 1)
        rows = _rows(keep, T, n)
        assert torch.equal(bits(sel.hi), bits(full.hi.index_select(0, rows)))
        if passes == 3:
            assert torch.equal(bits(sel.lo), bits(full.lo.index_select(0, rows)))
    return sel          # the three-pass planes


HAND_12 = [[0, 3, 5, 8, 11], [0, 1, 2, 10, 11]]


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("geom", ["p16", "p14"])
def test_gather_over_kept_patches_is_the_full_gathers_rows(geom, u8):
    # p16: B = 2, T = 3, 64 x 48, P = 16: 4 x 3 patches; p14 (ViT-L/14: 2-pixel groups, 588 columns padded to 640): 2 x 2 clips of 56 x 42
    B, T, H, W, P = (2, 3, 64, 48, 16) if geom == "p16" else (2, 2, 56, 42, 14)
    n, K = 12, 5
    g = torch.Generator().manual_seed(11)
    video = torch.randint(0, 256, (B, T, 3, H, W), generator=g, dtype=torch.uint8) if u8 else torch.randn(B, T, 3, H, W, generator=g)
    video = video.cuda()
    for keep in _tables(B, n, K, HAND_12):
        sel = _check_gather(video, P, n, T, keep)
        if geom == "p14":
            assert sel.cols == 640 and float(sel.hi[:, 588:].float().abs().max()) == 0.0 and float(sel.lo[:, 588:].float().abs().max()) == 0.0


def test_gather_clamps_a_table_entry_outside_the_grid():
    """A device table cannot be checked without a sync: the kernels clamp an entry into [0, n), as egv_patch_gather_u8_eval clamps its
    frame table -- the result is that of the clamped table."""
    from egovlp_amd import ops
    g = torch.Generator().manual_seed(12)
    video = torch.randn(2, 3, 3, 64, 48, generator=g).cuda()
    bad = torch.tensor([[-3, 3, 5, 8, 99], [0, 1, 2, 10, 12]], dtype=torch.int32, device="cuda")
    a, b = ops.patch_gather(video, 16, 3, keep=bad), ops.patch_gather(video, 16, 3, keep=bad.clamp(0, 11))
    assert torch.equal(bits(a.hi), bits(b.hi)) and torch.equal(bits(a.lo), bits(b.lo))


@pytest.mark.parametrize("R_,P", [(64, 16), (56, 14)])
def test_augmented_gather_over_kept_patches_is_the_full_gathers_rows(R_, P):
    # source 80 x 100, one box per clip: whole frame / a crop, flipped / a crop, not flipped
    B, T, Hs, Ws = 3, 2, 80, 100
    n, K = (R_ // P) ** 2, 6
    g = torch.Generator().manual_seed(13)
    u8 = torch.randint(0, 256, (B, T, 3, Hs, Ws), generator=g, dtype=torch.uint8).cuda()
    boxes = torch.tensor([[0, 0, Hs, Ws, 0], [7, 11, 50, 61, 1], [20, 3, 33, 90, 0]], dtype=torch.int32, device="cuda")
    hand = [[0, 2, 5, 9, 12, n - 1], [0, 1, 6, 7, 8, n - 1], [0, 3, 4, 10, 11, n - 1]]
    for keep in _tables(B, n, K, hand):
        _check_gather(u8, P, n, T, keep, aug=(boxes, R_))


# ------------------------------------------------------------------------------------------------ 3. the assembly
def test_assembly_forward_rows_and_backward_against_fp64_autograd():
    from egovlp_amd import ops
    B, T, n, K, D, T_model = 2, 3, 12, 5, 64, 5
    g = torch.Generator().manual_seed(14)
    pe_full = torch.randn(B * T * n, D, generator=g)
    cls, pos, tmp = torch.randn(1, 1, D, generator=g), torch.randn(1, n + 1, D, generator=g), torch.randn(1, T_model, D, generator=g)
    dx = torch.randn(B, 1 + T * K, D, generator=g)
    full = ops.assemble_tokens(pe_full.cuda(), cls.cuda(), pos.cuda(), tmp.cuda(), B, T, n, D)
    for keep in _tables(B, n, K, HAND_12):
        kc = keep.cpu()
        unkept = sorted(set(range(n)) - set(kc.reshape(-1).tolist()))
        assert unkept                                         # the table leaves positions out (a condition of this test, not a tolerance)
        pe = pe_full.index_select(0, _rows(kc, T, n))
        x = ops.assemble_tokens(pe.cuda(), cls.cuda(), pos.cuda(), tmp.cuda(), B, T, n, D, keep=keep)
        torch.cuda.synchronize()
        idx = R.token_index(kc.numpy(), T, n)
        assert tuple(x.shape) == (B, 1 + T * K, D)
        for b in range(B):
            assert torch.equal(x[b].cpu(), full[b].cpu().index_select(0, idx[b]))
        d_pe, d_cls, d_pos, d_tmp = ops.assemble_tokens_bwd(dx.cuda(), B, T, n, D, T_model, keep=keep)
        torch.cuda.synchronize()
        pe_, cls_, pos_, tmp_ = [t.double().requires_grad_(True) for t in (pe, cls, pos, tmp)]
        body = pe_.view(B, T, K, D) + pos_[0, 1 + kc.long()][:, None] + tmp_[0, :T][None, :, None]
        xr = torch.cat([(cls_ + pos_[:, :1]).expand(B, -1, -1), body.reshape(B, T * K, D)], 1)
        assert rel(x, xr) < 1e-6
        xr.backward(dx.double())
        errs = (rel(d_pe, pe_.grad), rel(d_cls, cls_.grad), rel(d_pos, pos_.grad), rel(d_tmp, tmp_.grad))
        print("assembly backward, unkept %s: d_pe %.1e d_cls %.1e d_pos %.1e d_temporal %.1e" % ((unkept,) + errs))
        assert tuple(d_pe.shape) == (B * T * K, D) and tuple(d_pos.shape) == (1, n + 1, D) and tuple(d_tmp.shape) == (1, T_model, D)
        assert all(e < 1e-6 for e in errs), errs
        assert float(d_pos[0, [1 + j for j in unkept]].abs().max()) == 0.0
        assert float(d_pos[0, [1 + j for j in range(n) if j not in unkept]].abs().max(dim=1).values.min()) > 0.0
        assert float(d_tmp[0, T:].abs().max()) == 0.0


def _identity(B, n):
    return torch.arange(n, dtype=torch.int32, device="cuda").expand(B, n).contiguous()


def test_identity_table_is_the_full_kernels():
    """keep[b] = 0 .. n-1 (K = n, the boundary the draw's "exactly K have rank < K" rests on): the *_sel entry points are their full twins.
    Gathers and assembly forward in every bit (both planes, passes 1 and 3); the assembly backward within the 1e-6 of this file -- its two
    position kernels sum in different orders."""
    from egovlp_amd import ops
    g = torch.Generator().manual_seed(15)
    n = 12
    for B, T, H, W, P in ((2, 3, 64, 48, 16), (2, 2, 56, 42, 14)):
        for u8 in (False, True):
            video = torch.randint(0, 256, (B, T, 3, H, W), generator=g, dtype=torch.uint8) if u8 else torch.randn(B, T, 3, H, W, generator=g)
            sel = _check_gather(video.cuda(), P, n, T, _identity(B, n))
            if P == 14:
                assert sel.cols == 640 and float(sel.hi[:, 588:].float().abs().max()) == 0.0 and float(sel.lo[:, 588:].float().abs().max()) == 0.0
    Bq, Tq, Hs, Ws = 3, 2, 80, 100
    src = torch.randint(0, 256, (Bq, Tq, 3, Hs, Ws), generator=g, dtype=torch.uint8).cuda()
    boxes = torch.tensor([[0, 0, Hs, Ws, 0], [7, 11, 50, 61, 1], [20, 3, 33, 90, 0]], dtype=torch.int32, device="cuda")
    for R_, P in ((64, 16), (56, 14)):
        _check_gather(src, P, (R_ // P) ** 2, Tq, _identity(Bq, (R_ // P) ** 2), aug=(boxes, R_))
    B, T, D, T_model = 2, 3, 64, 5
    pe = torch.randn(B * T * n, D, generator=g).cuda()
    cls, pos, tmp = torch.randn(1, 1, D, generator=g).cuda(), torch.randn(1, n + 1, D, generator=g).cuda(), torch.randn(1, T_model, D, generator=g).cuda()
    dx = torch.randn(B, 1 + T * n, D, generator=g).cuda()
    keep = _identity(B, n)
    assert torch.equal(bits(ops.assemble_tokens(pe, cls, pos, tmp, B, T, n, D, keep=keep)), bits(ops.assemble_tokens(pe, cls, pos, tmp, B, T, n, D)))
    full, sel = ops.assemble_tokens_bwd(dx, B, T, n, D, T_model), ops.assemble_tokens_bwd(dx, B, T, n, D, T_model, keep=keep)
    torch.cuda.synchronize()
    errs = [rel(s_, f_) for s_, f_ in zip(sel, full)]
    print("assembly backward, identity table against the full backward: d_pe %.1e d_cls %.1e d_pos %.1e d_temporal %.1e" % tuple(errs))
    assert all(tuple(s_.shape) == tuple(f_.shape) for s_, f_ in zip(sel, full)) and all(e < 1e-6 for e in errs), errs


def test_input_path_with_bad_arguments_launches_nothing():
    """Every refusal of the eleven entry points of csrc/video_input.hip but the draw's (above): a valid argument list per entry point
    (names and order of include/egovlp_hip.h), the named arguments of ONE case replaced, EGV_ERR_ARG expected and no output buffer
    touched.  The valid lists themselves are never sent."""
    import ctypes as C
    from egovlp_amd import _lib
    h = _lib.lib()
    BT, T, Cc, H, P, n, K, D, TM = 2, 2, 3, 32, 16, 4, 2, 8, 2                 # one clip of two 32 x 32 frames, 768 columns
    lda = Cc * P * P
    dev = "cuda"
    f32 = torch.zeros(BT, Cc, H, H, device=dev)
    u8 = torch.zeros(BT, Cc, 40, 40, dtype=torch.uint8, device=dev)             # the direct gathers read its first 32 x 32 x 3 x 2 bytes
    hi, lo = (torch.full((BT * n, lda), -7, dtype=torch.int16, device=dev) for _ in range(2))
    keep = torch.tensor([[0, 3]], dtype=torch.int32, device=dev)
    boxes = torch.tensor([[0, 0, 40, 40, 0]], dtype=torch.int32, device=dev)
    pe, cls, pos, tmp = (torch.zeros(r, D, device=dev) for r in (BT * n, 1, n + 1, TM))
    x, dxs = torch.full((1, 1 + T * n, D), -7.0, device=dev), torch.zeros(1, 1 + T * n, D, device=dev)
    d_pe, d_cls, d_pos, d_tmp = (torch.full((r, D), -7.0, device=dev) for r in (BT * n, 1, n + 1, TM))
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)
    std0, stdn = (C.c_float * 3)(0.25, 0.0, 0.25), (C.c_float * 3)(0.25, 0.25, -1.0)
    p = lambda t: t.data_ptr()
    planes = dict(a_hi=p(hi), a_lo=p(lo), lda=lda, stream=None)
    norm, table = dict(mean=mean, std=std), dict(keep=p(keep), K=K)
    aug = dict(video=p(u8), BT=BT, T=T, C=Cc, Hs=40, Ws=40, R=H, P=P, boxes=p(boxes))
    grads = dict(d_pe=p(d_pe), d_cls=p(d_cls), d_pos=p(d_pos), d_temporal=p(d_tmp), stream=None)
    valid = {
        "egv_patch_gather": dict(video=p(f32), BT=BT, C=Cc, H=H, W=H, P=P, **planes),
        "egv_patch_gather_u8": dict(video=p(u8), BT=BT, C=Cc, H=H, W=H, P=P, **norm, **planes),
        "egv_patch_gather_sel": dict(video=p(f32), BT=BT, T=T, C=Cc, H=H, W=H, P=P, **table, **planes),
        "egv_patch_gather_u8_sel": dict(video=p(u8), BT=BT, T=T, C=Cc, H=H, W=H, P=P, **norm, **table, **planes),
        "egv_patch_gather_u8_aug": dict(**aug, **norm, **planes),
        "egv_patch_gather_u8_aug_sel": dict(**aug, **norm, **table, **planes),
        "egv_patch_gather_u8_eval": dict(frames=p(u8), F=BT, index=None, BT=BT, C=Cc, Hs=40, Ws=40, S=H, R=H, P=P, **norm, **planes),
        "egv_assemble_tokens": dict(pe=p(pe), cls=p(cls), pos=p(pos), temporal=p(tmp), B=1, T=T, n=n, D=D, x=p(x), stream=None),
        "egv_assemble_tokens_sel": dict(pe=p(pe), cls=p(cls), pos=p(pos), temporal=p(tmp), keep=p(keep), B=1, T=T, n=n, K=K, D=D, x=p(x), stream=None),
        "egv_assemble_tokens_bwd": dict(dx=p(dxs), B=1, T=T, n=n, D=D, T_model=TM, **grads),
        "egv_assemble_tokens_bwd_sel": dict(dx=p(dxs), keep=p(keep), B=1, T=T, n=n, K=K, D=D, T_model=TM, **grads),
    }
    null = lambda *names: [{a: None} for a in names]
    zero = lambda *names: [{a: 0} for a in names]
    # GRID: more than 2^31 - 1 blocks.  These cases pass every other check with the small buffers above, so grid_of (csrc/video_input.hip)
    # alone stands between them and a launch far beyond those buffers.
    BIG = 1 << 30
    bad = {
        "egv_patch_gather": null("video", "a_hi") + zero("BT", "C", "H", "W", "P") + [dict(BT=-BT), dict(H=24), dict(P=15), dict(lda=lda - 2),
                            dict(lda=lda + 1), dict(BT=BIG, H=4096, W=4096)],
        "egv_patch_gather_sel": null("video", "a_hi", "keep") + zero("BT", "T", "C", "H", "W", "P", "K") + [dict(K=n + 1), dict(BT=3), dict(H=24),
                                dict(P=15), dict(lda=lda - 4), dict(lda=lda + 2), dict(BT=BIG, H=4096, W=4096, K=65536)],
        "egv_patch_gather_u8_aug": null("video", "boxes", "mean", "std", "a_hi") + zero("BT", "T", "C", "Hs", "Ws", "R", "P") + [
            dict(std=std0), dict(std=stdn), dict(C=5), dict(BT=3), dict(R=24), dict(R=30, P=6), dict(P=15), dict(lda=lda - 4), dict(lda=lda + 1),
            dict(BT=BIG, R=4096)],
        "egv_patch_gather_u8_eval": null("frames", "a_hi", "mean", "std") + zero("F", "BT", "C", "Hs", "Ws", "S", "R", "P") + [
            dict(std=std0), dict(std=stdn), dict(C=5), dict(BT=BT + 1), dict(R=24), dict(R=30, P=6), dict(P=15), dict(lda=lda - 2),
            dict(lda=lda + 1), dict(S=1 << 20), dict(index=p(keep), BT=BIG, R=4096)],
        "egv_assemble_tokens": null("pe", "cls", "pos", "temporal", "x") + zero("B", "T", "n", "D") + [dict(D=6), dict(B=BIG, T=64, n=1024, D=1024)],
        "egv_assemble_tokens_sel": null("pe", "cls", "pos", "temporal", "keep", "x") + zero("B", "T", "K", "D") + [dict(K=n + 1), dict(D=6),
                                   dict(B=BIG, T=64, n=1024, K=1024, D=1024)],
        "egv_assemble_tokens_bwd": null("dx") + zero("B", "T", "n", "D") + [dict(D=6), dict(T_model=T - 1), dict(B=BIG, T=64, T_model=64, n=1024, D=1024)],
        "egv_assemble_tokens_bwd_sel": null("dx", "keep") + zero("B", "T", "K", "D") + [dict(K=n + 1), dict(D=6), dict(T_model=T - 1),
                                       dict(B=BIG, T=64, T_model=64, n=1024, K=1024, D=1024)],
    }
    u8_extra = null("mean", "std") + [dict(std=std0), dict(std=stdn), dict(C=5)]
    bad["egv_patch_gather_u8"] = bad["egv_patch_gather"] + u8_extra
    bad["egv_patch_gather_u8_sel"] = bad["egv_patch_gather_sel"] + u8_extra
    bad["egv_patch_gather_u8_aug_sel"] = bad["egv_patch_gather_u8_aug"][:-1] + null("keep") + [dict(K=0), dict(K=n + 1), dict(lda=lda + 2),
                                                                                             dict(BT=BIG, R=4096, K=65536)]
    assert bad.keys() == valid.keys()
    for name, cases in bad.items():
        for case in cases:
            assert case.keys() <= valid[name].keys(), (name, case)
            assert getattr(h, name)(*{**valid[name], **case}.values()) == 1, (name, case)
    torch.cuda.synchronize()
    assert bool((hi == -7).all()) and bool((lo == -7).all())
    assert all(bool((t == -7.0).all()) for t in (x, d_pe, d_cls, d_pos, d_tmp))


# ------------------------------------------------------------------------------------------------ 4. the tower
ARCH = dict(img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2)
RATE, DPR = 0.5, 0.3
TOWER_SEED = 0      # torch seed at which the table of call 1 (B = 6, n = 16, K = 8) leaves position 13 unkept by every clip (found on the
#                     CPU with the mirror; the test asserts the condition)


def _tiny(arch=ARCH, **keys):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(arch)}
    vp.update(keys)
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    m.text_model.set_dropout(0.0, 0.0)
    return m


@pytest.fixture(scope="module")
def towers():
    """(rate 0.5, rate 0.5 + drop_path 0.3, built without the key), one set of weights."""
    from egovlp_amd.synth import synth_state_dict
    ms = [_tiny(patch_drop_rate=RATE), _tiny(patch_drop_rate=RATE, drop_path_rate=DPR), _tiny()]
    sd = synth_state_dict({k: v.shape for k, v in ms[0].state_dict().items()}, seed=7)
    for m in ms:
        m.load_state_dict(sd, strict=True)
        m.cuda()
        m.exec_ctx.set_precision("bf16x3", "bf16x3")
    return ms[0], ms[1], ms[2], sd


@pytest.mark.parametrize("with_drop_path", [False, True])
def test_tower_matches_the_fp64_reference_on_the_drawn_table(towers, with_drop_path):
    from egovlp_amd import ops
    from egovlp_amd.synth import synth_batch
    from oracle import egovlp_oracle as O
    m = towers[1] if with_drop_path else towers[0]
    sd = towers[3]
    B, T, n, K = 6, 2, 16, 8
    video = synth_batch(B, T=T, L=16, seed=31, res=64)["video"]
    gout = torch.randn(B, 128, generator=torch.Generator().manual_seed(4))
    m.train()
    m.exec_ctx.set_precision("bf16x3", "bf16x3")
    vm = m.video_model
    for prm in vm.parameters():
        prm.grad = None
    torch.manual_seed(TOWER_SEED)
    vm._drop_calls = 0
    m.exec_ctx.begin_step()
    emb = vm(video.cuda())
    emb.backward(gout.cuda())
    m.exec_ctx.join_side_stream()
    torch.cuda.synchronize()
    assert vm._drop_calls == 1
    keep = vm.last_patch_keep.cpu().numpy()
    assert keep.shape == (B, K) and np.array_equal(keep, R.patch_keep(B, n, K, vm._seed(vm.PATCH_DROP_SITE)))
    unkept = sorted(set(range(n)) - set(keep.reshape(-1).tolist()))
    assert unkept, "the table of this call keeps every position in some clip: choose another TOWER_SEED"
    scales, k = None, 1.0
    if with_drop_path:
        scales = [None] + [tuple(ops.drop_path_scales(B, vm.dpr[i], s_).cpu().double() for s_ in vm.drop_path_seeds(i)[:2]) for i in (1, 2)]
        for i in (1, 2):
            for s_, seed in zip(scales[i], vm.drop_path_seeds(i)[:2]):
                assert np.array_equal(s_.numpy(), DR.drop_path_scales(B, vm.dpr[i], seed).astype(np.float64))
        k = 1.0 / (1.0 - DPR)
    cfg = O.VideoCfg(num_frames=4, **ARCH)
    sdo = {k_: v.double().requires_grad_(True) for k_, v in sd.items() if k_.startswith("video_model.")}
    ref = R.tower(video.double(), sdo, cfg, keep, scales)
    (ref * gout.double()).sum().backward()
    e = rel(emb, ref)
    errs = {name: rel(prm.grad, sdo["video_model." + name].grad) for name, prm in vm.named_parameters()}
    worst = max(errs, key=errs.get)
    print("tower rate %.1f%s, unkept %s: embedding %.2e (bar %.1e), worst gradient %s %.2e (bar %.1e)" % (
        RATE, " + drop_path %.1f" % DPR if with_drop_path else "", unkept, e, 1e-3 * k, worst, errs[worst], 3e-3 * k))
    assert len(errs) == len(list(vm.parameters())) and all(prm.grad is not None for prm in vm.parameters())
    assert e < 1e-3 * k
    assert all(v < 3e-3 * k for v in errs.values()), {n_: v for n_, v in errs.items() if v >= 3e-3 * k}
    pg = vm.pos_embed.grad[0]
    assert float(pg[[1 + j for j in unkept]].abs().max()) == 0.0
    assert float(pg[0].abs().max()) > 0.0 and float(vm.temporal_embed.grad[0, T:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. the workload's kernels at their new sizes
def test_vit_b_width_at_rate_half_fp16_modes_against_bf16x3():
    """D = 768, 12 heads, depth 2, 224^2, B = 2, T = 4 at rate 0.5: K = 98, a space group of 99 keys, M = 2 x 393 = 786 rows in every
    GEMM -- the attention, LayerNorm and GEMM kernels of the workload at the sizes patch dropout gives them.  'f16mix' / 'f16' against
    'bf16x3' / 'bf16x3' on the SAME table (the call counter is put back between the runs)."""
    from test_gpu_model import F16_GRAD, _backward, _fbar
    from egovlp_amd.synth import synth_batch, synth_state_dict
    m = _tiny(dict(img_size=224, patch_size=16, embed_dim=768, depth=2, num_heads=12), patch_drop_rate=0.5)
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9), strict=True)
    m.cuda().train()
    vm = m.video_model
    B, T = 2, 4
    assert vm.patch_keep_count() == 98
    video = synth_batch(B, T=T, L=16, seed=32)["video"].cuda()
    gout = torch.randn(B, 768, generator=torch.Generator().manual_seed(5)).cuda()
    runs = {}
    c0 = vm._drop_calls
    for mode in (("bf16x3", "bf16x3"), ("f16mix", "f16")):
        m.exec_ctx.set_precision(*mode)
        for prm in m.parameters():
            prm.grad = None
        vm._drop_calls = c0
        m.exec_ctx.begin_step()
        emb = vm(video)
        _backward(m, (emb * gout).sum())
        m.exec_ctx.join_side_stream()
        torch.cuda.synchronize()
        runs[mode[0]] = (emb.detach().clone(), vm.last_patch_keep.clone(), {k: p.grad.detach().clone() for k, p in vm.named_parameters()})
    (e0, k0, g0), (e1, k1, g1) = runs["bf16x3"], runs["f16mix"]
    assert tuple(k0.shape) == (B, 98) and torch.equal(k0, k1)
    fbar = _fbar("f16mix")
    e = rel(e1, e0)
    errs = {k: rel(g1[k], g0[k]) for k in g0}
    worst = max(errs, key=errs.get)
    print("ViT-B width, K = 98, M = 786: f16mix/f16 against bf16x3: embedding %.2e (bar %.1e), worst gradient %s %.2e (bar %.1e)" % (
        e, fbar, worst, errs[worst], F16_GRAD))
    assert e < fbar
    assert all(v < F16_GRAD for v in errs.values()), {n_: v for n_, v in errs.items() if v >= F16_GRAD}


# ------------------------------------------------------------------------------------------------ 6. identity and replay
def test_eval_and_rate_zero_are_the_model_without_the_key(towers):
    from egovlp_amd.synth import synth_batch
    m, _, m0, _ = towers
    video = synth_batch(4, T=2, L=16, seed=33, res=64)["video"].cuda()
    vm, vm0 = m.video_model, m0.video_model
    m.eval()
    m0.eval()
    c0 = vm._drop_calls
    with torch.no_grad():
        assert torch.equal(vm(video), vm0(video))
    assert vm.last_patch_keep is None and vm._drop_calls == c0
    m.train()
    m0.train()
    vm.set_patch_drop_rate(0.0)
    try:
        assert torch.equal(vm(video), vm0(video)) and vm.last_patch_keep is None and vm._drop_calls == c0
    finally:
        vm.set_patch_drop_rate(RATE)


def test_fresh_tables_per_forward_and_replay_from_the_counter(towers):
    from egovlp_amd.synth import synth_batch
    m = towers[0]
    vm = m.video_model
    m.train()
    video = synth_batch(4, T=2, L=16, seed=34, res=64)["video"].cuda()
    c0 = vm._drop_calls
    with torch.no_grad():
        e1, k1 = vm(video), vm.last_patch_keep
        e2, k2 = vm(video), vm.last_patch_keep
        assert vm._drop_calls == c0 + 2 and tuple(k1.shape) == (4, 8)
        assert not torch.equal(k1, k2) and not torch.equal(e1, e2)
        vm._drop_calls = c0
        e3, k3 = vm(video), vm.last_patch_keep
        assert torch.equal(k3, k1) and torch.equal(e3, e1) and vm._drop_calls == c0 + 1
        # uint8 frames through the fused train transform with the identity box are the uint8 gather, bit for bit: the same table, the
        # same embedding
        u8 = torch.randint(0, 256, (4, 2, 3, 64, 64), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
        vm._drop_calls = c0
        e4 = vm(u8)
        vm._drop_calls = c0
        vm.set_input_augmentation(torch.tensor([[0, 0, 64, 64, 0]] * 4, dtype=torch.int32), 64)
        e5 = vm(u8)
        assert torch.equal(vm.last_patch_keep, k1) and torch.equal(e4, e5)


def test_cached_step_replays_its_tables(towers):
    """B = 8 in chunks of 4 at rate 0.5: pass 3 re-computes, bit for bit, the embeddings pass 1 cached (the video tower's call counter is
    put back per chunk by trainer/cached_step.py as it is); a second step draws other tables."""
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    m, _, _, sd = towers
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    torch.manual_seed(0)
    b = synth_batch(8, T=2, L=16, seed=35, res=64)
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
    print("cached step at patch_drop_rate %.1f: max |pass-3 - cached| %.3e, %.3e" % (RATE, diffs[0], diffs[1]))
    assert diffs == [0.0, 0.0]
    assert vm._drop_calls == c0 + 4                                          # once per chunk and step, not twice
    assert torch.equal(caches[0][0], caches[1][0])                           # the text tower draws nothing here
    assert not torch.equal(caches[0][1], caches[1][1])                       # the video tower drew other tables in the second step
