"""Mixup / CutMix inside the patch gather on a real MI355X (`pytest -m gpu`): egv_patch_gather_mix and egv_patch_gather_u8_aug_mix on
every input path the model has (fp32, uint8, uint8 + boxes, uint8 + boxes + colour; each over all patches and over K = 3 of 4 kept
positions), against the UNMIXED gathers of the same path.

1. CutMix is a selection: every element of both planes is a bit copy of the unmixed gather of the clip (outside the box) or of its
   partner (inside).  2. Mixup: lam 0 / 1 give the partner's / the clip's own bits; in between |device - (lam a + (1 - lam) b)| <= 4e-5
   with a, b the hi + lo values of the two unmixed gathers -- two plane-rounding steps of 2e-5 (the figure of tests/test_gpu_ops.py at
   |value| <= 2.7): one for the result's own split, at most one for the convex combination of the inputs' splits; the fp32 rounding of
   the blend is two orders of magnitude below.  3. op 0 everywhere: the bits of today's entry.  4. Tables out of range give the bits
   of the clamped tables; NULL tables, R % 4 != 0 and a colour table with C != 3 are EGV_ERR_ARG with nothing launched.  5. Through the
   tiny tower: the fused transform + mix on uint8 against the same forward on the host-made mixed clip, within the project's 1e-3.

Measured on MI355X.  1, 3, 4: bit equality on all eight path / keep combinations at both geometries.  2: max |device - (lam a +
(1 - lam) b)| 1.9e-5 / 1.7e-5 (fp32, P = 16 / 14), 2.4e-5 (uint8), 2.2e-5 / 1.8e-5 (boxes), 1.7e-5 (colour); bar 4e-5.  5: embedding
rel-L2 3.9e-6 against the host-made mixed clip (the unmixed forward is 0.48 away), 0 for the mix applied to the fp32 clip on the device.
The first build missed 1: 160 of 18 432 lo-plane elements of the train-transform paths differed in the last place, until the bilinear
arithmetic of `AugRow` was pinned (csrc/video_input.hip)."""
import ctypes as C

import pytest
import torch

import mix_ref as MR
from test_gpu_color_jitter import _model_inputs, _tiny, bits, code_of, host_transform, im2col, rel

pytestmark = pytest.mark.gpu

B, T, HS, WS = 3, 2, 40, 52
GEOMS = [(16, 32), (14, 28)]
PATHS = ["f32", "u8", "aug", "color"]


def _inputs(path, R, seed=31):
    """-> (video on the device, keyword arguments of ops.patch_gather for this input path)"""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (B, T, 3, HS, WS), generator=g, dtype=torch.uint8)
    f32 = torch.randn(B, T, 3, R, R, generator=g).clamp(-2.6, 2.6)           # |value| <= 2.7: the plane step the bars quote
    boxes = torch.tensor([[0, 0, HS, WS, 0], [3, 5, 30, 37, 1], [8, 16, R, R, 0]], dtype=torch.int32).cuda()
    color = torch.tensor([[0.6, 1.0, 0.0, code_of((1,))], [1.0, 1.4, 0.0, code_of((2,))], [1.0, 1.0, -0.1, code_of((3,))]],
                         dtype=torch.float32).cuda()
    if path == "f32":
        return f32.cuda(), {}
    if path == "u8":
        return u8[..., :R, :R].contiguous().cuda(), {}
    if path == "aug":
        return u8.cuda(), {"aug": (boxes, R)}
    return u8.cuda(), {"aug": (boxes, R), "color": color}


KEEP = torch.tensor([[0, 1, 3], [1, 2, 3], [0, 2, 3]], dtype=torch.int32)


def _table(rows, lam):
    """rows: (op, y0, y1, x0, x1) per clip; partner = the flipped batch"""
    idx = torch.tensor([[B - 1 - b] + list(r) for b, r in enumerate(rows)], dtype=torch.int32)
    return idx.cuda(), torch.tensor(lam, dtype=torch.float32).cuda()


def _gather(video, P, kw, keep=None, mix=None):
    from egovlp_amd import ops
    pl = ops.patch_gather(video, P, 3, keep=None if keep is None else keep.cuda(), **kw, **({} if mix is None else {"mix": mix}))
    return pl.hi, pl.lo


def _partner_rows(plane, partner):
    """rows of the full unmixed gather -> the same rows of every clip's partner (frame t of clip b -> frame t of partner[b])"""
    return plane.view(B, -1, plane.shape[1])[partner.long().cpu()].reshape(plane.shape)


def _kept_rows(keep, n):
    bt = torch.arange(B * T)
    return (bt[:, None] * n + keep.long()[bt // T]).reshape(-1).cuda()


def _box_mask(idx, R, P, cols):
    """[B*T*n, cols] bool: the elements of the planes that lie inside their clip's cutmix box"""
    m = torch.zeros(B, T, 3, R, R, dtype=torch.bool)
    for b, (_, op, y0, y1, x0, x1) in enumerate(MR.clamp_tables(idx.cpu(), B, R, R).tolist()):
        if op == 2:
            m[b, :, :, y0:y1, x0:x1] = True
    out = torch.zeros(B * T * (R // P) ** 2, cols, dtype=torch.bool)
    out[:, :3 * P * P] = im2col(m, P)
    return out.cuda()


def _cut_tables(R):
    """the four boxes of the issue, on two tables (clip 1 is its own partner): x0 / x1 no multiples of 4 and across a patch edge; empty;
    the whole frame; touching two borders"""
    return [_table([(2, 5, R - 9, 6, 19), (2, 7, 7, 3, 3), (2, 0, R, 0, R)], [0.6, 1.0, 0.0]),
            _table([(2, 0, 11, R - 9, R), (2, 0, R, 0, R), (2, 3, R - 2, 1, R - 13)], [0.7, 0.0, 0.5])]


@pytest.mark.parametrize("P,R", GEOMS)
@pytest.mark.parametrize("path", PATHS)
def test_1_cutmix_is_a_selection_bit_for_bit(path, P, R):
    video, kw = _inputs(path, R)
    n = (R // P) ** 2
    full = _gather(video, P, kw)
    for idx, lam in _cut_tables(R):
        inside = _box_mask(idx, R, P, full[0].shape[1])
        assert 0 < int(inside.sum()) < inside.numel()
        want = [torch.where(inside, bits(_partner_rows(pl, idx[:, 0])), bits(pl)) for pl in full]
        for keep in (None, KEEP):
            got = _gather(video, P, kw, keep, (idx, lam))
            torch.cuda.synchronize()
            rows = slice(None) if keep is None else _kept_rows(keep, n)
            for g, w, name in zip(got, want, ("hi", "lo")):
                assert g.shape[0] == B * T * (n if keep is None else 3)
                assert torch.equal(bits(g), w[rows]), (path, P, name, keep is not None)
    # the box did something: clip 0 and its partner differ inside it
    assert not torch.equal(bits(full[0])[inside], bits(_partner_rows(full[0], idx[:, 0]))[inside])


@pytest.mark.parametrize("P,R", GEOMS)
@pytest.mark.parametrize("path", PATHS)
def test_2_mixup_blends_the_two_unmixed_gathers(path, P, R):
    """Measured on MI355X, max |device - (lam a + (1 - lam) b)| over lam 0.3 / 0.75 and both keep variants: fp32 1.905e-5 (P = 16) /
    1.720e-5 (P = 14); uint8 2.442e-5 / 2.442e-5; boxes 2.175e-5 / 1.823e-5; boxes + colour 1.674e-5 / 1.675e-5.  Bar 4e-5."""
    video, kw = _inputs(path, R)
    n = (R // P) ** 2
    full = _gather(video, P, kw)
    own = [bits(pl) for pl in full]
    other = [bits(_partner_rows(pl, torch.tensor([2, 1, 0]))) for pl in full]
    a = full[0].double() + full[1].double()
    b = _partner_rows(full[0], torch.tensor([2, 1, 0])).double() + _partner_rows(full[1], torch.tensor([2, 1, 0])).double()
    worst = 0.0
    for keep in (None, KEEP):
        rows = slice(None) if keep is None else _kept_rows(keep, n)
        for lam, want in (([1.0, 1.0, 1.0], own), ([0.0, 0.0, 0.0], other)):
            got = _gather(video, P, kw, keep, _table([(1, 0, 0, 0, 0)] * B, lam))
            for g, w in zip(got, want):
                assert torch.equal(bits(g), w[rows]), (path, P, lam[0], keep is not None)
        lam = [0.3, 0.75, 0.3]
        got = _gather(video, P, kw, keep, _table([(1, 0, 0, 0, 0)] * B, lam))
        l32 = torch.tensor(lam, dtype=torch.float32).repeat_interleave(T * n).view(-1, 1).cuda()
        want = (l32.double() * a + (1.0 - l32).double() * b)[rows]
        err = float(((got[0].double() + got[1].double()) - want).abs().max())
        worst = max(worst, err)
        assert err <= 4e-5, (path, P, keep is not None, err)
    assert float((a - b).abs().max()) > 0.5                                  # the two clips differ: a blend is not a copy
    print("mixup %s P=%d: max |device - (lam a + (1 - lam) b)| %.3e (bar 4e-5)" % (path, P, worst))


@pytest.mark.parametrize("P,R", GEOMS)
@pytest.mark.parametrize("path", PATHS)
def test_3_op_zero_everywhere_is_todays_entry_and_4_bad_tables_are_clamped(path, P, R):
    video, kw = _inputs(path, R)
    wild = (torch.tensor([[B + 7, 2, -100, 900, -7, 13], [-5, 1, 0, 0, 0, 0], [1, 7, 2, 9, 2, 9]], dtype=torch.int32).cuda(),
            torch.tensor([0.6, 0.5, 0.25], dtype=torch.float32).cuda())
    tame = (MR.clamp_tables(wild[0].cpu(), B, R, R).to(torch.int32).cuda(), wild[1])
    assert tame[0].tolist() == [[2, 2, 0, R, 0, 13], [0, 1, 0, 0, 0, 0], [1, 3, 2, 9, 2, 9]]
    for keep in (None, KEEP):
        plain = _gather(video, P, kw, keep)
        zero = _gather(video, P, kw, keep, _table([(0, 3, 9, 3, 9), (0, 0, 0, 0, 0), (3, 0, R, 0, R)], [0.5, 0.0, 0.25]))
        a, b = _gather(video, P, kw, keep, wild), _gather(video, P, kw, keep, tame)
        torch.cuda.synchronize()
        for k in range(2):
            assert torch.equal(bits(zero[k]), bits(plain[k])), (path, P, keep is not None)
            assert torch.equal(bits(a[k]), bits(b[k])) and not torch.equal(bits(a[k]), bits(plain[k]))
        assert bool(torch.isfinite(a[0].float()).all())


def test_4_c_level_refusals_launch_nothing():
    from egovlp_amd import _lib
    h = _lib.lib()
    BT, T_, R, P, n = 2, 2, 32, 16, 4
    lda = 3 * P * P
    u8 = torch.zeros(BT, 4, 40, 40, dtype=torch.uint8, device="cuda")
    f32 = torch.zeros(BT, 3, R, R, device="cuda")
    hi, lo = (torch.full((BT * n, lda + 256), -7, dtype=torch.int16, device="cuda") for _ in range(2))
    keep = torch.tensor([[0, 3]], dtype=torch.int32, device="cuda")
    boxes = torch.tensor([[0, 0, 40, 40, 0]], dtype=torch.int32, device="cuda")
    color = torch.tensor([[1.2, 0.8, 0.1, code_of((1, 2, 3))]], dtype=torch.float32, device="cuda")
    idx = torch.tensor([[0, 2, 0, 8, 0, 8]], dtype=torch.int32, device="cuda")
    lam = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    mean, std = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5), (C.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    p = lambda t: t.data_ptr()
    aug = dict(video=p(u8), BT=BT, T=T_, C=3, Hs=40, Ws=40, R=R, P=P, boxes=p(boxes), color=p(color), mean=mean, std=std, idx=p(idx),
               lam=p(lam), keep=None, K=0, a_hi=p(hi), a_lo=p(lo), lda=lda + 256, stream=None)
    cases = [dict(idx=None), dict(lam=None), dict(R=30), dict(C=4), dict(C=1), dict(boxes=None), dict(video=None), dict(a_hi=None),
             dict(P=15), dict(BT=3), dict(lda=lda - 4), dict(std=(C.c_float * 4)(0.25, 0.0, 0.25, 0.25)), dict(BT=1 << 30, R=4096),
             dict(keep=p(keep), K=0), dict(keep=p(keep), K=n + 1)]
    for case in cases:
        assert h.egv_patch_gather_u8_aug_mix(*{**aug, **case}.values()) == 1, case
    plain = dict(video=p(f32), u8=0, BT=BT, T=T_, C=3, H=R, W=R, P=P, mean=None, std=None, idx=p(idx), lam=p(lam), keep=None, K=0,
                 a_hi=p(hi), a_lo=p(lo), lda=lda + 256, stream=None)
    for case in [dict(idx=None), dict(lam=None), dict(video=None), dict(a_hi=None), dict(P=15), dict(BT=3), dict(T=0), dict(lda=lda - 4),
                 dict(u8=1), dict(u8=1, mean=mean, std=(C.c_float * 4)(0.25, 0.0, 0.25, 0.25)), dict(keep=p(keep), K=n + 1)]:
        assert h.egv_patch_gather_mix(*{**plain, **case}.values()) == 1, case
    torch.cuda.synchronize()
    assert bool((hi == -7).all()) and bool((lo == -7).all())


def test_5_through_the_model_against_the_host_made_mixed_clip():
    Bm = 4
    u8, boxes, color = _model_inputs(Bm, 35)
    idx = torch.tensor([[3, 2, 9, 50, 14, 41], [2, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 2, 0, 30, 33, 64]], dtype=torch.int32)
    lam = torch.tensor([1.0 - 41 * 27 / 4096.0, 0.4, 0.7, 1.0 - 30 * 31 / 4096.0], dtype=torch.float32)
    host = host_transform(u8, boxes, color, 64)
    mixed = MR.mix_clips(host, idx, lam)
    m = _tiny()
    vm = m.video_model
    m.eval()
    with torch.no_grad():
        vm.set_input_augmentation(boxes, 64, color)
        vm.set_input_mix(idx, lam)                                          # host tables: validated, then moved
        e_dev = vm(u8.cuda())
        e_host = vm(mixed.cuda())
        vm.set_input_augmentation(boxes, 64, color)
        e_plain = vm(u8.cuda())                                             # one-shot: this forward mixes nothing
        e_unmixed = vm(host.cuda())
        vm.set_input_mix(idx.cuda(), lam.cuda())                            # the fp32 path, device tables
        e_f32 = vm(host.cuda())
    r, r0, rf = rel(e_dev, e_host), rel(e_plain, e_host), rel(e_f32, e_host)
    print("model: fused transform + mix on uint8 against the host-made mixed clip: embedding rel %.2e; the unmixed forward %.2e; "
          "the mix on the fp32 clip %.2e" % (r, r0, rf))
    assert r < 1e-3 and rf < 1e-3 and rel(e_plain, e_unmixed) < 1e-3
    assert r0 > 1e-2                                                        # the mix has happened: ten bars away from no mix
    # train mode with patch dropout: the mixed gather over the kept patches, finite gradients
    md = _tiny(patch_drop_rate=0.5)
    md.train()
    vd = md.video_model
    vd.set_input_augmentation(boxes.cuda(), 64, color.cuda())
    vd.set_input_mix(idx.cuda(), lam.cuda())
    out = vd(u8.cuda())
    out.sum().backward()
    md.exec_ctx.join_side_stream()
    torch.cuda.synchronize()
    assert tuple(vd.last_patch_keep.shape) == (Bm, 8) and bool(torch.isfinite(out).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in vd.parameters())
