"""The key-tiled ("long") attention kernels (csrc/attn_long.hip) for groups of more than 288 keys -- input resolutions above 224^2 and
captions of up to DistilBERT's 512 positions -- through the C ABI on a real MI355X (`pytest -m gpu`).

Same construction and the same bars as tests/test_gpu_ops.py (`test_divided_attention_fwd_bwd`, `test_text_attention_fwd_bwd`): the fp64
oracle on identical seeded inputs, rel-L2 <= 2e-5 (three products) / 1.2e-2 (one product) on outputs and twice that on gradients, patch
rows and the CLS row asserted separately.  The fp16 variants mirror tests/test_gpu_f16bwd.py with that file's bars.  The shapes are the
smallest at which each way the tiling can go wrong shows: the first size past the old limit, a ragged last tile, a last tile of ONE key
(577 = 9 * 64 + 1), the largest documented size (785 keys), and more groups than a 256-workgroup grid.  Largest size tested: 785 keys."""
import numpy as np
import pytest
import torch

import drop_path_ref as R

pytestmark = pytest.mark.gpu

from oracle import egovlp_oracle as O  # noqa: E402

TOL = {3: 2e-5, 1: 1.2e-2}
E = 2.0 ** -6


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


def planes_from(ops, x, passes):
    return ops.split_f32(x.cuda().contiguous(), passes)[0]


def _divided(ops, passes, mode, B, T, n, H):
    g = torch.Generator().manual_seed(100 * mode + n)
    S = 1 + T * n
    qkv = torch.randn(B * S, 3 * H * 64, generator=g)
    qkv_pl = planes_from(ops, qkv, passes)
    out, lse = ops.divided_attn_fwd(qkv_pl, B, T, n, H, mode, passes)
    qd = qkv.double().requires_grad_(True)
    ref = O.var_attention_core(qd.view(B, S, -1), H, "space" if mode == 0 else "time", n, T)
    tol = TOL[passes]
    e_patch, e_cls = rel(out.float().view(B, S, -1)[:, 1:], ref[:, 1:]), rel(out.float().view(B, S, -1)[:, 0], ref[:, 0])
    print("attention mode %d passes %d (B, T, n, H) = %s: out patch rows %.2e, CLS row %.2e" % (mode, passes, (B, T, n, H), e_patch, e_cls))
    assert e_patch < tol
    assert e_cls < tol                               # CLS row: per-group partials + combine kernel
    if mode == 0 and T == 1:                         # one frame group: the patch rows' lse is the plain log-sum-exp over CLS + n keys
        q, k, _ = qkv.double().view(B, S, 3, H, 64).unbind(2)
        sc = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125
        lse_ref = torch.logsumexp(sc, -1)
        assert rel(lse[:, :, 1:], lse_ref[:, :, 1:]) < tol      # (an error of the scores moves lse by at most as much)
    d_out = torch.randn(B * S, H * 64, generator=g)
    ref.backward(d_out.view(B, S, -1).double())
    dqkv = ops.divided_attn_bwd(qkv_pl, out, planes_from(ops, d_out, passes), lse, B, T, n, H, mode, passes)
    got = dqkv.float().view(B, S, -1)
    want = qd.grad.view(B, S, -1)
    g_patch, g_cls = rel(got[:, 1:], want[:, 1:]), rel(got[:, 0], want[:, 0])
    print("   dqkv patch rows %.2e, CLS row %.2e" % (g_patch, g_cls))
    assert g_patch < tol * 2
    assert g_cls < tol * 2                           # the CLS token's own gradients: fp32 atomics + finish kernel


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("B,T,n,H", [(1, 1, 288, 1),      # 289 keys: the first size past the LDS-resident kernels
                                     (1, 2, 300, 2),      # ragged last tile, two frame groups sharing one CLS
                                     (2, 1, 576, 1),      # 577 keys: the last 64-key tile holds ONE key
                                     (1, 2, 784, 2),      # 785 keys: the largest documented size
                                     (3, 4, 300, 24)])    # 288 groups (x 3 query blocks): more than a 256-workgroup grid
def test_space_attention_past_288_keys(ops, passes, B, T, n, H):
    _divided(ops, passes, 0, B, T, n, H)


@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("B,T,n,H", [(1, 2, 300, 2), (1, 16, 324, 2)])
def test_time_attention_at_high_resolution_patch_counts(ops, passes, B, T, n, H):
    """The other half of a high-resolution block: B n H groups of T keys (its kernels do not depend on n beyond the group count)."""
    _divided(ops, passes, 1, B, T, n, H)


@pytest.mark.parametrize("B,T,n,H", [(1, 2, 300, 2), (2, 1, 576, 1)])
def test_fp16_output_formats_and_fp16_gradient_planes_past_288_keys(ops, B, T, n, H):
    """tests/test_gpu_f16bwd.py::test_attention_fp16_output_formats_and_fp16_gradient_planes on the long path."""
    mode = 0
    S, D = 1 + T * n, H * 64
    g = torch.Generator().manual_seed(B + T + n)
    qkv = ops.split_f32((torch.randn(B * S, 3 * D, generator=g) * 1.5).cuda(), 3)[0]
    ref, lse = ops.divided_attn_fwd(qkv, B, T, n, H, mode, 3)
    o_ref = ref.float().cpu().double()
    outs = {}
    for fmt in ("f16x2", "f16", "bf16+f16"):
        o, l2 = ops.divided_attn_fwd(qkv, B, T, n, H, mode, 3, out_fmt=fmt)
        assert torch.equal(l2, lse)
        outs[fmt] = o
    assert rel(outs["f16x2"].hi.cpu().double() + outs["f16x2"].lo.cpu().double(), o_ref) < 2e-5       # a1 + a2 = O to ~2^-17
    assert rel(outs["f16x2"].hi.cpu().double() / (1.0 - E), o_ref) < 4e-4
    assert rel(outs["f16"].hi.cpu(), o_ref) < 4e-4 and outs["f16"].lo is None
    assert torch.equal(outs["bf16+f16"].lo.cpu().view(torch.int16), outs["f16"].hi.cpu().view(torch.int16))
    d_out = ops.split_f32((torch.randn(B * S, D, generator=g) * 200.0).cuda(), 1)[0]           # a "scaled" gradient
    base = ops.divided_attn_bwd(qkv, outs["bf16+f16"], d_out, lse, B, T, n, H, mode, 1)
    for fmt in ("f16x2", "f16"):
        got = ops.divided_attn_bwd(qkv, outs[fmt], d_out, lse, B, T, n, H, mode, 1, grad_f16=True)
        assert got.fmt == "f16" and got.lo is None
        r = rel(got.hi.cpu(), base.hi.cpu().float())
        print("long attention backward, O as %s, dqkv as fp16 vs the bf16-plane result: %.2e" % (fmt, r))
        assert r < 4e-3                       # the bf16 rounding of the baseline's output dominates
    huge = ops.split_f32((torch.randn(B * S, D, generator=g) * 3.0e6).cuda(), 1)[0]
    got = ops.divided_attn_bwd(qkv, outs["f16"], huge, lse, B, T, n, H, mode, 1, grad_f16=True)
    assert bool(torch.isinf(got.hi.float()).any())          # overflow -> inf, never a clamped finite gradient


@pytest.mark.parametrize("B,T,n,H", [(1, 2, 300, 2), (2, 1, 576, 1)])
def test_fp16_attention_past_288_keys(ops, B, T, n, H):
    """tests/test_gpu_f16bwd.py::test_fp16_attention_matches_the_split_bf16_attention_and_beats_the_bf16_backward on the long path:
    fp16-split qkv forward into each of the four output formats, fp16 backward (fp16 q / k / v / dO, dqkv as one fp16 plane)."""
    mode = 0
    S, D = 1 + T * n, H * 64
    g = torch.Generator().manual_seed(B + T + n)
    x = torch.randn(B * S, 3 * D, generator=g) * 1.5
    qkv3 = ops.split_f32(x.cuda(), 3)[0]
    hi = x.to(torch.float16)
    qkv16 = ops.Planes(hi.cuda(), (x - hi.float()).to(torch.float16).cuda(), B * S, 3 * D, "f16s")
    ref, lse = ops.divided_attn_fwd(qkv3, B, T, n, H, mode, 3)
    o_ref = ref.float().cpu().double()
    got, lse16 = ops.divided_attn_fwd(qkv16, B, T, n, H, mode, 3, out_fmt="f16x2")
    r_fwd = rel(got.hi.cpu().double() + got.lo.cpu().double(), o_ref)
    assert r_fwd < 3e-5 and rel(lse16, lse) < 1e-5, (r_fwd, rel(lse16, lse))
    one, _ = ops.divided_attn_fwd(qkv16, B, T, n, H, mode, 3, out_fmt="f16")
    assert rel(one.hi.cpu(), o_ref) < 4e-4
    split, _ = ops.divided_attn_fwd(qkv16, B, T, n, H, mode, 3)                        # split-bf16 planes
    assert rel(split.float(), o_ref) < 3e-5
    both, _ = ops.divided_attn_fwd(qkv16, B, T, n, H, mode, 3, out_fmt="bf16+f16")
    assert torch.equal(both.lo.cpu().view(torch.int16), one.hi.cpu().view(torch.int16))
    dy = torch.randn(B * S, D, generator=g) * 200.0
    want = ops.divided_attn_bwd(qkv3, ref, ops.split_f32(dy.cuda(), 3)[0], lse, B, T, n, H, mode, 3).float().cpu().double()
    bf = ops.divided_attn_bwd(qkv3, ref, ops.split_f32(dy.cuda(), 1)[0], lse, B, T, n, H, mode, 1).hi.cpu().float()
    d16 = ops.f16_cast(dy.cuda())
    for o in (got, one):
        f16 = ops.divided_attn_bwd(qkv16, o, d16, lse16, B, T, n, H, mode, 1, grad_f16=True)
        r16, rbf = rel(f16.hi.cpu(), want), rel(bf, want)
        print("long attention backward (O as %s): fp16 operands %.2e, bf16 operands %.2e from the three-product result" % (o.fmt, r16, rbf))
        assert r16 < 1.2e-3 and r16 < rbf / 3
    huge = ops.f16_cast((dy * 1.0e4).cuda())
    bad = ops.divided_attn_bwd(qkv16, one, huge, lse16, B, T, n, H, mode, 1, grad_f16=True)
    assert not bool(torch.isfinite(bad.hi.float()).all())


# ------------------------------------------------------------------------------------------------ text
@pytest.mark.parametrize("passes", [3, 1])
@pytest.mark.parametrize("L", [289, 384, 512])
def test_text_attention_past_288_tokens(ops, passes, L):
    g = torch.Generator().manual_seed(11)
    B, H = 3, 2
    q, k, v = [torch.randn(B * L, H * 64, generator=g) for _ in range(3)]
    lens = torch.tensor([L, 9, (2 * L) // 3])
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    out, lse = ops.text_attn_fwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), B, L, H, passes)
    qd, kd, vd = [t.double().view(B, L, -1).requires_grad_(True) for t in (q, k, v)]
    ref = O.text_attention_core(qd, kd, vd, mask, H)
    e = rel(out.float().view(B, L, -1), ref)
    print("text attention L=%d passes %d: out %.2e" % (L, passes, e))
    assert e < TOL[passes]
    d_out = torch.randn(B * L, H * 64, generator=g)
    ref.backward(d_out.view(B, L, -1).double())
    dq, dk, dv = ops.text_attn_bwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), d_out.cuda(), lse, B, L, H, passes)
    for name, a, b in (("dq", dq, qd.grad), ("dk", dk, kd.grad), ("dv", dv, vd.grad)):
        e = rel(a.view(B, L, -1), b)
        print("   %s %.2e" % (name, e))
        assert e < TOL[passes] * 2


def _keep_scale(B, H, L, p, seed):
    """fp32 [B, H, L, L]: the counter-based mask of csrc/common.h at element index ((b H + h) L + q) L + k -- what egv_text_attn_fwd
    multiplies the attention weights by (numpy mirror of egv_mix32 / egv_make_drop: tests/drop_path_ref.py)."""
    idx = np.arange(B * H * L * L, dtype=np.uint64)
    s0, s1 = np.uint32(seed & R.M32), np.uint32(seed >> 32)
    thresh, scale = R.drop_params(p)
    h = R.mix32(R.mix32((idx & np.uint64(R.M32)).astype(np.uint32) ^ s0) ^ (idx >> np.uint64(32)).astype(np.uint32) ^ s1)
    return torch.from_numpy(np.where(h >= np.uint32(thresh), scale, np.float32(0.0)).astype(np.float32)).view(B, H, L, L)


def _masked_attention_ref(q, k, v, mask, keep, B, L, H):
    """fp64: softmax(q k^T / 8 + key mask) o keep . v -- HF's eager attention with the dropout mask as an input."""
    qd, kd, vd = [t.double().view(B, L, H, 64).transpose(1, 2).detach().requires_grad_(True) for t in (q, k, v)]
    sc = qd @ kd.transpose(-1, -2) * 0.125
    sc = sc.masked_fill(mask.view(B, 1, 1, L) == 0, float("-inf"))
    out = (torch.softmax(sc, -1) * keep.double()) @ vd
    return (qd, kd, vd), out.transpose(1, 2).reshape(B, L, H * 64)


@pytest.mark.parametrize("passes", [3, 1])
def test_text_attention_dropout_past_288_tokens(ops, passes):
    """p = 0.1 at L = 320: forward and backward against the fp64 attention that takes the counter-based mask as an input."""
    B, L, H, p, seed = 3, 320, 2, 0.1, 0x1234567855
    g = torch.Generator().manual_seed(12)
    q, k, v = [torch.randn(B * L, H * 64, generator=g) for _ in range(3)]
    lens = torch.tensor([L, 9, (2 * L) // 3])
    mask = (torch.arange(L)[None] < lens[:, None]).long()
    keep = _keep_scale(B, H, L, p, seed)
    out, lse = ops.text_attn_fwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), B, L, H, passes, p, seed)
    (qd, kd, vd), ref = _masked_attention_ref(q, k, v, mask, keep, B, L, H)
    e = rel(out.float().view(B, L, -1), ref)
    print("text attention with dropout L=%d passes %d: out %.2e" % (L, passes, e))
    assert e < TOL[passes]
    d_out = torch.randn(B * L, H * 64, generator=g)
    ref.backward(d_out.view(B, L, -1).double())
    dq, dk, dv = ops.text_attn_bwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), d_out.cuda(), lse, B, L, H, passes, dropout_p=p, seed=seed)
    for name, a, b in (("dq", dq, qd.grad), ("dk", dk, kd.grad), ("dv", dv, vd.grad)):
        e = rel(a.view(B, L, H, 64).transpose(1, 2), b)
        print("   %s %.2e" % (name, e))
        assert e < TOL[passes] * 2
    same, _ = ops.text_attn_fwd(q.cuda(), k.cuda(), v.cuda(), mask.cuda(), B, L, H, passes, p, seed)
    assert torch.equal(out.hi, same.hi)


@pytest.mark.parametrize("L", [256, 320])
def test_dropout_mask_is_the_same_function_of_b_h_q_k_on_both_paths(ops, L):
    """q = k = 0 -> uniform weights; V = one-hot rows for the first 64 keys -> output channel j of query i IS the dropped weight of key
    j: the kept pattern of the leading 64 x 64 corner is the reference generator's at element index ((b H + h) L + q) L + k, at L = 256
    (LDS-resident kernel) and at L = 320 (key-tiled kernel) alike."""
    B, H, p, seed = 2, 3, 0.25, 77
    D = H * 64
    q = torch.zeros(B * L, D, device="cuda")
    k = torch.zeros_like(q)
    v = torch.zeros(B * L, D, device="cuda")
    for j in range(64):
        v.view(B, L, H, 64)[:, j, :, j] = 1.0
    mask = torch.ones(B, L, dtype=torch.long, device="cuda")
    out, _ = ops.text_attn_fwd(q, k, v, mask, B, L, H, 3, p, seed)
    w = out.float().view(B, L, H, 64).permute(0, 2, 1, 3).cpu()                # [B, H, query, key < 64]
    keep = _keep_scale(B, H, L, p, seed)[:, :, :, :64]
    assert torch.equal(w[:, :, :64] > 0, keep[:, :, :64] > 0)                  # the 64 x 64 corner
    assert torch.equal(w > 0, keep > 0)                                        # and every query row (the later query blocks too)
    assert torch.allclose(w, keep / L, rtol=1e-4, atol=0)
