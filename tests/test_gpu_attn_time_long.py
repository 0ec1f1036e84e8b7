"""The time-attention kernels for 16 < T <= 64 frames (csrc/attn_time_long.hip: NT = ceil(T / 16) 16-row tiles per location, one workgroup
of NT waves per (clip, location, head)) through the C ABI on a real MI355X (`pytest -m gpu`).

Same construction and the same bars as tests/test_gpu_attn_long.py and tests/test_gpu_ops.py: the fp64 oracle on identical seeded inputs,
rel-L2 <= 2e-5 (three products) / 1.2e-2 (one product) on outputs and twice that on gradients, patch rows and the CLS row asserted
separately.  The fp16 variants mirror the two fp16 tests of tests/test_gpu_attn_long.py with their bars.  Each shape is the smallest that
exposes one way the tiling can go wrong (see the parametrisation).  Largest T tested: 64, the bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import egovlp_oracle as O  # noqa: E402

TOL = {3: 2e-5, 1: 1.2e-2}
E = 2.0 ** -6
TIME = 1


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


def _divided(ops, passes, B, T, n, H):
    """tests/test_gpu_attn_long.py::_divided with mode = 1."""
    mode = TIME
    g = torch.Generator().manual_seed(100 * mode + n)
    S = 1 + T * n
    qkv = torch.randn(B * S, 3 * H * 64, generator=g)
    qkv_pl = planes_from(ops, qkv, passes)
    out, lse = ops.divided_attn_fwd(qkv_pl, B, T, n, H, mode, passes)
    qd = qkv.double().requires_grad_(True)
    ref = O.var_attention_core(qd.view(B, S, -1), H, "time", n, T)
    tol = TOL[passes]
    e_patch, e_cls = rel(out.float().view(B, S, -1)[:, 1:], ref[:, 1:]), rel(out.float().view(B, S, -1)[:, 0], ref[:, 0])
    print("time attention passes %d (B, T, n, H) = %s: out patch rows %.2e, CLS row %.2e" % (passes, (B, T, n, H), e_patch, e_cls))
    assert e_patch < tol
    assert e_cls < tol                               # CLS row: per-location partials + combine kernel
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
@pytest.mark.parametrize("B,T,n,H", [(1, 17, 3, 1),       # the first size past the old limit: ONE frame in the second tile
                                     (2, 32, 5, 2),       # two full tiles; location 0 (which carries the CLS key) among others
                                     (1, 33, 2, 2),       # a third tile holding one frame
                                     (1, 48, 1, 1),       # a single location: the CLS partial has one group
                                     (1, 64, 3, 2),       # the bound
                                     (2, 24, 37, 3)])     # index decoding over many workgroups, n a multiple of nothing
def test_time_attention_past_16_frames(ops, passes, B, T, n, H):
    _divided(ops, passes, B, T, n, H)


@pytest.mark.parametrize("B,T,n,H", [(1, 17, 3, 1), (1, 40, 2, 2)])
def test_fp16_output_formats_and_fp16_gradient_planes_past_16_frames(ops, B, T, n, H):
    """tests/test_gpu_attn_long.py::test_fp16_output_formats_and_fp16_gradient_planes_past_288_keys in mode 1."""
    mode = TIME
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
        print("time attention backward T = %d, O as %s, dqkv as fp16 vs the bf16-plane result: %.2e" % (T, fmt, r))
        assert r < 4e-3                       # the bf16 rounding of the baseline's output dominates
    huge = ops.split_f32((torch.randn(B * S, D, generator=g) * 3.0e6).cuda(), 1)[0]
    got = ops.divided_attn_bwd(qkv, outs["f16"], huge, lse, B, T, n, H, mode, 1, grad_f16=True)
    assert bool(torch.isinf(got.hi.float()).any())          # overflow -> inf, never a clamped finite gradient


@pytest.mark.parametrize("B,T,n,H", [(1, 17, 3, 1), (1, 40, 2, 2)])
def test_fp16_attention_past_16_frames(ops, B, T, n, H):
    """tests/test_gpu_attn_long.py::test_fp16_attention_past_288_keys in mode 1: fp16-split qkv forward into each of the four output
    formats, fp16 backward (fp16 q / k / v / dO, dqkv as one fp16 plane)."""
    mode = TIME
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
        print("time attention backward T = %d (O as %s): fp16 operands %.2e, bf16 operands %.2e from the three-product result" % (T, o.fmt, r16, rbf))
        assert r16 < 1.2e-3 and r16 < rbf / 3
    huge = ops.f16_cast((dy * 1.0e4).cuda())
    bad = ops.divided_attn_bwd(qkv16, one, huge, lse16, B, T, n, H, mode, 1, grad_f16=True)
    assert not bool(torch.isfinite(bad.hi.float()).all())


def test_more_than_64_frames_is_refused_before_any_launch(ops, monkeypatch):
    """T = 65 in mode 1: a ValueError that names the limit, raised before the library is called (space mode has no bound on T)."""
    from egovlp_amd import _lib

    def no_lib():
        raise AssertionError("the library was reached")
    B, T, n, H = 1, 65, 1, 1
    S = 1 + T * n
    qkv = planes_from(ops, torch.zeros(B * S, 3 * H * 64), 1)
    monkeypatch.setattr(_lib, "lib", no_lib)
    with pytest.raises(ValueError, match="64"):
        ops.divided_attn_fwd(qkv, B, T, n, H, TIME, 1)
    with pytest.raises(ValueError, match="64"):
        ops.divided_attn_bwd(qkv, qkv, qkv, None, B, T, n, H, TIME, 1)
