"""LAMB (egovlp_amd.optim.LAMB, csrc/lamb.hip) without a GPU: the fp64 restatement of tests/lamb_ref.py judged on its own -- it is the
only oracle there is -- and the host side on CPU tensors over the do-nothing C-ABI stand-in (tests/mock_hip.py): which entry points a
step calls, in which order, and that AdamW's steps call what they called before LAMB existed.  The kernels' values:
tests/test_gpu_lamb.py."""
import math
import os
import re

import pytest
import torch

import lamb_ref as L
import multi_tensor_ref as R
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMB_CALLS = ("egv_lamb_parts", "egv_lamb_stage1_multi", "egv_lamb_ratio", "egv_lamb_stage2_multi")
THREE = ["egv_lamb_stage1_multi", "egv_lamb_ratio", "egv_lamb_stage2_multi"]


def _inputs(numels=(1, 5, 300, 0, 4099), step=7, seed=3):
    return R.adamw_inputs(list(numels), step, 1.0, seed)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _naive(ps, gs, ms, vs, lr, b1, b2, eps, wd, t, grad_scale, always_adapt, trust_clip, correct_bias=True):
    """The rule written a second time, tensor by tensor with torch's in-place fp64 operations (the shape of timm's loop)."""
    lr, b1, b2, eps, wd, grad_scale = (R.f32(x) for x in (lr, b1, b2, eps, wd, grad_scale))
    out = []
    for p, g, m, v in zip(ps, gs, ms, vs):
        p, g, m, v = p.double().clone(), g.double() * grad_scale, m.double().clone(), v.double().clone()
        m.mul_(b1).add_(g, alpha=float(torch.tensor(1.0) - torch.tensor(b1, dtype=torch.float32)))
        v.mul_(b2).addcmul_(g, g, value=float(torch.tensor(1.0) - torch.tensor(b2, dtype=torch.float32)))
        c = math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if correct_bias else 1.0
        u = (m / v.sqrt().add_(eps)).mul_(c).add_(p, alpha=wd)
        r = 1.0
        if wd != 0.0 or always_adapt:
            pn, un = float(torch.linalg.vector_norm(p)), float(torch.linalg.vector_norm(u))
            if pn > 0.0 and un > 0.0:
                r = pn / un
        if trust_clip:
            r = min(r, 1.0)
        p.add_(u, alpha=-lr * r)
        out.append((p, m, v, r))
    return out


@pytest.mark.parametrize("wd,always_adapt,trust_clip,cb", [(0.01, False, False, True), (0.0, False, False, True), (0.0, True, True, True),
                                                             (0.01, False, True, False)])
def test_reference_agrees_with_a_naive_per_tensor_loop(wd, always_adapt, trust_clip, cb):
    ps, gs, ms, vs = _inputs()
    b1, b2 = L.BETAS
    ref = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, wd, L.correction(b1, b2, 7, cb), 0.5, always_adapt, trust_clip)
    for k, (p, m, v, r) in enumerate(_naive(ps, gs, ms, vs, L.LR, b1, b2, L.EPS, wd, 7, 0.5, always_adapt, trust_clip, cb)):
        assert abs(ref["r"][k] - r) <= 1e-13 * r
        for a, b in ((ref["p"][k], p), (ref["m"][k], m), (ref["v"][k], v)):
            assert torch.allclose(a, b, rtol=1e-13, atol=0.0)
    assert ref["r"][3] == 1.0 and ref["p"][3].numel() == 0                           # the empty tensor


def test_without_adaptation_the_reference_is_the_fp64_adamw_rule():
    """wd = 0 and always_adapt off: r = 1 and u = c m / (sqrt(v) + eps), so the step is adamw_ref64's with step_size = lr c."""
    from egovlp_amd.optim import adamw_step_size
    ps, gs, ms, vs = _inputs()
    b1, b2 = L.BETAS
    for t, cb in ((1, True), (7, True), (7, False)):
        c = L.correction(b1, b2, t, cb)
        ref = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, 0.0, c, 0.25)
        assert ref["r"] == [1.0] * len(ps)
        for k in range(len(ps)):
            a = R.adamw_ref64(ps[k], gs[k], ms[k], vs[k], L.LR, b1, b2, L.EPS, 0.0, t, cb, 0.25, round_scalars=False)
            assert abs(R.f32(L.LR) * c - adamw_step_size(R.f32(L.LR), R.f32(b1), R.f32(b2), t, cb)) <= 1e-18
            assert torch.allclose(ref["p"][k], a[0], rtol=1e-15, atol=0.0)
            assert torch.equal(ref["m"][k], a[1]) and torch.equal(ref["v"][k], a[2])


def test_the_rules_branches():
    ps, gs, ms, vs = _inputs()
    c = L.correction(*L.BETAS, 7)
    run = lambda p=ps, g=gs, m=ms, v=vs, **kw: L.lamb_ref64(p, g, m, v, L.LR, L.BETAS, L.EPS, kw.pop("wd", L.WD), c, **kw)
    # an all-zero tensor: r = 1, and it moves (by lr u)
    zeros = [torch.zeros_like(p) for p in ps]
    z = run(p=zeros)
    assert z["r"] == [1.0] * len(ps) and all(bool((q != 0).all()) for q in z["p"] if q.numel())
    # zero gradients, zero moments, wd = 0: u = 0, r = 1, p unchanged
    n = run(g=zeros, m=zeros, v=zeros, wd=0.0, always_adapt=True)
    assert n["r"] == [1.0] * len(ps) and all(torch.equal(q, p.double()) for q, p in zip(n["p"], ps))
    # the wd = 0 group is not adapted; always_adapt turns it on
    off, on = run(wd=0.0), run(wd=0.0, always_adapt=True)
    assert off["r"] == [1.0] * len(ps)
    for k in (0, 1, 2, 4):
        assert on["r"][k] == on["p_norm"][k] / on["u_norm"][k] != 1.0
        assert torch.equal(on["u"][k], off["u"][k])
    # trust_clip caps r at 1: scaled-up parameters make r > 1
    big = [p * 1e3 for p in ps]
    free, capped = run(p=big, wd=1e-6), run(p=big, wd=1e-6, trust_clip=True)
    assert all(r > 1.0 for k, r in enumerate(free["r"]) if ps[k].numel()) and capped["r"] == [1.0] * len(ps)
    small = run(trust_clip=True)
    assert all(small["r"][k] == run()["r"][k] < 1.0 for k in (2, 4))
    # lr = 0: the moments advance, p stays bit-identical
    z = L.lamb_ref64(ps, gs, ms, vs, 0.0, L.BETAS, L.EPS, L.WD, c)
    assert all(torch.equal(q, p.double()) for q, p in zip(z["p"], ps)) and not torch.equal(z["m"][4], ms[4].double())


def test_scaling_the_gradients_by_k_with_1_over_k_in_the_hyper_block_changes_nothing():
    ps, gs, ms, vs = _inputs()
    c = L.correction(*L.BETAS, 7)
    a = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c, 1.0)
    b = L.lamb_ref64(ps, [g * 1024.0 for g in gs], ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c, 1.0 / 1024.0)      # a power of two: exact
    for k in range(len(ps)):
        assert a["r"][k] == b["r"][k]
        assert all(torch.equal(a[key][k], b[key][k]) for key in ("p", "m", "v"))


# ---------------------------------------------------------------------------------------------------------------- the bounds
def _fp32_restatement(ps, gs, ms, vs, lr, betas, eps, wd, c, grad_scale, ratios):
    """The kernels' expressions in fp32 torch arithmetic (un-fused: at least as many roundings as the kernels), c = step_size / lr
    from the fp32 step size, the ratio taken from the reference."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    lr32, b1, b2 = f(lr), f(betas[0]), f(betas[1])
    c32 = (lr32.double() * c).float() / lr32
    out = []
    for p, g, m, v, r in zip(ps, gs, ms, vs, ratios):
        ge = g * f(grad_scale)
        m2 = m * b1 + (f(1.0) - b1) * ge
        v2 = v * b2 + (f(1.0) - b2) * ge * ge
        u = c32 * (m2 / (v2.sqrt() + f(eps))) + f(wd) * p
        out.append((p - (lr32 * f(r)) * u, m2, v2))
    return out


@pytest.mark.parametrize("step,grad_scale", [(1, 1.0), (1000, 1.0 / 1024)])
def test_fp32_restatement_stays_inside_the_bounds_on_the_gpu_tests_inputs(step, grad_scale):
    worst = [0.0, 0.0, 0.0]
    for which in L.CASES:
        ps, gs, ms, vs = L.case_inputs(which, step, grad_scale)
        c = L.correction(*L.BETAS, step)
        ref = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c, grad_scale)
        got = _fp32_restatement(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c, grad_scale, ref["r"])
        for k, (p2, m2, v2) in enumerate(got):
            w = L.check_lamb(p2, m2, v2, ref, k, ps[k], ms[k], L.LR, c, what="%s tensor %d" % (which, k))
            worst = [max(a, b) for a, b in zip(worst, w)]
    print("step %d: largest err / bound of p, m, v: %.3f %.3f %.3f" % (step, *worst))
    assert max(worst) <= 1.0


def test_the_bound_sees_one_element_off_and_a_ratio_off():
    ps, gs, ms, vs = L.case_inputs("boundaries")
    c = L.correction(*L.BETAS, 1000)
    ref = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c)
    k = max(range(len(ps)), key=lambda i: ps[i].numel())
    good = (ref["p"][k].float(), ref["m"][k].float(), ref["v"][k].float())
    L.check_lamb(*good, ref, k, ps[k], ms[k], L.LR, c)
    i = 40000
    bad = good[0].clone()
    bad[i] = float(ref["p"][k][i] + 2.0 * (L.K_P * L.U * (abs(float(ps[k][i])) + abs(float(ref["delta"][k][i]))) + L.RHO * abs(float(ref["delta"][k][i]))))
    with pytest.raises(AssertionError, match=r"p\[40000 of"):
        L.check_lamb(bad, good[1], good[2], ref, k, ps[k], ms[k], L.LR, c)
    # a trust ratio off by 2 RHO moves every element by 2 RHO |D|: outside the parameter bound wherever |D| dominates, and check_ratio
    L.check_ratio(R.f32(ref["r"][k]), ref["r"][k])
    with pytest.raises(AssertionError):
        L.check_ratio(ref["r"][k] * (1.0 + 2.0 * L.RHO), ref["r"][k])
    assert L.N_ADD == 74 and L.RHO == 74 * 2.0 ** -24 and L.K_P == 20


def test_constants_and_header():
    from egovlp_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "egovlp_hip.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in LAMB_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, nc), name
        assert name in _lib.PROTOTYPES
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", txt).group(1)) == 6 == _lib.ABI_VERSION
    assert "lamb.hip" in open(os.path.join(ROOT, "egovlp_amd", "csrc", "Makefile")).read()
    consts = R.source_constants("lamb.hip")
    assert consts == {"LAMB_MAX_T": L.TABLE, "LAMB_RATIO_MAX_T": L.RATIO_TABLE, "CHUNK": L.CHUNK}
    assert ops.LAMB_CHUNK == L.CHUNK == R.source_constants("adamw.hip")["CHUNK"]


# ---------------------------------------------------------------------------------------------------------------- the host side
def _five(scale=1.0):
    g = torch.Generator().manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (3, 70, 64, 65, 4)]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * scale
    return params


def _two_groups(ps):
    return [{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 0.0}]


# What AdamW.step() enqueued at the parent commit of LAMB (recorded there with this file's scenarios): first and second step of one
# group; two groups.  egv_grad_sqnorm_parts is the size query of a first clipped step.
ADAMW_PARENT = {
    ("plain", 1): [["egv_adamw_multi"]] * 2,
    ("scaler", 1): [["egv_grad_nonfinite_multi", "egv_loss_scale_update", "egv_adamw_multi"]] * 2,
    ("clip", 1): [["egv_grad_sqnorm_parts", "egv_grad_sqnorm_multi", "egv_grad_clip_update", "egv_adamw_multi"],
                  ["egv_grad_sqnorm_multi", "egv_grad_clip_update", "egv_adamw_multi"]],
    ("clip+scaler", 1): [["egv_grad_sqnorm_parts", "egv_grad_sqnorm_multi", "egv_loss_scale_update", "egv_grad_clip_update", "egv_adamw_multi"],
                         ["egv_grad_sqnorm_multi", "egv_loss_scale_update", "egv_grad_clip_update", "egv_adamw_multi"]],
    ("plain", 2): [["egv_adamw_multi"] * 2] * 2,
    ("scaler", 2): [["egv_grad_nonfinite_multi", "egv_loss_scale_update", "egv_adamw_multi", "egv_loss_scale_update", "egv_adamw_multi"]] * 2,
    ("clip", 2): [["egv_grad_sqnorm_parts", "egv_grad_sqnorm_multi", "egv_grad_clip_update", "egv_adamw_multi", "egv_adamw_multi"],
                  ["egv_grad_sqnorm_multi", "egv_grad_clip_update", "egv_adamw_multi", "egv_adamw_multi"]],
    ("clip+scaler", 2): [["egv_grad_sqnorm_parts", "egv_grad_sqnorm_multi", "egv_loss_scale_update", "egv_loss_scale_update",
                          "egv_grad_clip_update", "egv_adamw_multi", "egv_adamw_multi"],
                         ["egv_grad_sqnorm_multi", "egv_loss_scale_update", "egv_loss_scale_update", "egv_grad_clip_update",
                          "egv_adamw_multi", "egv_adamw_multi"]],
}


def _two_steps(cls, variant, groups, calls, **kw):
    from egovlp_amd.optim import LossScaler
    ps = _five()
    opt = cls(_two_groups(ps) if groups == 2 else ps, lr=1e-3, max_grad_norm=1.0 if "clip" in variant else None, **kw)
    sc = LossScaler(init_scale=4.0, device="cpu") if "scaler" in variant else None
    out = []
    for _ in range(2):
        del calls[:]
        opt.step(scaler=sc) if sc is not None else opt.step()
        out.append(list(calls))
    return out, opt


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "scaler", "clip", "clip+scaler"])
def test_adamw_enqueues_what_it_enqueued_and_lamb_swaps_only_the_update(variant, groups):
    from egovlp_amd.optim import LAMB, AdamW
    with mock_hip() as calls:
        adamw, _ = _two_steps(AdamW, variant, groups, calls)
        lamb, opt = _two_steps(LAMB, variant, groups, calls)
    assert adamw == ADAMW_PARENT[(variant, groups)]
    for a, l in zip(adamw, lamb):
        l = [c for c in l if c != "egv_lamb_parts"]                                  # a size query on the host, not a launch
        assert "egv_adamw_multi" not in l
        want = []
        for c in a:
            want += THREE if c == "egv_adamw_multi" else [c]
        assert l == want
    # the steady state asks for no sizes and builds no tables
    assert "egv_lamb_parts" not in lamb[1]
    assert opt.trust_ratios().tolist() == [1.0] * 5                                  # the dry run computes nothing: the initial ones


def test_lamb_host_side():
    import egovlp_amd.optim as module_optim
    from egovlp_amd.optim import LAMB, AdamW
    assert issubclass(LAMB, AdamW) and getattr(module_optim, "LAMB") is LAMB         # what `"optimizer": {"type": "LAMB"}` resolves to
    with mock_hip() as calls:
        ps = _five()
        opt = LAMB(_two_groups(ps), lr=2e-3, trust_clip=True)
        # timm's defaults; the two switches are group defaults and travel with the groups
        assert opt.defaults["weight_decay"] == 0.01 and opt.defaults["eps"] == 1e-6 and opt.max_grad_norm == 1.0
        assert [g["trust_clip"] for g in opt.param_groups] == [True, True] and [g["always_adapt"] for g in opt.param_groups] == [False, False]
        assert opt.trust_ratios() is None and opt.skip_flag() is None
        opt.step()
        assert opt.skip_flag() is not None and opt._lamb_partials.numel() == 2 * 5 and opt._lamb_ratios.numel() == 5
        buf = opt._lamb_partials
        opt.step()
        assert opt._lamb_partials is buf                                            # sized once ...
        ps[1].grad = None
        opt.step()
        assert opt._lamb_partials is not buf and opt._lamb_ratios.numel() == 4      # ... re-sized when the gradient list changes
        sd = opt.state_dict()
        assert sd["param_groups"][0]["trust_clip"] is True and sd["param_groups"][1]["always_adapt"] is False and sd["max_grad_norm"] == 1.0
        assert sd["param_groups"][1]["weight_decay"] == 0.0
        other = LAMB(_two_groups(_five()), lr=1.0, always_adapt=True)
        other.load_state_dict(sd)
        assert other.param_groups[0]["lr"] == 2e-3 and other.param_groups[0]["trust_clip"] is True
        assert other.param_groups[0]["always_adapt"] is False
        assert other.state_dict()["state"][0]["step"] == 3 and other.state_dict()["state"][1]["step"] == 2
        del calls[:]
        other.step()
        # parameter 1 sits at step 2, its neighbours at 3 -> three launch groups in the first parameter group, one in the second,
        # each with its own three calls
        assert [c for c in calls if c in THREE] == THREE * 4
        # the wrapper survives a size query that answers 0 and refuses buffers that are too small
        from egovlp_amd import ops
        big = [torch.zeros(2 * L.CHUNK + 1)]
        assert ops.lamb_parts(big) == 3 and ops.lamb_parts([]) == 0
        with pytest.raises(ValueError):
            ops.lamb_multi(big, big, big, big, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1, True, 1.0, torch.zeros(4), torch.zeros(1), True, False)
        with pytest.raises(ValueError):
            ops.lamb_multi(big, big, big, big, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1, True, 1.0, torch.zeros(6), torch.zeros(0), True, False)
