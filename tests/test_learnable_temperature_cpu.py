"""Learnable temperature of EgoNCE / NormSoftmaxLoss, the part that needs no GPU: the identity dL/ds = sum G o X the kernels rely on
against fp64 autograd on the oracle, the long head's partial scheme restated in torch, the modules' parameter / state_dict behaviour,
the optimizer group of the loss, the declared entry points and (on the do-nothing library of tests/mock_hip.py) which C calls the
modules make."""
import math
import os
import re

import pytest
import torch

import egonce_long_ref as R
import learnable_temperature_ref as LT
from mock_hip import mock_hip
from oracle import egovlp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("egv_egonce_fwd_bwd_ls", "egv_egonce_long_fwd_bwd_ls", "egv_egonce_from_sim_ls")

# EgoNCE in its three mask modes + NormSoftmaxLoss
KINDS = {"ego": (True, True), "noun": (True, False), "verb": (False, True), "nsl": None}


def _case(n, kind, D=64):
    text, video, noun, verb = R.make_inputs(n, D, seed=n)
    if kind == "nsl":
        return text, video, None, None, True, True
    return (text, video, noun, verb) + KINDS[kind]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [1, 5, 65, 129])
def test_identity_against_fp64_autograd(n, kind):
    """autograd through temperature = exp(-s) (s.requires_grad) gives sum_ij G_ij x_ij, to fp64 round-off"""
    text, video, noun, verb, un, uv = _case(n, kind)
    for tau in (0.05, 1.0):
        o = LT.oracle_scale(O, text, video, noun, verb, tau, un, uv)
        assert abs(o["d_scale"] - o["identity"]) <= 1e-12 * max(o["abs_sum"], 1e-30) + 1e-15, (n, kind, tau, o["d_scale"], o["identity"])
        if n == 1:
            assert o["d_scale"] == 0.0 and o["identity"] == 0.0


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [1, 5, 65, 129])
def test_long_head_partial_scheme(n, kind):
    """one partial per (row tile, column range), rows and columns past n masked: their sum is the oracle's gradient (fp64 restatement:
    1e-10 of sum |G X|; fp32 restatement: the 1e-4 bar of the GPU tests)"""
    text, video, noun, verb, un, uv = _case(n, kind)
    o = LT.oracle_scale(O, text, video, noun, verb, 0.05, un, uv)
    part, total = LT.long_scale_partials(text, video, noun, verb, 0.05, use_noun=un, use_verb=uv)
    ntiles = (n + 63) // 64
    assert part.shape == (LT.grad_split(ntiles)[1], ntiles) and bool(torch.isfinite(part).all())
    assert abs(total - o["d_scale"]) <= 1e-10 * max(o["abs_sum"], 1e-30) + 1e-15, (n, kind, total, o["d_scale"])
    _, total32 = LT.long_scale_partials(text, video, noun, verb, 0.05, use_noun=un, use_verb=uv, dtype=torch.float32)
    if n == 1:
        assert abs(total32) < 1e-6
    else:
        assert abs(total32 - o["d_scale"]) < 1e-4 * abs(o["d_scale"]), (n, kind, total32, o["d_scale"])


def test_grad_split_matches_the_sizes_the_gpu_tests_rely_on():
    """n = 65 is the first size with two column ranges; n = 1025 has nine, the last one short"""
    assert LT.grad_split(1) == (1, 1) and LT.grad_split(2) == (1, 2)
    tps, ns = LT.grad_split(17)
    assert (tps, ns) == (2, 9) and 17 - (ns - 1) * tps == 1


# ---------------------------------------------------------------------------------------------------------------- modules
def _losses():
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    return EgoNCE, NormSoftmaxLoss


def test_off_is_the_module_as_it_was():
    for cls in _losses():
        m = cls()
        assert list(m.parameters()) == [] and len(m.state_dict()) == 0 and not hasattr(m, "logit_scale")
        assert m.learnable_temperature is False and m.temperature == 0.05 and m.current_temperature() == 0.05
        m.clamp_logit_scale_()                                  # nothing to clamp, nothing raised
    EgoNCE, _ = _losses()
    m = EgoNCE(0.07, False, True)                               # the reference's positional order still holds
    assert (m.temperature, m.noun, m.verb) == (0.07, False, True)


@pytest.mark.parametrize("tau", [0.05, 0.01, 1.0])
def test_on_has_one_fp32_parameter_initialised_to_log_inverse_tau(tau):
    for cls in _losses():
        m = cls(temperature=tau, learnable_temperature=True)
        (p,) = list(m.parameters())
        assert p is m.logit_scale and p.shape == (1,) and p.dtype == torch.float32 and p.requires_grad
        assert float(p.detach()) == float(torch.tensor(math.log(1.0 / tau), dtype=torch.float32))
        assert list(m.state_dict().keys()) == ["logit_scale"]
        assert abs(m.current_temperature() - tau) < 1e-6 * tau
        assert m.max_logit_scale == math.log(100)


def test_config_style_construction_and_state_dict_round_trip():
    EgoNCE, NormSoftmaxLoss = _losses()
    args = {"temperature": 0.07, "noun": True, "verb": False, "learnable_temperature": True, "max_logit_scale": 3.0}
    a = EgoNCE(**args)
    assert a.max_logit_scale == 3.0 and a.verb is False
    with torch.no_grad():
        a.logit_scale.fill_(1.2345)
    b = EgoNCE(**args)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.logit_scale, b.logit_scale) and float(b.logit_scale.detach()) == float(torch.tensor(1.2345))
    c = NormSoftmaxLoss(learnable_temperature=True)
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.logit_scale, a.logit_scale)
    with pytest.raises(RuntimeError):
        EgoNCE().load_state_dict(a.state_dict())                # a fixed-temperature module has no such key
    with pytest.raises(ValueError):
        EgoNCE(temperature=0.0, learnable_temperature=True)


def test_clamp_logit_scale():
    for cls in _losses():
        m = cls(learnable_temperature=True)
        for start, want in ((math.log(100) + 1.0, math.log(100)), (-0.5, 0.0), (2.0, 2.0)):
            with torch.no_grad():
                m.logit_scale.fill_(start)
            ptr = m.logit_scale.data_ptr()
            assert m.clamp_logit_scale_() is m
            got = float(m.logit_scale.detach())
            assert got <= math.log(100) and abs(got - want) < 1e-6 and m.logit_scale.data_ptr() == ptr     # <= in fp64: tau >= 0.01
        m = cls(learnable_temperature=True, max_logit_scale=1.0)
        m.clamp_logit_scale_()
        assert float(m.logit_scale.detach()) == 1.0


# ---------------------------------------------------------------------------------------------------------------- optimizer group
def _model_and_opt(lr=3e-5, weight_decay=0.01):
    from egovlp_amd.optim import AdamW
    model = torch.nn.Linear(4, 4)
    return model, AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)


def test_register_loss_parameters():
    from egovlp_amd.trainer.common import register_loss_parameters
    EgoNCE, _ = _losses()
    loss = EgoNCE(learnable_temperature=True)
    _, opt = _model_and_opt()
    g = register_loss_parameters(opt, loss)
    assert len(opt.param_groups) == 2 and g is opt.param_groups[1]
    assert len(g["params"]) == 1 and g["params"][0] is loss.logit_scale
    assert g["weight_decay"] == 0.0 and g["lr"] == 3e-5 and opt.param_groups[0]["weight_decay"] == 0.01
    assert g["betas"] == opt.param_groups[0]["betas"] and g["eps"] == opt.param_groups[0]["eps"]
    # idempotent
    assert register_loss_parameters(opt, loss) is None and len(opt.param_groups) == 2
    # the lr override
    _, opt2 = _model_and_opt()
    g2 = register_loss_parameters(opt2, loss, lr=1e-3)
    assert g2["lr"] == 1e-3 and opt2.param_groups[0]["lr"] == 3e-5
    # already in the optimizer (a caller who built it from model + loss parameters): nothing is added
    from egovlp_amd.optim import AdamW
    model = torch.nn.Linear(4, 4)
    opt3 = AdamW(list(model.parameters()) + list(loss.parameters()), lr=3e-5)
    assert register_loss_parameters(opt3, loss) is None and len(opt3.param_groups) == 1
    # a loss without parameters, and one that is no module
    _, opt4 = _model_and_opt()
    assert register_loss_parameters(opt4, EgoNCE()) is None and register_loss_parameters(opt4, lambda x: x) is None
    assert len(opt4.param_groups) == 1
    # the group survives the optimizer's state_dict
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2 and sd["param_groups"][1]["weight_decay"] == 0.0


def test_lr_schedule_keeps_the_loss_groups_own_rate():
    from types import SimpleNamespace
    from egovlp_amd.trainer.common import TrainerBase, register_loss_parameters
    EgoNCE, _ = _losses()
    args = SimpleNamespace(learning_rate1=3e-5, schedule=[2, 4])
    for lr, want in ((None, [3e-5, 3e-6]), (1e-3, [1e-3, 1e-4])):
        _, opt = _model_and_opt()
        register_loss_parameters(opt, EgoNCE(learnable_temperature=True), lr=lr)
        for epoch, k in ((1, 0), (3, 1)):
            TrainerBase._adjust_learning_rate(None, opt, epoch, args)
            assert abs(opt.param_groups[0]["lr"] - [3e-5, 3e-6][k]) < 1e-12
            assert abs(opt.param_groups[1]["lr"] - want[k]) < 1e-9 * want[k]


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_header_and_binding_declare_the_entry_points():
    import ctypes
    from egovlp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "egovlp_hip.h")).read()
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", txt).group(1)) == 6 and _lib.ABI_VERSION == 6
    nc = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRIES:
        decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, nc, flags=re.S)
        assert decl, name
        assert "const float* logit_scale" in decl.group(1) and "float* d_logit_scale" in decl.group(1) and "temperature" not in decl.group(1)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32 and len(args) == len(decl.group(1).split(","))
    assert "sum_ij G_ij x_ij" in txt and "model/loss.py" in txt
    if os.path.exists(_lib.LIB_PATH):
        h = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(h, name) for name in NEW_ENTRIES)


@pytest.mark.parametrize("n,entry", [(64, "egv_egonce_fwd_bwd"), (1025, "egv_egonce_long_fwd_bwd")])
def test_which_c_calls_the_modules_make(n, entry):
    """fixed temperature: the calls of before, none of the new ones; learnable: the *_ls entry of the same head, and the gradient
    reaches logit_scale with the parameter's shape"""
    EgoNCE, NormSoftmaxLoss = _losses()
    from egovlp_amd.trainer.common import egoclip_head_loss
    t = torch.randn(n, 64, requires_grad=True)
    v = torch.randn(n, 64, requires_grad=True)
    noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
    with mock_hip() as calls:
        egoclip_head_loss(EgoNCE(), t, v, noun, verb).backward()
        assert calls.count(entry) == 1 and not any(c.endswith("_ls") for c in calls)
        del calls[:]
        for loss_fn, extra in ((EgoNCE(learnable_temperature=True), (noun, verb)), (NormSoftmaxLoss(learnable_temperature=True), (None, None))):
            egoclip_head_loss(loss_fn, t, v, *extra).backward()
            assert calls.count(entry + "_ls") == 1 and entry not in calls, calls
            assert loss_fn.logit_scale.grad.shape == (1,)
            del calls[:]
        if n <= 64:
            loss_fn = EgoNCE(learnable_temperature=True)
            egoclip_head_loss(loss_fn, t, v, noun, verb, fused_head=False).backward()
            assert calls.count("egv_egonce_from_sim_ls") == 1 and "egv_egonce_from_sim" not in calls
            assert loss_fn.logit_scale.grad.shape == (1,)


def test_steps_clamp_only_a_learnable_loss():
    from egovlp_amd.trainer.common import clamp_loss_scale
    EgoNCE, _ = _losses()
    clamp_loss_scale(EgoNCE())
    clamp_loss_scale(object())
    m = EgoNCE(learnable_temperature=True)
    with torch.no_grad():
        m.logit_scale.fill_(9.0)
    clamp_loss_scale(m)
    assert math.log(100) - 1e-6 < float(m.logit_scale.detach()) <= math.log(100)
