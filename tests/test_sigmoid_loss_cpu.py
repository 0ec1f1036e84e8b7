"""The pairwise sigmoid head, the part that needs no GPU: the closed-form gradients against fp64 autograd, the kernels' tile scheme
restated in torch (tests/sigmoid_ref.py) against the oracle, the m = I case against an independently written SigLIP loss, finite
results at the ends of the parameter range, and the module surface of SigmoidLoss / EgoSigmoidLoss: parameters, state_dict, optimizer
group, clamp, config entry, routing (on the do-nothing library of tests/mock_hip.py) and the CPU-tensor error."""
import math
import os
import re

import pytest
import torch

import sigmoid_ref as S
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("egv_sigmoid_head_fwd_bwd", "egv_sigmoid_head_work_floats", "egv_sigmoid_from_sim")
PARAMS = ((S.LN10, -10.0), (S.LN20, -3.0))
# (use_noun, use_verb) as the kernels take them; "identity": no noun / verb vectors
MODES = {"ego": (True, True), "noun": (True, False), "verb": (False, True), "identity": None}

_ORACLE = {}


def _case(n, mode, D=64):
    text, video, noun, verb = S.make_inputs(n, D, seed=n)
    if mode == "identity":
        return text, video, None, None, True, True
    return (text, video, noun, verb) + MODES[mode]


def _oracle(n, mode, s, b, D=64):
    key = (n, mode, s, b, D)
    if key not in _ORACLE:
        text, video, noun, verb, un, uv = _case(n, mode, D)
        _ORACLE[key] = S.oracle(text, video, noun, verb, s, b, un, uv)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------- formulas
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [1, 5, 65])
def test_closed_form_equals_autograd(n, mode):
    """G = -(t / n) z p, dL/ds = sum G x, dL/db = -(1 / n) sum z p: fp64 autograd through the formulas, to 1e-12"""
    for s, b in PARAMS:
        o = _oracle(n, mode, s, b)
        loss, G, ds, db = S.closed_form(o["x"], o["mask"], s, b)
        assert abs(float(loss) - float(o["loss"])) <= 1e-12 * max(1.0, abs(float(o["loss"])))
        assert float((G - o["G"]).abs().max()) <= 1e-12 * max(float(o["G"].abs().max()), 1e-30)
        assert abs(float(ds) - o["d_scale"]) <= 1e-12 * max(o["abs_scale"], 1e-30)
        assert abs(float(db) - o["d_bias"]) <= 1e-12 * max(o["abs_bias"], 1e-30)


@pytest.mark.parametrize("n", [5, 65])
def test_identity_mask_is_plain_siglip(n):
    """m = I: the loss is -sum log sigmoid(z u) / n, written independently of softplus"""
    for s, b in PARAMS:
        o = _oracle(n, "identity", s, b)
        z = 2.0 * torch.eye(n, dtype=torch.float64) - 1.0
        want = -torch.log(torch.sigmoid(z * (math.exp(s) * o["x"] + b))).sum() / n
        assert abs(float(o["loss"]) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
        assert bool(o["mask"].equal(torch.eye(n, dtype=torch.bool)))


def test_the_mask_modes_differ_on_the_shared_inputs():
    text, video, noun, verb = S.make_inputs(65, 64, seed=65)
    ms = [S.mask_of(65, noun, verb, *MODES[k]) for k in ("ego", "noun", "verb")] + [S.mask_of(65, None, None)]
    assert all(bool(m.diagonal().all()) and bool(m.equal(m.t())) for m in ms)
    assert len({int(m.sum()) for m in ms}) == 4
    assert bool((ms[0] == ((ms[1] & ms[2]) | ms[3])).all())


# ---------------------------------------------------------------------------------------------------------------- tile scheme
def _check_scheme(n, got, o, bar_loss, bar_grad, bar_par):
    assert abs(got["loss"] - float(o["loss"])) <= bar_loss * max(1.0, abs(float(o["loss"])))
    assert S.rel(got["d_text"], o["d_text"]) <= bar_grad and S.rel(got["d_video"], o["d_video"]) <= bar_grad
    for k, a in (("d_scale", "abs_scale"), ("d_bias", "abs_bias")):
        bar = bar_par * (o[a] if o[a] > 10.0 * abs(o[k]) else abs(o[k]))
        assert abs(got[k] - o[k]) <= bar, (n, k, got[k], o[k])


@pytest.mark.parametrize("n", [65, 130, 1030, 1473])
def test_tile_scheme_equals_the_oracle(n):
    """row tiles x column ranges with the padding masked, summed in the fixed order: the oracle to 1e-12 in fp64 and within the bars of
    the GPU tests in fp32"""
    D = 64
    text, video, noun, verb, un, uv = _case(n, "ego", D)
    ntiles = (n + 63) // 64
    for s, b in PARAMS:
        o = _oracle(n, "ego", s, b, D)
        got = S.tile_scheme(text, video, noun, verb, s, b, un, uv)
        assert got["partials"].shape == (3, S.walk_split(ntiles)[1], ntiles)
        _check_scheme(n, got, o, 1e-12, 1e-12, 1e-12)
        got32 = S.tile_scheme(text, video, noun, verb, s, b, un, uv, dtype=torch.float32)
        _check_scheme(n, got32, o, 1e-4, 1e-4, 1e-4)


def test_walk_split_matches_the_sizes_the_gpu_tests_rely_on():
    """up to 23 tiles (1 472 rows) a workgroup walks one column tile; 1 473 rows: 24 tiles in twelve ranges of two, the last tile one row;
    25 tiles: thirteen ranges, the last one short"""
    assert S.walk_split(1) == (1, 1) and S.walk_split(2) == (1, 2) and S.walk_split(17) == (1, 17) and S.walk_split(23) == (1, 23)
    assert S.walk_split(24) == (2, 12)
    tps, ns = S.walk_split(25)
    assert (tps, ns) == (2, 13) and 25 - (ns - 1) * tps == 1
    assert S.walk_split(256) == (128, 2) and S.walk_split(1024) == (1024, 1)


def test_unmasked_padding_is_what_the_padding_test_tells_apart():
    """n = 65, (s, b) = (ln 10, 0): every padded pair left in adds log 2 to the sum -- far outside the loss bar"""
    n = 65
    text, video, noun, verb, un, uv = _case(n, "ego")
    o = S.oracle(text, video, noun, verb, S.LN10, 0.0, un, uv)
    good = S.tile_scheme(text, video, noun, verb, S.LN10, 0.0, un, uv)
    bad = S.tile_scheme(text, video, noun, verb, S.LN10, 0.0, un, uv, mask_padding=False)
    assert abs(good["loss"] - float(o["loss"])) <= 1e-12 * max(1.0, float(o["loss"]))
    padded_pairs = 128 * 128 - n * n
    assert abs((bad["loss"] - good["loss"]) - padded_pairs * math.log(2.0) / n) < 1e-9
    assert abs(bad["loss"] - float(o["loss"])) > 1e-4 * max(1.0, float(o["loss"]))
    assert abs(bad["d_bias"] - o["d_bias"]) > 1e-4 * abs(o["d_bias"])


@pytest.mark.parametrize("b", [50.0, -50.0])
def test_finite_at_the_ends_of_the_range(b):
    """(s, b) = (ln 100, +-50): |u| reaches 150; softplus as max(a, 0) + log1p(exp(-|a|)) stays finite, in fp32 too"""
    n = 65
    text, video, noun, verb, un, uv = _case(n, "ego")
    o = S.oracle(text, video, noun, verb, S.LN100, b, un, uv)
    assert math.isfinite(float(o["loss"])) and bool(torch.isfinite(o["d_text"]).all())
    got = S.tile_scheme(text, video, noun, verb, S.LN100, b, un, uv, dtype=torch.float32)
    assert math.isfinite(got["loss"]) and math.isfinite(got["d_scale"]) and math.isfinite(got["d_bias"])
    assert bool(torch.isfinite(got["d_text"]).all()) and bool(torch.isfinite(got["d_video"]).all())
    assert abs(got["loss"] - float(o["loss"])) < 1e-4 * max(1.0, abs(float(o["loss"])))
    x = torch.tensor([[1.0, -1.0], [-1.0, 1.0]], dtype=torch.float32)
    loss, G, ds, db = S.closed_form(x, torch.eye(2, dtype=torch.bool), S.LN100, b)      # |u| = 150 exactly
    assert all(math.isfinite(float(v)) for v in (loss, ds, db)) and bool(torch.isfinite(G).all())


# ---------------------------------------------------------------------------------------------------------------- modules
def _losses():
    from egovlp_amd.model.loss import EgoSigmoidLoss, SigmoidLoss
    return SigmoidLoss, EgoSigmoidLoss


def test_parameters_and_state_dict():
    for cls in _losses():
        m = cls()
        assert [k for k, _ in m.named_parameters()] == ["logit_scale", "logit_bias"]
        assert list(m.state_dict().keys()) == ["logit_scale", "logit_bias"]
        for p, want in ((m.logit_scale, math.log(10.0)), (m.logit_bias, -10.0)):
            assert p.shape == (1,) and p.dtype == torch.float32 and p.requires_grad
            assert float(p.detach()) == float(torch.tensor(want, dtype=torch.float32))
        assert m.learnable and m.max_logit_scale == math.log(100)
        assert abs(m.current_temperature() - 0.1) < 1e-7 and m.current_bias() == -10.0
        f = cls(logit_scale=1.0, logit_bias=-3.0, learnable=False)
        assert list(f.state_dict().keys()) == ["logit_scale", "logit_bias"]
        assert not f.logit_scale.requires_grad and not f.logit_bias.requires_grad
        assert float(f.logit_scale) == 1.0 and float(f.logit_bias) == -3.0
        f.load_state_dict(m.state_dict())
        assert torch.equal(f.logit_scale, m.logit_scale) and torch.equal(f.logit_bias, m.logit_bias)
    _, Ego = _losses()
    e = Ego(noun=True, verb=False)
    assert (e.noun, e.verb) == (True, False) and Ego.takes_noun_verb and not _losses()[0].takes_noun_verb


def test_register_loss_parameters_adds_one_group_with_both():
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.common import register_loss_parameters
    for cls in _losses():
        model = torch.nn.Linear(4, 4)
        opt = AdamW(model.parameters(), lr=3e-5, weight_decay=0.01)
        loss = cls()
        g = register_loss_parameters(opt, loss, lr=1e-3)
        assert len(opt.param_groups) == 2 and g is opt.param_groups[1]
        assert len(g["params"]) == 2 and g["params"][0] is loss.logit_scale and g["params"][1] is loss.logit_bias
        assert g["weight_decay"] == 0.0 and g["lr"] == 1e-3 and opt.param_groups[0]["weight_decay"] == 0.01
        assert register_loss_parameters(opt, loss) is None and len(opt.param_groups) == 2
        opt2 = AdamW(model.parameters(), lr=3e-5)
        assert register_loss_parameters(opt2, cls(learnable=False)) is None and len(opt2.param_groups) == 1


def test_clamp_reaches_the_scale_and_not_the_bias():
    from egovlp_amd.trainer.common import clamp_loss_scale
    for cls in _losses():
        m = cls()
        for start, want in ((math.log(100) + 1.0, math.log(100)), (-0.5, 0.0), (2.0, 2.0)):
            with torch.no_grad():
                m.logit_scale.fill_(start)
                m.logit_bias.fill_(-77.0)
            clamp_loss_scale(m)
            got = float(m.logit_scale.detach())
            assert got <= math.log(100) and abs(got - want) < 1e-6 and float(m.logit_bias.detach()) == -77.0
        f = cls(logit_scale=9.0, learnable=False)
        clamp_loss_scale(f)
        assert float(f.logit_scale) == 9.0                      # a fixed scale is the caller's


def test_config_entry_resolves(tmp_path):
    import egovlp_amd.model.loss as module_loss
    from egovlp_amd.utils.config import DictConfig
    cfg = {"loss": {"type": "EgoSigmoidLoss", "args": {"logit_scale": 2.0, "logit_bias": -5.0, "noun": True, "verb": False}},
           "trainer": {"save_dir": str(tmp_path)}}
    m = DictConfig(cfg, save_dir=str(tmp_path)).initialize(name="loss", module=module_loss)
    assert type(m).__name__ == "EgoSigmoidLoss" and float(m.logit_scale.detach()) == 2.0 and float(m.logit_bias.detach()) == -5.0 and m.verb is False
    cfg["loss"] = {"type": "SigmoidLoss", "args": {}}
    assert type(DictConfig(cfg, save_dir=str(tmp_path)).initialize(name="loss", module=module_loss)).__name__ == "SigmoidLoss"


def test_fused_and_forward_on_cpu_tensors_raise():
    from egovlp_amd._lib import EgovlpHipError
    Sig, Ego = _losses()
    t, v = torch.randn(4, 8), torch.randn(4, 8)
    with pytest.raises(EgovlpHipError):
        Sig().fused(t, v)
    with pytest.raises(EgovlpHipError):
        Ego().fused(t, v, torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(EgovlpHipError):
        Sig()(torch.randn(4, 4))


# ---------------------------------------------------------------------------------------------------------------- boundary
def test_header_and_binding_declare_the_entry_points():
    import ctypes
    from egovlp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "egovlp_hip.h")).read()
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", txt).group(1)) == 6 and _lib.ABI_VERSION == 6
    nc = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRIES:
        decl = re.search(r"int(?:64_t)?\s+%s\s*\((.*?)\)\s*;" % name, nc, flags=re.S)
        assert decl, name
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == len(decl.group(1).split(","))
        if name != "egv_sigmoid_head_work_floats":
            assert res is ctypes.c_int32
            assert all(w in decl.group(1) for w in ("const float* logit_scale", "const float* logit_bias", "float* d_scale", "float* d_bias"))
    if os.path.exists(_lib.LIB_PATH):
        h = ctypes.CDLL(_lib.LIB_PATH)
        assert all(hasattr(h, name) for name in NEW_ENTRIES)


@pytest.mark.parametrize("n", [64, 1030])
def test_which_c_calls_the_modules_make(n):
    """the sigmoid losses make the sigmoid head's calls, one per step, at any n; EgoNCE and NormSoftmaxLoss keep theirs; the gradients
    reach both parameters with their shapes, and none is asked for with learnable=False"""
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    from egovlp_amd.trainer.common import egoclip_head_loss
    Sig, Ego = _losses()
    t = torch.randn(n, 64, requires_grad=True)
    v = torch.randn(n, 64, requires_grad=True)
    noun, verb = torch.zeros(n, 16), torch.zeros(n, 12)
    with mock_hip() as calls:
        for loss_fn in (Ego(), Sig()):
            egoclip_head_loss(loss_fn, t, v, noun, verb).backward()
            assert calls.count("egv_sigmoid_head_fwd_bwd") == 1 and not any("egonce" in c for c in calls), calls
            assert loss_fn.logit_scale.grad.shape == (1,) and loss_fn.logit_bias.grad.shape == (1,)
            del calls[:]
        fixed = Ego(learnable=False)
        egoclip_head_loss(fixed, t, v, noun, verb).backward()
        assert calls.count("egv_sigmoid_head_fwd_bwd") == 1 and fixed.logit_scale.grad is None and fixed.logit_bias.grad is None
        del calls[:]
        for loss_fn in (EgoNCE(), NormSoftmaxLoss()):
            egoclip_head_loss(loss_fn, t, v, noun, verb).backward()
            assert not any("sigmoid" in c for c in calls) and sum("egonce" in c and "work" not in c for c in calls) == 1, calls
            del calls[:]
        if n <= 64:
            for loss_fn in (Ego(), Sig()):
                egoclip_head_loss(loss_fn, t, v, noun, verb, fused_head=False).backward()
                assert calls.count("egv_sigmoid_from_sim") == 1 and "egv_sigmoid_head_fwd_bwd" not in calls
                assert loss_fn.logit_scale.grad.shape == (1,) and loss_fn.logit_bias.grad.shape == (1,)
                del calls[:]
