"""Learnable temperature of EgoNCE / NormSoftmaxLoss on a real MI355X (`pytest -m gpu`): the *_ls entry points of the short, the long
and the from-sim head against the fp64 oracle with autograd through temperature = exp(-s) (tests/learnable_temperature_ref.py), at
the smallest sizes at which the reduction of dL/ds can go wrong; then the autograd nodes, the 1 / W convention, whole steps (plain,
fp16 backward, cached), the trainer's optimizer group and checkpoints, and that the fixed-temperature calls are untouched.

Bars.  Loss < 1e-4 max(1, |ref|) and embedding gradients rel-L2 < 1e-4: the bars of tests/test_gpu_egonce_long.py.  d_logit_scale:
|got - ref| < 1e-4 |ref| at tau in {0.05, 0.01}; at tau = 1.0, where sum G X cancels up to 240-fold, |got - ref| < 1e-4 sum |G X| of
the oracle; at n = 1, |got| < 1e-6.  Measured values: DESIGN 4.5a."""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import egonce_long_ref as R  # noqa: E402
import learnable_temperature_ref as LT  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

LOSS_BAR = 1e-4
GRAD_BAR = 1e-4
SCALE_BAR = 1e-4
TAUS = (0.05, 0.01, 1.0)
KINDS = {"ego": (True, True), "noun": (True, False), "verb": (False, True), "nsl": None}


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import loss_ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


_INPUTS, _ORACLE = {}, {}


def inputs(n, D):
    if (n, D) not in _INPUTS:
        _INPUTS[(n, D)] = R.make_inputs(n, D, seed=n + D)
    return _INPUTS[(n, D)]


def oracle(n, D, kind, tau):
    """fp64 oracle on the shared inputs, computed once per case and never modified"""
    key = (n, D, kind, tau)
    if key not in _ORACLE:
        text, video, noun, verb = inputs(n, D)
        if kind == "nsl":
            o = LT.oracle_scale(O, text, video, None, None, tau)
        else:
            o = LT.oracle_scale(O, text, video, noun, verb, tau, *KINDS[kind])
        o.pop("G")
        _ORACLE[key] = o
    return _ORACLE[key]


def scale_of(tau):
    return torch.tensor([math.log(1.0 / tau)], dtype=torch.float32, device="cuda")


def head_args(n, D, kind):
    text, video, noun, verb = (t.cuda() for t in inputs(n, D))
    if kind == "nsl":
        return text, video, None, None, dict(use_noun=True, use_verb=True)
    un, uv = KINDS[kind]
    return text, video, noun, verb, dict(use_noun=un, use_verb=uv or not un)      # as EgoNCE.fused maps noun = verb = False


def check_head(tag, n, got, o, tau):
    """got = (loss, d_text, d_video, d_logit_scale) of a head call; prints every figure before it asserts"""
    loss, dt, dv, dls = float(got[0]), got[1].cpu(), got[2].cpu(), float(got[3])
    rl = float(o["loss"])
    el, et, ev = abs(loss - rl), R.rel(dt, o["d_text"]), R.rel(dv, o["d_video"])
    ref = o["d_scale"]
    es = abs(dls - ref)
    canc = o["abs_sum"] / max(abs(ref), 1e-300)
    print("%s: loss |diff| %.2e (bar %.1e) d_text rel %.2e d_video rel %.2e (bar %.1e); d_logit_scale %.8e oracle %.8e |diff| %.2e "
          "= %.2e |ref| = %.2e sum|GX| (cancellation %.1f)" % (tag, el, LOSS_BAR * max(1.0, abs(rl)), et, ev, GRAD_BAR, dls, ref, es,
                                                                es / max(abs(ref), 1e-300), es / max(o["abs_sum"], 1e-300), canc))
    assert el < LOSS_BAR * max(1.0, abs(rl)), (tag, el)
    # n = 1, or every row matches every row (n = 2 with a shared noun): P = Z bit for bit, the loss and every gradient are exactly 0 and
    # the oracle's are fp64 round-off -- there is nothing to be relative to
    if n == 1 or (o["abs_sum"] < 1e-12 and float(o["d_text"].abs().max()) < 1e-12):
        assert float(dt.abs().max()) < 1e-6 and float(dv.abs().max()) < 1e-6 and abs(dls) < 1e-6, (tag, dls)
        return
    assert et < GRAD_BAR and ev < GRAD_BAR, (tag, et, ev)
    if tau == 1.0:
        assert es < SCALE_BAR * o["abs_sum"], (tag, es, o["abs_sum"])
    else:
        assert es < SCALE_BAR * abs(ref), (tag, es, ref)


# ------------------------------------------------------------------------------------------------------------ the heads
# 63 .. 65: one wave / one tile; 255 .. 257: the 256-thread row stride of the grad kernel; 300: a ragged size
@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 255, 256, 257, 300])
def test_short_head_matches_the_oracle(ops, n, D):
    for kind in KINDS:
        text, video, noun, verb, kw = head_args(n, D, kind)
        for tau in TAUS:
            loss, sim, dt, dv, dls = ops.egonce_fwd_bwd(text, video, noun, verb, None, logit_scale=scale_of(tau), **kw)
            assert sim is None and dls.shape == (1,)
            check_head("short n=%d D=%d %s tau=%g" % (n, D, kind, tau), n, (loss, dt, dv, dls), oracle(n, D, kind, tau), tau)


# 65: the first size with two column ranges; 1025: nine ranges, the last one short, and padded rows
@pytest.mark.parametrize("n,D", [(1, 256), (63, 256), (64, 256), (65, 256), (129, 256), (1025, 256), (65, 64)])
def test_long_head_matches_the_oracle(ops, n, D):
    for kind in KINDS:
        text, video, noun, verb, kw = head_args(n, D, kind)
        for tau in TAUS:
            got = ops.egonce_long_fwd_bwd(text, video, noun, verb, None, logit_scale=scale_of(tau), **kw)
            assert len(got) == 4 and got[3].shape == (1,)
            check_head("long n=%d D=%d %s tau=%g" % (n, D, kind, tau), n, got, oracle(n, D, kind, tau), tau)


def test_long_and_short_head_agree(ops):
    n, D = 300, 256
    for kind in KINDS:
        text, video, noun, verb, kw = head_args(n, D, kind)
        for tau in TAUS:
            o = oracle(n, D, kind, tau)
            s = float(ops.egonce_fwd_bwd(text, video, noun, verb, None, logit_scale=scale_of(tau), **kw)[4])
            g = float(ops.egonce_long_fwd_bwd(text, video, noun, verb, None, logit_scale=scale_of(tau), **kw)[3])
            bar = SCALE_BAR * (o["abs_sum"] if tau == 1.0 else abs(o["d_scale"]))
            print("n=300 %s tau=%g: short %.8e long %.8e |diff| %.2e (bar %.2e)" % (kind, tau, s, g, abs(s - g), bar))
            assert abs(s - g) < bar, (kind, tau, s, g)


def test_routing_past_the_short_heads_cap(ops):
    n, D = 1025, 256
    text, video, noun, verb, kw = head_args(n, D, "ego")
    s = scale_of(0.05)
    a = ops.egonce_fwd_bwd(text, video, noun, verb, None, logit_scale=s, **kw)
    b = ops.egonce_long_fwd_bwd(text, video, noun, verb, None, logit_scale=s, **kw)
    torch.cuda.synchronize()
    assert len(a) == 5 and a[1] is None
    assert torch.equal(a[4], b[3]) and torch.equal(a[0], b[0]) and torch.equal(a[2], b[1]) and torch.equal(a[3], b[2])
    with pytest.raises(ValueError):
        ops.egonce_fwd_bwd(text, video, noun, verb, None, logit_scale=s, want_sim=True, **kw)


@pytest.mark.parametrize("n", [65, 300])
def test_from_sim_path_gives_the_fused_gradient(ops, n):
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    from egovlp_amd.model.model import sim_matrix
    D = 256
    text, video, noun, verb = (t.cuda() for t in inputs(n, D))
    for kind, tau in (("ego", 0.05), ("noun", 0.01), ("nsl", 0.05), ("ego", 1.0)):
        o = oracle(n, D, kind, tau)
        res = []
        for fused in (True, False):
            loss_fn = (NormSoftmaxLoss(temperature=tau, learnable_temperature=True) if kind == "nsl" else
                       EgoNCE(tau, *KINDS[kind], learnable_temperature=True)).cuda()
            tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
            if kind == "nsl":
                loss = loss_fn.fused(tc, vc) if fused else loss_fn(sim_matrix(tc, vc))
            else:
                loss = loss_fn.fused(tc, vc, noun, verb) if fused else loss_fn(sim_matrix(tc, vc), sim_matrix(verb, verb), sim_matrix(noun, noun))
            loss.backward()
            assert loss_fn.logit_scale.grad.shape == (1,)
            res.append((loss.detach(), tc.grad, vc.grad, loss_fn.logit_scale.grad))
        check_head("from-sim n=%d %s tau=%g" % (n, kind, tau), n, res[1], o, tau)
        bar = SCALE_BAR * (o["abs_sum"] if tau == 1.0 else abs(o["d_scale"]))
        assert abs(float(res[0][3]) - float(res[1][3])) < bar


def test_loss_only_when_no_gradients_are_asked_for(ops):
    for n, fn in ((65, ops.egonce_fwd_bwd), (1025, ops.egonce_fwd_bwd), (65, ops.egonce_long_fwd_bwd)):
        text, video, noun, verb, kw = head_args(n, 256, "ego")
        out = fn(text, video, noun, verb, None, logit_scale=scale_of(0.05), want_grads=False, **kw)
        assert all(x is None for x in out[1:])
        assert abs(float(out[0]) - float(oracle(n, 256, "ego", 0.05)["loss"])) < LOSS_BAR * max(1.0, float(oracle(n, 256, "ego", 0.05)["loss"]))
    from egovlp_amd import loss_ops
    from egovlp_amd.model.model import sim_matrix
    text, video, _, _, _ = head_args(65, 256, "nsl")
    loss, dx, dls = loss_ops.egonce_from_sim(sim_matrix(text, video), None, None, None, True, True, want_grad=False, logit_scale=scale_of(0.05))
    assert dx is None and dls is None and abs(float(loss) - float(oracle(65, 256, "nsl", 0.05)["loss"])) < LOSS_BAR * 10


def test_two_calls_are_bit_identical(ops):
    for n, fn in ((300, ops.egonce_fwd_bwd), (1025, ops.egonce_long_fwd_bwd), (129, ops.egonce_long_fwd_bwd)):
        text, video, noun, verb, kw = head_args(n, 256, "ego")
        s = scale_of(0.05)
        a = fn(text, video, noun, verb, None, logit_scale=s, **kw)
        b = fn(text, video, noun, verb, None, logit_scale=s, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a[-1], b[-1]) and torch.equal(a[0], b[0])
        assert all(torch.equal(x, y) for x, y in zip(a, b) if x is not None)


def test_fixed_temperature_calls_are_untouched(ops):
    """the fixed-temperature call before and after a learnable call in the same process: bit-identical (no workspace state leaks), and
    the learnable call at s = log(1 / tau) reproduces its loss to the rounding of exp(s)"""
    for n, fixed, learn in ((300, ops.egonce_fwd_bwd, ops.egonce_fwd_bwd), (1025, ops.egonce_long_fwd_bwd, ops.egonce_long_fwd_bwd)):
        text, video, noun, verb, kw = head_args(n, 256, "ego")
        before = fixed(text, video, noun, verb, 0.05, **kw)
        mid = learn(text, video, noun, verb, None, logit_scale=scale_of(0.05), **kw)
        after = fixed(text, video, noun, verb, 0.05, **kw)
        torch.cuda.synchronize()
        assert len(before) == len(mid) - 1
        assert all(torch.equal(x, y) for x, y in zip(before, after) if x is not None)
        assert abs(float(mid[0]) - float(before[0])) < LOSS_BAR


def test_bad_arguments_are_refused(ops):
    import ctypes
    from egovlp_amd import _lib
    h = _lib.lib()
    t = torch.ones(64, 8).cuda()
    w = torch.zeros(1 << 16).cuda()
    out, s = torch.zeros(1).cuda(), scale_of(0.05)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    g = torch.zeros(64, 8).cuda()
    # no scale pointer; gradients without a place for the scale's; the long head's scale gradient needs d_text
    assert h.egv_egonce_fwd_bwd_ls(p(t), p(t), None, None, 8, 8, 0, 0, None, 1e-8, 1, 1, p(out), None, None, None, None, p(w), None) == 1
    assert h.egv_egonce_fwd_bwd_ls(p(t), p(t), None, None, 8, 8, 0, 0, p(s), 1e-8, 1, 1, p(out), None, p(g), None, None, p(w), None) == 1
    assert h.egv_egonce_long_fwd_bwd_ls(p(t), p(t), None, None, 8, 8, 0, 0, None, 1e-8, 1, 1, p(out), None, None, None, p(w), None) == 1
    assert h.egv_egonce_long_fwd_bwd_ls(p(t), p(t), None, None, 8, 8, 0, 0, p(s), 1e-8, 1, 1, p(out), None, p(g), p(out), p(w), None) == 1
    assert h.egv_egonce_from_sim_ls(p(t), None, None, 8, None, 1, 1, p(out), None, None, p(w), None) == 1
    assert h.egv_egonce_from_sim_ls(p(t), None, None, 8, p(s), 1, 1, p(out), p(g), None, p(w), None) == 1
    assert h.egv_egonce_long_fwd_bwd_ls(p(t), p(t), None, None, 8, 8, 0, 0, p(s), 1e-8, 1, 1, p(out), None, None, None, p(w), None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.egonce_fwd_bwd(t, t, None, None, None, logit_scale=torch.zeros(2).cuda())
    with pytest.raises(ValueError):
        ops.egonce_fwd_bwd(t, t, None, None, None, logit_scale=torch.zeros(1))


# ------------------------------------------------------------------------------------------------------------ autograd nodes
def _fused_backward(n, factor=1.0):
    from egovlp_amd.model.loss import EgoNCE
    text, video, noun, verb = (t.cuda() for t in inputs(n, 256))
    loss_fn = EgoNCE(learnable_temperature=True).cuda()
    tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
    loss = loss_fn.fused(tc, vc, noun, verb)
    (loss if factor == 1.0 else factor * loss).backward()
    return loss.detach(), tc.grad, vc.grad, loss_fn.logit_scale.grad


@pytest.mark.parametrize("n", [300, 1025])
def test_upstream_factor(n):
    plain, tripled = _fused_backward(n), _fused_backward(n, 3.0)
    torch.cuda.synchronize()
    assert torch.equal(tripled[3], 3.0 * plain[3])
    assert torch.equal(tripled[1], 3.0 * plain[1]) and torch.equal(tripled[2], 3.0 * plain[2])
    check_head("EgoNCE.fused n=%d upstream 3.0" % n, n, (plain[0], tripled[1] / 3.0, tripled[2] / 3.0, tripled[3] / 3.0),
               oracle(n, 256, "ego", 0.05), 0.05)


def test_gradient_is_stored_over_the_world_size(monkeypatch):
    from egovlp_amd import gather
    one = _fused_backward(300)
    monkeypatch.setattr(gather, "_world", lambda: 2)
    two = _fused_backward(300)
    torch.cuda.synchronize()
    assert torch.equal(two[3], one[3] / 2.0) and float(one[3]) != 0.0
    assert torch.equal(two[1], one[1]) and torch.equal(two[2], one[2])            # the embedding gradients go through the gather's backward


# ------------------------------------------------------------------------------------------------------------ whole steps
@pytest.fixture(scope="module")
def full():
    """the model and batch configuration of tests/test_gpu_cached_step.py"""
    import test_gpu_cached_step as CS
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m, sd = CS.build_full()
    from egovlp_amd.synth import synth_batch
    dev = CS.to_dev(synth_batch(8, T=4, L=32, seed=4321, ragged=True))
    yield CS, m, sd, dev
    Precision.set("bf16x3")


def _step(full, mode, start=None, scale_lr=1e-3, chunk=None, max_grad_norm=None, params=None):
    """one EgoClip step with a learnable EgoNCE; the model's learning rate is 0 -> (loss_fn, optimizer, s before, S)"""
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached, register_loss_parameters
    CS, m, sd, dev = full
    CS._set_mode(mode)
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    for p in m.parameters():
        p.grad = None
    loss_fn = EgoNCE(learnable_temperature=True).cuda()
    if start is not None:
        with torch.no_grad():
            loss_fn.logit_scale.fill_(start)
    opt = AdamW(m.parameters() if params is None else params(m), lr=0.0, max_grad_norm=max_grad_norm)
    assert register_loss_parameters(opt, loss_fn, lr=scale_lr) is not None
    s0 = float(loss_fn.logit_scale.detach())
    ec = m.exec_ctx
    S = ec.loss_scaler(device="cuda").get_scale() if ec.bwd_passes == 4 else 1.0
    if chunk is None:
        loss = egoclip_step(m, loss_fn, opt, dev)
    else:
        loss = egoclip_step_cached(m, loss_fn, opt, dev, chunk)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return loss_fn, opt, s0, S


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix"])
def test_a_whole_step_moves_the_scale_by_adams_first_step(full, mode):
    from egovlp_amd.optim import adamw_step_size
    lr = 1e-3
    try:
        loss_fn, opt, s0, S = _step(full, mode, scale_lr=lr)
        g = float(loss_fn.logit_scale.grad) / S
        s1 = float(loss_fn.logit_scale.detach())
        # Adam's first step with bias correction: -step_size (1 - b1) g / (sqrt((1 - b2) g^2) + eps) = -lr sign(g) up to eps
        b1, b2 = opt.param_groups[1]["betas"]
        want = -adamw_step_size(lr, b1, b2, 1) * (1.0 - b1) * g / (math.sqrt((1.0 - b2) * g * g) + opt.param_groups[1]["eps"])
        print("%s: dL/ds %.6e (loss scale %g), s0 %.7f s1 %.7f step %.6e, -lr sign %.6e, Adam's %.6e" % (
            mode, g, S, s0, s1, s1 - s0, -lr * math.copysign(1.0, g), want))
        assert abs(g) > 1e-3                                       # far above eps / sqrt(1 - b2): the step is lr sign(g)
        assert abs((s1 - s0) - (-lr * math.copysign(1.0, g))) < 0.01 * lr
        assert abs((s1 - s0) - want) < 0.01 * lr
        assert 0.0 <= s1 <= math.log(100)
    finally:
        full[0]._set_mode("bf16x3")


def test_a_step_started_past_the_cap_ends_clamped(full):
    loss_fn, _, s0, _ = _step(full, "bf16x3", start=math.log(100) + 1.0)
    s1 = float(loss_fn.logit_scale.detach())
    print("clamp: s0 %.6f s1 %.6f (ln 100 = %.6f)" % (s0, s1, math.log(100)))
    assert s0 > math.log(100) and s1 <= math.log(100)


def test_grad_norm_includes_the_scales_gradient(full):
    """the optimizer holds ONE small model parameter and the scale, so the scale's share of the norm is not lost in rounding"""
    name = "vid_proj.0.bias"
    loss_fn, opt, _, _ = _step(full, "bf16x3", max_grad_norm=1e9, params=lambda m: [dict(m.named_parameters())[name]])
    g_model = dict(full[1].named_parameters())[name].grad.double().norm()
    g_scale = loss_fn.logit_scale.grad.double().norm()
    want = float((g_model ** 2 + g_scale ** 2).sqrt())
    got = opt.grad_norm()
    print("grad_norm %.6e; model part %.6e scale part %.6e; both %.6e" % (got, float(g_model), float(g_scale), want))
    assert abs(got - want) < 1e-5 * want
    assert abs(got - float(g_model)) > 1e-3 * want                # the bar tells "with" from "without" the scale


def test_cached_step_gives_the_plain_steps_scale_gradient(full):
    CS = full[0]
    plain, _, _, _ = _step(full, "bf16x3", scale_lr=0.0)
    cached, _, _, _ = _step(full, "bf16x3", scale_lr=0.0, chunk=2)
    r = CS.rel(cached.logit_scale.grad, plain.logit_scale.grad)
    print("logit_scale.grad plain %.7e cached %.7e rel %.2e (bar %.0e)" % (float(plain.logit_scale.grad), float(cached.logit_scale.grad), r,
                                                                            2 * CS.GRAD_BAR["bf16x3"]))
    assert float(plain.logit_scale.grad) != 0.0 and r <= 2 * CS.GRAD_BAR["bf16x3"]


# ------------------------------------------------------------------------------------------------------------ trainer
TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
CFG = {"name": "EgoClip_tiny", "n_gpu": 1,
       "arch": {"type": "FrozenInTime", "args": {"video_params": TINY_VIDEO, "text_params": TINY_TEXT, "projection": "minimal",
                                                 "load_checkpoint": ""}},
       "optimizer": {"type": "AdamW", "args": {"lr": 3e-5}},
       "loss": {"type": "EgoNCE", "args": {"learnable_temperature": True}},
       "metrics": [],
       "trainer": {"epochs": 1, "max_samples_per_epoch": 500000, "save_dir": "unused", "save_period": 1, "verbosity": 2,
                   "monitor": "off", "init_val": False, "neptune": False}}


class _Loader:
    batch_size, n_samples, dataset_name = 4, 8, "EgoClip-synthetic"

    def __len__(self):
        return 2

    def __iter__(self):
        from egovlp_amd.synth import synth_batch
        for i in range(2):
            b = synth_batch(4, T=2, L=8, seed=50 + i, res=32)
            yield {"video": b["video"], "text": dict(b["text"]), "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


class _Writer:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, key, value, step):
        self.scalars.append((key, value))


def _trainer(tmp, resume=None, learnable=True, temperature_lr=None, writer=None):
    import copy
    import egovlp_amd.model.loss as module_loss
    import egovlp_amd.model.model as module_arch
    import egovlp_amd.optim as module_optim
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.trainer.trainer_egoclip import Multi_Trainer_dist
    from egovlp_amd.utils.config import DictConfig
    Precision.set("bf16x3")
    cfg = copy.deepcopy(CFG)
    cfg["loss"]["args"] = {"learnable_temperature": True} if learnable else {}
    config = DictConfig(cfg, save_dir=tmp, resume=resume)
    model = config.initialize('arch', module_arch)
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=2))
    model.text_model.set_dropout(0.0, 0.0)
    loss = config.initialize(name="loss", module=module_loss)
    optimizer = config.initialize('optimizer', module_optim, filter(lambda p: p.requires_grad, model.parameters()))
    args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=2e-4, schedule=[60, 80])
    if temperature_lr is not None:
        args.temperature_lr = temperature_lr
    return Multi_Trainer_dist(args, model, loss, [], optimizer, config=config, data_loader=[_Loader()], valid_data_loader=None,
                              tokenizer=None, writer=writer, max_samples_per_epoch=500000)


def test_trainer_group_checkpoint_and_resume(tmp_path):
    import os
    from egovlp_amd.utils.util import load_checkpoint_file
    w = _Writer()
    tr = _trainer(tmp_path / "run1", temperature_lr=1e-3, writer=w)
    assert tr.loss.logit_scale.is_cuda
    assert len(tr.optimizer.param_groups) == 2
    g = tr.optimizer.param_groups[1]
    assert g["params"][0] is tr.loss.logit_scale and g["weight_decay"] == 0.0 and g["lr"] == 1e-3
    s0 = float(tr.loss.logit_scale.detach())
    tr.train()                                                  # one epoch of two steps, checkpoint-epoch1.pth
    s1 = float(tr.loss.logit_scale.detach())
    assert s1 != s0 and abs(s1 - s0) < 2.1e-3                   # two Adam steps at lr 1e-3
    temps = [v for k, v in w.scalars if k == "Loss_training/temperature_0"]
    assert temps and all(abs(t - 0.05) < 1e-3 for t in temps)   # logged next to the loss
    assert tr.optimizer.param_groups[1]["lr"] == 1e-3 and tr.optimizer.param_groups[0]["lr"] == 2e-4   # the LR rule keeps the own rate
    path = str(tmp_path / "run1" / "checkpoint-epoch1.pth")
    ck = load_checkpoint_file(path, map_location="cpu", trusted=True)
    assert set(ck) == {"arch", "epoch", "state_dict", "optimizer", "monitor_best", "config", "loss_state_dict"}
    assert list(ck["loss_state_dict"]) == ["logit_scale"] and float(ck["loss_state_dict"]["logit_scale"]) == s1
    assert len(ck["optimizer"]["param_groups"]) == 2
    # resume restores the scale and its moments
    tr2 = _trainer(tmp_path / "run2", resume=path, temperature_lr=1e-3)
    assert tr2.start_epoch == 2 and float(tr2.loss.logit_scale.detach()) == s1
    assert tr2.optimizer.state[tr2.loss.logit_scale]["step"] == 2
    # a checkpoint without the key: resumes as before, the scale keeps its initial value
    del ck["loss_state_dict"]
    ck["config"] = None                                         # the loaded file holds a placeholder of the config class: not picklable
    torch.save(ck, str(tmp_path / "nokey.pth"))
    tr3 = _trainer(tmp_path / "run3", resume=str(tmp_path / "nokey.pth"))
    assert tr3.start_epoch == 2 and float(tr3.loss.logit_scale.detach()) == s0
    # a checkpoint of a fixed-temperature run (no key, one optimizer group) resumes into a learnable one and the other way round
    trf = _trainer(tmp_path / "run4", learnable=False)
    assert len(trf.optimizer.param_groups) == 1 and not hasattr(trf.loss, "logit_scale")
    trf.train()
    pf = str(tmp_path / "run4" / "checkpoint-epoch1.pth")
    ckf = load_checkpoint_file(pf, map_location="cpu", trusted=True)
    assert set(ckf) == {"arch", "epoch", "state_dict", "optimizer", "monitor_best", "config"}
    tr5 = _trainer(tmp_path / "run5", resume=pf)
    assert tr5.start_epoch == 2 and float(tr5.loss.logit_scale.detach()) == s0 and len(tr5.optimizer.param_groups) == 2
    assert tr5.optimizer.param_groups[1]["params"][0] is tr5.loss.logit_scale and tr5.optimizer.param_groups[1]["weight_decay"] == 0.0
    assert all(st["step"] == 2 for p_, st in tr5.optimizer.state.items() if p_ is not tr5.loss.logit_scale)
    assert os.path.exists(pf)
