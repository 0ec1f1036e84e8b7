"""The pairwise sigmoid head on a real MI355X (`pytest -m gpu`): egv_sigmoid_head_fwd_bwd and egv_sigmoid_from_sim against the fp64
oracle of tests/sigmoid_ref.py, then the autograd nodes, the 1 / W convention, whole steps (plain, cached), the trainer's optimizer
group, checkpoints and logs.

Bars (those of tests/test_gpu_egonce_long.py and tests/test_gpu_learnable_temperature.py).  Loss: |got - ref| < 1e-4 max(1, |ref|).
Embedding gradients: rel-L2 < 1e-4.  d_scale, d_bias: |got - ref| < 1e-4 |ref|; where the oracle's own cancellation
(sum |term| / |sum term|) exceeds 10, 1e-4 sum |term| instead.  n = 1: unlike the softmax heads, whose gradients are exactly zero
there, the sigmoid loss of one pair has a gradient (the oracle's is about 0.03 per element), so the 1e-6 bar of n = 1 is applied to
the largest |got - ref| of the embedding gradients, on top of the rel-L2 bar.

Sizes.  The walk's split differs from the long EgoNCE head's (about 512 workgroups, not 256: tests/sigmoid_ref.py walk_split), so
1 030 rows -- 17 tiles, the last one of 6 rows -- are still one column tile per workgroup; 1 473 rows are the smallest size at which
a workgroup walks more than one column tile (24 tiles in twelve ranges of two) and the last tile is partial (one row).  Both are in
the list.  Measured errors: DESIGN 4.5f."""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import sigmoid_ref as S  # noqa: E402

LOSS_BAR = 1e-4
GRAD_BAR = 1e-4
PARAM_BAR = 1e-4
PARAMS = ((S.LN10, -10.0), (S.LN20, -3.0))
SIZES = [(1, 256), (2, 64), (5, 64), (63, 256), (64, 256), (65, 256), (130, 252), (65, 32), (1030, 256), (1473, 256)]


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import loss_ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


_INPUTS, _ORACLE = {}, {}


def inputs(n, D, dn=16, dv=12):
    key = (n, D, dn, dv)
    if key not in _INPUTS:
        _INPUTS[key] = S.make_inputs(n, D, seed=n + D, dn=dn, dv=dv)
    return _INPUTS[key]


def oracle(n, D, s, b, mode="ego", dn=16, dv=12):
    """fp64 oracle on the shared inputs, computed once per case and never modified.  mode: 'ego', 'noun', 'verb', 'identity'"""
    key = (n, D, s, b, mode, dn, dv)
    if key not in _ORACLE:
        text, video, noun, verb = inputs(n, D, dn, dv)
        if mode == "identity":
            o = S.oracle(text, video, None, None, s, b)
        else:
            o = S.oracle(text, video, noun, verb, s, b, mode != "verb", mode != "noun")
        for k in ("x", "G", "mask"):
            o.pop(k)
        _ORACLE[key] = o
    return _ORACLE[key]


def dev1(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def head(ops, n, D, s, b, mode="ego", dn=16, dv=12, **kw):
    text, video, noun, verb = (t.cuda() for t in inputs(n, D, dn, dv))
    if mode == "identity":
        return ops.sigmoid_head_fwd_bwd(text, video, None, None, dev1(s), dev1(b), **kw)
    # noun = verb = False is mapped to the verb mode by EgoSigmoidLoss, as EgoNCE does
    return ops.sigmoid_head_fwd_bwd(text, video, noun, verb, dev1(s), dev1(b), use_noun=mode != "verb", use_verb=mode != "noun", **kw)


def param_bar(o, k):
    a = o["abs_scale" if k == "d_scale" else "abs_bias"]
    return PARAM_BAR * (a if a > 10.0 * abs(o[k]) else abs(o[k]))


def check_head(tag, n, got, o):
    """got = (loss, d_text, d_video, d_scale, d_bias); prints every figure before it asserts"""
    loss, dt, dv, ds, db = float(got[0]), got[1].cpu(), got[2].cpu(), float(got[3]), float(got[4])
    rl = float(o["loss"])
    el, et, ev = abs(loss - rl), S.rel(dt, o["d_text"]), S.rel(dv, o["d_video"])
    es, eb = abs(ds - o["d_scale"]), abs(db - o["d_bias"])
    at = float((dt.double() - o["d_text"]).abs().max())
    av = float((dv.double() - o["d_video"]).abs().max())
    print("%s: loss %.7e |diff| %.2e (bar %.1e); d_text rel %.2e max|diff| %.2e, d_video rel %.2e max|diff| %.2e (bar %.0e); "
          "d_scale %.7e oracle %.7e |diff| %.2e = %.2e |ref| (bar %.2e, cancellation %.1f); d_bias %.7e oracle %.7e |diff| %.2e = %.2e |ref| "
          "(bar %.2e, cancellation %.1f)" % (tag, loss, el, LOSS_BAR * max(1.0, abs(rl)), et, at, ev, av, GRAD_BAR, ds, o["d_scale"], es,
                                            es / max(abs(o["d_scale"]), 1e-300), param_bar(o, "d_scale"),
                                            o["abs_scale"] / max(abs(o["d_scale"]), 1e-300), db, o["d_bias"], eb,
                                            eb / max(abs(o["d_bias"]), 1e-300), param_bar(o, "d_bias"),
                                            o["abs_bias"] / max(abs(o["d_bias"]), 1e-300)))
    assert math.isfinite(loss) and el < LOSS_BAR * max(1.0, abs(rl)), (tag, el)
    assert et < GRAD_BAR and ev < GRAD_BAR, (tag, et, ev)
    if n == 1:
        assert at < 1e-6 and av < 1e-6, (tag, at, av)
    assert es < param_bar(o, "d_scale"), (tag, ds, o["d_scale"])
    assert eb < param_bar(o, "d_bias"), (tag, db, o["d_bias"])


# ------------------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("n,D", SIZES)
def test_head_matches_the_oracle(ops, n, D):
    for s, b in PARAMS:
        got = head(ops, n, D, s, b)
        assert all(g.shape == (1,) for g in (got[0], got[3], got[4])) and got[1].shape == (n, D) and got[2].shape == (n, D)
        check_head("n=%d D=%d s=%.3f b=%g" % (n, D, s, b), n, got, oracle(n, D, s, b))


def test_packed_words_across_a_word_boundary(ops):
    """dn = 33, dv = 65: the last noun / verb sits in bit 0 of a second / third word"""
    n, D = 130, 256
    _, _, noun, verb = inputs(n, D, 33, 65)
    assert float(noun[:, 32].sum()) > 0 and float(verb[:, 64].sum()) > 0
    for s, b in PARAMS:
        check_head("dn=33 dv=65 s=%.3f b=%g" % (s, b), n, head(ops, n, D, s, b, dn=33, dv=65), oracle(n, D, s, b, dn=33, dv=65))


def test_padding_is_masked_out(ops):
    """n = 65, (s, b) = (ln 10, 0): each of the 128 * 128 - 65 * 65 padded pairs has u = 0 and would add log 2 to the sum, a half to
    sum z p"""
    check_head("padding trap n=65", 65, head(ops, 65, 256, S.LN10, 0.0), oracle(65, 256, S.LN10, 0.0))
    check_head("padding trap n=1473", 1473, head(ops, 1473, 256, S.LN10, 0.0), oracle(1473, 256, S.LN10, 0.0))


def test_mask_modes(ops):
    n, D = 130, 256
    s, b = PARAMS[0]
    default = float(oracle(n, D, s, b)["loss"])
    for mode in ("noun", "verb", "identity"):
        o = oracle(n, D, s, b, mode)
        assert abs(float(o["loss"]) - default) > 1e-3, (mode, float(o["loss"]), default)       # the bar tells the mode from the default
        check_head("mode %s" % mode, n, head(ops, n, D, s, b, mode), o)
    # neither flag: the reference's else-branch, verb -- the mapping is the module's
    from egovlp_amd.model.loss import EgoSigmoidLoss
    text, video, noun, verb = (t.cuda() for t in inputs(n, D))
    loss_fn = EgoSigmoidLoss(noun=False, verb=False).cuda()
    tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
    loss_fn.fused(tc, vc, noun, verb).backward()
    check_head("noun=False verb=False", n, (loss_fn.fused(tc, vc, noun, verb).detach(), tc.grad, vc.grad, loss_fn.logit_scale.grad,
                                              loss_fn.logit_bias.grad), oracle(n, D, s, b, "verb"))


def test_eps_paths(ops):
    """a zero text row and a zero video row: tn = 0 / eps, and the backward of the normalisation takes its g / eps branch"""
    n, D = 65, 256
    text, video, noun, verb = (t.clone() for t in inputs(n, D))
    text[3] = 0.0
    video[64] = 0.0
    s, b = PARAMS[1]
    o = S.oracle(text, video, noun, verb, s, b)
    got = ops.sigmoid_head_fwd_bwd(text.cuda(), video.cuda(), noun.cuda(), verb.cuda(), dev1(s), dev1(b))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    check_head("zero rows", n, got, o)
    keep_t = [i for i in range(n) if i != 3]
    keep_v = [i for i in range(n) if i != 64]
    et, ev = S.rel(got[1].cpu()[keep_t], o["d_text"][keep_t]), S.rel(got[2].cpu()[keep_v], o["d_video"][keep_v])
    print("without the zero rows: d_text rel %.2e d_video rel %.2e" % (et, ev))
    assert et < GRAD_BAR and ev < GRAD_BAR
    assert float(got[1][3].abs().max()) > 1e3 and float(got[2][64].abs().max()) > 1e3          # g / eps


@pytest.mark.parametrize("b", [50.0, -50.0])
def test_range(ops, b):
    n, D = 65, 256
    got = head(ops, n, D, S.LN100, b)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    check_head("s=ln 100 b=%g" % b, n, got, oracle(n, D, S.LN100, b))


def test_a_bad_noun_entry_makes_the_loss_nan(ops):
    n, D = 65, 256
    text, video, noun, verb = (t.cuda() for t in inputs(n, D))
    for bad in (-1.0, float("nan")):
        for which in (0, 1):
            nn_, vv = noun.clone(), verb.clone()
            (nn_ if which == 0 else vv)[64, 5] = bad
            for kw in ({}, {"want_grads": False}):
                loss = ops.sigmoid_head_fwd_bwd(text, video, nn_, vv, dev1(S.LN10), dev1(-10.0), **kw)[0]
                assert math.isnan(float(loss)), (bad, which, kw)
    assert math.isfinite(float(ops.sigmoid_head_fwd_bwd(text, video, noun, verb, dev1(S.LN10), dev1(-10.0))[0]))


def test_two_calls_are_bit_identical(ops):
    for n in (130, 1473):
        a = head(ops, n, 256, *PARAMS[0])
        b = head(ops, n, 256, *PARAMS[0])
        torch.cuda.synchronize()
        assert len(a) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_loss_only_call(ops):
    for n in (65, 1473):
        full_ = head(ops, n, 256, *PARAMS[0])
        only = head(ops, n, 256, *PARAMS[0], want_grads=False)
        assert all(x is None for x in only[1:])
        o = oracle(n, 256, *PARAMS[0])
        print("loss-only n=%d: %.8e with gradients %.8e oracle %.8e" % (n, float(only[0]), float(full_[0]), float(o["loss"])))
        assert torch.equal(only[0], full_[0])                      # the same walk without the second product
        fixed = head(ops, n, 256, *PARAMS[0], want_param_grads=False)
        assert fixed[3] is None and fixed[4] is None and torch.equal(fixed[1], full_[1]) and torch.equal(fixed[2], full_[2])


def test_bad_arguments_are_refused(ops):
    import ctypes
    from egovlp_amd import _lib
    h = _lib.lib()
    t = torch.ones(64, 8).cuda()
    w = torch.zeros(1 << 16).cuda()
    out, s, b = torch.zeros(1).cuda(), dev1(S.LN10), dev1(-10.0)
    g1, g2, ds, db = torch.zeros(64, 8).cuda(), torch.zeros(64, 8).cuda(), torch.zeros(1).cuda(), torch.zeros(1).cuda()
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(n=8, D=8, s_=s, b_=b, dt=None, dv=None, dsc=None, dbi=None):
        return h.egv_sigmoid_head_fwd_bwd(p(t), p(t), None, None, n, D, 0, 0, p(s_), p(b_), 1e-8, 1, 1, p(out), p(dt), p(dv), p(dsc), p(dbi),
                                          p(w), None)
    assert call(n=0) == 1 and call(n=65537) == 1 and call(D=260) == 1 and call(D=6) == 1
    assert call(s_=None) == 1 and call(b_=None) == 1
    assert call(dsc=ds, dbi=db) == 1                               # the parameter gradients ride on the embedding gradients' walk
    assert call(dt=g1) == 1 and call(dt=g1, dv=g2, dsc=ds) == 1    # each pair comes together
    assert h.egv_sigmoid_head_work_floats(0, 8, 0, 0) == 0 and h.egv_sigmoid_head_work_floats(8, 6, 0, 0) == 0
    x = torch.zeros(8, 8).cuda()
    fs = lambda n=8, s_=s, b_=b, dx=None, dsc=None, dbi=None, sv=None, sn=None: h.egv_sigmoid_from_sim(
        p(x), p(sv), p(sn), n, p(s_), p(b_), 1, 1, p(out), p(dx), p(dsc), p(dbi), p(w), None)
    assert fs(n=0) == 1 and fs(n=4097) == 1 and fs(s_=None) == 1 and fs(b_=None) == 1 and fs(dsc=ds, dbi=db) == 1 and fs(sv=x) == 1
    assert call() == 0 and call(dt=g1, dv=g2) == 0 and call(dt=g1, dv=g2, dsc=ds, dbi=db) == 0 and fs() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.sigmoid_head_fwd_bwd(t, t, None, None, torch.zeros(2).cuda(), b)
    with pytest.raises(ValueError):
        ops.sigmoid_head_fwd_bwd(t, t, None, None, s, torch.zeros(1))


# ------------------------------------------------------------------------------------------------------------ autograd nodes
@pytest.mark.parametrize("n", [65, 300])
def test_from_sim_path_gives_the_fused_gradient(ops, n):
    from egovlp_amd.model.loss import EgoSigmoidLoss, SigmoidLoss
    from egovlp_amd.model.model import sim_matrix
    D = 256
    text, video, noun, verb = (t.cuda() for t in inputs(n, D))
    for mode, (s, b) in (("ego", PARAMS[0]), ("noun", PARAMS[1]), ("identity", PARAMS[0]), ("verb", PARAMS[1])):
        o = oracle(n, D, s, b, mode)
        res = []
        for fused in (True, False):
            if mode == "identity":
                loss_fn = SigmoidLoss(s, b).cuda()
            else:
                loss_fn = EgoSigmoidLoss(s, b, noun=mode != "verb", verb=mode != "noun").cuda()
            tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
            if mode == "identity":
                loss = loss_fn.fused(tc, vc) if fused else loss_fn(sim_matrix(tc, vc))
            else:
                loss = loss_fn.fused(tc, vc, noun, verb) if fused else loss_fn(sim_matrix(tc, vc), sim_matrix(verb, verb), sim_matrix(noun, noun))
            loss.backward()
            assert loss_fn.logit_scale.grad.shape == (1,) and loss_fn.logit_bias.grad.shape == (1,)
            res.append((loss.detach(), tc.grad, vc.grad, loss_fn.logit_scale.grad, loss_fn.logit_bias.grad))
        check_head("from-sim n=%d %s" % (n, mode), n, res[1], o)
        r_t, r_v = S.rel(res[1][1], res[0][1]), S.rel(res[1][2], res[0][2])
        print("from-sim against fused n=%d %s: d_text rel %.2e d_video rel %.2e" % (n, mode, r_t, r_v))
        assert r_t < 2 * GRAD_BAR and r_v < 2 * GRAD_BAR          # each is within one bar of the oracle
        assert abs(float(res[0][3]) - float(res[1][3])) < 2 * param_bar(o, "d_scale")
        assert abs(float(res[0][4]) - float(res[1][4])) < 2 * param_bar(o, "d_bias")


def _fused_backward(n, factor=1.0, learnable=True):
    from egovlp_amd.model.loss import EgoSigmoidLoss
    text, video, noun, verb = (t.cuda() for t in inputs(n, 256))
    loss_fn = EgoSigmoidLoss(learnable=learnable).cuda()
    tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
    loss = loss_fn.fused(tc, vc, noun, verb)
    (loss if factor == 1.0 else factor * loss).backward()
    return loss.detach(), tc.grad, vc.grad, loss_fn.logit_scale.grad, loss_fn.logit_bias.grad


@pytest.mark.parametrize("n", [300, 1473])
def test_upstream_factor(n):
    plain, tripled = _fused_backward(n), _fused_backward(n, 3.0)
    torch.cuda.synchronize()
    assert all(torch.equal(tripled[k], 3.0 * plain[k]) for k in (1, 2, 3, 4))
    check_head("EgoSigmoidLoss.fused n=%d upstream 3.0" % n, n, (plain[0],) + tuple(tripled[k] / 3.0 for k in (1, 2, 3, 4)),
               oracle(n, 256, *PARAMS[0]))


def test_fixed_parameters_get_no_gradient():
    fixed, plain = _fused_backward(300, learnable=False), _fused_backward(300)
    assert fixed[3] is None and fixed[4] is None
    assert torch.equal(fixed[0], plain[0]) and torch.equal(fixed[1], plain[1]) and torch.equal(fixed[2], plain[2])


def test_parameter_gradients_are_stored_over_the_world_size(monkeypatch):
    from egovlp_amd import gather
    one = _fused_backward(300)
    monkeypatch.setattr(gather, "_world", lambda: 4)
    four = _fused_backward(300)
    torch.cuda.synchronize()
    assert torch.equal(four[3], one[3] / 4.0) and torch.equal(four[4], one[4] / 4.0) and float(one[3]) != 0.0 and float(one[4]) != 0.0
    assert torch.equal(four[1], one[1]) and torch.equal(four[2], one[2])          # the embedding gradients go through the gather's backward


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


def _step(full, lr=1e-3, chunk=None):
    """one EgoClip step with EgoSigmoidLoss; the model's learning rate is 0 -> (loss_fn, optimizer, (s0, b0), the step's loss)"""
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoSigmoidLoss
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached, register_loss_parameters
    CS, m, sd, dev = full
    CS._set_mode("bf16x3")
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    for p in m.parameters():
        p.grad = None
    loss_fn = EgoSigmoidLoss().cuda()
    opt = AdamW(m.parameters(), lr=0.0)
    g = register_loss_parameters(opt, loss_fn, lr=lr)
    assert g is not None and len(g["params"]) == 2
    before = (float(loss_fn.logit_scale.detach()), float(loss_fn.logit_bias.detach()))
    if chunk is None:
        loss = egoclip_step(m, loss_fn, opt, dev)
    else:
        loss = egoclip_step_cached(m, loss_fn, opt, dev, chunk)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    return loss_fn, opt, before, float(loss)


def test_a_whole_step_moves_both_parameters_by_adams_first_step(full):
    from egovlp_amd.optim import adamw_step_size
    lr = 1e-3
    loss_fn, opt, (s0, b0), loss = _step(full, lr=lr)
    b1_, b2_ = opt.param_groups[1]["betas"]
    for name, p, v0 in (("logit_scale", loss_fn.logit_scale, s0), ("logit_bias", loss_fn.logit_bias, b0)):
        g, v1 = float(p.grad), float(p.detach())
        # Adam's first step with bias correction: -step_size (1 - b1) g / (sqrt((1 - b2) g^2) + eps) = -lr sign(g) up to eps
        want = -adamw_step_size(lr, b1_, b2_, 1) * (1.0 - b1_) * g / (math.sqrt((1.0 - b2_) * g * g) + opt.param_groups[1]["eps"])
        print("%s: gradient %.6e, %.7f -> %.7f step %.6e, -lr sign %.6e, Adam's %.6e" % (name, g, v0, v1, v1 - v0,
                                                                                      -lr * math.copysign(1.0, g), want))
        assert abs(g) > 1e-3                                       # far above eps / sqrt(1 - b2): the step is lr sign(g)
        assert abs((v1 - v0) - (-lr * math.copysign(1.0, g))) < 0.01 * lr
        assert abs((v1 - v0) - want) < 0.01 * lr
    assert 0.0 <= float(loss_fn.logit_scale.detach()) <= math.log(100)
    # the step's loss is the oracle's on the gathered embeddings (the model's learning rate is 0: the same weights give them again)
    CS, m, sd, dev = full
    with torch.no_grad(), m.exec_ctx.train_kernels_without_grad():
        te, ve = m(dev)
    o = S.oracle(te.float().cpu(), ve.float().cpu(), dev["noun_vec"].float().cpu(), dev["verb_vec"].float().cpu(), s0, b0)
    print("step loss %.7e oracle on the embeddings %.7e |diff| %.2e" % (loss, float(o["loss"]), abs(loss - float(o["loss"]))))
    assert abs(loss - float(o["loss"])) < LOSS_BAR * max(1.0, abs(float(o["loss"])))


def test_cached_step_gives_the_plain_steps_parameter_gradients(full):
    CS = full[0]
    plain, _, _, l0 = _step(full, lr=0.0)
    cached, _, _, l1 = _step(full, lr=0.0, chunk=2)
    for name in ("logit_scale", "logit_bias"):
        a, b = getattr(plain, name).grad, getattr(cached, name).grad
        r = CS.rel(b, a)
        print("%s.grad plain %.7e cached %.7e rel %.2e (bar %.0e)" % (name, float(a), float(b), r, 2 * CS.GRAD_BAR["bf16x3"]))
        assert float(a) != 0.0 and r <= 2 * CS.GRAD_BAR["bf16x3"]
    assert abs(l0 - l1) < LOSS_BAR * max(1.0, abs(l0))


# ------------------------------------------------------------------------------------------------------------ trainer
TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
CFG = {"name": "EgoClip_tiny", "n_gpu": 1,
       "arch": {"type": "FrozenInTime", "args": {"video_params": TINY_VIDEO, "text_params": TINY_TEXT, "projection": "minimal",
                                                 "load_checkpoint": ""}},
       "optimizer": {"type": "AdamW", "args": {"lr": 3e-5}},
       "loss": {"type": "EgoSigmoidLoss", "args": {}},
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


def _trainer(tmp, resume=None, writer=None):
    import copy
    import egovlp_amd.model.loss as module_loss
    import egovlp_amd.model.model as module_arch
    import egovlp_amd.optim as module_optim
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.trainer.trainer_egoclip import Multi_Trainer_dist
    from egovlp_amd.utils.config import DictConfig
    Precision.set("bf16x3")
    config = DictConfig(copy.deepcopy(CFG), save_dir=tmp, resume=resume)
    model = config.initialize('arch', module_arch)
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=2))
    model.text_model.set_dropout(0.0, 0.0)
    loss = config.initialize(name="loss", module=module_loss)
    optimizer = config.initialize('optimizer', module_optim, filter(lambda p: p.requires_grad, model.parameters()))
    args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=2e-4, schedule=[60, 80], temperature_lr=1e-3)
    return Multi_Trainer_dist(args, model, loss, [], optimizer, config=config, data_loader=[_Loader()], valid_data_loader=None,
                              tokenizer=None, writer=writer, max_samples_per_epoch=500000)


def test_trainer_group_checkpoint_resume_and_logs(tmp_path):
    from egovlp_amd.utils.util import load_checkpoint_file
    w = _Writer()
    tr = _trainer(tmp_path / "run1", writer=w)
    assert type(tr.loss).__name__ == "EgoSigmoidLoss" and tr.loss.logit_scale.is_cuda and tr.loss.logit_bias.is_cuda
    assert len(tr.optimizer.param_groups) == 2
    g = tr.optimizer.param_groups[1]
    assert len(g["params"]) == 2 and g["params"][0] is tr.loss.logit_scale and g["params"][1] is tr.loss.logit_bias
    assert g["weight_decay"] == 0.0 and g["lr"] == 1e-3
    s0, b0 = float(tr.loss.logit_scale.detach()), float(tr.loss.logit_bias.detach())
    tr.train()                                                  # one epoch of two steps, checkpoint-epoch1.pth
    s1, b1 = float(tr.loss.logit_scale.detach()), float(tr.loss.logit_bias.detach())
    assert s1 != s0 and abs(s1 - s0) < 2.1e-3 and b1 != b0 and abs(b1 - b0) < 2.1e-3      # two Adam steps at lr 1e-3
    temps = [v for k, v in w.scalars if k == "Loss_training/temperature_0"]
    biases = [v for k, v in w.scalars if k == "Loss_training/bias_0"]
    losses = [v for k, v in w.scalars if k == "Loss_training/loss_0"]
    assert temps and len(temps) == len(biases) == len(losses)   # logged next to the loss
    assert all(abs(t - 0.1) < 1e-3 for t in temps) and all(abs(b + 10.0) < 3e-3 for b in biases)
    assert tr.optimizer.param_groups[1]["lr"] == 1e-3 and tr.optimizer.param_groups[0]["lr"] == 2e-4
    path = str(tmp_path / "run1" / "checkpoint-epoch1.pth")
    ck = load_checkpoint_file(path, map_location="cpu", trusted=True)
    assert list(ck["loss_state_dict"]) == ["logit_scale", "logit_bias"]
    assert float(ck["loss_state_dict"]["logit_scale"]) == s1 and float(ck["loss_state_dict"]["logit_bias"]) == b1
    assert len(ck["optimizer"]["param_groups"]) == 2
    # resume restores both values and their moments
    tr2 = _trainer(tmp_path / "run2", resume=path)
    assert tr2.start_epoch == 2 and float(tr2.loss.logit_scale.detach()) == s1 and float(tr2.loss.logit_bias.detach()) == b1
    assert tr2.optimizer.state[tr2.loss.logit_scale]["step"] == 2 and tr2.optimizer.state[tr2.loss.logit_bias]["step"] == 2
