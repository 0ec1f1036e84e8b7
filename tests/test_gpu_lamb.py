"""LAMB on a real MI355X (`pytest -m gpu`): the three kernels of csrc/lamb.hip at their table, chunk and alignment boundaries against
the fp64 oracle of tests/lamb_ref.py (element by element, sentinel guards around every tensor), the branches of the rule, bit-identical
repeats, the skipped step, `LAMB.step` over three steps, the whole EgoClip step (plain and cached) and the trainer with a checkpoint.

Bounds (derived in tests/lamb_ref.py, not measured): moments within 4 u s_m and 6 u v; a trust ratio within RHO = 74 u of the fp64
one; a parameter within 20 u (|p| + |D|) + RHO |D|, D = lr r u, u = 2^-24."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import lamb_ref as L  # noqa: E402
import multi_tensor_ref as R  # noqa: E402
from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402

DEV = "cuda"
CHUNK = L.CHUNK
GUARD = 0x7FC5A5A5          # a NaN pattern around the ratio and partial buffers


def _bits(t):
    return t.detach().view(torch.int32)


class _Run:
    """One stage-1 / ratio / stage-2 pass over a case on the device, with everything a test looks at afterwards."""

    def __init__(self, specs, inputs):
        self.inputs = inputs
        self.arenas = {s: R.Arena(specs[s]).fill(x).to(DEV) for s, x in zip("pgmv", inputs)}
        self.n = len(inputs[0])
        self.parts = L.parts_of([t.numel() for t in inputs[0]])
        # both buffers sit between guard words: a store outside them shows
        self._pbuf = torch.full((2 * self.parts + 8,), GUARD, dtype=torch.int32, device=DEV).view(torch.float32)
        self._rbuf = torch.full((self.n + 8,), GUARD, dtype=torch.int32, device=DEV).view(torch.float32)
        self.partials, self.ratios = self._pbuf[4:4 + 2 * self.parts], self._rbuf[4:4 + self.n]

    def go(self, lr=L.LR, wd=L.WD, step=1, correct_bias=True, grad_scale=1.0, hyper=None, adapt=None, trust_clip=False, stages=3):
        from egovlp_amd import ops
        a = self.arenas
        ps, gs, ms, vs = (a[s].views for s in "pgmv")
        adapt = (wd != 0.0) if adapt is None else adapt
        hyper_dev = None if hyper is None else torch.tensor(hyper, dtype=torch.float32, device=DEV)
        b1, b2 = L.BETAS
        tables = ops.lamb_tables(ps, ms, vs)
        assert tables[4] == self.parts
        ops.lamb_stage1_multi(ps, gs, ms, vs, lr, b1, b2, L.EPS, wd, step, correct_bias, grad_scale, self.partials, hyper_dev, tables)
        if stages >= 2:
            ops.lamb_ratio(ps, self.partials, self.ratios, adapt, trust_clip, hyper_dev, tables)
        if stages >= 3:
            ops.lamb_stage2_multi(ps, ms, vs, lr, b1, b2, L.EPS, wd, step, correct_bias, self.ratios, hyper_dev, tables)
        torch.cuda.synchronize()
        return self

    def guards(self, what):
        for s in "pgmv":
            self.arenas[s].assert_guards("%s arena, %s" % (s, what))
        for buf, n in ((self._pbuf, 2 * self.parts), (self._rbuf, self.n)):
            edge = torch.cat([_bits(buf)[:4], _bits(buf)[4 + n:]]).cpu()
            assert bool((edge == GUARD).all()), (what, "a store outside the partial / ratio buffer")

    def results(self):
        return tuple(self.arenas[s].tensors_cpu() for s in "pmv") + (self.ratios.cpu(),)


def _compare(run, ref, lr, c, what, ratio_exact=None):
    """p, m, v of every tensor and every ratio against the oracle -> the largest err / bound seen (p, m, v, ratio)."""
    ps, gs, ms, vs = run.inputs
    got_p, got_m, got_v, got_r = run.results()
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(run.n):
        w = L.check_lamb(got_p[k], got_m[k], got_v[k], ref, k, ps[k], ms[k], lr, c, what="%s tensor %d (numel %d)" % (what, k, ps[k].numel()))
        if ratio_exact is not None:
            assert float(got_r[k]) == ratio_exact, (what, k, float(got_r[k]))
            wr = 0.0
        else:
            wr = L.check_ratio(got_r[k], ref["r"][k], what="%s tensor %d (numel %d)" % (what, k, ps[k].numel()))
        worst = [max(a, b) for a, b in zip(worst, w + (wr,))]
    return worst


# ------------------------------------------------------------------------------------------------ 1. the kernels at their boundaries
_CASES = {}


def _case(which, step, grad_scale):
    key = (which, step, grad_scale)
    if key not in _CASES:
        _CASES[key] = (L.case_specs(which), L.case_inputs(which, step, grad_scale))
    return _CASES[key]


@pytest.mark.parametrize("variant", ["host scalars, step 1", "hyper block, step 1000"])
@pytest.mark.parametrize("which", L.CASES)
def test_kernels_at_their_boundaries(which, variant):
    step, gsc = (1, 1.0) if variant.startswith("host") else (1000, 1.0 / 1024)
    specs, inputs = _case(which, step, gsc)
    run = _Run(specs, inputs)
    views = run.arenas["p"].views
    if which == "boundaries":
        assert any(v.numel() > CHUNK and v.data_ptr() % 16 == 4 for v in views)
        assert any(v.numel() % 4 == 3 and v.data_ptr() % 16 == 0 for v in views)
        assert any(v.numel() == 0 for v in views[1:-1])
    elif which == "n97":
        first_table = [v for v in views if v.numel()][:L.TABLE]
        assert any(v.numel() > CHUNK for v in [v for v in views if v.numel()][L.TABLE:]) and len(first_table) == L.TABLE
    c = L.correction(*L.BETAS, step)
    hyper = None
    if not variant.startswith("host"):
        # what egv_loss_scale_update / egv_grad_clip_update leave: {lr, fp32(lr c), (1 / S) coef, 0}; the host scalars are decoys
        hyper = [R.f32(L.LR), R.f32(R.f32(L.LR) * c), gsc, 0.0]
    # stage 1 alone first: it writes neither p nor g
    p0, g0 = run.arenas["p"].snapshot(), run.arenas["g"].snapshot()
    kw = dict(hyper=hyper) if hyper is not None else dict(step=step, grad_scale=gsc)
    if hyper is not None:
        kw.update(lr=123.0, step=3, grad_scale=77.0)
    run.go(stages=2, **kw)
    assert torch.equal(run.arenas["p"].bits, p0) and torch.equal(run.arenas["g"].bits, g0)
    run.guards("%s after stage 1" % which)
    m1, v1 = run.arenas["m"].snapshot(), run.arenas["v"].snapshot()
    from egovlp_amd import ops
    hyper_dev = None if hyper is None else torch.tensor(hyper, dtype=torch.float32, device=DEV)
    a = run.arenas
    ops.lamb_stage2_multi(a["p"].views, a["m"].views, a["v"].views, kw.get("lr", L.LR), *L.BETAS, L.EPS, L.WD, kw.get("step", 1), True,
                          run.ratios, hyper_dev)
    torch.cuda.synchronize()
    run.guards("%s after stage 2" % which)
    assert torch.equal(a["g"].bits, g0) and torch.equal(a["m"].bits, m1) and torch.equal(a["v"].bits, v1)      # stage 2 writes p alone
    ref = L.lamb_ref64(*inputs, L.LR, L.BETAS, L.EPS, L.WD, c, gsc)
    worst = _compare(run, ref, L.LR, c, "%s, %s" % (which, variant))
    # an empty tensor keeps its slot (ratio 1) and shifts nothing: its neighbours were compared with their own references above
    got_r = run.ratios.cpu()
    for k, t in enumerate(inputs[0]):
        if t.numel() == 0:
            assert float(got_r[k]) == 1.0 and ref["r"][k] == 1.0
    print("%s, %s: %d tensors, largest err / bound: p %.3f m %.3f v %.3f ratio %.3f" % (which, variant, run.n, *worst))


# ------------------------------------------------------------------------------------------------ 2. the rule's branches
BR_SIZES = [5, 1025, 0, CHUNK + 1, 3]
BR_SPECS = {s: [(n, 0) for n in BR_SIZES] for s in "pgmv"}


def _branch_inputs(step=1):
    return R.adamw_inputs(BR_SIZES, step, 1.0, 77)


def test_an_all_zero_tensor_moves_at_lr():
    ps, gs, ms, vs = _branch_inputs()
    ps = [torch.zeros_like(p) if k in (1, 3) else p for k, p in enumerate(ps)]
    run = _Run(BR_SPECS, (ps, gs, ms, vs)).go()
    c = L.correction(*L.BETAS, 1)
    ref = L.lamb_ref64(ps, gs, ms, vs, L.LR, L.BETAS, L.EPS, L.WD, c)
    _compare(run, ref, L.LR, c, "zero tensors")
    got_p, _, _, got_r = run.results()
    for k in (1, 3):
        assert float(got_r[k]) == 1.0 and bool((got_p[k] != 0).all())
        assert abs(float(got_p[k].abs().mean()) - L.LR * c * (1 - 0.9) / (1 - 0.999) ** 0.5) < 1e-3 * L.LR     # |u| = c (1 - b1) / sqrt(1 - b2) = 1
    run.guards("zero tensors")


def test_zero_gradients_and_moments_without_decay_leave_p_untouched():
    ps, gs, ms, vs = _branch_inputs()
    zeros = [torch.zeros_like(p) for p in ps]
    run = _Run(BR_SPECS, (ps, zeros, zeros, zeros))
    p0 = run.arenas["p"].snapshot()
    run.go(wd=0.0, adapt=True)
    assert torch.equal(run.arenas["p"].bits, p0) and run.ratios.cpu().tolist() == [1.0] * len(ps)
    assert all(not bool(t.any()) for t in run.arenas["m"].tensors_cpu() + run.arenas["v"].tensors_cpu())


@pytest.mark.parametrize("always_adapt", [False, True])
def test_a_group_without_decay_is_adapted_only_with_always_adapt(always_adapt):
    inputs = _branch_inputs(1000)
    run = _Run(BR_SPECS, inputs).go(wd=0.0, adapt=always_adapt, step=1000)
    c = L.correction(*L.BETAS, 1000)
    ref = L.lamb_ref64(*inputs, L.LR, L.BETAS, L.EPS, 0.0, c, always_adapt=always_adapt)
    _compare(run, ref, L.LR, c, "wd = 0, always_adapt %s" % always_adapt, ratio_exact=None if always_adapt else 1.0)
    if always_adapt:
        assert all(abs(r - 1.0) > 1e-3 for k, r in enumerate(run.ratios.cpu().tolist()) if BR_SIZES[k])


def test_trust_clip_caps_the_ratio_at_one():
    ps, gs, ms, vs = _branch_inputs()
    lr, c = 1e-4, L.correction(*L.BETAS, 1)
    big = [p * 8.0 for p in ps]                           # |u| is about 1 at step 1, so r is about ||p|| / sqrt(n) = 10
    free = _Run(BR_SPECS, (big, gs, ms, vs)).go(lr=lr)
    assert all(r > 2.0 for k, r in enumerate(free.ratios.cpu().tolist()) if BR_SIZES[k])      # |p| >= 4 and |u| <= 1.2 everywhere
    _compare(free, L.lamb_ref64(big, gs, ms, vs, lr, L.BETAS, L.EPS, L.WD, c), lr, c, "unclipped")
    capped = _Run(BR_SPECS, (big, gs, ms, vs)).go(lr=lr, trust_clip=True)
    _compare(capped, L.lamb_ref64(big, gs, ms, vs, lr, L.BETAS, L.EPS, L.WD, c, trust_clip=True), lr, c, "clipped", ratio_exact=1.0)
    # ... and a ratio below 1 passes the cap unchanged
    small_in = _branch_inputs(1000)
    a, b = _Run(BR_SPECS, small_in).go(step=1000), _Run(BR_SPECS, small_in).go(step=1000, trust_clip=True)
    ra, rb = a.ratios.cpu(), b.ratios.cpu()
    assert torch.equal(_bits(ra), _bits(rb)) and all(r < 1.0 for k, r in enumerate(ra.tolist()) if BR_SIZES[k])


@pytest.mark.parametrize("how", ["host scalar", "hyper block"])
def test_lr_zero_advances_the_moments_and_keeps_p(how):
    inputs = _branch_inputs(1000)
    run = _Run(BR_SPECS, inputs)
    p0 = run.arenas["p"].snapshot()
    c = L.correction(*L.BETAS, 1000)
    run.go(lr=0.0, step=1000) if how == "host scalar" else run.go(lr=5.0, step=1000, hyper=[0.0, 0.0, 1.0, 0.0])
    assert torch.equal(run.arenas["p"].bits, p0)
    ref = L.lamb_ref64(*inputs, 0.0, L.BETAS, L.EPS, L.WD, c)
    _compare(run, ref, 0.0, c, "lr = 0, %s" % how)                             # the moments advanced, the ratios are defined
    assert not torch.equal(run.arenas["m"].tensors_cpu()[3], inputs[2][3])


# ------------------------------------------------------------------------------------------------ 3. bit-identical repeats
def test_two_runs_give_the_same_bits():
    specs, inputs = _case("n97", 1000, 1.0 / 1024)
    a, b = _Run(specs, inputs).go(step=1000, grad_scale=1.0 / 1024), _Run(specs, inputs).go(step=1000, grad_scale=1.0 / 1024)
    assert torch.equal(_bits(a.ratios), _bits(b.ratios)) and torch.equal(_bits(a.partials), _bits(b.partials))
    for s in "pmv":
        assert torch.equal(a.arenas[s].bits, b.arenas[s].bits), s


# ------------------------------------------------------------------------------------------------ 4. the skipped step
FIVE = [3, CHUNK - 1, CHUNK, CHUNK + 1, 4]
OPT_LR = 1e-3


def _five_inputs(seed=4, steps=3):
    g = torch.Generator().manual_seed(seed)
    ps = R.adamw_inputs(FIVE, 1, 1.0, seed)[0]                                   # |p| in [0.5, 2]: the precondition of the bound
    k = 10.0 / sum(FIVE) ** 0.5                                                  # a global norm of about 10: the clip binds
    grads = [[torch.randn(n, generator=g) * k for n in FIVE] for _ in range(steps)]
    return ps, grads


def _holder(ps):
    holder = torch.nn.Module()
    holder.p = torch.nn.ParameterList([torch.nn.Parameter(p.clone().to(DEV)) for p in ps])
    return holder, list(holder.p)


def _groups(params):
    return [{"params": params[:3]}, {"params": params[3:], "weight_decay": 0.0}]


@pytest.mark.parametrize("variant", ["scaler", "clip"])
def test_a_skipped_step_leaves_everything_bit_identical(variant):
    from egovlp_amd.ema import ModelEMA
    from egovlp_amd.optim import LAMB, LossScaler
    ps, grads = _five_inputs()
    holder, params = _holder(ps)
    S = 2.0 ** 10 if variant == "scaler" else 1.0
    scaler = LossScaler(init_scale=S, growth_interval=1000) if variant == "scaler" else None
    opt = LAMB(_groups(params), lr=OPT_LR, max_grad_norm=None if variant == "scaler" else 1.0)
    ema = ModelEMA(holder, decay=0.9, warmup=False)

    def step(gs, poison):
        for p, g in zip(params, gs):
            p.grad = (g * S).to(DEV)
        if poison:
            params[2].grad[CHUNK // 2] = float("inf")
        opt.step(scaler=scaler) if scaler is not None else opt.step()
        ema.update(opt)

    step(grads[0], False)
    assert float(opt.skip_flag()) == 0.0 and ema.num_updates() == 1
    state = lambda: [_bits(p).clone() for p in params] + [_bits(opt.state[p][k]).clone() for p in params for k in ("exp_avg", "exp_avg_sq")] + \
        [_bits(opt._lamb_ratios).clone(), _bits(ema._arena).clone()]
    before = state()
    ratios = opt.trust_ratios()
    assert all(r != 1.0 for r in ratios[:3].tolist()) and ratios[3:].tolist() == [1.0, 1.0]
    step(grads[1], True)
    assert float(opt.skip_flag()) != 0.0
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    assert ema.num_updates() == 1 and ema.skipped_updates() == 1
    if variant == "clip":
        assert opt.nonfinite_steps() == 1
    else:
        assert scaler.skipped_steps() == 1
    step(grads[2], False)                                                        # ... and the next good step is applied
    assert float(opt.skip_flag()) == 0.0 and ema.num_updates() == 2 and not torch.equal(_bits(params[2]), before[2])


# ------------------------------------------------------------------------------------------------ 5. LAMB.step over three steps
@pytest.mark.parametrize("arm", ["scaler+clip", "clip", "neither"])
def test_three_steps_on_two_groups_follow_the_oracle(arm):
    from egovlp_amd.optim import LAMB, LossScaler
    ps, grads = _five_inputs()
    _, params = _holder(ps)
    S = 2.0 ** 10 if arm == "scaler+clip" else 1.0
    scaler = LossScaler(init_scale=S, growth_interval=1000) if arm == "scaler+clip" else None
    opt = LAMB(_groups(params), lr=OPT_LR, max_grad_norm=None if arm == "neither" else 1.0)
    wds = [L.WD] * 3 + [0.0] * 2
    worst = [0.0, 0.0, 0.0, 0.0]
    for t, gs in enumerate(grads, 1):
        for p, g in zip(params, gs):
            p.grad = (g * S).to(DEV)
        # the oracle starts every step from the device's own p, m, v: the single-step bound applies
        p0 = [p.detach().cpu() for p in params]
        m0 = [opt.state[p]["exp_avg"].cpu() if t > 1 else torch.zeros_like(q) for p, q in zip(params, p0)]
        v0 = [opt.state[p]["exp_avg_sq"].cpu() if t > 1 else torch.zeros_like(q) for p, q in zip(params, p0)]
        g0 = [p.grad.cpu() for p in params]
        opt.step(scaler=scaler) if scaler is not None else opt.step()
        gsc = 1.0 / S
        if arm != "neither":
            norm = float(torch.cat(gs).double().norm())
            coef = opt.clip_coef()
            assert abs(coef - 1.0 / (norm + 1e-6)) <= 2e-5 * coef and coef < 0.2                     # the clip binds (NORM_BAR of the clip tests)
            gsc = R.f32(R.f32(1.0 / S) * coef)
        c = L.correction(*L.BETAS, t)
        got_r = opt.trust_ratios()
        for lo, hi, wd in ((0, 3, L.WD), (3, 5, 0.0)):
            ref = L.lamb_ref64(p0[lo:hi], g0[lo:hi], m0[lo:hi], v0[lo:hi], OPT_LR, L.BETAS, L.EPS, wd, c, gsc)
            for k in range(hi - lo):
                p = params[lo + k]
                w = L.check_lamb(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ref, k, p0[lo + k], m0[lo + k], OPT_LR, c,
                                 what="%s step %d tensor %d" % (arm, t, lo + k))
                wr = L.check_ratio(got_r[lo + k], ref["r"][k], what="%s step %d tensor %d" % (arm, t, lo + k))
                if wd == 0.0:
                    assert float(got_r[lo + k]) == 1.0
                worst = [max(a, b) for a, b in zip(worst, w + (wr,))]
        assert opt.state[params[0]]["step"] == t
    assert (opt.skip_flag() is None) == (arm == "neither")
    print("%s: largest err / bound over 3 steps: p %.3f m %.3f v %.3f ratio %.3f" % (arm, *worst))


# ------------------------------------------------------------------------------------------------ 6. the whole EgoClip step
STEP_LR = 1e-4
ZEROED = ["video_model.temporal_embed", "video_model.blocks.0.timeattn.proj.weight", "video_model.blocks.0.timeattn.proj.bias"]
# the tensors of tests/test_gpu_grad_clip.py's step test, and the largest one (30 522 x 768: 1 431 pieces for one workgroup of the ratio kernel)
WATCH = ["video_model.blocks.3.attn.qkv.weight", "text_model.transformer.layer.2.ffn.lin1.weight", "video_model.pos_embed",
         "vid_proj.0.weight", "video_model.blocks.7.norm3.bias", "text_model.embeddings.word_embeddings.weight"]


@pytest.fixture(scope="module")
def real():
    """The 4-frame base_patch16_224 model of tests/test_gpu_grad_clip.py's step test with synthetic weights -- three tensors zeroed, as
    the shipped initialisation leaves the time attention and temporal_embed -- and its B = 4, L = 16 batch on the device."""
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=3)
    for k in ZEROED:
        sd[k] = torch.zeros_like(sd[k])
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    m = m.cuda().train()
    batch = synth_batch(4, T=4, L=16, seed=12, ragged=True)
    dev = {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
           "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}
    yield m, sd, dev
    Precision.set("bf16x3")


@pytest.mark.parametrize("chunk", [None, 2], ids=["plain", "cached"])
def test_whole_egoclip_step(real, chunk):
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import LAMB
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    m, sd, dev = real
    try:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()
        named = [(k, p) for k, p in m.named_parameters()]
        opt = LAMB([p for _, p in named], lr=STEP_LR)
        loss = egoclip_step(m, EgoNCE(), opt, dev) if chunk is None else egoclip_step_cached(m, EgoNCE(), opt, dev, chunk)
        assert bool(torch.isfinite(loss)) and float(opt.skip_flag()) == 0.0
        with_grad = [(k, p) for k, p in named if p.grad is not None]
        assert len(with_grad) > 300 and all(k in dict(with_grad) for k in ZEROED)
        ratios = opt.trust_ratios()
        assert ratios.numel() == len(with_grad)
        c = L.correction(*L.BETAS, 1)
        gsc = R.f32(opt.clip_coef())
        worst = [0.0, 0.0, 0.0, 0.0]
        assert all(k in dict(with_grad) for k in WATCH)
        for i, (k, p) in enumerate(with_grad):
            # every tensor with a gradient moved (compared on the device) ...
            assert not torch.equal(p.detach().reshape(-1), sd[k].to(DEV).reshape(-1)), "%s did not move" % k
            if k not in WATCH + ZEROED:
                continue
            # ... and the watched ones (the fp64 oracle over all 180.9 M parameters would take a minute on the host) follow the oracle
            p0 = sd[k].reshape(-1)
            zero = torch.zeros_like(p0)
            ref = L.lamb_ref64([p0], [p.grad.cpu()], [zero], [zero], STEP_LR, L.BETAS, L.EPS, opt.defaults["weight_decay"], c, gsc)
            w = L.check_lamb(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], ref, 0, p0, zero, STEP_LR, c, what=k)
            wr = L.check_ratio(ratios[i], ref["r"][0], what=k)
            worst = [max(a, b) for a, b in zip(worst, w + (wr,))]
            if k in ZEROED:
                assert float(ratios[i]) == 1.0
        print("%s: loss %.6f, coef %.4f, %d tensors, ratios %.3g .. %.3g, largest err / bound: p %.3f m %.3f v %.3f ratio %.3f" % (
            "cached" if chunk else "plain", float(loss), gsc, len(with_grad), float(ratios.min()), float(ratios.max()), *worst))
    finally:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()


# ------------------------------------------------------------------------------------------------ 7. the trainer
CFG = {"name": "EgoClip_4f", "n_gpu": 1,
       "arch": {"type": "FrozenInTime", "args": {
           "video_params": {"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                            "pretrained": True, "time_init": "rand"},
           "text_params": {"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
           "projection": "minimal", "load_checkpoint": ""}},
       "optimizer": {"type": "LAMB", "args": {"lr": 1e-4, "trust_clip": True}},
       "loss": {"type": "EgoNCE", "args": {}},
       "metrics": ["egomcq_accuracy_metrics"],
       "trainer": {"epochs": 1, "max_samples_per_epoch": 500000, "save_dir": "unused", "save_period": 1, "verbosity": 2,
                   "monitor": "off", "init_val": False, "neptune": False}}


class _Loader:
    """Two batches of B clips with tokenised captions."""
    dataset_name = "EgoClip-synthetic"

    def __init__(self, B, n_batches=2):
        self.batch_size, self.n_batches, self.n_samples = B, n_batches, B * n_batches

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            b = synth_batch(self.batch_size, T=2, L=8, seed=50 + i)
            yield {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


def _questions():
    """Two EgoMCQ questions, one of each type (the epoch's validation needs both)."""
    g = torch.Generator().manual_seed(99)
    out = []
    for q in range(2):
        ids = torch.randint(1000, 30000, (1, 16), generator=g)
        ids[:, 0] = 101
        mask = torch.ones(1, 16, dtype=torch.long)
        mask[:, 10 + q:] = 0
        out.append({"video": torch.randn(1, 5, 4, 3, 224, 224, generator=g), "text": {"input_ids": ids, "attention_mask": mask},
                    "correct": torch.tensor([q % 5]), "type": torch.tensor([1 + q % 2])})
    return out


class _ValLoader(list):
    batch_size = 1
    dataset_name = "EgoMCQ-synthetic"


def _make_trainer(tmp, resume=None):
    import egovlp_amd.model.loss as module_loss
    import egovlp_amd.model.model as module_arch
    import egovlp_amd.optim as module_optim
    from egovlp_amd.model.metric import egomcq_accuracy_metrics
    from egovlp_amd.ops import Precision
    from egovlp_amd.trainer.trainer_egoclip import Multi_Trainer_dist
    from egovlp_amd.utils.config import DictConfig
    Precision.set("bf16x3")
    config = DictConfig(CFG, save_dir=tmp, resume=resume)
    model = config.initialize('arch', module_arch)
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=2))
    model.text_model.set_dropout(0.0, 0.0)
    loss = config.initialize(name="loss", module=module_loss)
    optimizer = config.initialize('optimizer', module_optim, filter(lambda p: p.requires_grad, model.parameters()))
    args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=1e-4, schedule=[60, 80])
    return Multi_Trainer_dist(args, model, loss, [egomcq_accuracy_metrics], optimizer, config=config, data_loader=[_Loader(2)],
                              valid_data_loader=[_ValLoader(_questions())], tokenizer=None,
                              max_samples_per_epoch=CFG['trainer']['max_samples_per_epoch'])


def test_trainer_runs_lamb_from_the_config_and_resumes_it(tmp_path):
    from egovlp_amd.optim import LAMB
    tr = _make_trainer(tmp_path / "run1")
    assert type(tr.optimizer) is LAMB and tr.optimizer.param_groups[0]["trust_clip"] is True
    tr.train()
    opt = tr.optimizer
    params = [p for g in opt.param_groups for p in g["params"]]
    assert all(opt.state[p]["step"] == 2 for p in params if p in opt.state) and len(opt.state) > 300
    ratios = opt.trust_ratios()
    assert ratios.numel() == len(opt.state) and float(ratios.max()) <= 1.0 and float(ratios.min()) > 0.0
    path = str(tmp_path / "run1" / "checkpoint-epoch1.pth")
    assert os.path.exists(path)
    tr2 = _make_trainer(tmp_path / "run2", resume=path)
    opt2 = tr2.optimizer
    assert type(opt2) is LAMB and tr2.start_epoch == 2 and opt2.max_grad_norm == opt.max_grad_norm
    assert [{k: v for k, v in g.items() if k != "params"} for g in opt2.param_groups] == \
        [{k: v for k, v in g.items() if k != "params"} for g in opt.param_groups]
    params2 = [p for g in opt2.param_groups for p in g["params"]]
    # the same gradients into both: the resumed optimizer's next step is the uninterrupted one, bit for bit
    gen = torch.Generator().manual_seed(8)
    for p, q in zip(params, params2):
        assert torch.equal(_bits(p), _bits(q))
        g = (torch.randn(p.shape, generator=gen) * 1e-3).to(DEV) if p in opt.state else None
        p.grad, q.grad = g, (None if g is None else g.clone())
    opt.step()
    opt2.step()
    assert torch.equal(_bits(opt.trust_ratios()), _bits(opt2.trust_ratios()))
    for p, q in zip(params, params2):
        assert torch.equal(_bits(p), _bits(q))
        if p in opt.state:
            assert opt2.state[q]["step"] == 3
            assert torch.equal(_bits(opt.state[p]["exp_avg"]), _bits(opt2.state[q]["exp_avg"]))
            assert torch.equal(_bits(opt.state[p]["exp_avg_sq"]), _bits(opt2.state[q]["exp_avg_sq"]))
