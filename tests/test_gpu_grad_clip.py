"""Gradient clipping by global norm on a real MI355X (`pytest -m gpu`): egv_grad_sqnorm_multi / egv_grad_clip_update at their table and
block boundaries, and `AdamW(max_grad_norm=...)` around them -- with and without a loss scale, with two parameter groups, and in the
whole EgoClip step (plain and cached) -- against torch.nn.utils.clip_grad_norm_ + the oracle's AdamW on fp32 CPU copies.

Bound of the norm (derived, not measured): all terms of sum(g * g) are >= 0, and each faces at most 256 sequential lane additions
plus 8 tree levels of 2^-24 each inside a block -> 1.6e-5 relative on a partial and on their sum (the partials are summed in double),
half that on the root: NORM_BAR = 2e-5.  The AdamW tolerance is test_adamw_matches_transformers_4_2_1_semantics's (1e-6)."""
import ctypes as C
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

DEV = "cuda"
BLOCK = 65536                    # elements per block of the reduction (4 * CHUNK)
NORM_BAR = 2e-5
ADAMW_BAR = 1e-6
SENTINEL = -7.0                  # no sum of squares is negative
EDGE_SIZES = [1, 3, 4, BLOCK - 1, BLOCK, BLOCK + 1]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _h():
    from egovlp_amd import _lib
    return _lib.lib()


def _stream():
    from egovlp_amd import ops
    return ops._stream()


def _norm64(tensors):
    return math.sqrt(sum(float((t.detach().double().cpu() ** 2).sum()) for t in tensors))


def _boundary_list(g):
    """1, 3, 4, 65 535, 65 536, 65 537 elements; a view one float behind a 16-byte boundary (the scalar path, more than one block); an
    aligned base with n % 4 != 0 (16-byte body + scalar tail); an empty tensor in the middle."""
    ts = [torch.randn(n, generator=g).to(DEV) for n in EDGE_SIZES]
    odd = torch.randn(BLOCK + 1030, generator=g).to(DEV)[1:]
    tail = torch.randn(4 * 300 + 3, generator=g).to(DEV)
    assert odd.data_ptr() % 16 == 4 and tail.data_ptr() % 16 == 0 and tail.numel() % 4 == 3
    return ts[:3] + [torch.empty(0, device=DEV)] + ts[3:] + [odd, tail]


def _many(count, g):
    """`count` small tensors of mixed sizes and alignments, one of them more than a block long and placed behind the first table."""
    buf = torch.randn(count * 400 + 8, generator=g).to(DEV)
    out, at = [], 0
    for i in range(count):
        n = 1 + (i * 37) % 300
        out.append(buf[at:at + n])
        at += n
    out[96] = torch.randn(BLOCK + 5, generator=g).to(DEV)
    return out


def _expected_parts(tensors):
    return sum((t.numel() + BLOCK - 1) // BLOCK for t in tensors)


def _sqnorm_raw(tensors, capacity_delta=0, state=None):
    """egv_grad_sqnorm_multi through the C ABI into a sentinel-filled buffer one slot longer than the count -> (rc, parts, buffer)."""
    n = len(tensors)
    G = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    N = (C.c_int64 * n)(*[t.numel() for t in tensors])
    parts = _h().egv_grad_sqnorm_parts(n, N)
    buf = torch.full((parts + 1,), SENTINEL, dtype=torch.float32, device=DEV)
    rc = _h().egv_grad_sqnorm_multi(n, G, N, buf.data_ptr(), parts + capacity_delta, state.data_ptr() if state is not None else None,
                                    _stream())
    torch.cuda.synchronize()
    return rc, parts, buf


def _decide(buf, parts, max_norm, grad_scale=1.0):
    """egv_grad_clip_update without a scaler, one hyper block -> (norm block on the host, hyper block on the host)."""
    from egovlp_amd import ops
    nb = torch.zeros(8, dtype=torch.int32, device=DEV)
    hyper = torch.zeros(4, dtype=torch.float32, device=DEV)
    ops.grad_clip_update(buf, parts, nb, max_norm, [hyper], grad_scale=grad_scale, lrs=[1e-3], step_sizes=[2e-3])
    torch.cuda.synchronize()
    return nb.cpu(), hyper.cpu()


@pytest.mark.parametrize("which", ["boundaries", "97 tensors", "193 tensors"])
def test_norm_kernel_at_its_boundaries(which):
    """Block edges, the scalar path, a tail, an empty tensor; 97 and 193 tensors cross the 96-tensor table once and twice (two and three
    launches, the partial index carried over).  Norm within NORM_BAR of the fp64 norm, bit-identical between two runs, exactly
    egv_grad_sqnorm_parts partials written (the slot behind them keeps its sentinel)."""
    from egovlp_amd.optim import clip_coefficient
    g = torch.Generator().manual_seed(11)
    ts = _boundary_list(g) if which == "boundaries" else _many(97 if which.startswith("97") else 193, g)
    ref = _norm64(ts)
    blocks = []
    for run in range(2):
        rc, parts, buf = _sqnorm_raw(ts)
        assert rc == 0 and parts == _expected_parts(ts)
        host = buf.cpu()
        assert bool((host[:parts] >= 0).all()) and float(host[parts]) == SENTINEL
        nb, hyper = _decide(buf, parts, max_norm=0.5 * ref)
        blocks.append((nb, hyper, host))
    nb, hyper, host = blocks[0]
    norm, coef = float(nb.view(torch.float32)[0]), float(nb.view(torch.float32)[1])
    err = abs(norm - ref) / ref
    print("%s: %d tensors, %d partials, norm %.9g fp64 %.9g rel %.2e (bar %.0e)" % (which, len(ts), parts, norm, ref, err, NORM_BAR))
    assert err <= NORM_BAR
    assert all(torch.equal(a, b) for a, b in zip(blocks[0], blocks[1]))                     # the same bits, run after run
    # every partial is the sum of squares of ITS block: list order, tensor by tensor, block by block
    k = 0
    for t in ts:
        for at in range(0, t.numel(), BLOCK):
            want = float((t[at:at + BLOCK].double() ** 2).sum())
            assert abs(float(host[k]) - want) <= 1.6e-5 * want, (k, t.numel(), at)
            k += 1
    assert k == parts
    assert abs(coef - clip_coefficient(norm, 0.5 * ref)) <= 1e-6 and int(nb[2]) == 0 and int(nb[3]) == 1 and int(nb[4]) == 0
    assert hyper.tolist() == [pytest.approx(1e-3), pytest.approx(2e-3), coef, 0.0]          # {lr, step size, grad_scale * coef, skip}


def test_norm_kernel_arguments():
    """A capacity below the count is an invalid argument and launches nothing; so are a negative size and a NULL pointer of a non-empty
    tensor; an empty list writes nothing; with a scaler state the same pass sets the found-inf flag."""
    g = torch.Generator().manual_seed(12)
    ts = _boundary_list(g)
    rc, parts, buf = _sqnorm_raw(ts, capacity_delta=-1)
    assert rc == 1 and bool((buf.cpu() == SENTINEL).all())
    h = _h()
    P1, N1 = (lambda p: (C.c_void_p * 1)(p)), (lambda n: (C.c_int64 * 1)(n))
    out = torch.full((4,), SENTINEL, device=DEV)
    a = torch.ones(8, device=DEV)
    assert h.egv_grad_sqnorm_parts(1, N1(-4)) == -1 and h.egv_grad_sqnorm_parts(-1, None) == -1 and h.egv_grad_sqnorm_parts(0, None) == 0
    assert h.egv_grad_sqnorm_multi(1, P1(a.data_ptr()), N1(-4), out.data_ptr(), 4, None, _stream()) == 1
    assert h.egv_grad_sqnorm_multi(1, P1(None), N1(8), out.data_ptr(), 4, None, _stream()) == 1
    assert h.egv_grad_sqnorm_multi(1, P1(a.data_ptr()), N1(8), None, 4, None, _stream()) == 1
    assert h.egv_grad_sqnorm_multi(0, None, None, None, 0, None, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())
    assert h.egv_grad_sqnorm_multi(1, P1(a.data_ptr()), N1(8), out.data_ptr(), 1, None, _stream()) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [8.0, SENTINEL, SENTINEL, SENTINEL]
    # the scan rides along: no flag on finite gradients, the flag on one inf (a value, as in the loss-scale tests)
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc, parts, buf = _sqnorm_raw(ts, state=state)
    assert rc == 0 and int(state[2]) == 0
    ts[5][BLOCK - 3] = float("inf")
    rc, parts, buf = _sqnorm_raw(ts, state=state)
    assert rc == 0 and int(state[2]) == 1
    nb, _ = _decide(buf, parts, 1.0)
    assert int(nb[2]) == 1 and float(nb.view(torch.float32)[1]) == 0.0 and int(nb[4]) == 1 and int(nb[3]) == 0


# ------------------------------------------------------------------------------------------------------------- the optimizer
SIZES = [3, BLOCK - 1, BLOCK, BLOCK + 1, 4]
MAX_NORM = 1.0
LR, WD = 1e-2, 0.01


def _inputs(seed=4, steps=3):
    """Initial parameters and `steps` gradient lists whose global norm is about 10 x MAX_NORM (CPU fp32)."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) for n in SIZES]
    k = 10.0 * MAX_NORM / math.sqrt(sum(SIZES))
    grads = [[torch.randn(n, generator=g) * k for n in SIZES] for _ in range(steps)]
    return ps, grads


_REF = {}


def _reference(lrs=(LR, LR, LR, LR, LR)):
    """clip_grad_norm_ on fp32 CPU copies, then the oracle's AdamW (transformers 4.2.1), 3 steps -> (parameters, norms, coefs)."""
    if lrs not in _REF:
        from egovlp_amd.optim import clip_coefficient
        ps, grads = _inputs()
        ref_p = [torch.nn.Parameter(p.clone()) for p in ps]
        ref_m = [torch.zeros_like(p) for p in ps]
        ref_v = [torch.zeros_like(p) for p in ps]
        norms, coefs = [], []
        for step, gs in enumerate(grads, 1):
            for p, gr in zip(ref_p, gs):
                p.grad = gr.clone()
            norms.append(_norm64(gs))
            coefs.append(clip_coefficient(norms[-1], MAX_NORM))
            torch.nn.utils.clip_grad_norm_(ref_p, MAX_NORM)
            with torch.no_grad():
                for p, m, v, lr in zip(ref_p, ref_m, ref_v, lrs):
                    O.adamw_step(p, p.grad, m, v, step, lr=lr, weight_decay=WD)
        _REF[lrs] = ([p.detach() for p in ref_p], norms, coefs)
    return _REF[lrs]


def _run(opt_kwargs, scale=1.0, scaler=None, groups=None, grads=None):
    """3 steps of the device optimizer on _inputs() (gradients times `scale`) -> (optimizer, parameters, per-step norms, coefs)."""
    from egovlp_amd.optim import AdamW
    ps, gl = _inputs()
    gl = grads if grads is not None else gl
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    arg = params if groups is None else [{"params": [params[i] for i in idx], "lr": lr} for idx, lr in groups]
    opt = AdamW(arg, lr=LR, weight_decay=WD, **opt_kwargs)
    norms, coefs = [], []
    for gs in gl:
        for p, gr in zip(params, gs):
            p.grad = (gr * scale).to(DEV)
        opt.step(scaler=scaler) if scaler is not None else opt.step()
        if opt.max_grad_norm is not None:
            norms.append(opt.grad_norm())
            coefs.append(opt.clip_coef())
    return opt, params, norms, coefs


def test_clipped_update_matches_clip_grad_norm_and_the_oracle_adamw():
    from egovlp_amd.optim import clip_coefficient
    ref_p, ref_norms, ref_coefs = _reference()
    opt, params, norms, coefs = _run({"max_grad_norm": MAX_NORM})
    assert 9.0 < ref_norms[0] < 11.0
    for got, want in zip(norms, ref_norms):
        assert abs(got - want) <= NORM_BAR * want
    for got, n in zip(coefs, norms):
        assert abs(got - clip_coefficient(n, MAX_NORM)) <= 1e-6 * got
    for p, r in zip(params, ref_p):
        assert rel(p, r) < ADAMW_BAR
    assert opt.clipped_steps() == 3 and opt.nonfinite_steps() == 0


def test_a_clip_that_does_not_bind_changes_nothing():
    """max_grad_norm = 1e30: coef = 1.  With a LossScaler both optimizers read the device hyper block and x * 1.0f is exact: parameters,
    moments and scaler state bit for bit.  Without one the hyper block replaces the host's step size (host and device pow may differ in
    the last place): the AdamW tolerance."""
    from egovlp_amd.optim import LossScaler
    S = 2.0 ** 10
    sc_a, sc_b = LossScaler(init_scale=S, growth_interval=2), LossScaler(init_scale=S, growth_interval=2)
    opt_a, pa, _, coefs = _run({"max_grad_norm": 1e30}, scale=S, scaler=sc_a)
    opt_b, pb, _, _ = _run({}, scale=S, scaler=sc_b)
    assert coefs == [1.0, 1.0, 1.0] and opt_a.clipped_steps() == 0 and opt_a.nonfinite_steps() == 0
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[a][key].view(torch.int32), opt_b.state[b][key].view(torch.int32)), key
    assert torch.equal(sc_a.state, sc_b.state) and sc_a.get_scale() == 2 * S             # the scale grew once in 3 steps, in both
    opt_c, pc, _, coefs_c = _run({"max_grad_norm": 1e30})
    opt_d, pd, _, _ = _run({})
    assert coefs_c == [1.0, 1.0, 1.0] and opt_c.clipped_steps() == 0
    for c, d in zip(pc, pd):
        assert rel(c, d) < ADAMW_BAR


def test_loss_scaled_gradients_report_the_unscaled_norm_and_an_overflow_skips_the_step():
    from egovlp_amd.optim import LossScaler
    S = 2.0 ** 16
    ref_p, ref_norms, ref_coefs = _reference()
    sc = LossScaler(init_scale=S, growth_interval=1000)
    opt, params, norms, coefs = _run({"max_grad_norm": MAX_NORM}, scale=S, scaler=sc)
    for got, want in zip(norms, ref_norms):
        assert abs(got - want) <= NORM_BAR * want                                      # the UN-scaled norm
    for p, r in zip(params, ref_p):
        assert rel(p, r) < ADAMW_BAR                                                   # the update of the un-scaled case
    assert opt.clipped_steps() == 3 and sc.get_scale() == S and sc.skipped_steps() == 0
    # one inf in one gradient (the project's forced-overflow input): nothing moves, S halves, coef = 0, the clip counter stays
    before = [p.detach().clone() for p in params]
    _, gl = _inputs()
    for p, gr in zip(params, gl[0]):
        p.grad = (gr * S).to(DEV)
    params[2].grad[BLOCK // 2] = float("inf")
    opt.step(scaler=sc)
    for p, b in zip(params, before):
        assert torch.equal(p.detach().view(torch.int32), b.view(torch.int32))
    assert sc.get_scale() == S / 2 and sc.skipped_steps() == 1
    assert opt.clip_coef() == 0.0 and opt.clipped_steps() == 3 and opt.nonfinite_steps() == 1
    # and the step after it is applied again, at the new scale
    for p, gr in zip(params, gl[1]):
        p.grad = (gr * (S / 2)).to(DEV)
    opt.step(scaler=sc)
    assert abs(opt.grad_norm() - ref_norms[1]) <= NORM_BAR * ref_norms[1] and opt.clipped_steps() == 4
    assert not torch.equal(params[2].detach(), before[2])
    # without a scaler the same input is NOT applied either (the stated deviation from clip_grad_norm_, which would write NaN)
    opt2, params2, _, _ = _run({"max_grad_norm": MAX_NORM}, grads=gl[:1])
    before2 = [p.detach().clone() for p in params2]
    for p, gr in zip(params2, gl[1]):
        p.grad = gr.to(DEV)
    params2[2].grad[BLOCK // 2] = float("inf")
    opt2.step()
    for p, b in zip(params2, before2):
        assert torch.equal(p.detach().view(torch.int32), b.view(torch.int32))
        assert bool(torch.isfinite(opt2.state[p]["exp_avg"]).all())
    assert opt2.nonfinite_steps() == 1 and opt2.clipped_steps() == 1 and opt2.clip_coef() == 0.0


@pytest.mark.parametrize("scaled", [False, True], ids=["no scaler", "scaler"])
def test_two_parameter_groups_share_the_global_coefficient(scaled):
    from egovlp_amd.optim import LossScaler, adamw_step_size, clip_coefficient
    lr0, lr1 = 1e-2, 1e-3
    groups = [([0, 1, 2], lr0), ([3, 4], lr1)]
    ref_p, ref_norms, _ = _reference((lr0, lr0, lr0, lr1, lr1))
    S = 2.0 ** 12 if scaled else 1.0
    sc = LossScaler(init_scale=S, growth_interval=1000) if scaled else None
    opt, params, norms, coefs = _run({"max_grad_norm": MAX_NORM}, scale=S, scaler=sc, groups=groups)
    for got, want in zip(norms, ref_norms):
        assert abs(got - want) <= NORM_BAR * want                       # the norm over BOTH groups, not a group's
    for p, r in zip(params, ref_p):
        assert rel(p, r) < ADAMW_BAR
    blocks = [sc.hyper_block(0), sc.hyper_block(1)] if scaled else [opt._clip_hyper[0], opt._clip_hyper[1]]
    h0, h1 = (b.cpu().tolist() for b in blocks)
    want = torch.tensor(1.0 / S, dtype=torch.float32) * torch.tensor(coefs[-1], dtype=torch.float32)
    assert h0[2] == h1[2] == float(want) and h0[3] == h1[3] == 0.0       # ONE coefficient, the global one, in both blocks
    assert abs(coefs[-1] - clip_coefficient(ref_norms[-1], MAX_NORM)) <= 2 * NORM_BAR * coefs[-1]
    assert h0[0] == pytest.approx(lr0, rel=1e-7) and h1[0] == pytest.approx(lr1, rel=1e-7)
    # the step size as every entry point of csrc/adamw.hip computes it: in double, from the fp32 roundings of lr and the betas (their C
    # arguments are floats; 1 - beta2^3 at fp32(0.999) is 1.3e-5 away from its value at the double 0.999)
    f32 = lambda x: C.c_float(x).value
    for h, lr in ((h0, lr0), (h1, lr1)):
        assert h[1] == pytest.approx(adamw_step_size(f32(lr), f32(0.9), f32(0.999), 3), rel=1e-6)
    assert opt.clipped_steps() == 3


# ------------------------------------------------------------------------------------------------------------- the whole step
WATCH = ["video_model.blocks.3.attn.qkv.weight", "text_model.transformer.layer.2.ffn.lin1.weight", "video_model.pos_embed",
         "vid_proj.0.weight", "video_model.blocks.7.norm3.bias"]
PARITY = 1e-3
GRAD_BAR = {"bf16x3": 3e-3, "f16mix": 1e-2}          # the gradient bars of tests/test_gpu_cached_step.py, which bound the norm too
UPDATE_BAR = {"bf16x3": 2e-2, "f16mix": 1.5e-1}      # test_train_step_matches_oracle: fp32-grade / single-pass backward
STEP_LR = 3e-5


@pytest.fixture(scope="module")
def stepped():
    """The 4-frame model, a B = 4 batch, and ONE oracle step on the CPU: loss, the global gradient norm, max_grad_norm = half of it
    (so that the clip binds, coef ~ 0.5) and the clipped AdamW update of the watched tensors."""
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import clip_coefficient
    Precision.set("bf16x3")
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=3)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    m = m.cuda().train()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    batch = synth_batch(4, T=4, L=16, seed=12, ragged=True)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    te, ve = O.frozen_in_time(batch, sdo, O.VideoCfg(num_frames=4), O.TextCfg())
    ref, _ = O.egoclip_loss(te, ve, batch["noun_vec"], batch["verb_vec"])
    ref.backward()
    named = [(k, v) for k, v in sdo.items() if v.grad is not None]
    norm = _norm64([v.grad for _, v in named])
    max_norm = 0.5 * norm
    ps = [torch.nn.Parameter(v.detach().clone()) for _, v in named]
    for p, (_, v) in zip(ps, named):
        p.grad = v.grad.clone()
    torch.nn.utils.clip_grad_norm_(ps, max_norm)
    upd = {}
    for p, (k, v) in zip(ps, named):
        if k in WATCH:
            q = v.detach().clone()
            O.adamw_step(q, p.grad, torch.zeros_like(q), torch.zeros_like(q), 1, lr=STEP_LR)
            upd[k] = q - sd[k]
    dev = {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
           "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}
    yield m, sd, dev, float(ref.detach()), norm, max_norm, clip_coefficient(norm, max_norm), upd
    Precision.set("bf16x3")


def _one_step(m, sd, dev, mode, max_norm, chunk=None):
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    Precision.set("f16mix", "f16") if mode == "f16mix" else Precision.set(mode)
    try:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()
        opt = AdamW(m.parameters(), lr=STEP_LR, max_grad_norm=max_norm)
        loss = egoclip_step(m, EgoNCE(), opt, dev) if chunk is None else egoclip_step_cached(m, EgoNCE(), opt, dev, chunk)
        new = {k: p.detach().cpu() for k, p in m.named_parameters() if k in WATCH}
        return float(loss), opt, new
    finally:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()
        Precision.set("bf16x3")


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix"])
def test_whole_step_clips_like_the_oracle_step_with_clip_grad_norm(stepped, mode):
    """egoclip_step with a binding max_grad_norm against the CPU oracle step with clip_grad_norm_ before its optimizer.  Loss at the
    parity bar; the norm is a function of the gradients, so it carries the mode's gradient bar; the update carries the bar of
    test_train_step_matches_oracle for the kind of backward.  'f16mix' is the fp16 backward under the model's own loss scale: the norm
    read back is the un-scaled one."""
    m, sd, dev, ref_loss, ref_norm, max_norm, ref_coef, upd_ref = stepped
    loss, opt, new = _one_step(m, sd, dev, mode, max_norm)
    norm, coef = opt.grad_norm(), opt.clip_coef()
    print("%s: loss %.6f oracle %.6f | norm %.6g oracle %.6g rel %.2e | coef %.6f oracle %.6f" % (
        mode, loss, ref_loss, norm, ref_norm, abs(norm - ref_norm) / ref_norm, coef, ref_coef))
    assert abs(loss - ref_loss) < PARITY * abs(ref_loss)
    assert abs(norm - ref_norm) <= GRAD_BAR[mode] * ref_norm
    assert abs(coef - ref_coef) <= 2 * GRAD_BAR[mode] * ref_coef and coef < 0.6
    assert opt.clipped_steps() == 1 and opt.nonfinite_steps() == 0
    for k in WATCH:
        r = rel(new[k] - sd[k], upd_ref[k])
        print("  %s clipped update %-55s rel %.2e (bar %.1e)" % (mode, k, r, UPDATE_BAR[mode]))
        assert r < UPDATE_BAR[mode], k


def test_cached_step_clips_once_on_the_summed_gradients(stepped):
    """chunk = half the batch: the norm is that of the SUMMED chunk gradients -- the plain step's, within the two gradient bars the
    cached-step tests allow between the two steps -- and the step is clipped once."""
    m, sd, dev, ref_loss, ref_norm, max_norm, ref_coef, _ = stepped
    _, opt_p, new_p = _one_step(m, sd, dev, "bf16x3", max_norm)
    _, opt_c, new_c = _one_step(m, sd, dev, "bf16x3", max_norm, chunk=2)
    n_p, n_c = opt_p.grad_norm(), opt_c.grad_norm()
    print("norm plain %.6g cached %.6g rel %.2e" % (n_p, n_c, abs(n_p - n_c) / n_p))
    assert abs(n_p - n_c) <= 2 * GRAD_BAR["bf16x3"] * n_p
    assert opt_c.clipped_steps() == 1 and abs(opt_c.clip_coef() - opt_p.clip_coef()) <= 2 * GRAD_BAR["bf16x3"] * opt_p.clip_coef()
    for k in WATCH:
        assert rel(new_c[k] - sd[k], new_p[k] - sd[k]) < 2 * UPDATE_BAR["bf16x3"], k
