"""The EgoNCE head with a queue of past embeddings (egv_egonce_queue_fwd_bwd / _push, egovlp_amd/csrc/egonce_long.hip) on a real MI355X
(`pytest -m gpu`) against the fp64 oracle with autograd (tests/egonce_queue_ref.py), at the smallest sizes at which each thing can
break: a single anchor, tile edges, a validity edge inside a queue tile next to a wholly unused tile, more than one column range, a
batch past the short head's cap; every mask mode, the operand map, the learnable scale, determinism, the ring (wrap, overwritten
slots), the poison rule, the loss modules and the two EgoClip steps.

Bars (the project's for these heads): loss < 1e-4 max(1, |ref|), gradients rel-L2 < 1e-4, dL/ds |diff| < 1e-4 max(1, |ref|).
Unused slots of a hand-filled queue hold NaN rows and all-ones words: anything that reads them shows."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import egonce_long_ref as R  # noqa: E402
import egonce_queue_ref as QR  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

LOSS_BAR = 1e-4
GRAD_BAR = 1e-4


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import loss_ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


_INPUTS, _ORACLE = {}, {}


def inputs(n, Q, D=256):
    if (n, Q, D) not in _INPUTS:
        _INPUTS[(n, Q, D)] = QR.split_inputs(n, Q, D, seed=n + Q)
    return _INPUTS[(n, Q, D)]


def oracle(n, Q, K, D=256, kind="ego", use_noun=True, use_verb=True, logit_scale=None):
    """fp64 oracle on the shared inputs, computed once -> (loss, d_text, d_video, d_logit_scale, batch x queue mask)"""
    key = (n, Q, K, D, kind, use_noun, use_verb, logit_scale)
    if key not in _ORACLE:
        batch, queue = inputs(n, Q, D)
        if kind == "nsl":
            batch, queue = batch[:2] + (None, None), queue[:2] + (None, None)
        _ORACLE[key] = QR.oracle(O, *batch, *queue, K, use_noun=use_noun, use_verb=use_verb, logit_scale=logit_scale)
    return _ORACLE[key]


def words_i32(noun, verb):
    "the kernels' packed rows: the noun words, then the verb words, as int32 bit patterns"
    w = torch.cat([R.pack_bits(noun), R.pack_bits(verb)], 1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def device_queue(ops, Q, D, q_text, q_video, q_noun, q_verb, K, head=None):
    """an EgonceQueue whose slots 0 .. K - 1 hold the given rows; the others NaN rows and all-ones words"""
    vec = q_noun is not None
    q = ops.EgonceQueue(Q, D, q_noun.shape[1] if vec else 0, q_verb.shape[1] if vec else 0, "cuda")
    q.text.fill_(float("nan"))
    q.video.fill_(float("nan"))
    q.words.fill_(-1)
    q.text[:K] = 0.0
    q.video[:K] = 0.0
    q.text[:K, :D] = q_text[:K].float().cuda()
    q.video[:K, :D] = q_video[:K].float().cuda()
    if vec:
        assert q.W == words_i32(q_noun[:1], q_verb[:1]).shape[1]
        q.words[:K] = words_i32(q_noun[:K], q_verb[:K]).cuda()
    q.state.copy_(torch.tensor([K % Q if head is None else head, K], dtype=torch.int32))
    return q


def run_queue(ops, batch, q, temperature=0.05, **kw):
    "-> (loss, d_text, d_video[, d_logit_scale]) on the host; the work buffer is dropped"
    c = lambda t: None if t is None else t.cuda()
    out = ops.egonce_queue_fwd_bwd(c(batch[0]), c(batch[1]), c(batch[2]), c(batch[3]), temperature, q, **kw)
    return (float(out[0]),) + tuple(None if t is None else t.cpu() for t in out[1:-1])


def check(tag, got, ref, loss_bar=LOSS_BAR, grad_bar=GRAD_BAR):
    loss, dt, dv = got[:3]
    rl = float(ref[0])
    el, et, ev = abs(loss - rl), R.rel(dt, ref[1]), R.rel(dv, ref[2])
    print("%s: loss %.7f oracle %.7f |diff| %.2e (bar %.1e); d_text rel %.2e d_video rel %.2e (bar %.1e)" % (
        tag, loss, rl, el, loss_bar * max(1.0, abs(rl)), et, ev, grad_bar))
    assert el < loss_bar * max(1.0, abs(rl)), (tag, el)
    assert et < grad_bar and ev < grad_bar, (tag, et, ev)
    if len(got) > 3:
        rs = float(ref[3])
        es = abs(float(got[3]) - rs)
        print("%s: d_logit_scale %.7f oracle %.7f |diff| %.2e (bar %.1e)" % (tag, float(got[3]), rs, es, LOSS_BAR * max(1.0, abs(rs))))
        assert es < LOSS_BAR * max(1.0, abs(rs)), (tag, es)


def density_ok(tag, mq):
    dens = float(mq.double().mean())
    print("%s: batch x queue mask density %.4f, anchors with a queue positive %.2f" % (tag, dens, float(mq.any(1).double().mean())))
    assert 0.01 <= dens <= 0.50              # a mask of all ones or all zeros would hide a mask bug


# a single anchor; tile edges; a validity edge inside a queue tile and a wholly unused tile; more than one column range; past the
# short head's cap
@pytest.mark.parametrize("n,Q,K", [(1, 64, 64), (63, 64, 64), (64, 64, 64), (65, 128, 128), (64, 192, 100), (129, 1024, 1000),
                                   (1025, 2048, 2048)])
def test_queue_head_matches_the_oracle(ops, n, Q, K):
    batch, queue = inputs(n, Q)
    ref = oracle(n, Q, K)
    tag = "n=%d Q=%d filled=%d" % (n, Q, K)
    density_ok(tag, ref[4])
    check(tag, run_queue(ops, batch, device_queue(ops, Q, 256, *queue, K)), ref)


@pytest.mark.parametrize("D", [132, 4])
def test_narrow_rows(ops, D):
    n, Q = 65, 128
    batch, queue = inputs(n, Q, D)
    ref = oracle(n, Q, Q, D)
    density_ok("D=%d" % D, ref[4])
    check("n=65 Q=128 D=%d" % D, run_queue(ops, batch, device_queue(ops, Q, D, *queue, Q)), ref)


@pytest.mark.parametrize("use_noun,use_verb", [(True, False), (False, True), (False, False)])
def test_mask_modes(ops, use_noun, use_verb):
    """noun only, verb only, and noun = verb = False: the reference's else-branch (verb), mapped as EgoNCE.fused maps it"""
    n, Q = 65, 128
    batch, queue = inputs(n, Q)
    ref = oracle(n, Q, Q, use_noun=use_noun, use_verb=use_verb)
    density_ok("noun=%s verb=%s" % (use_noun, use_verb), ref[4])
    got = run_queue(ops, batch, device_queue(ops, Q, 256, *queue, Q), use_noun=use_noun, use_verb=use_verb or not use_noun)
    check("n=65 Q=128 noun=%s verb=%s" % (use_noun, use_verb), got, ref)
    if use_noun != use_verb:
        assert abs(float(ref[0]) - float(oracle(n, Q, Q)[0])) > 1e-3             # the modes are told apart by the bar


def test_norm_softmax(ops):
    """no vectors: the queue adds negatives only, and no word buffer exists (W = 0)"""
    n, Q = 65, 128
    batch, queue = inputs(n, Q)
    ref = oracle(n, Q, Q, kind="nsl")
    assert not bool(ref[4].any())
    q = device_queue(ops, Q, 256, queue[0], queue[1], None, None, Q)
    assert q.W == 0
    check("n=65 Q=128 NormSoftmaxLoss", run_queue(ops, batch[:2] + (None, None), q), ref)
    assert abs(float(ref[0]) - float(R.oracle_head(O, batch[0], batch[1], None, None)[0])) > 1e-1


def test_an_empty_queue_is_the_plain_loss(ops):
    n, Q = 65, 128
    batch, queue = inputs(n, Q)
    ref = R.oracle_head(O, *batch)
    check("n=65 Q=128 filled=0", run_queue(ops, batch, device_queue(ops, Q, 256, *queue, 0)), ref)


def test_identity_text_against_asymmetric_video_and_queues(ops):
    """The operand-map check: text = I, an asymmetric video, and two asymmetric queues that differ from each other -- a text / video
    queue swap or a transposed product shows in the gradients."""
    n = Q = D = 64
    idx = torch.arange(n * D, dtype=torch.float32).view(n, D)
    row = torch.arange(n)[:, None].float()
    text = torch.eye(n)
    video = (idx % 17.0) - 3.0 * (row % 5) + 1.0
    q_text = QR.normalise((idx % 13.0) - 2.0 * (row % 7) + 0.5)
    q_video = QR.normalise((idx % 11.0) * (1.0 + row % 3) - 4.0)
    assert not torch.equal(video, video.t()) and not torch.equal(q_text, q_text.t()) and not torch.equal(q_video, q_video.t())
    assert R.rel(q_text, q_video) > 0.1
    (_, _, noun, verb), (_, _, q_noun, q_verb) = inputs(64, 64)
    batch = (text, video, noun, verb)
    ref = QR.oracle(O, *batch, q_text, q_video, q_noun, q_verb, Q)
    swapped = QR.oracle(O, *batch, q_video, q_text, q_noun, q_verb, Q)
    assert R.rel(swapped[1], ref[1]) > 100 * GRAD_BAR                             # the bar tells a swap apart
    check("text = I, asymmetric video and queues", run_queue(ops, batch, device_queue(ops, Q, D, q_text, q_video, q_noun, q_verb, Q)), ref)


@pytest.mark.parametrize("n,Q,K", [(65, 128, 100), (129, 1024, 1000)])
def test_learnable_scale(ops, n, Q, K):
    s = 2.75
    batch, queue = inputs(n, Q)
    ref = oracle(n, Q, K, logit_scale=s)
    got = run_queue(ops, batch, device_queue(ops, Q, 256, *queue, K), temperature=123.0, logit_scale=torch.tensor([s]).cuda())
    assert len(got) == 4
    check("n=%d Q=%d filled=%d s=%.2f" % (n, Q, K, s), got, ref)
    # the loss alone: no gradient is written and none is needed
    out = run_queue(ops, batch, device_queue(ops, Q, 256, *queue, K), logit_scale=torch.tensor([s]).cuda(), want_grads=False)
    assert abs(out[0] - float(ref[0])) < LOSS_BAR * max(1.0, abs(float(ref[0])))


def test_two_calls_are_bit_identical(ops):
    n, Q, K = 129, 1024, 1000
    batch, queue = inputs(n, Q)
    q = device_queue(ops, Q, 256, *queue, K)
    dev = [t.cuda() for t in batch]
    s = torch.tensor([3.0]).cuda()
    a = ops.egonce_queue_fwd_bwd(*dev, 0.05, q, logit_scale=s)[:-1]
    b = ops.egonce_queue_fwd_bwd(*dev, 0.05, q, logit_scale=s)[:-1]
    torch.cuda.synchronize()
    assert len(a) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))


def ring_batch(k, n=65):
    return R.make_inputs(n, 256, seed=100 + k)


def test_the_ring_wraps(ops):
    """Q = 128, batches of 65 pushed three times: the second push wraps, the third overwrites; the fourth call sees the ring of the host
    model."""
    Q, n = 128, 65
    q = ops.EgonceQueue(Q, 256, 582, 118, "cuda")
    ring = QR.Ring(Q, 256)
    for k in range(4):
        batch = ring_batch(k)
        ref = QR.oracle(O, *batch, *ring.columns())
        out = ops.egonce_queue_fwd_bwd(*(t.cuda() for t in batch), 0.05, q)
        check("ring call %d (filled %d)" % (k, ring.filled), (float(out[0]),) + tuple(t.cpu() for t in out[1:3]), ref)
        ops.egonce_queue_push(out[-1], out[0], n, q)
        ring.push(*batch, loss=float(out[0]))
        assert (q.head(), q.filled()) == (ring.head, ring.filled) == ((65, 65), (2, 128), (67, 128), (4, 128))[k]
        assert R.rel(q.text.cpu()[:ring.filled], ring.text[:ring.filled]) < 1e-6
        assert R.rel(q.video.cpu()[:ring.filled], ring.video[:ring.filled]) < 1e-6
        assert torch.equal(q.words.cpu()[:ring.filled], words_i32(ring.noun[:ring.filled], ring.verb[:ring.filled]))


@pytest.mark.parametrize("poison", ["text", "noun"])
def test_a_loss_that_is_not_finite_pushes_nothing(ops, poison):
    """A NaN text row / a negative noun entry: the loss is NaN, head, filled and the buffers stay bit for bit; the next clean call
    matches the oracle on the untouched queue."""
    n, Q, K = 65, 128, 100
    batch, queue = inputs(n, Q)
    q = device_queue(ops, Q, 256, *queue, K)
    q.text[K:], q.video[K:] = 0.5, 0.25                                           # comparable bit for bit (no NaN)
    before = [t.clone() for t in (q.text, q.video, q.words, q.state)]
    bad = [t.clone() for t in batch]
    if poison == "text":
        bad[0][17, 5] = float("nan")
    else:
        bad[2][40, 7] = -1.0
    out = ops.egonce_queue_fwd_bwd(*(t.cuda() for t in bad), 0.05, q)
    ops.egonce_queue_push(out[-1], out[0], n, q)
    torch.cuda.synchronize()
    assert float(out[0]) != float(out[0])
    assert all(torch.equal(a, b) for a, b in zip(before, (q.text, q.video, q.words, q.state)))
    assert (q.head(), q.filled()) == (K, K)
    out = ops.egonce_queue_fwd_bwd(*(t.cuda() for t in batch), 0.05, q)
    check("clean call after a poisoned %s" % poison, (float(out[0]),) + tuple(t.cpu() for t in out[1:3]), oracle(n, Q, K))
    ops.egonce_queue_push(out[-1], out[0], n, q)
    assert (q.head(), q.filled()) == ((K + n) % Q, Q)


def test_bad_arguments_are_refused(ops):
    from egovlp_amd import _lib
    h = _lib.lib()
    t = torch.ones(64, 8).cuda()
    qb = torch.zeros(128, 64).cuda()
    st = torch.zeros(2, dtype=torch.int32).cuda()
    w = torch.zeros(int(h.egv_egonce_queue_work_floats(8, 8, 0, 0, 128))).cuda()
    out = torch.zeros(1).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(n=8, D=8, Q=128, tau=0.05, ls=None, dt=None, dv=None, dls=None, state=p(st), noun=None):
        return h.egv_egonce_queue_fwd_bwd(p(t), p(t), noun, None, n, D, 8, 8, p(qb), p(qb), None, Q, state, tau, ls, 1e-8, 1, 1,
                                          p(out), dt, dv, dls, p(w), None)
    assert call(n=0) == 1 and call(n=129) == 1 and call(D=6) == 1 and call(D=260) == 1 and call(tau=0.0) == 1
    assert call(Q=100) == 1 and call(Q=0) == 1 and call(Q=65600) == 1 and call(state=None) == 1 and call(noun=p(t)) == 1
    assert call(dt=p(t)) == 1 and call(dv=p(t)) == 1                               # both gradients or neither
    assert call(ls=p(out), dt=p(t), dv=p(t)) == 1 and call(dt=p(t), dv=p(t), dls=p(out)) == 1
    assert h.egv_egonce_queue_push(p(w), p(out), 129, 8, 0, 0, p(qb), p(qb), None, 128, p(st), None) == 1
    assert h.egv_egonce_queue_push(p(w), p(out), 8, 8, 0, 0, p(qb), p(qb), None, 128, None, None) == 1
    assert call() == 0                                                             # the loss alone
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and int(st[1]) == 0


# ---------------------------------------------------------------------------------------------- the modules
def test_module_trajectory_eval_and_upstream_factor(ops):
    """EgoNCE(queue_size=128).fused stepped three times in train() against the oracle fed from the host ring (the third batch sees a
    wrapped ring); gradients carry the upstream factor; eval() is the plain head, bit for bit, and enqueues nothing."""
    from egovlp_amd.model.loss import EgoNCE
    loss_fn, ring = EgoNCE(queue_size=128), QR.Ring(128, 256)
    assert loss_fn.queue_filled() == 0
    for k in range(3):
        batch = ring_batch(k)
        ref = QR.oracle(O, *batch, *ring.columns())
        tc, vc = batch[0].cuda().requires_grad_(True), batch[1].cuda().requires_grad_(True)
        loss = loss_fn.fused(tc, vc, batch[2].cuda(), batch[3].cuda())
        (3.0 * loss).backward()
        check("EgoNCE(queue_size=128).fused step %d, upstream 3.0" % k, (float(loss.detach()), tc.grad.cpu() / 3.0, vc.grad.cpu() / 3.0), ref)
        assert R.rel(tc.grad, 3.0 * ref[1]) < GRAD_BAR
        ring.push(*batch, loss=float(loss.detach()))
        assert loss_fn.queue_filled() == ring.filled == (65, 128, 128)[k]
    assert len(loss_fn.state_dict()) == 0 and len(list(loss_fn.buffers())) == 4
    # eval(): the plain head's bits, nothing enqueued
    batch = [t.cuda() for t in ring_batch(3)]
    state = loss_fn.queue_state.clone()
    outs = []
    for fn in (loss_fn.eval(), EgoNCE()):
        tc, vc = batch[0].clone().requires_grad_(True), batch[1].clone().requires_grad_(True)
        loss = fn.fused(tc, vc, batch[2], batch[3])
        loss.backward()
        outs.append((loss.detach(), tc.grad, vc.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and torch.equal(state, loss_fn.queue_state)
    # back in train(): the queue is still there; reset_queue empties it
    loss_fn.train()
    ref = QR.oracle(O, *ring_batch(3), *ring.columns())
    assert abs(float(loss_fn.fused(*batch)) - float(ref[0])) < LOSS_BAR * max(1.0, abs(float(ref[0])))
    assert loss_fn.reset_queue().queue_filled() == 0
    ref = R.oracle_head(O, *ring_batch(3))
    assert abs(float(loss_fn.fused(*batch)) - float(ref[0])) < LOSS_BAR * max(1.0, abs(float(ref[0])))
    assert loss_fn.queue_filled() == 65


def test_queue_size_zero_is_the_module_as_it_was(ops):
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    batch = [t.cuda() for t in ring_batch(0)]
    for a, b, extra in ((EgoNCE(queue_size=0), EgoNCE(), batch[2:]), (NormSoftmaxLoss(queue_size=0), NormSoftmaxLoss(), [])):
        outs = []
        for fn in (a, b):
            tc, vc = batch[0].clone().requires_grad_(True), batch[1].clone().requires_grad_(True)
            loss = fn.fused(tc, vc, *extra)
            loss.backward()
            outs.append((loss.detach(), tc.grad, vc.grad))
        assert all(torch.equal(x, y) for x, y in zip(*outs))
        assert list(a.buffers()) == [] and len(a.state_dict()) == 0


def test_norm_softmax_module_with_a_learnable_temperature(ops):
    """NormSoftmaxLoss(queue_size=64, learnable_temperature=True): two steps; the second sees the first batch as negatives and the
    parameter's gradient is the oracle's dL/ds."""
    import math
    from egovlp_amd.model.loss import NormSoftmaxLoss
    loss_fn = NormSoftmaxLoss(queue_size=64, learnable_temperature=True).cuda()
    ring = QR.Ring(64, 256)
    for k in range(2):
        text, video = ring_batch(k, n=33)[:2]
        ref = QR.oracle(O, text, video, None, None, ring.text, ring.video, None, None, ring.filled, logit_scale=math.log(1.0 / 0.05))
        tc, vc = text.cuda().requires_grad_(True), video.cuda().requires_grad_(True)
        loss_fn.logit_scale.grad = None
        loss = loss_fn.fused(tc, vc)
        loss.backward()
        check("NormSoftmaxLoss(queue_size=64, learnable) step %d" % k,
              (float(loss.detach()), tc.grad.cpu(), vc.grad.cpu(), loss_fn.logit_scale.grad.cpu()), ref)
        ring.push(text, video, None, None, loss=float(loss.detach()))
    assert loss_fn.queue_filled() == 64 and len(loss_fn.state_dict()) == 1          # the logit scale alone


# ---------------------------------------------------------------------------------------------- the steps
# the builders of tests/test_gpu_cached_step.py
PARITY = 1e-3
STEP_GRAD_BAR = 3e-3                 # 'bf16x3'
WATCH = ["video_model.blocks.3.attn.qkv.weight", "text_model.transformer.layer.2.ffn.lin1.weight", "video_model.pos_embed",
         "vid_proj.0.weight", "video_model.blocks.7.norm3.bias", "video_model.patch_embed.proj.weight",
         "video_model.blocks.0.timeattn.qkv.weight"]


def to_dev(batch):
    return {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
            "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}


def build_full(time_init="zeros"):
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.synth import synth_state_dict
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16,
                                   "pretrained": True, "time_init": time_init},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    return m.cuda(), sd


def run_step(m, sd, dev, loss_fn, chunk=None):
    """One step with an optimizer whose lr is 0 -> (loss, {watched: gradient}).  chunk None: the plain step."""
    from egovlp_amd import weights
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    Precision.set("bf16x3")
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    opt = AdamW(m.parameters(), lr=0.0)
    loss = egoclip_step(m, loss_fn, opt, dev) if chunk is None else egoclip_step_cached(m, loss_fn, opt, dev, chunk)
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    return float(loss), {k: params[k].grad.detach().cpu().clone() for k in WATCH}


def test_the_steps_take_a_loss_with_a_queue(ops):
    """Two egoclip_steps with queue_size=64: the second sees the first batch in the queue, so its loss differs from a queue-less run's;
    egoclip_step_cached over the same data from the same starting queue gives the plain step's loss and gradients within the bar of
    tests/test_gpu_cached_step.py for cached against plain (2 x PARITY on the loss, 2 x the gradient bar), and pushes once."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.synth import synth_batch
    m, sd = build_full()
    first, second = (to_dev(synth_batch(8, T=4, L=32, seed=s, ragged=True)) for s in (4321, 977))
    plain, cached, none = EgoNCE(queue_size=64), EgoNCE(queue_size=64), EgoNCE()
    l1, _ = run_step(m, sd, first, plain)
    l1c, _ = run_step(m, sd, first, cached)
    assert l1 == l1c and plain.queue_filled() == cached.queue_filled() == 8
    assert torch.equal(plain.queue_text, cached.queue_text) and torch.equal(plain.queue_words, cached.queue_words)
    l2, g2 = run_step(m, sd, second, plain)
    l2c, g2c = run_step(m, sd, second, cached, chunk=2)
    l2n, _ = run_step(m, sd, second, none)
    print("second step: plain with a queue %.6f, cached with a queue %.6f, without a queue %.6f" % (l2, l2c, l2n))
    assert plain.queue_filled() == cached.queue_filled() == 16
    assert abs(l2 - l2n) > 10 * PARITY * abs(l2n)
    assert abs(l2 - l2c) < 2 * PARITY * abs(l2)
    for k in WATCH:
        r = R.rel(g2c[k], g2[k])
        print("  cached vs plain grad %-50s rel %.2e" % (k, r))
        assert r <= 2 * STEP_GRAD_BAR, (k, r)
