"""The EgoNCE head with a queue of past embeddings (egovlp_amd/csrc/egonce_long.hip) without a GPU: the test inputs' properties, the
tiled algorithm restated in torch (tests/egonce_queue_ref.py) against the fp64 oracle, the host model of the ring, the constructor
argument `queue_size` of EgoNCE / NormSoftmaxLoss, and the new entries of the C ABI.  Values on the device:
tests/test_gpu_egonce_queue.py."""
import os
import re

import pytest
import torch

import egonce_long_ref as R
import egonce_queue_ref as QR
from oracle import egovlp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 64), (63, 64), (65, 128), (64, 192), (129, 1000), (256, 4096)]
NEW_ENTRIES = ["egv_egonce_queue_fwd_bwd", "egv_egonce_queue_layout", "egv_egonce_queue_push", "egv_egonce_queue_work_floats"]

_CASES = {}


def case(n, Q):
    """the split inputs and both oracles (with the queue, without it), computed once"""
    if (n, Q) not in _CASES:
        batch, queue = QR.split_inputs(n, Q, 256, seed=n + Q)
        _CASES[(n, Q)] = (batch, queue, QR.oracle(O, *batch, *queue, Q), QR.oracle(O, *batch, *queue, 0))
    return _CASES[(n, Q)]


@pytest.mark.parametrize("n,Q", SHAPES)
def test_the_inputs_make_the_queue_matter(n, Q):
    """The mask between batch and queue is neither empty nor full, about half of the anchors have a positive in the queue, and the
    queue moves d_text by tens of percent: a head that drops or mis-masks the queue cannot pass a 1e-4 bar."""
    batch, queue, ref, alone = case(n, Q)
    dens, pos = float(ref[4].double().mean()), float(ref[4].any(1).double().mean())
    change = R.rel(ref[1], alone[1]) if n > 1 else float("nan")          # n = 1: the queue-less gradient is zero
    print("n = %d Q = %d: batch x queue mask density %.3f, anchors with a queue positive %.2f, d_text moved by %.3f" % (n, Q, dens, pos, change))
    assert 0.03 <= dens <= 0.18
    if n > 1:
        assert 0.4 <= pos <= 0.65
        assert 0.25 <= change <= 0.45


@pytest.mark.parametrize("n,Q", SHAPES)
def test_the_oracle_without_a_queue_is_the_long_heads_oracle(n, Q):
    batch, queue, _, alone = case(n, Q)
    ref = R.oracle_head(O, *batch)
    el = abs(float(alone[0]) - float(ref[0]))
    et, ev = float((alone[1] - ref[1]).abs().max()), float((alone[2] - ref[2]).abs().max())
    print("n = %d: K = 0 against oracle_head: loss |diff| %.1e, max |d_text diff| %.1e, max |d_video diff| %.1e" % (n, el, et, ev))
    assert el <= 3e-16 * max(1.0, abs(float(ref[0]))) and et <= 3e-16 and ev <= 3e-16


@pytest.mark.parametrize("n,Q", SHAPES)
def test_tiled_restatement_matches_the_fp64_oracle(n, Q):
    """fp32 restatement against the fp64 oracle: rel < 1e-5 (fp32 rounding over rows of at most 4 352 terms is a few 1e-7)"""
    batch, queue, ref, _ = case(n, Q)
    loss, dt, dv, _ = QR.queue_head_ref(*batch, *queue, Q)
    el, et, ev = abs(float(loss) - float(ref[0])) / max(1.0, abs(float(ref[0]))), R.rel(dt, ref[1]), R.rel(dv, ref[2])
    print("n = %d Q = %d: loss %.7f oracle %.7f rel %.2e; d_text rel %.2e d_video rel %.2e" % (n, Q, float(loss), float(ref[0]), el, et, ev))
    assert el < 1e-5 and et < 1e-5 and ev < 1e-5


@pytest.mark.parametrize("n,Q,K", [(65, 128, 100), (64, 192, 100)])
def test_restatement_with_a_partly_filled_queue_and_the_scale_gradient(n, Q, K):
    """validity edge inside a queue tile; rows past K hold garbage that must not count; dL/ds against the oracle's"""
    batch, queue, _, _ = case(n, Q)
    s = 2.5
    ref = QR.oracle(O, *batch, *queue, K, logit_scale=s)
    dirty = [q.clone() for q in queue]
    dirty[0][K:], dirty[1][K:] = float("nan"), 7.0
    dirty[2][K:], dirty[3][K:] = 1.0, 1.0
    loss, dt, dv, dls = QR.queue_head_ref(*batch, *dirty, K, temperature=float(torch.tensor(-s, dtype=torch.float64).exp()))
    assert abs(float(loss) - float(ref[0])) < 1e-5 * max(1.0, abs(float(ref[0])))
    assert R.rel(dt, ref[1]) < 1e-5 and R.rel(dv, ref[2]) < 1e-5
    assert abs(float(dls) - float(ref[3])) < 1e-5 * max(1.0, abs(float(ref[3])))


@pytest.mark.parametrize("flags", [(True, False), (False, True), (False, False), None])
def test_restatement_modes(flags):
    n, Q = 65, 128
    batch, queue, full, _ = case(n, Q)
    use_noun, use_verb = flags or (None, None)
    if flags is None:                                        # NormSoftmaxLoss: no vectors, no queue positives
        batch, queue = batch[:2] + (None, None), queue[:2] + (None, None)
        ref = QR.oracle(O, *batch, *queue, Q)
        got = QR.queue_head_ref(*batch, *queue, Q)
        assert not bool(ref[4].any())
    else:
        ref = QR.oracle(O, *batch, *queue, Q, use_noun=use_noun, use_verb=use_verb)
        got = QR.queue_head_ref(*batch, *queue, Q, use_noun=use_noun, use_verb=use_verb or not use_noun)
    assert abs(float(got[0]) - float(ref[0])) < 1e-5 * max(1.0, abs(float(ref[0])))
    assert R.rel(got[1], ref[1]) < 1e-5 and R.rel(got[2], ref[2]) < 1e-5
    assert abs(float(ref[0]) - float(full[0])) > 1e-3        # the modes are told apart


@pytest.mark.parametrize("n,Q", SHAPES[:5])
def test_restatement_with_an_empty_queue_is_the_long_restatement(n, Q):
    batch, queue, _, _ = case(n, Q)
    a, b = QR.queue_head_ref(*batch, *queue, 0), R.long_head_ref(*batch)
    assert float(a[0]) == float(b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_the_ring_wraps_and_skips_a_loss_that_is_not_finite():
    Q, n, D = 128, 65, 8
    ring = QR.Ring(Q, D, dn=3, dv=2)
    rows = []
    for step in range(3):
        g = torch.Generator().manual_seed(step)
        t, v = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
        noun, verb = torch.full((n, 3), float(step)), torch.full((n, 2), float(step))
        ring.push(t, v, noun, verb, loss=1.0)
        rows.append(QR.normalise(t.double()))
        assert (ring.head, ring.filled) == ((65, 65), (2, 128), (67, 128))[step]
    # slots 0, 1 hold the tail of batch 1 until batch 2 overwrites them with its first rows; 2 .. 66 are batch 2's, 67 .. 127 batch 1's
    assert torch.equal(ring.text[2:67], rows[2]) and torch.equal(ring.text[67:128], rows[1][2:63])
    assert torch.equal(ring.text[0:2], rows[1][63:65])
    assert float(ring.noun[2, 0]) == 2.0 and float(ring.noun[127, 0]) == 1.0 and float(ring.noun[0, 0]) == 1.0
    before = (ring.head, ring.filled, ring.text.clone())
    ring.push(torch.ones(n, D), torch.ones(n, D), noun, verb, loss=float("nan"))
    ring.push(torch.ones(n, D), torch.ones(n, D), noun, verb, loss=float("inf"))
    assert (ring.head, ring.filled) == before[:2] and torch.equal(ring.text, before[2])


def test_queue_size_of_the_loss_modules():
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    for cls in (EgoNCE, NormSoftmaxLoss):
        for bad in (1, 63, 100, 65, 32, 65536 + 64, -64, 64.0, True):
            with pytest.raises(ValueError):
                cls(queue_size=bad)
        for good in (64, 128, 16384, 65536):
            assert cls(queue_size=good).queue_size == good
        off = cls(queue_size=0)
        assert off.queue_size == 0 and len(off.state_dict()) == 0 and list(off.buffers()) == [] and list(off.parameters()) == []
        on = cls(queue_size=128)
        assert len(on.state_dict()) == 0 and on.queue_filled() == 0      # nothing allocated before the first fused call
        assert on.reset_queue() is on
    x = torch.eye(4)
    with pytest.raises(ValueError, match="fused"):
        EgoNCE(queue_size=64)(x, x, x)
    with pytest.raises(ValueError, match="fused"):
        NormSoftmaxLoss(queue_size=64)(x)


def test_head_loss_refuses_the_matrix_path_with_a_queue():
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.trainer.common import egoclip_head_loss
    t = torch.randn(4, 8)
    with pytest.raises(ValueError, match="fused"):
        egoclip_head_loss(EgoNCE(queue_size=64), t, t, torch.zeros(4, 3), torch.zeros(4, 3), fused_head=False)
    with pytest.raises(ValueError, match="fused"):                       # D = 6 is outside the one-call head
        egoclip_head_loss(EgoNCE(queue_size=64), t[:, :6], t[:, :6], torch.zeros(4, 3), torch.zeros(4, 3))


def test_header_and_binding_declare_the_queue_entries():
    from egovlp_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egovlp_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(egv_egonce_queue_[a-z0-9_]+)\s*\(", txt)))
    assert declared == NEW_ENTRIES == sorted(k for k in _lib.PROTOTYPES if k.startswith("egv_egonce_queue_"))
    for name in NEW_ENTRIES:                                 # the binding passes as many arguments as the header declares
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, txt, flags=re.S).group(1)
        assert len(params.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", txt).group(1)) == _lib.ABI_VERSION == 6


def test_size_queries_and_limits():
    from egovlp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libegovlp_hip.so not built (run __graft_entry__.build())")
    import ctypes
    h = _lib.lib()
    Dp, W = ctypes.c_int32(), ctypes.c_int32()
    assert h.egv_egonce_queue_layout(256, 582, 118, ctypes.byref(Dp), ctypes.byref(W)) == 0 and (Dp.value, W.value) == (256, 24)
    assert h.egv_egonce_queue_layout(48, 0, 0, ctypes.byref(Dp), ctypes.byref(W)) == 0 and (Dp.value, W.value) == (64, 0)
    assert h.egv_egonce_queue_layout(6, 0, 0, ctypes.byref(Dp), ctypes.byref(W)) == 1
    assert h.egv_egonce_queue_layout(260, 0, 0, ctypes.byref(Dp), ctypes.byref(W)) == 1
    wf = h.egv_egonce_queue_work_floats
    assert wf(256, 256, 582, 118, 16128) > 0 and wf(64, 256, 582, 118, 64) > 0 and wf(65536, 256, 0, 0, 65536) > 0
    for n, D, Q in [(0, 256, 64), (65, 256, 64), (64, 256, 100), (64, 256, 32), (64, 256, 65600), (64, 6, 64), (64, 260, 64)]:
        assert wf(n, D, 582, 118, Q) == 0, (n, D, Q)
    # linear in n and bounded in Q: the partials of at most ~512 / ~256 workgroups
    assert wf(256, 256, 582, 118, 65536) < 4 * wf(256, 256, 582, 118, 4096)


def test_which_c_calls_a_module_with_a_queue_makes():
    """Over the do-nothing C-ABI stand-in: train() mode with a queue is the queue head followed by the push, for any n (also n <= 1 024);
    eval() mode and queue_size=0 make the calls of the module without the argument; the scale's gradient reaches the parameter."""
    from mock_hip import mock_hip
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    from egovlp_amd.trainer.common import egoclip_head_loss
    n = 64
    t, v = torch.randn(n, 64, requires_grad=True), torch.randn(n, 64, requires_grad=True)
    noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
    heads = lambda calls: [c for c in calls if c.startswith("egv_egonce")]
    with mock_hip() as calls:
        egoclip_head_loss(EgoNCE(), t, v, noun, verb).backward()
        plain = list(calls)
        assert heads(plain).count("egv_egonce_fwd_bwd") == 1
        del calls[:]
        egoclip_head_loss(EgoNCE(queue_size=0), t, v, noun, verb).backward()
        assert list(calls) == plain
        del calls[:]
        loss_fn = EgoNCE(queue_size=128)
        for _ in range(2):
            egoclip_head_loss(loss_fn, t, v, noun, verb).backward()
        assert heads(calls) == ["egv_egonce_queue_layout"] + ["egv_egonce_queue_work_floats", "egv_egonce_queue_fwd_bwd",
                                                               "egv_egonce_queue_push"] * 2
        assert len(loss_fn.state_dict()) == 0 and len(list(loss_fn.buffers())) == 4
        del calls[:]
        loss_fn.eval()
        egoclip_head_loss(loss_fn, t, v, noun, verb).backward()
        assert list(calls) == plain
        del calls[:]
        learn = NormSoftmaxLoss(queue_size=64, learnable_temperature=True)
        egoclip_head_loss(learn, t, v, None, None).backward()
        assert heads(calls).count("egv_egonce_queue_fwd_bwd") == 1 and learn.logit_scale.grad.shape == (1,)
        assert list(learn.state_dict()) == ["logit_scale"]
        with pytest.raises(ValueError):                      # a batch larger than the ring
            egoclip_head_loss(learn, torch.randn(65, 64), torch.randn(65, 64), None, None)
        with pytest.raises(ValueError):                      # the ring was allocated for 582 nouns
            loss_fn.train().fused(t, v, noun[:, :5], verb)
