"""The long EgoNCE head (egovlp_amd/csrc/egonce_long.hip) without a GPU: its algorithm restated in torch (tests/egonce_long_ref.py)
against the fp64 oracle -- which pins the bit-mask rule and the symmetry argument the kernels rest on --, the host-side switch at
1 024 rows over the do-nothing C-ABI stand-in, and the size of the workspace.  Values on the device: tests/test_gpu_egonce_long.py."""
import os

import pytest
import torch

import egonce_long_ref as R
from mock_hip import mock_hip
from oracle import egovlp_oracle as O


@pytest.mark.parametrize("n", [65, 130, 1100])
def test_tiled_restatement_matches_the_fp64_oracle(n):
    """fp64 arithmetic in the restatement: what is left is the algorithm (bits instead of float masks, online statistics, swapped
    roles for the columns), so the bar is rounding, not the head's 1e-4."""
    text, video, noun, verb = R.make_inputs(n, 256, seed=n)
    ref, rdt, rdv, mask = R.oracle_head(O, text, video, noun, verb)
    dens = R.offdiag_density(mask)
    alone = float((mask.sum(1) == 1).double().mean())
    print("n = %d: off-diagonal density of the oracle's mask %.4f, rows matching only themselves %.2f" % (n, dens, alone))
    assert 0.01 <= dens <= 0.50
    assert torch.equal(mask, mask.t())
    loss, dt, dv = R.long_head_ref(text, video, noun, verb, dtype=torch.float64)
    el, et, ev = abs(float(loss) - float(ref)), R.rel(dt, rdt), R.rel(dv, rdv)
    print("  loss %.9f oracle %.9f |diff| %.2e; d_text rel %.2e d_video rel %.2e" % (float(loss), float(ref), el, et, ev))
    assert el < 1e-10 and et < 1e-10 and ev < 1e-10


@pytest.mark.parametrize("use_noun,use_verb", [(True, False), (False, True), (False, False)])
def test_restatement_modes(use_noun, use_verb):
    n = 130
    text, video, noun, verb = R.make_inputs(n, 64, seed=7)
    # EgoNCE.fused maps (False, False) to the reference's else-branch: verb only
    ref, rdt, rdv, _ = R.oracle_head(O, text, video, noun, verb, use_noun=use_noun, use_verb=use_verb)
    loss, dt, dv = R.long_head_ref(text, video, noun, verb, use_noun=use_noun, use_verb=use_verb or not use_noun, dtype=torch.float64)
    assert abs(float(loss) - float(ref)) < 1e-10 and R.rel(dt, rdt) < 1e-10 and R.rel(dv, rdv) < 1e-10


def test_restatement_norm_softmax_and_fp32():
    """mask = I (NormSoftmaxLoss), and the fp32 restatement within the head's own bars"""
    n = 130
    text, video, noun, verb = R.make_inputs(n, 256, seed=3)
    ref, rdt, rdv, _ = R.oracle_head(O, text, video, None, None)
    loss, dt, dv = R.long_head_ref(text, video, None, None, dtype=torch.float64)
    assert abs(float(loss) - float(ref)) < 1e-10 and R.rel(dt, rdt) < 1e-10 and R.rel(dv, rdv) < 1e-10
    ref, rdt, rdv, _ = R.oracle_head(O, text, video, noun, verb)
    loss, dt, dv = R.long_head_ref(text, video, noun, verb, dtype=torch.float32)
    assert abs(float(loss) - float(ref)) < 1e-4 * max(1.0, abs(float(ref))) and R.rel(dt, rdt) < 1e-4 and R.rel(dv, rdv) < 1e-4


def test_restatement_flags_a_negative_entry():
    text, video, noun, verb = R.make_inputs(65, 64, seed=1)
    noun[7, 3] = -1.0
    loss, _, _ = R.long_head_ref(text, video, noun, verb)
    assert bool(torch.isnan(loss))


@pytest.mark.parametrize("n,entry", [(1024, "egv_egonce_fwd_bwd"), (1025, "egv_egonce_long_fwd_bwd")])
def test_head_loss_dispatch(n, entry):
    """egoclip_head_loss: the short head up to 1 024 rows, the long head past it -- never the reference's decomposition"""
    from egovlp_amd.model.loss import EgoNCE, NormSoftmaxLoss
    from egovlp_amd.trainer.common import egoclip_head_loss
    t = torch.randn(n, 256, requires_grad=True)
    v = torch.randn(n, 256, requires_grad=True)
    noun, verb = torch.zeros(n, 582), torch.zeros(n, 118)
    with mock_hip() as calls:
        loss = egoclip_head_loss(EgoNCE(), t, v, noun, verb)
        loss.backward()
        assert calls.count(entry) == 1
        assert all(c in (entry, entry.replace("fwd_bwd", "work_floats")) for c in calls), calls
        assert t.grad.shape == t.shape and v.grad.shape == v.shape
        del calls[:]
        egoclip_head_loss(NormSoftmaxLoss(), t, v, None, None)
        assert calls.count(entry) == 1 and "egv_sim_matrix_fwd" not in calls
        del calls[:]
        egoclip_head_loss(EgoNCE(), t, v, noun, verb, fused_head=False)
        assert calls.count("egv_sim_matrix_fwd") == 3 and calls.count("egv_egonce_from_sim") == 1 and entry not in calls


def test_want_sim_is_refused_past_the_cap():
    from egovlp_amd import loss_ops as ops
    with mock_hip():
        loss, sim, dt, dv = ops.egonce_fwd_bwd(torch.randn(1024, 8), torch.randn(1024, 8), None, None, 0.05, want_sim=True)
        assert sim.shape == (1024, 1024)
        with pytest.raises(ValueError):
            ops.egonce_fwd_bwd(torch.randn(1025, 8), torch.randn(1025, 8), None, None, 0.05, want_sim=True)
        loss, sim, dt, dv = ops.egonce_fwd_bwd(torch.randn(1025, 8), torch.randn(1025, 8), None, None, 0.05)
        assert sim is None and dt.shape == (1025, 8)


def test_workspace_has_no_term_in_n_squared():
    """work_floats(2n) <= 2 work_floats(n) + a constant.  The constant is the bound on the per-range partials, which do not grow
    with n: at most 512 + n / 64 statistics ranges x 64 rows x 6 floats and 256 + n / 64 gradient ranges x 64 rows x Dp floats beyond
    the linear part -- (32 768 x 6 + 16 384 x 256) floats at D = 256."""
    import ctypes
    from egovlp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libegovlp_hip.so not built (run __graft_entry__.build())")
    h = ctypes.CDLL(_lib.LIB_PATH)
    f = h.egv_egonce_long_work_floats
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int32] * 4
    const = 32768 * 6 + 16384 * 256
    for n in (1, 63, 64, 65, 1024, 1025, 2048, 4100, 16384, 32768):
        w1, w2 = f(n, 256, 582, 118), f(2 * n, 256, 582, 118)
        assert w1 > 0 and w2 <= 2 * w1 + const, (n, w1, w2)
    # linear in n at the top of the range: 2 n Dp for the normalised rows, one gradient range, words and statistics
    assert f(65536, 256, 582, 118) <= 65536 * (3 * 256 + 24 + 16) + const
    assert f(65537, 256, 582, 118) == 0 and f(0, 256, 582, 118) == 0 and f(64, 260, 582, 118) == 0
