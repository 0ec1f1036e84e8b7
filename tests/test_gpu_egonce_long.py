"""The long EgoNCE head (egv_egonce_long_fwd_bwd, egovlp_amd/csrc/egonce_long.hip) on a real MI355X (`pytest -m gpu`) against the fp64
oracle with autograd (oracle.egovlp_oracle), at the smallest sizes at which each thing can break: tile edges, the first row past the
short head's cap, a ragged size, a size past the old fallback's limit; every mask mode, the eps paths, the last bit of the last word,
determinism, the NaN flag, the host-side switch and the cached step end to end.

Bars (the project's for this head): loss < 1e-4 max(1, |ref|), gradients rel-L2 < 1e-4.  Where the SHORT head itself misses 1e-4 at
n = 1 024 (small temperatures) the bar is 4 x the short head's error measured in the same test (rows four times longer).

Measured on MI355X (loss |diff| / d_text rel / d_video rel): see DESIGN 4.5a."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import egonce_long_ref as R  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

LOSS_BAR = 1e-4
GRAD_BAR = 1e-4


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


def oracle(n, D, kind="ego", temperature=0.05, use_noun=True, use_verb=True):
    """fp64 oracle on the shared inputs, computed once -> (loss, d_text, d_video, mask)"""
    key = (n, D, kind, temperature, use_noun, use_verb)
    if key not in _ORACLE:
        text, video, noun, verb = inputs(n, D)
        if kind == "nsl":
            noun = verb = None
        _ORACLE[key] = R.oracle_head(O, text, video, noun, verb, temperature, use_noun, use_verb)
    return _ORACLE[key]


def run_long(ops, text, video, noun, verb, temperature=0.05, **kw):
    c = lambda t: None if t is None else t.cuda()
    loss, dt, dv = ops.egonce_long_fwd_bwd(c(text), c(video), c(noun), c(verb), temperature, **kw)
    return float(loss), dt.cpu(), dv.cpu()


def check(tag, got, ref, loss_bar=LOSS_BAR, t_bar=GRAD_BAR, v_bar=GRAD_BAR):
    loss, dt, dv = got
    rl, rdt, rdv = float(ref[0]), ref[1], ref[2]
    el, et, ev = abs(loss - rl), R.rel(dt, rdt), R.rel(dv, rdv)
    print("%s: loss %.7f oracle %.7f |diff| %.2e (bar %.1e); d_text rel %.2e (bar %.1e) d_video rel %.2e (bar %.1e)" % (
        tag, loss, rl, el, loss_bar * max(1.0, abs(rl)), et, t_bar, ev, v_bar))
    assert el < loss_bar * max(1.0, abs(rl)), (tag, el)
    assert et < t_bar and ev < v_bar, (tag, et, ev)
    return el, et, ev


# tile edges; the first row past the cap, an exact tile multiple, a ragged size; past the old fallback's 4 096
@pytest.mark.parametrize("n,D", [(63, 256), (64, 256), (65, 256), (129, 256), (1025, 256), (1088, 256), (1531, 256), (4100, 256),
                                 (65, 132), (65, 4), (1025, 132), (1025, 4)])
def test_long_head_matches_the_oracle(ops, n, D):
    text, video, noun, verb = inputs(n, D)
    ref = oracle(n, D)
    dens = R.offdiag_density(ref[3])
    print("n = %d: off-diagonal density of the oracle's mask %.4f" % (n, dens))
    assert 0.01 <= dens <= 0.50              # a mask of all ones or all zeros would hide a mask bug
    check("n=%d D=%d" % (n, D), run_long(ops, text, video, noun, verb), ref)


def test_a_single_row(ops):
    """n = 1: P = Z bit for bit, so the loss and both gradients are exactly zero (the oracle's are, up to fp64 rounding)"""
    text, video, noun, verb = inputs(1, 256)
    ref = oracle(1, 256)
    loss, dt, dv = run_long(ops, text, video, noun, verb)
    print("n=1: loss %.3e (oracle %.3e), max |d_text| %.3e max |d_video| %.3e" % (loss, float(ref[0]), float(dt.abs().max()), float(dv.abs().max())))
    assert abs(loss - float(ref[0])) < LOSS_BAR
    assert float(dt.abs().max()) < 1e-6 and float(dv.abs().max()) < 1e-6 and float(ref[1].abs().max()) < 1e-12


def test_identity_text_against_an_asymmetric_video(ops):
    """The operand-map check of an MFMA kernel: A = I and an asymmetric B, so X = B^T row-normalised and a row <-> column swap in either
    product shows in the gradients (the loss alone is symmetric in the two directions)."""
    n = D = 64
    text = torch.eye(n)
    video = (torch.arange(n * D, dtype=torch.float32).view(n, D) % 17.0) - 3.0 * (torch.arange(n)[:, None] % 5).float() + 1.0
    assert not torch.equal(video, video.t())
    _, _, noun, verb = inputs(64, 256)
    ref = R.oracle_head(O, text, video, noun, verb)
    check("A = I, asymmetric B", run_long(ops, text, video, noun, verb), ref)


@pytest.mark.parametrize("use_noun,use_verb", [(True, False), (False, True), (False, False)])
def test_mask_modes(ops, use_noun, use_verb):
    """noun only, verb only, and noun = verb = False: the reference's else-branch (verb), mapped as EgoNCE.fused maps it"""
    n = 1025
    text, video, noun, verb = inputs(n, 256)
    ref = oracle(n, 256, use_noun=use_noun, use_verb=use_verb)
    got = run_long(ops, text, video, noun, verb, use_noun=use_noun, use_verb=use_verb or not use_noun)
    check("n=1025 noun=%s verb=%s" % (use_noun, use_verb), got, ref)
    if use_noun != use_verb:
        assert abs(float(ref[0]) - float(oracle(n, 256)[0])) > 1e-3          # the modes are told apart by the bar


def test_norm_softmax(ops):
    n = 1025
    text, video, _, _ = inputs(n, 256)
    check("n=1025 NormSoftmaxLoss", run_long(ops, text, video, None, None), oracle(n, 256, kind="nsl"))


@pytest.mark.parametrize("temperature", [0.01, 1.0])
def test_temperatures(ops, temperature):
    """The short head at n = 1 024 on the same inputs gives the bar where it misses 1e-4 itself."""
    n = 1025
    text, video, noun, verb = inputs(n, 256)
    ref_s = R.oracle_head(O, text[:1024], video[:1024], noun[:1024], verb[:1024], temperature)
    ls, _, dts, dvs = ops.egonce_fwd_bwd(text[:1024].cuda(), video[:1024].cuda(), noun[:1024].cuda(), verb[:1024].cuda(), temperature)
    es = (abs(float(ls) - float(ref_s[0])) / max(1.0, abs(float(ref_s[0]))), R.rel(dts, ref_s[1]), R.rel(dvs, ref_s[2]))
    print("tau=%g short head at n=1024: loss err / max(1, |ref|) %.2e, d_text rel %.2e, d_video rel %.2e" % ((temperature,) + es))
    bars = [1e-4 if e < 1e-4 else 4.0 * e for e in es]
    ref = oracle(n, 256, temperature=temperature)
    check("n=1025 tau=%g" % temperature, run_long(ops, text, video, noun, verb, temperature), ref, *bars)


@pytest.mark.parametrize("which", ["text", "video", "noun"])
def test_eps_paths(ops, which):
    """an all-zero text row, video row (the g / eps branch of the normalisation backward) and noun row (matches only itself)"""
    n = 65
    text, video, noun, verb = (t.clone() for t in inputs(n, 256))
    {"text": text, "video": video, "noun": noun}[which][17] = 0.0
    ref = R.oracle_head(O, text, video, noun, verb)
    got = run_long(ops, text, video, noun, verb)
    check("n=65 zero %s row" % which, got, ref)
    keep = torch.arange(n) != 17                             # the zero row's gradient is 1 / eps times the others': look at them alone too
    check("n=65 zero %s row, other rows" % which, (got[0], got[1][keep], got[2][keep]), (ref[0], ref[1][keep], ref[2][keep]))
    if which == "noun":
        assert int(ref[3][17].sum()) == 1


def test_bit_edges(ops):
    """6 rows: 0 / 1 share ONLY noun 581 and verb 117 (the last bit of the last word); 2 / 3 share a noun but no verb; 4 / 5 share noun
    32 and verb 32 (bit 0 of the second word) next to an unshared class 31 (bit 31 of the first)."""
    g = torch.Generator().manual_seed(6)
    text, video = torch.randn(6, 64, generator=g), torch.randn(6, 64, generator=g)
    noun, verb = torch.zeros(6, 582), torch.zeros(6, 118)
    noun[0, 581] = noun[1, 581] = 1.0
    verb[0, 117] = verb[1, 117] = 1.0
    noun[0, 100], noun[1, 101] = 1.0, 1.0
    noun[2, 5] = noun[3, 5] = 1.0
    verb[2, 1], verb[3, 2] = 1.0, 1.0
    noun[4, 31] = noun[4, 32] = noun[5, 32] = 1.0
    verb[4, 32] = verb[5, 32] = verb[5, 31] = 1.0
    ref = R.oracle_head(O, text, video, noun, verb)
    want = torch.eye(6, dtype=torch.bool)
    want[0, 1] = want[1, 0] = want[4, 5] = want[5, 4] = True
    assert torch.equal(ref[3], want)
    check("bit edges", run_long(ops, text, video, noun, verb), ref)
    # noun only: 2 / 3 join
    ref_n = R.oracle_head(O, text, video, noun, verb, use_noun=True, use_verb=False)
    assert bool(ref_n[3][2, 3]) and abs(float(ref_n[0]) - float(ref[0])) > 1e-3
    check("bit edges, noun only", run_long(ops, text, video, noun, verb, use_noun=True, use_verb=False), ref_n)


def test_two_calls_are_bit_identical(ops):
    n = 1531
    text, video, noun, verb = (t.cuda() for t in inputs(n, 256))
    a = ops.egonce_long_fwd_bwd(text, video, noun, verb, 0.05)
    b = ops.egonce_long_fwd_bwd(text, video, noun, verb, 0.05)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_negative_or_nan_entry_makes_the_loss_nan(ops):
    n = 65
    text, video, noun, verb = (t.clone() for t in inputs(n, 256))
    assert run_long(ops, text, video, noun, verb)[0] == run_long(ops, text, video, noun, verb)[0]     # finite, not NaN
    noun[40, 7] = -1.0
    assert run_long(ops, text, video, noun, verb)[0] != run_long(ops, text, video, noun, verb)[0]
    noun[40, 7] = 0.0
    verb[64, 117] = float("nan")
    loss = run_long(ops, text, video, noun, verb)[0]
    assert loss != loss


def test_bad_arguments_are_refused(ops):
    from egovlp_amd import _lib
    h = _lib.lib()
    t = torch.ones(64, 8).cuda()
    w = torch.zeros(int(h.egv_egonce_long_work_floats(8, 8, 8, 8))).cuda()
    out = torch.zeros(1).cuda()
    p = lambda x: ctypes.c_void_p(x.data_ptr())

    def call(n, D, noun=None, verb=None, tau=0.05):
        return h.egv_egonce_long_fwd_bwd(p(t), p(t), noun, verb, n, D, 8, 8, tau, 1e-8, 1, 1, p(out), None, None, p(w), None)
    assert call(0, 8) == 1 and call(65537, 8) == 1 and call(8, 6) == 1 and call(8, 260) == 1 and call(8, 8, tau=0.0) == 1
    assert call(8, 8, noun=p(t)) == 1 and call(8, 8, verb=p(t)) == 1
    assert call(8, 8) == 0                                   # both gradient pointers NULL: the loss alone
    torch.cuda.synchronize()


def test_fused_autograd_with_an_upstream_factor(ops):
    from egovlp_amd.model.loss import EgoNCE
    n = 1025
    text, video, noun, verb = inputs(n, 256)
    ref = oracle(n, 256)
    tc, vc = text.cuda().requires_grad_(True), video.cuda().requires_grad_(True)
    loss = EgoNCE().fused(tc, vc, noun.cuda(), verb.cuda())
    (3.0 * loss).backward()
    check("EgoNCE.fused n=1025, upstream 3.0", (float(loss.detach()), tc.grad.cpu() / 3.0, vc.grad.cpu() / 3.0), ref)
    assert R.rel(tc.grad, 3.0 * ref[1]) < GRAD_BAR and R.rel(vc.grad, 3.0 * ref[2]) < GRAD_BAR


def test_head_loss_fused_equals_the_decomposition(ops):
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.trainer.common import egoclip_head_loss
    n = 1500
    text, video, noun, verb = (t.cuda() for t in inputs(n, 256))
    out = []
    for fused in (True, False):
        tc, vc = text.clone().requires_grad_(True), video.clone().requires_grad_(True)
        loss = egoclip_head_loss(EgoNCE(), tc, vc, noun, verb, fused_head=fused)
        loss.backward()
        out.append((float(loss.detach()), tc.grad.cpu(), vc.grad.cpu()))
    check("n=1500 fused_head=True against fused_head=False", out[0], out[1])


def test_want_sim_past_the_cap(ops):
    text, video, noun, verb = (t.cuda() for t in inputs(1025, 256))
    with pytest.raises(ValueError):
        ops.egonce_fwd_bwd(text, video, noun, verb, 0.05, want_sim=True)
    loss, sim, dt, dv = ops.egonce_fwd_bwd(text, video, noun, verb, 0.05)
    assert sim is None and abs(float(loss) - float(oracle(1025, 256)[0])) < LOSS_BAR * float(oracle(1025, 256)[0])
    loss, sim, dt, dv = ops.egonce_fwd_bwd(text[:1024], video[:1024], noun[:1024], verb[:1024], 0.05, want_sim=True)
    assert sim.shape == (1024, 1024)


TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


def test_cached_step_over_1100_rows(ops):
    """The toy towers of tests/test_cached_step_cpu.py: B = 1 100 rows in chunks of 275, so the head of the step is the long one.  The
    returned loss is the fp64 oracle head applied to the step's cached embeddings and the batch's noun / verb vectors."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step_cached
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    Precision.set("bf16x3")
    m = FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=7), strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    m = m.train().cuda()
    b = synth_batch(1100, T=2, L=16, seed=3, res=32)
    dev = {"video": b["video"].cuda(), "text": {k: v.cuda() for k, v in b["text"].items()}, "noun_vec": b["noun_vec"].cuda(),
           "verb_vec": b["verb_vec"].cuda()}
    opt = AdamW(m.parameters(), lr=0.0)
    loss = egoclip_step_cached(m, EgoNCE(), opt, dev, 275, check_replay=True)
    torch.cuda.synchronize()
    te, ve = (x.detach().cpu() for x in m.last_cached_embeddings)
    assert te.shape[0] == 1100
    ref, _ = O.egoclip_loss(te.double(), ve.double(), b["noun_vec"].double(), b["verb_vec"].double())
    print("cached step B=1100: loss %.7f oracle head on the cached embeddings %.7f; replay max |diff| %.3e" % (
        float(loss), float(ref), float(m.last_replay_max_abs_diff)))
    assert abs(float(loss) - float(ref)) < LOSS_BAR * max(1.0, abs(float(ref)))
    assert float(m.last_replay_max_abs_diff) == 0.0
