"""CPU checks of Mixup / CutMix and label smoothing: the fp64 restatement tests/mix_ref.py against torch's own cross-entropy on
probability targets and with `label_smoothing=` (the independent yardstick: the reference has neither); the invariants of the host
draws (`mix_params`); the column layout of the gathered block with and without the soft columns; the refusals that happen before any
library call; and host dry runs over tests/mock_hip.py: with every switch off the step makes the calls it made before."""
import collections
import types

import pytest
import torch
import torch.nn.functional as F

import mix_ref as MR
from mock_hip import mock_hip

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


# ------------------------------------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize("C,n", [(2, 4), (2, 33), (17, 4), (17, 32), (17, 257)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_restated_soft_loss_is_torchs_cross_entropy_on_probability_targets(C, n, eps):
    g = torch.Generator().manual_seed(100 * C + n)
    x = (3.0 * torch.randn(n, C, generator=g)).double()
    t, t2 = torch.randint(0, C, (n,), generator=g), torch.randint(0, C, (n,), generator=g)
    lam = torch.rand(n, generator=g).double()
    lam[0], lam[1] = 1.0, 0.0
    q = MR.soft_targets(t, t2, lam, eps, C)
    assert float((q.sum(1) - 1.0).abs().max()) < 1e-15 and float(q.min()) >= 0.0
    loss, dlogits = MR.soft_loss(x, q)
    xa = x.clone().requires_grad_(True)
    want = F.cross_entropy(xa, q)
    want.backward()
    assert abs(float(loss) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    assert float((dlogits - xa.grad).abs().max()) <= 1e-12
    # timm's form: lam CE_eps(x, t) + (1 - lam) CE_eps(x, t2), row by row
    rows = lam * F.cross_entropy(x, t, label_smoothing=eps, reduction="none") + \
        (1.0 - lam) * F.cross_entropy(x, t2, label_smoothing=eps, reduction="none")
    assert abs(float(loss) - float(rows.mean())) <= 1e-12 * abs(float(want.detach()))
    # smoothing alone is torch's label_smoothing
    only, d_only = MR.soft_loss(x, MR.soft_targets(t, None, None, eps, C))
    xb = x.clone().requires_grad_(True)
    want_only = F.cross_entropy(xb, t, label_smoothing=eps)
    want_only.backward()
    assert abs(float(only) - float(want_only.detach())) <= 1e-12 * abs(float(want_only.detach()))
    assert float((d_only - xb.grad).abs().max()) <= 1e-12


def test_restated_head_chain_is_autograd_of_the_same_chain():
    g = torch.Generator().manual_seed(5)
    n, K, C, row0, B = 8, 12, 17, 4, 4
    feats, W, b = torch.randn(n, K, generator=g).double(), torch.randn(C, K, generator=g).double(), torch.randn(C, generator=g).double()
    t, t2 = torch.randint(0, C, (n,), generator=g), torch.randint(0, C, (n,), generator=g)
    lam, state = torch.rand(n, generator=g).double(), torch.tensor([1, 0, 1, 1, 0, 1, 1, 1])
    got = MR.soft_head(feats, W, b, t, t2, lam, 0.1, state=state, row0=row0, B=B)
    Wa, ba, mine = W.clone().requires_grad_(True), b.clone().requires_grad_(True), feats[row0:row0 + B].clone().requires_grad_(True)
    with torch.no_grad():
        others = F.linear(feats, W, b)
    scores = torch.cat([others[:row0], F.linear(mine, Wa, ba), others[row0 + B:]])
    loss = torch.mean(state.double()) * F.cross_entropy(scores, MR.soft_targets(t, t2, lam, 0.1, C))
    loss.backward()
    assert abs(float(got["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for k, w in (("dW", Wa.grad), ("db", ba.grad), ("dfeats", mine.grad)):
        assert float((got[k] - w).abs().max()) <= 1e-12, k


def test_mix_clips_restatement():
    A = torch.arange(3 * 2 * 1 * 4 * 6, dtype=torch.float64).view(3, 2, 1, 4, 6)
    idx = torch.tensor([[2, 2, 1, 3, 2, 5], [1, 1, 0, 0, 0, 0], [0, 0, 0, 4, 0, 6]], dtype=torch.int32)
    lam = torch.tensor([0.5, 0.25, 1.0])
    out = MR.mix_clips(A, idx, lam)
    box = torch.zeros(4, 6, dtype=torch.bool)
    box[1:3, 2:5] = True
    assert torch.equal(out[0], torch.where(box, A[2], A[0])) and torch.equal(out[1], A[1]) and torch.equal(out[2], A[2])
    idx[1, 0] = 0
    assert torch.equal(MR.mix_clips(A, idx, lam)[1], 0.25 * A[1] + 0.75 * A[0])
    # the tables as the kernels read them
    wild = torch.tensor([[-5, 2, -100, 900, -7, 3], [10, 7, 0, 4, 0, 6], [0, 6, 1, 2, 1, 2]], dtype=torch.int32)
    assert MR.clamp_tables(wild, 3, 4, 6).tolist() == [[0, 2, 0, 4, 0, 3], [2, 3, 0, 4, 0, 6], [0, 2, 1, 2, 1, 2]]


# ------------------------------------------------------------------------------------------------ the host draws
SETTINGS = [dict(), dict(mode="elem"), dict(prob=0.5), dict(prob=0.5, mode="elem"), dict(switch_prob=0.0), dict(switch_prob=1.0),
            dict(mixup_alpha=0.0), dict(cutmix_alpha=0.0), dict(mixup_alpha=0.2, cutmix_alpha=0.3, mode="elem")]


@pytest.mark.parametrize("kw", SETTINGS, ids=[str(s) for s in SETTINGS])
@pytest.mark.parametrize("B,H,W", [(5, 32, 32), (4, 28, 40)])
def test_mix_params_invariants(kw, B, H, W):
    from egovlp_amd.data_loader.transforms import mix_params
    g = torch.Generator().manual_seed(17)
    ops_seen = collections.Counter()
    for _ in range(200):
        idx, lam = mix_params(B, H, W, generator=g, **kw)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (B, 6) and lam.dtype == torch.float32 and tuple(lam.shape) == (B,)
        assert bool(torch.isfinite(lam).all()) and float(lam.min()) >= 0.0 and float(lam.max()) <= 1.0
        for b in range(B):
            p, op, y0, y1, x0, x1 = idx[b].tolist()
            ops_seen[op] += 1
            assert op in (0, 1, 2)
            if op == 0:
                assert (p, y0, y1, x0, x1) == (b, 0, 0, 0, 0) and float(lam[b]) == 1.0
                continue
            assert p == B - 1 - b
            if op == 2:
                assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
                assert float(lam[b]) == float(torch.tensor(1.0 - (y1 - y0) * (x1 - x0) / float(H * W), dtype=torch.float32))
            else:
                assert (y0, y1, x0, x1) == (0, 0, 0, 0)
        if kw.get("mode", "batch") == "batch":
            assert len({tuple(r[1:]) for r in idx.tolist()}) == 1 and len(set(lam.tolist())) == 1
    if kw.get("switch_prob") == 0.0 or kw.get("cutmix_alpha") == 0.0:
        assert ops_seen[2] == 0 and ops_seen[1] > 0
    elif kw.get("switch_prob") == 1.0 or kw.get("mixup_alpha") == 0.0:
        assert ops_seen[1] == 0 and ops_seen[2] > 0
    else:
        assert ops_seen[1] > 0 and ops_seen[2] > 0
    assert (ops_seen[0] > 0) == ("prob" in kw)
    if kw.get("mode") == "elem":
        assert len(set(lam.tolist())) > 1                                   # its own draw per clip


def test_mix_params_off_and_refusals():
    from egovlp_amd.data_loader.transforms import mix_params
    assert mix_params(4, 32, 32, mixup_alpha=0.0, cutmix_alpha=0.0) == (None, None)
    assert mix_params(4, 32, 32, prob=0.0) == (None, None)
    for bad in (dict(mode="pair"), dict(mixup_alpha=-1.0), dict(prob=1.5), dict(switch_prob=-0.1)):
        with pytest.raises(ValueError):
            mix_params(4, 32, 32, **bad)
    with pytest.raises(ValueError):
        mix_params(0, 32, 32)
    # the same generator state gives the same tables
    a = mix_params(6, 32, 32, mode="elem", generator=torch.Generator().manual_seed(3))
    b = mix_params(6, 32, 32, mode="elem", generator=torch.Generator().manual_seed(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the gathered block
def test_cls_layout_soft_columns_come_last_and_nothing_else_moves():
    from egovlp_amd.loss_ops import ClsLayout
    today = {("oscc", False): dict(ld=3, target=2, state=-1, fps=-1, start=-1, end=-1, pnr=-1),
             ("pnr", False): dict(ld=18, target=16, state=17, fps=-1, start=-1, end=-1, pnr=-1),
             ("pnr", True): dict(ld=23, target=16, state=17, fps=18, start=20, end=21, pnr=22)}
    for (task, ev), want in today.items():
        C = 2 if task == "oscc" else 16
        for lay in (ClsLayout(C, task, evaluate=ev), ClsLayout(C, task, ev, soft=False)):
            assert {k: getattr(lay, k) for k in want} == want and (lay.target2, lay.lam) == (-1, -1)
        soft = ClsLayout(C, task, evaluate=ev, soft=True)
        assert {k: getattr(soft, k) for k in want if k != "ld"} == {k: v for k, v in want.items() if k != "ld"}
        assert (soft.target2, soft.lam, soft.ld) == (want["ld"], want["ld"] + 1, want["ld"] + 2)
    lay = ClsLayout(2, "oscc", soft=True)
    blk = torch.zeros(3, lay.ld)
    lay.fill(blk, torch.tensor([1, 0, 1]), target2=torch.tensor([0, 0, 1]), lam=torch.tensor([0.25, 1.0, 0.5]))
    assert blk[:, 2:].tolist() == [[1.0, 0.0, 0.25], [0.0, 0.0, 1.0], [1.0, 1.0, 0.5]]
    hard = torch.zeros(3, 3)
    ClsLayout(2, "oscc").fill(hard, torch.tensor([1, 0, 1]))
    assert torch.equal(hard, blk[:, :3])


# ------------------------------------------------------------------------------------------------ refusals before any library call
def _tiny(classes=2, **extra):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
    vp.update(extra)
    return FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", projection_dim=classes,
                        load_checkpoint="").train()


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return _tiny()


def _mix(B, op=2, lam=0.75):
    idx = torch.tensor([[B - 1 - b, op, 8, 40, 4, 36] for b in range(B)], dtype=torch.int32)
    return idx, torch.full((B,), lam, dtype=torch.float32)


def test_refusals_happen_before_any_library_call(tiny):
    from egovlp_amd import ops
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.trainer.trainer_oscc import classification_step
    from egovlp_amd.trainer.trainer_pnr import Multi_Trainer_dist_PNR
    vm = tiny.video_model
    idx, lam = _mix(3)
    video = torch.zeros(3, 2, 3, 64, 64)
    with mock_hip() as calls:
        # PNR + mix: the step and the trainer's constructor
        with pytest.raises(ValueError, match="pnr"):
            classification_step(None, CrossEntropy(), None, {"video": video}, task="pnr", mix=(idx, lam))
        for name in ("mixup_alpha", "cutmix_alpha"):
            with pytest.raises(ValueError, match="PNR"):
                Multi_Trainer_dist_PNR(types.SimpleNamespace(**{name: 0.8}), None, None, None, None, None, None)
        # table shapes and dtypes, at the op and at the model
        bad = [(idx[:2], lam), (idx[:, :5].contiguous(), lam), (idx.long(), lam), (idx, lam.double()), (idx, lam[:2]), (idx.float(), lam),
               (idx.t().contiguous().t(), lam), (idx, None), (None, lam)]
        for m in bad:
            with pytest.raises(ValueError, match="mix"):
                ops.patch_gather(video, 16, 3, mix=m)
        for m in [(idx[:, :5], lam), (idx.float(), lam), (idx, lam[:2]), (idx, lam.long()), (idx.view(-1), lam), (None, lam), (idx, None)]:
            with pytest.raises(ValueError, match="set_input_mix"):
                vm.set_input_mix(*m)
        # lam outside [0, 1] or not finite, a partner outside the batch
        for v in (-0.01, 1.01, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=r"\[0, 1\]"):
                vm.set_input_mix(idx, torch.tensor([0.5, v, 0.5]))
        for p in (-1, 3):
            wrong = idx.clone()
            wrong[1, 0] = p
            with pytest.raises(ValueError, match="partner"):
                vm.set_input_mix(wrong, lam)
        assert getattr(vm, "_input_mix", None) is None                      # a refused table leaves nothing pending
        # mix and the eval transform exclude each other, whichever comes first
        vm.set_input_eval_transform(72, 64)
        with pytest.raises(ValueError, match="eval"):
            vm.set_input_mix(idx, lam)
        vm._input_eval = None
        vm.set_input_mix(idx, lam)
        assert vm._input_mix[0].dtype == torch.int32 and vm._input_mix[1].dtype == torch.float32
        with pytest.raises(ValueError, match="set_input_mix"):
            vm.set_input_eval_transform(72, 64)
        # a table for another batch size is refused in forward, and consumed
        with pytest.raises(ValueError, match="rows"):
            vm(torch.zeros(2, 2, 3, 64, 64))
        assert vm._input_mix is None
        # module arguments
        for e in (-0.1, 1.5):
            with pytest.raises(ValueError):
                CrossEntropy(label_smoothing=e)
        with pytest.raises(ValueError, match="target2"):
            CrossEntropy()(torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), None, lam)
        assert list(calls) == []


# ------------------------------------------------------------------------------------------------ host dry runs: the calls of a step
def _batch(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"video": torch.randn(B, 2, 3, 64, 64, generator=g), "state": torch.randint(0, 2, (B,), generator=g)}


@pytest.mark.parametrize("fused", [True, False])
def test_step_with_every_switch_off_makes_the_calls_of_before_and_the_mixed_step_the_new_ones(tiny, fused):
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_oscc import classification_step
    B = 3
    opt = AdamW(tiny.parameters(), lr=3e-5)
    with mock_hip() as calls:
        tiny.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            classification_step(tiny, CrossEntropy(), opt, _batch(B), fused_head=fused)      # builds the caches
            calls.clear()
            classification_step(tiny, CrossEntropy(), opt, _batch(B), fused_head=fused)
            before = list(calls)
            calls.clear()
            classification_step(tiny, CrossEntropy(label_smoothing=0.0), opt, _batch(B), fused_head=fused, mix=None)
            assert list(calls) == before
            hard = "egv_cls_head_loss_bwd" if fused else "egv_cross_entropy_fwd_bwd"
            soft = "egv_cls_head_loss_bwd_soft" if fused else "egv_cross_entropy_soft_fwd_bwd"
            assert before.count(hard) == 1 and before.count("egv_patch_gather") == 1 and not any("mix" in c or "soft" in c for c in before)
            # smoothing alone: the soft loss in place of the hard one, the gather untouched
            calls.clear()
            classification_step(tiny, CrossEntropy(label_smoothing=0.1), opt, _batch(B), fused_head=fused)
            assert [soft if c == hard else c for c in before] == list(calls)
            # a mix: the mixed gather in place of the plain one as well
            calls.clear()
            loss = classification_step(tiny, CrossEntropy(label_smoothing=0.1), opt, _batch(B), fused_head=fused, mix=_mix(B))
            want = [soft if c == hard else "egv_patch_gather_mix" if c == "egv_patch_gather" else c for c in before]
            assert want == list(calls) and loss.shape == ()
            assert getattr(tiny.video_model, "_input_mix", None) is None    # one-shot
        finally:
            tiny.exec_ctx.set_precision("bf16x3", "bf16x3")


def test_every_input_path_takes_one_of_the_two_mixed_entries():
    from egovlp_amd import ops
    B = 3
    idx, lam = _mix(B)
    f32, u8 = torch.zeros(B, 2, 3, 32, 32), torch.zeros(B, 2, 3, 40, 52, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 40, 52, 0]] * B, dtype=torch.int32)
    color = torch.zeros(B, 4)
    keep = torch.tensor([[0, 1, 3]] * B, dtype=torch.int32)

    class Dev(torch.Tensor):
        is_cuda = True                                                       # ops.patch_gather asks the aug tables where they live
    dev = lambda t: t.as_subclass(Dev)
    with mock_hip() as calls:
        for kp in (None, keep):
            rows = B * 2 * (4 if kp is None else 3)
            assert ops.patch_gather(f32, 16, 3, keep=kp, mix=(idx, lam)).rows == rows
            assert ops.patch_gather(u8[..., :32, :32].contiguous(), 16, 3, keep=kp, mix=(idx, lam)).rows == rows
            assert ops.patch_gather(u8, 16, 3, aug=(dev(boxes), 32), keep=kp, mix=(idx, lam)).rows == rows
            assert ops.patch_gather(u8, 16, 3, aug=(dev(boxes), 32), color=dev(color), keep=kp, mix=(idx, lam)).rows == rows
        assert list(calls) == ["egv_patch_gather_mix"] * 2 + ["egv_patch_gather_u8_aug_mix"] * 2 + ["egv_patch_gather_mix"] * 2 + \
            ["egv_patch_gather_u8_aug_mix"] * 2


def test_oscc_trainer_draws_per_step_only_when_switched_on(tiny):
    from egovlp_amd.trainer.trainer_oscc import Multi_Trainer_dist_OSCC
    tr = Multi_Trainer_dist_OSCC.__new__(Multi_Trainer_dist_OSCC)
    data = _batch(4)
    for off in (types.SimpleNamespace(rank=0), types.SimpleNamespace(rank=0, mixup_alpha=0, cutmix_alpha=0.0, mix_prob=1.0),
                types.SimpleNamespace(rank=0, mixup_alpha=None, cutmix_alpha=None)):
        tr.args = off
        assert tr._draw_mix(data) is None and tr.last_mix_lambda is None and tr._mix_generator is None
    tr.args = types.SimpleNamespace(rank=0, seed=1, mixup_alpha=0.8, cutmix_alpha=1.0, mix_mode="elem")
    idx, lam = tr._draw_mix(data)
    assert tuple(idx.shape) == (4, 6) and idx[:, 0].tolist() == [3, 2, 1, 0] and tr.last_mix_lambda == float(lam.mean())
    idx2, _ = tr._draw_mix(data)
    assert not torch.equal(idx, idx2)                                       # a fresh draw per step
    assert int(idx[:, 3].max()) <= 64 and int(idx[:, 5].max()) <= 64          # boxes in the frame the tower patches
    tr.args = types.SimpleNamespace(rank=0, mixup_alpha=0.8, cutmix_alpha=0.0, mix_prob=0.0)
    assert tr._draw_mix(data) is None                                       # prob 0: off
