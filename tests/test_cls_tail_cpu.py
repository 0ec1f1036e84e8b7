"""Host-side wiring of the CLS tail (egv_block_geom.train bit 1: the tower's last block computes only the B CLS rows of its output) on
CPU tensors against the do-nothing stand-in for the HIP library (tests/mock_hip.py): which egv_block_fwd / egv_block_bwd calls of a step
carry the bit.  Numerics: tests/test_gpu_cls_tail.py."""
import ctypes as C

import pytest
import torch

from mock_hip import mock_hip


def _model():
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                      "pretrained": True, "time_init": "rand"},
                        text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                        projection="minimal", load_checkpoint="")


def _batch(B=8, T=4, L=16, res=224):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=T, L=L, seed=3, res=res)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return _model().train()


def _record_train(seen):
    """Wrap the mock's egv_block_fwd / egv_block_bwd: `seen[name]` collects egv_block_geom.train of every call, in order."""
    from egovlp_amd import _lib
    keep = []
    for name in ("egv_block_fwd", "egv_block_bwd"):
        inner = getattr(_lib._lib, name)
        res, args = _lib.PROTOTYPES[name]

        def cb(*a, _inner=inner, _name=name):
            seen.setdefault(_name, []).append(int(C.cast(a[0], C.POINTER(_lib.BlockGeom)).contents.train))
            return _inner(*a)

        fn = C.CFUNCTYPE(res, *args)(cb)
        keep.append(fn)
        setattr(_lib._lib, name, fn)
    return keep


def _train_step(model):
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    opt = AdamW(model.parameters(), lr=3e-5)
    seen = {}
    with mock_hip() as calls:
        keep = _record_train(seen)
        for p in model.parameters():
            p.grad = None
        egoclip_step(model, EgoNCE(), opt, _batch(), 1, 0)
        del keep
    return seen, list(calls)


def test_the_bit_rides_on_the_last_forward_and_the_first_backward_call(model):
    seen, calls = _train_step(model)
    assert seen["egv_block_fwd"] == [1] * 11 + [3], seen
    assert seen["egv_block_bwd"] == [3] + [1] * 11, seen
    # the tail lives inside the C block calls: the host launches none of its pieces itself
    assert not [c for c in calls if c.startswith("egv_cls_")]


def _eval_forward(model):
    seen = {}
    with mock_hip(), torch.no_grad():
        keep = _record_train(seen)
        e = model.video_model(_batch()["video"])
        del keep
    return seen, e


def test_eval_forward_carries_the_bit_too(model):
    """eval(): the bit rides on the last call whether the kernels keep what a backward needs (trainable parameters: bit 0, see
    ExecContext.forward_is_train) or not (frozen parameters: an extraction run)."""
    model.eval()
    try:
        seen, e = _eval_forward(model)
        assert seen == {"egv_block_fwd": [1] * 11 + [3]}, seen
        assert tuple(e.shape) == (8, 768)
        for p in model.video_model.parameters():
            p.requires_grad_(False)
        seen, e = _eval_forward(model)
        assert seen == {"egv_block_fwd": [0] * 11 + [2]}, seen
        assert tuple(e.shape) == (8, 768)
    finally:
        for p in model.video_model.parameters():
            p.requires_grad_(True)
        model.train()


def test_switched_off_by_the_setting_and_by_the_environment(model, monkeypatch):
    model.exec_ctx.set(cls_tail=False)
    try:
        seen, _ = _train_step(model)
    finally:
        model.exec_ctx.unset("cls_tail")
    assert seen["egv_block_fwd"] == [1] * 12 and seen["egv_block_bwd"] == [1] * 12, seen
    assert model.exec_ctx.cls_tail
    monkeypatch.setenv("EGV_CLS_TAIL", "0")
    assert not model.exec_ctx.cls_tail
    seen, _ = _train_step(model)
    assert seen["egv_block_fwd"] == [1] * 12 and seen["egv_block_bwd"] == [1] * 12, seen


def test_a_last_block_that_drops_paths_keeps_the_full_path(model):
    last = model.video_model.blocks[-1]
    last.drop_path = 0.1
    try:
        seen, calls = _train_step(model)          # train mode: the last block takes the per-kernel path (stochastic depth is not in the C calls)
        assert seen["egv_block_fwd"] == [1] * 11 and seen["egv_block_bwd"] == [1] * 11, seen
        assert "egv_drop_path_add" in calls
        model.eval()                              # eval: no paths are dropped, the tail is back
        seen, _ = _eval_forward(model)
        assert seen == {"egv_block_fwd": [1] * 11 + [3]}, seen
    finally:
        last.drop_path = 0.0
        model.train()


def test_a_toy_model_takes_the_per_kernel_path_with_the_same_calls():
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    torch.manual_seed(0)
    m = SpaceTimeTransformer(img_size=32, patch_size=16, num_classes=0, embed_dim=128, depth=2, num_heads=2, num_frames=2).train()
    video = torch.randn(2, 2, 3, 32, 32)
    lists = {}
    for on in (True, True, False):               # the first pass builds the weight-plane cache: its list is replaced by the second's
        m.exec_ctx.set(cls_tail=on)
        m.exec_ctx.begin_step()
        for p in m.parameters():
            p.grad = None
        with mock_hip() as calls:
            e = m(video)
            e.sum().backward()
        lists[on] = list(calls)
        assert tuple(e.shape) == (2, 128)
    assert lists[True] == lists[False]
    assert not [c for c in lists[True] if c.startswith("egv_block_") or c.startswith("egv_cls_")]
    assert lists[True].count("egv_zero") >= 1      # the [B, S, D] gradient of norm(x)[:, 0] is still zero-filled on this path
