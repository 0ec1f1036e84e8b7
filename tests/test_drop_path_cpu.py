"""Stochastic depth in the video tower, everything that needs no GPU: the model surface (constructor, FrozenInTime's extension key, what
still raises), the seeds, the host logic of block and cached step over the do-nothing C ABI (tests/mock_hip.py, wrapped here to log
the seeds the drop-path entry points receive), and the fp64 reference helper of the GPU tests against the oracle's own block.  Values
on the device: tests/test_gpu_drop_path.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import drop_path_ref as R
from mock_hip import mock_hip

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


def _video_params(arch="custom", **extra):
    vp = {"model": "SpaceTimeTransformer", "arch_config": arch, "num_frames": 4, "pretrained": True, "time_init": "rand"}
    if arch == "custom":
        vp["arch_kwargs"] = dict(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2)
    vp.update(extra)
    return vp


def _tiny(**extra):
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params=_video_params(**extra), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _batch(B):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=3, res=32)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


@pytest.mark.parametrize("rate,depth", [(0.1, 12), (0.2, 24), (0.3, 3), (0.25, 1), (0.0, 4)])
def test_constructor_builds_the_references_decay_rule(rate, depth):
    """model/video_transformer.py:246-250: dpr = linspace(0, rate, depth), block i gets dpr[i] (block 0 always 0)."""
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    m = SpaceTimeTransformer(img_size=32, embed_dim=128, depth=depth, num_heads=2, num_frames=2, drop_path_rate=rate)
    want = [x.item() for x in torch.linspace(0, rate, depth)]
    assert m.dpr == want and [blk.drop_path for blk in m.blocks] == want
    assert m.blocks[0].drop_path == 0.0 and m.drop_path_rate == rate
    if depth > 1:
        assert m.blocks[-1].drop_path == pytest.approx(rate, rel=1e-6)


def test_block_accepts_drop_path_and_rejects_what_is_no_probability():
    from egovlp_amd.model.video_transformer import SpaceTimeBlock, SpaceTimeTransformer
    assert SpaceTimeBlock(dim=128, num_heads=2, qkv_bias=True, drop_path=0.2).drop_path == pytest.approx(0.2)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            SpaceTimeBlock(dim=128, num_heads=2, qkv_bias=True, drop_path=bad)
        with pytest.raises(ValueError):
            SpaceTimeTransformer(img_size=32, embed_dim=128, depth=2, num_heads=2, drop_path_rate=bad)


def test_elementwise_dropout_still_raises():
    from egovlp_amd.model.video_transformer import Mlp, SpaceTimeBlock, SpaceTimeTransformer, VarAttention
    kw = dict(img_size=32, embed_dim=128, depth=2, num_heads=2)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(drop_rate=0.1, **kw)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(attn_drop_rate=0.1, **kw)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(drop_rate=0.1, drop_path_rate=0.1, **kw)
    with pytest.raises(NotImplementedError):
        SpaceTimeBlock(dim=128, num_heads=2, drop=0.1)
    with pytest.raises(NotImplementedError):
        VarAttention(128, num_heads=2, attn_drop=0.1)
    with pytest.raises(NotImplementedError):
        Mlp(128, drop=0.1)


def test_frozen_in_time_passes_the_key_through():
    """`video_params['drop_path_rate']` (an extension key; absent = 0 = the reference's configs) for all three arch_configs."""
    m = _tiny(drop_path_rate=0.3)
    assert m.video_model.dpr == [x.item() for x in torch.linspace(0, 0.3, 3)]
    assert _tiny().video_model.dpr == [0.0, 0.0, 0.0]
    from egovlp_amd.model import model as mm
    seen = []

    class Spy(mm.SpaceTimeTransformer):
        def __init__(self, *a, **kw):
            seen.append(kw.get("drop_path_rate"))
            kw.update(depth=1, embed_dim=128, num_heads=2, img_size=32)       # keep the stand-in small
            kw.pop("patch_size", None)
            super().__init__(*a, **kw)
    real = mm.SpaceTimeTransformer
    mm.SpaceTimeTransformer = Spy
    try:
        for arch in ("base_patch16_224", "large_patch14_224"):
            mm.FrozenInTime(video_params=_video_params(arch, drop_path_rate=0.15), text_params=dict(TINY_TEXT), projection="minimal",
                            load_checkpoint="")
            mm.FrozenInTime(video_params=_video_params(arch), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    finally:
        mm.SpaceTimeTransformer = real
    assert seen == [0.15, 0.0, 0.15, 0.0]


def test_seeds_differ_by_call_site_and_rank():
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    torch.manual_seed(1234)
    m = SpaceTimeTransformer(img_size=32, embed_dim=128, depth=4, num_heads=2, num_frames=2, drop_path_rate=0.2)
    assert m._drop_calls == 0 and m.seed_rank == 0 and m.seed_device is None
    seeds = set()
    for calls in (1, 2, 3):
        for rank in (0, 1, 5):
            m._drop_calls, m.seed_rank = calls, rank
            for layer in range(4):
                ss, sm, dev = m.drop_path_seeds(layer)
                assert dev is None and 0 <= ss < 2 ** 64 and 0 <= sm < 2 ** 64
                seeds.update((ss, sm))
    assert len(seeds) == 3 * 3 * 4 * 2
    # a function of its inputs (the backward and the cached step's replay rely on it), and of torch's seed
    m._drop_calls, m.seed_rank = 2, 1
    a = m.drop_path_seeds(3)
    assert a == m.drop_path_seeds(3)
    torch.manual_seed(4321)
    assert a != m.drop_path_seeds(3)
    # the draws behind two different seeds are different draws
    assert not np.array_equal(R.drop_path_scales(64, 0.5, a[0]), R.drop_path_scales(64, 0.5, a[1]))


def test_mirror_statistics_and_edge_cases():
    for p in (0.1, 0.5):
        s = R.drop_path_scales(4096, p, 0x1234_5678_9ABC_DEF0)
        keep = float((s != 0).mean())
        assert abs(keep - (1 - p)) < 4 * (p * (1 - p) / 4096) ** 0.5
        assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert np.array_equal(R.drop_path_scales(100, 0.0, 77), np.ones(100, np.float32))
    assert np.array_equal(R.drop_path_scales(64, 0.5, 77, seed_dev=5), R.drop_path_scales(64, 0.5, 77 ^ 5))
    assert int(R.mix32(np.array([0], np.uint32))[0]) == 0 and int(R.mix32(np.array([1], np.uint32))[0]) != 1


def test_reference_helper_equals_the_oracle_at_all_ones_scales():
    """The fp64 helper the GPU tests compare with IS the oracle's block / tower when nothing is dropped; a zero scale removes the branch."""
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    from oracle import egovlp_oracle as O
    cfg = O.VideoCfg(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_frames=2)
    m = SpaceTimeTransformer(img_size=32, embed_dim=128, depth=2, num_heads=2, num_frames=2, time_init="rand")
    sd = {"video_model." + k: v.double() for k, v in synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=2).items()}
    g = torch.Generator().manual_seed(0)
    B, T, n = 3, 2, 4
    x = torch.randn(B, 1 + T * n, 128, generator=g, dtype=torch.float64)
    p = "video_model.blocks.1."
    ones = torch.ones(B, dtype=torch.float64)
    assert torch.equal(R.block(x, sd, p, cfg, n, T), O.space_time_block(x, sd, p, cfg, n, T))
    assert torch.equal(R.block(x, sd, p, cfg, n, T, ones, ones), O.space_time_block(x, sd, p, cfg, n, T))
    video = torch.randn(B, T, 3, 32, 32, generator=g, dtype=torch.float64)
    assert torch.equal(R.tower(video, sd, cfg), O.video_encoder(video, sd, cfg))
    # both branches of sample 1 dropped: its rows pass through; sample 0 and 2 are untouched by it (no coupling across samples)
    z = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    y = R.block(x, sd, p, cfg, n, T, z, z)
    assert torch.equal(y[1], x[1]) and torch.equal(y[[0, 2]], O.space_time_block(x, sd, p, cfg, n, T)[[0, 2]])
    # a kept branch is amplified: s = 2 on the MLP branch doubles that branch
    two = 2 * ones
    full, sr_only = O.space_time_block(x, sd, p, cfg, n, T), R.block(x, sd, p, cfg, n, T, ones, 0 * ones)
    assert torch.allclose(R.block(x, sd, p, cfg, n, T, ones, two), sr_only + 2 * (full - sr_only), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ host logic over the mock C ABI
def _log_drop_path_calls(log):
    """Replace the mock's three drop-path entry points by callbacks (real prototypes) that record (name, p, seed) and stay in the
    call log.  The library object is the mock of the enclosing `with mock_hip()`."""
    from egovlp_amd import _lib
    mock, keep = _lib._lib, []
    where = {"egv_drop_path_scales": (1, 2), "egv_drop_path_add": (6, 7), "egv_drop_path_grad": (5, 6)}     # (p, seed) argument slots
    for name, (ip, iseed) in where.items():
        res, args = _lib.PROTOTYPES[name]
        inner = getattr(mock, name)

        def cb(*a, _name=name, _ip=ip, _is=iseed, _inner=inner):
            log.append((_name, round(float(a[_ip]), 6), int(a[_is])))
            return _inner(*a)
        fn = C.CFUNCTYPE(res, *args)(cb)
        keep.append(fn)
        setattr(mock, name, fn)
    return keep


def test_block_paths_and_seeds_of_a_train_and_an_eval_forward():
    """Train mode: the blocks with p > 0 run the per-kernel path with two egv_drop_path_add in the forward and two egv_drop_path_grad
    in the backward, from the seeds of the forward (MLP branch first in the backward); block 0 and eval() run what a rate-0 model runs,
    call for call."""
    torch.manual_seed(0)
    m, m0 = _tiny(drop_path_rate=0.3), _tiny()
    m0.load_state_dict(m.state_dict())
    vm = m.video_model
    video = _batch(2)["video"]
    with mock_hip() as calls:
        log = []
        keep = _log_drop_path_calls(log)          # noqa: F841  (the callbacks must outlive the calls)
        for mod in (m, m0):
            mod.exec_ctx.set_precision("bf16x3", "bf16")
            mod.video_model(video)                                          # builds the weight-plane cache
        calls.clear()
        del log[:]
        c0 = vm._drop_calls
        y = vm(video)
        assert vm._drop_calls == c0 + 1
        want = []
        for layer in (1, 2):
            ss, sm, _ = vm.drop_path_seeds(layer)
            p = round(float(np.float32(vm.dpr[layer])), 6)
            want += [("egv_drop_path_add", p, ss), ("egv_drop_path_add", p, sm)]
        assert log == want and vm.drop_path_seeds(1)[0] != vm.drop_path_seeds(2)[0]
        del log[:]
        y.sum().backward()
        back = []
        for layer in (2, 1):
            ss, sm, _ = vm.drop_path_seeds(layer)
            p = round(float(np.float32(vm.dpr[layer])), 6)
            back += [("egv_drop_path_grad", p, sm), ("egv_drop_path_grad", p, ss)]
        assert log == back
        # another forward: other seeds
        del log[:]
        vm(video)
        assert len(log) == 4 and not {e[2] for e in log} & {e[2] for e in want}
        # eval(): nothing is dropped, the counter stays, and the launches are those of the rate-0 model
        m.eval()
        m0.eval()
        c1 = vm._drop_calls
        runs = []
        for mod in (m, m0):
            calls.clear()
            del log[:]
            with torch.no_grad():
                mod.video_model(video)
            runs.append(list(calls))
            assert not log
        assert runs[0] == runs[1] and vm._drop_calls == c1
        # a capture-safe device seed word stops the host counter
        m.train()
        vm.seed_device = torch.zeros(1, dtype=torch.int64)
        vm(video)
        assert vm._drop_calls == c1
        vm.seed_device = None


def test_block_calls_are_refused_for_a_dropping_forward():
    from egovlp_amd import ops
    from egovlp_amd.model.video_transformer import block_calls_ok
    ec = ops.new_context()
    ec.set_precision("bf16x3", "bf16")
    M, D, Hd = 8 * 785, 768, 3072
    assert block_calls_ok(ec, M, D, Hd) and block_calls_ok(ec, M, D, Hd, drop_path=False)
    assert not block_calls_ok(ec, M, D, Hd, drop_path=True)


def test_cached_step_restores_the_video_counter():
    """B = 4 in chunks of 2 at rate 0.3: pass 3 re-encodes every chunk from the seeds of its pass 1 (forward and backward), the
    chunks draw different seeds, and the counter advanced once per chunk over the step."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    torch.manual_seed(0)
    m = _tiny(drop_path_rate=0.3)
    m.text_model.set_dropout(0.0, 0.0)
    opt = AdamW(m.parameters(), lr=3e-5)
    vm = m.video_model
    with mock_hip():
        log = []
        keep = _log_drop_path_calls(log)          # noqa: F841
        m.exec_ctx.set_precision("bf16x3", "bf16")
        c0 = vm._drop_calls
        egoclip_step_cached(m, EgoNCE(), opt, _batch(4), 2)
    assert vm._drop_calls == c0 + 2
    per_fwd = 4                                   # two blocks with p > 0, two branches each
    adds = [e[2] for e in log if e[0] == "egv_drop_path_add"]
    assert len(adds) == 4 * per_fwd
    p1c0, p1c1, p3c0, p3c1 = (adds[i * per_fwd:(i + 1) * per_fwd] for i in range(4))
    assert p3c0 == p1c0 and p3c1 == p1c1
    assert not set(p1c0) & set(p1c1) and len(set(p1c0)) == per_fwd
    # the order of the step: both chunks' cache passes, then (forward, backward) per chunk; each backward regenerates its forward's draws
    names = [e[0] for e in log]
    assert names == ["egv_drop_path_add"] * (2 * per_fwd) + (["egv_drop_path_add"] * per_fwd + ["egv_drop_path_grad"] * per_fwd) * 2
    grads = [e[2] for e in log if e[0] == "egv_drop_path_grad"]
    assert sorted(grads[:per_fwd]) == sorted(p1c0) and sorted(grads[per_fwd:]) == sorted(p1c1)
