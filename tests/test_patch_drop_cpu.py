"""Patch dropout in the video tower, everything that needs no GPU: the model surface (constructor, set_patch_drop_rate, FrozenInTime's
extension key, what still raises), the rule for K, the numpy mirror of the draw and its statistics, the host logic over the do-nothing C
ABI (tests/mock_hip.py, wrapped here to log the sizes the new entry points and the attention receive), and the fp64 reference tower of
the GPU tests against the oracle's own.  Values on the device: tests/test_gpu_patch_drop.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import patch_drop_ref as R
from mock_hip import mock_hip

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
SEEDS = (0x0123456789ABCDEF, 0xF00DFACE12345678)
NEW = ("egv_patch_keep_draw", "egv_patch_gather_sel", "egv_patch_gather_u8_sel", "egv_patch_gather_u8_aug_sel",
       "egv_assemble_tokens_sel", "egv_assemble_tokens_bwd_sel")
FULL = ("egv_patch_gather", "egv_patch_gather_u8", "egv_patch_gather_u8_aug", "egv_patch_gather_u8_eval", "egv_assemble_tokens",
        "egv_assemble_tokens_bwd")


def _video_params(arch="custom", **extra):
    vp = {"model": "SpaceTimeTransformer", "arch_config": arch, "num_frames": 4, "pretrained": True, "time_init": "rand"}
    if arch == "custom":
        vp["arch_kwargs"] = dict(img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2)
    vp.update(extra)
    return vp


def _tiny(**extra):
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params=_video_params(**extra), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _batch(B):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=3, res=64)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


# ------------------------------------------------------------------------------------------------ the model surface
def test_constructor_and_setter_validate_the_rate():
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    kw = dict(img_size=32, embed_dim=128, depth=2, num_heads=2, num_frames=2)
    m = SpaceTimeTransformer(**kw)
    assert m.patch_drop_rate == 0.0 and m.last_patch_keep is None
    m = SpaceTimeTransformer(patch_drop_rate=0.5, **kw)
    assert m.patch_drop_rate == 0.5 and m.last_patch_keep is None
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            SpaceTimeTransformer(patch_drop_rate=bad, **kw)
        with pytest.raises(ValueError):
            m.set_patch_drop_rate(bad)
        assert m.patch_drop_rate == 0.5                      # a refused value changes nothing
    m.set_patch_drop_rate(0.0)                               # FLIP's last, unmasked epochs
    assert m.patch_drop_rate == 0.0
    m.set_patch_drop_rate(0.75)
    assert m.patch_drop_rate == 0.75
    # a trailing keyword: the reference's positional signature is untouched
    import inspect
    assert list(inspect.signature(SpaceTimeTransformer.__init__).parameters)[-1] == "patch_drop_rate"


@pytest.mark.parametrize("n,rate,want", [(196, 0.5, 98), (196, 0.75, 49), (196, 0.9, 19), (4, 0.9, 1), (257, 0.5, 128)])
def test_kept_count_is_timms_rule(n, rate, want):
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    m = SpaceTimeTransformer(img_size=32, embed_dim=128, depth=1, num_heads=2, num_frames=2, patch_drop_rate=rate)
    assert m.patch_keep_count(n) == want == R.keep_count(n, rate)
    m.set_patch_drop_rate(0.0)
    assert m.patch_keep_count(n) == n


def test_frozen_in_time_passes_the_key_through():
    """`video_params['patch_drop_rate']` (an extension key; absent = 0 = the reference's configs) for all three arch_configs, and
    `arch_kwargs` of 'custom'."""
    assert _tiny(patch_drop_rate=0.5).video_model.patch_drop_rate == 0.5
    assert _tiny().video_model.patch_drop_rate == 0.0
    vp = _video_params()
    vp["arch_kwargs"]["patch_drop_rate"] = 0.25
    from egovlp_amd.model import model as mm
    assert mm.FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal",
                           load_checkpoint="").video_model.patch_drop_rate == 0.25
    with pytest.raises(ValueError):
        _tiny(patch_drop_rate=1.0)
    seen = []

    class Spy(mm.SpaceTimeTransformer):
        def __init__(self, *a, **kw):
            seen.append((kw.get("patch_drop_rate"), kw.get("drop_path_rate")))
            kw.update(depth=1, embed_dim=128, num_heads=2, img_size=32)       # keep the stand-in small
            kw.pop("patch_size", None)
            super().__init__(*a, **kw)
    real = mm.SpaceTimeTransformer
    mm.SpaceTimeTransformer = Spy
    try:
        for arch in ("base_patch16_224", "large_patch14_224"):
            mm.FrozenInTime(video_params=_video_params(arch, patch_drop_rate=0.5, drop_path_rate=0.1), text_params=dict(TINY_TEXT),
                            projection="minimal", load_checkpoint="")
            mm.FrozenInTime(video_params=_video_params(arch), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    finally:
        mm.SpaceTimeTransformer = real
    assert seen == [(0.5, 0.1), (0.0, 0.0)] * 2


def test_elementwise_dropout_still_raises():
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    kw = dict(img_size=32, embed_dim=128, depth=2, num_heads=2)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(drop_rate=0.1, patch_drop_rate=0.5, **kw)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(attn_drop_rate=0.1, patch_drop_rate=0.5, **kw)
    with pytest.raises(NotImplementedError):
        SpaceTimeTransformer(drop_rate=0.1, **kw)


# ------------------------------------------------------------------------------------------------ the mirror of the draw
@pytest.mark.parametrize("B,n,K", [(3, 4, 1), (2, 37, 18), (5, 196, 98), (2, 257, 64), (1, 1024, 256), (2, 16, 16)])
def test_mirror_draws_k_distinct_ascending_positions(B, n, K):
    for seed in SEEDS:
        keep = R.patch_keep(B, n, K, seed)
        assert keep.shape == (B, K) and keep.dtype == np.int32
        assert keep.min() >= 0 and keep.max() < n
        assert bool((np.diff(keep, axis=1) > 0).all())                  # ascending, hence distinct
        # the kept positions ARE the K smallest (key, position) pairs
        h = R.keys(B, n, seed).astype(np.int64) * 2048 + np.arange(n)
        for b in range(B):
            assert set(keep[b].tolist()) == set(np.argsort(h[b], kind="stable")[:K].tolist())
        if K == n:
            assert np.array_equal(keep, np.tile(np.arange(n, dtype=np.int32), (B, 1)))


def test_a_device_seed_word_changes_the_sets():
    a = R.patch_keep(8, 196, 98, SEEDS[0])
    assert np.array_equal(a, R.patch_keep(8, 196, 98, SEEDS[0], seed_dev=0))
    assert not np.array_equal(a, R.patch_keep(8, 196, 98, SEEDS[0], seed_dev=0x5DEECE66D1234567))
    assert np.array_equal(R.patch_keep(8, 196, 98, SEEDS[0], seed_dev=5), R.patch_keep(8, 196, 98, SEEDS[0] ^ 5))
    assert not np.array_equal(a, R.patch_keep(8, 196, 98, SEEDS[1]))
    # clips of one call draw different sets
    assert len({tuple(r) for r in a.tolist()}) == 8


@pytest.mark.parametrize("B,n,K", [(4096, 16, 8), (4096, 196, 98), (2048, 37, 9)])
@pytest.mark.parametrize("seed", SEEDS)
def test_mirror_statistics(B, n, K, seed):
    """Uniform without replacement: every position is kept with probability K / n.  Over B independent clips the kept frequency of a
    position is binomial: within 5 sigma of K / n, sigma = sqrt(p (1 - p) / B)."""
    keep = R.patch_keep(B, n, K, seed)
    freq = np.bincount(keep.reshape(-1), minlength=n) / B
    p = K / n
    sigma = (p * (1 - p) / B) ** 0.5
    worst = float(np.abs(freq - p).max() / sigma)
    print("B = %d, n = %d, K = %d, seed %#x: worst position %.2f sigma" % (B, n, K, seed, worst))
    assert worst < 5.0
    if n == 196:
        assert len({r.tobytes() for r in keep}) == B               # 4 096 distinct sets


# ------------------------------------------------------------------------------------------------ host logic over the mock C ABI
def _log_sizes(log):
    """Replace some of the mock's entry points by callbacks (real prototypes) that record the sizes they are handed and stay in the
    call log.  The library object is the mock of the enclosing `with mock_hip()`."""
    from egovlp_amd import _lib
    mock, keep = _lib._lib, []
    where = {"egv_patch_keep_draw": (0, 1, 2, 3), "egv_divided_attn_fwd": (2, 3, 4), "egv_divided_attn_bwd": (7, 8, 9),
             "egv_assemble_tokens_sel": (5, 6, 7, 8), "egv_assemble_tokens_bwd_sel": (2, 3, 4, 5), "egv_patch_gather_sel": (1, 2, 8)}
    for name, slots in where.items():
        res, args = _lib.PROTOTYPES[name]
        inner = getattr(mock, name)

        def cb(*a, _name=name, _slots=slots, _inner=inner):
            log.append((_name,) + tuple(int(a[i]) for i in _slots))
            return _inner(*a)
        fn = C.CFUNCTYPE(res, *args)(cb)
        keep.append(fn)
        setattr(mock, name, fn)
    return keep


def test_dry_run_of_a_train_step_an_eval_forward_and_rate_zero():
    torch.manual_seed(0)
    m, m0, mz = _tiny(patch_drop_rate=0.5), _tiny(), _tiny(patch_drop_rate=0.0)
    vm = m.video_model
    B, T, n, K = 2, 2, 16, 8
    video = _batch(B)["video"]
    with mock_hip() as calls:
        log = []
        hold = _log_sizes(log)          # noqa: F841  (the callbacks must outlive the calls)
        for mod in (m, m0, mz):
            mod.exec_ctx.set_precision("bf16x3", "bf16")
            mod.video_model(video).sum().backward()                         # builds the weight-plane and workspace-size caches
        calls.clear()
        del log[:]
        c0 = vm._drop_calls
        y = vm(video)
        assert vm._drop_calls == c0 + 1
        assert tuple(y.shape) == (B, 128)
        assert vm.last_patch_keep is not None and tuple(vm.last_patch_keep.shape) == (B, K) and vm.last_patch_keep.dtype == torch.int32
        fwd = list(calls)
        seed = vm._seed(vm.PATCH_DROP_SITE)
        assert log[0] == ("egv_patch_keep_draw", B, n, K, seed)
        assert log[1] == ("egv_patch_gather_sel", B * T, T, K) and log[2] == ("egv_assemble_tokens_sel", B, T, n, K)
        attn = [e for e in log if e[0] == "egv_divided_attn_fwd"]
        assert len(attn) == 2 * 3 and all(e[1:] == (B, T, K) for e in attn)        # the blocks are handed K, not n
        y.sum().backward()
        both = list(calls)
        assert [e for e in log if e[0] == "egv_assemble_tokens_bwd_sel"] == [("egv_assemble_tokens_bwd_sel", B, T, n, K)]
        back = [e for e in log if e[0] == "egv_divided_attn_bwd"]
        assert len(back) == 2 * 3 and all(e[1:] == (B, T, K) for e in back)
        for name in ("egv_patch_keep_draw", "egv_patch_gather_sel", "egv_assemble_tokens_sel", "egv_assemble_tokens_bwd_sel"):
            assert both.count(name) == 1, name
        assert both.count("egv_patch_gather_u8_sel") == 0 and both.count("egv_patch_gather_u8_aug_sel") == 0
        assert not set(both) & set(FULL)
        assert fwd.index("egv_patch_keep_draw") < fwd.index("egv_patch_gather_sel") < fwd.index("egv_assemble_tokens_sel")
        # another forward: another seed
        del log[:]
        vm(video)
        assert vm._drop_calls == c0 + 2 and vm._seed(vm.PATCH_DROP_SITE) != seed

        # a train-mode forward + backward of the rate-0 model and of the model built without the key: one call list, none of the new ones
        runs = []
        for mod in (mz, m0):
            calls.clear()
            c = mod.video_model._drop_calls
            mod.video_model(video).sum().backward()
            runs.append(list(calls))
            assert mod.video_model._drop_calls == c and mod.video_model.last_patch_keep is None
        assert runs[0] == runs[1] and not set(runs[0]) & set(NEW) and "egv_patch_gather" in runs[0]
        # eval(): all patches, the counter stays, and the launches are those of the model built without the key
        for mod in (m, m0):
            mod.eval()
        c1 = vm._drop_calls
        runs = []
        for mod in (m, m0):
            calls.clear()
            with torch.no_grad():
                mod.video_model(video)
            runs.append(list(calls))
        assert runs[0] == runs[1] and not set(runs[0]) & set(NEW) and vm._drop_calls == c1 and vm.last_patch_keep is None
        # set_patch_drop_rate(0.) in train mode is the model as it was
        m.train()
        m0.train()
        vm.set_patch_drop_rate(0.0)
        runs = []
        for mod in (m, m0):
            calls.clear()
            mod.video_model(video)
            runs.append(list(calls))
        assert runs[0] == runs[1] and vm._drop_calls == c1
        vm.set_patch_drop_rate(0.5)
        # a capture-safe device seed word stops the host counter and reaches the draw
        vm.seed_device = torch.zeros(1, dtype=torch.int64)
        vm(video)
        assert vm._drop_calls == c1
        vm.seed_device = None


def test_uint8_input_takes_its_own_sel_gather():
    torch.manual_seed(0)
    m = _tiny(patch_drop_rate=0.5)
    vm = m.video_model
    u8 = (torch.rand(2, 2, 3, 64, 64) * 255).to(torch.uint8)
    with mock_hip() as calls:
        m.exec_ctx.set_precision("bf16x3", "bf16")
        vm(u8)
        assert calls.count("egv_patch_gather_u8_sel") == 1 and not set(calls) & set(FULL)


def test_counter_advances_once_with_both_kinds_of_drop():
    torch.manual_seed(0)
    m = _tiny(patch_drop_rate=0.5, drop_path_rate=0.3)
    vm = m.video_model
    video = _batch(2)["video"]
    with mock_hip() as calls:
        m.exec_ctx.set_precision("bf16x3", "bf16")
        for k in range(3):
            c0 = vm._drop_calls
            vm(video)
            assert vm._drop_calls == c0 + 1
        assert calls.count("egv_patch_keep_draw") == 3 and calls.count("egv_drop_path_add") == 3 * 4
        # the table's site is none of the drop-path sites
        assert vm._seed(vm.PATCH_DROP_SITE) not in {s for li in range(3) for s in vm.drop_path_seeds(li)[:2]}


def test_eval_transform_in_train_mode_raises():
    m = _tiny(patch_drop_rate=0.5)
    vm = m.video_model
    frames = (torch.rand(2, 2, 3, 80, 100) * 255).to(torch.uint8)
    with mock_hip() as calls:
        m.exec_ctx.set_precision("bf16x3", "bf16")
        vm.set_input_eval_transform(center_crop=72, out_res=64)
        c0 = vm._drop_calls
        with pytest.raises(ValueError, match="patch dropout"):
            vm(frames)
        assert vm._drop_calls == c0 and not calls
        # eval() takes the transform, and so does train mode at rate 0
        vm.eval()
        vm.set_input_eval_transform(center_crop=72, out_res=64)
        with torch.no_grad():
            vm(frames)
        assert "egv_patch_gather_u8_eval" in calls
        vm.train()
        vm.set_patch_drop_rate(0.0)
        vm.set_input_eval_transform(center_crop=72, out_res=64)
        vm(frames)


def test_ops_refuse_a_bad_table_before_any_launch():
    from egovlp_amd import ops
    video = torch.zeros(2, 3, 3, 64, 48)
    pe = torch.zeros(2 * 3 * 5, 64)
    cls, pos, tmp = torch.zeros(1, 1, 64), torch.zeros(1, 13, 64), torch.zeros(1, 5, 64)
    good = torch.zeros(2, 5, dtype=torch.int32)
    with mock_hip() as calls:
        for bad in (good.long(), good[:1], torch.zeros(2, 13, dtype=torch.int32), torch.zeros(2, 0, dtype=torch.int32), good.t().contiguous().t(),
                    good.view(-1), [[0] * 5] * 2):
            with pytest.raises(ValueError):
                ops.patch_gather(video, 16, 3, keep=bad)
            with pytest.raises(ValueError):
                ops.assemble_tokens(pe, cls, pos, tmp, 2, 3, 12, 64, keep=bad)
            with pytest.raises(ValueError):
                ops.assemble_tokens_bwd(torch.zeros(2, 16, 64), 2, 3, 12, 64, 5, keep=bad)
        with pytest.raises(ValueError):
            ops.assemble_tokens(pe[:-1], cls, pos, tmp, 2, 3, 12, 64, keep=good)
        with pytest.raises(ValueError):
            ops.assemble_tokens_bwd(torch.zeros(2, 17, 64), 2, 3, 12, 64, 5, keep=good)
        for args in ((0, 4, 1), (2, 4, 0), (2, 4, 5), (2, 1025, 8)):
            with pytest.raises(ValueError):
                ops.patch_keep_draw(*args, seed=1, device="cpu")
        assert not calls
        assert tuple(ops.patch_keep_draw(3, 4, 1, 7, device="cpu").shape) == (3, 1)
        assert ops.patch_gather(video, 16, 3, keep=good).rows == 2 * 3 * 5
        assert tuple(ops.assemble_tokens(pe, cls, pos, tmp, 2, 3, 12, 64, keep=good).shape) == (2, 16, 64)
        assert list(calls) == ["egv_patch_keep_draw", "egv_patch_gather_sel", "egv_assemble_tokens_sel"]


def test_cached_step_restores_the_counter_and_replays_the_tables():
    """B = 4 in chunks of 2 at rate 0.5: pass 3 re-encodes every chunk from the seed of its pass 1, the chunks draw from different seeds,
    and the counter advanced once per chunk over the step -- with trainer/cached_step.py as it is."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    torch.manual_seed(0)
    m = _tiny(patch_drop_rate=0.5)
    m.text_model.set_dropout(0.0, 0.0)
    opt = AdamW(m.parameters(), lr=3e-5)
    vm = m.video_model
    with mock_hip():
        log = []
        hold = _log_sizes(log)          # noqa: F841
        m.exec_ctx.set_precision("bf16x3", "bf16")
        c0 = vm._drop_calls
        egoclip_step_cached(m, EgoNCE(), opt, _batch(4), 2)
    assert vm._drop_calls == c0 + 2
    draws = [e for e in log if e[0] == "egv_patch_keep_draw"]
    assert len(draws) == 4 and all(e[1:4] == (2, 16, 8) for e in draws)
    p1c0, p1c1, p3c0, p3c1 = (e[4] for e in draws)
    assert p3c0 == p1c0 and p3c1 == p1c1 and p1c0 != p1c1


# ------------------------------------------------------------------------------------------------ the fp64 reference tower
def test_reference_tower_at_k_equals_n_is_the_oracle():
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    from oracle import egovlp_oracle as O
    cfg = O.VideoCfg(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_frames=2)
    m = SpaceTimeTransformer(img_size=32, embed_dim=128, depth=2, num_heads=2, num_frames=2, time_init="rand")
    sd = {"video_model." + k: v.double() for k, v in synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=2).items()}
    g = torch.Generator().manual_seed(0)
    B, T, n = 3, 2, 4
    video = torch.randn(B, T, 3, 32, 32, generator=g, dtype=torch.float64)
    full = np.tile(np.arange(n, dtype=np.int32), (B, 1))
    assert torch.equal(R.tower(video, sd, cfg, full), O.video_encoder(video, sd, cfg))
    assert np.array_equal(R.patch_keep(B, n, n, SEEDS[0]), full)
    # the kept tokens are rows of the full sequence: [CLS, frame 0's, frame 1's]
    keep = np.array([[0, 3], [1, 2], [2, 3]], dtype=np.int32)
    assert R.token_index(keep, T, n).tolist() == [[0, 1, 4, 5, 8], [0, 2, 3, 6, 7], [0, 3, 4, 7, 8]]
    x = O.video_tokens(video, sd, cfg)
    assert torch.equal(R.select_tokens(x, keep, T, n)[1], x[1][[0, 2, 3, 6, 7]])
    # a dropped patch is not an input: changing it changes nothing
    v2 = video.clone()
    v2[0, :, :, :16, 16:] += 1.0            # position 1 of clip 0, every frame
    v2[0, :, :, 16:, :16] -= 1.0            # position 2
    assert torch.equal(R.tower(v2, sd, cfg, keep), R.tower(video, sd, cfg, keep))
    assert not torch.equal(R.tower(v2, sd, cfg, full)[0], R.tower(video, sd, cfg, full)[0])
