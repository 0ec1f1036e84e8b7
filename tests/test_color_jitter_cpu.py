"""Colour jitter in the fused train transform, everything that needs no GPU: known values of the torch restatement of torchvision's ops
(tests/color_jitter_ref.py), the host draws (`train_transform_params_color`), the host logic over the do-nothing C ABI
(tests/mock_hip.py) and the header.  Values on the device: tests/test_gpu_color_jitter.py."""
import itertools
import os
import re

import pytest
import torch

import color_jitter_ref as CJ
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
COLOR = ("egv_patch_gather_u8_aug_color", "egv_patch_gather_u8_aug_color_sel")


def px(r, g, b, dtype=torch.float64):
    return torch.tensor([r, g, b], dtype=dtype).view(3, 1, 1)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_known_values_of_the_restatement(dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 5, 7, generator=g, dtype=torch.float64).to(dtype)
    gray = 0.2989 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2]
    sat0 = CJ.saturation(x, 0.0)
    for c in range(3):
        assert torch.allclose(sat0[:, c], gray, rtol=0, atol=1e-6)
    assert float(CJ.brightness(x, 0.0).abs().max()) == 0.0
    # hue + 1/3: pure red -> pure green -> pure blue -> pure red
    red, green, blue = px(1, 0, 0, dtype), px(0, 1, 0, dtype), px(0, 0, 1, dtype)
    assert torch.allclose(CJ.hue(red, 1.0 / 3.0), green, rtol=0, atol=1e-6)
    assert torch.allclose(CJ.hue(green, 1.0 / 3.0), blue, rtol=0, atol=1e-6)
    assert torch.allclose(CJ.hue(blue, 1.0 / 3.0), red, rtol=0, atol=1e-6)
    # grey pixels (black and white among them) are invariant under saturation and hue, and nothing is NaN.  Under saturation as far as
    # torchvision's grey weights allow: they sum to 0.9999, so a grey level L moves by (1 - f) * 1e-4 * L (clamped at 1)
    for lvl in (0.0, 0.25, 0.5, 1.0):
        p = px(lvl, lvl, lvl, dtype)
        for f in (0.0, 0.6, 1.4, 2.0):
            assert torch.allclose(CJ.saturation(p, f), p, rtol=0, atol=abs(1.0 - f) * 1e-4 * lvl + 1e-6)
        for d in (-0.5, -0.1, 0.1, 0.5):
            out = CJ.hue(p, d)
            assert bool(torch.isfinite(out).all()) and torch.allclose(out, p, rtol=0, atol=1e-6)
    for p in (px(0, 0, 0, dtype), px(1, 1, 1, dtype)):
        for row in ((0.6, 2.0, 0.5, 1 | 2 << 2 | 3 << 4), (1.4, 0.0, -0.5, 3 | 2 << 2 | 1 << 4)):
            assert bool(torch.isfinite(CJ.apply(p, row)).all())
    # hue + 0.5 twice is the identity
    assert torch.allclose(CJ.hue(CJ.hue(x, 0.5), 0.5), x, rtol=0, atol=1e-6)
    # the table row: digits are applied lowest first
    row = (0.5, 0.0, 0.25, 2 | 1 << 2)                      # saturation 0 (-> gray), then brightness 0.5
    want = (0.5 * gray).unsqueeze(1).expand(-1, 3, -1, -1)
    assert torch.allclose(CJ.apply(x, row), want, rtol=0, atol=1e-6)
    assert CJ.ops_of(2 | 1 << 2) == [2, 1] and CJ.ops_of(0) == [] and CJ.ops_of(3 << 4) == [3]
    assert torch.equal(CJ.apply(x, (0.3, 0.3, 0.3, 0)), x)


# ------------------------------------------------------------------------------------------------ the draws
def _draw(n, cj, seed=5, **kw):
    from egovlp_amd.data_loader.transforms import train_transform_params_color
    return train_transform_params_color(n, 256, 341, (0.5, 1.0), cj, generator=torch.Generator().manual_seed(seed), **kw)


def test_draws_ranges_orders_and_determinism():
    boxes, color = _draw(512, (0.4, 0.4, 0.1))
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (512, 5)
    assert color.dtype == torch.float32 and tuple(color.shape) == (512, 4)
    assert bool(((boxes[:, 0] + boxes[:, 2]) <= 256).all()) and bool(((boxes[:, 1] + boxes[:, 3]) <= 341).all())
    assert set(boxes[:, 4].tolist()) <= {0, 1}
    assert 0.6 <= float(color[:, 0].min()) and float(color[:, 0].max()) <= 1.4 and float(color[:, 0].max() - color[:, 0].min()) > 0.7
    assert 0.6 <= float(color[:, 1].min()) and float(color[:, 1].max()) <= 1.4
    assert -0.1 <= float(color[:, 2].min()) and float(color[:, 2].max()) <= 0.1 and float(color[:, 2].min()) < 0 < float(color[:, 2].max())
    orders = {tuple(CJ.ops_of(c)) for c in color[:, 3].tolist()}
    assert orders == set(itertools.permutations((1, 2, 3)))                 # all six orders of three enabled ops
    assert all(float(c) == int(c) and 0 <= int(c) <= 63 for c in color[:, 3].tolist())
    b2, c2 = _draw(512, (0.4, 0.4, 0.1))
    assert torch.equal(boxes, b2) and torch.equal(color, c2)
    b3, c3 = _draw(512, (0.4, 0.4, 0.1), seed=6)
    assert not torch.equal(color, c3)


def test_a_disabled_op_has_no_digit_and_all_disabled_is_the_plain_draw():
    from egovlp_amd.data_loader.transforms import train_transform_params
    _, color = _draw(256, (0.4, 0, 0.1))
    assert bool((color[:, 1] == 1.0).all())
    assert {tuple(CJ.ops_of(c)) for c in color[:, 3].tolist()} == {(1, 3), (3, 1)}
    _, color = _draw(64, (0, 0, 0.5))
    assert {tuple(CJ.ops_of(c)) for c in color[:, 3].tolist()} == {(3,)} and bool((color[:, 3] == 3.0).all())
    assert bool((color[:, 0] == 1.0).all()) and float(color[:, 2].abs().max()) <= 0.5
    # a (1, 1) pair collapses onto the identity as a scalar 0 does
    _, color = _draw(64, ((1.0, 1.0), 0.4, (0.0, 0.0)))
    assert {tuple(CJ.ops_of(c)) for c in color[:, 3].tolist()} == {(2,)}
    for cj in ((0, 0, 0), (0.0, (1, 1), (0, 0))):
        boxes, color = _draw(32, cj, seed=9)
        assert color is None
        assert torch.equal(boxes, train_transform_params(32, 256, 341, (0.5, 1.0), generator=torch.Generator().manual_seed(9)))


def test_pairs_are_honoured_and_bad_ranges_raise():
    _, color = _draw(256, ((0.2, 0.3), (1.5, 3.0), (0.25, 0.5)))
    assert 0.2 <= float(color[:, 0].min()) and float(color[:, 0].max()) <= 0.3
    assert 1.5 <= float(color[:, 1].min()) and float(color[:, 1].max()) <= 3.0 and float(color[:, 1].max()) > 2.0
    assert 0.25 <= float(color[:, 2].min()) and float(color[:, 2].max()) <= 0.5
    _, color = _draw(256, (2.0, 0.4, 0.1))                                   # a scalar above 1: the lower end is clipped at 0
    assert 0.0 <= float(color[:, 0].min()) < 0.2 and 2.5 < float(color[:, 0].max()) <= 3.0
    for bad in ((0.4, 0.4, 0.6), (0.4, 0.4, (-0.6, 0.1)), (-0.1, 0.4, 0.1), (0.4, (1.2, 0.8), 0.1), (0.4, (-0.5, 1.0), 0.1), (0.4, 0.4, -0.1)):
        with pytest.raises(ValueError):
            _draw(4, bad)
    with pytest.raises(TypeError):
        _draw(4, (0.4, "0.4", 0.1))
    with pytest.raises(ValueError):
        _draw(4, (0.4, 0.4))


# ------------------------------------------------------------------------------------------------ host logic over the mock C ABI
class OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: what the host code treats as a device-resident table (never read, never
    validated).  The mock library computes nothing, so nothing dereferences it."""
    is_cuda = True


def dev(t):
    return t.as_subclass(OnDevice)


def _tiny(**extra):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
    vp.update(extra)
    return FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _tables(B, seed=1):
    from egovlp_amd.data_loader.transforms import train_transform_params_color
    return train_transform_params_color(B, 80, 100, (0.5, 1.0), (0.4, 0.4, 0.1), generator=torch.Generator().manual_seed(seed))


def _log_color(log):
    """The two colour entry points of the mock replaced by callbacks that record (name, frames, the four numbers of the table's first
    row): the table is host memory here, so the pointer the host code passed can be read."""
    import ctypes as C
    from egovlp_amd import _lib
    mock, hold = _lib._lib, []
    for name in COLOR:
        res, args = _lib.PROTOTYPES[name]
        inner = getattr(mock, name)

        def cb(*a, _name=name, _inner=inner):
            first = C.cast(a[9], C.POINTER(C.c_float))
            log.append((_name, int(a[1])) + tuple(first[k] for k in range(4)))
            return _inner(*a)
        fn = C.CFUNCTYPE(res, *args)(cb)
        hold.append(fn)
        setattr(mock, name, fn)
    return hold


def test_forward_without_a_table_makes_the_parents_calls_and_with_one_the_colour_gather():
    torch.manual_seed(0)
    m, md = _tiny(), _tiny(patch_drop_rate=0.5)
    B = 2
    u8 = (torch.rand(B, 2, 3, 80, 100) * 255).to(torch.uint8)
    boxes, color = _tables(B)
    with mock_hip() as calls:
        for mod in (m, md):
            mod.exec_ctx.set_precision("bf16x3", "bf16")
        vm, vd = m.video_model, md.video_model
        for v_ in (vm, vd):
            v_.set_input_augmentation(dev(boxes), 64)
            v_(u8).sum().backward()                                         # builds the weight-plane and workspace-size caches
        calls.clear()
        # no table: the calls of set_input_augmentation(boxes, out_res) as they were
        vm.set_input_augmentation(dev(boxes), 64)
        vm(u8)
        plain = list(calls)
        calls.clear()
        vm.set_input_augmentation(dev(boxes), 64, color=None)
        vm(u8)
        assert list(calls) == plain and plain.count("egv_patch_gather_u8_aug") == 1 and not any("_color" in c for c in plain)
        # with a table: exactly one colour gather in place of the plain one, everything else as before
        calls.clear()
        vm.set_input_augmentation(dev(boxes), 64, dev(color))
        assert tuple(vm(u8).shape) == (B, 128)
        with_color = list(calls)
        assert with_color.count("egv_patch_gather_u8_aug_color") == 1 and "egv_patch_gather_u8_aug" not in with_color
        assert "egv_patch_gather_u8_aug_color_sel" not in with_color
        assert [c.replace("_aug_color", "_aug") for c in with_color] == plain
        # one-shot: the next forward on fp32 frames is the plain gather
        calls.clear()
        vm(torch.randn(B, 2, 3, 64, 64))
        assert calls.count("egv_patch_gather") == 1 and not any("_aug" in c for c in calls)
        # patch dropout in train mode: the _sel twin; in eval mode the full kernel
        calls.clear()
        vd.set_input_augmentation(dev(boxes), 64, dev(color))
        vd(u8).sum().backward()
        assert calls.count("egv_patch_gather_u8_aug_color_sel") == 1 and calls.count("egv_patch_keep_draw") == 1
        assert not {"egv_patch_gather_u8_aug_color", "egv_patch_gather_u8_aug", "egv_patch_gather_u8_aug_sel"} & set(calls)
        calls.clear()
        vd.set_input_augmentation(dev(boxes), 64)
        vd(u8)
        assert calls.count("egv_patch_gather_u8_aug_sel") == 1 and not any("_color" in c for c in calls)
        calls.clear()
        md.eval()
        vd.set_input_augmentation(dev(boxes), 64, dev(color))
        with torch.no_grad():
            vd(u8)
        assert calls.count("egv_patch_gather_u8_aug_color") == 1 and "egv_patch_gather_u8_aug_color_sel" not in calls


def test_ops_refuse_a_bad_colour_table_before_any_launch():
    from egovlp_amd import ops
    B = 2
    u8 = torch.zeros(B, 2, 3, 80, 100, dtype=torch.uint8)
    boxes, color = _tables(B)
    boxes, color = dev(boxes), dev(color)
    keep = torch.zeros(B, 5, dtype=torch.int32)
    with mock_hip() as calls:
        for bad in (color.double(), color[:1], color[:, :3], color.t().contiguous().t(), color.view(-1), color.tolist(),
                    torch.ones(B, 4)):                                     # the last: not on the device
            with pytest.raises(ValueError):
                ops.patch_gather(u8, 16, 3, aug=(boxes, 64), color=bad)
        with pytest.raises(ValueError):
            ops.patch_gather(u8, 16, 3, color=color)                        # no aug
        with pytest.raises(ValueError):
            ops.patch_gather(torch.zeros(B, 2, 4, 80, 100, dtype=torch.uint8), 16, 3, (0.5,) * 4, (0.25,) * 4, aug=(boxes, 64), color=color)
        assert not calls
        assert ops.patch_gather(u8, 16, 3, aug=(boxes, 64), color=color).rows == B * 2 * 16
        assert ops.patch_gather(u8, 16, 3, aug=(boxes, 64), color=color, keep=keep).rows == B * 2 * 5
        assert ops.patch_gather(u8, 16, 3, aug=(boxes, 64)).rows == B * 2 * 16
        assert list(calls) == ["egv_patch_gather_u8_aug_color", "egv_patch_gather_u8_aug_color_sel", "egv_patch_gather_u8_aug"]


def test_host_table_is_validated_and_a_device_table_is_not_read():
    m = _tiny()
    vm = m.video_model
    boxes, color = _tables(2)

    def with_(col, val, row=0):
        c = color.clone()
        c[row, col] = val
        return c
    bad = [with_(0, float("nan")), with_(1, float("inf")), with_(0, -0.1), with_(1, -1e-3), with_(2, 0.51), with_(2, -0.6),
           with_(3, 64.0), with_(3, -1.0), with_(3, 2.5), with_(3, float("nan"), 1),
           color[:1], color[:, :3], color.view(-1), color.long(), color.tolist()]
    for c in bad:
        with pytest.raises(ValueError, match="color"):
            vm.set_input_augmentation(boxes, 64, c)
        assert getattr(vm, "_input_aug", None) is None                      # a refused table leaves nothing pending
    for c in bad[:10]:
        with pytest.raises(ValueError, match="finite.*>= 0.*0.5.*0..63"):    # the message names the rule
            vm.set_input_augmentation(boxes, 64, c)
    # the corners of the rule pass
    ok = color.clone()
    ok[0] = torch.tensor([0.0, 3.0, 0.5, 63.0])
    ok[1] = torch.tensor([1.0, 0.0, -0.5, 0.0])
    vm.set_input_augmentation(boxes, 64, ok)
    assert len(vm._input_aug) == 4 and vm._input_aug[3].dtype == torch.float32
    vm._input_aug = None
    vm.set_input_augmentation(boxes, 64, ok.double())                       # any float type; the kernel's is fp32
    assert vm._input_aug[3].dtype == torch.float32
    vm._input_aug = None
    # a device table is taken as it is: these rows would be refused on the host
    vm.set_input_augmentation(dev(boxes), 64, dev(with_(0, float("nan"))))
    vm._input_aug = None
    # not combinable with a pending eval transform, as without a table
    vm.set_input_eval_transform(72, 64)
    with pytest.raises(ValueError):
        vm.set_input_augmentation(boxes, 64, color)
    vm._input_eval = None


def test_cached_step_passes_each_chunk_its_slice_in_both_passes():
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    torch.manual_seed(0)
    B, chunk, T = 4, 2, 2
    b = synth_batch(B, T=T, L=16, seed=3, res=64)
    data = {"video": (torch.rand(B, T, 3, 80, 100) * 255).to(torch.uint8), "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}
    boxes, color = _tables(B, seed=2)
    assert len({tuple(r) for r in color.tolist()}) == B
    for keys, name in ((dict(), COLOR[0]), (dict(patch_drop_rate=0.5), COLOR[1])):
        m = _tiny(**keys)
        m.text_model.set_dropout(0.0, 0.0)
        opt = AdamW(m.parameters(), lr=3e-5)
        with mock_hip() as calls:
            log = []
            hold = _log_color(log)              # noqa: F841  (the callbacks must outlive the calls)
            m.exec_ctx.set_precision("bf16x3", "bf16")
            egoclip_step_cached(m, EgoNCE(), opt, data, chunk, aug_boxes=dev(boxes), aug_color=dev(color))
            rows = [tuple(color[lo].tolist()) for lo in (0, 2)]
            assert log == [(name, chunk * T) + r for r in rows] * 2, log      # pass 1 over the chunks, then pass 3
            assert not {"egv_patch_gather_u8_aug", "egv_patch_gather_u8_aug_sel"} & set(calls)
            # without a table: the calls the step made before
            calls.clear()
            del log[:]
            egoclip_step_cached(m, EgoNCE(), opt, data, chunk, aug_boxes=dev(boxes))
            assert not log and calls.count(name.replace("_color", "")) == 4
            with pytest.raises(ValueError):
                egoclip_step_cached(m, EgoNCE(), opt, data, chunk, aug_color=dev(color))


# ------------------------------------------------------------------------------------------------ the header
def test_header_prototypes_match_the_ctypes_prototypes():
    """The two declarations, argument by argument: pointers -> c_void_p, int32_t -> c_int32, int64_t -> c_int64; and the plain
    entry points' lists with `color` taken out."""
    import ctypes as C
    from egovlp_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egovlp_hip.h")).read(), flags=re.S)
    kind = {"int32_t": C.c_int32, "int64_t": C.c_int64}

    def declared(name):
        args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, flags=re.S).group(1)
        out = []
        for a in args.split(","):
            a = a.strip()
            out.append((a.split()[-1].lstrip("*"), C.c_void_p if "*" in a else kind[a.split()[0]]))
        return out
    for name in COLOR:
        d = declared(name)
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int32 and [t for _, t in d] == list(args), name
        names = [n for n, _ in d]
        assert names.index("color") == names.index("boxes") + 1
        plain = declared(name.replace("_color", ""))
        assert [x for x in d if x[0] != "color"] == plain
        assert list(_lib.PROTOTYPES[name.replace("_color", "")][1]) == [t for _, t in plain]
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", hdr).group(1)) == 6 == _lib.ABI_VERSION
