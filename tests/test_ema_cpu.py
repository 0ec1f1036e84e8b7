"""The weight average (egovlp_amd/ema.py, csrc/ema.hip) without a GPU: the references of tests/ema_ref.py judged on their own, and the
host side -- ModelEMA, AdamW.skip_flag(), the trainers' switch, checkpoints -- on CPU tensors over the do-nothing C-ABI stand-in
(tests/mock_hip.py): which entry points an epoch calls, in which order.  Nothing about the kernels' values: tests/test_gpu_ema.py."""
import ctypes
import logging
import os
import re
import types

import pytest
import torch

import ema_ref as E
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA_CALLS = ("egv_ema_decide", "egv_ema_update_multi", "egv_swap_multi")


# ---------------------------------------------------------------------------------------------------------------- the references
def test_fp32_restatement_stays_inside_the_bound_on_the_gpu_tests_inputs():
    """e + w * (p - e) in fp32 torch arithmetic (three roundings) against ema_ref64 on every case and weight tests/test_gpu_ema.py runs."""
    worst = 0.0
    for which in E.CASES:
        es, ps = E.case_inputs(which)
        e, p = torch.cat(es), torch.cat(ps)
        for w in E.WEIGHTS:
            wf = torch.tensor(E.f32(w), dtype=torch.float32)
            got = e + wf * (p - e)
            ratio = E.check_ema(got, E.ema_ref64(e, p, w), e, p, w, what="%s w=%g" % (which, w))
            print("%-12s w = %-8g largest err / (u s) = %.3f" % (which, w, ratio))
            worst = max(worst, ratio)
    print("largest err / (u s) over all cases: %.3f (allowed %d)" % (worst, E.K_EMA))
    assert worst <= E.K_EMA


def test_check_ema_sees_one_element_moved_by_8_u_s():
    g = torch.Generator().manual_seed(5)
    e, p, w = torch.randn(130000, generator=g), torch.randn(130000, generator=g), 0.25
    ref = E.ema_ref64(e, p, w)
    got = ref.float()
    E.check_ema(got, ref, e, p, w)
    i = 77777
    s = float(E.ema_scale(e, p, w)[i])
    bad = got.clone()
    bad[i] = float(ref[i] + 8 * E.U * s)
    with pytest.raises(AssertionError, match=r"\[77777 of 130000\]"):
        E.check_ema(bad, ref, e, p, w)


def test_decay_rule_against_values_written_out_by_hand():
    f = lambda x: ctypes.c_float(x).value
    assert E.decay_ref(0.9999, True, 0) == (f(0.1), f(0.9))                      # (1 + 0) / (10 + 0)
    assert E.decay_ref(0.9999, True, 90) == (f(0.91), f(1.0 - 0.91))             # 91 / 100
    # the warm-up term reaches 0.9999 at t = 89 990: 89 991 / 90 000 = 0.9999, and one update earlier it is still below
    assert abs((1.0 + 89990) / (10.0 + 89990) - 0.9999) < 1e-15 and (1.0 + 89989) / (10.0 + 89989) < 0.9999
    assert E.decay_ref(0.9999, True, 89000)[0] == f(89001.0 / 89010.0) < f(0.9999)
    for t in (89990, 89991, 10 ** 6, 2 ** 31 - 2):
        assert E.decay_ref(0.9999, True, t) == (f(0.9999), f(1.0 - f(0.9999)))
    # the decay in effect never decreases and never exceeds the configured one
    ds = [E.decay_ref(0.9999, True, t)[0] for t in range(0, 100000, 997)]
    assert ds == sorted(ds) and ds[-1] == f(0.9999)
    # warm-up off: the configured decay from the first update on
    for t in (0, 1, 90, 89990):
        assert E.decay_ref(0.9999, False, t) == (f(0.9999), f(1.0 - f(0.9999)))
    assert E.decay_ref(0.0, False, 0) == (0.0, 1.0) and E.decay_ref(0.0, True, 5) == (0.0, 1.0)
    # a skipped call moves nothing but the skipped count and w
    st = {"t": 3, "w": 0.5, "skipped": 1, "decay": 0.5}
    assert E.decide_ref(st, True, 0.9, True) == {"t": 3, "w": 0.0, "skipped": 2, "decay": 0.5}
    assert E.decide_ref(st, False, 0.9, True) == {"t": 4, "w": f(1.0 - 4.0 / 13.0), "skipped": 1, "decay": f(4.0 / 13.0)}


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    from egovlp_amd import _lib
    txt = open(os.path.join(ROOT, "include", "egovlp_hip.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in EMA_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, nc), name
        assert name in _lib.PROTOTYPES
    assert int(re.search(r"#define EGV_ABI_VERSION (\d+)", txt).group(1)) == 6 == _lib.ABI_VERSION
    assert "ema.hip" in open(os.path.join(ROOT, "egovlp_amd", "csrc", "Makefile")).read()
    assert E.TABLE == E.R.source_constants("ema.hip")["EMA_MAX_T"] and E.CHUNK == E.R.source_constants("ema.hip")["CHUNK"]


# ---------------------------------------------------------------------------------------------------------------- ops / optimizer
def test_wrappers_reuse_their_tables_and_check_their_arguments():
    from egovlp_amd import ops
    with mock_hip() as calls:
        a, b = [torch.zeros(5), torch.zeros(8)], [torch.ones(5), torch.ones(8)]
        state = torch.zeros(8, dtype=torch.int32)
        assert ops.ema_update_multi([], [], state).n == 0 and ops.swap_multi([], []).n == 0 and calls == []
        t1 = ops.ema_update_multi(a, b, state)
        t2 = ops.ema_update_multi(a, b, state, t1)
        assert t2 is t1                                               # same addresses, same sizes: the tables are reused
        assert ops.swap_multi(a, b, t1) is t1
        b2 = [torch.ones(5), torch.ones(8)]
        t3 = ops.ema_update_multi(a, b2, state, t1)
        assert t3 is not t1 and t3.key != t1.key                      # another data_ptr(): rebuilt
        assert ops.ema_update_multi(a[:1], b[:1], state, t1) is not t1
        assert calls == ["egv_ema_update_multi"] * 2 + ["egv_swap_multi"] + ["egv_ema_update_multi"] * 2
        ops.ema_decide(state, None, 0.99, True)
        ops.ema_decide(state, torch.zeros(1), 0.0, False)
        assert calls[-2:] == ["egv_ema_decide"] * 2
        for bad in (1.0, -0.1, float("nan")):
            with pytest.raises(ValueError):
                ops.ema_decide(state, None, bad, True)
        for fn in (lambda x, y: ops.ema_update_multi(x, y, state), ops.swap_multi):
            with pytest.raises(ValueError):
                fn(a, b[:1])
            with pytest.raises(ValueError):
                fn([a[0]], [b[0][:4]])
            with pytest.raises(ValueError):
                fn([a[0]], [b[0].double()])
            with pytest.raises(ValueError):
                fn([torch.zeros(4, 4).t()], [torch.zeros(4, 4)])


def _five(scale=1.0):
    g = torch.Generator().manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (3, 70, 64, 65, 4)]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g) * scale
    return params


def test_skip_flag_is_none_without_scaler_and_clipping_and_a_view_otherwise():
    from egovlp_amd.optim import AdamW, LossScaler
    with mock_hip() as calls:
        params = _five()
        opt = AdamW(params, lr=1e-3)
        assert opt.skip_flag() is None
        opt.step()
        plain = list(calls)
        assert opt.skip_flag() is None                                  # such a step is always applied
        # a scaler: the [3] element of the scaler's own block (state words 4 .. 7)
        sc = LossScaler(init_scale=4.0, device="cpu")
        opt.step(scaler=sc)
        f = opt.skip_flag()
        assert f.dtype == torch.float32 and f.numel() == 1 and f.data_ptr() == sc.state.data_ptr() + 7 * 4
        opt.step()
        assert opt.skip_flag() is None                                  # the LAST step decides
        # clipping without a scaler: the optimizer's own first block; with one: the scaler's
        clip = AdamW(_five(), lr=1e-3, max_grad_norm=1.0)
        del calls[:]
        clip.step()
        f = clip.skip_flag()
        assert f.dtype == torch.float32 and f.numel() == 1 and f.data_ptr() == clip._clip_hyper.data_ptr() + 3 * 4
        clip.step(scaler=sc)
        assert clip.skip_flag().data_ptr() == sc.state.data_ptr() + 7 * 4
        # an accessor only: no entry point is called by it, and the plain step makes the calls it made
        n = len(calls)
        clip.skip_flag(), opt.skip_flag()
        assert len(calls) == n
        del calls[:]
        opt.step()
        assert list(calls) == plain == ["egv_adamw_multi"]
        # two groups, the first without gradients: the flag is the block of the first launch
        ps = _five()
        ps[0].grad = None
        two = AdamW([{"params": ps[:1]}, {"params": ps[1:]}], lr=1e-3)
        two.step(scaler=sc)
        assert two.skip_flag().data_ptr() == sc.hyper_block(1).data_ptr() + 3 * 4


def test_model_ema_host_side():
    from egovlp_amd import weights
    from egovlp_amd.ema import ModelEMA
    from egovlp_amd.optim import AdamW
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 7, bias=False))
    net[1].weight.requires_grad_(False)                                # covered whatever its requires_grad
    wrapped = types.SimpleNamespace(module=net)
    with mock_hip() as calls:
        ema = ModelEMA(wrapped, decay=0.99)
        assert list(ema.shadow) == ["0.weight", "0.bias", "1.weight"]
        assert all(v.data_ptr() % 16 == 0 for v in ema._views) and ema.arena_bytes() == 4 * (16 + 4 + 24)
        for k, p in net.named_parameters():
            assert torch.equal(ema.shadow[k], p.detach()) and ema.shadow[k].dtype == torch.float32
        assert calls == []                                             # the arena is filled by a copy, no entry point
        opt = AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3)
        ema.update(opt)
        tables = ema._tables
        ema.update()
        assert calls == ["egv_ema_decide", "egv_ema_update_multi"] * 2 and ema._tables is tables
        epoch = weights.EPOCH
        with ema.swapped():
            assert weights.EPOCH == epoch + 1 and ema.is_swapped()
            with pytest.raises(RuntimeError):
                ema.update(opt)
            with pytest.raises(RuntimeError):
                ema.load_state_dict(ema.state_dict())
        assert weights.EPOCH == epoch + 2 and not ema.is_swapped() and ema._tables is tables
        with pytest.raises(ZeroDivisionError):
            with ema.swapped():
                1 / 0
        assert not ema.is_swapped()                                    # swapped back in a `finally`
        assert calls[4:] == ["egv_swap_multi"] * 4
        sd = ema.state_dict()
        assert set(sd) == {"shadow", "num_updates", "skipped", "decay", "warmup"} and sd["decay"] == 0.99 and sd["warmup"] is True
        assert all(v.device.type == "cpu" and v.dtype == torch.float32 and v.shape == dict(net.named_parameters())[k].shape
                   for k, v in sd["shadow"].items())
        net.load_state_dict(sd["shadow"], strict=False)                # loads into the model as it is
        # strict names and shapes
        other = ModelEMA(net, decay=0.5, warmup=False)
        sd["num_updates"], sd["skipped"] = 7, 2
        sd["shadow"]["0.bias"] = torch.full((3,), 2.5)
        other.load_state_dict(sd)
        assert other.num_updates() == 7 and other.skipped_updates() == 2 and float(other.shadow["0.bias"][1]) == 2.5
        assert other.decay == 0.5 and other.warmup is False
        with pytest.raises(KeyError):
            other.load_state_dict({"shadow": {k: v for k, v in sd["shadow"].items() if k != "0.bias"}})
        with pytest.raises(KeyError):
            other.load_state_dict({"shadow": dict(sd["shadow"], extra=torch.zeros(1))})
        with pytest.raises(ValueError):
            other.load_state_dict({"shadow": dict(sd["shadow"], **{"0.bias": torch.zeros(4)})})
        other.copy_to()
        assert float(net[0].bias.detach()[1]) == 2.5
    with pytest.raises(ValueError):
        ModelEMA(net, decay=1.0)
    with pytest.raises(ValueError):
        ModelEMA(torch.nn.Linear(2, 2).double())


# ---------------------------------------------------------------------------------------------------------------- the trainer
TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
STEPS = 3


def _tiny():
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _batch(B):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=3, res=32)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


class _Loader:
    batch_size, n_samples = 4, 4 * STEPS

    def __len__(self):
        return STEPS

    def __iter__(self):
        return iter([_batch(self.batch_size) for _ in range(STEPS)])


class _ValLoader:
    """Two EgoMCQ questions: one query, five candidate clips."""

    def __iter__(self):
        for k in range(2):
            b = _batch(5)
            yield {"video": b["video"][None], "text": {key: v[:1] for key, v in b["text"].items()},
                   "correct": torch.tensor([k]), "type": torch.tensor([1])}


class _Writer:
    def __init__(self):
        self.tags = []

    def add_scalar(self, tag, value, step):
        self.tags.append(tag)


def _trainer(model, **args):
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import AllGather_multi, Multi_Trainer_dist
    tr = Multi_Trainer_dist.__new__(Multi_Trainer_dist)          # without Multi_BaseTrainer_dist.__init__, which needs a HIP device
    tr.args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=3e-5, schedule=[], **args)
    tr.model, tr.loss, tr.metrics, tr.device = model, EgoNCE(), [], torch.device("cpu")
    tr.optimizer = AdamW(model.parameters(), lr=3e-5)
    tr.data_loader, tr.valid_data_loader, tr.do_validation = [_Loader()], [_ValLoader()], True
    tr.len_epoch, tr.total_batch_sum, tr.max_samples_per_epoch = STEPS, 4, 50000
    tr.batch_size, tr.log_step, tr.n_gpu = 4, 1, 1
    tr.tokenizer, tr.writer, tr.grad_sync, tr.allgather = None, _Writer(), None, AllGather_multi.apply
    tr._guard = types.SimpleNamespace(maybe_check=lambda data: None)
    tr.logger, tr.config, tr.mnt_best = logging.getLogger("test_ema"), {}, 0
    return tr


def _epoch(tr, calls):
    del calls[:]
    tr._train_epoch(1)
    return list(calls)


def _steps(seq):
    """The call list of an epoch cut behind every step's last AdamW call -> the pieces that FOLLOW each step's optimizer calls."""
    ends = [i for i, n in enumerate(seq) if n == "egv_adamw_multi" and (i + 1 == len(seq) or seq[i + 1] != "egv_adamw_multi")]
    return [seq[a + 1:b + 1] for a, b in zip(ends, ends[1:] + [len(seq) - 1])]


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return _tiny()


def test_epoch_call_lists_with_the_average_off_and_on(tiny):
    with mock_hip() as calls:
        tiny.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            _epoch(_trainer(tiny), calls)                                    # builds the weight-plane cache, asks for the workspace sizes
            _epoch(_trainer(tiny, embed_cache_chunk=2), calls)               # ... and for those of the chunks' shapes
            absent = _trainer(tiny)
            off_absent = _epoch(absent, calls)
            off_none = _epoch(_trainer(tiny, model_ema_decay=None), calls)
            off_zero = _epoch(_trainer(tiny, model_ema_decay=0), calls)
            tr = _trainer(tiny, model_ema_decay=0.99)
            on = _epoch(tr, calls)
            on_cached = _epoch(_trainer(tiny, model_ema_decay=0.99, embed_cache_chunk=2), calls)
            off_cached = _epoch(_trainer(tiny, embed_cache_chunk=2), calls)
            no_eval = _epoch(_trainer(tiny, model_ema_decay=0.99, model_ema_eval=False), calls)
            tags_on, tags_off = tr.writer.tags, absent.writer.tags
        finally:
            tiny.exec_ctx.unset("fwd_passes", "bwd_passes")
    # off: the same list whether the attribute is absent, None or 0, and no entry point of the average in it
    assert off_absent == off_none == off_zero and not any(n in EMA_CALLS for n in off_absent)
    assert off_absent.count("egv_adamw_multi") >= STEPS and absent.ema is None
    # on: the off list plus the average's calls, nothing else moved
    assert [n for n in on if n not in EMA_CALLS] == off_absent
    assert [n for n in on_cached if n not in EMA_CALLS] == off_cached and off_cached.count("egv_grad_accumulate_multi") == STEPS
    # exactly one decide right behind the AdamW calls of each step, the update launch right behind that decide
    for seq in (on, on_cached, no_eval):
        assert seq.count("egv_ema_decide") == seq.count("egv_ema_update_multi") == STEPS
        tails = _steps(seq)
        assert len(tails) == STEPS
        for tail in tails:
            assert tail[:2] == ["egv_ema_decide", "egv_ema_update_multi"], tail[:4]
    # the same calls per step with the embedding cache: one update per optimizer step, not per chunk
    assert [n for n in on_cached if n in EMA_CALLS] == [n for n in on if n in EMA_CALLS]
    # validation is bracketed by the two swaps: every call behind the last update belongs to it
    last = max(i for i, n in enumerate(on) if n == "egv_ema_update_multi")
    val = on[last + 1:]
    assert val[0] == "egv_swap_multi" and val[-1] == "egv_swap_multi" and val.count("egv_swap_multi") == 2
    assert len(val) > 2 and val[1:-1] == off_absent[len(off_absent) - (len(val) - 2):]
    assert "egv_swap_multi" not in on[:last] and "egv_swap_multi" not in no_eval
    assert [n for n in no_eval if n not in EMA_CALLS] == off_absent
    assert not tr.ema.is_swapped() and tr.ema.num_updates() == 0              # the stand-in computes nothing: the state block stays zero
    # the writer logs the decay where the loss is logged
    assert tags_on.count("Loss_training/ema_decay_0") == tags_on.count("Loss_training/loss_0") == STEPS
    assert not any("ema" in t for t in tags_off)


def test_checkpoint_carries_the_average_and_a_resume_restores_it(tiny, tmp_path):
    with mock_hip():
        tiny.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            tr = _trainer(tiny, model_ema_decay=0.99)
            tr.do_validation = False
            tr._train_epoch(1)
            tr.ema._state[0], tr.ema._state[2] = 5, 1                          # what three applied updates would leave is the kernel's business
            tr.ema._views[3].fill_(0.125)
            state = tr._checkpoint_state(1)
            assert set(state["ema_state_dict"]) == {"shadow", "num_updates", "skipped", "decay", "warmup"}
            assert state["ema_state_dict"]["num_updates"] == 5 and list(state["ema_state_dict"]["shadow"]) == [k for k, _ in tiny.named_parameters()]
            assert "ema_state_dict" not in _trainer(tiny)._checkpoint_state(1)  # off: the checkpoint is what it was
            with tr.ema.swapped():
                with pytest.raises(RuntimeError):
                    tr._checkpoint_state(1)                                     # never while the model holds the averaged weights
            path = tmp_path / "ck.pth"
            torch.save({k: v for k, v in state.items() if k != "config"} | {"config": {}}, str(path))
            fresh = _trainer(tiny, model_ema_decay=0.99)
            fresh._resume_checkpoint(str(path))
            assert fresh.ema.num_updates() == 5 and fresh.ema.skipped_updates() == 1 and fresh.start_epoch == 2
            for a, b in zip(fresh.ema._views, tr.ema._views):
                assert torch.equal(a, b)
            assert float(fresh.ema._views[3][0]) == 0.125
            # a checkpoint without the key: the average starts from the loaded weights, counters at zero
            old = {k: v for k, v in torch.load(str(path), weights_only=False).items() if k != "ema_state_dict"}
            torch.save(old, str(path))
            again = _trainer(tiny, model_ema_decay=0.99)
            again._resume_checkpoint(str(path))
            assert again.ema.num_updates() == 0 and again.ema.skipped_updates() == 0
            for v, p in zip(again.ema._views, again.ema._params):
                assert torch.equal(v, p.detach().reshape(-1))
            off = _trainer(tiny)
            off._resume_checkpoint(str(path))
            assert off.ema is None
        finally:
            tiny.exec_ctx.unset("fwd_passes", "bwd_passes")
