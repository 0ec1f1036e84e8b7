"""Host side of gradient clipping by global norm (`AdamW(max_grad_norm=...)`, egovlp_amd/optim.py) on CPU tensors: the call census of
the EgoClip steps over the do-nothing C-ABI stand-in (tests/mock_hip.py), the host restatement of the rule against
torch.nn.utils.clip_grad_norm_, constructor validation, the state_dict round trip and the configuration path.  Values on the device:
tests/test_gpu_grad_clip.py.

tests/golden/grad_clip_parent_calls.json holds, for the four (precision, step) cases of `census`, the length and the SHA-256 of the
call list of the commit BEFORE `max_grad_norm` existed (written by running `census({})` of this file on that commit): with clipping
off a step must make exactly those calls, in that order."""
import collections
import hashlib
import inspect
import json
import math
import os

import pytest
import torch

from mock_hip import mock_hip

HERE = os.path.dirname(os.path.abspath(__file__))

TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
MODES = {"bf16": ("bf16x3", "bf16"), "f16": ("f16mix", "f16")}       # without / with the model's loss scaler


def _tiny():
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _batch(B):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=3, rank=0, res=32)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


def census(opt_kwargs):
    """{"<mode>/<step>": call list} of a steady-state `egoclip_step` (B = 2) and of `egoclip_step_cached` (B = 6 in 3 chunks)."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    out = {}
    for mode, prec in MODES.items():
        torch.manual_seed(0)
        model = _tiny()
        opt = AdamW(model.parameters(), lr=3e-5, **opt_kwargs)
        with mock_hip() as calls:
            model.exec_ctx.set_precision(*prec)
            egoclip_step(model, EgoNCE(), opt, _batch(2), 1, 0)              # builds the weight-plane cache and the optimizer's plans
            calls.clear()
            egoclip_step(model, EgoNCE(), opt, _batch(2), 1, 0)
            out[mode + "/plain"] = list(calls)
            calls.clear()
            egoclip_step_cached(model, EgoNCE(), opt, _batch(6), 2, 1, 0)
            out[mode + "/cached"] = list(calls)
    return out


def digest(calls):
    return {"n": len(calls), "sha256": hashlib.sha256("\n".join(calls).encode()).hexdigest()}


@pytest.fixture(scope="module")
def parent_calls():
    with open(os.path.join(HERE, "golden", "grad_clip_parent_calls.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("off", [{}, {"max_grad_norm": None}, {"max_grad_norm": 0}, {"max_grad_norm": float("inf")}],
                         ids=["default", "None", "0", "inf"])
def test_clipping_off_makes_exactly_the_calls_of_the_parent_commit(parent_calls, off):
    got = census(off)
    assert set(got) == set(parent_calls)
    for case, calls in got.items():
        assert digest(calls) == parent_calls[case], case
        assert "egv_grad_sqnorm_multi" not in calls and "egv_grad_clip_update" not in calls and "egv_grad_sqnorm_parts" not in calls


def test_clipping_on_replaces_the_scan_and_decides_once_per_step():
    off, on = census({}), census({"max_grad_norm": 1.0})
    for case in off:
        a, b = collections.Counter(off[case]), collections.Counter(on[case])
        scaler = case.startswith("f16")
        assert a["egv_grad_nonfinite_multi"] == (1 if scaler else 0), case
        # one reduction group and one decision per STEP, also in the cached step with its 3 chunks; the scan is gone
        assert b["egv_grad_sqnorm_multi"] == 1 and b["egv_grad_clip_update"] == 1 and b["egv_grad_nonfinite_multi"] == 0, case
        assert b["egv_grad_sqnorm_parts"] == 0, case                 # steady state: the partials buffer is sized once
        if case.endswith("cached"):
            assert b["egv_grad_accumulate_multi"] == 2, case
        # nothing else changes: the same calls, as often
        for name in set(a) | set(b):
            if name not in ("egv_grad_nonfinite_multi", "egv_grad_sqnorm_multi", "egv_grad_clip_update"):
                assert a[name] == b[name], (case, name)
        seq = on[case]
        i_sq, i_clip = seq.index("egv_grad_sqnorm_multi"), seq.index("egv_grad_clip_update")
        first_adam = seq.index("egv_adamw_multi")
        assert i_sq < i_clip < first_adam, case                      # reduce, decide, update
        if scaler:
            lsu = [i for i, n in enumerate(seq) if n == "egv_loss_scale_update"]
            assert i_sq < lsu[0] and lsu[-1] < i_clip, case          # the clip decision follows the scale decision
        else:
            assert "egv_loss_scale_update" not in seq, case
        if case.endswith("cached"):
            assert max(i for i, n in enumerate(seq) if n == "egv_grad_accumulate_multi") < i_sq, case    # the norm of the SUMMED gradients


def test_partials_follow_the_parameter_set():
    """The partials buffer is sized at the first step and again when the list of gradient sizes changes -- not in between."""
    from egovlp_amd.optim import AdamW
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (5, 70000, 3)]
    opt = AdamW(ps, lr=1e-3, max_grad_norm=1.0)
    with mock_hip() as calls:
        for _ in range(2):
            for p in ps:
                p.grad = torch.ones_like(p)
            opt.step()
        assert calls.count("egv_grad_sqnorm_parts") == 1 and calls.count("egv_grad_sqnorm_multi") == 2
        ps[1].grad = None                                            # a parameter drops out: another list
        opt.step()
        assert calls.count("egv_grad_sqnorm_parts") == 2 and calls.count("egv_grad_clip_update") == 3
        for p in ps:
            p.grad = None
        opt.step()                                                   # no gradients at all: nothing to do
        assert calls.count("egv_grad_sqnorm_multi") == 3 and calls.count("egv_grad_clip_update") == 3


def test_clip_coefficient_is_clip_grad_norm_s_scaling():
    from egovlp_amd.optim import clip_coefficient
    g = torch.Generator().manual_seed(7)
    for scale, max_norm in [(1.0, 0.5), (1.0, 1e3), (30.0, 1.0), (1e-4, 1.0), (2.0, 2.0)]:
        ps = [torch.nn.Parameter(torch.zeros(s)) for s in ((7,), (33, 5), (1,))]
        grads = [torch.randn(p.shape, generator=g, dtype=torch.float64) * scale for p in ps]
        for p, gr in zip(ps, grads):
            p.grad = gr.float()
        before = [p.grad.clone() for p in ps]
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        norm = math.sqrt(sum(float((b.double() ** 2).sum()) for b in before))
        assert abs(total - norm) <= 1e-6 * norm
        c = clip_coefficient(norm, max_norm)
        assert 0.0 < c <= 1.0 and (c == 1.0) == (max_norm >= norm + 1e-6)
        for p, b in zip(ps, before):
            assert torch.allclose(p.grad, b * c, rtol=1e-6, atol=0.0)        # what torch did to the gradients
    assert clip_coefficient(0.0, 1.0) == 1.0 and clip_coefficient(10.0, 1.0) == pytest.approx(1.0 / (10.0 + 1e-6))


def test_constructor_validation_and_off_values():
    from egovlp_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    for off in (None, 0, 0.0, float("inf")):
        assert AdamW(p, max_grad_norm=off).max_grad_norm is None
    assert AdamW(p).max_grad_norm is None
    assert AdamW(p, max_grad_norm=2).max_grad_norm == 2.0
    for bad in (-1.0, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            AdamW(p, max_grad_norm=bad)
    opt = AdamW(p, max_grad_norm=1.0)
    assert "max_grad_norm" not in opt.param_groups[0]                # a property of the step, not of a group
    assert opt.grad_norm() is None and opt.clip_coef() is None and opt.clipped_steps() == 0 and opt.nonfinite_steps() == 0


def test_max_grad_norm_round_trips_through_state_dict(tmp_path):
    from egovlp_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    sd = AdamW(p, lr=1e-3, max_grad_norm=0.75).state_dict()
    assert sd["max_grad_norm"] == 0.75 and set(sd) == {"state", "param_groups", "max_grad_norm"}
    path = tmp_path / "opt.pth"
    torch.save(sd, path)
    fresh = AdamW(p, lr=1e-3)
    fresh.load_state_dict(torch.load(path))
    assert fresh.max_grad_norm == 0.75
    off = AdamW(p, lr=1e-3, max_grad_norm=3.0)
    off.load_state_dict(AdamW(p, lr=1e-3).state_dict())
    assert off.max_grad_norm is None
    keep = AdamW(p, lr=1e-3, max_grad_norm=3.0)
    keep.load_state_dict({k: v for k, v in sd.items() if k != "max_grad_norm"})      # a checkpoint written before the option existed
    assert keep.max_grad_norm == 3.0


def _initialize(config, name, module, *args):
    """The reference's ConfigParser.initialize for a section without an index, as tests/test_boundary_cpu.py restates it."""
    cls = getattr(module, config[name]["type"])
    kwargs = dict(config[name]["args"])
    for p in inspect.signature(cls.__init__).parameters:
        if p not in kwargs and p in config:
            kwargs[p] = config[p]
    return cls(*args, **kwargs)


def test_max_grad_norm_in_the_json_args_reaches_the_optimizer():
    import egovlp_amd.optim as module_optim
    with open(os.path.join(HERE, "golden", "egoclip_config.json")) as f:
        config = json.load(f, object_pairs_hook=collections.OrderedDict)
    config["optimizer"] = json.loads('{"type": "AdamW", "args": {"lr": 3e-5, "max_grad_norm": 1.0}}')
    params = [torch.nn.Parameter(torch.zeros(4))]
    opt = _initialize(config, "optimizer", module_optim, params)
    assert type(opt).__name__ == "AdamW" and opt.max_grad_norm == 1.0 and opt.param_groups[0]["lr"] == 3e-5
    assert opt.param_groups[0]["eps"] == 1e-6 and opt.param_groups[0]["betas"] == (0.9, 0.999)


def test_trainer_logs_the_norm_only_when_clipping_is_on():
    """TrainerBase._train_epoch writes grad_norm / clip_coef next to the loss, at the same cadence, and reads nothing back otherwise."""
    import types
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.common import TrainerBase

    class Writer:
        def __init__(self):
            self.tags = []

        def add_scalar(self, tag, value, step):
            self.tags.append(tag)

    class Loader(list):
        batch_size = 4
        n_samples = 64

    def run(opt):
        t = TrainerBase.__new__(TrainerBase)
        t.model = torch.nn.Linear(2, 2)
        t.device = "cpu"
        t.data_loader = [Loader([{"x": torch.zeros(1)} for _ in range(4)])]
        t.len_epoch, t.max_samples_per_epoch, t.total_batch_sum, t.n_gpu, t.log_step = 4, 1000, 4, 1, 2
        t.tokenizer, t.do_validation, t.writer, t.optimizer = None, False, Writer(), opt
        t.args = types.SimpleNamespace(rank=0, precision_guard_interval=1000, learning_rate1=1e-3, schedule=[])
        t._guard = types.SimpleNamespace(maybe_check=lambda data: None)
        t._step = lambda data: torch.tensor(1.0)
        t._train_epoch(1)
        return t.writer.tags
    p = [torch.nn.Parameter(torch.zeros(3))]
    off = AdamW(p, lr=1e-3)
    off.grad_norm = off.clip_coef = lambda: pytest.fail("a readback with clipping off")
    tags = run(off)
    assert tags.count("Loss_training/loss_0") == 2 and not any(t.startswith("Grad_training") for t in tags)
    on = AdamW(p, lr=1e-3, max_grad_norm=1.0)
    on.grad_norm, on.clip_coef = (lambda: 3.0), (lambda: 1.0 / 3.0)
    tags = run(on)
    assert tags.count("Grad_training/grad_norm_0") == tags.count("Grad_training/clip_coef_0") == tags.count("Loss_training/loss_0") == 2
