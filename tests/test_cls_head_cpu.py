"""CPU checks of the OSCC / PNR fine-tuning feature: the fixture tests/golden/cls_head.npz (recorded from the reference's own
CrossEntropy, loss expressions and metric functions) against the plain-torch restatement tests/cls_head_ref.py that the GPU tests
use; the cases the fixture promises; agreement of header, ctypes prototypes and built library on the three new entry points and
their argument checks; host-side dry runs of classification_step and of both trainers over tests/mock_hip.py (wiring and launch
census, no numerics); the column layout of the gathered block; pnr_metrics on the host; the log lines."""
import collections
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import cls_head_ref as CR
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("egv_cls_head_fwd", "egv_cls_head_loss_bwd", "egv_cls_eval_update")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_head.npz"))


# ------------------------------------------------------------------------------------------------ fixture <-> restatement
@pytest.mark.parametrize("name", list(CR.CASES))
def test_restatement_reproduces_reference_goldens(gold, name):
    inp = CR.make_inputs(name, int(gold[name + "_seed"]))
    r64 = CR.head(name, inp, torch.float64)
    l64 = float(gold[name + "_loss64"])
    assert abs(float(r64["loss"]) - l64) <= 1e-12 * abs(l64)
    for k in ("dW", "db", "dfeats", "scores"):                  # stored rounded to fp32: 2^-24 per element
        assert CR.rel(r64[k], gold[f"{name}_{k}64"]) < 1e-7, k
    assert np.array_equal(r64["pred"].numpy(), gold[name + "_pred"])
    r32 = CR.head(name, inp, torch.float32)
    assert abs(float(r32["loss"]) - float(gold[name + "_loss32"])) <= 1e-6 * max(abs(l64), 1e-30) or l64 == 0.0
    assert np.array_equal(r32["pred"].numpy(), gold[name + "_pred"])


def test_fixture_holds_the_promised_cases(gold):
    C = CR.CASES
    assert any(c[:4] == ("oscc", 32, 768, 2) for c in C.values()) and any(c[:4] == ("pnr", 32, 768, 16) for c in C.values())
    assert any(c[3] == 17 for c in C.values()) and any(c[2] == 1024 for c in C.values())
    assert any(c[1] == 4096 and c[1] // c[4] == 256 for c in C.values())
    assert {(1, 0), (2, 1), (8, 5)} <= {(c[4], c[5]) for c in C.values()}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cls_head.npz")) < (1 << 20)
    for name, (task, n, K, Cc, world, rank, kind) in C.items():
        assert float(gold[name + "_gap"]) >= CR.MIN_GAP
        for k in ("loss", "dW", "db", "dfeats"):
            e = float(gold[f"{name}_err32_{k}"])
            assert (e == 0.0 and kind == "all0") or CR.ERR_FLOOR <= e < 1e-5, (name, k, e)
    # some clips without a state change: zero label rows, target 0, also among the local rows
    inp = CR.make_inputs("pnr_n32_some0", int(gold["pnr_n32_some0_seed"]))
    lo, B = CR.local_rows("pnr_n32_some0")
    zero = inp["state"] == 0
    assert 0 < int(zero.sum()) < 32 and bool(zero[lo:lo + B].any()) and int(inp["labels"][zero].abs().sum()) == 0
    assert bool((CR.targets("pnr_n32_some0", inp)[0][zero] == 0).all())
    # all of them: loss 0, gradients 0
    assert float(gold["pnr_all0_loss64"]) == 0.0 and float(gold["pnr_all0_loss32"]) == 0.0
    assert not gold["pnr_all0_dW64"].any() and not gold["pnr_all0_db64"].any() and not gold["pnr_all0_dfeats64"].any()
    # an exact tie that decides the argmax: columns 1 and 2 equal everywhere, the maximum in some rows, the lower index taken
    s, p = gold["oscc_tie_scores64"], gold["oscc_tie_pred"]
    assert np.array_equal(s[:, 1], s[:, 2])
    top = (s[:, 1] >= s.max(axis=1))
    assert top.any() and (p[top] == 1).all() and not (p == 2).any()


@pytest.mark.parametrize("name", list(CR.METRIC_SETS))
def test_metric_restatement_and_host_metrics_equal_the_reference(gold, name):
    from egovlp_amd.model.metric import oscc_metrics, pnr_metrics
    task, rows, C, fps, kind = CR.METRIC_SETS[name]
    m = CR.make_metric_inputs(name, int(gold[name + "_seed"]))
    want = float(gold[name + "_value"])
    if task == "oscc":
        got = [CR.oscc_accuracy(m["preds"], m["state"]), oscc_metrics(m["preds"], m["state"])["accuracy"]]
    else:
        res = pnr_metrics(m["preds"], m["labels"], m["state"], m["fps"], m["start"], m["end"], m["pnr"])
        assert set(res) == {"keyframe_distance"}
        got = [CR.pnr_distance(m), res["keyframe_distance"]]
    for g in got:
        if kind == "nopos":
            assert math.isnan(g) and math.isnan(want)
        else:
            assert abs(g - want) <= 1e-12 * abs(want)
    assert {"pnr_2997", "pnr_30", "pnr_nopos", "oscc_set"} <= set(CR.METRIC_SETS)
    assert CR.METRIC_SETS["pnr_2997"][3] == 29.97 and CR.METRIC_SETS["pnr_30"][3] == 30.0


def test_metrics_from_counts():
    from egovlp_amd.model.metric import oscc_metrics_from_counts, pnr_metrics_from_counts
    assert oscc_metrics_from_counts([3.0, 4.0, 0.0, 0.0]) == {"accuracy": 75.0}
    assert pnr_metrics_from_counts([0.0, 9.0, 5.0, 4.0]) == {"keyframe_distance": 1.25}
    assert math.isnan(pnr_metrics_from_counts([0.0, 9.0, 0.0, 0.0])["keyframe_distance"])


# ------------------------------------------------------------------------------------------------ ABI
def _ctype_of(p):
    if "*" in p:
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int64_t": ctypes.c_int64}[p.split()[0]]


def test_new_entry_points_agree_across_header_binding_and_library():
    from egovlp_amd import _lib
    raw = open(os.path.join(ROOT, "include", "egovlp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NEW:
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name + " is not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int32 and [_ctype_of(p) for p in params] == list(args), name
        assert params[-1].startswith("void*")                      # the stream comes last
    assert "#define EGV_ABI_VERSION 6" in raw and _lib.ABI_VERSION == 6
    assert "cls_head.hip" in open(os.path.join(ROOT, "egovlp_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libegovlp_hip.so not built (run __graft_entry__.build())")
    h = ctypes.CDLL(_lib.LIB_PATH)
    fn = {}
    for name in NEW:
        fn[name] = getattr(h, name)
        fn[name].restype, fn[name].argtypes = _lib.PROTOTYPES[name]
    p = ctypes.c_void_p(64)

    # argument errors are refused before any launch (no device is touched): null-ish pointers are enough to show it
    def fwd(B=4, K=768, C=2, ld=3, ldf=None):
        return fn["egv_cls_head_fwd"](p, K if ldf is None else ldf, p, p, B, K, C, p, ld, None)

    def lb(n=32, C=2, col_t=2, col_s=-1, row0=0, B=4, K=768, ld=4):
        return fn["egv_cls_head_loss_bwd"](p, ld, n, C, col_t, col_s, row0, B, p, K, p, K, p, p, p, p, K, None, p, None)

    def ev(n=32, C=16, col_t=16, col_s=17, ld=23):
        return fn["egv_cls_eval_update"](p, ld, n, C, col_t, col_s, 18, 20, 21, 22, p, None)
    assert fwd(C=65) == 1 and fwd(K=1028) == 1 and fwd(K=770) == 1 and fwd(B=257) == 1 and fwd(C=2, ld=1) == 1 and fwd(ldf=766) == 1
    assert lb(C=65, col_t=65, ld=70) == 1 and lb(K=1028) == 1 and lb(K=770) == 1 and lb(n=4097) == 1 and lb(n=32, row0=30, B=4) == 1
    assert lb(col_t=1) == 1 and lb(col_t=0) == 1 and lb(col_t=4) == 1 and lb(col_s=1) == 1 and lb(col_s=2) == 1 and lb(B=257, n=512) == 1
    assert ev(n=4097) == 1 and ev(C=65) == 1 and ev(col_s=3) == 1 and ev(ld=22) == 1 and ev(n=0) == 1
    assert fn["egv_cls_eval_update"](p, 3, 8, 2, 1, -1, -1, -1, -1, -1, p, None) == 1       # col_target inside [0, C)


def test_limits_helper_and_layout():
    from egovlp_amd.loss_ops import ClsLayout, cls_head_ok
    assert cls_head_ok(32, 4, 768, 2) and cls_head_ok(4096, 256, 1024, 64)
    assert not cls_head_ok(4097, 4, 768, 2) and not cls_head_ok(512, 257, 768, 2) and not cls_head_ok(32, 4, 770, 2)
    assert not cls_head_ok(32, 4, 1028, 2) and not cls_head_ok(32, 4, 768, 65) and not cls_head_ok(2, 4, 768, 2)
    o, p, e = ClsLayout(2), ClsLayout(16, "pnr"), ClsLayout(16, "pnr", evaluate=True)
    assert (o.target, o.state, o.ld) == (2, -1, 3) and (p.target, p.state, p.ld) == (16, 17, 18)
    assert (e.target, e.state, e.fps, e.start, e.end, e.pnr, e.ld) == (16, 17, 18, 20, 21, 22, 23)
    blk = e.fill(torch.zeros(2, e.ld), torch.tensor([3, 0]), torch.tensor([1, 0]), torch.tensor([29.97, 30.0], dtype=torch.float64),
                 torch.tensor([100, 7]), torch.tensor([340, 250]), torch.tensor([200, 90]))
    assert blk[:, 16:18].tolist() == [[3.0, 1.0], [0.0, 0.0]] and blk[:, 20:].tolist() == [[100.0, 340.0, 200.0], [7.0, 250.0, 90.0]]
    fps = blk[:, 18].double() + blk[:, 19].double()
    assert abs(float(fps[0]) - 29.97) < 29.97 * 2.0 ** -47 and float(fps[1]) == 30.0 and float(blk[0, 19]) != 0.0


# ------------------------------------------------------------------------------------------------ host dry runs
def _model(classes):
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                      "pretrained": True, "time_init": "rand"},
                        text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                        projection="minimal", projection_dim=classes, load_checkpoint="")


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    return {"oscc": _model(2).train(), "pnr": _model(16).train()}


def _batch(task, B=2, seed=3, val=False):
    g = torch.Generator().manual_seed(seed)
    d = {"video": torch.randn(B, 2, 3, 224, 224, generator=g), "state": torch.randint(0, 2, (B,), generator=g)}
    if task == "pnr":
        lab = torch.zeros(B, 16, dtype=torch.long)
        lab[torch.arange(B), torch.randint(0, 16, (B,), generator=g)] = 1
        lab[d["state"] == 0] = 0
        d["labels"] = lab
        if val:
            d.update(fps=torch.full((B,), 29.97, dtype=torch.float64), parent_start_frame=torch.arange(B) * 10,
                     parent_end_frame=torch.arange(B) * 10 + 240, parent_pnr_frame=torch.arange(B) * 10 + 100)
    return d


@pytest.mark.parametrize("task", ["oscc", "pnr"])
def test_classification_step_wiring(models, task):
    """Fused path: one egv_cls_head_fwd, one egv_cls_head_loss_bwd, no egv_cross_entropy_fwd_bwd; the fallback the reverse; every
    video parameter and no text parameter receives a gradient either way."""
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_oscc import classification_step
    model = models[task]
    opt = AdamW(model.parameters(), lr=3e-5)
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            for fused in (True, False):
                calls.clear()
                loss = classification_step(model, CrossEntropy(), opt, _batch(task), 1, 0, task=task, fused_head=fused)
                c = collections.Counter(calls)
                assert loss.shape == () and c["egv_adamw_multi"] >= 1
                want = (1, 1, 0) if fused else (0, 0, 1)
                assert (c["egv_cls_head_fwd"], c["egv_cls_head_loss_bwd"], c["egv_cross_entropy_fwd_bwd"]) == want, c
                assert c["egv_cls_eval_update"] == 0
                for k, p in model.named_parameters():
                    text = k.startswith("text_model.") or k.startswith("txt_proj.")
                    assert (p.grad is None) == text, k
        finally:
            model.exec_ctx.unset("fwd_passes", "bwd_passes")


def test_gathered_block_has_the_documented_layout(monkeypatch):
    """_ClsHeadFn with the collective replaced by a two-rank stand-in: [0, C) scores, C the class index, C + 1 the state; the loss
    kernel is handed the gathered block and this rank's row offset."""
    from egovlp_amd import loss_ops
    from egovlp_amd.model.loss import _ClsHeadFn
    from egovlp_amd import gather as T
    monkeypatch.setattr(T, "_gather_rows", lambda t, world: torch.cat([t + 100.0, t]))
    seen = {}
    real = loss_ops.cls_head_loss_bwd

    def spy(packed, C, col_target, col_state=-1, row0=0, B=None, **kw):
        seen.update(shape=tuple(packed.shape), cols=(C, col_target, col_state), row0=row0, B=B)
        return real(packed, C, col_target, col_state, row0=row0, B=B, **kw)
    monkeypatch.setattr(loss_ops, "cls_head_loss_bwd", spy)
    feats = torch.randn(3, 8, requires_grad=True)
    W, b = torch.randn(16, 8, requires_grad=True), torch.randn(16, requires_grad=True)
    with mock_hip() as calls:
        loss, block = _ClsHeadFn.apply(feats, W, b, torch.tensor([5, 0, 15]), torch.tensor([1, 0, 1]), 2, 1, None)
        loss.backward()
    assert list(calls) == ["egv_cls_head_fwd", "egv_cls_head_loss_bwd"]
    assert block.shape == (6, 18) and seen == {"shape": (6, 18), "cols": (16, 16, 17), "row0": 3, "B": 3}
    assert block[3:, 16].tolist() == [5.0, 0.0, 15.0] and block[3:, 17].tolist() == [1.0, 0.0, 1.0]
    assert block[:3, 16].tolist() == [105.0, 100.0, 115.0]
    assert feats.grad.shape == feats.shape and W.grad.shape == W.shape and b.grad.shape == b.shape
    with mock_hip():
        _, block = _ClsHeadFn.apply(feats, W, None, torch.tensor([1, 0, 1]), None, 2, 0, None)
    assert block.shape == (6, 17) and block[3:, 16].tolist() == [1.0, 0.0, 1.0]


class _Loader:
    dataset_name = "synthetic"

    def __init__(self, task, B, n_batches, val=False, last=None):
        self.task, self.batch_size, self.n_batches, self.val, self.last = task, B, n_batches, val, last
        self.n_samples = B * n_batches

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            B = self.last if (self.last and i == self.n_batches - 1) else self.batch_size
            yield _batch(self.task, B, seed=20 + i, val=self.val)


class _Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(msg)
    warning = debug = info


class _Tok:
    def __call__(self, *a, **k):
        raise AssertionError("the classification trainers make no tokenizer call")


def _bare_trainer(cls, model, metrics, task):
    """The trainer without Multi_BaseTrainer_dist.__init__ (which needs a HIP device): the attributes its loops read."""
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import AllGather_multi
    tr = cls.__new__(cls)
    tr.args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=2e-4, schedule=[1, 80])
    tr.model, tr.loss, tr.metrics, tr.device = model, CrossEntropy(), metrics, torch.device("cpu")
    tr.optimizer = AdamW(model.parameters(), lr=3e-5)
    tr.data_loader, tr.valid_data_loader = [_Loader(task, 2, 2)], [_Loader(task, 2, 3, val=True, last=1)]
    tr.do_validation = True
    tr.len_epoch, tr.total_batch_sum, tr.max_samples_per_epoch = 2, 2, 50000
    tr.batch_size, tr.log_step, tr.n_gpu = 2, 1, 1
    tr.tokenizer, tr.writer, tr.grad_sync, tr.logger = _Tok(), None, None, _Logger()
    tr.allgather, tr.fused_head = AllGather_multi.apply, True
    return tr


@pytest.mark.parametrize("task", ["oscc", "pnr"])
def test_trainers_epoch_loop_dry_run(models, task):
    from egovlp_amd.model import metric as M
    from egovlp_amd.trainer.trainer_epic import RetrievalTrainerBase
    from egovlp_amd.trainer.trainer_oscc import Multi_Trainer_dist_OSCC
    from egovlp_amd.trainer.trainer_pnr import Multi_Trainer_dist_PNR
    cls, metric = (Multi_Trainer_dist_OSCC, M.oscc_metrics) if task == "oscc" else (Multi_Trainer_dist_PNR, M.pnr_metrics)
    assert issubclass(cls, RetrievalTrainerBase)
    model = models[task]
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            tr = _bare_trainer(cls, model, [metric], task)
            log = tr._train_epoch(1)
        finally:
            model.exec_ctx.unset("fwd_passes", "bwd_passes")
    c = collections.Counter(calls)
    # two fused training steps; three validation batches: one forward, one loss call and one accumulator update each
    assert c["egv_cls_head_fwd"] == 2 + 3 and c["egv_cls_head_loss_bwd"] == 2 + 3 and c["egv_cls_eval_update"] == 3, c
    assert c["egv_cross_entropy_fwd_bwd"] == 0
    assert set(log) == {"loss_0", "val_loss_0", "nested_val_metrics"}
    assert isinstance(log["val_loss_0"], float)
    key = "accuracy" if task == "oscc" else "keyframe_distance"
    assert set(log["nested_val_metrics"][0][metric.__name__]) == {key}
    assert tr.optimizer.param_groups[0]["lr"] == pytest.approx(2e-5)          # schedule [1, 80] at epoch 1
    assert len(tr.logger.lines) == 1 and tr.logger.lines[0].startswith("synthetic epoch 1, " + ("Acc: " if task == "oscc" else "keyframe_distance: "))


def test_log_helpers():
    from egovlp_amd.trainer import trainer_oscc, trainer_pnr
    assert trainer_oscc.verbose(3, {"accuracy": 71.26}, "Ego4D_OSCC") == "Ego4D_OSCC epoch 3, Acc: 71.3"
    assert trainer_pnr.verbose(2, {"keyframe_distance": 0.6512}, "Ego4D_PNR") == "Ego4D_PNR epoch 2, keyframe_distance: 0.7"
    assert trainer_pnr.format_nested_metrics_for_writer({"keyframe_distance": 1.0}, "pnr_metrics", "D") == {"[pnr_metrics]D_keyframe_distance": 1.0}
    assert trainer_oscc.format_nested_metrics_for_writer({"accuracy": 1.0}, "oscc_metrics", "D") == {"[oscc_metrics]D_accuracy": 1.0}
