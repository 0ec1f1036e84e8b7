"""CPU checks of the retrieval fine-tuning feature: the fixture tests/golden/finetune_head.npz (recorded from the reference's own
sim_matrix + ranking losses + autograd) against the plain-torch restatement tests/finetune_ref.py that the GPU tests use as
their fp64 yardstick; the conditions the fixture promises (tau, ambiguous hinge terms, active share); host-side dry runs of
retrieval_step and of both trainers' loops over tests/mock_hip.py (wiring and launch census, no numerics); and the agreement
of header, ctypes prototypes and built library on the new entry points."""
import collections
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import finetune_ref as FR
from mock_hip import mock_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "finetune_head.npz"))


def _inputs(gold, name):
    return FR.make_inputs(name, int(gold[name + "_seed"]))


# ------------------------------------------------------------------------------------------------ fixture <-> restatement
@pytest.mark.parametrize("name", list(FR.CASES))
def test_restatement_reproduces_reference_goldens(gold, name):
    n, D, adaptive, fix_norm, _ = FR.CASES[name]
    text, video, weight = _inputs(gold, name)
    margin = FR.margin_of(adaptive)
    w64 = None if weight is None else weight.double()
    l64, x64, dt64, dv64 = FR.head(text.double(), video.double(), w64, margin, fix_norm)
    assert abs(float(l64) - float(gold[name + "_loss64"])) <= 1e-12 * abs(float(gold[name + "_loss64"]))
    if n <= FR.FULL_MAX_N:
        assert np.array_equal(text.numpy(), gold[name + "_text"]) and np.array_equal(video.numpy(), gold[name + "_video"])
        if adaptive:
            assert np.array_equal(weight.numpy(), gold[name + "_weight"])
        # stored rounded to fp32: 2^-24 per element
        assert FR.rel_fro(dt64, torch.from_numpy(gold[name + "_dt64"])) < 1e-7
        assert FR.rel_fro(dv64, torch.from_numpy(gold[name + "_dv64"])) < 1e-7
        assert float((x64 - torch.from_numpy(gold[name + "_sim64"]).double()).abs().max()) < 1e-7
    else:
        P = FR.projection(D)
        assert FR.rel_fro(dt64 @ P, torch.from_numpy(gold[name + "_dt64_proj"])) < 1e-10
        assert FR.rel_fro(dv64 @ P, torch.from_numpy(gold[name + "_dv64_proj"])) < 1e-10
        assert FR.rel_fro(dt64.norm(dim=1), torch.from_numpy(gold[name + "_dt64_rows"])) < 1e-10
        assert FR.rel_fro(dv64.norm(dim=1), torch.from_numpy(gold[name + "_dv64_rows"])) < 1e-10
        assert abs(float(dt64.norm()) - float(gold[name + "_dt64_norm"])) < 1e-10 * float(dt64.norm())
    # the fp32 restatement against the reference's fp32 loss (different summation orders: a few ulp of fp32)
    l32, _, dt32, dv32 = FR.head(text, video, weight, margin, fix_norm)
    assert abs(float(l32) - float(gold[name + "_loss32"])) <= 1e-5 * abs(float(gold[name + "_loss32"]))
    # ... and an fp32 implementation against the fp64 gradients under the GPU test's own rule (bar + ambiguous allowance)
    a_t, a_v, n_amb, n_kept = FR.ambiguous_allowance(text.double(), video.double(), w64, margin, fix_norm, float(gold[name + "_tau"]))
    assert (dt32.double() - dt64).norm() <= 1e-4 * dt64.norm() + a_t
    assert (dv32.double() - dv64).norm() <= 1e-4 * dv64.norm() + a_v


@pytest.mark.parametrize("name", list(FR.CASES))
def test_fixture_conditions(gold, name):
    """tau = 10 e; no ambiguous hinge term and an active share in [0.15, 0.6] for n <= 200; fewer than 1e-4 ambiguous at n = 1024."""
    n, D, adaptive, fix_norm, _ = FR.CASES[name]
    text, video, weight = _inputs(gold, name)
    e, tau = float(gold[name + "_e"]), float(gold[name + "_tau"])
    assert 0 < e < 1e-5 and tau == 10.0 * e
    x64 = FR.sim_matrix(text.double(), video.double())
    ar, ac, active = FR.ambiguous(x64, None if weight is None else weight.double(), FR.margin_of(adaptive), fix_norm, tau)
    n_amb, n_kept = int(ar.sum() + ac.sum()), int(2 * FR.kept(n, fix_norm).sum())
    assert n_amb == int(gold[name + "_n_amb"]) and n_kept == int(gold[name + "_n_kept"])
    assert abs(active - float(gold[name + "_active"])) < 1e-12
    assert 0.15 <= active <= 0.6
    if n <= 200:
        assert n_amb == 0
    else:
        assert n_amb <= 1e-4 * n_kept
    assert float(gold[name + "_err32_dt"]) < 1e-5 and float(gold[name + "_err32_dv"]) < 1e-5      # the reference's own fp32 error


def test_case_table_covers_what_the_feature_promises():
    ns = {c[0] for c in FR.CASES.values()}
    assert {4, 32, 48, 200, 1024} <= ns
    assert any(c[0] == 1024 and c[1] == 256 for c in FR.CASES.values())
    assert any(c[1] == 64 for c in FR.CASES.values()) and any(c[4] for c in FR.CASES.values())
    for adaptive in (False, True):
        for fix_norm in (False, True):
            assert any(c[2] == adaptive and c[3] == fix_norm for c in FR.CASES.values())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "finetune_head.npz")) < (1 << 20)


# ------------------------------------------------------------------------------------------------ ABI
def test_new_entry_points_agree_across_header_binding_and_library():
    from egovlp_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egovlp_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+egv_maxmargin_head_fwd_bwd\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, "egv_maxmargin_head_fwd_bwd is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.PROTOTYPES["egv_maxmargin_head_fwd_bwd"]
    assert res is ctypes.c_int32 and len(args) == len(params) == 14

    def ctype_of(p):
        if "*" in p:
            return ctypes.c_void_p
        return {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "int64_t": ctypes.c_int64}[p.split()[0]]
    assert [ctype_of(p) for p in params] == list(args)
    assert re.search(r"int64_t\s+egv_maxmargin_head_work_floats\s*\(\s*int32_t\s+n\s*,\s*int32_t\s+D\s*\)\s*;", txt)
    assert _lib.PROTOTYPES["egv_maxmargin_head_work_floats"] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32])
    assert "#define EGV_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "egovlp_hip.h")).read() and _lib.ABI_VERSION == 6
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libegovlp_hip.so not built (run __graft_entry__.build())")
    h = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(h, "egv_maxmargin_head_fwd_bwd") and hasattr(h, "egv_maxmargin_head_work_floats")
    wf = h.egv_maxmargin_head_work_floats
    wf.restype, wf.argtypes = ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]
    assert wf(1024, 256) == 2 * 1024 * 256 + 4 * 1024          # host function: no device needed; nothing n x n
    assert wf(1024, 256) < 1024 * 1024
    # argument errors are refused before any launch (no device is touched): null pointers are enough to show it
    f = h.egv_maxmargin_head_fwd_bwd
    f.restype, f.argtypes = _lib.PROTOTYPES["egv_maxmargin_head_fwd_bwd"]
    one = ctypes.c_void_p(16)
    for n, D in ((1025, 256), (8, 260), (8, 254), (0, 256), (1, 256)):
        assert f(one, one, None, n, D, 0.2, 1, 1e-8, one, None, one, one, one, None) == 1, (n, D)


# ------------------------------------------------------------------------------------------------ host dry runs
def _model():
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                      "pretrained": True, "time_init": "rand"},
                        text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                        projection="minimal", load_checkpoint="")


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return _model().train()


def _batch(B=2, seed=3, relation=False):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=seed)
    d = {"video": b["video"], "text": b["text"]}
    if relation:
        d["relation"] = torch.linspace(0.3, 1.0, B)
    return d


OLD_PATH = ("egv_sim_matrix_fwd", "egv_maxmargin_fwd_bwd", "egv_sim_matrix_bwd")


@pytest.mark.parametrize("adaptive", [False, True])
def test_retrieval_step_wiring(model, adaptive):
    """One egv_maxmargin_head_fwd_bwd per step on the fused path and none of the three old calls; the three old calls, once
    each, on the fallback path; every parameter receives a gradient either way."""
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss, MaxMarginRankingLoss
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_epic import retrieval_step
    loss_fn = AdaptiveMaxMarginRankingLoss() if adaptive else MaxMarginRankingLoss()
    opt = AdamW(model.parameters(), lr=3e-5)
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            loss = retrieval_step(model, loss_fn, opt, _batch(relation=adaptive), 1, 0)
            c = collections.Counter(calls)
            assert loss.shape == () and c["egv_maxmargin_head_fwd_bwd"] == 1 and c["egv_adamw_multi"] >= 1
            assert all(c[k] == 0 for k in OLD_PATH) and c["egv_egonce_fwd_bwd"] == 0
            calls.clear()
            seen = []
            hook = model.vid_proj[0].weight.register_hook(lambda g: seen.append(tuple(g.shape)))
            retrieval_step(model, loss_fn, opt, _batch(relation=adaptive), 1, 0, fused_head=False)
            hook.remove()
            c = collections.Counter(calls)
            assert c["egv_maxmargin_head_fwd_bwd"] == 0 and all(c[k] == 1 for k in OLD_PATH), c
            assert seen == [tuple(model.vid_proj[0].weight.shape)]
        finally:
            model.exec_ctx.unset("fwd_passes", "bwd_passes")


def test_adaptive_loss_needs_its_weight(model):
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_epic import retrieval_step
    with mock_hip():
        with pytest.raises(KeyError):
            retrieval_step(model, AdaptiveMaxMarginRankingLoss(), AdamW(model.parameters(), lr=1e-5), _batch(), 1, 0)
        with pytest.raises(TypeError):
            AdaptiveMaxMarginRankingLoss().fused(torch.zeros(4, 8), torch.zeros(4, 8))


def test_gather_rows_packs_and_unpacks(monkeypatch):
    """AllGatherRows with the collective replaced by a two-rank stand-in: columns are split back into the inputs' shapes, the
    backward hands each input its local rows."""
    from egovlp_amd import gather as T
    monkeypatch.setattr(T, "_gather_rows", lambda t, world: torch.cat([t, t + 100.0]))
    v = torch.arange(12.0).reshape(3, 4).requires_grad_(True)
    t = torch.arange(6.0).reshape(3, 2).requires_grad_(True)
    w = torch.tensor([[1.0], [2.0], [3.0]])
    V, Tt, W = T.AllGatherRows.apply(2, 1, v, t, w)
    assert V.shape == (6, 4) and Tt.shape == (6, 2) and W.shape == (6, 1)
    assert torch.equal(V[:3], v.detach()) and torch.equal(Tt[3:], t.detach() + 100.0) and torch.equal(W[3:, 0], w[:, 0] + 100.0)
    (V * torch.arange(6.0)[:, None]).sum().backward(retain_graph=True)
    assert torch.equal(v.grad, torch.arange(3.0, 6.0)[:, None].expand(3, 4))      # rank 1: rows 3..5 of the global gradient
    assert t.grad is None or float(t.grad.abs().sum()) == 0.0


class _Tok:
    def __call__(self, texts, return_tensors='pt', padding=True, truncation=True):
        L = 8
        ids = torch.full((len(texts), L), 1500, dtype=torch.long)
        ids[:, 0] = 101
        return {"input_ids": ids, "attention_mask": torch.ones(len(texts), L, dtype=torch.long)}


class _Loader:
    dataset_name = "synthetic"

    def __init__(self, B, n_batches, val=None, classes=0):
        self.batch_size, self.n_batches, self.val, self.classes = B, n_batches, val, classes
        self.n_samples = B * n_batches

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            d = _batch(self.batch_size, seed=20 + i, relation=True)
            d["text"] = ["a caption"] * self.batch_size
            d["meta"] = {"paths": torch.arange(i * self.batch_size, (i + 1) * self.batch_size)}
            d["target"] = torch.ones(self.batch_size, max(self.classes, 1))
            yield d


class _Logger:
    def info(self, *a, **k):
        pass
    warning = debug = info


def _bare_trainer(cls, model, loss_fn, metrics, valid=None, **extra):
    """The trainer without Multi_BaseTrainer_dist.__init__ (which needs a HIP device): the attributes its loops read."""
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import AllGather_multi
    tr = cls.__new__(cls)
    tr.args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=2e-4, schedule=[1, 80])
    tr.model, tr.loss, tr.metrics, tr.device = model, loss_fn, metrics, torch.device("cpu")
    tr.optimizer = AdamW(model.parameters(), lr=3e-5)
    tr.data_loader, tr.valid_data_loader = [_Loader(2, 2)], valid
    tr.do_validation = valid is not None
    tr.len_epoch, tr.total_batch_sum, tr.max_samples_per_epoch = 2, 2, 50000
    tr.batch_size, tr.log_step, tr.n_gpu = 2, 1, 1
    tr.tokenizer, tr.writer, tr.grad_sync, tr.logger = _Tok(), None, None, _Logger()
    tr.allgather, tr.fused_head = AllGather_multi.apply, True
    for k, v in extra.items():
        setattr(tr, k, v)
    return tr


def test_trainers_epoch_loop_dry_run(model):
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss, MaxMarginRankingLoss
    from egovlp_amd.trainer.trainer_charades import Multi_Trainer_dist_Charades
    from egovlp_amd.trainer.trainer_epic import Multi_Trainer_dist_MIR
    seen = {}

    def mir_metrics(sims, idx, **kw):
        seen["mir"] = (tuple(sims.shape), idx.tolist(), kw.get("annotations"))
        return {k: 0.5 for k in ("nDCG_V2T", "nDCG_T2V", "nDCG_AVG", "mAP_V2T", "mAP_T2V", "mAP_AVG")}

    def charades_metrics(sims, targets):
        seen["charades"] = (tuple(sims.shape), tuple(targets.shape))
        return {"mAP": 0.25}

    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        try:
            tr = _bare_trainer(Multi_Trainer_dist_MIR, model, MaxMarginRankingLoss(), [mir_metrics], valid=[_Loader(2, 3)],
                               annotations="ANN")
            log = tr._train_epoch(1)
            c = collections.Counter(calls)
            assert c["egv_maxmargin_head_fwd_bwd"] == 2 and all(c[k] == 0 for k in OLD_PATH[1:])      # two steps, fused
            assert c["egv_sim_matrix_fwd"] == 1                                                      # the validation similarity
            assert set(log) == {"loss_0", "val_loss_0", "nested_val_metrics"} and log["val_loss_0"] == 0.0
            assert seen["mir"] == ((6, 6), [0, 1, 2, 3, 4, 5], "ANN")
            assert set(log["nested_val_metrics"][0]["mir_metrics"]) == {"nDCG_V2T", "nDCG_T2V", "nDCG_AVG", "mAP_V2T", "mAP_T2V", "mAP_AVG"}
            assert tr.optimizer.param_groups[0]["lr"] == pytest.approx(2e-5)          # schedule [1, 80] at epoch 1
            calls.clear()
            tc = _bare_trainer(Multi_Trainer_dist_Charades, model, AdaptiveMaxMarginRankingLoss(), [charades_metrics],
                               valid=[_Loader(2, 2, classes=5)], class_sentences=["holding a box"] * 5)
            tc.fused_head = False
            log = tc._train_epoch(1)
            c = collections.Counter(calls)
            assert c["egv_maxmargin_head_fwd_bwd"] == 0 and c["egv_maxmargin_fwd_bwd"] == 2 and c["egv_sim_matrix_bwd"] == 2
            assert c["egv_sim_matrix_fwd"] == 3                                       # two steps + the validation similarity
            assert seen["charades"] == ((4, 5), (4, 5))
            assert log["nested_val_metrics"][0]["charades_metrics"] == {"mAP": 0.25}
        finally:
            model.exec_ctx.unset("fwd_passes", "bwd_passes")


def test_log_helpers():
    from egovlp_amd.trainer import trainer_charades, trainer_epic
    m = {"nDCG_V2T": 0.5, "nDCG_T2V": 0.25, "nDCG_AVG": 0.375, "mAP_V2T": 0.1, "mAP_T2V": 0.2, "mAP_AVG": 0.15}
    assert trainer_epic.verbose(3, m, "mir_metrics", "EpicKitchens_MIR") == \
        "[mir_metrics]EpicKitchens_MIR epoch 3, nDCG_V2T: 0.500, nDCG_T2V: 0.250, nDCG_AVG: 0.375,, mAP_V2T: 0.100, mAP_T2V: 0.200, mAP_AVG: 0.150"
    assert trainer_charades.verbose(1, {"mAP": 0.5}, "charades_metrics", "CharadesEgo") == "[charades_metrics]CharadesEgo epoch 1, mAP: 0.500"
    assert trainer_epic.format_nested_metrics_for_writer({"mAP": 1.0}, "m", "D") == {"[m]D_mAP": 1.0}


def test_class_sentences_file(tmp_path):
    from egovlp_amd.trainer.trainer_charades import read_class_sentences
    p = tmp_path / "classes.txt"
    p.write_text("c000 Holding some clothes\nc001 Putting clothes somewhere\n")
    assert read_class_sentences(str(p)) == ["Holding some clothes", "Putting clothes somewhere"]
