"""GPU checks of the OSCC / PNR fine-tuning feature.  Numbers first: the three kernels of csrc/cls_head.hip against the fp64
goldens of tests/golden/cls_head.npz, which tests/golden/make_golden_cls_head.py recorded from the REFERENCE's own CrossEntropy,
loss expressions and metric functions; then one classification_step of the whole model at the configs' geometry (B = 4, T = 16)
against the CPU oracle, on the fused and on the fallback route; then an epoch of each trainer with its on-device validation.

Measured on MI355X (relative errors against fp64; bar = 10 x the reference's own fp32 error of that case, 5e-7 .. 3.3e-6):
loss <= 4.5e-8, dW <= 2.9e-8, db <= 9.6e-8, dfeats <= 3.1e-8 over the eight cases, exact zeros in the all-state-0 case
(the table is in DESIGN 4.5d)."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import cls_head_ref as CR  # noqa: E402
from egovlp_amd.synth import synth_state_dict  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_head.npz"))


def _run_kernels(name, inp, want_pred=True):
    """forward kernel -> block (as the step packs it) -> loss + backward kernel, for this case's rank."""
    from egovlp_amd import loss_ops
    task = CR.CASES[name][0]
    lo, B = CR.local_rows(name)
    feats, W, b = inp["feats"].cuda(), inp["W"].cuda(), inp["b"].cuda()
    target, state = CR.targets(name, inp)
    lay = loss_ops.ClsLayout(W.shape[0], task)
    n = feats.shape[0]
    block = torch.empty((n, lay.ld), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 256):                        # every rank's rows (the forward kernel takes up to 256)
        loss_ops.cls_head_fwd(feats[r0:r0 + 256], W, b, out=block[r0:r0 + 256])
    lay.fill(block, target.cuda(), None if state is None else state.cuda())
    loss, dW, db, dx, pred = loss_ops.cls_head_loss_bwd(block, W.shape[0], lay.target, lay.state, row0=lo, B=B,
                                                        feats=feats[lo:lo + B], weight=W, want_pred=want_pred)
    return {"loss": loss, "dW": dW, "db": db, "dfeats": dx, "pred": pred, "scores": block[:, :W.shape[0]].clone()}, block, lay


# ------------------------------------------------------------------------------------------------ 1. kernels vs the fixture
@pytest.mark.parametrize("name", list(CR.CASES))
def test_kernels_match_fp64_goldens(gold, name):
    inp = CR.make_inputs(name, int(gold[name + "_seed"]))
    got, _, _ = _run_kernels(name, inp)
    torch.cuda.synchronize()
    l64 = float(gold[name + "_loss64"])
    errs = {"loss": 0.0 if (l64 == 0.0 and float(got["loss"]) == 0.0) else abs(float(got["loss"]) - l64) / abs(l64) if l64 else float("inf")}
    for k in ("dW", "db", "dfeats"):
        errs[k] = CR.rel(got[k], gold[f"{name}_{k}64"])
    bars = {k: 10.0 * float(gold[f"{name}_err32_{k}"]) for k in errs}
    print("cls_head %-14s " % name + "  ".join("%s %.2e (bar %.2e)" % (k, errs[k], bars[k]) for k in errs)
          + "  scores %.2e" % CR.rel(got["scores"], gold[name + "_scores64"]))
    assert np.array_equal(got["pred"].cpu().numpy(), gold[name + "_pred"])
    for k in errs:
        assert errs[k] <= bars[k], (name, k, errs[k], bars[k])
    assert CR.rel(got["scores"], gold[name + "_scores64"]) < 1e-6


@pytest.mark.parametrize("name", ["pnr_n32_some0", "oscc_n4096", "oscc_tie"])
def test_kernels_are_bit_reproducible(gold, name):
    inp = CR.make_inputs(name, int(gold[name + "_seed"]))
    a, _, _ = _run_kernels(name, inp)
    b, _, _ = _run_kernels(name, inp)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_out_of_range_target_gives_nan_everywhere(gold):
    from egovlp_amd import loss_ops
    name = "oscc_w2"
    inp = CR.make_inputs(name, int(gold[name + "_seed"]))
    _, block, lay = _run_kernels(name, inp)
    lo, B = CR.local_rows(name)
    feats, W = inp["feats"].cuda(), inp["W"].cuda()
    for bad in (2.0, -1.0, 0.5):
        blk = block.clone()
        blk[0, lay.target] = bad                        # a row of ANOTHER rank: the global loss is void all the same
        loss, dW, db, dx, pred = loss_ops.cls_head_loss_bwd(blk, 2, lay.target, lay.state, row0=lo, B=B, feats=feats[lo:lo + B],
                                                            weight=W, want_pred=True)
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dW).all()) and bool(torch.isnan(db).all()) and bool(torch.isnan(dx).all())
        assert np.array_equal(pred.cpu().numpy(), gold[name + "_pred"])
    with pytest.raises(Exception):
        loss_ops.cls_head_fwd(torch.zeros(4, 770, device="cuda"), torch.zeros(2, 770, device="cuda"), None)
    torch.cuda.synchronize()


def test_autograd_node_scales_the_stored_gradients(gold):
    """CrossEntropy.fused on leaves: loss and the three gradients of the fixture, times a non-unit upstream gradient."""
    from egovlp_amd.model.loss import CrossEntropy
    name = "oscc_n32"
    inp = CR.make_inputs(name, int(gold[name + "_seed"]))
    feats = inp["feats"].cuda().requires_grad_(True)
    W, b = inp["W"].cuda().requires_grad_(True), inp["b"].cuda().requires_grad_(True)
    loss = CrossEntropy().fused(feats, W, b, inp["state"].cuda())
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - float(gold[name + "_loss64"])) < 1e-6 * float(gold[name + "_loss64"])
    assert CR.rel(W.grad, 2.0 * gold[name + "_dW64"]) < 1e-6 and CR.rel(b.grad, 2.0 * gold[name + "_db64"]) < 1e-6
    assert CR.rel(feats.grad, 2.0 * gold[name + "_dfeats64"]) < 1e-6


# ------------------------------------------------------------------------------------------------ 2. the validation accumulator
def _metric_block(name, m):
    from egovlp_amd.loss_ops import ClsLayout
    task, rows, C, fps, kind = CR.METRIC_SETS[name]
    lay = ClsLayout(C, task, evaluate=True)
    block = torch.empty((rows, lay.ld), dtype=torch.float32, device="cuda")
    block[:, :C] = m["preds"].cuda()
    if task == "oscc":
        lay.fill(block, m["state"].cuda())
    else:
        lay.fill(block, torch.argmax(m["labels"], 1).cuda(), m["state"].cuda(), m["fps"].cuda(), m["start"].cuda(), m["end"].cuda(),
                 m["pnr"].cuda())
    return block, lay


@pytest.mark.parametrize("name", list(CR.METRIC_SETS))
def test_eval_update_equals_the_reference_metrics(gold, name):
    from egovlp_amd.trainer.classification_eval import ClassificationEvaluator
    task, rows, C, fps, kind = CR.METRIC_SETS[name]
    m = CR.make_metric_inputs(name, int(gold[name + "_seed"]))
    block, lay = _metric_block(name, m)
    metric = "oscc_metrics" if task == "oscc" else "pnr_metrics"
    key = "accuracy" if task == "oscc" else "keyframe_distance"
    ev = ClassificationEvaluator([metric])
    ev.update(block[:5], lay)                           # something to forget
    ev.reset()
    want = float(gold[name + "_value"])
    for rnd in range(2):                                # the accumulators are reused after compute()'s reset
        cuts = [0, 7, 8, 8 + 64, rows] if rows > 80 else [0, 3, rows]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            ev.update(block[lo:hi], lay)
        assert float(ev.accum[0][1]) == rows
        res, _ = ev.compute()
        got = res[0][metric][key]
        print("cls_eval %-10s round %d: %r (reference %r)" % (name, rnd, got, want))
        if kind == "nopos":
            assert math.isnan(got) and math.isnan(want)
        else:
            assert abs(got - want) <= 1e-12 * abs(want)
        assert float(ev.accum[0].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. the whole model, B = 4, T = 16
WATCH = ["vid_proj.0.weight", "vid_proj.0.bias", "video_model.blocks.11.mlp.fc2.weight", "video_model.blocks.0.attn.qkv.weight",
         "video_model.blocks.0.timeattn.qkv.weight", "video_model.patch_embed.proj.weight"]
F16_GRAD = 1e-2           # tests/test_gpu_model.py:38


def _model(classes, frames):
    from egovlp_amd.model.model import FrozenInTime
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": frames,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", projection_dim=classes, load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=21)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train(), sd


def _task_batch(task, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"video": torch.randn(B, T, 3, 224, 224, generator=g), "state": torch.randint(0, 2, (B,), generator=g)}
    if task == "pnr":
        d["state"][0], d["state"][1] = 1, 0
        lab = torch.zeros(B, 16, dtype=torch.long)
        lab[torch.arange(B), torch.randint(0, 16, (B,), generator=g)] = 1
        lab[d["state"] == 0] = 0
        d["labels"] = lab
    return d


@pytest.mark.parametrize("task", ["oscc", "pnr"])
def test_classification_step_matches_cpu_oracle_at_config_geometry(task):
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_oscc import classification_step
    classes, B, T = (2, 4, 16) if task == "oscc" else (16, 4, 16)
    Precision.set("bf16x3")
    m, sd = _model(classes, T)
    data = _task_batch(task, B, T, seed=8)
    # the CPU oracle's video encoder + F.linear + the reference's loss expression on the whole batch
    sdo = {k: v.clone().requires_grad_(k in WATCH) for k, v in sd.items()}
    feats = O.video_encoder(data["video"], sdo, O.VideoCfg(num_frames=T))
    ref_scores = F.linear(feats, sdo["vid_proj.0.weight"], sdo["vid_proj.0.bias"])
    if task == "oscc":
        ref_loss = F.cross_entropy(ref_scores, data["state"])
    else:
        ref_loss = torch.mean(data["state"] * F.cross_entropy(ref_scores.squeeze(dim=-1), torch.argmax(data["labels"].long(), dim=1)))
    ref_loss.backward()
    dev = {k: v.cuda() for k, v in data.items()}
    params = dict(m.named_parameters())
    results = {}
    try:
        for mode, gbar in ((("bf16x3",), 3e-3), (("f16mix", "f16"), F16_GRAD)):
            for fused in (True, False):
                Precision.set(*mode)
                m.load_state_dict(sd, strict=True)
                k = 1.0
                if len(mode) == 2:
                    k = 1.0 / m.exec_ctx.loss_scaler(device=torch.device("cuda", 0)).get_scale()
                with torch.no_grad():
                    scores = m(dev, video_only=True).clone()
                loss = classification_step(m, CrossEntropy(), AdamW(m.parameters(), lr=1e-6), dev, task=task, fused_head=fused)
                torch.cuda.synchronize()
                errs = {"scores": CR.rel(scores, ref_scores), "loss": abs(float(loss) - float(ref_loss.detach())) / abs(float(ref_loss.detach()))}
                for w in WATCH:
                    errs["d " + w] = CR.rel(params[w].grad * k, sdo[w].grad)
                print("classification_step %s %s %s:" % (task, "/".join(mode), "fused" if fused else "fallback"),
                      {n: "%.2e" % v for n, v in errs.items()})
                assert errs["scores"] < 1e-3 and errs["loss"] < 1e-3, errs
                assert all(v < gbar for n, v in errs.items() if n.startswith("d ")), errs
                assert all(p.grad is None for n, p in params.items() if n.startswith("text_model.") or n.startswith("txt_proj."))
                results[(mode, fused)] = (float(loss), {w: (params[w].grad * k).detach().clone() for w in WATCH})
            la, ga = results[(mode, True)]
            lb, gb = results[(mode, False)]
            assert abs(la - lb) < 1e-3 * abs(lb)
            assert all(CR.rel(ga[w], gb[w]) < gbar for w in WATCH), {w: CR.rel(ga[w], gb[w]) for w in WATCH}
    finally:
        Precision.set("bf16x3")


# ------------------------------------------------------------------------------------------------ 4. an epoch of each trainer
class _Loader:
    dataset_name = "cls-synthetic"

    def __init__(self, task, sizes, seed):
        self.task, self.sizes, self.seed = task, sizes, seed
        self.batch_size, self.n_samples = sizes[0], sum(sizes)

    def __len__(self):
        return len(self.sizes)

    def __iter__(self):
        for i, B in enumerate(self.sizes):
            d = _task_batch(self.task, B, 2, seed=self.seed + i)
            if self.task == "pnr":
                g = torch.Generator().manual_seed(700 + self.seed + i)
                start = torch.randint(0, 100000, (B,), generator=g)
                d.update(fps=torch.full((B,), 29.97, dtype=torch.float64), parent_start_frame=start,
                         parent_end_frame=start + 240, parent_pnr_frame=start + torch.randint(20, 220, (B,), generator=g))
            yield d


class _Logger:
    def info(self, *a, **k):
        pass
    warning = debug = info


@pytest.mark.parametrize("task", ["oscc", "pnr"])
def test_trainer_epoch_with_device_validation(task):
    from egovlp_amd.model import metric as M
    from egovlp_amd.model.loss import CrossEntropy
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import AllGather_multi
    from egovlp_amd.trainer.trainer_oscc import Multi_Trainer_dist_OSCC
    from egovlp_amd.trainer.trainer_pnr import Multi_Trainer_dist_PNR
    Precision.set("bf16x3")
    classes = 2 if task == "oscc" else 16
    model, _ = _model(classes, 4)
    cls, metric = (Multi_Trainer_dist_OSCC, M.oscc_metrics) if task == "oscc" else (Multi_Trainer_dist_PNR, M.pnr_metrics)
    tr = cls.__new__(cls)               # the constructor is RetrievalTrainerBase's (tests/test_gpu_finetune.py runs it); its attributes:
    tr.args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=3e-5, schedule=[60, 80])
    tr.model, tr.loss, tr.metrics, tr.device = model, CrossEntropy(), [metric], torch.device("cuda", 0)
    tr.optimizer = AdamW(model.parameters(), lr=3e-5)
    tr.data_loader, tr.valid_data_loader = [_Loader(task, [4, 4], 40)], [_Loader(task, [4, 4, 3], 60)]
    tr.do_validation, tr.len_epoch, tr.total_batch_sum, tr.max_samples_per_epoch = True, 2, 4, 50000
    tr.batch_size, tr.log_step, tr.n_gpu = 4, 2, 1
    tr.tokenizer, tr.writer, tr.grad_sync, tr.logger = None, None, None, _Logger()
    tr.allgather, tr.fused_head, tr.keep_val_blocks = AllGather_multi.apply, True, True
    log = tr._train_epoch(1)
    torch.cuda.synchronize()
    assert set(log) == {"loss_0", "val_loss_0", "nested_val_metrics"} and math.isfinite(log["loss_0"])
    blocks = tr.last_val_blocks[0]
    assert [b.shape[0] for b in blocks] == [4, 4, 3]
    C = classes
    local = []
    for b in blocks:                                    # the three rank-local losses, separately, with the existing CrossEntropy
        ce = CrossEntropy()(b[:, :C].contiguous(), b[:, C].long())
        local.append(float(ce if task == "oscc" else torch.mean(b[:, C + 1] * ce)))
    print("trainer %s: val_loss_0 %.8f, separately %.8f; metrics %r" % (task, log["val_loss_0"], sum(local) / 3,
                                                                        log["nested_val_metrics"][0]))
    assert log["val_loss_0"] > 0.0 and abs(log["val_loss_0"] - sum(local) / 3) <= 1e-5 * abs(sum(local) / 3)
    allb = torch.cat(blocks).cpu()
    if task == "oscc":
        want = M.oscc_metrics(allb[:, :C], allb[:, C].long())["accuracy"]
        got = log["nested_val_metrics"][0]["oscc_metrics"]["accuracy"]
    else:
        fps = allb[:, C + 2].double() + allb[:, C + 3].double()
        assert float((fps - 29.97).abs().max()) < 1e-12
        want = M.pnr_metrics(allb[:, :C], None, allb[:, C + 1].long(), fps, allb[:, C + 4].long(), allb[:, C + 5].long(),
                             allb[:, C + 6].long())["keyframe_distance"]
        got = log["nested_val_metrics"][0]["pnr_metrics"]["keyframe_distance"]
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
