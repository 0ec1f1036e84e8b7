"""Retrieval fine-tuning on a real MI355X: the one-call ranking-loss head (egv_maxmargin_head_fwd_bwd) against the fp64 goldens
recorded from the reference (tests/golden/finetune_head.npz, tests/finetune_ref.py), its determinism and argument checks, the
`fused` methods of the two loss classes against the existing sim_matrix + loss path, one full `retrieval_step` against the CPU
oracle, and `Multi_Trainer_dist_MIR` / `Multi_Trainer_dist_Charades` end to end on synthetic loaders.

Bars of the head are the EgoNCE head's (tests/test_gpu_ops.py::test_egonce_fused_matches_oracle): loss 1e-4 relative, gradients
1e-4 in relative Frobenius norm, similarity 1e-5.  A hinge has no gradient at its corner; the fixture's cases up to n = 200 hold
no hinge term within tau = 10 x (the reference's own fp32 similarity error) of zero and are compared in full.  At n = 1024 no
seed is clean: the gradients get an allowance equal to the exact fp64 gradient of those ambiguous terms, which may be at most
1e-4 of the kept terms."""
import os
import socket
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import finetune_ref as FR  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "finetune_head.npz"))


def _case(gold, name):
    n, D, adaptive, fix_norm, _ = FR.CASES[name]
    text, video, weight = FR.make_inputs(name, int(gold[name + "_seed"]))
    return text, video, weight, FR.margin_of(adaptive), fix_norm


# ------------------------------------------------------------------------------------------------ 1. the head vs fp64 goldens
@pytest.mark.parametrize("name", list(FR.CASES))
def test_head_matches_fp64_goldens(gold, name):
    from egovlp_amd import loss_ops
    n, D, adaptive, _, _ = FR.CASES[name]
    text, video, weight, margin, fix_norm = _case(gold, name)
    w64 = None if weight is None else weight.double()
    l64, x64, dt64, dv64 = FR.head(text.double(), video.double(), w64, margin, fix_norm)      # pinned to the reference by the CPU tests
    assert abs(float(l64) - float(gold[name + "_loss64"])) <= 1e-12 * abs(float(l64))
    if n <= FR.FULL_MAX_N:
        assert FR.rel_fro(dt64, torch.from_numpy(gold[name + "_dt64"])) < 1e-7
    loss, sim, dt, dv = loss_ops.maxmargin_head(text.cuda(), video.cuda(), None if weight is None else weight.cuda(), margin,
                                                fix_norm, want_sim=True)
    torch.cuda.synchronize()
    tau = float(gold[name + "_tau"])
    a_t, a_v, n_amb, n_kept = FR.ambiguous_allowance(text.double(), video.double(), w64, margin, fix_norm, tau)
    e_loss = abs(float(loss) - float(l64)) / abs(float(l64))
    e_sim = float((sim.cpu().double() - x64).abs().max())
    d_t, d_v = float((dt.cpu().double() - dt64).norm()), float((dv.cpu().double() - dv64).norm())
    print(f"maxmargin_head {name}: loss rel {e_loss:.2e} sim max {e_sim:.2e} d_text rel {d_t / float(dt64.norm()):.2e} "
          f"d_video rel {d_v / float(dv64.norm()):.2e} ambiguous {n_amb}/{n_kept} allowance {a_t / float(dt64.norm()):.2e} "
          f"{a_v / float(dv64.norm()):.2e} (reference fp32: {float(gold[name + '_err32_dt']):.2e} {float(gold[name + '_err32_dv']):.2e})")
    if n <= 200:
        assert n_amb == 0
    assert n_amb <= 1e-4 * n_kept
    assert e_loss < 1e-4
    assert e_sim < 1e-5
    assert d_t <= 1e-4 * float(dt64.norm()) + a_t
    assert d_v <= 1e-4 * float(dv64.norm()) + a_v
    # without `sim` the same numbers, bit for bit
    loss2, none, dt2, dv2 = loss_ops.maxmargin_head(text.cuda(), video.cuda(), None if weight is None else weight.cuda(), margin, fix_norm)
    assert none is None and torch.equal(loss, loss2) and torch.equal(dt, dt2) and torch.equal(dv, dv2)


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("name", ["mm_n200", "ada_n200_nofix", "mm_n1024", "ada_n1024"])
def test_head_is_bit_reproducible(gold, name):
    from egovlp_amd import loss_ops
    text, video, weight, margin, fix_norm = _case(gold, name)
    t, v, w = text.cuda(), video.cuda(), None if weight is None else weight.cuda()
    first = loss_ops.maxmargin_head(t, v, w, margin, fix_norm)
    for _ in range(3):
        again = loss_ops.maxmargin_head(t, v, w, margin, fix_norm)
        assert torch.equal(first[0], again[0]) and torch.equal(first[2], again[2]) and torch.equal(first[3], again[3])


# ------------------------------------------------------------------------------------------------ 3. loss.fused vs the old path
@pytest.mark.parametrize("name", ["mm_n32_nofix", "ada_n32", "mm_n48_zero", "ada_n48_d64_nofix", "mm_n200"])
def test_fused_agrees_with_sim_matrix_plus_loss(gold, name):
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss, MaxMarginRankingLoss
    from egovlp_amd.model.model import sim_matrix
    n, D, adaptive, _, _ = FR.CASES[name]
    text, video, weight, margin, fix_norm = _case(gold, name)
    loss_fn = (AdaptiveMaxMarginRankingLoss if adaptive else MaxMarginRankingLoss)(margin=margin, fix_norm=fix_norm)
    w = None if weight is None else weight.cuda()

    def run(fused, scale):
        t, v = text.cuda().requires_grad_(True), video.cuda().requires_grad_(True)
        if fused:
            loss = loss_fn.fused(t, v, w) if adaptive else loss_fn.fused(t, v)
        else:
            loss = loss_fn(sim_matrix(t, v), w) if adaptive else loss_fn(sim_matrix(t, v))
        (scale * loss).backward()
        return loss.detach(), t.grad, v.grad
    lf, tf, vf = run(True, 1.0)
    lo, to, vo = run(False, 1.0)
    e_l = abs(float(lf) - float(lo)) / abs(float(lo))
    print(f"fused vs sim_matrix + loss {name}: loss rel {e_l:.2e} d_text rel {FR.rel_fro(tf.cpu(), to.cpu()):.2e} d_video rel {FR.rel_fro(vf.cpu(), vo.cpu()):.2e}")
    assert lf.shape == () and e_l < 1e-5
    assert FR.rel_fro(tf.cpu(), to.cpu()) < 1e-4 and FR.rel_fro(vf.cpu(), vo.cpu()) < 1e-4        # clean cases: no hinge near its corner
    l3, t3, v3 = run(True, 3.0)
    assert torch.equal(l3, lf)
    assert FR.rel_fro(t3.cpu(), 3.0 * tf.cpu()) < 1e-6 and FR.rel_fro(v3.cpu(), 3.0 * vf.cpu()) < 1e-6


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_head_refuses_bad_arguments():
    from egovlp_amd import loss_ops
    from egovlp_amd._lib import EgovlpHipError
    g = torch.Generator().manual_seed(0)

    def rn(n, D):
        return torch.randn(n, D, generator=g).cuda()
    for n, D in ((1025, 256), (8, 260), (8, 254)):
        with pytest.raises(EgovlpHipError, match="nothing was launched"):
            loss_ops.maxmargin_head(rn(n, D), rn(n, D), None, 0.2, True)
    with pytest.raises(ValueError):
        loss_ops.maxmargin_head(rn(8, 256), rn(8, 256), torch.ones(7).cuda(), 0.4, True)
    with pytest.raises(ValueError):
        loss_ops.maxmargin_head(rn(8, 256), rn(9, 256), None, 0.2, True)
    with pytest.raises(EgovlpHipError):
        loss_ops.maxmargin_head(torch.randn(8, 256), torch.randn(8, 256), None, 0.2, True)
    with pytest.raises(EgovlpHipError):
        loss_ops.maxmargin_head(rn(8, 256), rn(8, 256), torch.ones(8), 0.4, True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. one full step vs the CPU oracle
def _synth_model(seed=3):
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    Precision.set("bf16x3")
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=seed)
    m.load_state_dict(sd)
    m.text_model.set_dropout(0.0, 0.0)
    return m.cuda().train(), sd


WATCH = ["video_model.blocks.0.mlp.fc1.weight", "video_model.blocks.11.attn.qkv.weight", "text_model.transformer.layer.0.ffn.lin1.weight",
         "vid_proj.0.weight", "txt_proj.1.weight"]


def _oracle_step(batch, sd, margin, fix_norm, weight):
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    rt, rv = O.frozen_in_time(batch, sdo, O.VideoCfg(num_frames=4), O.TextCfg())
    rl = O.max_margin_ranking_loss(O.sim_matrix(rt, rv), margin=margin, fix_norm=fix_norm, weight=weight)
    rl.backward()
    return rl.detach(), sdo


@pytest.mark.parametrize("adaptive", [False, True])
def test_retrieval_step_matches_cpu_oracle(adaptive):
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss, MaxMarginRankingLoss
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.trainer_epic import retrieval_step
    m, sd = _synth_model()
    batch = synth_batch(4, T=2, L=16, seed=11, ragged=True)
    relation = torch.tensor([1.0, 0.5, 0.75, 0.25])
    loss_fn = AdaptiveMaxMarginRankingLoss() if adaptive else MaxMarginRankingLoss()
    rl, sdo = _oracle_step(batch, sd, loss_fn.margin, loss_fn.fix_norm, relation if adaptive else None)
    data = {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()}, "relation": relation.cuda()}
    before = {w: dict(m.named_parameters())[w].detach().clone() for w in WATCH}
    opt = AdamW(m.parameters(), lr=3e-5)
    loss = retrieval_step(m, loss_fn, opt, data)
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    errs = {"loss": abs(float(loss) - float(rl)) / abs(float(rl))}
    for w in WATCH:
        errs[w] = FR.rel_fro(params[w].grad.cpu(), sdo[w].grad)
    print("retrieval_step (%s) vs CPU oracle:" % type(loss_fn).__name__, {k: "%.2e" % v for k, v in errs.items()})
    assert loss.shape == () and not loss.requires_grad
    assert all(v < 1e-3 for v in errs.values()), errs
    assert all(not torch.equal(params[w].detach(), before[w]) for w in WATCH)                   # the optimizer stepped
    # the fallback path (the reference's own decomposition) lands on the same loss
    m2, _ = _synth_model()
    loss_b = retrieval_step(m2, loss_fn, AdamW(m2.parameters(), lr=3e-5), data, fused_head=False)
    assert abs(float(loss_b) - float(loss)) < 1e-5 * abs(float(loss))


# ------------------------------------------------------------------------------------------------ 6. / 7. the trainers
CFG = {"name": "EpicKitchens_MIR_4f", "n_gpu": 1,
       "arch": {"type": "FrozenInTime", "args": {
           "video_params": {"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                            "pretrained": True, "time_init": "rand"},
           "text_params": {"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
           "projection": "minimal", "load_checkpoint": ""}},
       "optimizer": {"type": "AdamW", "args": {"lr": 3e-5}},
       "loss": {"type": "MaxMarginRankingLoss", "args": {"margin": 0.2}},
       "metrics": ["mir_metrics"],
       "trainer": {"epochs": 2, "max_samples_per_epoch": 500000, "save_dir": "unused", "save_period": 1, "verbosity": 2,
                   "monitor": "min val_loss_0", "init_val": False, "neptune": False}}


class FakeTokenizer:
    """Deterministic stand-in for the HF tokenizer (as tests/test_gpu_trainer.py): words -> ids, padded to the longest caption."""

    def __call__(self, texts, return_tensors='pt', padding=True, truncation=True):
        rows = [[101] + [1000 + (sum(map(ord, w)) * 7919) % 28000 for w in t.split()][:30] + [102] for t in texts]
        L = max(len(r) for r in rows)
        ids = torch.zeros(len(rows), L, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return {"input_ids": ids, "attention_mask": mask}


WORDS = "c opens the drawer and picks a knife from it then cuts an onion on the board while the man looks".split()
CLASSES = ["holding some clothes", "putting clothes somewhere", "opening a door", "washing a cup", "cutting an onion"]


class Loader:
    """`n_batches` batches of B clips with captions as STRINGS, the clip index under meta.paths, a relation weight and
    multi-hot Charades targets."""
    dataset_name = "finetune-synthetic"

    def __init__(self, B, n_batches=2, seed=50):
        self.batch_size, self.n_batches, self.seed = B, n_batches, seed
        self.n_samples = B * n_batches

    def __len__(self):
        return self.n_batches

    def batch(self, i):
        from egovlp_amd.synth import synth_batch
        B = self.batch_size
        b = synth_batch(B, T=2, L=8, seed=self.seed + i)
        g = torch.Generator().manual_seed(900 + self.seed + i)
        caps = [" ".join(WORDS[int(j)] for j in torch.randint(0, len(WORDS), (5 + k % 4,), generator=g)) for k in range(B)]
        target = (torch.rand(B, len(CLASSES), generator=g) < 0.4).float()
        target[0, 0] = 1.0
        return {"video": b["video"], "text": caps, "relation": torch.rand(B, generator=g) * 0.5 + 0.5,
                "meta": {"paths": torch.arange(i * B, (i + 1) * B)}, "target": target}

    def __iter__(self):
        return (self.batch(i) for i in range(self.n_batches))


def _annotations():
    """4 validation clips, 3 unique sentences (clips 1 and 2 share one), one fractional relevancy."""
    from egovlp_amd.model.metric import RetrievalAnnotations
    rel = np.zeros((4, 3))
    rel[[0, 1, 2, 3], [0, 1, 1, 2]] = 1.0
    rel[0, 2] = 0.5
    return RetrievalAnnotations(np.arange(4), np.array([0, 1, 3]), rel)


def _build(tmp, cfg, resume=None):
    import egovlp_amd.model.loss as module_loss
    import egovlp_amd.model.model as module_arch
    import egovlp_amd.optim as module_optim
    from egovlp_amd.ops import Precision
    from egovlp_amd.synth import synth_state_dict
    from egovlp_amd.utils.config import DictConfig
    Precision.set("bf16x3")
    config = DictConfig(cfg, save_dir=tmp, resume=resume)
    model = config.initialize('arch', module_arch)
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=2))
    model.text_model.set_dropout(0.0, 0.0)
    loss = config.initialize(name="loss", module=module_loss)
    optimizer = config.initialize('optimizer', module_optim, filter(lambda p: p.requires_grad, model.parameters()))
    return config, model, loss, optimizer


ARGS = dict(world_size=1, rank=0, local_rank=0, learning_rate1=2e-4, schedule=[2, 80])


def _mir_trainer(tmp, resume=None):
    from egovlp_amd.model.metric import mir_metrics
    from egovlp_amd.trainer.trainer_epic import Multi_Trainer_dist_MIR
    config, model, loss, optimizer = _build(tmp, CFG, resume)
    tr = Multi_Trainer_dist_MIR(types.SimpleNamespace(**ARGS), model, loss, [mir_metrics], optimizer, config=config,
                                data_loader=[Loader(2)], valid_data_loader=[Loader(2, seed=80)], tokenizer=FakeTokenizer(),
                                max_samples_per_epoch=CFG['trainer']['max_samples_per_epoch'])
    tr.annotations = _annotations()
    return tr


MIR_KEYS = {"nDCG_V2T", "nDCG_T2V", "nDCG_AVG", "mAP_V2T", "mAP_T2V", "mAP_AVG"}


def test_mir_trainer_train_checkpoint_resume_validate(tmp_path):
    from egovlp_amd.trainer.retrieval_eval import RetrievalEvaluator
    from egovlp_amd.utils.util import load_checkpoint_file
    tr = _mir_trainer(tmp_path / "run1")
    logs = []
    orig = tr._train_epoch
    tr._train_epoch = lambda epoch: logs.append(orig(epoch)) or logs[-1]
    tr.train()
    files = sorted(os.listdir(tmp_path / "run1"))
    assert files == ["checkpoint-epoch1.pth", "checkpoint-epoch2.pth", "model_best.pth"]      # val_loss_0 = 0.0 is a new "best" every epoch
    ck1 = load_checkpoint_file(str(tmp_path / "run1" / "checkpoint-epoch1.pth"), map_location="cpu", trusted=True)
    assert set(ck1) == {"arch", "epoch", "state_dict", "optimizer", "monitor_best", "config"}
    assert ck1["arch"] == "FrozenInTime" and ck1["epoch"] == 1 and len(ck1["state_dict"]) == 327 and ck1["monitor_best"] == 0.0
    assert ck1["optimizer"]["param_groups"][0]["lr"] == 2e-4               # the LR rule after epoch 1: no milestone reached
    assert tr.optimizer.param_groups[0]["lr"] == pytest.approx(2e-5)       # ... after epoch 2: milestone 2
    assert len(logs) == 2
    for log in logs:
        assert set(log) == {"loss_0", "val_loss_0", "nested_val_metrics"} and log["val_loss_0"] == 0.0 and log["loss_0"] > 0
        res = log["nested_val_metrics"][0]["mir_metrics"]
        assert set(res) == MIR_KEYS and all(0.0 < float(v) <= 100.0 for v in res.values()), res      # percentages
    # the same validation numbers from a RetrievalEvaluator fed by hand
    val = tr._valid_epoch(2)["nested_val_metrics"][0]["mir_metrics"]
    ev = RetrievalEvaluator(["mir_metrics"], annotations=_annotations())
    tok, tr_model = FakeTokenizer(), tr.model.eval()
    with torch.no_grad():
        for d in Loader(2, seed=80):
            data = {"video": d["video"].cuda(), "text": {k: v.cuda() for k, v in tok(d["text"]).items()}}
            te, ve = tr_model(data, return_embeds=True)
            ev.update(te, ve, d["meta"]["paths"])
    hand = ev.compute()[0]["mir_metrics"]
    assert set(hand) == MIR_KEYS
    for k in MIR_KEYS:
        assert float(val[k]) == pytest.approx(float(hand[k]), rel=1e-6), (k, val, hand)
        assert float(val[k]) == pytest.approx(float(logs[1]["nested_val_metrics"][0]["mir_metrics"][k]), rel=1e-6)
    final1 = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    # ---- resume from the epoch-1 file: epoch 2 runs again from the saved weights + optimizer state
    tr2 = _mir_trainer(tmp_path / "run2", resume=str(tmp_path / "run1" / "checkpoint-epoch1.pth"))
    assert tr2.start_epoch == 2
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v.cpu(), ck1["state_dict"][k]), k
    st = tr2.optimizer.state_dict()["state"]
    assert len(st) == 327 and all(s["step"] == 2 for s in st.values())
    tr2.train()
    assert "checkpoint-epoch2.pth" in os.listdir(tmp_path / "run2")
    num = den = 0.0
    for k, v in tr2.model.state_dict().items():
        d1 = final1[k] - ck1["state_dict"][k]
        d2 = v.cpu() - ck1["state_dict"][k]
        num += float((d1 - d2).double().pow(2).sum())
        den += float(d1.double().pow(2).sum())
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5                   # the bar of tests/test_gpu_trainer.py (atomics in the towers)


def test_charades_trainer_epoch_and_validation(tmp_path):
    from egovlp_amd.model.metric import charades_metrics
    from egovlp_amd.model.model import sim_matrix
    from egovlp_amd.trainer.trainer_charades import Multi_Trainer_dist_Charades
    cfg = dict(CFG, name="CharadesEgo_4f", metrics=["charades_metrics"],
               loss={"type": "AdaptiveMaxMarginRankingLoss", "args": {"margin": 0.4}},
               trainer=dict(CFG["trainer"], epochs=1, monitor="off"))
    config, model, loss, optimizer = _build(tmp_path / "ch", cfg)
    tr = Multi_Trainer_dist_Charades(types.SimpleNamespace(**ARGS), model, loss, [charades_metrics], optimizer, config=config,
                                     data_loader=[Loader(2)], valid_data_loader=[Loader(2, n_batches=3, seed=80)],
                                     tokenizer=FakeTokenizer(), max_samples_per_epoch=500000, class_sentences=CLASSES)
    before = tr.model.vid_proj[0].weight.detach().clone()
    log = tr._train_epoch(1)
    assert set(log) == {"loss_0", "val_loss_0", "nested_val_metrics"} and log["loss_0"] > 0 and log["val_loss_0"] == 0.0
    assert not torch.equal(before, tr.model.vid_proj[0].weight.detach())
    res = log["nested_val_metrics"][0]["charades_metrics"]
    assert set(res) == {"mAP"}
    # by hand: class sentences through the text tower, the clips through the video tower, sim_matrix(text, video).T vs targets
    tok, m = FakeTokenizer(), tr.model.eval()
    vids, targets = [], []
    with torch.no_grad():
        m.exec_ctx.begin_step()
        text = m.compute_text({k: v.cuda() for k, v in tok(CLASSES).items()})
        for d in Loader(2, n_batches=3, seed=80):
            vids.append(m({"video": d["video"].cuda()}, video_only=True))
            targets.append(d["target"])
        sims = sim_matrix(text, torch.cat(vids)).t()
    assert sims.shape == (6, len(CLASSES)) and tr.last_val_similarity.shape == (6, len(CLASSES))
    assert float((sims - tr.last_val_similarity).abs().max()) < 1e-6
    hand = charades_metrics(sims, torch.cat(targets))
    assert res["mAP"] == pytest.approx(hand["mAP"], rel=1e-6) and 0.0 < res["mAP"] <= 1.0
    assert tr.train() == 0 and "checkpoint-epoch1.pth" in os.listdir(tmp_path / "ch")


# ------------------------------------------------------------------------------------------------ 8. the packed collective path
@pytest.mark.parametrize("adaptive", [False, True])
def test_forced_gather_path_gives_the_same_loss(monkeypatch, adaptive):
    """EGV_FORCE_GATHER=1 at world size 1: the embeddings (and the relation weight) go through ONE all_gather_into_tensor of a
    packed row block on an RCCL process group of one rank; the loss is that of the plain run."""
    import datetime
    import torch.distributed as dist
    from egovlp_amd.model.loss import AdaptiveMaxMarginRankingLoss, MaxMarginRankingLoss
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd import gather
    from egovlp_amd.trainer.trainer_epic import retrieval_step
    batch = synth_batch(4, T=2, L=16, seed=11, ragged=True)
    data = {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
            "relation": torch.tensor([1.0, 0.5, 0.75, 0.25]).cuda()}
    loss_fn = AdaptiveMaxMarginRankingLoss() if adaptive else MaxMarginRankingLoss()
    m, _ = _synth_model()
    plain = float(retrieval_step(m, loss_fn, AdamW(m.parameters(), lr=3e-5), data))
    gathers = []
    orig = gather._gather_rows
    monkeypatch.setattr(gather, "_gather_rows", lambda t, world: gathers.append(tuple(t.shape)) or orig(t, world))
    monkeypatch.setenv("EGV_FORCE_GATHER", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        monkeypatch.setenv("MASTER_PORT", str(s.getsockname()[1]))
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0),
                            timeout=datetime.timedelta(seconds=120))
    try:
        m2, _ = _synth_model()
        forced = float(retrieval_step(m2, loss_fn, AdamW(m2.parameters(), lr=3e-5), data))
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert gathers == [(4, 256 + 256 + (1 if adaptive else 0))]           # one collective, everything packed
    assert abs(forced - plain) < 1e-5 * abs(plain), (forced, plain)
