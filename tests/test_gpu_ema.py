"""The weight average on a real MI355X (`pytest -m gpu`): the three entry points of csrc/ema.hip at their table, chunk and alignment
boundaries against tests/ema_ref.py (element by element, sentinel guards around every tensor), the device-side decision, the skip
of an optimizer step that was not applied, the in-place swap on the real model and the trainers' switch.

Bound of an update (derived in tests/ema_ref.py, not measured): |got - ref| <= 3 u s, s = |e| + w |p - e|, u = 2^-24.  After n <= 4
updates in a row each contributes at most 3 u s_i and an earlier error is carried on with a factor (1 - w) <= 1, so the error of the
last shadow is at most 4 * 3 u * max_i s_i: the bound of test 5."""
import ctypes as C
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_ref as E  # noqa: E402
import multi_tensor_ref as R  # noqa: E402
from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402

DEV = "cuda"


def _h():
    from egovlp_amd import _lib
    return _lib.lib()


def _stream():
    from egovlp_amd import ops
    return ops._stream()


def _state(w=None, t=0):
    host = torch.zeros(8, dtype=torch.int32)
    host[0] = t
    if w is not None:
        host.view(torch.float32)[1] = E.f32(w)
    return host.to(DEV)


_CASES = {}


def _case(which):
    """The CPU inputs of a case, built once: (shadow specs, parameter specs, shadows, parameters)."""
    if which not in _CASES:
        es_specs, ps_specs = E.case_specs(which)
        es, ps = E.case_inputs(which)
        _CASES[which] = (es_specs, ps_specs, es, ps)
    return _CASES[which]


def _arenas(which):
    es_specs, ps_specs, es, ps = _case(which)
    ea = R.Arena(es_specs).fill(es).to(DEV)
    pa = R.Arena(ps_specs).fill(ps).to(DEV)
    return ea, pa, es, ps


# ------------------------------------------------------------------------------------------------------------ 1. the update kernel
@pytest.mark.parametrize("w", E.WEIGHTS, ids=["w1e-4", "w0.9", "w1"])
@pytest.mark.parametrize("which", E.CASES)
def test_update_kernel_at_its_boundaries(which, w):
    from egovlp_amd import ops
    ea, pa, es, ps = _arenas(which)
    if which == "boundaries":
        assert any(v.numel() > E.CHUNK and v.data_ptr() % 16 == 4 for v in ea.views) and ea.views[0].data_ptr() % 16 == 0
    p_before = pa.snapshot()
    ops.ema_update_multi(ea.views, pa.views, _state(w))
    torch.cuda.synchronize()
    ea.assert_guards("shadow arena, %s" % which)
    assert torch.equal(pa.bits, p_before)                                   # the parameters are read only: guards and values
    worst = 0.0
    for i, (got, e, p) in enumerate(zip(ea.tensors_cpu(), es, ps)):
        worst = max(worst, E.check_ema(got, E.ema_ref64(e, p, w), e, p, w, what="%s w=%g tensor %d (numel %d)" % (which, w, i, e.numel())))
    print("%s w=%g: %d tensors, largest err / (u s) = %.3f (allowed %d)" % (which, w, len(es), worst, E.K_EMA))


@pytest.mark.parametrize("which", ["boundaries", "2*table+1"])
def test_update_with_w_zero_touches_nothing(which):
    from egovlp_amd import ops
    ea, pa, es, ps = _arenas(which)
    k = max(range(len(ps)), key=lambda i: ps[i].numel())                    # the longest tensor: a NaN in its middle
    j = next(i for i in range(len(ps)) if ps[i].numel() > 0 and i != k)     # the first one: a NaN in its first element
    pa.views[k][ps[k].numel() // 2] = float("nan")
    pa.views[j][0] = float("nan")
    e_before, p_before = ea.snapshot(), pa.snapshot()
    ops.ema_update_multi(ea.views, pa.views, _state(0.0))
    torch.cuda.synchronize()
    assert torch.equal(ea.bits, e_before) and torch.equal(pa.bits, p_before)
    # ... and with any other weight each NaN does reach its element (the pass above was skipped, not lucky)
    ops.ema_update_multi(ea.views, pa.views, _state(0.5))
    torch.cuda.synchronize()
    assert int(torch.isnan(ea.views[k]).sum()) == 1 and int(torch.isnan(ea.views[j]).sum()) == 1
    assert bool(torch.isnan(ea.views[k][ps[k].numel() // 2])) and bool(torch.isnan(ea.views[j][0]))
    ea.assert_guards("after the NaN update")


# ------------------------------------------------------------------------------------------------------------ 2. the swap kernel
@pytest.mark.parametrize("which", E.CASES)
def test_swap_kernel_exchanges_bit_for_bit(which):
    from egovlp_amd import ops
    es_specs, ps_specs, _, _ = _case(which)
    g = torch.Generator().manual_seed(23)
    bits_a = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32) for n, _ in es_specs]
    bits_b = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32) for n, _ in ps_specs]
    for bits in (bits_a, bits_b):                                            # NaN payloads, quiet and signalling, and both infinities
        for t in bits:
            if t.numel() >= 5:
                t[0], t[1], t[2], t[-1] = 0x7FC12345, 0x7F812345, 0x7F800000, -(2 ** 31) + 0x7F800001 + 0x00012345
    aa = R.Arena(es_specs).fill([t.view(torch.float32) for t in bits_a]).to(DEV)
    ba = R.Arena(ps_specs).fill([t.view(torch.float32) for t in bits_b]).to(DEV)
    a0, b0 = aa.snapshot(), ba.snapshot()
    tables = ops.swap_multi(aa.views, ba.views)
    torch.cuda.synchronize()
    aa.assert_guards("a, %s" % which)
    ba.assert_guards("b, %s" % which)
    for i, (x, y, wa, wb) in enumerate(zip(aa.tensors_cpu(), ba.tensors_cpu(), bits_a, bits_b)):
        assert torch.equal(x.view(torch.int32), wb) and torch.equal(y.view(torch.int32), wa), (which, i, wa.numel())
    assert ops.swap_multi(aa.views, ba.views, tables) is tables              # swapping twice is the identity
    torch.cuda.synchronize()
    assert torch.equal(aa.bits, a0) and torch.equal(ba.bits, b0)


# ------------------------------------------------------------------------------------------------------------ 3. arguments
def test_arguments_of_the_three_entry_points():
    h, s = _h(), _stream()
    P1 = lambda x: (C.c_void_p * 1)(x)
    N1 = lambda n: (C.c_int64 * 1)(n)
    a, b = torch.full((32,), 1.0, device=DEV), torch.full((32,), 2.0, device=DEV)
    st = _state(0.5, t=3)
    st0 = st.clone()
    upd = lambda n, A, B, N, S=st.data_ptr(): h.egv_ema_update_multi(n, A, B, N, S, s)
    swp = lambda n, A, B, N: h.egv_swap_multi(n, A, B, N, s)
    for f in (upd, swp):
        assert f(-1, None, None, None) == 1
        assert f(1, None, None, None) == 1
        assert f(1, P1(a.data_ptr()), P1(None), N1(4)) == 1                  # a NULL pointer of a non-empty item
        assert f(1, P1(None), P1(b.data_ptr()), N1(4)) == 1
        assert f(1, P1(a.data_ptr()), P1(b.data_ptr()), N1(-4)) == 1         # a negative size
        assert f(1, P1(a.data_ptr()), P1(a.data_ptr() + 8), N1(16)) == 1     # overlapping ranges
        assert f(1, P1(a.data_ptr()), P1(a.data_ptr()), N1(16)) == 1
        two = lambda x, y: (C.c_void_p * 2)(x, y)
        assert f(2, two(a.data_ptr(), a.data_ptr() + 64), two(b.data_ptr(), None), (C.c_int64 * 2)(16, 16)) == 1   # a bad item BEHIND a good one
        assert f(0, None, None, None) == 0
        assert f(1, P1(None), P1(None), N1(0)) == 0                          # a size of 0 is skipped
    assert upd(1, P1(a.data_ptr()), P1(b.data_ptr()), N1(4), None) == 1      # no state block
    assert h.egv_ema_decide(None, None, 0.9, 1, s) == 1
    for bad in (1.0, 1.5, -0.01, float("nan")):
        assert h.egv_ema_decide(st.data_ptr(), None, bad, 1, s) == 1
    torch.cuda.synchronize()
    assert torch.equal(a, torch.full_like(a, 1.0)) and torch.equal(b, torch.full_like(b, 2.0)) and torch.equal(st, st0)
    assert h.egv_ema_decide(st.data_ptr(), None, 0.0, 0, s) == 0             # decay = 0 is allowed: w = 1
    torch.cuda.synchronize()
    assert int(st[0]) == 4 and float(st.view(torch.float32)[1]) == 1.0


# ------------------------------------------------------------------------------------------------------------ 4. the decision
@pytest.mark.parametrize("decay,warmup", [(0.9999, True), (0.9, False)])
def test_decision_follows_the_python_restatement(decay, warmup):
    from egovlp_amd import ops
    st = _state()
    flag = torch.zeros(1, dtype=torch.float32, device=DEV)
    ref = {"t": 0, "w": 0.0, "skipped": 0, "decay": 0.0}
    for call in range(1, 13):
        skip = call in (3, 7)
        flag.fill_(2.0 if skip else 0.0)
        ops.ema_decide(st, flag if call != 5 else None, decay, warmup)       # call 5: no flag at all
        ref = E.decide_ref(ref, skip, decay, warmup)
        got = st.cpu()
        gf = got.view(torch.float32)
        assert int(got[0]) == ref["t"] and int(got[2]) == ref["skipped"], (call, got.tolist(), ref)
        assert got[4:].tolist() == [0, 0, 0, 0]
        if skip:
            assert float(gf[1]) == 0.0
        else:
            assert R.ulp_distance_f32(float(gf[1]), ref["w"]) <= 1, (call, float(gf[1]), ref["w"])
        assert R.ulp_distance_f32(float(gf[3]), ref["decay"]) <= 1, (call, float(gf[3]), ref["decay"])
    assert ref["t"] == 10 and ref["skipped"] == 2


# ------------------------------------------------------------------------------------------------------------ 5. through the optimizer
BLOCK = 65536
FIVE = [3, BLOCK - 1, BLOCK, BLOCK + 1, 4]
LR, WD = 1e-2, 0.01


def _five_inputs(seed=4, steps=4):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) for n in FIVE]
    k = 10.0 / sum(FIVE) ** 0.5
    grads = [[torch.randn(n, generator=g) * k for n in FIVE] for _ in range(steps)]
    return ps, grads


@pytest.mark.parametrize("variant", ["scaler", "clip", "neither"])
def test_skipped_optimizer_steps_do_not_move_the_average(variant):
    from egovlp_amd.ema import ModelEMA
    from egovlp_amd.optim import AdamW, LossScaler
    ps, grads = _five_inputs()
    holder = torch.nn.Module()
    holder.p = torch.nn.ParameterList([torch.nn.Parameter(p.clone().to(DEV)) for p in ps])
    params = list(holder.p)
    S = 2.0 ** 10 if variant == "scaler" else 1.0
    scaler = LossScaler(init_scale=S, growth_interval=1000) if variant == "scaler" else None
    opt = AdamW(params, lr=LR, weight_decay=WD, max_grad_norm=1.0 if variant == "clip" else None)
    decay, warmup = 0.9, True
    ema = ModelEMA(holder, decay=decay, warmup=warmup)
    ref = [p.double() for p in ps]
    scale_max = [r.abs() for r in ref]
    applied = 0
    for step, gs in enumerate(grads, 1):
        bad = step == 2 and variant != "neither"          # without scaler and clipping nothing can tell: such a step is always applied
        for p, gr in zip(params, gs):
            p.grad = (gr * S).to(DEV)
        if bad:
            params[2].grad[BLOCK // 2] = float("inf")
        before = [p.detach().clone() for p in params]
        opt.step(scaler=scaler) if scaler is not None else opt.step()
        assert (opt.skip_flag() is None) == (variant == "neither")
        ema.update(opt)
        moved = not all(torch.equal(p.detach(), b) for p, b in zip(params, before))
        assert moved == (not bad), (variant, step)
        if not bad:
            w = E.decay_ref(decay, warmup, applied)[1]
            applied += 1
            for i, p in enumerate(params):
                snap = p.detach().cpu()
                scale_max[i] = torch.maximum(scale_max[i], E.ema_scale(ref[i], snap, w))
                ref[i] = E.ema_ref64(ref[i], snap, w)
    want = 3 if variant != "neither" else 4
    assert ema.num_updates() == want == applied and ema.skipped_updates() == 4 - want
    worst = 0.0
    names = list(ema.shadow)
    assert len(names) == 5
    for i, k in enumerate(names):
        got = ema.shadow[k].detach().cpu().double()
        err = (got - ref[i]).abs()
        bound = 4 * E.K_EMA * E.U * scale_max[i]
        worst = max(worst, float((err / (E.U * scale_max[i])).max()))
        assert bool((err <= bound).all()), (variant, k, float((err / (E.U * scale_max[i])).max()))
    print("%s: %d updates, largest err / (u max s) = %.3f (allowed %d)" % (variant, applied, worst, 4 * E.K_EMA))
    assert ema.current_decay() == E.decay_ref(decay, warmup, applied - 1)[0]


# ------------------------------------------------------------------------------------------------------------ 6. the real model
STEP_LR = 1e-4


@pytest.fixture(scope="module")
def real():
    """The 4-frame base_patch16_224 model with synthetic weights and a B = 4, L = 16 batch on the device."""
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=3)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    m = m.cuda().train()
    batch = synth_batch(4, T=4, L=16, seed=12, ragged=True)
    dev = {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
           "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}
    yield m, sd, dev
    Precision.set("bf16x3")


def _embed(m, dev):
    with torch.no_grad():
        te, ve = m({"video": dev["video"], "text": dev["text"]}, return_embeds=True)
    return te.clone(), ve.clone()


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix"])
def test_swap_on_the_real_model(real, mode):
    from egovlp_amd import weights
    from egovlp_amd.ema import ModelEMA
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.ops import Precision
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    m, sd, dev = real
    Precision.set("f16mix", "f16") if mode == "f16mix" else Precision.set(mode)
    try:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()
        m.train()
        params = [p for p in m.parameters()]
        param_bytes = sum(p.numel() for p in params) * 4
        torch.cuda.synchronize()
        mem0 = torch.cuda.memory_allocated()
        ema = ModelEMA(m, decay=0.5, warmup=False)
        grown = torch.cuda.memory_allocated() - mem0
        # no second model: the arena (parameter bytes + at most 12 bytes of alignment per tensor), the 32-byte state block and the
        # caching allocator's rounding of the two (below 2 MiB, whatever the model's size)
        assert ema.arena_bytes() <= param_bytes + 12 * len(params)
        assert ema.arena_bytes() <= grown <= ema.arena_bytes() + (2 << 20), (grown, ema.arena_bytes())
        opt = AdamW(m.parameters(), lr=STEP_LR)
        for _ in range(2):
            egoclip_step(m, EgoNCE(), opt, dev)
            assert (opt.skip_flag() is not None) == (mode == "f16mix")
            ema.update(opt)
        assert ema.num_updates() == 2 and ema.skipped_updates() == 0
        m.eval()
        emb_train = _embed(m, dev)
        assert _same(emb_train, _embed(m, dev))                               # the eval forward repeats itself bit for bit
        before = [p.detach().clone() for p in params]
        shadow_before = ema._arena.clone()
        torch.cuda.synchronize()
        mem1 = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with ema.swapped():
            peak_swap = torch.cuda.max_memory_allocated() - mem1
            emb_swapped = _embed(m, dev)
            big = max(range(len(params)), key=lambda i: params[i].numel())
            assert not torch.equal(params[big].detach(), before[big])                      # the model holds the averaged weights ...
            assert torch.equal(ema._views[big], before[big].reshape(-1))                   # ... and the arena the training weights
        torch.cuda.synchronize()
        assert peak_swap < param_bytes // 20, peak_swap                       # the exchange itself allocates nothing: no backup copy
        assert torch.cuda.memory_allocated() - mem1 < param_bytes // 20
        # after the context: every parameter and the shadow bit-identical to before, and the original embeddings
        assert _same(params, before) and torch.equal(ema._arena.view(torch.int32), shadow_before.view(torch.int32))
        emb_after = _embed(m, dev)
        print("%s: max |swapped - training| text %.3e video %.3e" % (mode, float((emb_swapped[0] - emb_train[0]).abs().max()),
                                                                     float((emb_swapped[1] - emb_train[1]).abs().max())))
        assert _same(emb_after, emb_train)
        assert not torch.equal(emb_swapped[0], emb_train[0]) and not torch.equal(emb_swapped[1], emb_train[1])
        # the same model with the averaged weights LOADED: what a missing plane invalidation inside swapped() would differ from
        missing = m.load_state_dict(ema.state_dict()["shadow"], strict=False)
        assert not missing.unexpected_keys
        weights.bump_epoch()
        emb_loaded = _embed(m, dev)
        print("%s: max |swapped - loaded| text %.3e video %.3e" % (mode, float((emb_swapped[0] - emb_loaded[0]).abs().max()),
                                                                   float((emb_swapped[1] - emb_loaded[1]).abs().max())))
        assert _same(emb_swapped, emb_loaded)
    finally:
        m.load_state_dict(sd, strict=True)
        weights.bump_epoch()
        m.train()
        Precision.set("bf16x3")


# ------------------------------------------------------------------------------------------------------------ 7. the trainer
CFG = {"name": "EgoClip_4f", "n_gpu": 1,
       "arch": {"type": "FrozenInTime", "args": {
           "video_params": {"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                            "pretrained": True, "time_init": "rand"},
           "text_params": {"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
           "projection": "minimal", "load_checkpoint": ""}},
       "optimizer": {"type": "AdamW", "args": {"lr": 1e-4}},
       "loss": {"type": "EgoNCE", "args": {}},
       "metrics": ["egomcq_accuracy_metrics"],
       "trainer": {"epochs": 1, "max_samples_per_epoch": 500000, "save_dir": "unused", "save_period": 1, "verbosity": 2,
                   "monitor": "off", "init_val": False, "neptune": False}}


class _Loader:
    """Two batches of B clips with tokenised captions."""
    dataset_name = "EgoClip-synthetic"

    def __init__(self, B, n_batches=2):
        self.batch_size, self.n_batches, self.n_samples = B, n_batches, B * n_batches

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        for i in range(self.n_batches):
            b = synth_batch(self.batch_size, T=2, L=8, seed=50 + i)
            yield {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


def _questions():
    g = torch.Generator().manual_seed(99)
    out = []
    for q in range(2):
        ids = torch.randint(1000, 30000, (1, 16), generator=g)
        ids[:, 0] = 101
        mask = torch.ones(1, 16, dtype=torch.long)
        mask[:, 10 + q:] = 0
        out.append({"video": torch.randn(1, 5, 4, 3, 224, 224, generator=g), "text": {"input_ids": ids, "attention_mask": mask},
                    "correct": torch.tensor([q % 5]), "type": torch.tensor([1 + q % 2])})
    return out


class _ValLoader(list):
    batch_size = 1
    dataset_name = "EgoMCQ-synthetic"


def _make_trainer(tmp, resume=None):
    import egovlp_amd.model.loss as module_loss
    import egovlp_amd.model.model as module_arch
    import egovlp_amd.optim as module_optim
    from egovlp_amd.model.metric import egomcq_accuracy_metrics
    from egovlp_amd.ops import Precision
    from egovlp_amd.trainer.trainer_egoclip import Multi_Trainer_dist
    from egovlp_amd.utils.config import DictConfig
    Precision.set("bf16x3")
    config = DictConfig(CFG, save_dir=tmp, resume=resume)
    model = config.initialize('arch', module_arch)
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, seed=2))
    model.text_model.set_dropout(0.0, 0.0)
    loss = config.initialize(name="loss", module=module_loss)
    optimizer = config.initialize('optimizer', module_optim, filter(lambda p: p.requires_grad, model.parameters()))
    args = types.SimpleNamespace(world_size=1, rank=0, local_rank=0, learning_rate1=1e-4, schedule=[60, 80], model_ema_decay=0.99)
    return Multi_Trainer_dist(args, model, loss, [egomcq_accuracy_metrics], optimizer, config=config, data_loader=[_Loader(2)],
                              valid_data_loader=[_ValLoader([dict(q) for q in _questions()])], tokenizer=None,
                              max_samples_per_epoch=CFG['trainer']['max_samples_per_epoch'])


def test_trainer_validates_under_the_average_and_checkpoints_it(tmp_path):
    from egovlp_amd import weights
    from egovlp_amd.model.model import sim_matrix
    from egovlp_amd.utils.util import load_checkpoint_file
    tr = _make_trainer(tmp_path / "run1")
    tr.train()
    ema = tr.ema
    assert ema is not None and not ema.is_swapped() and ema.num_updates() == 2 and ema.skipped_updates() == 0
    assert ema.current_decay() == E.decay_ref(0.99, True, 1)[0]
    logged = tr.last_val_predictions[0]
    assert logged.shape == (2, 5)
    # the same predictions by hand, from the shadow weights loaded into the model
    train_sd = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    shadow = {k: v.detach().clone() for k, v in ema.shadow.items()}
    assert any(not torch.equal(shadow[k], train_sd[k]) for k in shadow)
    tr.model.load_state_dict(shadow, strict=False)
    weights.bump_epoch()
    tr.model.eval()

    def predict():
        rows = []
        with torch.no_grad():
            for q in _questions():
                te, ve = tr.model({"video": q["video"][0].cuda(), "text": {k: v.cuda() for k, v in q["text"].items()}}, return_embeds=True)
                rows.append(sim_matrix(te, ve))
        return torch.cat(rows).cpu()
    by_hand = predict()
    tr.model.load_state_dict(train_sd, strict=True)
    weights.bump_epoch()
    of_training = predict()
    print("max |logged - by hand| %.3e, max |logged - training weights'| %.3e" % (float((logged - by_hand).abs().max()),
                                                                                 float((logged - of_training).abs().max())))
    assert torch.equal(logged, by_hand) and not torch.equal(logged, of_training)
    # the checkpoint: the training weights under 'state_dict', the average under 'ema_state_dict'; a fresh trainer resumes both
    path = str(tmp_path / "run1" / "checkpoint-epoch1.pth")
    assert os.path.exists(path)
    ck = load_checkpoint_file(path, map_location="cpu", trusted=True)
    assert ck["ema_state_dict"]["num_updates"] == 2 and set(ck["ema_state_dict"]["shadow"]) == set(shadow)
    for k, v in train_sd.items():
        assert torch.equal(ck["state_dict"][k], v.cpu()), k
    tr2 = _make_trainer(tmp_path / "run2", resume=path)
    assert tr2.ema is not None and tr2.ema.num_updates() == 2 and tr2.ema.skipped_updates() == 0 and tr2.start_epoch == 2
    for k, v in tr2.ema.shadow.items():
        assert torch.equal(v.view(torch.int32), shadow[k].view(torch.int32)), k
