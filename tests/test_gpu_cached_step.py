"""The embedding-cache step (`egoclip_step_cached`, egovlp_amd/trainer/cached_step.py) on a real MI355X (`pytest -m gpu`): loss and
gradients of the WHOLE batch against the fp32 CPU oracle, agreement with the plain step, bit-exact replay of the cached embeddings
under dropout, the accumulate kernel against torch, the skipped step after an overflow, and the memory bound.

The bars are the project's (tests/test_gpu_model.py): PARITY = 1e-3 on the loss, 3e-3 on gradients in 'bf16x3', 1e-2 with the fp16
backward ('f16mix')."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

PARITY = 1e-3
GRAD_BAR = {"bf16x3": 3e-3, "f16mix": 1e-2}

# test_train_step_matches_oracle's list + the two deepest tensors of the video tower
WATCH = ["video_model.blocks.3.attn.qkv.weight", "text_model.transformer.layer.2.ffn.lin1.weight", "video_model.pos_embed",
         "vid_proj.0.weight", "video_model.blocks.7.norm3.bias", "video_model.patch_embed.proj.weight",
         "video_model.blocks.0.timeattn.qkv.weight"]


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def to_dev(batch):
    return {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
            "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}


def build_full(time_init="zeros"):
    from egovlp_amd.model.model import FrozenInTime
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 16,
                                   "pretrained": True, "time_init": time_init},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    return m.cuda(), sd


def _set_mode(mode):
    from egovlp_amd.ops import Precision
    if mode == "f16mix":
        Precision.set("f16mix", "f16")
    else:
        Precision.set(mode)


@pytest.fixture(scope="module")
def full():
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m, sd = build_full()
    yield m, sd
    Precision.set("bf16x3")


_ORACLE = {}


def oracle(sd, B, seed):
    """-> (host batch, oracle loss over ALL B rows, {watched parameter: its gradient}) -- fp32 autograd on the CPU, once per batch."""
    key = (B, seed)
    if key not in _ORACLE:
        torch.set_num_threads(min(os.cpu_count() or 1, 16))
        batch = synth_batch(B, T=4, L=32, seed=seed, ragged=True)
        sdo = {k: v.clone().requires_grad_(k in WATCH) for k, v in sd.items()}
        te, ve = O.frozen_in_time(batch, sdo, O.VideoCfg(), O.TextCfg())
        ref, _ = O.egoclip_loss(te, ve, batch["noun_vec"], batch["verb_vec"])
        ref.backward()
        _ORACLE[key] = (batch, float(ref.detach()), {k: sdo[k].grad.clone() for k in WATCH}, (te.detach(), ve.detach()))
    return _ORACLE[key]


def run_step(m, sd, dev, mode, chunk=None, **kw):
    """One step with an optimizer whose lr is 0 (the parameters stay, p.grad is what the step summed) -> (loss, {watched: un-scaled
    gradient}).  chunk None: the plain step."""
    from egovlp_amd import weights
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    _set_mode(mode)
    m.load_state_dict(sd, strict=True)
    weights.bump_epoch()
    m.train()
    opt = AdamW(m.parameters(), lr=0.0)
    ec = m.exec_ctx
    S = ec.loss_scaler(device="cuda").get_scale() if ec.bwd_passes == 4 else 1.0
    if chunk is None:
        loss = egoclip_step(m, EgoNCE(), opt, dev)
    else:
        loss = egoclip_step_cached(m, EgoNCE(), opt, dev, chunk, **kw)
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    grads = {k: (params[k].grad / S).detach().cpu() for k in WATCH}
    assert all(torch.equal(params[k].detach().cpu(), sd[k]) for k in WATCH)         # lr = 0: nothing moved
    return float(loss), grads


def check_against_oracle(tag, loss, grads, ref_loss, ref_grads, bar):
    r_l = abs(loss - ref_loss) / abs(ref_loss)
    print("%s: loss %.6f oracle %.6f rel %.2e" % (tag, loss, ref_loss, r_l))
    errs = {k: rel(grads[k], ref_grads[k]) for k in WATCH}
    for k, r in errs.items():
        print("  %s grad %-50s rel %.2e (bar %.0e)" % (tag, k, r, bar))
    assert r_l < PARITY, (tag, r_l)
    for k, r in errs.items():
        assert r < bar, (tag, k, r)
    return errs


# chunk = 2 is M = 1 570 tokens per chunk: below the big-tile kernels the fp16 formats need, so 'f16mix' runs its video blocks
# split-bf16 there (ops.uses_big_gemm); chunk = 4 (M = 3 140) runs the fp16 forward and backward proper
@pytest.mark.parametrize("mode,chunk", [("bf16x3", 2), ("f16mix", 2), ("f16mix", 4)])
def test_cached_step_matches_the_oracle_on_the_whole_batch(full, mode, chunk):
    """B = 8 in chunks: the loss is EgoNCE over all 8 rows (a mean of chunk losses would miss the bar by far: other negatives) and the
    summed chunk gradients are the gradients of that loss."""
    m, sd = full
    batch, ref_loss, ref_grads, (te, ve) = oracle(sd, 8, 4321)
    try:
        loss, grads = run_step(m, sd, to_dev(batch), mode, chunk)
        check_against_oracle("B=8 chunk=%d %s" % (chunk, mode), loss, grads, ref_loss, ref_grads, GRAD_BAR[mode])
        # what a mean of per-chunk losses would have been (oracle embeddings) -- the bar tells the two apart
        parts = [float(O.egoclip_loss(te[i:i + chunk], ve[i:i + chunk], batch["noun_vec"][i:i + chunk], batch["verb_vec"][i:i + chunk])[0])
                 for i in range(0, 8, chunk)]
        mean_of_chunks = sum(parts) / len(parts)
        print("  mean of chunk losses would be %.6f (rel %.2e from the whole-batch loss)" % (mean_of_chunks, abs(mean_of_chunks - ref_loss) / abs(ref_loss)))
        assert abs(mean_of_chunks - ref_loss) > 10 * PARITY * abs(ref_loss)
    finally:
        _set_mode("bf16x3")


def test_ragged_chunks(full):
    """B = 6, chunk = 4: chunks of 4 and 2 rows."""
    m, sd = full
    batch, ref_loss, ref_grads, _ = oracle(sd, 6, 977)
    loss, grads = run_step(m, sd, to_dev(batch), "bf16x3", 4)
    check_against_oracle("B=6 chunk=4 bf16x3", loss, grads, ref_loss, ref_grads, GRAD_BAR["bf16x3"])


def test_cached_step_agrees_with_the_plain_step(full):
    """Same batch, 'bf16x3': chunk = 2 against `egoclip_step`.  Each is within one gradient bar of the oracle, so they are within two
    of each other."""
    m, sd = full
    batch, ref_loss, ref_grads, _ = oracle(sd, 8, 4321)
    dev = to_dev(batch)
    bar = GRAD_BAR["bf16x3"]
    loss_p, g_p = run_step(m, sd, dev, "bf16x3", None)
    loss_c, g_c = run_step(m, sd, dev, "bf16x3", 2)
    check_against_oracle("plain  B=8 bf16x3", loss_p, g_p, ref_loss, ref_grads, bar)
    check_against_oracle("cached B=8 chunk=2 bf16x3", loss_c, g_c, ref_loss, ref_grads, bar)
    print("plain loss %.7f cached loss %.7f" % (loss_p, loss_c))
    assert abs(loss_p - loss_c) < 2 * PARITY * abs(ref_loss)
    for k in WATCH:
        r = rel(g_c[k], g_p[k])
        print("  cached vs plain grad %-50s rel %.2e" % (k, r))
        assert r <= 2 * bar, (k, r)


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix"])
def test_replay_reproduces_the_cached_embeddings_under_dropout(full, mode):
    """Text dropout 0.1 / 0.1: pass 3 must re-compute, bit for bit, the embeddings pass 1 cached -- same train-mode kernels, same
    counter-based masks (the dropout call counter is put back per chunk).  The spread of two identical train-mode forwards is measured
    and printed next to it (a forward kernel that is not bit-reproducible would show there).  A second step draws other masks."""
    m, sd = full
    batch = synth_batch(8, T=4, L=32, seed=611, ragged=True)
    dev = to_dev(batch)
    m.text_model.set_dropout(0.1, 0.1)
    try:
        _, _ = run_step(m, sd, dev, mode, 4, check_replay=True)
        d1 = float(m.last_replay_max_abs_diff)
        t1, v1 = (x.clone() for x in m.last_cached_embeddings)
        # the spread of two identical train-mode forwards (same rows, same dropout counter)
        ec, tm = m.exec_ctx, m.text_model
        outs = []
        for _ in range(2):
            c0 = tm._drop_calls
            with torch.no_grad(), ec.train_kernels_without_grad():
                te, ve = m({"video": dev["video"][:4], "text": {k: v[:4] for k, v in dev["text"].items()}})
            tm._drop_calls = c0
            outs.append((te.clone(), ve.clone()))
        spread = max(float((outs[0][0] - outs[1][0]).abs().max()), float((outs[0][1] - outs[1][1]).abs().max()))
        _, _ = run_step(m, sd, dev, mode, 4, check_replay=True)
        d2 = float(m.last_replay_max_abs_diff)
        t2, v2 = m.last_cached_embeddings
        print("%s replay: max |pass-3 - cached| step 1 %.3e step 2 %.3e; spread of two identical forwards %.3e; "
              "text cache step 2 vs step 1 rel %.2e, video %.2e" % (mode, d1, d2, spread, rel(t2, t1), rel(v2, v1)))
        assert spread == 0.0
        assert d1 == 0.0 and d2 == 0.0
        assert not torch.equal(t1, t2)                          # the counter advanced: other masks
        assert torch.equal(v1, v2)                              # the video tower has no dropout
    finally:
        m.text_model.set_dropout(0.0, 0.0)
        _set_mode("bf16x3")


def test_accumulate_kernel_is_bit_equal_to_torch():
    from egovlp_amd import ops
    g = torch.Generator().manual_seed(5)
    sizes = [1, 3, 768, 590592, 1027, 4098, 16384, 16385, 2 * 16384 + 7]
    dst, src = [], []
    for n in sizes:
        dst.append(torch.randn(n, generator=g).cuda())
        src.append(torch.randn(n, generator=g).cuda())
    # views at a 4-byte offset: destination only, source only, both
    for n, od, os_ in ((590592, 1, 0), (5000, 0, 1), (16384 + 9, 1, 1), (3, 1, 3)):
        dst.append(torch.randn(n + 4, generator=g).cuda()[od:od + n])
        src.append(torch.randn(n + 4, generator=g).cuda()[os_:os_ + n])
    # more tensors than one kernel-argument table holds, 2-d shapes, an empty tensor
    for i in range(130):
        dst.append(torch.randn(3 + i % 5, 7, generator=g).cuda())
        src.append(torch.randn(3 + i % 5, 7, generator=g).cuda())
    dst.append(torch.zeros(0).cuda())
    src.append(torch.zeros(0).cuda())
    assert any(d.data_ptr() % 16 for d in dst) and any(s.data_ptr() % 16 for s in src)
    want = [d + s for d, s in zip(dst, src)]
    ops.grad_accumulate_multi(dst, src)
    torch.cuda.synchronize()
    for i, (d, w) in enumerate(zip(dst, want)):
        assert torch.equal(d, w), (i, d.numel())
    assert dst[len(sizes)].storage_offset() == 1
    # count = 0 is a no-op; a non-finite value survives the sum
    ops.grad_accumulate_multi([], [])
    a, b = torch.zeros(1030).cuda(), torch.zeros(1030).cuda()
    b[517], b[1029] = float("inf"), float("nan")
    ops.grad_accumulate_multi([a], [b])
    assert bool(torch.isinf(a[517])) and bool(torch.isnan(a[1029])) and int(torch.isfinite(a).sum()) == 1028
    # bad arguments: an error, nothing launched
    from egovlp_amd import _lib
    import ctypes as C
    h = _lib.lib()
    P1, N1 = (C.c_void_p * 1), (C.c_int64 * 1)
    assert h.egv_grad_accumulate_multi(-1, None, None, None, None) == 1
    assert h.egv_grad_accumulate_multi(1, None, None, None, None) == 1
    assert h.egv_grad_accumulate_multi(1, P1(a.data_ptr()), P1(None), N1(4), None) == 1
    assert h.egv_grad_accumulate_multi(1, P1(a.data_ptr()), P1(b.data_ptr()), N1(-4), None) == 1
    assert h.egv_grad_accumulate_multi(1, P1(a.data_ptr()), P1(a.data_ptr() + 8), N1(16), None) == 1      # overlapping ranges
    assert h.egv_grad_accumulate_multi(0, None, None, None, None) == 0


def test_offset_views_leave_their_neighbours_alone():
    from egovlp_amd import ops
    buf = torch.full((16384 + 64,), 7.0).cuda()
    src = torch.ones(16384 + 11).cuda()
    ops.grad_accumulate_multi([buf[1:1 + src.numel()]], [src])
    torch.cuda.synchronize()
    assert float(buf[0]) == 7.0 and bool((buf[1:1 + src.numel()] == 8.0).all()) and bool((buf[1 + src.numel():] == 7.0).all())


def test_overflow_in_a_chunk_skips_the_step():
    """'f16mix' with the fp16 backward and a loss scale of 2^30 (where tests/test_gpu_f16bwd.py starts its skipped-step test): the fp16
    gradient planes of the chunks overflow to inf, the inf survives the fp32 sums, the optimizer's scan of the ACCUMULATORS skips the
    step -- parameters bit-unchanged, one skipped step, S halved.  The next step at a sane scale applies."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW, LossScaler
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step_cached
    m, sd = build_full(time_init="rand")
    m = m.train()
    m.exec_ctx.set_precision("f16mix", "f16")
    dev = to_dev(synth_batch(8, T=4, L=16, seed=21))
    opt = AdamW(m.parameters(), lr=3e-5)
    sc = LossScaler(init_scale=2.0 ** 30, growth_interval=1000, max_scale=2.0 ** 30)
    watch = [m.video_model.blocks[0].attn.qkv.weight, m.video_model.blocks[11].mlp.fc2.weight, m.text_model.transformer.layer[0].ffn.lin1.weight]
    before = [w.detach().clone() for w in watch]
    loss = egoclip_step_cached(m, EgoNCE(), opt, dev, 4, scaler=sc)
    assert bool(torch.isfinite(loss))
    assert sc.skipped_steps() == 1 and sc.get_scale() == 2.0 ** 29
    assert all(torch.equal(w.detach(), b0) for w, b0 in zip(watch, before))
    assert not bool(torch.isfinite(watch[0].grad).all())          # the accumulator carries the overflow
    sc.load_state_dict({"scale": 2.0 ** 16, "growth_tracker": 0, "skipped": 1})
    loss2 = egoclip_step_cached(m, EgoNCE(), opt, dev, 4, scaler=sc)
    assert bool(torch.isfinite(loss2)) and sc.skipped_steps() == 1 and sc.get_scale() == 2.0 ** 16
    assert all(not torch.equal(w.detach(), b0) for w, b0 in zip(watch, before))
    assert all(bool(torch.isfinite(w).all()) for w in watch)


def test_memory_is_bounded_by_the_chunk():
    """b = 16: the cached step over 4b rows in chunks of b peaks below the plain step over 2b rows."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    b = 16
    m, _ = build_full(time_init="rand")
    m = m.train()
    m.exec_ctx.set_precision("f16mix", "f16")
    opt = AdamW(m.parameters(), lr=3e-5)
    big = to_dev(synth_batch(4 * b, T=4, L=32, seed=99))

    def rows(n):
        return {"video": big["video"][:n], "text": {k: v[:n] for k, v in big["text"].items()}, "noun_vec": big["noun_vec"][:n],
                "verb_vec": big["verb_vec"][:n]}

    def peak(fn):
        fn()                                      # first call: optimizer state, weight planes, workspaces of this shape
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    base = torch.cuda.memory_allocated()
    p_b = peak(lambda: egoclip_step(m, EgoNCE(), opt, rows(b)))
    p_2b = peak(lambda: egoclip_step(m, EgoNCE(), opt, rows(2 * b)))
    p_c = peak(lambda: egoclip_step_cached(m, EgoNCE(), opt, big, b))
    print("peak allocated: plain B=%d %.2f GB, plain B=%d %.2f GB, cached B=%d chunk=%d %.2f GB (resident before the steps: %.2f GB)" % (
        b, p_b / 2 ** 30, 2 * b, p_2b / 2 ** 30, 4 * b, b, p_c / 2 ** 30, base / 2 ** 30))
    assert p_c < p_2b
