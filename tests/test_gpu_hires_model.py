"""A video tower at a higher input resolution, end to end on a real MI355X (`pytest -m gpu`): img_size 288 / patch 16 = 324 patches per
frame, 325 keys per space-attention group -- past the 288 keys of the LDS-resident kernels, so every space attention here runs the
key-tiled kernels of csrc/attn_long.hip, and the patch gather, token assembly, LayerNorm, GEMMs, time attention (B n H groups) and
stochastic depth run at n = 324.  Bars: those of tests/test_gpu_model.py (embeddings 1e-3 in 'bf16x3' and 7e-4 on a batch in 'f16mix';
gradients 3e-3 / 1e-2 with the fp16 backward) against the CPU oracle on identical seeded weights and inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

PARITY = 1e-3          # tests/test_gpu_model.py
MIX_BAR = 7e-4
F16_GRAD = 1e-2

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
IMG, PATCH, DIM, HEADS, DEPTH, FRAMES, B = 288, 16, 128, 2, 2, 2, 2
VCFG = O.VideoCfg(img_size=IMG, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, num_frames=FRAMES)
TCFG = O.TextCfg(dim=128, n_layers=2, n_heads=2, hidden_dim=256)


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def to_dev(batch):
    return {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
            "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}


def _tower(rate=0.0):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": FRAMES, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(img_size=IMG, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS)}
    if rate:
        vp["drop_path_rate"] = rate
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    assert m.video_model.patches_per_frame == 324
    return m.cuda().train(), sd


@pytest.fixture(scope="module")
def reference():
    """The CPU oracle's embeddings, loss and every parameter gradient at this geometry: computed once, shared, left unchanged."""
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m, sd = _tower()
    batch = synth_batch(B, T=FRAMES, L=16, seed=31, res=IMG, ragged=True)
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    rt, rv = O.frozen_in_time(batch, sdo, VCFG, TCFG)
    rl, _ = O.egoclip_loss(rt, rv, batch["noun_vec"], batch["verb_vec"])
    rl.backward()
    grads = {k: v.grad.detach().clone() for k, v in sdo.items() if v.grad is not None}
    yield m, batch, rt.detach(), rv.detach(), rl.detach(), grads
    Precision.set("bf16x3")


@pytest.mark.parametrize("mode", ["bf16x3", "f16mix/f16"])
def test_high_resolution_tower_matches_the_cpu_oracle(reference, mode):
    """Embeddings and EVERY parameter gradient at 325 keys per group, in the parity mode and in the benchmarked pairing ('f16mix'
    forward, fp16 backward on the loss times the device-side loss scale)."""
    from egovlp_amd.model.loss import EgoNCE
    m, batch, rt, rv, rl, grads = reference
    ec = m.exec_ctx
    try:
        if mode == "bf16x3":
            ec.set_precision("bf16x3")
        else:
            ec.set_precision(*mode.split("/"))
        fbar, gbar = (PARITY, 3 * PARITY) if mode == "bf16x3" else (MIX_BAR, F16_GRAD)
        for p_ in m.parameters():
            p_.grad = None
        d = to_dev(batch)
        te, ve = m(d)
        loss = EgoNCE().fused(te, ve, d["noun_vec"], d["verb_vec"])
        k = 1.0
        if ec.bwd_passes == 4:
            sc = ec.loss_scaler()
            k = 1.0 / sc.get_scale()
            sc.scale(loss).backward()
        else:
            loss.backward()
        ec.join_side_stream()
        torch.cuda.synchronize()
        r_t, r_v, r_l = rel(te, rt), rel(ve, rv), abs(float(loss.detach()) - float(rl)) / abs(float(rl))
        print("hires tower %s: text %.2e video %.2e loss %.2e (bar %.1e)" % (mode, r_t, r_v, r_l, fbar))
        errs = {}
        got = {name: p_.grad * k for name, p_ in m.named_parameters()}
        for name in got:
            if name.endswith("attention.k_lin.bias"):
                # a key bias shifts every score of a query row by the same q . b: the softmax does not see it and the exact gradient
                # is ZERO (the oracle's own value is its fp32 round-off) -- held to the bar as a fraction of the query bias's gradient
                errs[name] = float(got[name].double().norm().cpu() / grads[name.replace("k_lin", "q_lin")].double().norm())
            elif name in grads and float(grads[name].norm()) > 0:
                errs[name] = rel(got[name], grads[name])
        worst = max(errs, key=errs.get)
        for name, e in errs.items():
            print("   grad %-58s %.2e" % (name, e))
        print("hires tower %s: worst gradient %s %.2e (bar %.1e) over %d tensors" % (mode, worst, errs[worst], gbar, len(errs)))
        assert r_t < fbar and r_v < fbar and r_l < fbar
        assert len(errs) >= len(grads) - 2
        assert all(e < gbar for e in errs.values()), {n: e for n, e in errs.items() if e >= gbar}
    finally:
        ec.set_precision("bf16x3")
        for p_ in m.parameters():
            p_.grad = None


# ---- the C block calls reach the long kernels: tests/test_gpu_block.py's comparison at n = 324 ------------------------------------
def _block(D=768, H=12, seed=0):
    from functools import partial
    from torch import nn
    from egovlp_amd.model.video_transformer import SpaceTimeBlock
    torch.manual_seed(seed)
    blk = SpaceTimeBlock(dim=D, num_heads=H, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), time_init='rand')
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return blk.cuda().train()


def _run(blk, ec, x, g, Bb, T, n, block_calls):
    from egovlp_amd.model import video_transformer as vt
    ec.set(block_calls=block_calls, wgrad_side_stream=False)
    for p in blk.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    ec.begin_step()
    y = blk(xin, Bb, T, n, ec)
    used = "c" if isinstance(y.grad_fn, vt._SpaceTimeBlockCFn._backward_cls) else "k"
    y.backward(g)
    ec.join_side_stream()
    torch.cuda.synchronize()
    return y.detach().clone(), xin.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in blk.named_parameters()}, used


@pytest.mark.parametrize("mode", [("bf16x3", "bf16x3"), ("bf16x3", "bf16"), ("f16x2", "f16")])
def test_block_calls_reach_the_long_kernels(mode):
    """egv_block_fwd / egv_block_bwd go through the same *_impl functions as the per-kernel path: at 325 keys both must run the
    key-tiled kernels and agree as they do at 197 (bit for bit upstream of the fp32 atomics, 1e-4 / 3e-4 downstream)."""
    from egovlp_amd import ops
    Bb, T, n, D = 4, 4, 324, 768
    blk = _block(D)
    blk.layer_index, blk.depth = 5, 12
    ec = ops.new_context()
    ec.set_precision(*mode)
    torch.manual_seed(5)
    x = torch.randn(Bb, 1 + T * n, D, device="cuda")
    g = torch.randn(Bb, 1 + T * n, D, device="cuda") * 0.1
    y_c, dx_c, gr_c, used_c = _run(blk, ec, x, g, Bb, T, n, True)
    y_k, dx_k, gr_k, used_k = _run(blk, ec, x, g, Bb, T, n, False)
    assert (used_c, used_k) == ("c", "k")
    assert torch.equal(y_c, y_k)

    def r(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())
    diffs = {"dx": r(dx_c, dx_k), **{k: r(gr_c[k], gr_k[k]) for k in gr_k}}
    print("n = 324 %s: block calls vs per-kernel path:" % (mode,), {k: "%.1e" % v for k, v in diffs.items() if v})
    bar = 1e-4 if mode[1] != "f16" and mode[0] != "f16x2" else 3e-4           # tests/test_gpu_block.py's two bars
    assert all(v < bar for v in diffs.values()), diffs
    assert diffs["mlp.fc2.weight"] == 0.0 and diffs["mlp.fc1.weight"] == 0.0, diffs


# ---- training at this geometry ----------------------------------------------------------------------------------------------------
def test_train_step_with_stochastic_depth_at_324_patches():
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    m, sd = _tower(rate=0.1)
    assert [blk.drop_path for blk in m.video_model.blocks] == pytest.approx([0.0, 0.1])
    opt = AdamW(m.parameters(), lr=3e-5)
    batch = to_dev(synth_batch(8, T=FRAMES, L=16, seed=32, res=IMG, ragged=True))
    c0 = m.video_model._drop_calls
    loss = egoclip_step(m, EgoNCE(), opt, batch)
    torch.cuda.synchronize()
    assert m.video_model._drop_calls == c0 + 1                     # the stochastic-depth path ran
    assert bool(torch.isfinite(loss))
    w = m.video_model.blocks[1].attn.qkv.weight
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach().cpu(), sd["video_model.blocks.1.attn.qkv.weight"])


def test_egoclip_step_and_egomcq_forward_in_the_benchmarked_mode():
    """One `egoclip_step` in 'f16mix' / 'f16' under the model's LossScaler (finite loss, no skipped step), then an EgoMCQ-shaped
    forward (one question: a text query and five candidate clips) under no_grad in eval mode."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.model.model import sim_matrix
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    m, sd = _tower()
    m.exec_ctx.set_precision("f16mix", "f16")
    opt = AdamW(m.parameters(), lr=3e-5)
    batch = to_dev(synth_batch(B, T=FRAMES, L=16, seed=33, res=IMG, ragged=True))
    sc = m.exec_ctx.loss_scaler()
    loss = egoclip_step(m, EgoNCE(), opt, batch, scaler=sc)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert sc.skipped_steps() == 0
    w = m.video_model.blocks[0].attn.qkv.weight
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach().cpu(), sd["video_model.blocks.0.attn.qkv.weight"])
    m.eval()
    q = synth_batch(5, T=FRAMES, L=16, seed=34, res=IMG)
    with torch.no_grad():
        te, ve = m({"video": q["video"].cuda(), "text": {k: v[:1].cuda() for k, v in q["text"].items()}})
        pred = sim_matrix(te, ve)
    assert pred.shape == (1, 5) and bool(torch.isfinite(pred).all())


# ---- the text tower past 288 tokens -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_calls", [True, False])
def test_distilbert_at_320_tokens_through_both_layer_paths(block_calls):
    """DistilBERT has 512 positions; the tower has no length cap of its own, and both the C layer call (egv_text_layer_fwd / _bwd) and the
    per-kernel path reach the key-tiled attention at L = 320: last_hidden_state and two weight gradients against the CPU oracle."""
    from egovlp_amd.model import text_transformer as tt
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    cfg = dict(vocab_size=2000, dim=256, n_layers=1, n_heads=4, hidden_dim=512)
    m = tt.DistilBertModel(tt.DistilBertConfig(**cfg))
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=13)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    m.set_dropout(0.0, 0.0)
    Bt, L = 2, 320
    ec = m.exec_ctx
    ec.set(block_calls=block_calls, wgrad_side_stream=False)
    assert tt.text_calls_ok(ec, Bt * L, 256, 512, 4) == block_calls
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 2000, (Bt, L), generator=g)
    mask = (torch.arange(L)[None] < torch.tensor([L, 301])[:, None]).long()
    out = m(input_ids=ids.cuda(), attention_mask=mask.cuda()).last_hidden_state
    out.square().sum().backward()
    ec.join_side_stream()
    torch.cuda.synchronize()
    sdo = {"text_model." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.distilbert(ids, mask, sdo, O.TextCfg(vocab_size=2000, dim=256, n_layers=1, n_heads=4, hidden_dim=512))
    ref.square().sum().backward()
    r = rel(out, ref)
    print("DistilBERT L = 320 (block_calls=%s): last_hidden_state %.2e" % (block_calls, r))
    assert r < PARITY
    for name in ("transformer.layer.0.attention.q_lin.weight", "transformer.layer.0.attention.v_lin.weight",
                 "embeddings.position_embeddings.weight"):
        rg = rel(dict(m.named_parameters())[name].grad, sdo["text_model." + name].grad)
        print("   grad %-45s %.2e" % (name, rg))
        assert rg < 3 * PARITY, (name, rg)
