"""A video tower of 24 frames, end to end on a real MI355X (`pytest -m gpu`): past the 16 frames of the one-tile time-attention kernels, so
every time attention here runs csrc/attn_time_long.hip (two 16-row tiles per location, the second one half full), and the patch gather,
token assembly, space attention (B T H groups), LayerNorm, GEMMs, stochastic depth and patch dropout run at T = 24.  Construction and
bars: tests/test_gpu_hires_model.py (embeddings 1e-3 in 'bf16x3' and 7e-4 on a batch in 'f16mix'; gradients 3e-3 / 1e-2 with the fp16
backward) against the CPU oracle on identical seeded weights and inputs."""
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
IMG, PATCH, DIM, HEADS, DEPTH, FRAMES, B = 32, 16, 128, 2, 2, 24, 2
VCFG = O.VideoCfg(img_size=IMG, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, num_frames=FRAMES)
TCFG = O.TextCfg(dim=128, n_layers=2, n_heads=2, hidden_dim=256)


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def to_dev(batch):
    return {"video": batch["video"].cuda(), "text": {k: v.cuda() for k, v in batch["text"].items()},
            "noun_vec": batch["noun_vec"].cuda(), "verb_vec": batch["verb_vec"].cuda()}


def _tower(**extra):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": FRAMES, "pretrained": True, "time_init": "rand",
          "arch_kwargs": dict(img_size=IMG, patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS)}
    vp.update(extra)
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=9)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    assert m.video_model.patches_per_frame == 4 and m.video_model.num_frames == FRAMES
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
def test_24_frame_tower_matches_the_cpu_oracle(reference, mode):
    """Embeddings and EVERY parameter gradient at 24 frames, in the parity mode and in the benchmarked pairing ('f16mix' forward, fp16
    backward on the loss times the device-side loss scale)."""
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
        print("24-frame tower %s: text %.2e video %.2e loss %.2e (bar %.1e)" % (mode, r_t, r_v, r_l, fbar))
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
        print("24-frame tower %s: worst gradient %s %.2e (bar %.1e) over %d tensors" % (mode, worst, errs[worst], gbar, len(errs)))
        assert r_t < fbar and r_v < fbar and r_l < fbar
        assert len(errs) >= len(grads) - 2
        assert all(e < gbar for e in errs.values()), {n: e for n, e in errs.items() if e >= gbar}
    finally:
        ec.set_precision("bf16x3")
        for p_ in m.parameters():
            p_.grad = None


# ---- the C block calls reach the new kernels: tests/test_gpu_hires_model.py's comparison at T = 24 --------------------------------
def _block(D=256, H=4, seed=0):
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
def test_block_calls_reach_the_24_frame_kernels(mode):
    """egv_block_fwd / egv_block_bwd go through the same *_impl functions as the per-kernel path: at T = 24 both must run the tiled
    time kernels and agree as they do at T <= 16 (bit for bit upstream of the fp32 atomics, 1e-4 / 3e-4 downstream)."""
    from egovlp_amd import ops
    # the smallest the C calls take in all three modes (block_calls_ok): D >= 256, and M = 7 972 rows are 32 x 4 = 128 tiles of the fc1
    # GEMM, from where the 'f16x2' block keeps its format (f16x2_block_ok)
    Bb, T, n, D, H = 4, 24, 83, 256, 4
    blk = _block(D, H)
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
    print("T = 24 %s: block calls vs per-kernel path:" % (mode,), {k: "%.1e" % v for k, v in diffs.items() if v})
    bar = 1e-4 if mode[1] != "f16" and mode[0] != "f16x2" else 3e-4           # tests/test_gpu_block.py's two bars
    assert all(v < bar for v in diffs.values()), diffs
    assert diffs["mlp.fc2.weight"] == 0.0 and diffs["mlp.fc1.weight"] == 0.0, diffs


# ---- training at this geometry ----------------------------------------------------------------------------------------------------
def test_train_step_with_patch_dropout_and_stochastic_depth_at_24_frames():
    """patch_drop_rate 0.5 (time attention over K = 2 of the 4 locations) and drop_path_rate 0.1 in one train-mode forward / backward:
    a finite loss and finite gradients in every parameter that has one."""
    from egovlp_amd.model.loss import EgoNCE
    m, sd = _tower(patch_drop_rate=0.5, drop_path_rate=0.1)
    assert [blk.drop_path for blk in m.video_model.blocks] == pytest.approx([0.0, 0.1])
    d = to_dev(synth_batch(8, T=FRAMES, L=16, seed=32, res=IMG, ragged=True))
    c0 = m.video_model._drop_calls
    te, ve = m(d)
    loss = EgoNCE().fused(te, ve, d["noun_vec"], d["verb_vec"])
    loss.backward()
    m.exec_ctx.join_side_stream()
    torch.cuda.synchronize()
    assert m.video_model._drop_calls == c0 + 1                     # the stochastic-depth path ran
    assert tuple(m.video_model.last_patch_keep.shape) == (8, 2)    # ... and the tower ran on 2 of the 4 patch positions
    assert bool(torch.isfinite(loss))
    n_grads = 0
    for name, p_ in m.named_parameters():
        if p_.grad is not None:
            assert bool(torch.isfinite(p_.grad).all()), name
            n_grads += 1
    assert n_grads > 0 and m.video_model.blocks[1].timeattn.qkv.weight.grad is not None


# ---- the other ways into the tower, at 24 frames ----------------------------------------------------------------------------------
def test_uint8_input_augmentation_and_the_extraction_transform_at_24_frames():
    """Decoded uint8 frames [b, 24, 3, 32, 32]: the fused train transform with the identity box is the plain uint8 gather, bit for bit;
    the fused eval transform on a frame BANK with a [b, 24] window table (the extraction path) is the same transform on the gathered
    frames, bit for bit."""
    m, _ = _tower()
    vm = m.video_model.eval()
    g = torch.Generator().manual_seed(6)
    u8 = torch.randint(0, 256, (B, FRAMES, 3, IMG, IMG), generator=g, dtype=torch.uint8).cuda()
    with torch.no_grad():
        e_plain = vm(u8)
        vm.set_input_augmentation(torch.tensor([[0, 0, IMG, IMG, 0]] * B, dtype=torch.int32), IMG)
        e_aug = vm(u8)
        assert e_plain.shape == (B, DIM) and bool(torch.isfinite(e_plain).all())
        assert torch.equal(e_plain, e_aug)
        bank = torch.randint(0, 256, (40, 3, 48, 40), generator=g, dtype=torch.uint8).cuda()
        table = torch.stack([torch.arange(0, FRAMES), torch.arange(16, 16 + FRAMES)]).to(torch.int32)
        vm.set_input_eval_transform(center_crop=IMG, out_res=IMG, frame_index=table)
        e_bank = vm(bank)
        vm.set_input_eval_transform(center_crop=IMG, out_res=IMG)
        e_clips = vm(bank[table.long().cuda()])
        assert e_bank.shape == (B, DIM) and bool(torch.isfinite(e_bank).all())
        assert torch.equal(e_bank, e_clips)


def test_cached_step_at_24_frames():
    """`egoclip_step_cached` over B = 4 in chunks of 2 with patch dropout: pass 3 re-computes, bit for bit, the embeddings pass 1 cached."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    m, sd = _tower(patch_drop_rate=0.5)
    torch.manual_seed(0)
    dev = to_dev(synth_batch(4, T=FRAMES, L=16, seed=35, res=IMG))
    opt = AdamW(m.parameters(), lr=3e-5)
    loss = egoclip_step_cached(m, EgoNCE(), opt, dev, 2, check_replay=True)
    torch.cuda.synchronize()
    assert float(m.last_replay_max_abs_diff) == 0.0
    assert bool(torch.isfinite(loss))
    w = m.video_model.blocks[0].timeattn.qkv.weight
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach().cpu(), sd["video_model.blocks.0.timeattn.qkv.weight"])
