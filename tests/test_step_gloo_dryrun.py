"""The WHOLE data-parallel step on two (and three) real ranks, on CPU: `egoclip_step` of the real model (host code, autograd functions,
execution context) over the do-nothing C-ABI stand-in (tests/mock_hip.py), with a real gloo process group underneath -- the
embedding all-gather of forward, the hook-free bucket launches from the polls inside backward, the direct exchange
(all-to-all of slices -> fp32 slice sum -> all-gather), finish(), the optimizer call.  It is the closest this GPU-less container
gets to `bench.py --gpus 2`: what it pins is that the two ranks issue the SAME collectives in the SAME order (a mismatch hangs:
the test has a timeout), that buckets leave during backward on both ranks, that rank 0's initial weights arrive everywhere and
that every rank ends the step with bit-identical gradients.  Kernels compute nothing here (gradients are whatever torch.empty
left in them), so nothing is said about values -- tests/test_gradsync_gloo.py pins the arithmetic of the exchange, the -m gpu
tests the kernels."""
import hashlib
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _pack(grads, flat, offsets, scale):
    for g, o in zip(grads, offsets):
        flat[o:o + g.numel()] = (g.reshape(-1) * scale).to(torch.bfloat16)


def _unpack(grads, flat, offsets):
    for g, o in zip(grads, offsets):
        g.copy_(flat[o:o + g.numel()].float().view_as(g))


def _slice_sum(recv, world, slice_elems, out):
    out.copy_(recv.view(world, slice_elems).float().sum(0).to(torch.bfloat16))


def _digest(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


def _worker(rank, world, port, out, exchange, tiny=False, B=2, precision=("bf16x3", "bf16"), T=2, uneven=False):
    for p in (HERE, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mock_hip import mock_hip
    from egovlp_amd.dist import Bf16GradSync
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.optim import AdamW
    from egovlp_amd.synth import synth_batch
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step
    # the ORDER of collectives this rank issues (op, payload elements): what must be identical on every rank, whatever their pace
    coll_log = []
    for _name in ("all_to_all_single", "all_gather_into_tensor", "all_reduce", "broadcast"):
        def _wrap(fn, _name=_name):
            def logged(*a, **k):
                coll_log.append((_name, int(a[0].numel())))
                return fn(*a, **k)
            return logged
        setattr(dist, _name, _wrap(getattr(dist, _name)))
    torch.manual_seed(100 + rank)                         # different initial weights per rank: the broadcast must fix that
    if tiny:
        model = FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()
    else:
        model = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                           "pretrained": True, "time_init": "rand"},
                             text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                             projection="minimal", load_checkpoint="").train()
    model.text_model.seed_rank = rank
    ec = model.exec_ctx
    sync = Bf16GradSync(model.parameters(), use_hooks=False, order_hint=model.gradient_ready_order(), exec_ctx=ec,
                        exchange=exchange, pack_fn=_pack, unpack_fn=_unpack, slice_sum_fn=_slice_sum,
                        **({"bucket_mb": 1.0} if tiny else {}))
    w0 = _digest(p for p in model.parameters())
    if uneven:
        # UNEQUAL host speeds: every rank stalls for its own, step- and call-dependent time at every poll of backward (where buckets are
        # launched) -- a rank that is ahead launches its buckets long before a slow one does; the collectives must still pair up in order
        import time
        _poll, _n = sync.poll, [0]

        def slow_poll():
            _n[0] += 1
            time.sleep(0.004 * ((rank * 5 + _n[0] * 3) % 7))
            _poll()
        ec.set(backward_poll=slow_poll, gemm_grid=248)
    else:
        ec.set(backward_poll=sync.poll, gemm_grid=248)
    ec.set_precision(*precision)
    opt = AdamW(model.parameters(), lr=3e-5)
    b = synth_batch(B, T=T, L=16, seed=3, rank=rank, **({"res": 32} if tiny else {}))
    data = {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}
    steps = []
    gathered = []
    if tiny:    # what the loss sees after the fused gather: record the shapes egv_egonce_fwd_bwd is called with
        from egovlp_amd import loss_ops as _ops
        _orig = _ops.egonce_fwd_bwd

        def spy(text, video, noun, verb, *a, **k):
            gathered.append((tuple(text.shape), tuple(video.shape), tuple(noun.shape), tuple(verb.shape)))
            return _orig(text, video, noun, verb, *a, **k)
        _ops.egonce_fwd_bwd = spy
        import egovlp_amd.model.loss as _loss_mod
        if hasattr(_loss_mod, "loss_ops"):
            _loss_mod.loss_ops.egonce_fwd_bwd = spy
    with mock_hip() as calls:
        for step in range(2):
            calls.clear()
            # gradients come out of torch.empty (the kernels are stand-ins): give every rank DIFFERENT, finite ones, so that
            # "identical after the exchange" means something -- the wgrad buffers are allocated by the host code, fill them
            # right before the exchange reads them (the pack stand-in sees p.grad)
            def pack(grads, flat, offsets, scale, _step=step):
                for i, g in enumerate(grads):
                    g.copy_(torch.full_like(g, float(rank + 1) + 0.25 * _step + (i % 7)))
                _pack(grads, flat, offsets, scale)
            sync.pack_fn = pack
            egoclip_step(model, EgoNCE(), opt, data, world, rank, grad_sync=sync)
            steps.append({"during": sync.stats["launched_during_backward"], "buckets": sync.stats["buckets"],
                          "grads": _digest(p.grad for p in model.parameters()),
                          "first": float(next(model.parameters()).grad.reshape(-1)[0]),
                          "gemm_calls": calls.count("egv_gemm_nt"), "adamw": calls.count("egv_adamw_multi"),
                          "text_layers": calls.count("egv_text_layer_bwd"), "blocks": calls.count("egv_block_bwd"),
                          "x2_refresh": calls.count("egv_f16x2_encode_multi")})
    torch.save({"w0": w0, "steps": steps, "gathered": gathered, "slices": [int(x) for x in getattr(sync, "slice_elems", [])], "collectives": coll_log},
               os.path.join(out, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("exchange,world", [("direct", 2), ("allreduce", 2), ("direct", 3)])
def test_multi_rank_step_on_the_real_model(tmp_path, exchange, world):
    port = 29671 + (exchange == "direct") + 2 * (world - 2)
    mp.spawn(_worker, args=(world, port, str(tmp_path), exchange), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt"), weights_only=False) for i in range(world)]
    assert all(x["w0"] == r[0]["w0"] for x in r)                      # rank 0's initial weights everywhere
    for step in range(2):
        a = r[0]["steps"][step]
        for x in r[1:]:
            b = x["steps"][step]
            assert a["buckets"] == b["buckets"] >= 5
            assert a["grads"] == b["grads"], step                     # bit-identical gradients on every rank after finish()
        if world == 2:
            # the mean of the two ranks' fills of a parameter: ((1 + s/4 + i%7) + (2 + s/4 + i%7)) / 2 -- exact in bf16
            assert abs(a["first"] - round(a["first"] * 4) / 4) < 1e-6 and abs((a["first"] % 1.0) - (0.5 + 0.25 * step) % 1.0) < 1e-6, a["first"]
        for x in (y["steps"][step] for y in r):
            assert x["during"] >= x["buckets"] - 1, x                 # only the tail bucket may be left to finish()
            # 12 video blocks x 18 GEMMs (per-kernel at this toy token count), patch embedding, two heads; the six DistilBERT
            # layers go through their layer calls (csrc/text_layer.hip)
            assert x["gemm_calls"] == 12 * 18 + 2 + 2 * 3 and x["text_layers"] == 6 and x["adamw"] >= 1


@pytest.mark.timeout(900)
def test_eight_rank_step_on_a_toy_model(tmp_path):
    """World size 8 (the node the metric is quoted on) -- on a toy dual encoder so that eight CPU processes fit: the fused
    embedding gather hands the loss the GLOBAL batch (n = 8 x 32 = 256 rows of each of the four gathered tensors: the size
    egv_egonce_fwd_bwd runs at on the 8-GPU node), the direct exchange cuts every bucket into 8 slices (slice alignment), all
    ranks issue the same collectives in the same order (else: hang -> timeout) and end with bit-identical gradients."""
    world, B = 8, 32
    mp.spawn(_worker, args=(world, 29699, str(tmp_path), "direct", True, B), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt"), weights_only=False) for i in range(world)]
    assert all(x["w0"] == r[0]["w0"] for x in r)
    for step in range(2):
        a = r[0]["steps"][step]
        for x in r[1:]:
            assert x["steps"][step]["grads"] == a["grads"] and x["steps"][step]["buckets"] == a["buckets"] >= 2
        # mean over the eight ranks of (rank + 1 + s/4 + i%7) = 4.5 + s/4 + i%7: exact in bf16
        assert abs((a["first"] % 1.0) - (0.5 + 0.25 * step) % 1.0) < 1e-6, a["first"]
    for x in r:
        assert x["gathered"] and all(g[0][0] == world * B and g[1][0] == world * B and g[2][0] == world * B and g[3][0] == world * B
                                     for g in x["gathered"]), x["gathered"][:1]


@pytest.mark.timeout(900)
def test_two_rank_step_in_the_benchmarked_mode(tmp_path):
    """The data-parallel step as bench.py --gpus 2 runs it: precision f16mix (fp16-product forward of the video blocks' Linears -- two
    products in the first quarter of the tower, one behind it --, single-pass backward) at a token count where the 12 SpaceTimeBlocks and the 6 DistilBERT layers go through their one-call-per-
    direction C entry points (B = 8, T = 4 per rank: M = 6 280), buckets leaving from the polls inside the block backward calls."""
    world = 2
    mp.spawn(_worker, args=(world, 29711, str(tmp_path), "direct", False, 8, ("f16mix",), 4), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt"), weights_only=False) for i in range(world)]
    assert r[0]["w0"] == r[1]["w0"]
    for step in range(2):
        a, b = r[0]["steps"][step], r[1]["steps"][step]
        assert a["grads"] == b["grads"] and a["buckets"] == b["buckets"] >= 5
        for x in (a, b):
            # the first step builds the f16x2 weight planes one by one at first use; from then on ONE multi-encode per step refreshes them
            assert x["blocks"] == 12 and x["text_layers"] == 6 and x["x2_refresh"] == (1 if step else 0)
            assert x["during"] >= x["buckets"] - 1, x
            assert x["gemm_calls"] == 2 + 2 * 3            # patch embedding (forward + wgrad) and the two heads: everything else is inside the calls


@pytest.mark.timeout(900)
def test_eight_ranks_at_unequal_host_speeds_issue_the_same_collectives_in_the_same_order(tmp_path):
    """Round-5 verdict, next 9: the one N > 1 failure mode a CPU test can still catch before multi-GPU hardware exists.  World size 8,
    hook-free direct exchange, every rank stalling for a different, changing time at every poll of backward (a fast rank launches its
    buckets while a slow one is still blocks behind): every rank must log the SAME sequence of collectives (kind and payload size) --
    a data-dependent or pace-dependent launch order would pair an all-to-all with an all-gather and hang (timeout) or, worse, match the
    wrong buckets -- and end with bit-identical gradients."""
    world, B = 8, 4
    mp.spawn(_worker, args=(world, 29723, str(tmp_path), "direct", True, B, ("bf16x3", "bf16"), 2, True), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt"), weights_only=False) for i in range(world)]
    ref = r[0]["collectives"]
    kinds = {k for k, _ in ref}
    assert {"all_to_all_single", "all_gather_into_tensor", "broadcast"} <= kinds and len(ref) >= 2 * (1 + 2 * r[0]["steps"][0]["buckets"])
    for i, x in enumerate(r[1:], 1):
        assert x["collectives"] == ref, (i, [(a, b) for a, b in zip(x["collectives"], ref) if a != b][:3])
    for step in range(2):
        a = r[0]["steps"][step]
        assert all(x["steps"][step]["grads"] == a["grads"] for x in r[1:])
        assert abs((a["first"] % 1.0) - (0.5 + 0.25 * step) % 1.0) < 1e-6, a["first"]
