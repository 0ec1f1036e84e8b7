"""Host side of the embedding-cache step (`egoclip_step_cached`, egovlp_amd/trainer/cached_step.py) on CPU tensors over the do-nothing
C-ABI stand-in (tests/mock_hip.py): which entry points a step calls and how often, that the gradient exchange is held until the last
chunk's backward has returned (two real gloo ranks), argument checks, and the trainer's switch.  Nothing about values: those are
tests/test_gpu_cached_step.py."""
import collections
import os
import sys
import time
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mock_hip import mock_hip

HERE = os.path.dirname(os.path.abspath(__file__))

TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}


def _tiny():
    from egovlp_amd.model.model import FrozenInTime
    return FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="").train()


def _batch(B, rank=0):
    from egovlp_amd.synth import synth_batch
    b = synth_batch(B, T=2, L=16, seed=3, rank=rank, res=32)
    return {"video": b["video"], "text": b["text"], "noun_vec": b["noun_vec"], "verb_vec": b["verb_vec"]}


# forward-only entry points of the two towers' blocks on the per-kernel path (the toy geometry): two attention calls per video block
# forward, one per text layer forward
FWD_ENTRIES = ("egv_divided_attn_fwd", "egv_text_attn_fwd", "egv_patch_gather", "egv_embed_fwd")


def test_call_sequence_of_a_cached_step():
    """B = 6 in chunks of 2: ONE loss-head call for the whole batch, every chunk encoded twice (the forward entries of the blocks run
    2 x 3 times what one plain step at B = 2 runs them), K - 1 = 2 accumulate calls, the optimizer entries once."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step, egoclip_step_cached
    torch.manual_seed(0)
    model = _tiny()
    opt = AdamW(model.parameters(), lr=3e-5)
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        egoclip_step(model, EgoNCE(), opt, _batch(2), 1, 0)              # builds the weight-plane cache
        calls.clear()
        egoclip_step(model, EgoNCE(), opt, _batch(2), 1, 0)
        plain = collections.Counter(calls)
        calls.clear()
        drop0 = model.text_model._drop_calls
        loss = egoclip_step_cached(model, EgoNCE(), opt, _batch(6), 2, 1, 0, check_replay=True)
        c = collections.Counter(calls)
        order = list(calls)
    assert loss.shape == () and not loss.requires_grad
    assert plain["egv_egonce_fwd_bwd"] == 1 and c["egv_egonce_fwd_bwd"] == 1
    assert c["egv_sim_matrix_fwd"] == 0 and c["egv_egonce_from_sim"] == 0
    for name in FWD_ENTRIES:
        assert plain[name] > 0 and c[name] == 2 * plain[name] * 3, (name, plain[name], c[name])
    assert plain["egv_divided_attn_fwd"] == 2 * 2 and plain["egv_text_attn_fwd"] == 2
    # backward entries: once per chunk
    assert c["egv_divided_attn_bwd"] == 3 * plain["egv_divided_attn_bwd"] and c["egv_text_attn_bwd"] == 3 * plain["egv_text_attn_bwd"]
    assert plain["egv_grad_accumulate_multi"] == 0 and c["egv_grad_accumulate_multi"] == 2
    assert c["egv_adamw_multi"] == plain["egv_adamw_multi"] >= 1
    # the head sits between the two passes: half of the forwards before it, and no backward entry before it
    head = order.index("egv_egonce_fwd_bwd")
    assert order[:head].count("egv_divided_attn_fwd") == c["egv_divided_attn_fwd"] // 2 and "egv_divided_attn_bwd" not in order[:head]
    # an accumulate follows the 2nd and the 3rd chunk's backward, the optimizer comes last
    acc = [i for i, n in enumerate(order) if n == "egv_grad_accumulate_multi"]
    bwd = [i for i, n in enumerate(order) if n == "egv_divided_attn_bwd"]
    per = len(bwd) // 3
    assert bwd[2 * per - 1] < acc[0] < bwd[2 * per] and bwd[-1] < acc[1] < order.index("egv_adamw_multi")
    # every parameter ends the step with a gradient of its own shape; the dropout counter advanced once per chunk, not twice
    assert all(p.grad is not None and p.grad.shape == p.shape for p in model.parameters())
    assert model.text_model._drop_calls == drop0 + 3
    assert model.last_replay_max_abs_diff.shape == ()


def test_single_chunk_and_ragged_chunks():
    """chunk >= B is one chunk (no accumulate call); B = 5 in chunks of 2 is chunks of 2, 2 and 1."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    torch.manual_seed(0)
    model = _tiny()
    opt = AdamW(model.parameters(), lr=3e-5)
    seen = []
    hook = model.register_forward_pre_hook(lambda mod, args: seen.append((args[0]["video"].shape[0], args[0]["text"]["input_ids"].shape[0],
                                                                          torch.is_grad_enabled())))
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        egoclip_step_cached(model, EgoNCE(), opt, _batch(4), 8)
        assert calls.count("egv_grad_accumulate_multi") == 0 and calls.count("egv_egonce_fwd_bwd") == 1
        assert seen == [(4, 4, False), (4, 4, True)]
        del seen[:]
        calls.clear()
        egoclip_step_cached(model, EgoNCE(), opt, _batch(5), 2)
        assert calls.count("egv_grad_accumulate_multi") == 2 and calls.count("egv_egonce_fwd_bwd") == 1
    hook.remove()
    assert seen == [(2, 2, False), (2, 2, False), (1, 1, False), (2, 2, True), (2, 2, True), (1, 1, True)]


def test_train_kernels_run_in_the_cache_pass():
    """Pass 1 runs under no_grad but must run the kernels of a forward that is back-propagated.  The `train` flag of a block / layer
    forward is "some input needs a gradient": with trainable parameters that holds under no_grad too, but a FROZEN block is train in
    pass 2 (its input carries a gradient) and would not be in pass 1 -- the cache pass asks for the train kernels explicitly."""
    from egovlp_amd import ops
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.cached_step import egoclip_step_cached
    torch.manual_seed(0)
    model = _tiny()
    for mod in (model.video_model.blocks[1], model.text_model.transformer.layer[1]):
        for p in mod.parameters():
            p.requires_grad_(False)
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=3e-5)
    ec = model.exec_ctx
    flags = []
    orig = ops.ExecContext.forward_is_train

    def spy(self, ctx):
        out = orig(self, ctx)
        flags.append((torch.is_grad_enabled(), any(ctx.needs_input_grad), out))
        return out
    ops.ExecContext.forward_is_train = spy
    try:
        with mock_hip():
            ec.set_precision("bf16x3", "bf16")
            egoclip_step_cached(model, EgoNCE(), opt, _batch(4), 2)
            with torch.no_grad():
                model(_batch(2))
    finally:
        ops.ExecContext.forward_is_train = orig
    n = 2 + 2                                     # per forward: video block 0, 1 (frozen), text layer 0, 1 (frozen)
    cached, replay, plain_eval = flags[:2 * n], flags[2 * n:4 * n], flags[4 * n:]
    assert len(plain_eval) == n
    assert all(f[2] for f in cached) and all(f[2] for f in replay)                     # train kernels in both passes
    assert [f[1] for f in cached] == [True, False, True, False] * 2                    # ... although nothing asks the frozen ones for a gradient
    assert all(f[1] for f in replay)
    assert [f[2] for f in plain_eval] == [True, False, True, False]                    # an ordinary no_grad forward is unchanged
    assert not ec._train_kernels
    assert all((p.grad is not None) == p.requires_grad for p in model.parameters())


def test_arguments():
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step_cached
    model = _tiny()
    opt = AdamW(model.parameters(), lr=3e-5)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            egoclip_step_cached(model, EgoNCE(), opt, _batch(2), bad)


def test_accumulate_wrapper_checks_its_arguments():
    from egovlp_amd import ops
    with mock_hip() as calls:
        ops.grad_accumulate_multi([], [])
        assert calls == []                         # count = 0: not even a call
        a, b = torch.zeros(5), torch.ones(5)
        ops.grad_accumulate_multi([a, a[1:]], [b, b[1:]])
        assert calls == ["egv_grad_accumulate_multi"]
        with pytest.raises(ValueError):
            ops.grad_accumulate_multi([a], [b, b])
        with pytest.raises(ValueError):
            ops.grad_accumulate_multi([a], [b[:4]])
        with pytest.raises(ValueError):
            ops.grad_accumulate_multi([a], [b.double()])
        with pytest.raises(ValueError):
            ops.grad_accumulate_multi([torch.zeros(4, 4).t()], [torch.zeros(4, 4)])


def test_trainer_switches_on_embed_cache_chunk():
    """Multi_Trainer_dist._step: args.embed_cache_chunk > 0 takes the cached step with that chunk and the precision guard is handed the
    first chunk; without it the path is the plain step's."""
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import Multi_Trainer_dist
    torch.manual_seed(0)
    model = _tiny()
    tr = Multi_Trainer_dist.__new__(Multi_Trainer_dist)
    tr.args = types.SimpleNamespace(world_size=1, rank=0, embed_cache_chunk=2)
    tr.model, tr.loss, tr.optimizer, tr.n_gpu, tr.grad_sync = model, EgoNCE(), AdamW(model.parameters(), lr=3e-5), 1, None
    data = _batch(6)
    assert tr._guard_batch(data)["video"].shape[0] == 2
    with mock_hip() as calls:
        model.exec_ctx.set_precision("bf16x3", "bf16")
        tr._step(data)
        assert calls.count("egv_grad_accumulate_multi") == 2 and calls.count("egv_egonce_fwd_bwd") == 1
        calls.clear()
        tr.args.embed_cache_chunk = 0
        assert tr._guard_batch(data) is data
        tr._step(data)
        assert calls.count("egv_grad_accumulate_multi") == 0 and calls.count("egv_egonce_fwd_bwd") == 1
        del tr.args.embed_cache_chunk
        assert tr._guard_batch(data) is data


# ---------------------------------------------------------------------------------------------------------------- two gloo ranks
def _pack(grads, flat, offsets, scale):
    for g, o in zip(grads, offsets):
        flat[o:o + g.numel()] = (g.reshape(-1) * scale).to(torch.bfloat16)


def _unpack(grads, flat, offsets):
    for g, o in zip(grads, offsets):
        g.copy_(flat[o:o + g.numel()].float().view_as(g))


def _slice_sum(recv, world, slice_elems, out):
    out.copy_(recv.view(world, slice_elems).float().sum(0).to(torch.bfloat16))


def _digest(tensors):
    import hashlib
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _worker(rank, world, port, out, B, chunk):
    for p in (HERE, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from egovlp_amd.dist import Bf16GradSync
    from egovlp_amd.model.loss import EgoNCE
    from egovlp_amd.optim import AdamW
    from egovlp_amd.trainer.trainer_egoclip import egoclip_step_cached
    log = []                                              # collectives (op, payload elements) and "backward returned" marks, in order
    for _name in ("all_to_all_single", "all_gather_into_tensor", "all_reduce", "broadcast"):
        def _wrap(fn, _name=_name):
            def logged(*a, **k):
                log.append((_name, int(a[0].numel())))
                return fn(*a, **k)
            return logged
        setattr(dist, _name, _wrap(getattr(dist, _name)))
    _bw = torch.autograd.backward

    def backward(*a, **k):
        r = _bw(*a, **k)
        log.append(("backward_returned", 0))
        return r
    torch.autograd.backward = backward
    torch.manual_seed(100 + rank)
    model = _tiny()
    model.text_model.seed_rank = rank
    ec = model.exec_ctx
    sync = Bf16GradSync(model.parameters(), use_hooks=False, order_hint=model.gradient_ready_order(), exec_ctx=ec, exchange="direct",
                        pack_fn=_pack, unpack_fn=_unpack, slice_sum_fn=_slice_sum, bucket_mb=1.0)
    ec.set(backward_poll=sync.poll, gemm_grid=248)
    ec.set_precision("bf16x3", "bf16")
    opt = AdamW(model.parameters(), lr=3e-5)
    data = _batch(B, rank=rank)
    steps = []
    with mock_hip() as calls:
        for step in range(2):
            calls.clear()
            log.append(("step", step))

            def pack(grads, flat, offsets, scale, _step=step):       # the kernels are stand-ins: give every rank different, finite gradients
                for i, g in enumerate(grads):
                    g.copy_(torch.full_like(g, float(rank + 1) + 0.25 * _step + (i % 7)))
                _pack(grads, flat, offsets, scale)
            sync.pack_fn = pack
            egoclip_step_cached(model, EgoNCE(), opt, data, chunk, world, rank, grad_sync=sync)
            steps.append({"during": sync.stats["launched_during_backward"], "buckets": sync.stats["buckets"],
                          "grads": _digest(p.grad for p in model.parameters()), "accumulate": calls.count("egv_grad_accumulate_multi"),
                          "head": calls.count("egv_egonce_fwd_bwd"), "adamw": calls.count("egv_adamw_multi")})
    width = 2 * 256 + data["noun_vec"].shape[1] + data["verb_vec"].shape[1]
    torch.save({"steps": steps, "log": log, "embed_elems": world * B * width}, os.path.join(out, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _spawn(fn, args, nprocs, seconds):
    """mp.spawn with a deadline of its own: ranks that stop pairing their collectives hang, they do not fail."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.time() + seconds
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish in %d s (collectives out of step?)" % seconds)


@pytest.mark.timeout(600)
def test_two_ranks_hold_the_exchange_until_the_last_chunk(tmp_path):
    world, B, chunk = 2, 6, 2
    K = 3
    _spawn(_worker, (world, 29741, str(tmp_path), B, chunk), world, 480)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt"), weights_only=False) for i in range(world)]
    assert r[0]["log"] == r[1]["log"]                                   # the same collectives (and backward marks) in the same order
    embed = ("all_gather_into_tensor", r[0]["embed_elems"])
    log = r[0]["log"]
    for step in range(2):
        lo = log.index(("step", step))
        hi = log.index(("step", step + 1)) if step == 0 else len(log)
        seg = log[lo + 1:hi]
        assert seg.count(embed) == 1                                    # ONE embedding gather per step
        marks = [i for i, e in enumerate(seg) if e[0] == "backward_returned"]
        assert len(marks) == 1 + K                                      # the head's backward, then one per chunk
        assert seg.index(embed) < marks[0]
        exchange = [i for i, e in enumerate(seg) if e[0] in ("all_to_all_single", "all_reduce") or (e[0] == "all_gather_into_tensor" and e != embed)]
        assert exchange and min(exchange) > marks[-1], (marks, exchange[:3])    # nothing leaves before the last chunk's backward returned
        a, b = r[0]["steps"][step], r[1]["steps"][step]
        assert a["grads"] == b["grads"]                                 # bit-identical gradients on both ranks after finish()
        for x in (a, b):
            assert x["during"] == 0 and x["buckets"] >= 2
            assert seg.count(("all_to_all_single", seg[exchange[0]][1])) >= 1 and sum(e[0] == "all_to_all_single" for e in seg) == x["buckets"]
            assert x["accumulate"] == K - 1 and x["head"] == 1 and x["adamw"] >= 1


def test_hold_blocks_poll_and_finish_refuses_inside_it():
    """Bf16GradSync.hold(): poll() launches nothing inside (every gradient present), finish() inside is an error, finish() after it
    launches every bucket; without hold() poll() launches as before."""
    from egovlp_amd.dist import Bf16GradSync
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", "29747"
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        ps = [torch.nn.Parameter(torch.zeros(8)), torch.nn.Parameter(torch.zeros(3, 3))]
        sync = Bf16GradSync(ps, use_hooks=False, pack_fn=_pack, unpack_fn=_unpack, slice_sum_fn=_slice_sum, exchange="allreduce")
        for p in ps:
            p.grad = torch.ones_like(p)
        with sync.hold():
            sync.poll()
            assert sync.stats["collectives_last_step"] == 0
            with pytest.raises(RuntimeError):
                sync.finish()
        st = sync.finish()
        assert st["collectives_last_step"] == st["buckets"] >= 1 and st["launched_during_backward"] == 0
        sync.poll()
        assert sync.stats["collectives_last_step"] == st["buckets"]      # behaviour without hold() is unchanged
        sync.finish()
        # hook mode: two backward passes inside a hold fire every hook twice and launch nothing; finish() sends every bucket on the sums
        qs = [torch.nn.Parameter(torch.ones(8)), torch.nn.Parameter(torch.ones(3, 3))]
        hooked = Bf16GradSync(qs, use_hooks=True, pack_fn=_pack, unpack_fn=_unpack, slice_sum_fn=_slice_sum, exchange="allreduce")

        def backward():
            (qs[0].sum() * 2.0 + qs[1].sum() * 3.0).backward()
        backward()
        hooked.finish()                                                  # first step: observes the ready order, builds the buckets
        for q in qs:
            q.grad = None
        with hooked.hold():
            backward()
            backward()
            assert hooked.stats["collectives_last_step"] == 0
        st = hooked.finish()
        assert st["collectives_last_step"] == st["buckets"] >= 1 and st["launched_during_backward"] == 0
        assert torch.equal(qs[0].grad, torch.full((8,), 4.0)) and torch.equal(qs[1].grad, torch.full((3, 3), 6.0))
        for q in qs:
            q.grad = None
        backward()                                                       # without a hold the hooks launch as before
        assert hooked.stats["collectives_last_step"] == st["buckets"]
        hooked.finish()
        hooked.remove_hooks()
    finally:
        dist.destroy_process_group()
