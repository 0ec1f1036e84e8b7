"""The multi-tensor launches at their table and chunk boundaries, on a real MI355X (`pytest -m gpu`): egv_adamw_multi (with its bf16
plane refresh and device-side hyper block), egv_grad_nonfinite_multi, egv_loss_scale_update and the optimizer around them,
egv_grad_pack_bf16 / egv_grad_unpack_bf16, egv_split_f32_multi, egv_f16x2_encode_multi and egv_splitk_reduce_multi -- each against a
plain reference of the same operation (tests/multi_tensor_ref.py), element by element, with sentinel guards around every tensor.

Bounds.  AdamW: |p - p_ref| <= k u s_i, u = 2^-24, k = 13 fp32 roundings on the way to p without weight decay, 16 with it, 4 for m,
6 for v -- counted operation by operation from adamw_kernel in the docstring of tests/multi_tensor_ref.py, where the first-order
error analysis that shows the counts suffice is written out.  Split-k reduce: (ks - 1) u sum_z |partial_z| (ks - 1 additions).
Everything else is bit-exact.

Table sizes and CHUNK come from multi_tensor_ref (tests/test_multi_tensor_cpu.py checks them against the .hip sources)."""
import ctypes as C

import numpy as np
import pytest
import torch

import multi_tensor_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, (B1, B2), EPS = R.ADAMW_LR, R.ADAMW_BETAS, R.ADAMW_EPS
BIG = 65536 + 4096 + 4


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


def _h():
    from egovlp_amd import _lib
    return _lib.lib()


def _vp(vals):
    return (C.c_void_p * len(vals))(*vals)


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _i32(vals):
    return (C.c_int32 * len(vals))(*vals)


def _stream(ops):
    return ops._stream()


_WORST = {"p": 0.0, "m": 0.0, "v": 0.0}


def _note(ratios, what):
    for k, r in zip("pmv", ratios):
        _WORST[k] = max(_WORST[k], r)
    print("%s: largest err / (u s): p %.2f m %.2f v %.2f   (all AdamW cases so far: p %.2f m %.2f v %.2f)" % (
        what, ratios[0], ratios[1], ratios[2], _WORST["p"], _WORST["m"], _WORST["v"]))


def _adamw_arenas(numels, plan, tensors):
    """{stream: Arena on the device} for p, g, m, v."""
    return {s: R.Arena([(n, plan[s][i]) for i, n in enumerate(numels)]).fill(ts).to(DEV) for s, ts in zip("pgmv", tensors)}


def _adamw_call(ops, ar, numels, lr, wd, step, cb, gs, hyper=None, w_hi=None, w_lo=None):
    rc = _h().egv_adamw_multi(len(numels), _vp(ar["p"].ptrs()), _vp(ar["g"].ptrs()), _vp(ar["m"].ptrs()), _vp(ar["v"].ptrs()),
                              _vp(w_hi) if w_hi is not None else None, _vp(w_lo) if w_lo is not None else None, _i64(numels),
                              float(lr), B1, B2, EPS, float(wd), int(step), int(cb), float(gs),
                              hyper.data_ptr() if hyper is not None else None, _stream(ops))
    torch.cuda.synchronize()
    return rc


def _adamw_check(ar, numels, before, wd, step, cb, gs, what, lr=LR, step_size=None):
    """Every tensor of the arenas against adamw_ref64 of its fp32 inputs, element-wise; guards; g untouched.  -> p after (CPU)."""
    from egovlp_amd.optim import adamw_step_size
    ps, gs_, ms, vs = before
    got_p, got_g, got_m, got_v = (ar[s].tensors_cpu() for s in "pgmv")
    ss = step_size if step_size is not None else R.f32(adamw_step_size(R.f32(lr), R.f32(B1), R.f32(B2), step, bool(cb)))
    worst = [0.0, 0.0, 0.0]
    for i, n in enumerate(numels):
        ref = R.adamw_ref64(ps[i], gs_[i], ms[i], vs[i], lr, B1, B2, EPS, wd, step, cb, gs, step_size=step_size)
        r = R.check_adamw((got_p[i], got_m[i], got_v[i]), ref, ps[i], wd, ss, "%s tensor %d (numel %d, misaligned %s)" % (
            what, i, n, [ar[s].offsets[i] % 4 for s in "pgmv"]))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert torch.equal(got_g[i].view(torch.int32), gs_[i].view(torch.int32)), (what, i, "the gradient is read-only")
    for s in "pgmv":
        ar[s].assert_guards("%s stream %s" % (what, s))
    _note(worst, what)
    return got_p


# ------------------------------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("case", R.adamw_cases(), ids=[c[0] for c in R.adamw_cases()])
def test_adamw_multi(ops, case):
    """1 / T-1 / T / T+1 / 2T+1 non-empty tensors (T = 48) of every size around the 16384-element chunk, zero-numel entries interleaved,
    each of the four streams misaligned on its own: every element of p, m, v within k u s of the fp64 reference (k = 13 / 16, 4, 6 fp32
    roundings; tests/multi_tensor_ref.py), every guard element intact.  The test prints the largest err / (u s) of every case and of all cases so far
    (the fp32 CPU oracle reaches p 3.55, m 1.93, v 1.98 on the same inputs: tests/test_multi_tensor_cpu.py)."""
    cid, count, wd, cb, step, gs, seed = case
    numels, plan = R.adamw_case_layout(count, seed)
    before = R.adamw_inputs(numels, step, gs, seed)
    ar = _adamw_arenas(numels, plan, before)
    assert _adamw_call(ops, ar, numels, LR, wd, step, cb, gs) == 0
    _adamw_check(ar, numels, before, wd, step, cb, gs, cid)


@pytest.mark.parametrize("n,stream", [(5, "p"), (16385, "g"), (BIG, "m"), (BIG, "v"), (16388, "p"), (1024, None), (3, None)])
def test_adamw_one_tensor_one_stream_misaligned(ops, n, stream):
    """count = 1: the sizes on both sides of a chunk with exactly one of p / g / m / v one element behind a 16-byte boundary."""
    numels = [n]
    plan = {s: [1 if s == stream else 0] for s in "pgmv"}
    before = R.adamw_inputs(numels, 1000, 1.0, 40 + n % 7)
    ar = _adamw_arenas(numels, plan, before)
    assert _adamw_call(ops, ar, numels, LR, 0.01, 1000, 1, 1.0) == 0
    _adamw_check(ar, numels, before, 0.01, 1000, 1, 1.0, "one tensor n=%d misaligned %s" % (n, stream))


def _plane_case(seed):
    numels = [0, 4, 5, 1024, 0, 16384, 16385, 16388, 2 * 16384 + 4, 1023, 65536, 3, BIG, 16384, 1024, 8]
    plan = R.misalign_plan(numels, "pgmv", seed)
    for s in "pgmv":                                   # the fp32 streams of the plane cases below stay aligned unless said otherwise
        plan[s] = [0] * len(numels)
    plan["g"][6] = 2
    # which planes an entry has: b = both, h = hi only, l = lo only, - = none; and how far each plane sits behind an 8-byte boundary
    kinds = ["-", "b", "b", "b", "b", "b", "b", "h", "l", "b", "-", "b", "b", "b", "h", "b"]
    mis_hi = [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 2, 0]
    mis_lo = [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 2]
    return numels, plan, kinds, mis_hi, mis_lo


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_refreshes_the_bf16_planes(ops, wd):
    """w_hi / w_lo of egv_adamw_multi (NULL through ops.adamw_multi): after the step the planes are split_bf16(p_after) bit for bit, on
    the 16-byte path (everything aligned, numel % 4 == 0) and on the scalar path (odd sizes, a misaligned gradient, a plane that is
    2-byte but not 8-byte aligned), with planes given for only some entries; entries without a plane and all guards stay untouched."""
    numels, plan, kinds, mis_hi, mis_lo = _plane_case(9)
    before = R.adamw_inputs(numels, 1000, 1.0, 9)
    ar = _adamw_arenas(numels, plan, before)
    hi = R.Arena([(n if k in "bh" else 0, mh) for n, k, mh in zip(numels, kinds, mis_hi)], dtype=torch.bfloat16).to(DEV)
    lo = R.Arena([(n if k in "bl" else 0, ml) for n, k, ml in zip(numels, kinds, mis_lo)], dtype=torch.bfloat16).to(DEV)
    w_hi = [v.data_ptr() if (k in "bh" and n) else None for v, k, n in zip(hi.views, kinds, numels)]
    w_lo = [v.data_ptr() if (k in "bl" and n) else None for v, k, n in zip(lo.views, kinds, numels)]
    assert any(p is not None and p % 8 == 2 for p in w_hi) and any(p is not None and p % 8 == 6 for p in w_hi)
    assert _adamw_call(ops, ar, numels, LR, wd, 1000, 1, 1.0, w_hi=w_hi, w_lo=w_lo) == 0
    p_after = _adamw_check(ar, numels, before, wd, 1000, 1, 1.0, "planes wd=%g" % wd)
    hi.assert_guards("w_hi")
    lo.assert_guards("w_lo")
    got_hi, got_lo = hi.tensors_cpu(), lo.tensors_cpu()
    for i, (n, k) in enumerate(zip(numels, kinds)):
        want_hi, want_lo = R.split_bf16_ref(p_after[i])
        if k in "bh":
            assert torch.equal(got_hi[i].view(torch.int16), want_hi.view(torch.int16)), ("w_hi", i, n)
        if k in "bl":
            assert torch.equal(got_lo[i].view(torch.int16), want_lo.view(torch.int16)), ("w_lo", i, n)
    # planes for ALL entries of a table that flushes (T + 1 tensors), everything on the 16-byte path
    T = R.TABLE["adamw"]
    numels = [16388 if i == T - 1 else (BIG if i == T else 4 * (1 + i % 300)) for i in range(T + 1)]
    plan = {s: [0] * len(numels) for s in "pgmv"}
    before = R.adamw_inputs(numels, 1, 1.0, 10)
    ar = _adamw_arenas(numels, plan, before)
    hi = R.Arena([(n, 0) for n in numels], dtype=torch.bfloat16).to(DEV)
    lo = R.Arena([(n, 0) for n in numels], dtype=torch.bfloat16).to(DEV)
    assert _adamw_call(ops, ar, numels, LR, wd, 1, 1, 1.0, w_hi=hi.ptrs(), w_lo=lo.ptrs()) == 0
    p_after = _adamw_check(ar, numels, before, wd, 1, 1, 1.0, "planes, T + 1 tensors, wd=%g" % wd)
    hi.assert_guards("w_hi")
    lo.assert_guards("w_lo")
    for i, (a, b) in enumerate(zip(hi.tensors_cpu(), lo.tensors_cpu())):
        want_hi, want_lo = R.split_bf16_ref(p_after[i])
        assert torch.equal(a.view(torch.int16), want_hi.view(torch.int16)) and torch.equal(b.view(torch.int16), want_lo.view(torch.int16)), i


def test_adamw_hyper_block_skips_or_overrides(ops):
    """hyper_dev = {lr, step_size, 1 / S, skip}.  skip = 1: parameters, moments and planes bit-identical to before the call.  skip = 0:
    the device values win over the host arguments (which are deliberately different: another lr, another step, another scale)."""
    T = R.TABLE["adamw"]
    numels = R.layout_sizes(T + 1, T, 77)
    plan = R.misalign_plan(numels, "pgmv", 77)
    S = 512.0
    before = R.adamw_inputs(numels, 1000, 1.0 / S, 77)
    ar = _adamw_arenas(numels, plan, before)
    hi = R.Arena([(n, 0) for n in numels], dtype=torch.bfloat16).to(DEV)
    lo = R.Arena([(n, 0) for n in numels], dtype=torch.bfloat16).to(DEV)
    w_hi = [p if n else None for p, n in zip(hi.ptrs(), numels)]
    w_lo = [p if n else None for p, n in zip(lo.ptrs(), numels)]
    snaps = {s: ar[s].snapshot() for s in "pgmv"}
    snap_hi, snap_lo = hi.snapshot(), lo.snapshot()
    lr_d, ss_d = R.f32(3e-3), R.f32(2.5e-3)
    hyper = torch.tensor([lr_d, ss_d, 1.0 / S, 1.0], dtype=torch.float32, device=DEV)
    assert _adamw_call(ops, ar, numels, 7e-3, 0.01, 3, 1, 1.0, hyper=hyper, w_hi=w_hi, w_lo=w_lo) == 0
    for s in "pgmv":
        assert torch.equal(ar[s].bits, snaps[s]), ("skipped step wrote stream", s)
    assert torch.equal(hi.bits, snap_hi) and torch.equal(lo.bits, snap_lo)
    hyper[3] = 0.0
    assert _adamw_call(ops, ar, numels, 7e-3, 0.01, 3, 1, 1.0, hyper=hyper, w_hi=w_hi, w_lo=w_lo) == 0
    # the reference runs on the DEVICE values; with the host's (lr 7e-3, step 3, scale 1) every element would be far outside the bound
    p_after = _adamw_check(ar, numels, before, 0.01, 1000, 1, 1.0 / S, "hyper block", lr=lr_d, step_size=ss_d)
    big = max(range(len(numels)), key=lambda i: numels[i])
    host = R.adamw_ref64(before[0][big], before[1][big], before[2][big], before[3][big], 7e-3, B1, B2, EPS, 0.01, 3, 1, 1.0)
    assert float((p_after[big].double() - host[0]).abs().max()) > 1e-4           # nothing like what the host arguments describe
    for i, (a, b) in enumerate(zip(hi.tensors_cpu(), lo.tensors_cpu())):
        want_hi, want_lo = R.split_bf16_ref(p_after[i])
        assert torch.equal(a.view(torch.int16), want_hi.view(torch.int16)) and torch.equal(b.view(torch.int16), want_lo.view(torch.int16)), i


# ------------------------------------------------------------------------------------------------------------------------- the scan
NONFINITE = {"+inf": 0x7F800000, "-inf": 0xFF800000, "quiet NaN": 0x7FC00000, "NaN, payload 1": 0x7F800001}
STATE0 = [0x44800000, 2, 0, 5, 0x3C23D70A, 0x3B03126F, 0x3A800000, 0]      # S = 1024, 2 good, flag, 5 skipped, a hyper block


def _s32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


def _scan(ops, arena, numels, state):
    rc = _h().egv_grad_nonfinite_multi(len(numels), _vp(arena.ptrs()), _i64(numels), state.data_ptr(), _stream(ops))
    assert rc == 0
    return state.cpu().tolist()


def _scan_list(idx, n_target, total=193):
    """`total` non-empty tensors (two flushes of the 96-entry table and one more), small ones everywhere but at `idx`; zero-numel
    entries in front, in the middle and at the flush.  -> (numels, position of the target in that list)."""
    numels, where = [], None
    for i in range(total):
        if i in (0, 95, 96, 97, 150):
            numels.append(0)
        if i == idx:
            where = len(numels)
            numels.append(n_target)
        else:
            numels.append(R.SMALL_SIZES[i % len(R.SMALL_SIZES)] if i % 11 else 4100)
    return numels, where


@pytest.mark.parametrize("idx", [0, 95, 96, 97, 191, 192])
def test_nonfinite_scan_finds_one_value_anywhere(ops, idx):
    """One +inf / -inf / quiet NaN / NaN with payload 1 in otherwise finite data, in tensor `idx` of 193 (the table holds 96): at the
    first and last element, on both sides of the scan's block edge (4 x CHUNK = 65536), inside the 4x-unrolled main loop and in the
    single-step remainder behind it (16-byte path), at the last element of a numel % 4 != 0 tensor (scalar path), and in a tensor one
    to three elements behind a 16-byte boundary.  Every case sets state[2] and leaves the other seven words alone."""
    gen = torch.Generator().manual_seed(idx)
    variants = [("16-byte path", BIG, 0, [0, BIG - 1, 65535, 65536, 12345, 40000 + 3 * 1024 + 2, 65536 + 4096 + 1, 65536 + 1024 + 5]),
                ("scalar path", 65537, 0, [0, 65536, 65535, 777]),
                ("scalar path, numel 16383", 16383, 0, [16382, 0]),
                ("misaligned", BIG, 1 + idx % 3, [0, BIG - 1, 65535, 65536])]
    state0 = torch.tensor([_s32(w) for w in STATE0], dtype=torch.int32)
    n_cases = 0
    for name, n, mis, positions in variants:
        numels, where = _scan_list(idx, n)
        arena = R.Arena([(m, mis if i == where else 0) for i, m in enumerate(numels)])
        arena.fill([torch.randn(m, generator=gen) for m in numels]).to(DEV)
        state = state0.to(DEV)
        assert _scan(ops, arena, numels, state) == state0.tolist(), (name, "finite data set the flag")
        target = arena.views[where].view(torch.int32)
        for pos in positions:
            for vname, bits in NONFINITE.items():
                keep = int(target[pos])
                target[pos] = _s32(bits)
                state.copy_(state0)
                got = _scan(ops, arena, numels, state)
                want = list(state0.tolist())
                want[2] = 1
                assert got == want, (name, "tensor %d" % idx, "position %d of %d" % (pos, n), vname, got)
                target[pos] = keep
                n_cases += 1
        assert _scan(ops, arena, numels, state0.to(DEV)) == state0.tolist()          # restored: finite again
        arena.assert_guards(name)
    assert n_cases == 4 * (8 + 4 + 2 + 4)


def test_nonfinite_scan_leaves_finite_data_alone(ops):
    """FLT_MAX, the smallest denormal, -0.0 and ordinary values: the flag stays 0 -- also for sizes whose 4x-unrolled loop ends exactly
    at the tensor's end (the guards behind every tensor are NaNs: a scan that reads one element too far sets the flag).  A flag that
    is already 1 stays 1."""
    gen = torch.Generator().manual_seed(3)
    sizes = R.layout_sizes(2 * R.TABLE["nonfinite"] + 1, R.TABLE["nonfinite"], 3)
    # (end - base) mod 4096 in [3072, 4092]: some lane's next unrolled step would start exactly at `end`
    sizes += [3072, 4096 + 3072, 3072 + 20, 65536 + 3072, 3 * 4096 + 4092, 16384 + 3072 + 1024, 0, 3072 + 512]
    specials = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38, 1.4e-45, -1.4e-45, -0.0, 0.0, 1.17549435e-38])
    data = []
    for n in sizes:
        t = torch.randn(n, generator=gen)
        if n:
            k = min(n, specials.numel())
            t[:k] = specials[:k]
            t[n - k:] = specials[:k]
        data.append(t)
    plan = R.misalign_plan(sizes, "g", 3)["g"]
    arena = R.Arena([(n, plan[i] if n < 3072 or n > 20000 else 0) for i, n in enumerate(sizes)]).fill(data).to(DEV)
    state0 = torch.tensor([_s32(w) for w in STATE0], dtype=torch.int32)
    assert _scan(ops, arena, sizes, state0.to(DEV)) == state0.tolist()
    set1 = state0.clone()
    set1[2] = 1
    assert _scan(ops, arena, sizes, set1.to(DEV)) == set1.tolist()
    arena.assert_guards("finite scan")
    ops.grad_nonfinite_multi([v for v in arena.views if v.numel()], (st := state0.to(DEV)))          # the wrapper, same answer
    assert st.cpu().tolist() == state0.tolist()


# ------------------------------------------------------------------------------------------------------------------------- loss scale
@pytest.mark.parametrize("growth,backoff,init,max_scale", [(2.0, 0.125, 16.0, 64.0), (1.7, 0.3, 10.0, 55.5)])
def test_loss_scale_update_follows_the_reference_for_240_steps(ops, growth, backoff, init, max_scale):
    """Random overflow draws, growth interval 3, a max_scale that is hit and a backoff deep enough for the floor of 1: after EVERY step S,
    the good-step count and the skipped count equal loss_scale_ref exactly, the hyper block is {lr, step size, 1 / S of this step,
    skip} with the step size within 2 ulp of float(adamw_step_size(lr, b1, b2, step - skipped)) (the device evaluates pow in double; its
    last bit is the runtime's).  A second, non-advancing call for another parameter group changes nothing but the block it writes."""
    rng = np.random.RandomState(12)
    lr, lr2 = 1e-2, 3e-3
    host = torch.zeros(8, dtype=torch.int32)
    host.view(torch.float32)[0] = init
    host.view(torch.float32)[6] = 1.0 / init
    state = host.to(DEV)
    extra = torch.zeros(4, dtype=torch.float32, device=DEV)
    ref = {"scale": np.float32(init), "good": 0, "skipped": 0, "inv": np.float32(1.0) / np.float32(init), "skip": 0.0}
    seen = set()
    for step in range(1, 241):
        overflow = bool(rng.rand() < (0.6 if 100 <= step < 112 else 0.1))
        cb = 0 if step % 17 == 0 else 1
        state[2] = int(overflow)
        ops.loss_scale_update(state, None, lr, B1, B2, step, cb, growth, backoff, 3, max_scale, advance=1)
        ref, hyper = R.loss_scale_ref(ref, overflow, lr, B1, B2, step, cb, growth, backoff, 3, max_scale)
        got = state.cpu()
        gf = got.view(torch.float32)
        assert float(gf[0]) == float(ref["scale"]) and int(got[1]) == ref["good"] and int(got[3]) == ref["skipped"], (step, got.tolist(), ref)
        assert int(got[2]) == 0                                                     # cleared for the next scan
        assert float(gf[4]) == hyper[0] and float(gf[6]) == hyper[2] and float(gf[7]) == hyper[3], (step, gf.tolist(), hyper)
        assert R.ulp_distance_f32(float(gf[5]), hyper[1]) <= 2, (step, float(gf[5]), hyper[1])
        ops.loss_scale_update(state, extra, lr2, B1, B2, step, 1, growth, backoff, 3, max_scale, advance=0)
        same, hyper2 = R.loss_scale_ref(ref, overflow, lr2, B1, B2, step, 1, growth, backoff, 3, max_scale, advance=0)
        assert same == ref and torch.equal(state.cpu(), got), (step, "a non-advancing call changed the state")
        ex = extra.cpu().tolist()
        assert ex[0] == hyper2[0] and ex[2] == hyper2[2] and ex[3] == hyper2[3] and R.ulp_distance_f32(ex[1], hyper2[1]) <= 2, (step, ex, hyper2)
        if float(ref["scale"]) == np.float32(max_scale):
            seen.add("max")
        if float(ref["scale"]) == 1.0:
            seen.add("floor")
        if step - ref["skipped"] < 1:
            seen.add("clamp")
    assert {"max", "floor"} <= seen, seen
    # advance = 0 with the default hyper block (state + 4): only words 4..7 may change
    before = state.cpu()
    ops.loss_scale_update(state, None, lr2, B1, B2, 240, 0, growth, backoff, 3, max_scale, advance=0)
    after = state.cpu()
    assert torch.equal(after[:4], before[:4]) and float(after.view(torch.float32)[4]) == R.f32(lr2) and float(after.view(torch.float32)[5]) == R.f32(lr2)
    assert torch.equal(after[6:], before[6:])


def test_optimizer_with_two_parameter_groups_under_one_scaler(ops):
    """egovlp_amd.optim.AdamW, two groups (lr 1e-2 / wd 0 and lr 3e-3 / wd 0.01), one LossScaler, 12 steps with overflows at steps 3, 4
    (two in a row, the inf in the SECOND group's last tensor's last element) and 8 (a NaN in the first group): the second group's
    hyper block carries its own lr / step size and the shared 1 / S / skip; every applied step moves every element of both groups to
    within k u s of adamw_ref64 of the state before it, un-scaled by 1 / S, bias correction at the number of APPLIED steps; a skipped
    step leaves parameters and moments of both groups bit-identical."""
    from egovlp_amd.optim import AdamW, LossScaler, adamw_step_size
    gen = torch.Generator().manual_seed(21)
    shapes = [[(16385,), (33, 5), (1024,)], [(65537,), (3,), (128, 130)]]
    groups_cpu = [R.adamw_inputs([int(np.prod(s)) for s in g], 1, 1.0, 50 + i)[0] for i, g in enumerate(shapes)]
    params = [[torch.nn.Parameter(p.reshape(s).to(DEV)) for p, s in zip(ps, g)] for ps, g in zip(groups_cpu, shapes)]
    hp = [{"lr": 1e-2, "weight_decay": 0.0}, {"lr": 3e-3, "weight_decay": 0.01}]
    opt = AdamW([dict(params=params[0], **hp[0]), dict(params=params[1], **hp[1])])
    sc = LossScaler(init_scale=1024.0, growth_interval=3, max_scale=4096.0)
    state_ref = {"scale": np.float32(1024.0), "good": 0, "skipped": 0, "inv": np.float32(1.0 / 1024), "skip": 0.0}
    for step in range(1, 13):
        S = float(state_ref["scale"])
        assert sc.get_scale() == S
        overflow = step in (3, 4, 8)
        grads = [[torch.randn(p.shape, generator=gen) for p in g] for g in params]
        for g, gg in zip(params, grads):
            for p, gr in zip(g, gg):
                p.grad = (gr * S).to(DEV)
        if step in (3, 4):
            params[1][2].grad[-1, -1] = float("inf")
        if step == 8:
            params[0][0].grad[16384] = float("nan")
        before = [[(p.detach().cpu().clone(), opt.state[p]["exp_avg"].cpu().clone() if p in opt.state and "exp_avg" in opt.state[p] else torch.zeros(p.shape),
                    opt.state[p]["exp_avg_sq"].cpu().clone() if p in opt.state and "exp_avg_sq" in opt.state[p] else torch.zeros(p.shape))
                   for p in g] for g in params]
        opt.step(scaler=sc)
        torch.cuda.synchronize()
        state_ref, _ = R.loss_scale_ref(state_ref, overflow, hp[0]["lr"], B1, B2, step, 1, 2.0, 0.5, 3, 4096.0)
        t = max(step - state_ref["skipped"], 1)
        assert sc.get_scale() == float(state_ref["scale"]) and sc.skipped_steps() == state_ref["skipped"]
        for gi in range(2):
            blk = sc.hyper_block(gi).cpu().tolist()
            want_ss = adamw_step_size(R.f32(hp[gi]["lr"]), R.f32(B1), R.f32(B2), t)
            assert blk[0] == R.f32(hp[gi]["lr"]) and blk[2] == 1.0 / S and blk[3] == float(overflow), (step, gi, blk)
            assert R.ulp_distance_f32(blk[1], want_ss) <= 2, (step, gi, blk[1], want_ss)
            for p, gr, (p0, m0, v0) in zip(params[gi], grads[gi], before[gi]):
                st = opt.state[p]
                if overflow:
                    assert torch.equal(p.detach().cpu().view(torch.int32), p0.view(torch.int32)), (step, gi, "a skipped step moved a parameter")
                    assert torch.equal(st["exp_avg"].cpu(), m0) and torch.equal(st["exp_avg_sq"].cpu(), v0), (step, gi, "a skipped step moved a moment")
                    continue
                gscaled = (gr * S).reshape(-1)
                ref = R.adamw_ref64(p0.reshape(-1), gscaled, m0.reshape(-1), v0.reshape(-1), hp[gi]["lr"], B1, B2, EPS, hp[gi]["weight_decay"],
                                    t, 1, 1.0 / S, step_size=blk[1])
                r = R.check_adamw((p.detach().cpu().reshape(-1), st["exp_avg"].cpu().reshape(-1), st["exp_avg_sq"].cpu().reshape(-1)), ref,
                                  p0.reshape(-1), hp[gi]["weight_decay"], blk[1], "step %d group %d %s" % (step, gi, tuple(p.shape)))
                _note(r, "optimizer step %d group %d %s" % (step, gi, tuple(p.shape)))
    assert sc.skipped_steps() == 3


# ------------------------------------------------------------------------------------------------------------------------- pack / unpack
SPECIALS = [float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1.4e-45, -1.4e-45, 1e-40, -0.0, 0.0,
            1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 3 * 2.0 ** -8)]


def _pack_layout(numels, seed):
    """Offsets into the flat bf16 buffer: at least 8 elements of padding between tensors; multiples of 8 (the 16-byte path) for most,
    odd or 2 mod 4 for every fifth (the scalar path).  -> (offsets, total)."""
    offs, cur = [], 8
    for i, n in enumerate(numels):
        start = (cur + 7) // 8 * 8
        if i % 5 == 3:
            start += 1 + 2 * (i % 2) if i % 10 == 3 else 2
        offs.append(start)
        cur = start + n + 8
    return offs, (cur + 7) // 8 * 8


@pytest.mark.parametrize("count", [95, 96, 97, 193])
@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0])
def test_grad_pack_and_unpack_bf16(ops, count, scale):
    """egv_grad_pack_bf16 is bit-exact against (g * scale).to(bf16) -- +-inf, +-FLT_MAX (-> inf at scale 1), denormals, -0.0 and ties
    included; a NaN stays a NaN -- and egv_grad_unpack_bf16 against the 16-bit shift, for 95 / 96 / 97 / 193 tensors (the table holds
    96) of sizes straddling CHUNK, misaligned fp32 views, flat offsets on the 16-byte and on the scalar path.  The padding of the flat
    buffer and the guards of the fp32 side stay untouched."""
    T = R.TABLE["gradsync"]
    numels = R.layout_sizes(count, T, count)
    plan = R.misalign_plan(numels, "g", count)["g"]
    gen = torch.Generator().manual_seed(count)
    data = []
    for i, n in enumerate(numels):
        t = torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-3, 3, (1,), generator=gen)))
        k = min(n, len(SPECIALS))
        if n and i % 3 == 0:
            t[n - k:] = torch.tensor(SPECIALS[:k])
        data.append(t)
    src = R.Arena([(n, plan[i]) for i, n in enumerate(numels)]).fill(data).to(DEV)
    offs, total = _pack_layout(numels, count)
    sent = R.SENTINEL[torch.bfloat16]
    flat = torch.full((total,), sent, dtype=torch.int16, device=DEV)
    assert _h().egv_grad_pack_bf16(len(numels), _vp(src.ptrs()), _i64(numels), flat.data_ptr(), _i64(offs), float(scale), _stream(ops)) == 0
    torch.cuda.synchronize()
    want = torch.full((total,), sent, dtype=torch.int16)
    for t, o in zip(data, offs):
        want[o:o + t.numel()] = (t * np.float32(scale)).to(torch.bfloat16).view(torch.int16)
    got = flat.cpu()
    nan_w = torch.isnan(want.view(torch.bfloat16).float())
    nan_g = torch.isnan(got.view(torch.bfloat16).float())
    assert torch.equal(nan_w, nan_g), "NaN positions (the padding's NaN sentinel included)"
    diff = (got != want) & ~nan_w
    assert not bool(diff.any()), ("pack", torch.nonzero(diff).reshape(-1)[:8].tolist())
    inside = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(offs, numels):
        inside[o:o + n] = True
    assert bool((got[~inside] == sent).all()), "padding of the flat buffer overwritten"
    if scale == 1.0:
        i = next(j for j, n in enumerate(numels) if n >= len(SPECIALS) and j % 3 == 0)
        tail = got[offs[i] + numels[i] - len(SPECIALS):offs[i] + numels[i]].view(torch.bfloat16).float()
        assert bool(torch.isinf(tail[3])) and bool(torch.isinf(tail[4])) and float(tail[4]) < 0          # FLT_MAX rounds to inf
        assert float(tail[5]) == 0.0 and float(tail[8]) == 0.0 and bool(torch.signbit(tail[8]))         # the smallest denormal vanishes, -0.0 keeps its sign
    src.assert_guards("pack source")
    assert torch.equal(torch.cat([t.view(torch.int32) for t in src.tensors_cpu()]), torch.cat([t.view(torch.int32) for t in data]))
    # --- unpack: arbitrary bf16 bit patterns (NaN payloads included) -> fp32 = bits << 16, exactly
    bits = torch.randint(-32768, 32768, (total,), generator=gen, dtype=torch.int32).to(torch.int16)
    flat2 = bits.to(DEV)
    dst = R.Arena([(n, plan[i]) for i, n in enumerate(numels)]).to(DEV)
    assert _h().egv_grad_unpack_bf16(len(numels), _vp(dst.ptrs()), _i64(numels), flat2.data_ptr(), _i64(offs), _stream(ops)) == 0
    torch.cuda.synchronize()
    for i, (t, o, n) in enumerate(zip(dst.tensors_cpu(), offs, numels)):
        assert torch.equal(t.view(torch.int32), bits[o:o + n].to(torch.int32) << 16), ("unpack", i, n)
    dst.assert_guards("unpack destination")
    assert torch.equal(flat2.cpu(), bits)


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("kind", ["one inf", "+inf and -inf"])
def test_exchange_keeps_a_nonfinite_gradient_nonfinite(ops, world, kind):
    """The simulated-rank exchange of tests/test_gpu_gradsync.py (pack with 1 / W, slice sum in fp32, unpack): one rank holds an inf in
    one element -- or one rank +inf and another -inf, whose sum is a NaN.  After the exchange that element is non-finite on the
    receiving side and egv_grad_nonfinite_multi, which runs behind the exchange, sets the flag; without the inf it does not."""
    from egovlp_amd.dist import _hip_pack, _hip_slice_sum, _hip_unpack
    shapes = [(2304,), (1000, 33), (17,), (16385,), (4096,)]
    numels = [int(np.prod(s)) for s in shapes]
    offs, off = [], 0
    for n in numels:
        offs.append(off)
        off += (n + 7) // 8 * 8
    q = 8 * world
    total = (off + q - 1) // q * q
    slice_elems = total // world
    gen = torch.Generator().manual_seed(world)
    hits = [(1, 32999), (3, 16384), (2, 16)]             # (tensor, element): 16-byte path, scalar path behind a chunk, a tiny tensor
    for poisoned in (False, True):
        for ti, ei in (hits if poisoned else hits[:1]):
            ranks = [[torch.randn(s, generator=gen) for s in shapes] for _ in range(world)]
            if poisoned:
                ranks[world - 1][ti].reshape(-1)[ei] = float("inf")
                if kind == "+inf and -inf":
                    ranks[0][ti].reshape(-1)[ei] = float("-inf")
            flats = []
            for p in range(world):
                flat = torch.zeros(total, dtype=torch.bfloat16, device=DEV)
                _hip_pack([t.to(DEV) for t in ranks[p]], flat, offs, 1.0 / world)
                flats.append(flat)
            red = torch.empty(total, dtype=torch.bfloat16, device=DEV)
            for r in range(world):
                recv = torch.cat([flats[p][r * slice_elems:(r + 1) * slice_elems] for p in range(world)]).contiguous()
                out = torch.empty(slice_elems, dtype=torch.bfloat16, device=DEV)
                _hip_slice_sum(recv, world, slice_elems, out)
                red[r * slice_elems:(r + 1) * slice_elems] = out
            outs = [torch.zeros(s, device=DEV) for s in shapes]
            _hip_unpack(outs, red, offs)
            state = torch.zeros(8, dtype=torch.int32, device=DEV)
            ops.grad_nonfinite_multi(outs, state)
            torch.cuda.synchronize()
            finite = [bool(torch.isfinite(o).all()) for o in outs]
            if poisoned:
                assert not bool(torch.isfinite(outs[ti].reshape(-1)[ei])), (world, kind, ti, ei, float(outs[ti].reshape(-1)[ei]))
                assert int(torch.isfinite(outs[ti]).logical_not().sum()) == 1 and all(f for j, f in enumerate(finite) if j != ti)
                assert state.cpu().tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
            else:
                assert all(finite) and state.cpu().tolist() == [0] * 8


# ------------------------------------------------------------------------------------------------------------------------- formats
def _matrix_shapes(count, mult):
    """Distinct small shapes, several 64 x 64 tiles in either direction for some; cols % mult == 0."""
    return [(1 + (37 * i) % 150, mult * (1 + (11 * i) % 21)) for i in range(count)]


@pytest.mark.parametrize("count", [39, 40, 41, 81])
def test_split_f32_multi_equals_the_one_tensor_entry_point(ops, count):
    """egv_split_f32_multi (table of 40) for T-1 / T / T+1 / 2T+1 matrices of distinct shapes -- row-major planes, transposed planes
    with their zero pad, or both per entry -- against egv_split_f32 on the same matrix, bit for bit, every output (those on both sides
    of the flush included)."""
    gen = torch.Generator().manual_seed(count)
    jobs, outs = [], []
    garbage = R.SENTINEL[torch.bfloat16]
    for i, (r, c) in enumerate(_matrix_shapes(count, 4)):
        x = (torch.randn(r, c, generator=gen) * 3).to(DEV)
        want_rm, want_t = i % 3 != 1, i % 3 != 0
        hi = torch.full((r, c), garbage, dtype=torch.int16, device=DEV).view(torch.bfloat16) if want_rm else None
        lo = torch.full((r, c), garbage, dtype=torch.int16, device=DEV).view(torch.bfloat16) if want_rm else None
        ldt = ops.pad32(r)
        thi = torch.full((c, ldt), garbage, dtype=torch.int16, device=DEV).view(torch.bfloat16) if want_t else None
        tlo = torch.full((c, ldt), garbage, dtype=torch.int16, device=DEV).view(torch.bfloat16) if want_t else None
        jobs.append((x, ops._p(hi), ops._p(lo), c, ops._p(thi), ops._p(tlo), ldt, ldt))
        outs.append((x, hi, lo, thi, tlo))
    ops.split_f32_multi(jobs)
    torch.cuda.synchronize()
    for i, (x, hi, lo, thi, tlo) in enumerate(outs):
        rp, rt, _ = ops.split_f32(x, 3, want_rowmajor=hi is not None, want_transposed=thi is not None)
        for got, want, name in ((hi, rp.hi if rp else None, "hi"), (lo, rp.lo if rp else None, "lo"), (thi, rt.hi if rt else None, "t_hi"),
                                (tlo, rt.lo if rt else None, "t_lo")):
            if got is not None:
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (i, tuple(x.shape), name)
        if thi is not None and x.shape[0] % 32:
            assert bool((thi[:, x.shape[0]:].float() == 0).all())            # the zero pad behind the last source row


@pytest.mark.parametrize("count", [47, 48, 49, 97])
def test_f16x2_encode_multi_equals_the_one_tensor_entry_point(ops, count):
    """egv_f16x2_encode_multi (table of 48, second-operand role) for T-1 / T / T+1 / 2T+1 matrices against egv_f16x2_encode."""
    gen = torch.Generator().manual_seed(count)
    jobs, outs = [], []
    garbage = R.SENTINEL[torch.float16]
    for r, c in _matrix_shapes(count, 8):
        x = (torch.randn(r, c, generator=gen) * 2).to(DEV)
        p1 = torch.full((r, c), garbage, dtype=torch.int16, device=DEV)
        p2 = torch.full((r, c), garbage, dtype=torch.int16, device=DEV)
        jobs.append((x, p1.data_ptr(), p2.data_ptr(), c))
        outs.append((x, p1, p2))
    ops.f16x2_encode_multi(jobs)
    torch.cuda.synchronize()
    for i, (x, p1, p2) in enumerate(outs):
        ref = ops.f16x2_encode(x, 1)
        assert torch.equal(p1, ref.hi.view(torch.int16)) and torch.equal(p2, ref.lo.view(torch.int16)), (i, tuple(x.shape))


# ------------------------------------------------------------------------------------------------------------------------- split-k reduce
def _reduce_case(entries, seed):
    """entries: (mn, ksplit, m or 0).  The partial buffer of an entry is its ksplit product slabs, then its ksplit column-sum slabs."""
    gen = torch.Generator().manual_seed(seed)
    partial = [(torch.randn(ks * (mn + m), generator=gen) * 10.0 ** float(torch.randint(-2, 3, (1,), generator=gen))).to(DEV) for mn, ks, m in entries]
    out = R.Arena([(mn, 0) for mn, _, _ in entries]).to(DEV)
    cs = R.Arena([(m, 0) for _, _, m in entries]).to(DEV)
    return partial, out, cs


def _reduce_call(ops, entries, partial, out, cs, count=None):
    n = len(entries) if count is None else count
    colsum = [p if m else None for p, (_, _, m) in zip(cs.ptrs(), entries)]
    rc = _h().egv_splitk_reduce_multi(n, _vp([p.data_ptr() for p in partial]), _vp(out.ptrs()), _i64([e[0] for e in entries]),
                                      _i32([e[1] for e in entries]), _vp(colsum), _i32([e[2] for e in entries]), _stream(ops))
    torch.cuda.synchronize()
    return rc


REDUCE_ENTRIES = [(3 * 1024 + 4, 2, 0), (20 * 1028, 7, 8), (4, 28, 2052), (5000, 28, 0), (1024, 2, 1024), (7 * 1024 + 12, 7, 1028),
                  (8, 2, 4), (2 * 1024 + 1020, 28, 0)]


@pytest.mark.parametrize("count", [1, 2, 8])
def test_splitk_reduce_multi(ops, count):
    """egv_splitk_reduce_multi for 1 / 2 / 8 entries (its table holds 8): mn not a multiple of the 1024 elements a block covers,
    ksplit 2 / 7 / 28, column sums for some entries only with m below and above 1024.  Every element within (ks - 1) u sum_z
    |partial_z| of the fp64 sum (ks - 1 fp32 additions), guards behind every out and colsum intact, a colsum that was not asked for
    untouched."""
    entries = REDUCE_ENTRIES[:count] if count != 2 else [REDUCE_ENTRIES[2], REDUCE_ENTRIES[5]]
    partial, out, cs = _reduce_case(entries, count)
    assert _reduce_call(ops, entries, partial, out, cs) == 0
    outs, css = out.tensors_cpu(), cs.tensors_cpu()
    for i, (mn, ks, m) in enumerate(entries):
        p = partial[i].cpu().double()
        for name, got, slab in (("out", outs[i], p[:ks * mn].reshape(ks, mn)), ("colsum", css[i], p[ks * mn:].reshape(ks, m))):
            if slab.numel() == 0:
                continue
            err = (got.double() - slab.sum(0)).abs()
            bound = (ks - 1) * R.U * slab.abs().sum(0)
            assert bool((err <= bound).all()), (name, i, mn, ks, m, int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max()))
    out.assert_guards("out")
    cs.assert_guards("colsum")


def test_splitk_reduce_multi_rejects_what_it_cannot_hold(ops):
    """9 entries (the table holds 8) and ksplit = 1 return EGV_ERR_ARG before anything is launched: the outputs keep their bits."""
    entries = REDUCE_ENTRIES + [(1024, 2, 0)]
    partial, out, cs = _reduce_case(entries, 99)
    snap_o, snap_c = out.snapshot(), cs.snapshot()
    assert _reduce_call(ops, entries, partial, out, cs) == 1
    bad = [(1024, 1, 0)]
    assert _reduce_call(ops, bad, partial[-1:], out, cs) == 1
    mixed = [REDUCE_ENTRIES[0], (1024, 1, 0)]
    assert _reduce_call(ops, mixed, [partial[0], partial[-1]], out, cs) == 1
    assert _reduce_call(ops, entries, partial, out, cs, count=0) == 1
    assert torch.equal(out.bits, snap_o) and torch.equal(cs.bits, snap_c)


# ------------------------------------------------------------------------------------------------------------------------- validation
def _bad_adamw(ops):
    n = R.TABLE["adamw"] + 1
    numels = [4] * n
    ar = _adamw_arenas(numels, {s: [0] * n for s in "pgmv"}, R.adamw_inputs(numels, 1000, 1.0, 5))
    g = ar["g"].ptrs()
    g[-1] = None
    outs = [ar[s] for s in "pmv"]
    call = lambda: _h().egv_adamw_multi(n, _vp(ar["p"].ptrs()), _vp(g), _vp(ar["m"].ptrs()), _vp(ar["v"].ptrs()), None, None, _i64(numels),
                                        LR, B1, B2, EPS, 0.01, 1000, 1, 1.0, None, _stream(ops))
    return [call], outs


def _bad_nonfinite(ops):
    n = R.TABLE["nonfinite"] + 1
    data = [torch.ones(4) for _ in range(n)]
    data[0][1] = float("inf")
    arena = R.Arena([(4, 0)] * n).fill(data).to(DEV)
    g = arena.ptrs()
    g[-1] = None
    state = torch.zeros(8, dtype=torch.int32, device=DEV)
    call = lambda: _h().egv_grad_nonfinite_multi(n, _vp(g), _i64([4] * n), state.data_ptr(), _stream(ops))
    return [call], [state]


def _bad_pack_unpack(ops):
    n = R.TABLE["gradsync"] + 1
    gen = torch.Generator().manual_seed(6)
    src = R.Arena([(4, 0)] * n).fill([torch.randn(4, generator=gen) for _ in range(n)]).to(DEV)
    dst = R.Arena([(4, 0)] * n).to(DEV)
    offs = [8 * i for i in range(n - 1)] + [-1]
    flat = torch.full((8 * n,), R.SENTINEL[torch.bfloat16], dtype=torch.int16, device=DEV)
    pack = lambda: _h().egv_grad_pack_bf16(n, _vp(src.ptrs()), _i64([4] * n), flat.data_ptr(), _i64(offs), 1.0, _stream(ops))
    unpack = lambda: _h().egv_grad_unpack_bf16(n, _vp(dst.ptrs()), _i64([4] * n), flat.data_ptr(), _i64(offs), _stream(ops))
    return [pack, unpack], [flat, dst]


def _bad_split(ops):
    n = R.TABLE["split"] + 1
    x = torch.randn(n, 4, 8, generator=torch.Generator().manual_seed(7)).to(DEV)
    hi, lo = (R.Arena([(32, 0)] * n, dtype=torch.bfloat16).to(DEV) for _ in range(2))
    cols = [8] * (n - 1) + [6]
    null, zero = _vp([None] * n), _i64([0] * n)
    call = lambda: _h().egv_split_f32_multi(n, _vp([x[i].data_ptr() for i in range(n)]), _i64([8] * n), _i32([4] * n), _i32(cols),
                                            _vp(hi.ptrs()), _vp(lo.ptrs()), _i64([8] * n), null, null, zero, _i32([0] * n), _stream(ops))
    return [call], [hi, lo]


def _bad_encode(ops):
    n = R.TABLE["f16x2"] + 1
    x = torch.randn(n, 4, 8, generator=torch.Generator().manual_seed(8)).to(DEV)
    p1, p2 = (R.Arena([(32, 0)] * n, dtype=torch.float16).to(DEV) for _ in range(2))
    cols = [8] * (n - 1) + [4]
    call = lambda: _h().egv_f16x2_encode_multi(n, _vp([x[i].data_ptr() for i in range(n)]), _i64([8] * n), _i32([4] * n), _i32(cols),
                                               _vp(p1.ptrs()), _vp(p2.ptrs()), _i64([8] * n), 1, _stream(ops))
    return [call], [p1, p2]


BAD_ITEM = {"egv_adamw_multi": _bad_adamw, "egv_grad_nonfinite_multi": _bad_nonfinite, "egv_grad_pack_bf16-egv_grad_unpack_bf16": _bad_pack_unpack,
            "egv_split_f32_multi": _bad_split, "egv_f16x2_encode_multi": _bad_encode}


@pytest.mark.parametrize("entry", list(BAD_ITEM))
def test_invalid_item_behind_the_first_table_enqueues_nothing(ops, entry):
    """One full table of valid items (4 to 32 elements each) and, directly behind it, an item the host refuses -- a NULL gradient,
    a NULL tensor of 4 elements, a flat offset of -1, cols = 6 (not a multiple of 4), cols = 4 (not a multiple of 8): the call
    returns 1 and, after a synchronize, every output -- p / m / v, the scaler's state (its found-inf word stays 0 although tensor 0
    holds an inf), the flat buffer and the fp32 destinations, the planes -- has the bits it had before, guards included: the
    first table was not launched."""
    calls, outs = BAD_ITEM[entry](ops)
    bits = lambda o: o.bits if isinstance(o, R.Arena) else o
    before = [bits(o).clone() for o in outs]
    torch.cuda.synchronize()
    for call in calls:
        assert call() == 1
    torch.cuda.synchronize()
    for i, (o, b) in enumerate(zip(outs, before)):
        assert torch.equal(bits(o), b), (entry, "output %d was written" % i)
