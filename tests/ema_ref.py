"""Plain references for the weight-average kernels (csrc/ema.hip): CPU only, no HIP.  Shared by tests/test_ema_cpu.py (the references
judged on their own) and tests/test_gpu_ema.py (the kernels against them); the case generator lives here so that the CPU test sees the
very inputs the GPU test hands to the kernel.

The bound.  With u = 2^-24 every fp32 operation returns exact * (1 + d), |d| <= u.  The kernel computes e' = fmaf(w, p - e, e): one
rounding on p - e and one on the fused multiply-add, two in all; the un-fused form e + w * (p - e) has three.  Each acts on a term
bounded by s = |e| + w |p - e| (|e'| <= s as well), so |got - ref| <= 3 u s covers either form to first order.  The bound allows
three roundings; it is not a measurement."""
import ctypes

import numpy as np
import torch

import multi_tensor_ref as R

U = 2.0 ** -24
K_EMA = 3
CHUNK = R.CHUNK
TABLE = 120                     # tensors per launch (EMA_MAX_T, csrc/ema.hip)
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK + 7]
WEIGHTS = [1.0 - 0.9999, 0.9, 1.0]


def f32(x):
    return float(np.float32(x))


def ema_ref64(e, p, w):
    """e + w (p - e) in fp64 on the fp32-rounded w."""
    e, p = e.detach().double().cpu(), p.detach().double().cpu()
    return e + f32(w) * (p - e)


def ema_scale(e, p, w):
    e, p = e.detach().double().cpu(), p.detach().double().cpu()
    return e.abs() + f32(w) * (p - e).abs()


def ema_ratio(got, ref, e, p, w):
    """The largest err / (u s) (0 where both are 0)."""
    err = (got.detach().double().cpu() - ref).abs()
    s = ema_scale(e, p, w)
    ratio = torch.where(s > 0, err / (U * s), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def check_ema(got, ref, e, p, w, what="", k=K_EMA):
    """Element-wise |got - ref| <= k u s, s = |e| + w |p - e| (k = 3 unless a test composes several updates) -> the largest ratio."""
    err = (got.detach().double().cpu() - ref).abs()
    s = ema_scale(e, p, w)
    bad = ~(err <= k * U * s)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError("%s: [%d of %d]: got %r, reference %r, |err| %.3e = %.2f u s (allowed %d); %d elements out of bound" % (
            what, i, err.numel(), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(err.reshape(-1)[i]),
            float(err.reshape(-1)[i] / (U * s.reshape(-1)[i])), k, int(bad.sum())))
    return ema_ratio(got, ref, e, p, w)


def decay_ref(decay, warmup, t):
    """The rule of egv_ema_decide in Python doubles -> (decay in effect, w), each rounded to fp32 as the device stores them."""
    d = float(ctypes.c_float(decay).value)
    if warmup:
        d = min(d, (1.0 + t) / (10.0 + t))
    return ctypes.c_float(d).value, ctypes.c_float(1.0 - d).value


def decide_ref(state, skip, decay, warmup):
    """One call of egv_ema_decide on state = dict(t, w, skipped, decay) -> the new state."""
    new = dict(state)
    if skip:
        new["w"] = 0.0
        new["skipped"] = state["skipped"] + 1
        return new
    new["decay"], new["w"] = decay_ref(decay, warmup, state["t"])
    new["t"] = state["t"] + 1
    return new


# ---------------------------------------------------------------------------------------------------------------------------- cases
def boundary_specs():
    """(numel, misalign) of the boundary list: every size of SIZES 16-byte aligned, then a view one element into its storage (the scalar
    path: more than one block, and a short one) and an empty tensor in the middle."""
    specs = [(n, 0) for n in SIZES]
    specs.insert(4, (0, 0))
    return specs + [(CHUNK + 1030, 1), (5, 1), (4 * 300 + 3, 0)]


def count_specs(count, seed):
    """`count` non-empty tensors around the table's flush boundaries (multi_tensor_ref.layout_sizes: a tensor that straddles chunks
    right behind every flush, zero-numel entries interleaved), some of them misaligned in one or both streams."""
    numels = R.layout_sizes(count, TABLE, seed, first_sizes=R.SMALL_SIZES)
    plan = R.misalign_plan(numels, "ep", seed)
    return numels, plan


def case_specs(which):
    """-> (specs of the shadow stream, specs of the parameter stream)."""
    if which == "boundaries":
        specs = boundary_specs()
        return specs, list(specs)
    count = {"table": TABLE, "table+1": TABLE + 1, "2*table+1": 2 * TABLE + 1}[which]
    numels, plan = count_specs(count, 7 + count)
    return [(n, m) for n, m in zip(numels, plan["e"])], [(n, m) for n, m in zip(numels, plan["p"])]


CASES = ["boundaries", "table", "table+1", "2*table+1"]


def case_inputs(which, seed=11):
    """fp32 CPU (e list, p list) of a case: N(0, 1) shadows, parameters a small step away from them plus a few far ones."""
    es_specs, _ = case_specs(which)
    g = torch.Generator().manual_seed(seed)
    es, ps = [], []
    for n, _ in es_specs:
        e = torch.randn(n, generator=g)
        p = e + 1e-3 * torch.randn(n, generator=g)
        far = torch.rand(n, generator=g) < 0.1
        p = torch.where(far, torch.randn(n, generator=g) * 4.0, p)
        es.append(e)
        ps.append(p)
    return es, ps
