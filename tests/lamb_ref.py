"""The LAMB rule of egovlp_amd.optim.LAMB (csrc/lamb.hip) restated in fp64: CPU only, no HIP.  No LAMB implementation is installed next
to this project (neither timm nor apex), so this file IS the oracle: tests/test_lamb_cpu.py judges it on its own, tests/test_gpu_lamb.py
judges the kernels against it.  The case generators live here so that both see the same inputs.

The rule, for one tensor p with gradient g, moments m, v and the group's lr, (b1, b2), eps, wd:

    g' = g * grad_scale                        grad_scale = (1 / S) * coef: loss scale and global-norm clip, as in AdamW
    m  = b1 m + (1 - b1) g'
    v  = b2 v + (1 - b2) g'^2
    c  = sqrt(1 - b2^t) / (1 - b1^t)           t = steps actually APPLIED; 1 when correct_bias is False
    u  = c * m / (sqrt(v) + eps) + wd * p      eps OUTSIDE the correction: per unit lr, the direction of this project's AdamW
    r  = ||p|| / ||u||  if adapt and ||p|| > 0 and ||u|| > 0 else 1        adapt = (wd != 0 or always_adapt)
    r  = min(r, 1)      if trust_clip
    p  = p - lr * r * u

timm's Lamb and apex's FusedLAMB correct m and v separately, which puts eps inside the correction; that is the one deviation.

The bounds (u = 2^-24: every fp32 operation returns exact * (1 + d), |d| <= u; derived, not measured).

Moments: the expressions are adamw_kernel's, so the counts of tests/multi_tensor_ref.py hold: |err m| <= 4 u s_m, s_m = |m b1| +
|(1 - b1) g'|; |err v| <= 6 u v.

Norms.  A block of stage 1 reduces at most 16 384 squares: a lane adds at most 64 of them into one accumulator on the scalar path
(16 into each of four on the 16-byte path), each add one rounding (the square is fused into it); the four accumulators are combined
(2 adds deep), the wave's butterfly has 6 levels, the four waves are added 2 deep.  Every term is >= 0, so a partial is off by at most
(64 + 2 + 6 + 2) u = 74 u relative (N_ADD); grad_sqnorm_kernel, with 65 536 elements per block, has 264 u = 1.6e-5.  The partials of a
tensor are added in double (nothing at this scale), and the square root halves the bound: 37 u on each norm.  The ratio of the two
norms gets the sum: RHO = 74 u = 4.4e-6.

Parameter, element-wise, with D = lr r u:   |err p| <= K_P u (|p| + |D|) + RHO |D|.
Roundings on the way to p, as the kernel is written: g' (1); m (3); v (4, halved by the root); sqrtf (1); + eps (1); the division (1);
c = step_size / lr on the device (2: the rounding of step_size, the division); c * (...) (1); fmaf(wd, p, ...) (1); r stored as fp32
(1); lr * r (1); the last fmaf (1): 18.  The three roundings of m act on s_m, which exceeds |m| only through cancellation, by at most
2 (1 - b1) |g'|, while sqrt(v) >= sqrt(1 - b2) |g'|: that excess adds at most 6 u c (1 - b1) / sqrt(1 - b2) = 19 u c to u whatever the
data (the same term as in the AdamW bound), 19 u c lr r to p.  It vanishes when the old moments are zero (nothing to cancel with);
otherwise check_lamb asserts 19 c lr r <= 2 min(|p| + |D|), which makes it worth at most 2 more roundings.  K_P = 18 + 2 = 20."""
import math

import numpy as np
import torch

import multi_tensor_ref as R

U = 2.0 ** -24
CHUNK = R.CHUNK
TABLE = 48                      # tensors per launch of the two element-wise stages (LAMB_MAX_T, csrc/lamb.hip)
RATIO_TABLE = 192               # tensors per launch of the ratio kernel (LAMB_RATIO_MAX_T)
N_ADD = 64 + 2 + 6 + 2          # fp32 additions on the longest path of one partial
RHO = N_ADD * U                 # on a ratio: N_ADD u / 2 from each of the two norms
K_P, K_M, K_V = 20, R.K_M, R.K_V
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK + 7]
LR, BETAS, EPS, WD = 1e-2, (0.9, 0.999), 1e-6, 0.01

f32 = R.f32


def correction(beta1, beta2, t, correct_bias=True):
    """c at t applied steps, in double on the fp32 betas (what the C entry points compute)."""
    if not correct_bias:
        return 1.0
    b1, b2 = f32(beta1), f32(beta2)
    return math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def trust_ratio(p_norm, u_norm, adapt, trust_clip):
    r = p_norm / u_norm if (adapt and p_norm > 0.0 and u_norm > 0.0) else 1.0
    return min(r, 1.0) if trust_clip else r


def lamb_ref64(ps, gs, ms, vs, lr, betas, eps, weight_decay, c, grad_scale=1.0, always_adapt=False, trust_clip=False):
    """The rule above on lists of fp32 tensors, in fp64; the scalars are the fp32 values the kernels receive, c is given (correction()).
    -> dict of per-tensor lists: p, m, v (new values), r, u, delta = lr r u, s_m, p_norm, u_norm."""
    lr, b1, b2, eps, wd, gsc = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(weight_decay), f32(grad_scale)
    one_m_b1, one_m_b2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    adapt = wd != 0.0 or bool(always_adapt)
    out = {k: [] for k in ("p", "m", "v", "r", "u", "delta", "s_m", "p_norm", "u_norm")}
    for p, g, m, v in zip(ps, gs, ms, vs):
        p, g, m, v = (t.detach().double().cpu().reshape(-1) for t in (p, g, m, v))
        ge = g * gsc
        m2 = m * b1 + one_m_b1 * ge
        v2 = v * b2 + one_m_b2 * ge * ge
        u = c * (m2 / (v2.sqrt() + eps)) + wd * p
        pn, un = math.sqrt(float((p * p).sum())), math.sqrt(float((u * u).sum()))
        r = trust_ratio(pn, un, adapt, trust_clip)
        delta = lr * r * u
        for k, x in zip(("p", "m", "v", "r", "u", "delta", "s_m", "p_norm", "u_norm"),
                        (p - delta, m2, v2, r, u, delta, (m * b1).abs() + (one_m_b1 * ge).abs(), pn, un)):
            out[k].append(x)
    return out


def _worst(err, scale):
    ratio = torch.where(scale > 0, err / scale, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def _fail(what, name, i, got, ref, err, allowed, bad):
    raise AssertionError("%s: %s[%d of %d]: got %r, reference %r, |err| %.3e, allowed %.3e; %d elements out of bound" % (
        what, name, i, err.numel(), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(err.reshape(-1)[i]),
        float(allowed.reshape(-1)[i]), int(bad.sum())))


def check_lamb(got_p, got_m, got_v, ref, k, p_old, m_old, lr, c, what=""):
    """Tensor k of a lamb_ref64 result against fp32 results, element by element: m within K_M u s_m, v within K_V u v, p within
    K_P u (|p| + |D|) + RHO |D|; the precondition of K_P (module docstring) is asserted.  -> (worst err / bound) of p, m, v."""
    p_old = p_old.detach().double().cpu().reshape(-1)
    delta = ref["delta"][k].abs()
    if p_old.numel() and bool((m_old.detach() != 0).any()):
        floor = float((p_old.abs() + delta).min())
        assert 19.0 * c * f32(lr) * ref["r"][k] <= 2.0 * floor, (what, "the cancellation term of the bound needs 19 c lr r <= 2 min(|p| + |D|)",
                                                                  c, lr, ref["r"][k], floor)
    bounds = (K_P * U * (p_old.abs() + delta) + RHO * delta, K_M * U * ref["s_m"][k], K_V * U * ref["v"][k])
    worst = []
    for name, got, want, allowed in zip("pmv", (got_p, got_m, got_v), (ref["p"][k], ref["m"][k], ref["v"][k]), bounds):
        got = got.detach().double().cpu().reshape(-1)
        err = (got - want).abs()
        bad = ~(err <= allowed)
        if bool(bad.any()):
            _fail(what, name, int(torch.nonzero(bad)[0]), got, want, err, allowed, bad)
        worst.append(_worst(err, allowed))
    return tuple(worst)


def check_ratio(got, ref_r, what=""):
    """|got - r| <= RHO r -> err / (RHO r)."""
    err = abs(float(got) - ref_r)
    assert err <= RHO * ref_r, "%s: ratio %r, reference %r, |err| / r = %.3e (allowed RHO = %.3e)" % (what, float(got), ref_r, err / ref_r, RHO)
    return err / (RHO * ref_r)


def parts_of(numels):
    return sum((n + CHUNK - 1) // CHUNK for n in numels)


# ---------------------------------------------------------------------------------------------------------------------------- cases
def boundary_specs():
    """(numel, misalign) per tensor: every size of SIZES 16-byte aligned, an empty tensor in the middle, a view one element behind a
    16-byte boundary that is longer than one piece (the scalar path over two blocks), an aligned tensor with n % 4 == 3."""
    specs = [(n, 0) for n in SIZES]
    specs.insert(5, (0, 0))
    return specs + [(CHUNK + 1030, 1), (4 * 300 + 3, 0)]


COUNTS = [47, 48, 49, 97]
CASES = ["boundaries"] + ["n%d" % n for n in COUNTS]


def case_specs(which):
    """-> {stream: [(numel, misalign)]} for the four streams p, g, m, v."""
    if which == "boundaries":
        specs = boundary_specs()
        return {s: list(specs) for s in "pgmv"}
    count = int(which[1:])
    numels = R.layout_sizes(count, TABLE, 300 + count)
    plan = R.misalign_plan(numels, "pgmv", 300 + count)
    return {s: [(n, mis) for n, mis in zip(numels, plan[s])] for s in "pgmv"}


def case_inputs(which, step=1000, grad_scale=1.0, seed=31):
    """fp32 CPU lists (p, g, m, v) of a case: tests/multi_tensor_ref.adamw_inputs (|p| in [0.5, 2], gradients N(0, 1) / grad_scale,
    zero moments at step 1 and a plausible history later)."""
    numels = [n for n, _ in case_specs(which)["p"]]
    return R.adamw_inputs(numels, step, grad_scale, seed)
