"""Plain references for the multi-tensor launches (csrc/adamw.hip, gradsync.hip, format.hip, f16x2.hip, gemm_nt.hip): CPU only, no HIP.

Shared by tests/test_multi_tensor_cpu.py (the references against the oracle and against hand-written traces) and
tests/test_gpu_multi_tensor.py (the kernels against the references).  The case generators live here so that the CPU test judges the
reference on the very inputs the GPU test hands to the kernel.

The AdamW bound.  With u = 2^-24 (every fp32 operation returns exact * (1 + d), |d| <= u) the kernel's expression

    ge = g * grad_scale                                   (1)
    m' = m * b1 + (1 - b1) * ge                           (2)(3)(4)      (1 - b1) is exact for 0.5 <= b1 <= 1
    v' = v * b2 + (1 - b2) * ge * ge                      (5)(6)(7)(8)
    denom = sqrtf(v') + eps                               (9)(10)
    p1 = p - step_size * (m' / denom)                     (11)(12)(13)
    p2 = p1 - lr * wd * p1            (wd > 0 only)       (14)(15)(16)

has 13 fp32 roundings on the way to p without weight decay and 16 with it, 4 on the way to m' and 5 on the way to v' (6 when the
two uses of ge are counted separately, which is what a worst case does).  These counts are K_P, K_M, K_V below.  A fused
multiply-add only removes roundings.  To first order in u, with upd = step_size * |m' / denom| and s_m = |m b1| + |(1 - b1) ge|:

    |err m'| <= 3 u s_m                   (the ge term carries (1), (3), (4))
    |err v'| <= 5 u v'                    (all terms positive; the ge^2 term carries (1) twice, (6), (7), (8))
    denom:     2.5 u (sqrt halves) + 1 u (9) + 1 u (10) = 4.5 u relative
    m'/denom:  3 u s_m / denom + (4.5 + 1) u |m'| / denom, then (12), (13)

s_m exceeds |m'| only through cancellation, by at most 2 (1 - b1) |ge|, and denom >= sqrt(1 - b2) |ge|, so that excess contributes
at most 6 u step_size (1 - b1) / sqrt(1 - b2) = 19 u step_size for the betas (0.9, 0.999) -- independent of the data.  Together

    |err p1| <= 10.5 u upd + 1 u |p| + 19 u step_size
    |err p2| <= 11.5 u upd + 2 u |p| + 19 u step_size + 2 u lr wd |p1|

and with step_size <= 1e-2 and |p| >= 0.1 (check_adamw asserts both: ADAMW_MIN_ABS_P, ADAMW_MAX_STEP_SIZE) the data-independent
term is below 1.9 u |p|, so K_P * u * s_i with s_i = |p| + upd + lr wd |p1| holds with more than 1 u to spare on every term."""
import math
import os
import re

import numpy as np
import torch

U = 2.0 ** -24
K_P_NO_WD, K_P_WD, K_M, K_V = 13, 16, 4, 6
ADAMW_MIN_ABS_P, ADAMW_MAX_STEP_SIZE = 0.1, 1e-2

# the table sizes and the chunk the kernels hard-code (tests/test_multi_tensor_cpu.py reads the sources and compares)
CHUNK = 16384
TABLE = {"adamw": 48, "nonfinite": 96, "accumulate": 120, "gradsync": 96, "split": 40, "f16x2": 48, "splitk_reduce": 8}
SOURCE_CONSTANTS = {            # file under egovlp_amd/csrc -> {constexpr name: value}
    "adamw.hip": {"MAX_T": TABLE["adamw"], "CHUNK": CHUNK, "NF_MAX_T": TABLE["nonfinite"], "ACC_MAX_T": TABLE["accumulate"]},
    "gradsync.hip": {"MAX_T": TABLE["gradsync"], "CHUNK": CHUNK},
    "format.hip": {"SPLIT_MAX_T": TABLE["split"]},
    "f16x2.hip": {"ENC_MAX_T": TABLE["f16x2"]},
    "gemm_nt.hip": {"RED_MAX_T": TABLE["splitk_reduce"]},
}
SIZES = [1, 3, 4, 5, 1023, 1024, 16383, 16384, 16385, 16388, 2 * 16384 + 4, 65535, 65536, 65537, 65536 + 4096 + 4]
SMALL_SIZES = [1, 3, 4, 5, 1023, 1024]

GUARD = 8
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FC5, torch.float16: 0x7EA5}       # NaNs: a scan that over-reads sees them
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def source_constants(fname):
    """{name: value} of every `constexpr int NAME = VALUE;` in egovlp_amd/csrc/<fname>."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "egovlp_amd", "csrc", fname)) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", f.read())}


def f32(x):
    """A Python float that is exactly the fp32 the C entry point receives."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------------- work list
MT_MAX_GRID = 2 ** 31 - 1


def mt_plan(blocks, max_t, launch_results=()):
    """What mt_for_each_launch (csrc/multi_tensor.h) does with a list of block counts and a table of max_t items, written out
    independently: -> (result, launches), a launch being (nb, [item of every slot], blk_start row of count + 1 entries).  A negative
    count or one above 2^31 - 1 anywhere: result 1 and no launch.  Zeros take no slot.  A launch goes out when the table is full or
    the next item would push its grid past 2^31 - 1.  launch_results[k]: what the k-th launch returns (0 when not given); the first
    non-zero one ends the call and is the result."""
    if any(b < 0 or b > MT_MAX_GRID for b in blocks):
        return 1, []
    groups, cur = [], []
    for i, b in enumerate(blocks):
        if b == 0:
            continue
        if len(cur) == max_t or sum(blocks[j] for j in cur) + b > MT_MAX_GRID:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    launches = []
    for k, items in enumerate(groups):
        starts = [sum(blocks[j] for j in items[:n]) for n in range(len(items) + 1)]
        launches.append((starts[-1], items, starts))
        rc = launch_results[k] if k < len(launch_results) else 0
        if rc:
            return rc, launches
    return 0, launches


# ------------------------------------------------------------------------------------------------------------------------- arena
class Arena:
    """The tensors of a case carved out of ONE flat buffer that is filled with a sentinel bit pattern: at least GUARD sentinel elements
    before and after each tensor.  specs: (numel, misalign) per tensor -- misalign 0 puts the tensor at a 16-byte boundary, 1 / 2 / 3
    that many ELEMENTS behind one (4-byte but not 16-byte aligned for fp32, 2-byte but not 8-byte aligned for bf16).  After a launch
    `assert_guards()` requires every element outside the tensors to be bit-identical: an out-of-range store of a 16-byte path lands
    there."""

    def __init__(self, specs, dtype=torch.float32, device="cpu"):
        self.dtype, self.bits_dtype = dtype, _BITS[dtype]
        per16 = 16 // torch.empty(0, dtype=dtype).element_size()
        self.offsets, self.numels = [], []
        cur = 0
        for n, mis in specs:
            assert 0 <= mis < 4 and n >= 0
            start = (cur + GUARD + per16 - 1) // per16 * per16 + mis
            self.offsets.append(start)
            self.numels.append(n)
            cur = start + n
        self.total = (cur + GUARD + per16 - 1) // per16 * per16
        s = SENTINEL[dtype]
        self.sentinel = s - (1 << 32) if (dtype == torch.float32 and s >= 1 << 31) else s
        self.bits = torch.full((self.total,), self.sentinel, dtype=self.bits_dtype, device=device)
        assert self.bits.data_ptr() % 16 == 0
        self.flat = self.bits.view(dtype)
        self.views = [self.flat[o:o + n] for o, n in zip(self.offsets, self.numels)]
        inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in zip(self.offsets, self.numels):
            inside[o:o + n] = True
        self._outside = (~inside).to(device)

    def to(self, device):
        """Move the buffer (one copy) and re-create the views."""
        self.bits = self.bits.to(device)
        assert self.bits.data_ptr() % 16 == 0
        self.flat = self.bits.view(self.dtype)
        self.views = [self.flat[o:o + n] for o, n in zip(self.offsets, self.numels)]
        self._outside = self._outside.to(device)
        return self

    def fill(self, tensors):
        for v, t in zip(self.views, tensors):
            v.copy_(t.reshape(-1))
        return self

    def ptrs(self):
        return [v.data_ptr() for v in self.views]

    def snapshot(self):
        return self.bits.clone()

    def tensors_cpu(self):
        host = self.flat.cpu()
        return [host[o:o + n].clone() for o, n in zip(self.offsets, self.numels)]

    def assert_guards(self, what=""):
        bad = (self.bits != self.sentinel) & self._outside
        if bool(bad.any()):
            idx = torch.nonzero(bad).reshape(-1)[:8].tolist()
            owners = []
            for i in idx:           # the tensor whose end (or start) is nearest
                k = min(range(len(self.offsets)), key=lambda j: min(abs(i - self.offsets[j]), abs(i - self.offsets[j] - self.numels[j])))
                owners.append((i, k, i - self.offsets[k], self.numels[k]))
            raise AssertionError("%s: guard elements overwritten (flat index, tensor, index relative to its start, its numel): %s" % (what, owners))


# ------------------------------------------------------------------------------------------------------------------------- AdamW
def adamw_ref64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, correct_bias=True, grad_scale=1.0, step_size=None,
                round_scalars=True):
    """The expression of adamw_kernel (csrc/adamw.hip) element-wise in fp64 from fp32 inputs.  The scalars are what the kernel
    receives: fp32 values; step_size = fp32(egovlp_amd.optim.adamw_step_size(...)) of the fp32 lr / betas unless given (a device-side
    hyper block overrides it); round_scalars=False leaves step_size and lr * wd in fp64, as the oracle
    has them.  -> (p, m, v, s_p, s_m, s_v), all fp64; s_* are the per-element error scales:
    s_p = |p_old| + step_size |m / denom| + lr wd |p|, s_m = |m b1| + |(1 - b1) ge|, s_v = v' (all its terms are positive)."""
    from egovlp_amd.optim import adamw_step_size
    lr, b1, b2, eps, wd, gs = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay), f32(grad_scale)
    if step_size is None:
        step_size = adamw_step_size(lr, b1, b2, int(step), bool(correct_bias))
        if round_scalars:
            step_size = f32(step_size)
    one_m_b1, one_m_b2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    ge = g * gs
    m2 = m * b1 + one_m_b1 * ge
    v2 = v * b2 + one_m_b2 * ge * ge
    denom = v2.sqrt() + eps
    upd = step_size * (m2 / denom)
    p1 = p - upd
    s_p = p.abs() + upd.abs()
    p2 = p1
    if wd > 0.0:
        lw = float(np.float32(lr) * np.float32(wd)) if round_scalars else lr * wd       # the kernel's fp32 product, rounding (14)
        p2 = p1 - lw * p1
        s_p = s_p + lw * p1.abs()
    s_m = (m * b1).abs() + (one_m_b1 * ge).abs()
    return p2, m2, v2, s_p, s_m, v2.clone()


def adamw_k_p(weight_decay):
    return K_P_WD if weight_decay > 0.0 else K_P_NO_WD


def adamw_ratios(got, ref):
    """got: (p, m, v) fp32 results; ref: adamw_ref64's tuple -> the largest err / (u * s) of p, m, v (0 where both are 0)."""
    out = []
    for x, r, s in zip(got, ref[:3], ref[3:]):
        err = (x.detach().double().cpu() - r).abs()
        ratio = torch.where(s > 0, err / (U * s), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        out.append(float(ratio.max()) if ratio.numel() else 0.0)
    return out


def check_adamw(got, ref, p_old, weight_decay, step_size, what=""):
    """Element-wise |got - ref| <= k u s for p, m and v (no norm); the preconditions of the bound's derivation are asserted too.
    -> the three largest ratios err / (u s)."""
    assert step_size <= ADAMW_MAX_STEP_SIZE * (1 + 1e-6), (what, step_size)
    if p_old.numel():
        assert float(p_old.detach().abs().min()) >= ADAMW_MIN_ABS_P, (what, "the bound is derived for |p| >= %g" % ADAMW_MIN_ABS_P)
    ks = (adamw_k_p(weight_decay), K_M, K_V)
    for name, x, r, s, k in zip("pmv", got, ref[:3], ref[3:], ks):
        err = (x.detach().double().cpu() - r).abs()
        bad = err > k * U * s
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            raise AssertionError("%s: %s[%d of %d]: got %r, reference %r, |err| %.3e = %.2f u s (allowed %d); %d elements out of bound" % (
                what, name, i, err.numel(), float(x.reshape(-1)[i]), float(r.reshape(-1)[i]), float(err.reshape(-1)[i]),
                float(err.reshape(-1)[i] / (U * s.reshape(-1)[i])), k, int(bad.sum())))
    return adamw_ratios(got, ref)


def layout_sizes(count, table, seed, first_sizes=SIZES):
    """The common case generator: `count` non-empty tensors -- every size of SIZES once (as far as count reaches; shuffled), a big
    tensor that straddles chunks right behind every table flush (index table, 2 * table) and an odd one behind it, small sizes
    elsewhere -- with zero-numel entries interleaved (they take no table slot: the flush boundaries stay where `table` puts them).
    -> list of numel, zeros included."""
    rng = np.random.RandomState(seed)
    sizes = list(first_sizes)
    rng.shuffle(sizes)
    sizes = sizes[:count] + [int(rng.choice(SMALL_SIZES)) for _ in range(max(0, count - len(sizes)))]
    for k in range(table, count, table):
        sizes[k] = 65536 + 4096 + 4
        if k + 1 < count:
            sizes[k + 1] = 16385
        sizes[k - 1] = 16388
    out = []
    for i, n in enumerate(sizes):
        if i in (0, 1, table - 1, table, table + 1) or i % 29 == 7:
            out.append(0)                   # in front of the first, between neighbours, on both sides of the flush
        out.append(int(n))
    out.append(0)
    assert sum(1 for n in out if n) == count
    return out


def misalign_plan(numels, streams, seed):
    """-> {stream: [misalign per tensor]}: most tensors 16-byte aligned in every stream, the others with ONE stream (each in turn) or
    all of them 1 / 2 / 3 elements behind a 16-byte boundary."""
    rng = np.random.RandomState(seed + 1)
    plan = {s: [0] * len(numels) for s in streams}
    k = 0
    for i, n in enumerate(numels):
        if n == 0 or n == 16388 or rng.rand() < 0.55:          # 16388: always the 16-byte path across a chunk edge
            continue
        which = k % (len(streams) + 1)
        k += 1
        for j, s in enumerate(streams):
            if which == len(streams) or which == j:
                plan[s][i] = 1 + int(rng.randint(3))
    return plan


ADAMW_GRID = [(wd, cb, step, gs) for wd in (0.0, 0.01) for cb in (1, 0) for step in (1, 1000) for gs in (1.0, 1.0 / 1024)]


def adamw_cases():
    """(id, count, weight_decay, correct_bias, step, grad_scale, seed): the whole hyper-parameter grid at T + 1 tensors, two corners of
    it at the other counts."""
    T = TABLE["adamw"]
    cases = []
    for count in (1, T - 1, T, T + 1, 2 * T + 1):
        grid = ADAMW_GRID if count == T + 1 else [ADAMW_GRID[0], ADAMW_GRID[-1], ADAMW_GRID[6]]
        for wd, cb, step, gs in grid:
            cid = "n%d-wd%g-cb%d-t%d-gs%s" % (count, wd, cb, step, "1" if gs == 1.0 else "2^-10")
            cases.append((cid, count, wd, cb, step, gs, 1000 + len(cases)))
    return cases


ADAMW_LR, ADAMW_BETAS, ADAMW_EPS = 1e-2, (0.9, 0.999), 1e-6


def adamw_inputs(numels, step, grad_scale, seed):
    """fp32 (p, g, m, v) lists for a case.  |p| in [0.5, 2] (the bound's precondition), gradients N(0, 1) / grad_scale (what a scaled
    backward leaves), moments zero at step 1 and a plausible history later (m ~ N(0, 1), v in [1e-4, 4] log-uniform)."""
    gen = torch.Generator().manual_seed(seed)
    ps, gs, ms, vs = [], [], [], []
    for n in numels:
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        ps.append(sign * (0.5 + 1.5 * torch.rand(n, generator=gen)))
        gs.append(torch.randn(n, generator=gen) * (1.0 / grad_scale))
        if step == 1:
            ms.append(torch.zeros(n))
            vs.append(torch.zeros(n))
        else:
            ms.append(torch.randn(n, generator=gen))
            vs.append(torch.exp(torch.rand(n, generator=gen) * math.log(4e4)) * 1e-4)
    return ps, gs, ms, vs


def adamw_case_layout(count, seed, sizes_for_one=(65536 + 4096 + 4,)):
    T = TABLE["adamw"]
    numels = [0, sizes_for_one[seed % len(sizes_for_one)], 0] if count == 1 else layout_sizes(count, T, seed)
    return numels, misalign_plan(numels, "pgmv", seed)


# ------------------------------------------------------------------------------------------------------------------------- loss scale
def loss_scale_ref(state, overflow, lr, beta1, beta2, step, correct_bias, growth, backoff, interval, max_scale, advance=1):
    """The state machine of loss_scale_update_kernel (csrc/adamw.hip) in Python ints / floats, S rounded to fp32 with numpy.float32.
    state: dict(scale, good, skipped, inv, skip) -- words [0], [1], [3], [6], [7] of the device block; `overflow`: its found-inf word
    [2], which an advancing call clears.  -> (new state, [lr, step_size, 1 / S, skip] = the hyper block the call writes); step_size is
    the fp64 value (the device rounds it to fp32)."""
    from egovlp_amd.optim import adamw_step_size
    S, good, skipped = np.float32(state["scale"]), int(state["good"]), int(state["skipped"])
    inv, skip = np.float32(state["inv"]), float(state["skip"])
    if advance:
        inv = np.float32(1.0) / S                       # the scale the gradients of THIS step carry
        if overflow:
            skip, skipped, good = 1.0, skipped + 1, 0
            S = max(np.float32(S * np.float32(backoff)), np.float32(1.0))
        else:
            skip = 0.0
            if good + 1 >= int(interval):
                S, good = min(np.float32(S * np.float32(growth)), np.float32(max_scale)), 0
            else:
                good += 1
    t = max(int(step) - skipped, 1)
    step_size = adamw_step_size(f32(lr), f32(beta1), f32(beta2), t, bool(correct_bias))
    new = {"scale": np.float32(S), "good": good, "skipped": skipped, "inv": np.float32(inv), "skip": skip}
    return new, [f32(lr), step_size, float(inv), skip]


# ------------------------------------------------------------------------------------------------------------------------- formats
def split_bf16_ref(x):
    """hi = bf16(x), lo = bf16(x - hi): the split of csrc/common.h split_bf16 (round to nearest even)."""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def ulp_distance_f32(a, b):
    """|bits(a) - bits(b)| of two positive fp32 values."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))
