"""Plain references, element-wise bounds and guarded buffers for the row kernels (csrc/layernorm.hip, the LayerNorm forward of
csrc/f16x2.hip, the embedding and relu-split kernels of csrc/format.hip): CPU only, no HIP.

Shared by tests/test_layernorm_cpu.py (the bounds judged against an fp32 emulation of the kernels' association order, against torch's
fp32 LayerNorm and against kernel-shaped mutants) and tests/test_gpu_layernorm.py / tests/test_gpu_text_input.py (the kernels against
the references).  The case generators live here so that the CPU test judges the bounds on the inputs the GPU test hands to the kernels.

Every bound has the form |got - ref| <= k u S_i with u = 2^-24: every fp32 operation returns exact (1 + d), |d| <= u; a fused
multiply-add only removes roundings, so the counts below are the uncontracted ones.  n = cols, NV = float4 per lane (<= MAXV = 4).

FORWARD (layernorm_fwd_kernel; layernorm_fwd_f16x2_kernel has the same operations with 8 channels per lane and round).
    s    = in-lane serial sum, wave butterfly              an element passes <= 3 (inside its float4) + NV (s +=) + 6 (xor 32 .. 1)
    mean = s / n                                           + 1                                         K_MEAN = 3 + 4 + 6 + 1 = 14
        |err mean| <= 14 u A,   A = mean_j |x_j|  (>= |mean|: the conditioning term -- the error of a sum scales with sum |x|)
    d    = x - mean                                        1 rounding, and it inherits err mean
    q   += d d                                             1 (square) + <= 4 NV + 6 = 22 additions
    var  = q / n                                           1
    rstd = 1 / sqrtf(var + eps)                            1 (+ eps) + 1 (sqrt) + 1 (divide), both correctly rounded
        sum_j (d_j - e)^2 = sum_j d_j^2 + n e^2 (sum_j d_j = 0): err mean enters var only in SECOND order, e^2 <= (14 u A)^2.
        rel err (var + eps) <= (2 + 1 + 22 + 1 + 1) u = 27 u;  the power -1/2 halves it, then sqrt and divide:  13.5 + 2 < K_RSTD = 16
        |err rstd| <= 16 u rstd + rstd (14 u A rstd)^2 / 2  =  16 u S,   S = rstd (1 + c2 / 16),  c2 = 14^2 u (A rstd)^2 / 2
        (c2 is 2.1 for N(-300, 0.5^2) rows, 0.005 for N(30, 1) and nothing for centred rows: written into the scale, not into k)
    y    = (d rstd) gamma + beta                           1 (d rstd) + 1 (gamma) + 1 (+ beta)
        err(d rstd) <= 14 u A rstd + |yhat| (1 [d] + 16 + c2 [rstd] + 1) u
        |err y| <= |gamma| (14 A rstd + (18 + c2) |yhat|) u + |gamma yhat| u + (|gamma yhat| + |beta|) u
                <= 20 u S_i,   S_i = |gamma_i| (|yhat_i| (1 + c2 / 20) + A rstd) + |beta_i|                            K_Y = 20
    x + x_add is ONE rounding and the statistics are those of the rounded sum: sum_out is compared bit for bit and the reference
    starts from it.

BACKWARD (layernorm_bwd_kernel<NV>; mean and rstd are INPUTS, so the reference takes the same fp32 values and no conditioning term
appears: x - mean is one rounding of an exact difference).
    xhat = (x - mean) rstd                                 2
    gy   = dy gamma                                        1
    c1   = (sum gy) (1 / n)                                1 + 22 additions + 1 (1 / n) + 1          -> 25 u G1,  G1 = mean_j |gy_j|
    c2   = (sum gy xhat) (1 / n)                           1 + 2 + 1 (product) + 22 + 2              -> 28 u G2,  G2 = mean_j |gy_j xhat_j|
    dx   = rstd (gy - c1 - xhat c2) + (add1 + add2)        1 (gy - c1) + 2 (xhat c2, subtract) + 1 (rstd) + 1 (+) and 1 (add1 + add2)
        with T = |gy| + G1 + |xhat| G2 (>= every intermediate):
        |err dx| <= rstd u (6 |gy| + 30 G1 + 34 |xhat| G2) + 2 u (|add1| + |add2|)
                 <= 34 u S_i,   S_i = rstd T_i + |add1_i| + |add2_i|                                                   K_DX = 34
    dgamma_c = sum_r dy xhat, dbeta_c = sum_r dy: a term of dgamma carries 3 roundings (xhat 2, product 1), a term of dbeta none; the
    longest chain of additions is  sweeps (a wave's serial adds over its rows, sweeps = ceil(rows / (4 parts)))  +  3 (4 waves)
    +  16 (a reduce wave's serial parts)  +  3 (4 waves)  +  ceil(parts / 64) (atomics onto the zeroed value):
        |err dgamma_c| <= (3 + adds(rows)) u sum_r |dy xhat|,     |err dbeta_c| <= adds(rows) u sum_r |dy|
    k depends on rows alone: dparam_adds(rows) below; 24 up to 256 rows, 25 .. 39 up to 4096, 40 for the second sweep.
    These scales hold for an algorithm that CENTRES x first, as the kernel does.  One that does not (torch's CPU backward forms
    b x + c on the un-centred x) is only backward stable: its error is that of the exact result for a mean moved by u A, which
    shifts every xhat of the row by u A rstd.  bwd_ref64 returns that wider scale too (s_dx_cond = S_i + rstd A rstd (G2 + |xhat| G1),
    s_dg_cond = sum_r |dy| (|xhat| + A rstd)); tests/test_layernorm_cpu.py holds torch to it and the emulation, like the GPU tests the
    kernel, to the narrow one.  On centred rows the two differ by less than 2x.

EMBEDDING.  word[ids] + pos[:L] is one rounding: bit-exact.  The backward's sums of c terms (atomics, any order) are within
(c - 1) u sum |terms|, and bit-exact for c <= 2 (one addition of two fp32 values is commutative).

The f16x2 planes decode to the value within f16x2_ref.rep_bound; a plain fp16 / bf16 plane is within half an ulp of it."""
import numpy as np
import torch

import f16x2_ref as F2
import multi_tensor_ref as MT
from multi_tensor_ref import GUARD, SENTINEL, U, Arena, source_constants, split_bf16_ref  # noqa: F401  (re-exported for the tests)

K_MEAN, K_RSTD, K_Y, K_DX, K_DG_TERM = 14, 16, 20, 34, 3

# what the kernels hard-code (tests/test_layernorm_cpu.py reads the sources and compares)
MAXV = 4                    # float4 per lane: cols <= MAXV * 256
MAX_COLS = MAXV * 256
ROWS_PER_BLOCK = 4          # one wave64 per row, 256 threads
MAX_PARTS = 1024            # grid cap of the backward
REDUCE_PARTS = 64           # parts summed by one block of the second stage (16 per wave)
F16X2_NP1_MAX = 512         # layernorm_fwd_f16x2_kernel<1> up to here, <2> beyond

FWD_ROWS = [1, 3, 4, 5, 9]
BWD_ROWS = [1, 4, 5, 256, 257, 260, 261, 4092, 4093, 4096, 4097, 4100, 4101]
ROW_SWEEP_COLS = [768, 260]
COLS = [4, 8, 64, 252, 256, 260, 508, 512, 516, 764, 768, 772, 1020, 1024]
COLS_F16X2 = [8, 64, 256, 504, 512, 520, 768, 1016, 1024]
COL_SWEEP_ROWS = 9
CLASSES = ["n01", "n30", "n300", "outlier", "zero_row"]
EPS = [1e-6, 1e-12]         # ViT, DistilBERT


def parts(rows):
    """egv_layernorm_bwd_parts: blocks of the backward = partial sums per column."""
    return min((rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK, MAX_PARTS)


def sweeps(rows):
    return (rows + ROWS_PER_BLOCK * parts(rows) - 1) // (ROWS_PER_BLOCK * parts(rows))


def nv_of(cols):
    """The NV the backward is instantiated with."""
    return max(1, (cols // 4 + 63) // 64)


def dparam_adds(rows):
    """Additions on the longest path from a term to dgamma / dbeta (module docstring)."""
    p = parts(rows)
    return sweeps(rows) + 3 + 16 + 3 + (p + REDUCE_PARTS - 1) // REDUCE_PARTS


# ------------------------------------------------------------------------------------------------------------------------- inputs
def make_rows(cls, rows, cols, seed):
    """fp32 [rows, cols] of an input class.  n01: N(0, 1); n30: N(30, 1); n300: N(-300, 0.5^2); outlier: N(0, 1) with one channel at
    200; zero_row: N(0, 1) with one row of zeros (the middle one)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    if cls == "n30":
        x = x + 30.0
    elif cls == "n300":
        x = x * 0.5 - 300.0
    elif cls == "outlier":
        x[:, min(cols - 1, 5)] = 200.0
    elif cls == "zero_row":
        x[rows // 2] = 0.0
    else:
        assert cls == "n01", cls
    return x.contiguous()


def make_affine(cols, seed):
    """gamma with mixed signs and one exact zero, beta ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed + 7919)
    gamma, beta = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    gamma[1 if cols > 1 else 0] = 0.0
    return gamma, beta


def stats_f32(x, eps):
    """mean / rstd [rows] as the backward receives them: the fp64 statistics rounded to fp32."""
    xd = x.double()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(1) + float(np.float32(eps)))
    return mean.float(), rstd.float()


# ------------------------------------------------------------------------------------------------------------------------- references
def fwd_ref64(x, gamma, beta, eps, x_add=None):
    """fp64 LayerNorm of fp32 inputs.  -> dict: y, mean, rstd, sum (fp32(x + x_add) or None), and the scales s_y, s_mean, s_rstd."""
    s32 = None
    if x_add is not None:
        s32 = x + x_add                         # ONE fp32 rounding; what sum_out holds and what the statistics are taken of
        x = s32
    xd, g, b = x.double(), gamma.double(), beta.double()
    eps = float(np.float32(eps))
    mean = xd.mean(1)
    d = xd - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(1) + eps)
    yhat = d * rstd[:, None]
    y = yhat * g + b
    A = xd.abs().mean(1)
    c2 = K_MEAN ** 2 * U * (A * rstd) ** 2 / 2.0
    s_y = g.abs() * (yhat.abs() * (1.0 + c2 / K_Y)[:, None] + (A * rstd)[:, None]) + b.abs()
    return {"y": y, "mean": mean, "rstd": rstd, "sum": s32, "s_y": s_y, "s_mean": A, "s_rstd": rstd * (1.0 + c2 / K_RSTD)}


def bwd_ref64(dy, x, gamma, mean, rstd, add1=None, add2=None):
    """fp64 LayerNorm backward of fp32 inputs (mean / rstd as given).  -> dict: dx (add1 + add2 included), dgamma, dbeta and the scales
    s_dx [rows, cols], s_dg, s_db [cols] (sums of absolute terms; the addition count comes from dparam_adds(rows))."""
    dyd, xd, g = dy.double(), x.double(), gamma.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xhat = (xd - mu) * rs
    gy = dyd * g
    c1 = gy.mean(1, keepdim=True)
    c2 = (gy * xhat).mean(1, keepdim=True)
    dx = rs * (gy - c1 - xhat * c2)
    T = gy.abs() + gy.abs().mean(1, keepdim=True) + xhat.abs() * (gy * xhat).abs().mean(1, keepdim=True)
    s_dx = rs.abs() * T
    for a in (add1, add2):
        if a is not None:
            dx = dx + a.double()
            s_dx = s_dx + a.double().abs()
    # the scales of a merely backward-stable algorithm (module docstring): mean moved by u A shifts every xhat of the row by u A rstd
    Ar = xd.abs().mean(1, keepdim=True) * rs.abs()
    s_dx_c = s_dx + rs.abs() * Ar * ((gy * xhat).abs().mean(1, keepdim=True) + xhat.abs() * gy.abs().mean(1, keepdim=True))
    s_dg = (dyd * xhat).abs().sum(0)
    return {"dx": dx, "dgamma": (dyd * xhat).sum(0), "dbeta": dyd.sum(0), "s_dx": s_dx, "s_dg": s_dg, "s_db": dyd.abs().sum(0),
            "s_dx_cond": s_dx_c, "s_dg_cond": s_dg + (dyd.abs() * Ar).sum(0)}


def embed_fwd_ref(ids, word, pos):
    """fp32 word[ids] + pos[:L] -> [B * L, D] (one rounding per element: what the kernel must give bit for bit)."""
    B, L = ids.shape
    return (word[ids] + pos[:L][None]).reshape(B * L, -1)


def embed_bwd_ref64(ids, de, V, P, pad_id=-1):
    """-> (d_word [V, D], d_pos [P, D], their sums of absolute terms, the number of terms per row of each), fp64 / int."""
    B, L = ids.shape
    D = de.shape[-1]
    ded = de.double().reshape(B, L, D)
    d_pos, s_pos = torch.zeros(P, D, dtype=torch.float64), torch.zeros(P, D, dtype=torch.float64)
    d_pos[:L], s_pos[:L] = ded.sum(0), ded.abs().sum(0)
    n_pos = torch.zeros(P, dtype=torch.int64)
    n_pos[:L] = B
    d_word, s_word = torch.zeros(V, D, dtype=torch.float64), torch.zeros(V, D, dtype=torch.float64)
    n_word = torch.zeros(V, dtype=torch.int64)
    flat = ids.reshape(-1)
    keep = flat != pad_id
    d_word.index_add_(0, flat[keep], ded.reshape(-1, D)[keep])
    s_word.index_add_(0, flat[keep], ded.reshape(-1, D)[keep].abs())
    n_word.index_add_(0, flat[keep], torch.ones(int(keep.sum()), dtype=torch.int64))
    return d_word, d_pos, s_word, s_pos, n_word, n_pos


def relu_ref(x):
    """nn.ReLU on fp32: NaN stays NaN, everything else that is not positive becomes +0."""
    return torch.relu(x) + 0.0              # (-0.0) + 0.0 = +0.0: the sign of a zero is not part of the contract


# ------------------------------------------------------------------------------------------------------------------------- bounds
def ratio(got, ref, scale, k):
    """The largest |got - ref| / (k u scale) (0 where both are 0, inf where the scale is 0 and the error is not)."""
    err = (got.detach().double().cpu() - ref).abs()
    bound = k * U * scale
    r = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)            # a NaN result is out of every bound
    return float(r.max()) if r.numel() else 0.0


def fwd_ratios(got, ref):
    """got: dict with any of y, mean, rstd (fp32) -> {name: largest err / bound}."""
    ks = {"y": (K_Y, "s_y"), "mean": (K_MEAN, "s_mean"), "rstd": (K_RSTD, "s_rstd")}
    return {n: ratio(got[n], ref[n], ref[s], k) for n, (k, s) in ks.items() if got.get(n) is not None}


def bwd_ratios(got, ref, rows, cond=False):
    """got: dict with any of dx, dgamma, dbeta -> {name: largest err / bound}; rows: the row count of the launch (it sets k).
    cond: against the scales of a backward-stable algorithm instead of the kernel's (never for the kernel or its emulation)."""
    a = dparam_adds(rows)
    c = "_cond" if cond else ""
    ks = {"dx": (K_DX, "s_dx" + c), "dgamma": (K_DG_TERM + a, "s_dg" + c), "dbeta": (a, "s_db")}
    return {n: ratio(got[n], ref[n], ref[s], k) for n, (k, s) in ks.items() if got.get(n) is not None}


def half_ulp_f16(v):
    """Half an ulp of fp16 at |v| (v fp64, inside fp16's range): 2^-11 |v| for normals, 2^-25 below them."""
    return torch.clamp(v.abs() * 2.0 ** -11, min=2.0 ** -25)


def half_ulp_bf16(v):
    return v.abs() * 2.0 ** -8              # 8 significant bits: an ulp is at most 2^-7 |v|


# ------------------------------------------------------------------------------------------------------------------------- emulation
def _f(a):
    return np.asarray(a, dtype=np.float32)


def _fma(a, b, c, fma=True):
    """fp32 a * b + c: fused (the product is exact in fp64; the fp64 sum is rounded once more, which differs from a true fma only in
    rare double-rounding ties) or as two fp32 operations."""
    if fma:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return _f(_f(a * b) + c)


def _butterfly(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 over the last axis (64 lanes)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = _f(v + v[..., lane ^ o])
    return v


def _lanes(a, cols, piece):
    """[rows, cols] -> [rows, rounds, 64, piece] zero-padded: lane l owns piece l + 64 i in round i."""
    rows = a.shape[0]
    per_round = 64 * piece
    rounds = (cols + per_round - 1) // per_round
    pad = np.zeros((rows, rounds * per_round), dtype=np.float32)
    pad[:, :cols] = a
    return pad.reshape(rows, rounds, 64, piece)


def _inside(cols, piece):
    rounds = (cols + 64 * piece - 1) // (64 * piece)
    return (np.arange(rounds * 64 * piece) < cols).reshape(1, rounds, 64, piece)


def _piece_sum(v, piece):
    """The kernel's in-piece sum: ((v0 + v1) + v2) + v3 per float4; the f16x2 form adds its two float4 sums."""
    s4 = [_f(_f(_f(v[..., k] + v[..., k + 1]) + v[..., k + 2]) + v[..., k + 3]) for k in range(0, piece, 4)]
    return s4[0] if piece == 4 else _f(s4[0] + s4[1])


def emu_fwd(x, gamma, beta, eps, x_add=None, piece=4, fma=True, mutant=None):
    """layernorm_fwd_kernel (piece = 4) / layernorm_fwd_f16x2_kernel (piece = 8) in fp32 numpy, in the kernels' association order.
    mutant: None | 'one_pass' (var = E[x^2] - mean^2) | 'skip_last' (the statistics miss the row's last float4) | 'padded_div'
    (division by the padded width NV * 256).  -> dict y, mean, rstd, sum (torch fp32)."""
    x = _f(x.numpy())
    if x_add is not None:
        x = _f(x + _f(x_add.numpy()))
    rows, cols = x.shape
    v = _lanes(x, cols, piece)
    inside = _inside(cols, piece)
    stat_in = inside.copy()
    if mutant == "skip_last":
        stat_in.reshape(-1)[cols - 4:cols] = False
    vs = np.where(stat_in, v, np.float32(0))
    n = np.float32(nv_of(cols) * 256 if mutant == "padded_div" else cols)
    s = np.zeros((rows, 64), dtype=np.float32)
    for i in range(v.shape[1]):
        s = _f(s + _piece_sum(vs[:, i], piece))
    mean = _f(_butterfly(s)[:, :1] / n)                                   # every lane holds the same bits
    q = np.zeros((rows, 64), dtype=np.float32)
    for i in range(v.shape[1]):
        for e in range(piece):
            if mutant == "one_pass":
                q = _fma(vs[:, i, :, e], vs[:, i, :, e], q, fma)
            else:
                d = np.where(stat_in[:, i, :, e], _f(v[:, i, :, e] - mean), np.float32(0))
                q = _fma(d, d, q, fma)
    var = _f(_butterfly(q)[:, :1] / n)
    if mutant == "one_pass":
        var = _f(var - _f(mean * mean))
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = _f(np.float32(1) / np.sqrt(_f(var + np.float32(eps))))
    g, b = _f(gamma.numpy())[None], _f(beta.numpy())[None]
    t = _f(_f(x - mean) * rstd)
    y = _fma(t, g, b, fma)
    return {"y": torch.from_numpy(y), "mean": torch.from_numpy(mean[:, 0].copy()), "rstd": torch.from_numpy(rstd[:, 0].copy()),
            "sum": torch.from_numpy(x.copy()) if x_add is not None else None}


def emu_bwd(dy, x, gamma, mean, rstd, add1=None, add2=None, fma=True, mutant=None):
    """layernorm_bwd_kernel<NV> + layernorm_bwd_reduce_kernel in fp32 numpy: rows dealt to (block, wave) as the grid does, per-lane
    serial dgamma / dbeta over the sweeps, 4 waves, 16 serial parts per reduce wave, 4 waves, the blocks of the second stage in turn.
    mutant: None | 'c2_from_dy' (c2 = mean(dy xhat), gamma forgotten) | 'drop_add2' | 'skip_row' (the LAST row contributes nothing to
    dgamma / dbeta: with rows past 4096 that is a row of the second sweep).  -> dict dx, dgamma, dbeta (torch fp32)."""
    dy, x, g = _f(dy.numpy()), _f(x.numpy()), _f(gamma.numpy())[None]
    rows, cols = x.shape
    mu, rs = _f(mean.numpy())[:, None], _f(rstd.numpy())[:, None]
    xh = _f(_f(x - mu) * rs)
    gy = _f(dy * g)
    tdg, tdb = dy, dy                                       # dg += d * xhat (fma), db += d
    # the wave sums: lane l owns float4 l + 64 i; serial over e inside a float4, over i
    gl, xl, dl = _lanes(gy, cols, 4), _lanes(xh, cols, 4), _lanes(dy, cols, 4)
    s1 = np.zeros((rows, 64), dtype=np.float32)
    s2 = np.zeros((rows, 64), dtype=np.float32)
    for i in range(gl.shape[1]):
        for e in range(4):
            s1 = _f(s1 + gl[:, i, :, e])
            s2 = _fma(dl[:, i, :, e] if mutant == "c2_from_dy" else gl[:, i, :, e], xl[:, i, :, e], s2, fma)
    inv = _f(np.float32(1) / np.float32(cols))
    c1 = _f(_butterfly(s1)[:, :1] * inv)
    c2 = _f(_butterfly(s2)[:, :1] * inv)
    ad = np.zeros_like(x)
    if add1 is not None:
        ad = _f(add1.numpy()).copy()
    if add2 is not None and mutant != "drop_add2":
        ad = _f(ad + _f(add2.numpy()))
    inner = _fma(-xh, np.broadcast_to(c2, xh.shape), _f(gy - c1), fma)
    dx = _fma(np.broadcast_to(rs, inner.shape), inner, ad, fma)
    # dgamma / dbeta
    P = parts(rows)
    dg = np.zeros((P, 4, cols), dtype=np.float32)
    db = np.zeros((P, 4, cols), dtype=np.float32)
    last = rows - 1 if mutant == "skip_row" else -1
    for k in range(sweeps(rows)):
        r0 = k * P * 4
        nr = min(rows - r0, P * 4)
        idx = np.arange(r0, r0 + nr)
        live = (idx != last)[:, None]
        full = np.zeros((P * 4, cols), dtype=np.float32)
        fullx = np.zeros((P * 4, cols), dtype=np.float32)
        full[:nr] = np.where(live, tdg[idx], np.float32(0))
        fullx[:nr] = xh[idx]
        dg = _fma(full.reshape(P, 4, cols), fullx.reshape(P, 4, cols), dg, fma)
        db = _f(db + full.reshape(P, 4, cols))
    work = [_f(_f(_f(a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) for a in (dg, db)]          # [P, cols] each
    out = []
    for w in work:
        nb = (P + REDUCE_PARTS - 1) // REDUCE_PARTS
        pad = np.zeros((nb * REDUCE_PARTS, cols), dtype=np.float32)
        pad[:P] = w
        pad = pad.reshape(nb, 4, 16, cols)
        a = np.zeros((nb, 4, cols), dtype=np.float32)
        for i in range(16):
            a = _f(a + pad[:, :, i])
        blk = _f(_f(_f(a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3])
        tot = np.zeros(cols, dtype=np.float32)
        for j in range(nb):
            tot = _f(tot + blk[j])
        out.append(tot)
    return {"dx": torch.from_numpy(dx), "dgamma": torch.from_numpy(out[0]), "dbeta": torch.from_numpy(out[1])}


# ------------------------------------------------------------------------------------------------------------------------- guarded buffers
class Guarded:
    """The tensors of a case -- [rows, cols] with a row stride ld >= cols -- carved out of ONE sentinel-filled Arena of a dtype.  Outputs
    (no data) keep the sentinel in every element, inputs and pre-set outputs hold their rows, and the GAPS between the rows of a
    strided tensor hold the sentinel like the guards around it.  assert_intact(): everything outside the rows is bit-identical
    afterwards; assert_untouched(): the whole buffer is (inputs)."""

    def __init__(self, dtype=torch.float32):
        self.dtype, self.items, self.order = dtype, {}, []

    def add(self, name, rows, cols, ld=None, data=None):
        ld = cols if ld is None else ld
        assert ld >= cols and name not in self.items
        self.items[name] = (rows, cols, ld, data)
        self.order.append(name)
        return self

    def build(self, device="cpu"):
        self.arena = Arena([((self.items[n][0] - 1) * self.items[n][2] + self.items[n][1], 0) for n in self.order], dtype=self.dtype)
        payload = torch.zeros(self.arena.total, dtype=torch.bool)
        for n, v, off in zip(self.order, self.arena.views, self.arena.offsets):
            rows, cols, ld, data = self.items[n]
            if data is not None:
                v.as_strided((rows, cols), (ld, 1)).copy_(data.reshape(rows, cols))
            payload[off:off + v.numel()].as_strided((rows, cols), (ld, 1)).fill_(True)
        self.arena.to(device)
        self._payload = payload.to(device)
        self._snap = self.arena.snapshot()
        return self

    def ptr(self, name):
        return self.arena.views[self.order.index(name)].data_ptr()

    def get(self, name):
        """-> the tensor's rows, [rows, cols] on the CPU."""
        rows, cols, ld, _ = self.items[name]
        return self.arena.views[self.order.index(name)].as_strided((rows, cols), (ld, 1)).cpu().clone()

    def assert_intact(self, what=""):
        bad = (self.arena.bits != self.arena.sentinel) & ~self._payload
        if bool(bad.any()):
            i = int(torch.nonzero(bad).reshape(-1)[0])
            k = max(j for j, o in enumerate(self.arena.offsets) if o - GUARD <= i) if any(o - GUARD <= i for o in self.arena.offsets) else 0
            rel = i - self.arena.offsets[k]
            raise AssertionError("%s: a guard or gap element was overwritten: flat index %d = tensor %r + %d (row stride %d, cols %d); %d in all" % (
                what, i, self.order[k], rel, self.items[self.order[k]][2], self.items[self.order[k]][1], int(bad.sum())))

    def assert_untouched(self, what=""):
        assert torch.equal(self.arena.bits, self._snap), "%s: an input buffer changed" % what

    def all_sentinel(self):
        return bool((self.arena.bits == self.arena.sentinel).all())


def rep_bound_f16x2(y):
    """|plane 1 + plane 2 - y| of the first-operand encoding (f16x2_ref.rep_bound)."""
    return F2.rep_bound(y)


def plane1_bound_f16x2(y):
    """|plane 1 - (1 - e) y|: one fp32 rounding of y - y e, then half an fp16 ulp (f16x2_ref.encode, role 0)."""
    return U * y.abs() + half_ulp_f16(y)


def ulp_distance_f32(a, b):
    return MT.ulp_distance_f32(a, b)
