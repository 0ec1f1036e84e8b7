"""The GEMM (csrc/gemm_nt.hip, gemm_big.hip, gemm_dispatch.h) element by element: the case table, the input generators, the references,
the bounds and a numpy model of the tile walk.  CPU only, no HIP.

Shared by tests/test_gemm_cases_cpu.py (the table against the dispatch header, the exactness proof, the erf polynomial, the tile-walk
model and its mutants) and tests/test_gpu_gemm_elements.py (egv_gemm_nt against the references).

EXACT-SUM INPUTS.  The kernels multiply the planes they are given; nothing requires `lo` to be the residual of `hi`.  A "grid" case
hands them planes of small integers: hi = i 2^-a_exp (A only; B: a_exp = 0), lo = j 2^-lo_exp 2^-a_exp, |i|, |j| <= amax; bias, residual
and the previous contents of out_f32 are integers times 2^-e_exp, alpha is a power of two.  Every product and every partial sum is
then a multiple of one power of two (the grain of Case.exactness) and below 2^24 of them (its magnitude: the sum of the absolute maxima
of every term that can ever be added), hence exactly representable in fp32 in WHATEVER order the MFMA, the k-segments, the split-K slabs and the
reduce add them: the expected value of an element is one integer computation and the comparison is bit for bit.

What the kernels form (read from the sources, restated by product64):
    passes 1 / 4   A_hi B_hi                                    (one bf16 / fp16 product; the lo planes are not read)
    passes 3       A_hi B_lo + A_lo B_hi + A_hi B_hi            (no lo lo term)
    passes 2       A_1 B_1 + A_2 B_2                            (hi = plane 1, lo = plane 2)
    TN             C[m, n] = sum_k A[k, m] B[k, n]; rows past K count as zero
    TN colsum      gemm_big.hip adds one MFMA of the A fragment against ones per k-step while the k-SEGMENT index is >= 1 (or there is one
                   segment only): passes 1 / 4: sum_k A_hi[k, m]; passes 3 (segments (A_hi, B_lo), (A_lo, B_hi), (A_hi, B_hi)):
                   sum_k (A_lo + A_hi)[k, m].  alpha scales the products, never the column sums.
Epilogue order (include/egovlp_hip.h): alpha, + bias, activation, + residual, stores.  A split-K launch of the big kernel has no
epilogue: NT slabs are summed as they are (alpha, bias, activation and residual are not applied), TN slabs carry alpha.  `accumulate`
is read by the slab reduce only; an un-split launch overwrites.

BOUNDS for what is not linear.  u = 2^-24; every fp32 operation returns exact (1 + d), |d| <= u; v_exp_f32 and v_rcp_f32 are good to
one ulp = 2 u; a contraction to fma only removes roundings.  gelu_parts (csrc/common.h) computes, for the exact fp32 z,
    y = (c z) z                     2                 e = exp2(y)                2   (one ulp)
    t = rcp(fma(p', |z|, 1))        1 + 2             poly = t (a1 + t (a2 + t (a3 + t (a4 + t a5))))      4 (mul, add) + 1 = 9
    half = (0.5 poly) e             1                 cdf = 1 - half  (or half)  1                          K_CDF = 18
Every one of them is a relative error of a quantity that ends in `half` <= 1/2, except the last, of cdf <= 1; the alternating
coefficients cancel to O(1) intermediate values while poly <= 1, which is why the count is taken on the scale 1 and not 1/2.  The error
of y moves e by 2 u (z^2 / 2) relative, i.e. cdf by at most 2 u max_z (z^2 / 2) erfc(|z| / sqrt 2) / 2 < 0.2 u: inside the slack.
    |cdf - Phi(z)| <= K_CDF u + E / 2,   E = ERF_E: the approximation error of A&S 7.1.26 the kernel's comment states
    gelu  = z cdf                    + 1:  |err| <= K_GELU u |z| + |z| / 2 E,                               K_GELU = 19
    gelu' = cdf + z pdf, pdf = c' e  (2 + 2 + 1 + 1 = 6 u of |z| pdf) + 1 (the sum):
            |err| <= K_GELU_GRAD u (1 + |z| pdf) + E / 2,                                                   K_GELU_GRAD = 19
A 16-bit saved gelu' adds half an ulp of its format; a product with gelu' adds one rounding; a residual behind a gelu one more.
A non-power-of-two alpha: one rounding of the product, one per further addition (bias, slabs, accumulate), on the sum of |terms|.

RANDOM CLASS.  randn data split by split_bf16_ref, the fp64 value of the same plane products as the reference, and the bound
2 (T + ksplit + e) u sum |a| |b| (T products per element, e epilogue operations; the factor 2 because the rounding of the MFMA's internal
adds is not documented)."""
import zlib
from dataclasses import dataclass, replace

import numpy as np
import torch

import f16x2_ref as F2
import gemm_dispatch_ref as R
from gemm_dispatch_ref import Desc
from layernorm_ref import half_ulp_bf16, half_ulp_f16
from multi_tensor_ref import U, split_bf16_ref

SMALL, BIG = R.SMALL, R.BIG
RAW, LINEAR, GELU, GELU_BWD, GENERIC, GELU_X2 = R.RAW, R.LINEAR, R.GELU, R.GELU_BWD, R.GENERIC, R.GELU_X2
EPI_NAMES = ("RAW", "LINEAR", "GELU", "GELU_BWD", "GENERIC", "GELU_X2")
RED_NONE, RED_EPILOGUE, RED_SLAB, RED_CALLER = R.RED_NONE, R.RED_EPILOGUE, R.RED_SLAB, R.RED_CALLER
ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_RELU_BWD = R.ACT_NONE, R.ACT_GELU, R.ACT_GELU_BWD, R.ACT_RELU_BWD

ERF_E = 1.5e-7                      # csrc/common.h: "erf by Abramowitz & Stegun 7.1.26 (|abs error| <= 1.5e-7 ...)"
K_CDF, K_GELU, K_GELU_GRAD = 18, 19, 19
ALPHA_X2 = float(np.float32(1.0) / (np.float32(1.0) - np.float32(F2.E)))        # 1 / (1 - e) of csrc/f16x2.h, as the fp32 the callers pass
OPERANDS = ("a_hi", "a_lo", "b_hi", "b_lo")


# ------------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    id: str
    d: Desc
    want: tuple                 # (family, mf, tn, epi, prod, mixed, reduce) the pick has to be, or None: EGV_ERR_ARG
    amax: int = 7               # grid class: |integers| of every plane, of bias / residual / previous contents
    lo_exp: int = 6             # lo = integer 2^-lo_exp
    a_exp: int = 0              # both planes of A times 2^-a_exp (brings a GELU's argument to O(1))
    e_exp: int = 0              # bias, residual, previous contents: integers 2^-e_exp
    ldaux_pad: int = 0
    ldr_pad: int = 0
    out_bf: bool = False        # out_fmt 1 / 2: the bf16 copy as a further plane
    klass: str = "grid"         # or "randn"
    edges: tuple = ()           # what of the issue's list this case stands for (the coverage statement counts them)

    @property
    def fp16(self):
        return self.d.passes in (2, 4)

    @property
    def ks(self):
        return self.d.ksplit if self.d.ksplit > 1 else 1

    @property
    def nprod(self):
        return {1: 1, 2: 2, 3: 3, 4: 1}[self.d.passes]

    @property
    def ldaux(self):
        return self.d.N + self.ldaux_pad

    @property
    def ldr(self):
        return self.d.N + self.ldr_pad

    @property
    def alpha_pow2(self):
        m, _ = np.frexp(self.d.alpha)
        return m == 0.5

    # -- the exactness claim (tests/test_gemm_cases_cpu.py proves it for every grid case)
    def exactness(self):
        """[(what, magnitude, grain)]: every term and every partial sum of `what` is a multiple of the power of two `grain`, and
        `magnitude` is the sum of the absolute maxima of everything that can ever be added into one of its elements."""
        d, lo = self.d, 2.0 ** -self.lo_exp
        g = {1: 0, 4: 0, 3: self.lo_exp, 2: 2 * self.lo_exp}[d.passes] + self.a_exp
        if self.alpha_pow2 and d.alpha < 1.0:
            g -= int(np.log2(d.alpha))
        per_k = self.amax ** 2 * {1: 1.0, 4: 1.0, 3: 1.0 + 2.0 * lo, 2: 1.0 + lo * lo}[d.passes] * 2.0 ** -self.a_exp
        extra = sum(1 for p in ("bias", "residual") if getattr(d, p)) + (1 if d.accumulate == 1 else 0)
        out = [("product", d.K * per_k * max(d.alpha, 1.0) + extra * self.amax * 2.0 ** -self.e_exp,
                2.0 ** -max(g, self.e_exp if extra else 0))]
        if d.colsum:
            out.append(("colsum", d.K * self.amax * (1.0 + (lo if d.passes == 3 else 0.0)) * 2.0 ** -self.a_exp,
                        2.0 ** -(self.a_exp + (self.lo_exp if d.passes == 3 else 0))))
        return out


def _case(cid, M, N, K, passes, want, outs=("out_f32",), ins=(), trans=0, ksplit=1, acc=0, act=0, out_fmt=0, aux16=0, alpha=1.0, cap=0, lda=0,
          ldb=0, ldo_pad=0, ldoh=0, x2=2, **kw):
    ptrs = frozenset(OPERANDS + tuple(outs) + tuple(ins) + (("partial",) if ksplit > 1 else ()))
    d = Desc(M=M, N=N, K=K, passes=passes, trans=trans, ksplit=ksplit, accumulate=acc, act=act, out_fmt=out_fmt, aux_bf16=aux16, alpha=alpha,
             grid_cap=cap, lda=lda, ldb=ldb, ldo_pad=ldo_pad, ldoh=ldoh, ptrs=ptrs, x2_seg=x2)
    return Case(cid, d, want, **kw)


def _big(mf, epi, prod, mixed=0, tn=0, red=RED_NONE):
    return (BIG, mf, tn, epi, prod, mixed, red)


def _small(red=RED_NONE):
    return (SMALL, 0, 0, 0, 0, 0, red)


# The smallest shapes that keep each pick, found with gemm_dispatch_ref.expected() from the shapes of tools/gemm_launch_census.py
# (256x256x64; 5376x3072x64; 5384x3072x64; 7176x2304x64 with grid_cap 8) and made ragged in both directions:
#   a bf16 / bf16x3 NT product takes the big kernel from 128 tiles of 256x256:      64 x 2 tiles -> M = 63 * 256 + 1, N = 256 + 4
#   320-row tiles (MF 5) win when 256-row tiles need a second round of 256 CUs:     129 x 2 = 258 tiles (103 x 2 of 320 rows)
#                                                                                   -> M = 128 * 256 + 1, N = 260; any product kind
#   mixed bands need MF 5 and two rounds of grid_cap workgroups:                    the same shape with grid_cap 8 (97 + 7 bands)
#   an fp16 product (passes 2 / 4) takes the big kernel from one tile:              M = 257, N = 260
# Rows x columns: 16 129 x 260 = 4.2 M elements where the census has 16.5 M; 32 769 x 260 = 8.5 M where it has 16.5 M.
M_BF16_MF4, M_MF5, M_F16_MF4, N_RAGGED = 63 * 256 + 1, 128 * 256 + 1, 257, 260
PASSES_OF = {0: 1, 3: 3, 2: 2}      # PROD -> passes (PROD 1: passes 4, or passes 2 under the default EGV_X2_SEG); PROD 0 with passes 3 -- the
#                                     three k-segments of the plain NT loop -- needs the diagnostics build (EGV_GEMM_F3=0): not in the table,
#                                     its instances are the PROD 0 ones that passes 1 reaches


def _epilogue(epi, prod, v, N):
    """The descriptor fields that select `epi` for a product kind, in two flavours: v = 0 the fp32 layout of the kernel's epilogue (fp32
    outputs, padded rows), v = 1 its plane layout (16-bit outputs, ldoh padded)."""
    f16 = prod in (1, 2)
    pad8 = (-N) % 8 + 8                         # a padded ldoh that is a multiple of 8 whatever N is (fp16 planes require it)
    if epi == RAW:
        return dict(outs=("out_f32",), ldo_pad=4 * v)
    if epi == LINEAR:
        if v == 0:
            return dict(outs=("out_f32",), ins=("bias", "residual"), ldo_pad=4, ldr_pad=12)
        return dict(outs=("out_hi", "out_lo"), ins=("bias",), ldoh=N + pad8, out_fmt=3 if f16 else 0)
    if epi == GELU:
        if v == 0:
            return dict(act=ACT_GELU, outs=("out_f32", "aux_out"), ins=("bias",), ldaux_pad=4, a_exp=7, e_exp=2)
        return dict(act=ACT_GELU, outs=("out_hi", "out_lo", "aux_out"), ins=("bias",), aux16=2, ldoh=N + pad8, ldaux_pad=pad8, a_exp=7, e_exp=2)
    if epi == GELU_X2:
        if v == 0:                              # ONE plane of plain fp16, the saved gelu' as bf16
            return dict(act=ACT_GELU, out_fmt=2, aux16=2, outs=("out_hi", "aux_out"), ins=("bias",), ldoh=N + pad8, ldaux_pad=pad8, a_exp=7, e_exp=2,
                        out_bf=True)
        return dict(act=ACT_GELU, out_fmt=1, aux16=3, outs=("out_hi", "out_lo", "aux_out"), ins=("bias",), ldoh=N + pad8, ldaux_pad=pad8, a_exp=7,
                    e_exp=2)
    if epi == GELU_BWD:
        if v == 0:
            return dict(act=ACT_GELU_BWD, outs=("out_f32",), ins=("aux_in",), ldaux_pad=4, ldo_pad=8)
        if prod == 1:                           # dZ of the fp16 backward: the saved gelu' as fp16, one plane of un-clamped fp16
            return dict(act=ACT_GELU_BWD, out_fmt=4, aux16=3, outs=("out_hi",), ins=("aux_in",), ldoh=N + pad8, ldaux_pad=pad8, a_exp=4)
        return dict(act=ACT_GELU_BWD, aux16=1, outs=("out_hi", "out_lo"), ins=("aux_in",), ldoh=N + pad8, ldaux_pad=pad8)
    assert epi == GENERIC
    if v == 0:
        return dict(act=ACT_RELU_BWD, outs=("out_f32",), ins=("aux_in",), ldaux_pad=4)
    return dict(alpha=0.5, outs=("out_f32", "out_hi", "out_lo"), ins=("bias", "residual"), ldoh=N + pad8, ldr_pad=4)


def _n_for(epi, prod, v):
    """N of an instance case: 256 + 4, or 256 + 8 where the check wants N % 8 == 0 (planes out of a GELU / GELU' epilogue of the big kernel:
    with N % 8 == 4 the two results of the overlap of a shifted tile column are not bit-identical, and (hi, lo) pairs tore -- the case
    refused-gelu-planes-N260 is the one that showed it, 3 of 8.5 M elements off by one bf16 ulp)."""
    f = _epilogue(epi, prod, v, N_RAGGED)
    return 264 if f.get("act") in (ACT_GELU, ACT_GELU_BWD) and "out_hi" in f["outs"] else N_RAGGED


def _instances(x2):
    """One case per instance of gemm_big_instance() that the product library reaches under EGV_X2_SEG = x2 (2: the default; 0: the fused
    f16x2 loop, PROD 2), plus, under the default, the two small-kernel instances."""
    out = []
    N = N_RAGGED
    if x2 == 2:
        kinds = [(0, 1), (3, 3), (1, 4), (1, 2)]          # (PROD, passes)
        epis = {0: (RAW, LINEAR, GELU, GELU_BWD, GENERIC), 3: (RAW, LINEAR, GELU, GELU_BWD, GENERIC), 1: (RAW, LINEAR, GELU_X2, GELU_BWD)}
    else:
        kinds = [(2, 2)]
        epis = {2: (RAW, LINEAR, GELU, GELU_X2)}
    for prod, passes in kinds:
        for mf in (4, 5):
            M = M_MF5 if mf == 5 else (M_F16_MF4 if prod in (1, 2) else M_BF16_MF4)
            for epi in epis[prod]:
                # both flavours of an epilogue are reached through the two tile heights; PROD 1 has two passes values to spread them over
                v = (mf == 5) if prod != 1 else ((passes == 2) != (mf == 5))
                if epi == GELU_BWD and passes == 2:
                    v = 0                                    # the 16-bit dZ flavour is passes 4's (MF 5)
                Ne = _n_for(epi, prod, int(v))
                out.append(_case("mf%d-p%d-x%d-%s" % (mf, prod, passes, EPI_NAMES[epi]), M, Ne, 64, passes, _big(mf, epi, prod), x2=x2,
                                 edges=("instance",), **_epilogue(epi, prod, int(v), Ne)))
    mixed = [(3, 3, LINEAR), (3, 3, GELU)] if x2 == 2 else [(2, 2, LINEAR), (2, 2, GELU), (2, 2, GELU_X2)]
    for prod, passes, epi in mixed:
        Ne = _n_for(epi, prod, 1)
        out.append(_case("mixed-p%d-%s" % (prod, EPI_NAMES[epi]), M_MF5, Ne, 64, passes, _big(5, epi, prod, mixed=1), cap=8, x2=x2,
                         edges=("instance", "many-tiles-per-workgroup"), **_epilogue(epi, prod, 1, Ne)))
    if x2 == 2:
        for passes in (1, 4):                                 # TN: PROD 0 (bf16) and PROD 1 (fp16)
            out.append(_case("tn-p%d-x%d-RAW" % (passes == 4, passes), 264, 264, 64, passes, _big(4, RAW, int(passes == 4), tn=1), trans=1,
                             outs=("out_f32", "colsum"), edges=("instance",)))
        for passes in (1, 3):
            out.append(_case("small-x%d" % passes, 128, 128, 64, passes, _small(), edges=("instance",)))
    return out


def _big_nt_edges():
    out = []
    lin_f = dict(outs=("out_f32",), ins=("bias", "residual"), ldo_pad=4, ldr_pad=4)
    # N = 256 k + 4, + 8, + 252: a shifted last column whose origin is 16-byte but not 64-byte aligned.  fp16 kinds at one tile row + 1, the
    # fused bf16x3 loop at the smallest M that reaches the big kernel; residual: an overlap computed twice must not add it twice
    for N in (260, 264, 508, 772):
        out.append(_case("nt-N%d-p1" % N, 257, N, 64, 4, _big(4, LINEAR, 1), edges=("shifted-column",), **lin_f))
    for N in (264, 508):
        out.append(_case("nt-N%d-p3" % N, M_BF16_MF4, N, 64, 3, _big(4, LINEAR, 3), edges=("shifted-column",), **lin_f))
    # M = whole tiles + 1, + 8, + tile - 1 rows (the + 1 rows of MF 4 / MF 5 / MIXED are the instance cases)
    for extra in (8, 255):
        out.append(_case("nt-M+%d-mf4-p1" % extra, 256 + extra, 260, 64, 2, _big(4, LINEAR, 1), edges=("shifted-row-mf4",), **lin_f))
        out.append(_case("nt-M+%d-mf4-p3" % extra, 63 * 256 + extra, 260, 64, 3, _big(4, RAW, 3), edges=("shifted-row-mf4",)))
    for extra in (1, 8, 319):
        out.append(_case("nt-M+%d-mf5-p3" % extra, 103 * 320 + extra, 260, 64, 3, _big(5, LINEAR, 3), edges=("shifted-row-mf5",), **lin_f))
    # MIXED: the 256-row bands start behind nb5 bands of 320 rows, and nb5 is chosen so that the bands R rounds hold exceed M by less than
    # 64 rows: with nb5 > 0 the last band always lies 193 .. 256 rows past the one before it (193 in the instance cases, 200 and 255
    # here).  1 and 8 rows exist only where nb5 is clamped to 0 -- the mixed pick with 256-row bands alone, every tile run with the fifth
    # fragment group off: 155 x 256 + 1 and + 8 rows under grid_cap 248 (found with the mirror over N, grid_cap and M)
    for M in (M_MF5 + 7, 32831):
        out.append(_case("nt-M%d-mixed-p3" % M, M, 260, 64, 3, _big(5, LINEAR, 3, mixed=1), cap=8, outs=("out_hi", "out_lo"), ins=("bias",),
                         ldoh=272, edges=("shifted-row-mixed", "many-tiles-per-workgroup")))
    for M in (155 * 256 + 1, 155 * 256 + 8):
        out.append(_case("nt-M%d-mixed-nb5-0-p3" % M, M, 260, 64, 3, _big(5, LINEAR, 3, mixed=1), cap=248, outs=("out_hi", "out_lo"),
                         ins=("bias",), ldoh=272, edges=("shifted-row-mixed",)))
    # K = 128, 768 (64 is everywhere else); lda / ldb = K + 8.  passes 2 with K = 768: lo on 2^-3 keeps the lo lo products inside 2^24 grains
    out.append(_case("nt-K128-mf4-p3", M_BF16_MF4, 260, 128, 3, _big(4, LINEAR, 3), lda=136, ldb=136, edges=("K128", "lda-ldb"), **lin_f))
    out.append(_case("nt-K128-mf5-p0", M_MF5, 260, 128, 1, _big(5, LINEAR, 0), lda=136, ldb=136, edges=("K128", "lda-ldb"), **lin_f))
    out.append(_case("nt-K128-mixed-p3", M_MF5, 264, 128, 3, _big(5, GELU, 3, mixed=1), cap=8, lda=136, ldb=136,
                     edges=("K128", "lda-ldb", "many-tiles-per-workgroup"), **_epilogue(GELU, 3, 1, 264)))
    out.append(_case("nt-K768-mf4-p1-x2", 513, 260, 768, 2, _big(4, LINEAR, 1), lda=776, ldb=776, lo_exp=3, edges=("K768", "lda-ldb"), **lin_f))
    out.append(_case("nt-K768-mf4-p1-x4", 264, 516, 768, 4, _big(4, RAW, 1), lda=776, ldb=776, ldo_pad=4, edges=("K768", "lda-ldb")))
    # big split-K (slab reduce): accumulate 0 and 1, ksplit dividing the k-tiles or not.  K = 768 is 24 k-tiles of the fused loop (32 deep),
    # 12 of the plain one (64 deep); 13 x 2 tiles x 5 slices = 130 work items reach the big kernel
    out.append(_case("nt-splitk5-p3-K768", 3073, 260, 768, 3, _big(4, RAW, 3, red=RED_SLAB), ksplit=5, edges=("K768", "big-splitk", "ksplit-uneven")))
    out.append(_case("nt-splitk5-p0-K768-acc", 3073, 260, 768, 1, _big(4, RAW, 0, red=RED_SLAB), ksplit=5, acc=1,
                     edges=("K768", "big-splitk", "ksplit-uneven", "accumulate-1")))
    out.append(_case("nt-splitk4-mf5-p3-K128-acc", 8193, 260, 128, 3, _big(5, RAW, 3, red=RED_SLAB), ksplit=4, acc=1, edges=("big-splitk", "accumulate-1")))
    # the header's contract for what a split-K launch of the big kernel leaves out: alpha, bias, an activation and residual given and not applied
    out.append(_case("nt-splitk2-p3-no-epilogue", M_BF16_MF4 // 2 + 1, 260, 64, 3, _big(4, RAW, 3, red=RED_SLAB), ksplit=2, alpha=0.5,
                     act=ACT_RELU_BWD, ins=("bias", "residual", "aux_in"), edges=("big-splitk",)))
    # un-split: `accumulate` is not read, the previous contents are overwritten
    out.append(_case("nt-unsplit-accumulate-ignored", 257, 260, 64, 4, _big(4, RAW, 1), acc=1, edges=("accumulate-unsplit",)))
    return out


def _tn_cases():
    """Weight gradients: bf16 passes 1 and 3, fp16 passes 4; output M, N in {256, 264, 504, 520}; K in {1, 63, 64, 65, 130}; ksplit 1, 2, 3 and
    more slices than k-tiles (the check ties no limit to K: 5 slices of a 1- or 2-tile contraction stand for "the largest"); column sums
    on and off; accumulate 0, 1, 2; alpha 1, 1/2, 1 / (1 - e); lda > M."""
    rows = [  # M, N, K, passes, ksplit, acc, colsum, alpha, lda
        (256, 256, 64, 1, 1, 0, 1, 1.0, 0), (264, 520, 1, 1, 1, 0, 1, 0.5, 272), (504, 264, 63, 3, 1, 0, 1, 1.0, 0),
        (520, 504, 65, 4, 1, 0, 0, ALPHA_X2, 528), (264, 256, 130, 3, 1, 1, 0, 1.0, 0),
        (256, 264, 130, 1, 2, 0, 1, 1.0, 264), (504, 520, 65, 3, 2, 1, 1, 0.5, 0), (264, 504, 64, 4, 2, 2, 1, 1.0, 0),
        (520, 256, 130, 4, 3, 0, 0, 1.0, 0), (256, 504, 63, 1, 3, 2, 0, 0.5, 0), (504, 256, 130, 3, 3, 2, 1, 1.0, 512),
        (264, 264, 1, 3, 3, 1, 1, 1.0, 0), (520, 520, 65, 1, 5, 0, 1, 1.0, 0), (256, 256, 1, 4, 5, 2, 1, ALPHA_X2, 0),
        (504, 504, 130, 4, 5, 1, 0, ALPHA_X2, 0), (264, 520, 64, 3, 5, 0, 0, 1.0, 0),
    ]
    out = []
    for M, N, K, passes, ks, acc, cs, alpha, lda in rows:
        red = RED_NONE if ks == 1 else (RED_CALLER if acc == 2 else RED_SLAB)
        tag = "alpha1" if alpha == 1.0 else ("alpha-half" if alpha == 0.5 else "alpha-x2")
        edges = ("tn", "tn-M%d" % M, "tn-N%d" % N, "tn-K%d" % K, "tn-ks%d" % ks, "tn-acc%d" % acc, "tn-colsum%d" % cs, "tn-" + tag,
                 "tn-p%d" % passes) + (("tn-lda",) if lda else ())
        out.append(_case("tn-%dx%dx%d-p%d-ks%d-acc%d-cs%d-%s%s" % (M, N, K, passes, ks, acc, cs, tag, "-lda" if lda else ""), M, N, K, passes,
                         _big(4, RAW, int(passes == 4), tn=1, red=red), trans=1, ksplit=ks, acc=acc, alpha=alpha, lda=lda,
                         ldo_pad=4 if ks == 1 else 0, outs=("out_f32",) + (("colsum",) if cs else ()), edges=edges))
    return out


def _small_cases():
    """The 128x128 kernel: M in {1, 127, 128, 129, 200}, N in {4, 72, 124, 128, 132}, K in {32, 96}; every epilogue, un-split and through the
    reduce-with-epilogue with 2 slices of 3 k-steps (uneven) and 5 slices of 3 or 1 (more slices than k-steps)."""
    eps = [
        ("alpha-bias", dict(alpha=0.5, ins=("bias",), outs=("out_f32",), ldo_pad=4)),
        ("gelu-aux", dict(act=ACT_GELU, ins=("bias",), outs=("out_f32", "aux_out"), ldaux_pad=4, a_exp=6, e_exp=2)),
        ("gelu-bwd", dict(act=ACT_GELU_BWD, ins=("aux_in",), outs=("out_f32",), ldaux_pad=8)),
        ("relu-bwd", dict(act=ACT_RELU_BWD, ins=("aux_in",), outs=("out_f32", "out_hi", "out_lo"), ldoh=0, ldaux_pad=4)),
        ("residual-planes", dict(ins=("bias", "residual"), outs=("out_f32", "out_hi", "out_lo"), ldoh=-8, ldr_pad=4)),
        ("planes-only", dict(ins=("bias",), outs=("out_hi",), ldoh=-16)),
        ("alpha-odd", dict(alpha=0.3, ins=("bias", "residual"), outs=("out_f32",))),
    ]
    shapes = [(1, 4, 32), (127, 72, 96), (128, 124, 96), (129, 128, 96), (200, 132, 96), (129, 132, 32), (200, 4, 96)]
    out = []
    for i, (name, f) in enumerate(eps):
        for j, ks in enumerate((1, 2, 5)):
            M, N, K = shapes[(i + 2 * j) % len(shapes)]
            if ks == 2:
                K = 96
            f2 = dict(f)
            if f2.get("ldoh", 0) < 0:
                f2["ldoh"] = N - f2["ldoh"]
            passes = 3 if (i + j) % 2 == 0 else 1
            edges = ("small", "small-M%d" % M, "small-N%d" % N, "small-K%d" % K, "small-ks%d" % ks, "small-" + name)
            out.append(_case("small-%s-%dx%dx%d-p%d-ks%d" % (name, M, N, K, passes, ks), M, N, K, passes,
                             _small(RED_EPILOGUE if ks > 1 else RED_NONE), ksplit=ks, edges=edges, **f2))
    return out


def _refused():
    """Calls the mirror refuses: EGV_ERR_ARG and every buffer intact."""
    return [
        _case("refused-big-splitk-padded-ldo", 3073, 260, 768, 3, None, ksplit=5, ldo_pad=4, edges=("refused",)),
        _case("refused-nt-accumulate-2", 3073, 260, 768, 3, None, ksplit=5, acc=2, edges=("refused",)),
        _case("refused-small-splitk-accumulate", 129, 128, 96, 3, None, ksplit=2, acc=1, edges=("refused",)),
        _case("refused-tn-N-260", 256, 260, 64, 1, None, trans=1, edges=("refused",)),
        _case("refused-fp16-planes-ldoh-260", 257, 260, 64, 4, None, outs=("out_hi", "out_lo"), ins=("bias",), out_fmt=3, edges=("refused",)),
        _case("refused-fp16-below-one-tile", 255, 260, 64, 4, None, edges=("refused",)),
        # accepted until these tests ran it: GELU' into (hi, lo) planes at N % 8 == 4 on the big kernel (see _n_for); and its forward twin
        _case("refused-gelu-planes-N260", M_MF5, 260, 64, 3, None, edges=("refused",), **_epilogue(GELU_BWD, 3, 1, 260)),
        # found by reading the epilogues: nothing looked at these two.  GELU' without aux_in read a null pointer; an fp16 saved gelu'
        # next to an fp32 output went through the rolled epilogue, which decodes every 16-bit aux as bf16
        _case("refused-gelu-bwd-without-aux-in", 128, 128, 64, 3, None, act=ACT_GELU_BWD, edges=("refused",)),
        _case("refused-f16-gelu-grad-into-fp32", 257, 264, 64, 4, None, act=ACT_GELU_BWD, aux16=3, ins=("aux_in",), edges=("refused",)),
        _case("refused-gelu-x2-planes-N260", 257, 260, 64, 4, None, edges=("refused",), **_epilogue(GELU_X2, 1, 0, 260)),
    ]


def _random():
    return [
        _case("randn-small", 200, 132, 96, 3, _small(RED_EPILOGUE), ksplit=2, klass="randn", edges=("randn",)),
        _case("randn-big-nt-ragged", M_BF16_MF4, 260, 64, 3, _big(4, RAW, 3), ldo_pad=4, klass="randn", edges=("randn",)),
        _case("randn-tn-tail", 264, 504, 130, 3, _big(4, RAW, 0, tn=1, red=RED_SLAB), trans=1, ksplit=2, outs=("out_f32", "colsum"), klass="randn",
              edges=("randn",)),
    ]


CASES = _instances(2) + _big_nt_edges() + _tn_cases() + _small_cases() + _refused() + _random()
X2_CASES = _instances(0)                # needs EGV_X2_SEG=0: read once per process
BY_ID = {c.id: c for c in CASES + X2_CASES}
assert len(BY_ID) == len(CASES) + len(X2_CASES)


def pick_of(c):
    """(family, mf, tn, epi, prod, mixed, reduce) of the mirror's answer, or None."""
    r = R.expected(c.d)
    return None if r is None else (r[0], r[1], r[2], r[3], r[4], r[5], r[12])


def big_id(want):
    """gemm_big_id of a pick."""
    _, mf, tn, epi, prod, mixed, _ = want
    return ((((mf - 4) * 2 + tn) * 6 + epi) * 4 + prod) * 2 + mixed


def big_instance(mf, tn, epi, prod, mixed):
    """gemm_big_instance (csrc/gemm_dispatch.h), restated."""
    if mf not in (4, 5) or not 0 <= prod <= 3 or not RAW <= epi <= GELU_X2:
        return False
    if tn:
        return mf == 4 and epi == RAW and prod <= 1 and not mixed
    if mixed:
        return mf == 5 and prod >= 2 and (epi in (LINEAR, GELU) or (epi == GELU_X2 and prod == 2))
    if prod == 1:
        return epi in (RAW, LINEAR, GELU_X2, GELU_BWD)
    if prod == 2:
        return epi in (RAW, LINEAR, GELU, GELU_X2)
    return epi != GELU_X2


# ------------------------------------------------------------------------------------------------------------------------- inputs
def _rng(c, salt=0):
    return np.random.RandomState((zlib.crc32(c.id.encode()) + salt) % (2 ** 31))


def _ints(rng, shape, amax, exp=0):
    return torch.from_numpy(rng.randint(-amax, amax + 1, size=shape).astype(np.float64) * 2.0 ** -exp)


def make_inputs(c):
    """-> {name: fp64 tensor of the VALUES} for a_hi, a_lo, b_hi, b_lo ([M, K] / [N, K]; TN: [K, M] / [K, N]) and whichever of bias [N],
    residual, aux_in, prev (the previous contents of out_f32) [M, N] the case has.  Every value is exactly representable in the format
    it travels in (bf16 / fp16 planes: 8 / 11 significant bits; fp32 otherwise)."""
    d, rng = c.d, _rng(c)
    sa, sb = ((d.K, d.M), (d.K, d.N)) if d.trans else ((d.M, d.K), (d.N, d.K))
    x = {}
    if c.klass == "grid":
        x["a_hi"], x["a_lo"] = _ints(rng, sa, c.amax, c.a_exp), _ints(rng, sa, c.amax, c.a_exp + c.lo_exp)
        x["b_hi"], x["b_lo"] = _ints(rng, sb, c.amax), _ints(rng, sb, c.amax, c.lo_exp)
    else:
        g = torch.Generator().manual_seed(int(rng.randint(2 ** 31)))
        for n, s, scale in (("a", sa, 1.0), ("b", sb, 0.05)):
            hi, lo = split_bf16_ref(torch.randn(*s, generator=g) * scale)
            x[n + "_hi"], x[n + "_lo"] = hi.double(), lo.double()
    if d.bias:
        x["bias"] = _ints(rng, (d.N,), c.amax, c.e_exp)
    if d.residual:
        x["residual"] = _ints(rng, (d.M, d.N), c.amax, c.e_exp)
    if d.accumulate == 1:
        x["prev"] = _ints(rng, (d.M, d.N), c.amax, c.e_exp)
    if d.aux_in:
        if d.act == ACT_GELU_BWD and d.aux_bf16 >= 2:          # the saved gelu' itself: powers of two, so that the product stays exact
            x["aux_in"] = torch.from_numpy(rng.choice(np.array([0.0, 0.5, -0.5, 1.0, 2.0, -0.25]), size=(d.M, d.N)))
        else:                                                  # a pre-activation: quarter steps in [-4, 4] (exact in bf16), zeros included
            x["aux_in"] = _ints(rng, (d.M, d.N), 16, 2)
    return x


def plane_dtype(c):
    return torch.float16 if c.fp16 else torch.bfloat16


def aux_dtype(c):
    return {0: torch.float32, 1: torch.bfloat16, 2: torch.bfloat16, 3: torch.float16}[c.d.aux_bf16]


def out_plane_dtype(c):
    return torch.float16 if c.d.out_fmt != 0 else torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------- references
def _mm(a, b, trans):
    return a.t() @ b if trans else a @ b.t()


def product64(c, x, k0=0, k1=None, lo_lo=False):
    """The plane products egv_gemm_nt is specified to form over the contraction range [k0, k1), in fp64 (exact for a grid case) -> [M, N]."""
    d = c.d
    k1 = d.K if k1 is None else min(k1, d.K)
    if k1 <= k0:
        return torch.zeros(d.M, d.N, dtype=torch.float64)
    sl = (lambda t: t[k0:k1]) if d.trans else (lambda t: t[:, k0:k1])
    ah, al, bh, bl = (sl(x[n]) for n in OPERANDS)
    out = _mm(ah, bh, d.trans)
    if d.passes == 3:
        out = out + _mm(ah, bl, d.trans) + _mm(al, bh, d.trans)
        if lo_lo:
            out = out + _mm(al, bl, d.trans)
    elif d.passes == 2:
        out = out + _mm(al, bl, d.trans)
    return out


def abs_product64(c, x):
    """sum |a| |b| over the same products."""
    return product64(c, {n: x[n].abs() for n in OPERANDS})


def colsum64(c, x, k0=0, k1=None):
    """What gemm_big.hip sums into colsum (module docstring) -> [M]."""
    d = c.d
    k1 = d.K if k1 is None else min(k1, d.K)
    a = x["a_hi"][k0:k1] + (x["a_lo"][k0:k1] if d.passes == 3 else 0.0)
    return a.sum(0)


def phi64(z):
    return 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5))


def pdf64(z):
    return torch.exp(-0.5 * z * z) / (2.0 * np.pi) ** 0.5


def gelu64(z):
    return z * phi64(z)


def gelu_grad64(z):
    return phi64(z) + z * pdf64(z)


def gelu_bound(z):
    return K_GELU * U * z.abs() + z.abs() / 2.0 * ERF_E


def gelu_grad_bound(z):
    return K_GELU_GRAD * U * (1.0 + z.abs() * pdf64(z)) + ERF_E / 2.0


@dataclass
class Check:
    """What one output has to be.  bits: the tensor (in the output's dtype) it must equal bit for bit.  Otherwise |decoded - ref| <= bound
    element-wise, where decoded is the fp64 value of the output (the sum of the two planes for a split output)."""
    name: str
    bits: object = None
    ref: object = None
    bound: object = None
    planes: tuple = ()          # bound checks of a plane PAIR: the names whose sum is decoded


def f16_split_ref(v32):
    """f16_split8 (csrc/f16x2.h): hi = fp16(clamp v), lo = fp16(clamp v - hi)."""
    v = v32.clamp(-65504.0, 65504.0)
    hi = v.to(torch.float16)
    return hi, (v - hi.float()).to(torch.float16)


def reference(c, x):
    """-> [Check] for every output of the case, given make_inputs(c).  For accumulate == 2 the checks are those of out_f32 / colsum AFTER
    egv_splitk_reduce_multi."""
    d = c.d
    acc = product64(c, x)
    big = c.want[0] == BIG
    exact = c.klass == "grid"
    checks = []
    if c.klass == "randn":
        assert d.act == ACT_NONE and d.alpha == 1.0 and not d.bias and not d.residual and not d.out_hi and d.accumulate == 0
        T = d.K * c.nprod
        checks.append(Check("out_f32", ref=acc, bound=2.0 * (T + c.ks) * U * abs_product64(c, x)))
        if d.colsum:
            a = (x["a_hi"].abs() + (x["a_lo"].abs() if d.passes == 3 else 0.0)).sum(0)
            checks.append(Check("colsum", ref=colsum64(c, x), bound=2.0 * (d.K * (2 if d.passes == 3 else 1) + c.ks) * U * a))
        return checks
    if d.colsum:
        checks.append(Check("colsum", bits=colsum64(c, x).float()))
    if d.trans or (big and c.ks > 1):
        # no epilogue: TN scales by alpha (every slab, or the direct output); an NT slab launch applies nothing at all
        alpha = d.alpha if d.trans else 1.0
        prev = x["prev"] if (d.accumulate == 1 and c.ks > 1) else None
        if c.alpha_pow2 or alpha == 1.0:
            v = acc * alpha + (prev if prev is not None else 0.0)
            checks.append(Check("out_f32", bits=v.float()))
        elif c.ks == 1:
            # ONE rounding of a 24-bit sum times a 24-bit factor: the fp64 product is exact, its rounding to fp32 is the kernel's
            checks.append(Check("out_f32", bits=(acc * float(np.float32(alpha))).float()))
        else:
            # every slab rounded once, ks - 1 additions, + 1 with the previous contents: on the sum of the absolute terms
            scale = abs_product64(c, x) * alpha + (prev.abs() if prev is not None else 0.0)
            v = acc * float(np.float32(alpha)) + (prev if prev is not None else 0.0)
            checks.append(Check("out_f32", ref=v, bound=(1 + c.ks - 1 + (prev is not None)) * U * scale))
        return checks
    # ---- the fused epilogue (small kernel: also behind its reduce): alpha, + bias, activation, + residual, stores
    k_lin, scale = 0, None                                      # roundings so far on the sum of |terms| (a non-power-of-two alpha only)
    v = acc * (d.alpha if c.alpha_pow2 else float(np.float32(d.alpha)))
    if not c.alpha_pow2:
        exact, k_lin, scale = False, 1, v.abs()
    if d.bias and not (big and c.want[3] == GELU_BWD):
        v = v + x["bias"]
        if not exact:
            k_lin, scale = k_lin + 1, scale + x["bias"].abs()
    bound = None if exact else k_lin * U * scale
    if d.act == ACT_GELU:
        assert exact, "a GELU case needs an exact pre-activation"
        z = v
        if d.aux_out:
            if d.aux_bf16 == 0:
                checks.append(Check("aux_out", bits=z.float()))
            elif d.aux_bf16 == 1:
                checks.append(Check("aux_out", bits=z.float().to(torch.bfloat16)))
            else:
                g = gelu_grad64(z)
                b = gelu_grad_bound(z)
                half = half_ulp_bf16 if d.aux_bf16 == 2 else half_ulp_f16
                checks.append(Check("aux_out", ref=g, bound=b + half(g.abs() + b)))
        v, bound, exact = gelu64(z), gelu_bound(z), False
    elif d.act == ACT_GELU_BWD:
        zv = x["aux_in"]
        if d.aux_bf16 >= 2:
            v = v * zv                                          # the stored derivative: a power of two here, the product is exact
        else:
            g, gb = gelu_grad64(zv), gelu_grad_bound(zv)
            bound = v.abs() * gb + (g.abs() + gb) * (bound if bound is not None else 0.0) + U * (v * g).abs()
            v, exact = v * g, False
    elif d.act == ACT_RELU_BWD:
        v = torch.where(x["aux_in"] > 0, v, torch.zeros_like(v))
    if d.residual:
        v = v + x["residual"]
        if not exact:
            bound = bound + U * (v.abs() + bound) if d.act != ACT_NONE else (k_lin + 1) * U * (scale + x["residual"].abs())
    # ---- stores
    if d.out_f32:
        checks.append(Check("out_f32", bits=v.float()) if exact else Check("out_f32", ref=v, bound=bound))
    if d.out_hi:
        fmt = d.out_fmt
        if exact:
            v32 = v.float()
            if fmt == 0:
                hi, lo = split_bf16_ref(v32)
            elif fmt == 3:
                hi, lo = f16_split_ref(v32)
            elif fmt == 4:
                hi, lo = v32.to(torch.float16), None
            else:
                raise AssertionError("out_fmt 1 / 2 come from a GELU")
            checks.append(Check("out_hi", bits=hi))
            if d.out_lo:
                checks.append(Check("out_lo", bits=lo))
        elif fmt == 0 and d.out_f32:
            checks.append(Check("out_hi", planes=("split-of-out_f32",)))           # the planes are the split of the fp32 the kernel stored
        elif fmt == 0:
            # hi + lo is within 2^-17 |value| of the value split_bf16 was given (csrc/common.h); hi alone within half a bf16 ulp
            names = ("out_hi", "out_lo") if d.out_lo else ("out_hi",)
            rep = 2.0 ** -17 * (v.abs() + bound) if d.out_lo else half_ulp_bf16(v.abs() + bound)
            checks.append(Check("out_hi", ref=v, bound=bound + rep, planes=names))
        elif fmt == 1:
            checks.append(Check("out_hi", ref=v, bound=bound + F2.rep_bound(v.abs() + bound), planes=("out_hi", "out_lo")))
        elif fmt == 2:
            checks.append(Check("out_hi", ref=v, bound=bound + half_ulp_f16(v.abs() + bound), planes=("out_hi",)))
        else:
            raise AssertionError("an inexact value into out_fmt %d" % fmt)
        if c.out_bf:
            checks.append(Check("out_bf", ref=v, bound=bound + half_ulp_bf16(v.abs() + bound), planes=("out_bf",)))
    return checks


# ------------------------------------------------------------------------------------------------------------------------- the tile walk
def bands(c):
    """[(m0, rows)] of the pick's row bands, the last one shifted inwards (big kernel) or clipped (small kernel)."""
    d = c.d
    r = R.expected(d)
    family, mf, mixed, nb5 = r[0], r[1], r[5], r[6]
    if family == SMALL:
        return [(m0, min(128, d.M - m0)) for m0 in range(0, d.M, 128)]
    if mixed:
        n4 = (d.M - nb5 * 320 + 255) // 256
        return [(min(i * 320, d.M - 320), 320) for i in range(nb5)] + [(min(nb5 * 320 + i * 256, d.M - 256), 256) for i in range(n4)]
    bm = mf * 64
    return [(min(i * bm, d.M - bm), bm) for i in range((d.M + bm - 1) // bm)]


def columns(c):
    d = c.d
    if c.want[0] == SMALL:
        return [(n0, min(128, d.N - n0)) for n0 in range(0, d.N, 128)]
    return [(min(i * 256, d.N - 256), 256) for i in range((d.N + 255) // 256)]


def k_slices(c):
    """[(k0, k1)] of the ksplit slices: whole k-tiles (32 deep: small kernel and the fused loops PROD 2 / 3; 64: the plain loops), the
    last ones possibly empty."""
    d = c.d
    ktd = 32 if (c.want[0] == SMALL or c.want[4] >= 2) else 64
    nkt = (d.K + ktd - 1) // ktd
    per = (nkt + c.ks - 1) // c.ks
    return [(min(z * per, nkt) * ktd, min(min((z + 1) * per, nkt) * ktd, d.K)) for z in range(c.ks)]


def locate(c, m, n):
    """Where the pick computes element (m, n): for the failure report."""
    bs, cs = bands(c), columns(c)
    tb = [i for i, (m0, r) in enumerate(bs) if m0 <= m < m0 + r]
    tc = [i for i, (n0, w) in enumerate(cs) if n0 <= n < n0 + w]
    return "row band(s) %s of %d (origin %s), tile column(s) %s of %d (origin %s), k-slices %s" % (
        tb, len(bs), [bs[i][0] for i in tb], tc, len(cs), [cs[i][0] for i in tc], k_slices(c))


MUTANTS = ("drop_last_kstep", "lo_lo", "residual_twice", "slab_twice", "colsum_twice")


def applies(c, mutant):
    d = c.d
    if c.want is None or c.klass != "grid":
        return False
    rows_shifted = any(a[0] + a[1] > b[0] for a, b in zip(bands(c)[:-1], bands(c)[1:]))
    shifted = rows_shifted or any(a[0] + a[1] > b[0] for a, b in zip(columns(c)[:-1], columns(c)[1:]))
    return {"drop_last_kstep": True, "lo_lo": d.passes == 3, "residual_twice": bool(d.residual) and shifted and c.want[0] == BIG and c.ks == 1,
            "slab_twice": d.accumulate == 1 and c.ks > 1, "colsum_twice": bool(d.colsum) and rows_shifted}[mutant]


def walk(c, x, mutant=None):
    """The launch as the pick lays it out, in numpy / torch fp32 ACCUMULATION (every partial sum rounded to fp32, which a grid case never
    notices): k-slices, row bands and tile columns with their shifted origins, slabs, the reduce, and the LINEAR part of the epilogue
    (alpha, bias, ReLU', residual).  -> {"out_f32": fp32 [M, N], "colsum": fp32 [M]}.  The mutants break it the way a kernel could."""
    d = c.d
    big = c.want[0] == BIG
    f = lambda t: t.float()                                                         # noqa: E731
    slabs, cs_slabs = [], []
    for (k0, k1) in k_slices(c):
        if mutant == "drop_last_kstep" and k1 > k0:
            k1 = max(k0, (k1 - 1) // 32 * 32)                                       # the slice's last 32-deep k-step never multiplied
        out = torch.full((d.M, d.N), float("nan"), dtype=torch.float32)
        visits = torch.zeros(d.M, d.N, dtype=torch.float32)
        cs = torch.zeros(d.M, dtype=torch.float32)
        for (m0, rows) in bands(c):
            for ci, (n0, w) in enumerate(columns(c)):
                sub = {n: (x[n][:, m0:m0 + rows] if n[0] == "a" else x[n][:, n0:n0 + w]) if d.trans else
                       (x[n][m0:m0 + rows] if n[0] == "a" else x[n][n0:n0 + w]) for n in OPERANDS}
                cc = replace(c, d=replace(d, M=rows, N=w))
                out[m0:m0 + rows, n0:n0 + w] = f(product64(cc, sub, k0, k1, lo_lo=(mutant == "lo_lo")))
                visits[m0:m0 + rows, n0:n0 + w] += 1
                if d.colsum and ci == 0:
                    part = f(colsum64(cc, sub, k0, k1))
                    if mutant == "colsum_twice":
                        cs[m0:m0 + rows] += part
                    else:
                        cs[m0:m0 + rows] = part
        assert not bool(torch.isnan(out).any()), "the tiles do not cover the output"
        slabs.append(out)
        cs_slabs.append(cs)
    res = {}
    if d.colsum:
        s = cs_slabs[0]
        for t in cs_slabs[1:]:
            s = s + t
        res["colsum"] = s
    if d.trans or (big and c.ks > 1):
        alpha = np.float32(d.alpha if d.trans else 1.0)
        s = slabs[0] * alpha
        for t in slabs[1:]:
            s = s + t * alpha
        if d.accumulate == 1 and c.ks > 1:
            s = s + f(x["prev"])
            if mutant == "slab_twice":
                for t in slabs:
                    s = s + t * alpha
        res["out_f32"] = s
        return res
    s = slabs[0]
    for t in slabs[1:]:
        s = s + t
    v = s * np.float32(d.alpha)
    if d.bias and not (big and c.want[3] == GELU_BWD):
        v = v + f(x["bias"])
    if d.act == ACT_RELU_BWD:
        v = torch.where(f(x["aux_in"]) > 0, v, torch.zeros_like(v))
    if d.residual:
        v = v + f(x["residual"]) * (visits if mutant == "residual_twice" else 1.0)
    res["out_f32"] = v
    return res


# ------------------------------------------------------------------------------------------------------------------------- erf
def emu_gelu_parts(z):
    """gelu_parts (csrc/common.h) in fp32 numpy, operation by operation (uncontracted) -> (cdf, pdf)."""
    f = np.float32
    z = np.asarray(z, dtype=np.float32)
    ax = np.abs(z)
    e = np.exp2(f(-0.72134752044448170) * z * z).astype(np.float32)
    t = (f(1.0) / (f(f(0.3275911) * f(0.70710678118654752)) * ax + f(1.0))).astype(np.float32)
    poly = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    half = f(0.5) * poly * e
    cdf = np.where(z < 0, half, f(1.0) - half).astype(np.float32)
    return cdf, (f(0.3989422804014327) * e).astype(np.float32)


def erf_poly64(u):
    """A&S 7.1.26 in fp64 for u >= 0."""
    t = 1.0 / (1.0 + 0.3275911 * u)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return 1.0 - poly * np.exp(-u * u)
