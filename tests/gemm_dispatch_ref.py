"""What egv_gemm_nt accepts and what it launches, restated in Python from the launchers as they stood before csrc/gemm_dispatch.h:
egv_gemm_nt and gemm_variant (gemm_nt.hip), egv_gemm_big_supports, egv_gemm_big_pick_mf, egv_gemm_big_launch, launch_epi,
pick_mixed_bands and launch_big (gemm_big.hip), function by function and in their order.  The header states each rule once; this file
deliberately does not share its shape.  It differs from those launchers in four ways only: a refusal that used to come behind the kernel's
launch (marked LATE) is simply a refusal here, grids are exact integers with the limits marked NEW (blocks and work ids within
2^31 - 1, the small kernel's k-slices within 65535), and the big kernel's GELU / GELU' epilogues write planes only for N % 8 == 0 (marked
TORN: the element-wise tests found the two results of a shifted tile column's overlap differing there, tests/gemm_ref.py).  Marked
UNASKED: two argument sets the launchers never looked at and the epilogues cannot run -- GELU' / ReLU' without aux_in, and an fp16 saved
gelu' (aux_bf16 3) anywhere but in the plane-only epilogue, the one place that reads and writes it as fp16.

A case is a Desc; expected() returns None (EGV_ERR_ARG) or the tuple the driver prints:
(family, mf, tn, epi, prod, mixed, nb5, passes, grid_x, grid_y, block, lds, reduce, reduce_grid, reduce_blocks1)."""
from dataclasses import dataclass

MAX_GRID = 2 ** 31 - 1
SMALL, BIG = 0, 1
RAW, LINEAR, GELU, GELU_BWD, GENERIC, GELU_X2 = range(6)
RED_NONE, RED_EPILOGUE, RED_SLAB, RED_CALLER = range(4)
ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_RELU_BWD = range(4)
POINTERS = ("a_hi", "a_lo", "b_hi", "b_lo", "bias", "residual", "aux_in", "aux_out", "out_f32", "out_hi", "out_lo", "partial", "colsum")


@dataclass(frozen=True)
class Desc:
    M: int = 256
    N: int = 256
    K: int = 64
    passes: int = 1
    trans: int = 0
    ksplit: int = 1
    accumulate: int = 0
    act: int = 0
    out_fmt: int = 0
    aux_bf16: int = 0
    alpha: float = 1.0
    grid_cap: int = 0
    lda: int = 0            # 0: the natural one (NT: K; TN: M)
    ldb: int = 0
    ldo_pad: int = 0        # ldo = N + ldo_pad
    ldoh: int = 0           # 0: N
    ptrs: frozenset = frozenset(("a_hi", "a_lo", "b_hi", "b_lo", "out_f32", "partial"))
    x2_seg: int = 2
    f3: int = 1

    def __getattr__(self, name):            # d.bias etc.: is the pointer there?
        if name in POINTERS:
            return name in self.ptrs
        raise AttributeError(name)

    def ld(self, which):
        v = getattr(self, which)
        if v:
            return v
        return {"lda": self.M if self.trans else self.K, "ldb": self.N if self.trans else self.K, "ldoh": self.N}[which]

    @property
    def ldo(self):
        return self.N + self.ldo_pad

    def words(self):
        """The driver's input line."""
        mask = sum(1 << i for i, p in enumerate(POINTERS) if p in self.ptrs)
        return " ".join(str(x) for x in (self.M, self.N, self.K, self.passes, self.trans, self.ksplit, self.accumulate, self.act, self.out_fmt,
                                         self.aux_bf16, repr(float(self.alpha)), self.grid_cap, self.ld("lda"), self.ld("ldb"), self.ldo,
                                         self.ld("ldoh"), mask, self.x2_seg, self.f3))


def cdiv(a, b):
    """C's integer division (towards zero)."""
    return abs(a) // b if a >= 0 else -(abs(a) // b)


# --------------------------------------------------------------------------------------------------------------------- gemm_big.hip
def big_supports(p):
    if p.M < 256 or p.N < 256 or p.N % 4 != 0:
        return False
    if p.ld("lda") % 8 != 0 or p.ld("ldb") % 8 != 0:
        return False
    if p.trans:
        return p.M % 8 == 0 and p.N % 8 == 0 and p.out_f32 and p.act == ACT_NONE and not p.bias and not p.residual and not p.out_hi
    return p.K % 64 == 0


def big_pick_mf(p):
    if p.trans or p.M < 320:
        return 4
    ks = p.ksplit if p.ksplit > 1 else 1
    tn = (p.N + 255) // 256
    best, best_mf = -1, 4
    for mf in (4, 5):
        tiles = ((p.M + mf * 64 - 1) // (mf * 64)) * tn * ks
        cost = ((tiles + 255) // 256) * mf
        if best < 0 or cost < best or (cost == best and mf == 5):
            best, best_mf = cost, mf
    return best_mf


def pick_mixed_bands(p, grid):
    if p.M < 640 or grid < 8:
        return -1
    tn = (p.N + 255) // 256
    tiles5 = ((p.M + 319) // 320) * tn
    R = (tiles5 + grid - 1) // grid
    if R < 2:
        return -1
    NB = (R * grid) // tn
    nb5 = cdiv(p.M - 256 * NB + 63, 64)
    if nb5 < 0:
        nb5 = 0
    if nb5 > NB:
        return -1
    r5 = (nb5 * tn + grid - 1) // grid
    cost = 5 * r5 + 4 * (R - r5)
    return nb5 if cost < 5 * R else -1


def launch_big(p, MF, TN, EPI, PROD, MIXED=False, nb5=0):
    """-> the instance and its launch: (mf, tn, epi, prod, mixed, nb5, grid, lds)."""
    BM = MF * 64
    lds = 2 * (BM * 128 + 256 * 128)
    bands = nb5 + cdiv(p.M - nb5 * 320 + 255, 256) if MIXED else (p.M + BM - 1) // BM
    tiles = bands * ((p.N + 255) // 256)
    ks = p.ksplit if p.ksplit > 1 else 1
    total = tiles * ks
    cap = p.grid_cap if p.grid_cap > 0 else 256
    return (MF, int(TN), EPI, PROD, int(MIXED), nb5, min(total, cap), lds)


def launch_epi(p, MF, TN, PROD):
    if p.out_fmt != 0:
        if PROD not in (1, 2) or p.out_fmt < 1 or p.out_fmt > 4:
            return None
        gelu_fwd = p.act == ACT_GELU and p.out_fmt in (1, 2)
        gelu_bwd16 = PROD == 1 and p.act == ACT_GELU_BWD and p.out_fmt == 4 and p.aux_in and p.aux_bf16 >= 2 and not p.bias
        lin_split = p.act == ACT_NONE and p.out_fmt == 3 and p.out_lo
        lin_grad = PROD == 1 and p.act == ACT_NONE and p.out_fmt == 4 and not p.bias
        if not (gelu_fwd or gelu_bwd16 or lin_split or lin_grad) or p.alpha != 1.0 or not p.out_hi or (p.out_fmt == 1 and not p.out_lo) or \
                p.residual or p.out_f32 or (p.aux_out and not p.aux_bf16) or p.ld("ldoh") % 8 != 0 or p.ksplit > 1 or TN:
            return None
    if p.aux_bf16 == 3 and PROD not in (1, 2):
        return None
    plain_f32 = not p.bias and not p.residual and not p.out_hi and p.out_f32
    if PROD == 1:
        if TN:
            return launch_big(p, 4, True, RAW, 1)
        if p.ksplit > 1 or p.alpha != 1.0:
            return None
        if p.act == ACT_NONE:
            return launch_big(p, MF, False, RAW if plain_f32 else LINEAR, 1)
        if p.act == ACT_GELU and p.out_fmt != 0:
            return launch_big(p, MF, False, GELU_X2, 1)
        if p.act == ACT_GELU_BWD and not p.bias:
            return launch_big(p, MF, False, GELU_BWD, 1)
        return None
    if p.ksplit > 1 or TN:
        if PROD == 2:
            return None
        return launch_big(p, MF, TN, RAW, PROD)
    if PROD != 0 and MF == 5 and not TN:
        cap = p.grid_cap if p.grid_cap > 0 else 256
        nb5 = pick_mixed_bands(p, cap)
        if nb5 >= 0 and p.alpha == 1.0:
            if p.act == ACT_NONE and (p.bias or p.residual or p.out_hi):
                return launch_big(p, 5, False, LINEAR, PROD, True, nb5)
            if p.act == ACT_GELU:
                if PROD == 2 and p.out_fmt != 0:
                    return launch_big(p, 5, False, GELU_X2, 2, True, nb5)
                return launch_big(p, 5, False, GELU, PROD, True, nb5)
    if p.alpha == 1.0 and p.act == ACT_NONE:
        return launch_big(p, MF, False, RAW if plain_f32 else LINEAR, PROD)
    if p.alpha == 1.0 and p.act == ACT_GELU:
        if PROD == 2 and p.out_fmt != 0:
            return launch_big(p, MF, False, GELU_X2, 2)
        return launch_big(p, MF, False, GELU, PROD)
    if PROD == 2:
        return None
    if p.alpha == 1.0 and p.act == ACT_GELU_BWD and not p.bias:
        return launch_big(p, MF, False, GELU_BWD, PROD)
    return launch_big(p, MF, False, GENERIC, PROD)


def big_launch(p):
    if p.trans:
        return launch_epi(p, 4, True, 1 if p.passes == 4 else 0)
    mf = big_pick_mf(p)
    if p.M < mf * 64:
        mf = 4
    f3 = p.passes == 3 and p.f3 != 0            # EGV_GEMM_F3, the diagnostics build's knob
    if p.passes == 2:
        seg = bool(p.x2_seg & 2) or (bool(p.x2_seg & 1) and p.K <= 768 and p.N <= 768)
        return launch_epi(p, mf, False, 1 if seg else 2)
    if p.passes == 4:
        return launch_epi(p, mf, False, 1)
    if f3:
        return launch_epi(p, mf, False, 3)
    return launch_epi(p, mf, False, 0)


# ---------------------------------------------------------------------------------------------------------------------- gemm_nt.hip
def gemm_variant(p):
    big_ok = big_supports(p)
    if p.trans:
        return 3 if big_ok else -1
    if p.passes in (2, 4):
        return 3 if big_ok else -1
    big_tiles = ((p.M + 255) // 256) * ((p.N + 255) // 256) * (p.ksplit if p.ksplit > 1 else 1)
    if big_ok and big_tiles >= 128:
        return 3
    return 1


def expected(p, late=True):
    """late = False: without the rules the former launchers applied only behind the kernel's launch."""
    if not p.a_hi or not p.b_hi:
        return None
    if p.passes < 1 or p.passes > 4:
        return None
    if p.passes in (2, 3) and (not p.a_lo or not p.b_lo):
        return None
    if p.out_fmt < 0 or p.out_fmt > 4:
        return None
    if p.M <= 0 or p.N <= 0 or p.K <= 0:
        return None
    if p.N % 4 != 0 or p.ld("lda") % 8 != 0 or p.ld("ldb") % 8 != 0:
        return None
    if not p.trans and p.K % 32 != 0:
        return None
    if p.ksplit > 1 and not p.partial:
        return None
    if p.colsum and not p.trans:
        return None
    if p.grid_cap != 0 and (p.grid_cap < 8 or p.grid_cap > 256 or p.grid_cap % 8 != 0):
        return None
    variant = gemm_variant(p)
    if variant < 0:
        return None
    if p.aux_bf16 < 0 or p.aux_bf16 > 3:
        return None
    if p.aux_bf16 and (variant < 3 or p.act == ACT_RELU_BWD):
        return None
    if p.aux_bf16 == 3 and p.passes != 4 and p.passes != 2:
        return None
    if variant >= 3 and p.out_hi and p.N % 8 != 0 and p.act in (ACT_GELU, ACT_GELU_BWD):       # TORN
        return None
    if p.act in (ACT_GELU_BWD, ACT_RELU_BWD) and not p.aux_in:                                  # UNASKED: the epilogues read aux_in
        return None
    if p.aux_bf16 == 3 and p.act in (ACT_GELU, ACT_GELU_BWD) and (not p.out_hi or p.residual or p.out_f32):     # UNASKED: fp16 gelu' is the
        return None                                                                             # plane epilogue's alone
    if (p.passes in (2, 4) or p.out_fmt != 0) and (variant < 3 or p.passes not in (2, 4)):
        return None
    if (p.passes == 2 or p.out_fmt != 0) and (p.trans or p.ksplit > 1):
        return None
    if p.passes == 4 and not p.trans and p.ksplit > 1:
        return None
    if p.alpha != 1.0 and p.trans and not (p.alpha > 0.0):
        return None
    tiles = ((p.M + 127) // 128) * ((p.N + 127) // 128)
    ks = p.ksplit if p.ksplit > 1 else 1
    if variant >= 3:
        big = big_launch(p)
        if big is None:
            return None
        if ((p.M + 255) // 256) * ((p.N + 255) // 256) * ks > MAX_GRID:        # NEW: the kernel counts its work ids in an int
            return None
        mf, tn, epi, prod, mixed, nb5, grid, lds = big
        head = (BIG, mf, tn, epi, prod, mixed, nb5, 0, grid, 1, 512, lds)
    else:
        if tiles > MAX_GRID or ks > 65535:                                      # NEW
            return None
        head = (SMALL, 0, 0, 0, 0, 0, 0, 3 if p.passes == 3 else 1, tiles, ks, 256, 2 * (4 if p.passes == 3 else 2) * 8192)
    blocks = (p.M * p.N // 4 + 255) // 256
    blocks2 = (p.M // 4 + 255) // 256 if p.colsum else 0
    if ks > 1 and blocks + blocks2 > MAX_GRID:                                  # NEW
        return None
    if ks > 1 and not p.trans and variant < 3:
        if late and p.accumulate:                                               # LATE
            return None
        return head + (RED_EPILOGUE, blocks, blocks)
    if ks > 1 and p.accumulate == 2:
        if late and (not p.trans or not p.out_f32 or p.ldo != p.N):             # LATE
            return None
        return head + (RED_CALLER, 0, 0)
    if ks > 1:
        if late and (not p.out_f32 or p.ldo != p.N):                            # LATE
            return None
        if late and p.colsum and p.M % 4 != 0:                                  # LATE
            return None
        return head + (RED_SLAB, blocks + blocks2, blocks)
    return head + (RED_NONE, 0, 0)


def line(result):
    """What the driver prints for one case (its last word: does the instance exist, gemm_big_instance)."""
    if result is None:
        return "1"
    return " ".join(["0"] + [str(int(x)) for x in result] + ["1"])
