"""What csrc/block_plan.h has to say, restated from the code it replaced: geom_ok and the inline derivations of fwd_layout, egv_block_fwd
and egv_block_bwd in csrc/block.hip before the plan header (lo, h16, bf, q1, a1p, Pa, P_qkv / P_fc1 / P_fc2, proj1, afmt, amode,
proj_desc, x2, walpha, ln_fmt, as_lo_f ...), in that code's own vocabulary.  tests/test_block_plan_cpu.py holds the header, and
model/layer_common.py::block_plan, to it."""
import struct
from collections import namedtuple

# the stub formulas of the test's driver for the library's workspace sizes
def attn_fwd_work_floats(B, T, n, H, mode):
    return B * H * (1 + T * n) * (3 if mode else 5) + 7


def attn_bwd_work_floats(B, T, n, H):
    return B * H * (1 + T * n) * 2 + 64 * H


def layernorm_bwd_parts(rows):
    return (rows + 63) // 64 if rows < 64 * 256 else 256


def cls_linear_work_floats(R, N, K):
    return R * K * 8 + N


Geom = namedtuple("Geom", "B T n H Hd P Pb train z_bf16 single")     # D = 64 H

A1_INV = 1.0 / (1.0 - 0.015625)


def geom_ok(g):
    D = g.H * 64
    if g.B <= 0 or g.T <= 0 or g.n <= 0 or g.H <= 0 or g.Hd <= 0 or D % 32 or g.Hd % 32:
        return False
    if g.P < 1 or g.P > 3 or g.Pb not in (1, 3, 4):
        return False
    if g.Pb == 3 and g.P != 3:
        return False
    if g.Pb == 4 and g.P != 2:
        return False
    if g.train < 0 or g.train > 3:
        return False
    if g.P == 2 and (g.Pb == 3 or ((g.train & 1) and not g.z_bf16)):
        return False
    if g.single < 0 or g.single > 15 or (g.single and g.P != 2):
        return False
    return True


def plan(g):
    """-> the fields of BlockPlan in the order the driver prints them, from the derivations of the former egv_block_fwd / _bwd."""
    P, Pb, s = g.P, g.Pb, g.single
    train, tail = bool(g.train & 1), bool(g.train & 2)
    # ---- egv_block_fwd
    Pa = 3 if P == 2 else P
    P_fc1, P_fc2, P_qkv = (4 if s & 1 else P), (4 if s & 2 else P), (4 if s & 4 else P)
    proj1 = bool(s & 8)
    h16 = Pb == 4
    afmt = (3 if proj1 else 2) if h16 else (1 if proj1 else 0)
    amode_fwd = (afmt << 1) | (8 if h16 else 0)
    # proj_desc: (operand planes, passes) by format -- 3: (a_hi, -) x4; 2: (a_hi, a_lo) x2; 1: (a_lo, -) x4; 0: (a_hi, a_lo) x Pa
    P_proj, proj_operand = {3: (4, 1), 2: (2, 0), 1: (4, 2), 0: (Pa, 0)}[afmt]
    passes = (P_qkv, P_proj, P_qkv, P_proj, P_fc1, P_fc2)
    # a single-product Linear reads ONE plane (its producer wrote no second one: fwd_layout's q1 / f16_single & 1 / & 2)
    operand = (int(P_qkv == 4), proj_operand, int(P_qkv == 4), proj_operand, int(P_fc1 == 4), int(P_fc2 == 4))
    # _block_params / _X2_FMTS on the Python side: qkv / fc1 / fc2 weights f16x2 in the f16x2 mode, proj split-bf16 unless proj_x2
    x2fmts = (1, 0, 1, 0, 1, 1)
    proj_x2 = bool(s & 8) or Pb == 4
    w_fmt = tuple((1 if (proj_x2 and i in (1, 3)) else x2fmts[i]) if P == 2 else 0 for i in range(6))
    walpha = (A1_INV if h16 and not (s & 4) else 1.0, A1_INV if h16 and not proj1 else 1.0, A1_INV if h16 and not (s & 4) else 1.0,
              A1_INV if h16 and not proj1 else 1.0, A1_INV if h16 and not (s & 1) else 1.0, A1_INV if h16 and not (s & 2) else 1.0)
    # ---- fwd_layout
    lo = P != 1
    bf = P == 2 and train and not h16
    q1 = bool(s & 4)
    a1p = h16 and bool(s & 8)
    # ---- egv_block_bwd
    x2 = P == 2 and not h16
    amode_bwd = (afmt << 1) | (8 | 16 if h16 else 0)
    return (train, tail) + passes + operand + w_fmt + walpha + (
        P != 1,                                 # w_lo: `P != 1 && !p.w_lo[i]` refuses
        P == 2,                                 # ln: `if (P == 2) return egv_layernorm_fwd_f16x2`
        lo and not q1, lo and not (s & 1), lo, lo and not a1p, lo and not (s & 2), bf,
        3 if h16 else 0,                        # `if (h16) d.out_fmt = 3` of the qkv GEMMs
        Pa, afmt, amode_fwd, amode_bwd,
        1 if h16 else 0,                        # egv_cls_attn_*: `h16 ? 1 : 0`
        ((2 if P_fc2 == 4 else 1) if P == 2 else 0),
        ((3 if h16 else 2) if g.z_bf16 else 0),
        ((2 if g.z_bf16 else 4) if train else 0),
        Pb, Pb == 3, x2,
        4 if h16 else 0,                        # `if (h16) d.out_fmt = 4` x 5, ln_in
        3 if h16 else 0,                        # ln_fmt
        1 if h16 else Pb,                       # `h16 ? 1 : Pb` of egv_divided_attn_bwd
        not (proj1 or h16),                     # as_lo_f / at_lo_f
        2 if h16 else 1)                        # `h16 ? 2 : 1` of the tail's last egv_cls_linear_dgrad


def fmt(v):
    if isinstance(v, bool):
        return "1" if v else "0"
    if isinstance(v, float):
        return "%.9g" % struct.unpack("f", struct.pack("f", v))[0]      # the header's alpha is a float
    return str(int(v))


class Bump:
    def __init__(self):
        self.off = 0

    def take(self, nbytes):
        o = self.off
        self.off += (nbytes + 255) // 256 * 256
        return o


def fwd_layout(g):
    """-> (offsets in the order of the former FwdLayout, total) as the former fwd_layout computed them."""
    S = 1 + g.T * g.n
    M, D, Hd, B = g.B * S, g.H * 64, g.Hd, g.B
    lo, h16, train, tail = g.P != 1, g.Pb == 4, bool(g.train & 1), bool(g.train & 2)
    bf = g.P == 2 and train and not h16
    b = Bump()
    plane = lambda cols: b.take(M * cols * 2)                     # noqa: E731
    plane_lo = lambda cols: b.take(M * cols * 2) if lo else -1    # noqa: E731
    plane_bf = lambda cols: b.take(M * cols * 2) if bf else -1    # noqa: E731
    q1 = bool(g.single & 4)
    L = {}
    L["n3_hi"] = plane(D); L["n3_lo"] = -1 if q1 else plane_lo(D)
    L["mean3"] = b.take(M * 4); L["rstd3"] = b.take(M * 4)
    L["qkvt_hi"] = plane(3 * D); L["qkvt_lo"] = plane_lo(3 * D)
    a1p = h16 and bool(g.single & 8)
    L["at_hi"] = plane(D); L["at_lo"] = -1 if a1p else plane_lo(D)
    L["lse_t"] = b.take(B * g.H * S * 4)
    L["work_t"] = b.take(attn_fwd_work_floats(B, g.T, g.n, g.H, 1) * 4)
    L["tr"] = b.take(M * D * 4)
    L["n1_hi"] = plane(D); L["n1_lo"] = -1 if q1 else plane_lo(D)
    L["mean1"] = b.take(M * 4); L["rstd1"] = b.take(M * 4)
    for k in ("n1c", "mean1c", "rstd1c", "qc", "oc", "n2c", "hc"):
        L[k] = -1
    if tail:
        L["qkvs_hi"] = plane(2 * D); L["qkvs_lo"] = plane_lo(2 * D)
        for k in ("as_hi", "as_lo", "work_s", "n2_hi", "n2_lo", "h_hi", "h_lo", "n2_bf", "h_bf"):
            L[k] = -1
        L["lse_s"] = b.take(B * g.H * 4)
        L["n1c"] = b.take(B * D * 4); L["mean1c"] = b.take(B * 4); L["rstd1c"] = b.take(B * 4)
        L["qc"] = b.take(B * D * 4); L["oc"] = b.take(B * D * 4)
        L["sr"] = b.take(B * D * 4)
        L["n2c"] = b.take(B * D * 4); L["mean2"] = b.take(B * 4); L["rstd2"] = b.take(B * 4)
        L["hc"] = b.take(B * Hd * 4)
        L["z"] = b.take(B * Hd * 4) if train else -1
        L["n3_bf"] = plane_bf(D); L["n1_bf"] = plane_bf(D)
    else:
        L["qkvs_hi"] = plane(3 * D); L["qkvs_lo"] = plane_lo(3 * D)
        L["as_hi"] = plane(D); L["as_lo"] = -1 if a1p else plane_lo(D)
        L["lse_s"] = b.take(B * g.H * S * 4)
        L["work_s"] = b.take(attn_fwd_work_floats(B, g.T, g.n, g.H, 0) * 4)
        L["sr"] = b.take(M * D * 4)
        L["n2_hi"] = plane(D); L["n2_lo"] = -1 if g.single & 1 else plane_lo(D)
        L["mean2"] = b.take(M * 4); L["rstd2"] = b.take(M * 4)
        L["h_hi"] = plane(Hd); L["h_lo"] = -1 if g.single & 2 else plane_lo(Hd)
        L["z"] = b.take(M * Hd * (2 if g.z_bf16 else 4)) if train else -1
        L["n3_bf"] = plane_bf(D); L["n1_bf"] = plane_bf(D); L["n2_bf"] = plane_bf(D); L["h_bf"] = plane_bf(Hd)
    return [L[k] for k in FWD_ORDER], b.off


FWD_ORDER = ("n3_hi n3_lo mean3 rstd3 qkvt_hi qkvt_lo at_hi at_lo lse_t work_t tr n1_hi n1_lo mean1 rstd1 qkvs_hi qkvs_lo as_hi as_lo lse_s "
             "work_s sr n2_hi n2_lo mean2 rstd2 h_hi h_lo z n3_bf n1_bf n2_bf h_bf n1c mean1c rstd1c qc oc n2c hc").split()


def wshape(D, Hd, i):
    return ((3 * D, D), (D, D), (3 * D, D), (D, D), (Hd, D), (D, Hd))[i]


def bwd_layout(g, ksplit):
    """-> (offsets in the order of the former BwdLayout, total) as the former bwd_layout computed them."""
    S = 1 + g.T * g.n
    M, D, Hd, B = g.B * S, g.H * 64, g.Hd, g.B
    lo, tail = g.Pb == 3, bool(g.train & 2)
    b = Bump()
    plane = lambda cols: b.take(M * cols * 2)                     # noqa: E731
    plane_lo = lambda cols: b.take(M * cols * 2) if lo else -1    # noqa: E731
    L = {k: -1 for k in BWD_ORDER}
    if tail:
        L["dzc"] = b.take(B * Hd * 4); L["dn2c"] = b.take(B * D * 4); L["dsrc"] = b.take(B * D * 4); L["doc"] = b.take(B * D * 4)
        L["dqc"] = b.take(B * D * 4)
        L["lin_work"] = b.take(cls_linear_work_floats(B, max(D, Hd), max(D, Hd)) * 4)
        L["dqkvs_hi"] = plane(2 * D); L["dqkvs_lo"] = plane_lo(2 * D)
    else:
        L["g_hi"] = plane(D); L["g_lo"] = plane_lo(D)
        L["dz_hi"] = plane(Hd); L["dz_lo"] = plane_lo(Hd)
        L["d_n2"] = b.take(M * D * 4)
        L["d_sr"] = b.take(M * D * 4)
        L["dsr_hi"] = plane(D); L["dsr_lo"] = plane_lo(D)
        L["das_hi"] = plane(D); L["das_lo"] = plane_lo(D)
        L["dqkvs_hi"] = plane(3 * D); L["dqkvs_lo"] = plane_lo(3 * D)
    L["d_n1"] = b.take(M * D * 4)
    L["d_tr"] = b.take(M * D * 4)
    L["dtr_hi"] = plane(D); L["dtr_lo"] = plane_lo(D)
    L["dat_hi"] = plane(D); L["dat_lo"] = plane_lo(D)
    L["dqkvt_hi"] = plane(3 * D); L["dqkvt_lo"] = plane_lo(3 * D)
    L["d_n3"] = b.take(M * D * 4)
    for i in range(3):
        L["ln_work%d" % i] = b.take(2 * D * layernorm_bwd_parts(M) * 4)
    L["attn_work"] = b.take(attn_bwd_work_floats(B, g.T, g.n, g.H) * 4)
    for i in range(6):
        N, K = wshape(D, Hd, i)
        ks = ksplit[i] if (ksplit and not (tail and i > 2)) else 1
        if tail and i == 2:
            N = 2 * D
        L["partial%d" % i] = b.take(ks * (N * K + N) * 4) if ks > 1 else -1
    return [L[k] for k in BWD_ORDER], b.off


BWD_ORDER = ("g_hi g_lo dz_hi dz_lo d_n2 d_sr dsr_hi dsr_lo das_hi das_lo dqkvs_hi dqkvs_lo d_n1 d_tr dtr_hi dtr_lo dat_hi dat_lo dqkvt_hi dqkvt_lo "
             "d_n3 ln_work0 ln_work1 ln_work2 attn_work partial0 partial1 partial2 partial3 partial4 partial5 dzc dn2c dsrc doc dqc lin_work").split()


def grad_layout(g):
    D, Hd = g.H * 64, g.Hd
    off, p = [], 0
    for n in [N * K for N, K in (wshape(D, Hd, i) for i in range(6))] + [wshape(D, Hd, i)[0] for i in range(6)] + [D] * 6:
        off.append(p)
        p += n
    return off, p


def lines(g, ksplit):
    """The driver's four lines of an accepted geometry."""
    fo, ft = fwd_layout(g)
    bo, bt = bwd_layout(g, ksplit)
    go, gt = grad_layout(g)
    return ["plan " + " ".join(fmt(v) for v in plan(g)), "fwd " + " ".join(map(str, fo + [ft])), "bwd " + " ".join(map(str, bo + [bt])),
            "grad " + " ".join(map(str, go + [gt]))]
