"""The LayerNorm kernels element by element on a real MI355X (`pytest -m gpu`): egv_layernorm_fwd, egv_layernorm_fwd_f16x2,
egv_layernorm_bwd / _bwd_fmt and the split egv_layernorm_bwd_partial + egv_layernorm_bwd_reduce, through the C ABI, against the fp64
references of tests/layernorm_ref.py -- every buffer (inputs too) inside sentinel guards, strided cases with sentinel-filled gaps
between the rows, at the sizes where the launch geometry changes (tests/test_layernorm_cpu.py checks those against the sources).

Bounds: |got - ref| <= k u S_i, u = 2^-24, k = 20 (y), 14 (mean), 16 (rstd), 34 (dx), 3 + adds(rows) (dgamma), adds(rows) (dbeta) with
adds = 24 .. 40 -- counted rounding by rounding in the docstring of tests/layernorm_ref.py, where the scales S_i are written out.
Planes, sum_out and everything the kernel only re-formats are compared bit for bit.

Largest err / bound observed on an MI355X over all cases of this module (each test prints its own and the running maximum):
y 0.20, mean 0.15, rstd 0.20, dx 0.23, dgamma 0.10, dbeta 0.10 (the fp32 emulation of the kernels' order reaches y 0.15, mean 0.19,
rstd 0.17, dx 0.08, dgamma 0.10, dbeta 0.13 on the CPU: tests/test_layernorm_cpu.py); the decoded f16x2 planes 0.82, plane 1 alone 0.97 of the forward
bound + the format's representation error, the plain fp16 / bf16 planes 0.995 of the forward bound + half an ulp (a rounding to
nearest reaches its half ulp)."""
import ctypes as C

import numpy as np
import pytest
import torch

import layernorm_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
ERR_ARG = 1
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

_WORST = {}


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


def _h():
    from egovlp_amd import _lib
    return _lib.lib()


def _note(ratios, what):
    for k, r in ratios.items():
        _WORST[k] = max(_WORST.get(k, 0.0), r)
    print("%s: largest err / bound: %s   (all cases so far: %s)" % (
        what, " ".join("%s %.3f" % kv for kv in sorted(ratios.items())), " ".join("%s %.3f" % kv for kv in sorted(_WORST.items()))))
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _untouched(t):
    """Every element still the sentinel its arena was filled with."""
    return bool((_bits(t) == L.SENTINEL[t.dtype]).all())


def _vp(vals):
    return (C.c_void_p * len(vals))(*vals)


# ------------------------------------------------------------------------------------------------------------------------- forward
def _fwd(ops, x, gamma, beta, eps, *, x_add=None, ldx=None, ldy=None, want_sum=False, yf=True, planes=3, stats=True, cols_arg=None,
         expect=0, what=""):
    """One egv_layernorm_fwd launch on guarded buffers -> dict of the outputs (CPU).  Asserts the return code, guards and gaps, and that
    the inputs are unchanged; with expect != 0 that every output still holds its sentinels."""
    rows, cols = x.shape
    ldx = cols if ldx is None else ldx
    ldy = cols if ldy is None else ldy
    gi = L.Guarded(F32).add("x", rows, cols, ldx, x).add("gamma", 1, cols, data=gamma).add("beta", 1, cols, data=beta)
    if x_add is not None:
        gi.add("x_add", rows, cols, ldx, x_add)
    gi.build(DEV)
    go = L.Guarded(F32).add("y", rows, cols, ldy).add("mean", 1, rows).add("rstd", 1, rows).add("sum", rows, cols, ldx).build(DEV)
    gp = L.Guarded(BF16).add("hi", rows, cols, ldy).add("lo", rows, cols, ldy).build(DEV)
    rc = _h().egv_layernorm_fwd(gi.ptr("x"), gi.ptr("x_add") if x_add is not None else None, ldx, gi.ptr("gamma"), gi.ptr("beta"),
                                float(eps), rows, cols if cols_arg is None else cols_arg, go.ptr("sum") if want_sum else None,
                                gp.ptr("hi") if planes else None, gp.ptr("lo") if planes == 3 else None, go.ptr("y") if yf else None,
                                ldy, go.ptr("mean") if stats else None, go.ptr("rstd") if stats else None, ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, (what, rc)
    gi.assert_untouched(what)
    if expect:
        assert go.all_sentinel() and gp.all_sentinel(), (what, "a refused call wrote")
        return None
    go.assert_intact(what)
    gp.assert_intact(what)
    out = {"y": go.get("y"), "mean": go.get("mean")[0], "rstd": go.get("rstd")[0], "sum": go.get("sum"), "hi": gp.get("hi"),
           "lo": gp.get("lo")}
    for name, used in (("y", yf), ("mean", stats), ("rstd", stats), ("sum", want_sum), ("hi", planes), ("lo", planes == 3)):
        if not used:
            assert _untouched(out[name]), (what, name, "written though NULL")
    return out


def _check_fwd(out, ref, what, zero_row=None, beta=None, eps=None):
    _note(L.fwd_ratios(out, ref), what)
    hi, lo = L.split_bf16_ref(out["y"])
    assert _same(out["hi"], hi) and _same(out["lo"], lo), (what, "planes are not the split of the fp32 y of the same launch")
    if zero_row is not None:
        assert _same(out["y"][zero_row], beta) and float(out["mean"][zero_row]) == 0.0, (what, "row of zeros")
        assert L.ulp_distance_f32(float(out["rstd"][zero_row]), np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))) <= 1


def _fwd_case(ops, rows, cols, cls, eps, seed, what):
    x = L.make_rows(cls, rows, cols, seed)
    gamma, beta = L.make_affine(cols, seed)
    ref = L.fwd_ref64(x, gamma, beta, eps)
    out = _fwd(ops, x, gamma, beta, eps, what=what)
    _check_fwd(out, ref, what, rows // 2 if cls == "zero_row" else None, beta, eps)
    one = _fwd(ops, x, gamma, beta, eps, yf=False, planes=1, stats=False, what=what + " passes 1")          # writes hi alone
    assert _same(one["hi"], out["hi"]), (what, "passes 1: hi differs from the three-pass launch")
    f32_only = _fwd(ops, x, gamma, beta, eps, planes=0, what=what + " fp32 only")
    assert _same(f32_only["y"], out["y"]) and _same(f32_only["mean"], out["mean"]) and _same(f32_only["rstd"], out["rstd"])


@pytest.mark.parametrize("cols", L.ROW_SWEEP_COLS)
@pytest.mark.parametrize("rows", L.FWD_ROWS)
def test_forward_rows(ops, rows, cols):
    """1 / 3 / 4 / 5 / 9 rows (4 per block): the last block partly filled, one block, more than one."""
    cls = L.CLASSES[(rows + cols) % len(L.CLASSES)]
    _fwd_case(ops, rows, cols, cls, 1e-6, 1000 + rows + cols, "fwd rows %d cols %d %s" % (rows, cols, cls))


@pytest.mark.parametrize("cols", L.COLS)
def test_forward_cols(ops, cols):
    """Every width at which a lane's fourth / third / second float4 comes or goes, one float4 and two in all, the widest."""
    for k, cls in enumerate(("n01", "n30")):
        _fwd_case(ops, L.COL_SWEEP_ROWS, cols, cls, L.EPS[k], 2000 + cols + k, "fwd cols %d %s" % (cols, cls))


@pytest.mark.parametrize("eps", L.EPS)
@pytest.mark.parametrize("cls", L.CLASSES)
def test_forward_input_classes(ops, cls, eps):
    """N(0, 1), N(30, 1), N(-300, 0.5^2), an outlier channel of 200, a row of zeros (y == beta bit for bit), at a partial NV = 4 width
    and at 768, with eps 1e-6 and 1e-12."""
    for cols in (772, 768):
        _fwd_case(ops, 9, cols, cls, eps, 3000 + cols, "fwd class %s eps %g cols %d" % (cls, eps, cols))


@pytest.mark.parametrize("cols", [260, 768])
def test_forward_of_a_sum(ops, cols):
    """x_add and sum_out: sum_out == fp32(x + x_add) bit for bit and the statistics are those of the sum; sum_out alone copies x."""
    rows = 9
    x, xa = L.make_rows("n30", rows, cols, 1), L.make_rows("n300", rows, cols, 2)
    gamma, beta = L.make_affine(cols, 3)
    ref = L.fwd_ref64(x, gamma, beta, 1e-6, x_add=xa)
    out = _fwd(ops, x, gamma, beta, 1e-6, x_add=xa, want_sum=True, what="fwd sum cols %d" % cols)
    assert _same(out["sum"], ref["sum"])
    _check_fwd(out, ref, "fwd x + x_add cols %d" % cols)
    nosum = _fwd(ops, x, gamma, beta, 1e-6, x_add=xa, what="fwd x_add without sum_out")
    assert _same(nosum["y"], out["y"])
    copy = _fwd(ops, x, gamma, beta, 1e-6, want_sum=True, what="fwd sum_out without x_add")
    assert _same(copy["sum"], x)


@pytest.mark.parametrize("cols", [64, 260, 768])
def test_forward_strided_rows(ops, cols):
    """rows = B, ldx = S D (the CLS row of every clip), ldy > cols: only the chosen rows are read (the others hold NaN sentinels) and,
    with sum_out (addressed with ldx like x and x_add), only they are written; the output gaps stay as they were."""
    B, S = 5, 7
    x, xa = L.make_rows("n01", B, cols, 4), L.make_rows("n30", B, cols, 5)
    gamma, beta = L.make_affine(cols, 6)
    ref = L.fwd_ref64(x, gamma, beta, 1e-12, x_add=xa)
    out = _fwd(ops, x, gamma, beta, 1e-12, x_add=xa, want_sum=True, ldx=S * cols, ldy=cols + 12, what="fwd strided cols %d" % cols)
    assert _same(out["sum"], ref["sum"])
    _check_fwd(out, ref, "fwd strided cols %d" % cols)


# ------------------------------------------------------------------------------------------------------------------------- f16x2 forward
def _fwd_f16x2(ops, x, gamma, beta, eps, *, ldx=None, ldy=None, two=True, bf=True, stats=True, cols_arg=None, ldy_arg=None, expect=0,
               what=""):
    rows, cols = x.shape
    ldx = cols if ldx is None else ldx
    ldy = cols if ldy is None else ldy
    gi = L.Guarded(F32).add("x", rows, cols, ldx, x).add("gamma", 1, cols, data=gamma).add("beta", 1, cols, data=beta).build(DEV)
    go = L.Guarded(F32).add("mean", 1, rows).add("rstd", 1, rows).build(DEV)
    g16 = L.Guarded(F16).add("y1", rows, cols, ldy).add("y2", rows, cols, ldy).build(DEV)
    gbf = L.Guarded(BF16).add("bf", rows, cols, ldy).build(DEV)
    rc = _h().egv_layernorm_fwd_f16x2(gi.ptr("x"), ldx, gi.ptr("gamma"), gi.ptr("beta"), float(eps), rows,
                                      cols if cols_arg is None else cols_arg, g16.ptr("y1"), g16.ptr("y2") if two else None,
                                      gbf.ptr("bf") if bf else None, ldy if ldy_arg is None else ldy_arg,
                                      go.ptr("mean") if stats else None, go.ptr("rstd") if stats else None, ops._stream())
    torch.cuda.synchronize()
    assert rc == expect, (what, rc)
    gi.assert_untouched(what)
    if expect:
        assert go.all_sentinel() and g16.all_sentinel() and gbf.all_sentinel(), (what, "a refused call wrote")
        return None
    for g in (go, g16, gbf):
        g.assert_intact(what)
    out = {"mean": go.get("mean")[0], "rstd": go.get("rstd")[0], "y1": g16.get("y1"), "y2": g16.get("y2"), "bf": gbf.get("bf")}
    if not two:
        assert _untouched(out["y2"]), (what, "plane 2 written though NULL")
    if not bf:
        assert _untouched(out["bf"]), (what, "bf plane written though NULL")
    return out


def _check_f16x2(out, ref, two, what):
    """mean / rstd inside the forward bounds; the decoded planes within the forward bound + the format's representation error; the
    single plane / the bf16 plane within the forward bound + their half ulp."""
    r = L.fwd_ratios({"mean": out["mean"], "rstd": out["rstd"]}, ref)
    yb = L.K_Y * L.U * ref["s_y"]                              # |y_kernel - y_ref| <=
    ymax = ref["y"].abs() + yb
    if two:
        dec = out["y1"].double() + out["y2"].double()
        r["y_f16x2"] = float(((dec - ref["y"]).abs() / (yb + L.rep_bound_f16x2(ymax))).max())
        # the GEMM multiplies the planes separately: plane 1 must be (1 - e) y on its own, not just one half of a sum that decodes
        r["plane1"] = float(((out["y1"].double() - (1.0 - L.F2.E) * ref["y"]).abs() / (yb + L.plane1_bound_f16x2(ymax))).max())
        r["bf_vs_decoded"] = float(((out["bf"].double() - dec).abs() / (L.half_ulp_bf16(ymax) + L.rep_bound_f16x2(ymax))).max())
    else:
        r["y_f16"] = float(((out["y1"].double() - ref["y"]).abs() / (yb + L.half_ulp_f16(ymax))).max())
        r["bf"] = float(((out["bf"].double() - ref["y"]).abs() / (yb + L.half_ulp_bf16(ymax))).max())
    _note(r, what)


@pytest.mark.parametrize("cols", L.COLS_F16X2)
def test_forward_f16x2_cols(ops, cols):
    """layernorm_fwd_f16x2_kernel<1> up to 512, <2> beyond, 8 channels per lane: both plane forms at every edge, ldy > cols."""
    rows = L.COL_SWEEP_ROWS
    for k, cls in enumerate(("n01", "n30", "zero_row")):
        x = L.make_rows(cls, rows, cols, 4000 + cols + k)
        gamma, beta = L.make_affine(cols, 4000 + cols)
        ref = L.fwd_ref64(x, gamma, beta, L.EPS[k % 2])
        what = "f16x2 cols %d %s" % (cols, cls)
        two = _fwd_f16x2(ops, x, gamma, beta, L.EPS[k % 2], ldy=cols + 8 * k, what=what)
        _check_f16x2(two, ref, True, what)
        one = _fwd_f16x2(ops, x, gamma, beta, L.EPS[k % 2], ldy=cols + 8 * k, two=False, what=what + " single")
        _check_f16x2(one, ref, False, what + " single")
        assert _same(one["bf"], two["bf"]) and _same(one["mean"], two["mean"]) and _same(one["rstd"], two["rstd"])


@pytest.mark.parametrize("rows", L.FWD_ROWS)
def test_forward_f16x2_rows(ops, rows):
    cols = 768
    x = L.make_rows("n300", rows, cols, 4100 + rows)
    gamma, beta = L.make_affine(cols, 4100)
    out = _fwd_f16x2(ops, x, gamma, beta, 1e-6, ldx=cols + 4, bf=False, what="f16x2 rows %d" % rows)
    ref = L.fwd_ref64(x, gamma, beta, 1e-6)
    r = L.fwd_ratios({"mean": out["mean"], "rstd": out["rstd"]}, ref)
    yb = L.K_Y * L.U * ref["s_y"]
    dec = out["y1"].double() + out["y2"].double()
    r["y_f16x2"] = float(((dec - ref["y"]).abs() / (yb + L.rep_bound_f16x2(ref["y"].abs() + yb))).max())
    _note(r, "f16x2 rows %d N(-300, 0.5^2)" % rows)


# ------------------------------------------------------------------------------------------------------------------------- backward
def _bwd(ops, dy, x, gamma, mean, rstd, *, add1=None, add2=None, dy_src="f32", lddy=None, ldx=None, lddx=None, planes=0, api="fmt",
         dx_init=None, dx_rows=None, cols_arg=None, fmt_arg=None, lo_arg=None, dy_f32_too=False, expect=0, what=""):
    """One backward on guarded buffers.  dy_src: 'f32' | 'bf16x2' (hi + lo planes of dy) | 'bf16' (hi alone) | 'f16' (one un-clamped
    fp16 plane, dx_fmt bit 1).  planes: 0 | 1 | 3 (split-bf16 planes of dx) | 4 (one un-clamped fp16 plane, dx_fmt bit 0).  api: 'fmt' |
    'bwd' (egv_layernorm_bwd, dx_fmt 0) | 'partial' (first stage only).  -> (outputs on the CPU, the fp32 dy the kernel decodes, the
    output Guarded of the fp32 streams)."""
    rows, cols = x.shape
    lddy = cols if lddy is None else lddy
    ldx = cols if ldx is None else ldx
    lddx = cols if lddx is None else lddx
    gi = L.Guarded(F32).add("x", rows, cols, ldx, x).add("gamma", 1, cols, data=gamma).add("mean", 1, rows, data=mean)
    gi.add("rstd", 1, rows, data=rstd)
    if dy_src == "f32" or dy_f32_too:
        gi.add("dy", rows, cols, lddy, dy)
    for name, a in (("add1", add1), ("add2", add2)):
        if a is not None:
            gi.add(name, rows, cols, lddx, a)
    gi.build(DEV)
    gib = gih = None
    dy_dec = dy
    if dy_src in ("bf16x2", "bf16"):
        hi, lo = L.split_bf16_ref(dy)
        gib = L.Guarded(BF16).add("dyh", rows, cols, lddy, hi).add("dyl", rows, cols, lddy, lo).build(DEV)
        dy_dec = hi.float() + lo.float() if dy_src == "bf16x2" else hi.float()
    elif dy_src == "f16":
        gih = L.Guarded(F16).add("dyh", rows, cols, lddy, dy.to(F16)).build(DEV)
        dy_dec = dy.to(F16).float()
    P = L.parts(rows)
    go = L.Guarded(F32)
    if dx_init is not None:
        go.add("dx", dx_rows, cols, data=dx_init)                # a pre-set [B S, D] buffer the kernel writes rows of (lddx = S D)
    else:
        go.add("dx", rows, cols, lddx)
    go.add("dgamma", 1, cols).add("dbeta", 1, cols).add("work", 1, 2 * cols * P).build(DEV)
    gpb = L.Guarded(BF16).add("hi", rows, cols).add("lo", rows, cols).build(DEV)          # the dx planes have ld = cols whatever lddx is
    gph = L.Guarded(F16).add("p", rows, cols).build(DEV)
    dyp = gi.ptr("dy") if (dy_src == "f32" or dy_f32_too) else None
    dyh = gib.ptr("dyh") if gib else (gih.ptr("dyh") if gih else None)
    dyl = gib.ptr("dyl") if dy_src == "bf16x2" else None
    dxh = gph.ptr("p") if planes == 4 else (gpb.ptr("hi") if planes else None)
    dxl = gpb.ptr("lo") if (planes == 3 or lo_arg) else None
    fmt = ((1 if planes == 4 else 0) | (2 if dy_src == "f16" else 0)) if fmt_arg is None else fmt_arg
    args = [dyp, dyh, dyl, lddy, gi.ptr("x"), ldx, gi.ptr("gamma"), gi.ptr("mean"), gi.ptr("rstd"), rows,
            cols if cols_arg is None else cols_arg, gi.ptr("add1") if add1 is not None else None,
            gi.ptr("add2") if add2 is not None else None, go.ptr("dx"), lddx, dxh, dxl]
    tail = [go.ptr("dgamma"), go.ptr("dbeta"), go.ptr("work"), ops._stream()]
    if api == "bwd":
        assert fmt == 0
        rc = _h().egv_layernorm_bwd(*args, *tail)
    else:
        rc = (_h().egv_layernorm_bwd_fmt if api == "fmt" else _h().egv_layernorm_bwd_partial)(*args, fmt, *tail)
    torch.cuda.synchronize()
    assert rc == expect, (what, rc)
    for g in (gi, gib, gih):
        if g is not None:
            g.assert_untouched(what)
    if expect:
        if dx_init is None:
            assert go.all_sentinel(), (what, "a refused call wrote")
        assert gpb.all_sentinel() and gph.all_sentinel(), (what, "a refused call wrote")
        return None, dy_dec, go
    for g in (go, gpb, gph):
        g.assert_intact(what)
    out = {"dx": go.get("dx"), "dgamma": go.get("dgamma")[0], "dbeta": go.get("dbeta")[0], "hi": gpb.get("hi"), "lo": gpb.get("lo"),
           "p16": gph.get("p")}
    if planes in (0, 4):
        assert gpb.all_sentinel(), (what, "bf16 planes written though not asked for")
    if planes == 1:
        assert _untouched(out["lo"]), (what, "lo written though NULL")
    if planes != 4:
        assert gph.all_sentinel(), (what, "fp16 plane written though not asked for")
    return out, dy_dec, go


def _check_planes(out, dx, planes, what):
    if planes in (1, 3):
        hi, lo = L.split_bf16_ref(dx)
        assert _same(out["hi"], hi), (what, "hi != bf16_rne(dx)")
        assert planes == 1 or _same(out["lo"], lo), (what, "lo != bf16_rne(dx - hi)")
    elif planes == 4:
        assert _same(out["p16"], dx.to(F16)), (what, "the fp16 plane is not the RNE fp16 of dx")


def _bwd_case(ops, rows, cols, cls, dcls, eps, seed, what, *, adds=2, dy_src="f32", planes=3, lddy=None, ldx=None, lddx=None, api="fmt"):
    x, dy = L.make_rows(cls, rows, cols, seed), L.make_rows(dcls, rows, cols, seed + 1)
    add1 = L.make_rows("n01", rows, cols, seed + 2) if adds >= 1 else None
    add2 = L.make_rows("n30", rows, cols, seed + 3) if adds >= 2 else None
    gamma, _ = L.make_affine(cols, seed)
    mean, rstd = L.stats_f32(x, eps)
    out, dy_dec, _ = _bwd(ops, dy, x, gamma, mean, rstd, add1=add1, add2=add2, dy_src=dy_src, planes=planes, lddy=lddy, ldx=ldx,
                          lddx=lddx, api=api, what=what)
    ref = L.bwd_ref64(dy_dec, x, gamma, mean, rstd, add1, add2)
    _note(L.bwd_ratios(out, ref, rows), what)
    _check_planes(out, out["dx"], planes, what)
    return out


@pytest.mark.parametrize("cols", L.ROW_SWEEP_COLS)
@pytest.mark.parametrize("rows", L.BWD_ROWS)
def test_backward_rows(ops, rows, cols):
    """The row loop and the second stage: 1 / 4 / 5 rows; parts 64 / 65 / 65 / 66 (one atomic per column, or two); parts 1023 / 1024; and
    the second sweep of `row += gridDim.x * 4` past 4096 rows -- one row of it, one full block, one more.  dgamma / dbeta held
    sentinels before the call: the kernel zeroes them itself."""
    assert _h().egv_layernorm_bwd_parts(rows) == L.parts(rows)
    i = L.BWD_ROWS.index(rows)
    cls = L.CLASSES[i % len(L.CLASSES)]
    _bwd_case(ops, rows, cols, cls, "n01" if cls == "zero_row" else cls, L.EPS[i % 2], 5000 + rows + cols,
              "bwd rows %d cols %d %s" % (rows, cols, cls), adds=i % 3, planes=(3, 1, 0)[i % 3])


@pytest.mark.parametrize("cols", L.COLS)
def test_backward_cols(ops, cols):
    """layernorm_bwd_kernel<NV> for NV = 1 .. 4, each partial and `full` (cols == NV * 256), with both addends and both planes."""
    assert L.nv_of(cols) == (cols // 4 + 63) // 64
    for k, cls in enumerate(("n01", "n30")):
        _bwd_case(ops, L.COL_SWEEP_ROWS, cols, cls, cls, L.EPS[k], 6000 + cols + k, "bwd cols %d %s" % (cols, cls))


@pytest.mark.parametrize("cls,dcls", [("n01", "n01"), ("n30", "n30"), ("n300", "n300"), ("outlier", "outlier"), ("zero_row", "n01"),
                                      ("n01", "zero_row"), ("n300", "n01")])
def test_backward_input_classes(ops, cls, dcls):
    for eps in L.EPS:
        for cols in (772, 768):
            _bwd_case(ops, 9, cols, cls, dcls, eps, 7000 + cols, "bwd class x %s dy %s eps %g cols %d" % (cls, dcls, eps, cols))


@pytest.mark.parametrize("dy_src", ["f32", "bf16x2", "bf16", "f16"])
@pytest.mark.parametrize("cols", [260, 768])
def test_backward_dy_sources_and_addends(ops, dy_src, cols):
    """dy as fp32, as split-bf16 planes with and without lo, as one un-clamped fp16 plane -- each against the reference fed the decoded
    dy, with lddy > cols (sentinels in the gaps: an over-read meets NaN) -- and add1 alone, add1 + add2, neither; egv_layernorm_bwd is
    egv_layernorm_bwd_fmt with dx_fmt 0."""
    for adds in (0, 1, 2):
        for planes in ((3, 4) if adds == 1 else (1,)):
            what = "bwd dy %s cols %d adds %d planes %d" % (dy_src, cols, adds, planes)
            out = _bwd_case(ops, 9, cols, "n01", "n01", 1e-6, 8000 + cols, what, adds=adds, dy_src=dy_src, planes=planes, lddy=cols + 8)
            if dy_src != "f16" and planes != 4:
                same = _bwd_case(ops, 9, cols, "n01", "n01", 1e-6, 8000 + cols, what + " egv_layernorm_bwd", adds=adds, dy_src=dy_src,
                                 planes=planes, lddy=cols + 8, api="bwd")
                assert all(_same(out[k], same[k]) for k in ("dx", "dgamma", "dbeta", "hi", "lo"))


def test_backward_fp16_plane_is_not_clamped(ops):
    """dx_fmt bit 0: the plane is the RNE fp16 of dx; 1e5 arriving through add1 reads +inf in the plane and stays finite in dx."""
    rows, cols = 9, 260
    x, dy, add1 = L.make_rows("n01", rows, cols, 1), L.make_rows("n01", rows, cols, 2), L.make_rows("n01", rows, cols, 3)
    add1[4, 17] = 1.0e5
    add1[5, 18] = -1.0e5
    gamma, _ = L.make_affine(cols, 4)
    mean, rstd = L.stats_f32(x, 1e-6)
    out, _, _ = _bwd(ops, dy, x, gamma, mean, rstd, add1=add1, planes=4, what="bwd fp16 plane overflow")
    _note(L.bwd_ratios(out, L.bwd_ref64(dy, x, gamma, mean, rstd, add1), rows), "bwd fp16 plane overflow")
    _check_planes(out, out["dx"], 4, "bwd fp16 plane overflow")
    assert float(out["p16"][4, 17]) == float("inf") and float(out["p16"][5, 18]) == float("-inf")
    assert bool(torch.isfinite(out["dx"]).all()) and float(out["dx"][4, 17]) > 9.0e4
    assert int(torch.isinf(out["p16"]).sum()) == 2


@pytest.mark.parametrize("cols", [64, 260, 768])
def test_backward_strided(ops, cols):
    """The strided backward.  (a) As _ClsNormFn.backward calls it: dx pre-zeroed [B S, D], rows = B, ldx = lddx = S D -- the rows other
    than the CLS rows stay exactly zero.  (b) ldx, lddx and lddy all different and > cols, add1 / add2 addressed with lddx and the dx
    planes with cols: a mix-up writes (or reads NaN) between the rows."""
    B, S = 5, 7
    x, dy = L.make_rows("n01", B, cols, 11), L.make_rows("n01", B, cols, 12)
    gamma, _ = L.make_affine(cols, 13)
    mean, rstd = L.stats_f32(x, 1e-6)
    out, _, _ = _bwd(ops, dy, x, gamma, mean, rstd, ldx=S * cols, lddx=S * cols, dx_init=torch.zeros(B * S, cols), dx_rows=B * S,
                     what="bwd cls rows cols %d" % cols)
    full = out["dx"].view(B, S, cols)
    assert bool((_bits(full[:, 1:]) == 0).all()), "rows other than the CLS rows were written"
    ref = L.bwd_ref64(dy, x, gamma, mean, rstd)
    _note(L.bwd_ratios({"dx": full[:, 0], "dgamma": out["dgamma"], "dbeta": out["dbeta"]}, ref, B), "bwd cls rows cols %d" % cols)
    _bwd_case(ops, 9, cols, "n01", "n01", 1e-6, 9000 + cols, "bwd strided cols %d" % cols, ldx=cols + 4, lddx=cols + 12, lddy=cols + 8)
    _bwd_case(ops, 9, cols, "n30", "n01", 1e-6, 9100 + cols, "bwd strided bf16 dy cols %d" % cols, ldx=3 * cols, lddx=2 * cols,
              lddy=cols + 4, dy_src="bf16x2")


@pytest.mark.parametrize("rows,cols", [(9, 768), (256, 260), (257, 260), (4101, 260)])
def test_backward_split_api(ops, rows, cols):
    """egv_layernorm_bwd_partial x 3 into three work buffers, then ONE egv_layernorm_bwd_reduce(3), and reduce(1) + reduce(2) (what
    csrc/block.hip does): each dgamma / dbeta inside its bound, dx final after the first stage, and for parts <= 64 bit-identical to
    egv_layernorm_bwd_fmt on the same inputs (one atomic onto the zero the first stage wrote)."""
    gamma, _ = L.make_affine(cols, 20)
    cases, parts = [], L.parts(rows)
    for j in range(3):
        x, dy = L.make_rows(("n01", "n30", "outlier")[j], rows, cols, 30 + j), L.make_rows("n01", rows, cols, 40 + j)
        mean, rstd = L.stats_f32(x, 1e-6)
        one, _, _ = _bwd(ops, dy, x, gamma, mean, rstd, what="split api: the one-call form %d" % j)
        part, _, go = _bwd(ops, dy, x, gamma, mean, rstd, api="partial", what="split api: partial %d" % j)
        assert _same(part["dx"], one["dx"]) and bool((_bits(part["dgamma"]) == 0).all()) and bool((_bits(part["dbeta"]) == 0).all())
        cases.append((go, one, L.bwd_ref64(dy, x, gamma, mean, rstd)))
    for counts in ((3,), (1, 2)):
        for go, _, _ in cases:                                          # back to what the first stage leaves
            go.arena.views[go.order.index("dgamma")].zero_()
            go.arena.views[go.order.index("dbeta")].zero_()
        first = 0
        for n in counts:
            sel = cases[first:first + n]
            rc = _h().egv_layernorm_bwd_reduce(n, _vp([c[0].ptr("work") for c in sel]), rows, cols, _vp([c[0].ptr("dgamma") for c in sel]),
                                               _vp([c[0].ptr("dbeta") for c in sel]), ops._stream())
            torch.cuda.synchronize()
            assert rc == 0
            first += n
        for j, (go, one, ref) in enumerate(cases):
            go.assert_intact("split api reduce %s" % (counts,))
            got = {"dgamma": go.get("dgamma")[0], "dbeta": go.get("dbeta")[0]}
            _note(L.bwd_ratios(got, ref, rows), "split api rows %d cols %d reduce%s entry %d" % (rows, cols, counts, j))
            if parts <= L.REDUCE_PARTS:
                assert _same(got["dgamma"], one["dgamma"]) and _same(got["dbeta"], one["dbeta"]), (rows, cols, counts, j)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(ops):
    """EGV_ERR_ARG with every output still holding its sentinels: nothing is launched."""
    cols = 1032
    x, dy = L.make_rows("n01", 5, cols, 1), L.make_rows("n01", 5, cols, 2)
    gamma, beta = L.make_affine(cols, 3)
    mean, rstd = L.stats_f32(x, 1e-6)
    for bad in (0, 6, 1028):
        _fwd(ops, x, gamma, beta, 1e-6, want_sum=True, cols_arg=bad, expect=ERR_ARG, what="fwd cols %d" % bad)
        _bwd(ops, dy, x, gamma, mean, rstd, cols_arg=bad, planes=3, expect=ERR_ARG, what="bwd cols %d" % bad)
    _fwd_f16x2(ops, x, gamma, beta, 1e-6, cols_arg=12, ldy_arg=16, expect=ERR_ARG, what="f16x2 cols 12")
    _fwd_f16x2(ops, x, gamma, beta, 1e-6, cols_arg=16, ldy_arg=12, expect=ERR_ARG, what="f16x2 ldy 12")
    _fwd_f16x2(ops, x, gamma, beta, 1e-6, cols_arg=1032, expect=ERR_ARG, what="f16x2 cols 1032")
    x, dy = x[:, :260].contiguous(), dy[:, :260].contiguous()
    gamma = gamma[:260].contiguous()
    _bwd(ops, dy, x, gamma, mean, rstd, planes=1, fmt_arg=1, lo_arg=True, expect=ERR_ARG, what="bwd dx_fmt 1 with a lo plane")
    _bwd(ops, dy, x, gamma, mean, rstd, dy_src="f32", fmt_arg=2, expect=ERR_ARG, what="bwd dx_fmt 2 with an fp32 dy")
    _bwd(ops, dy, x, gamma, mean, rstd, dy_src="f16", dy_f32_too=True, expect=ERR_ARG, what="bwd dx_fmt 2 with an fp32 dy next to the plane")
    go = L.Guarded(F32)
    for j in range(5):
        go.add("work%d" % j, 1, 2 * 260 * L.parts(5)).add("dg%d" % j, 1, 260).add("db%d" % j, 1, 260)
    go.build(DEV)
    ptrs = [_vp([go.ptr("%s%d" % (n, j)) for j in range(5)]) for n in ("work", "dg", "db")]
    for count in (0, 5):
        assert _h().egv_layernorm_bwd_reduce(count, ptrs[0], 5, 260, ptrs[1], ptrs[2], ops._stream()) == ERR_ARG
        torch.cuda.synchronize()
        assert go.all_sentinel(), "reduce count %d wrote" % count


# ------------------------------------------------------------------------------------------------------------------------- wrappers
def test_python_wrappers_hand_the_strides_over(ops):
    """ops.layernorm_fwd / ops.layernorm_bwd: want_sum, x_add, add2, rows / ldx / dx / lddx and planes_passes 1 / 3 / 4 reach the C
    calls as they expect them."""
    B, S, D = 5, 7, 264                     # % 8: the fp16 plane of planes_passes 4 comes in 16-byte pieces
    g = torch.Generator().manual_seed(5)
    x3, xa3 = torch.randn(B, S, D, generator=g) + 3.0, torch.randn(B, S, D, generator=g)
    gamma, beta = L.make_affine(D, 6)
    xc, xac, gc, bc = x3.to(DEV), xa3.to(DEV), gamma.to(DEV), beta.to(DEV)
    pl, yf, mean, rstd, s = ops.layernorm_fwd(xc.view(B * S, D), gc, bc, 1e-6, 3, x_add=xac.view(B * S, D), want_sum=True, want_f32=True)
    ref = L.fwd_ref64(x3.view(B * S, D), gamma, beta, 1e-6, x_add=xa3.view(B * S, D))
    assert _same(s.cpu(), ref["sum"])
    _note(L.fwd_ratios({"y": yf.cpu(), "mean": mean.cpu(), "rstd": rstd.cpu()}, ref), "wrapper fwd")
    hi, lo = L.split_bf16_ref(yf.cpu())
    assert _same(pl.hi.cpu(), hi) and _same(pl.lo.cpu(), lo)
    _, ycls, mcls, rcls, _ = ops.layernorm_fwd(xc.view(B * S, D), gc, bc, 1e-6, 1, want_f32=True, want_planes=False, rows=B, ldx=S * D)
    rcl = L.fwd_ref64(x3[:, 0].contiguous(), gamma, beta, 1e-6)
    _note(L.fwd_ratios({"y": ycls.cpu(), "mean": mcls.cpu(), "rstd": rcls.cpu()}, rcl), "wrapper fwd cls rows")
    # backward on the CLS rows into a pre-zeroed [B S, D] buffer
    dy = torch.randn(B, D, generator=g)
    dx = torch.zeros(B * S, D, device=DEV)
    got = ops.layernorm_bwd(dy.to(DEV), xc.view(B * S, D), gc, mcls, rcls, rows=B, ldx=S * D, dx=dx, lddx=S * D)
    rb = L.bwd_ref64(dy, x3[:, 0].contiguous(), gamma, mcls.cpu(), rcls.cpu())
    full = dx.cpu().view(B, S, D)
    assert got[0] is dx and bool((_bits(full[:, 1:]) == 0).all())
    _note(L.bwd_ratios({"dx": full[:, 0], "dgamma": got[1].cpu(), "dbeta": got[2].cpu()}, rb, B), "wrapper bwd cls rows")
    # add1 + add2 and the plane forms
    x2, dy2 = x3.view(B * S, D), torch.randn(B * S, D, generator=g)
    a1, a2 = torch.randn(B * S, D, generator=g), torch.randn(B * S, D, generator=g)
    m2, r2 = L.stats_f32(x2, 1e-6)
    rb2 = L.bwd_ref64(dy2, x2, gamma, m2, r2, a1, a2)
    for passes in (1, 3, 4):
        dxp, dg, db, plb = ops.layernorm_bwd(dy2.to(DEV), xc.view(B * S, D), gc, m2.to(DEV), r2.to(DEV), add1=a1.to(DEV), add2=a2.to(DEV),
                                             planes_passes=passes)
        _note(L.bwd_ratios({"dx": dxp.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}, rb2, B * S), "wrapper bwd planes_passes %d" % passes)
        out = {"hi": plb.hi.cpu(), "lo": plb.lo.cpu() if plb.lo is not None else None, "p16": plb.hi.cpu()}
        _check_planes(out, dxp.cpu(), passes, "wrapper planes_passes %d" % passes)
        assert (plb.lo is None) == (passes != 3)
