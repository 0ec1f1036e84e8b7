"""What the attention entry points accept and what they launch, restated in Python from the launchers as they stood before
csrc/attn_dispatch.h: one `if` ladder per direction and file, the way egv_divided_attn_fwd / _bwd, egv_text_attn_fwd / _bwd, launch_fwd /
launch_bwd (attn_mfma_fwd.hip, attn_mfma_bwd.hip), egv_attn_long_fwd / _bwd and the two time files wrote them.  The header states each
rule once; this file deliberately does not share its shape.  Three rules are the header's own and are marked NEW: every block count is
computed exactly and refused past 2^31 - 1, S = 1 + T n has to fit an int, and the text backward refuses non-positive sizes.

A check returns None (EGV_ERR_ARG) or the tuple the driver prints; a pick returns None or
(family, frags, products, f16, waves, threads, lds, grid, nblk)."""

MAX_GRID = 2 ** 31 - 1
RESIDENT, STREAM, TEXT_STREAM, KEY_TILED, TIME_TILE, TIME_LONG = range(6)
ROW = 128                                               # bytes of a 64-element bf16 row in LDS


# ------------------------------------------------------------------------------------------------------------------------- checks
def check_divided_fwd(B, T, n, H, mode, passes, required, qkv_lo, out_lo):
    if not required or B <= 0 or T <= 0 or n <= 0 or H <= 0:
        return None
    if passes not in (1, 3):
        return None
    if mode < 0 or mode > 15:
        return None
    out_fmt, f16, time = (mode >> 1) & 3, (mode >> 3) & 1, mode & 1
    if f16 and passes != 3:
        return None
    if out_fmt and passes != 3:
        return None
    if out_fmt == 3:
        out_lo = False
    if passes == 3 and ((not out_lo and out_fmt != 3) or not qkv_lo):
        return None
    if passes == 1:
        qkv_lo = out_lo = False
    if time and T > 64:                                 # egv_attn_time_fwd_impl
        return None
    if time and not qkv_lo:                             # the time launch_fwd: the one-product kernel is given out_fmt 0
        out_fmt = 0
    if T * n + 1 > 2 ** 31 - 1 or B * H > MAX_GRID:     # NEW
        return None
    return (time, out_fmt, f16, int(qkv_lo), int(out_lo))


def check_divided_bwd(B, T, n, H, mode, passes, required, qkv_lo, out_lo, dout_lo, dqkv_lo):
    if not required or B <= 0 or T <= 0 or n <= 0 or H <= 0:
        return None
    if passes not in (1, 3):
        return None
    if mode < 0 or mode > 31:
        return None
    o_fmt, g_fmt, f16, time = (mode >> 1) & 3, (4 if mode & 8 else 0), (mode >> 4) & 1, mode & 1
    if f16 and (passes != 1 or not g_fmt):
        return None
    if (o_fmt >= 2 or g_fmt) and passes != 1:
        return None
    if o_fmt:
        out_lo = False
    if passes == 3 and (not qkv_lo or (not out_lo and o_fmt == 0) or not dout_lo or not dqkv_lo):
        return None
    if passes == 1:
        qkv_lo = dout_lo = dqkv_lo = False
    if time and T > 64:                                 # egv_attn_time_bwd_impl -- behind the CLS delta kernel, before this change
        return None
    if T * n + 1 > 2 ** 31 - 1 or B * H > MAX_GRID:     # NEW
        return None
    return (time, o_fmt, g_fmt, f16, int(qkv_lo), int(out_lo), int(dout_lo), int(dqkv_lo))


def check_text_fwd(B, L, H, passes, required, out_lo, ldqkv, p):
    if not required or B <= 0 or L <= 0 or H <= 0:
        return None
    if passes not in (1, 3):
        return None
    if passes == 3 and not out_lo:
        return None
    if ldqkv < H * 64 or ldqkv % 4 != 0:
        return None
    if not (0.0 <= p < 1.0):
        return None
    return (int(out_lo and passes == 3),)               # launch_fwd hands the one-product kernel no second plane


def check_text_bwd(B, L, H, passes, required, ldqkv, lddqkv, p):
    if not required:
        return None
    if passes not in (1, 3):
        return None
    if ldqkv < H * 64 or lddqkv < H * 64 or ldqkv % 4 != 0 or lddqkv % 4 != 0:
        return None
    if not (0.0 <= p < 1.0):
        return None
    if B <= 0 or L <= 0 or H <= 0:                      # NEW
        return None
    return ()


# -------------------------------------------------------------------------------------------------------------------------- picks
def _pick(family, frags, products, f16, threads, lds, grid, nblk=1):
    if grid < 1 or grid > MAX_GRID:                     # NEW on the LDS-resident and the T <= 16 paths
        return None
    return (family, frags, products, f16, threads // 64, threads, lds, grid, nblk)


def _long_buf_bytes(passes, nvec):
    return (4 if passes == 3 else 2) * 64 * ROW + nvec * 64 * 4


def pick_fwd(space, groups, nq, nk, passes, f16):
    """dispatch_fwd -> launch_fwd<MODE, NKF> | egv_attn_long_fwd -> launch_long_fwd.  nq counts the CLS query in space mode."""
    if groups < 1 or groups > MAX_GRID:                 # NEW: `ngroups` is an int
        return None
    for limit, nkf in ((32, 2), (64, 4), (224, 14), (288, 18)):
        if nk <= limit:
            break
    else:
        nqb = (nq + 127) // 128
        return _pick(KEY_TILED, 0, passes, f16, 512, 2 * _long_buf_bytes(passes, 1), groups * nqb, nqb)
    planes = 4 if passes == 3 else 2
    lds = planes * nkf * 16 * ROW + nkf * 16 * 4
    if space and nkf in (14, 18):
        if passes == 3:
            return _pick(STREAM, nkf, 3, f16, 1024, lds, min(groups, 256))
        return _pick(RESIDENT, nkf, 1, f16, 512, lds, groups)
    return _pick(RESIDENT, nkf, passes, f16, 512, lds, groups)


def pick_bwd(space, groups, nq, nk, passes, f16):
    """dispatch_bwd -> launch_bwd<MODE, NF> | egv_attn_long_bwd -> launch_long_bwd: (dQ pick, dK / dV pick)."""
    m = max(nk, nq)
    if m <= 32:
        nf = 2
    elif m <= 64:
        nf = 4
    elif m <= 224:
        nf = 14
    elif m <= 288:
        nf = 18
    else:
        nqb, nkb = (nq + 127) // 128, (nk + 127) // 128
        return (_pick(KEY_TILED, 0, passes, f16, 512, 2 * _long_buf_bytes(passes, 1), groups * nqb, nqb),
                _pick(KEY_TILED, 0, passes, f16, 512, 2 * _long_buf_bytes(passes, 2), groups * nkb, nkb))
    planes = 4 if passes == 3 else 2
    lds = planes * nf * 16 * ROW + 2 * nf * 16 * 4
    if space and nf in (14, 18):
        lds1 = planes * nf * 16 * ROW + nf * 16 * 4
        if passes == 3:
            return _pick(STREAM, nf, 3, f16, 1024, lds1, groups), _pick(RESIDENT, nf, 3, f16, 256, lds, groups)
        return _pick(STREAM, nf, 1, f16, 512, lds1, groups), _pick(RESIDENT, nf, 1, f16, 512, lds, groups)
    if nf in (14, 18):
        if passes == 3:
            return _pick(TEXT_STREAM, nf, 3, f16, 512, lds, groups), _pick(RESIDENT, nf, 3, f16, 256, lds, groups)
        return _pick(TEXT_STREAM, nf, 1, f16, 512, lds, groups), _pick(RESIDENT, nf, 1, f16, 512, lds, groups)
    if passes == 3:
        return _pick(RESIDENT, nf, 3, f16, 256, lds, groups), _pick(RESIDENT, nf, 3, f16, 256, lds, groups)
    return _pick(RESIDENT, nf, 1, f16, 512, lds, groups), _pick(RESIDENT, nf, 1, f16, 512, lds, groups)


def pick_time(bwd, B, T, n, H, passes, f16):
    """egv_attn_time_*_impl (attn_small.hip) -> attn_time_mfma.hip launch_*<TP> | attn_time_long.hip launch_*<NT>."""
    if T < 1 or T > 64:
        return None
    if T > 16:
        nt = 2 if T <= 32 else 3 if T <= 48 else 4
        return _pick(TIME_LONG, nt, passes, f16, 64 * nt, 0, B * n * H)
    tp = 4 if T <= 4 else 8 if T <= 8 else 16
    locs = 16 // tp
    units = (n + locs - 1) // locs
    if not bwd:
        return _pick(TIME_TILE, tp, passes, f16, 256, 0, (B * units * H + 3) // 4)
    if passes == 3:
        return _pick(TIME_TILE, tp, 3, f16, 128, 0, B * H * ((units + 1) // 2))
    return _pick(TIME_TILE, tp, 1, f16, 256, 0, B * H * ((units + 3) // 4))


# --------------------------------------------------------------------------------------------------------------------------- lines
def line(result):
    """What the driver prints for one case."""
    if result is None:
        return "1"
    return " ".join(["0"] + [str(int(x)) for x in result])


def expected(case):
    kind, args = case[0], case[1:]
    if kind == "pick_dq":
        r = pick_bwd(*args)[0]
    elif kind == "pick_dkv":
        r = pick_bwd(*args)[1]
    else:
        r = {"check_dfwd": check_divided_fwd, "check_dbwd": check_divided_bwd, "check_tfwd": check_text_fwd, "check_tbwd": check_text_bwd,
             "pick_fwd": pick_fwd, "pick_time": pick_time}[kind](*args)
    return line(r)
