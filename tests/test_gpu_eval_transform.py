"""egv_patch_gather_u8_eval on a real MI355X (`pytest -m gpu`): the loader's val / test transform (Resize(S) -> CenterCrop(S) ->
Resize(R) -> Normalize on x / 255, data_loader/transforms.py:49-60; bilinear, align_corners = False, no antialias) fused into the
patch gather, against the same transform written out with torch on the CPU.

Tolerance.  The fp32 oracle is not exact: its source coordinate (dst + 0.5) * scale - 0.5 is an fp32 number of up to a few hundred
(ulp 3e-5), so an interpolation weight carries that error and a pixel moves by up to weight error * neighbour difference / std.  The
fp32 oracle differs from the same transform in fp64 by ~1e-4 at 256 x 341 -> 224 on noise frames; a per-element cap against the
fp32 oracle cannot tell a wrong kernel from another rounding.  So every case also computes the fp64 oracle and requires

    max |kernel - oracle64| <= 2 * max |oracle32 - oracle64|      and      mean |kernel - oracle64| <= 2 * mean |oracle32 - oracle64|

(an fp32 evaluation in another order adds at most its own rounding to the reference's).  oracle32 ends with the plain fp32
`ops.patch_gather`, so both sides carry the same split-bf16 plane rounding.  For the hi-only plane the bf16 step 2e-2 applies, as in
the train-transform test (tests/test_gpu_ops.py).  The four numbers of every case are printed."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from egovlp_amd.data_loader.transforms import eval_transform_geometry  # noqa: E402

# (Hs, Ws, S, R for P = 16, R for P = 14)
SOURCES = {"256x341_identity": (256, 341, 256, 224, 224), "270x480_landscape": (270, 480, 256, 224, 224),
           "480x270_portrait": (480, 270, 256, 224, 224), "180x240_upscale": (180, 240, 256, 224, 224),
           "45x80_toy": (45, 80, 40, 32, 28)}
BANK = 8
# repeated, out-of-order and overlapping-window entries: three windows of four
TABLE = [7, 7, 0, 3, 1, 2, 3, 4, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


def host_transform(u8, S, R, dtype, mean, std):
    """init_video_transform_dict()['test'] on [N, C, Hs, Ws] uint8 frames, in `dtype`"""
    H1, W1, top, left = eval_transform_geometry(u8.shape[-2], u8.shape[-1], S)
    x = u8.to(dtype) / 255
    x = F.interpolate(x, size=(H1, W1), mode="bilinear", align_corners=False)
    x = x[:, :, top:top + S, left:left + S]
    x = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False)
    m = torch.tensor(mean, dtype=dtype).view(1, -1, 1, 1)
    s = torch.tensor(std, dtype=dtype).view(1, -1, 1, 1)
    return (x - m) / s


def im2col(x, P):
    """[N, C, R, R] -> [N * (R/P)^2, C*P*P], rows (frame, patch row, patch column), columns (channel, row, column in the patch)"""
    N, Cc, R, _ = x.shape
    g = R // P
    return x.view(N, Cc, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, Cc * P * P)


def noise_bank(Hs, Ws, seed):
    return torch.randint(0, 256, (BANK, 3, Hs, Ws), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def smooth_bank(Hs, Ws, seed):
    """a low-frequency ramp plus small noise: a wrong tap or a shifted crop is a LARGE error here, not one drowned in noise"""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, Hs).view(1, 1, Hs, 1)
    xx = torch.linspace(0, 1, Ws).view(1, 1, 1, Ws)
    phase = torch.rand(BANK, 3, 1, 1, generator=g)
    img = 128 + 90 * torch.sin(6.28318 * (0.7 * yy + 1.3 * xx + phase)) + 20 * (xx - yy)
    img = img + torch.randint(-3, 4, (BANK, 3, Hs, Ws), generator=g)
    return img.round().clamp(0, 255).to(torch.uint8)


def check_case(ops, name, bank, S, R, P, table):
    mean, std = ops.IMAGENET_MEAN, ops.IMAGENET_STD
    sel = list(range(BANK)) if table is None else table
    K = 3 * P * P
    o64 = im2col(host_transform(bank, S, R, torch.float64, mean, std), P).view(BANK, -1, K)[sel].reshape(-1, K)
    host32 = host_transform(bank, S, R, torch.float32, mean, std)[sel]                     # [BT, C, R, R]
    o32 = ops.patch_gather(host32.view(-1, 4, *host32.shape[1:]).cuda().contiguous(), P, 3).float().cpu()[:, :K].double()
    index = None if table is None else torch.tensor(table, dtype=torch.int32).cuda()
    got = ops.patch_gather_eval(bank.cuda(), index, 4, P, 3, S, R, mean, std)
    got1 = ops.patch_gather_eval(bank.cuda(), index, 4, P, 1, S, R, mean, std)
    torch.cuda.synchronize()
    assert got.rows == o64.shape[0] and got.cols == (K + 63) // 64 * 64 and got.lo is not None
    full = got.float().cpu()
    if got.cols > K:
        assert float(full[:, K:].abs().max()) == 0.0                                       # the k-tile pad stays zero
    e_ref = (o32 - o64).abs()
    e_k = (full[:, :K].double() - o64).abs()
    print("eval transform %-18s P=%d %s: e_ref max %.3e mean %.3e | e_k max %.3e mean %.3e"
          % (name, P, "table" if table is not None else "plain", float(e_ref.max()), float(e_ref.mean()), float(e_k.max()),
             float(e_k.mean())))
    assert float(e_k.max()) <= 2 * float(e_ref.max()), (name, P, float(e_k.max()), float(e_ref.max()))
    assert float(e_k.mean()) <= 2 * float(e_ref.mean()), (name, P, float(e_k.mean()), float(e_ref.mean()))
    # one plane: bf16 rounding of the same values
    assert got1.lo is None and float((got1.float().cpu()[:, :K].double() - o64).abs().max()) < 2e-2


@pytest.mark.parametrize("table", [None, TABLE], ids=["plain", "table"])
@pytest.mark.parametrize("P", [16, 14])
@pytest.mark.parametrize("name", list(SOURCES))
def test_fused_eval_transform_matches_the_host_transform(ops, name, P, table):
    """Measured on MI355X (noise frames; P = 14 and the table variants agree to the digits shown except at the toy size, where
    P = 14 means R = 28: 1.790e-05 / 1.967e-06 on both sides):
        source               e_ref max   e_ref mean   e_k max     e_k mean
        256x341_identity     1.280e-04   1.131e-05    1.280e-04   1.131e-05
        270x480_landscape    1.577e-04   1.365e-05    1.577e-04   1.365e-05
        480x270_portrait     1.562e-04   1.365e-05    1.562e-04   1.365e-05
        180x240_upscale      7.257e-05   5.921e-06    7.257e-05   5.921e-06
        45x80_toy            1.599e-05   1.635e-06    1.599e-05   1.635e-06"""
    Hs, Ws, S, R16, R14 = SOURCES[name]
    check_case(ops, name, noise_bank(Hs, Ws, 11), S, R16 if P == 16 else R14, P, table)


@pytest.mark.parametrize("name", ["256x341_identity", "270x480_landscape", "480x270_portrait", "180x240_upscale"])
def test_fused_eval_transform_on_a_smooth_image(ops, name):
    Hs, Ws, S, R16, _ = SOURCES[name]
    check_case(ops, name + "_smooth", smooth_bank(Hs, Ws, 12), S, R16, 16, TABLE)


def test_a_one_pixel_source_is_read_inside_the_bank(ops):
    """Hs = Ws = 1: every tap of both stages is the one source pixel.  Each output equals (p / 255 - mean) / std up to the two
    interpolations' rounding (two bilinear blends of equal values: <= 4 ulp of a value <= 1, 5e-7, / std >= 0.224 -> 2e-6) and the
    split-bf16 plane step (2^-17 relative of |v| <= 2.7: 2e-5): bound 3e-5."""
    bank = torch.tensor([0, 255, 37, 128, 200, 91, 5, 250, 64, 13, 99, 180], dtype=torch.uint8).view(4, 3, 1, 1)
    got = ops.patch_gather_eval(bank.cuda(), None, 4, 16, 3, 40, 32).float().cpu()
    torch.cuda.synchronize()
    mean, std = torch.tensor(ops.IMAGENET_MEAN, dtype=torch.float64), torch.tensor(ops.IMAGENET_STD, dtype=torch.float64)
    want = ((bank.double().view(4, 3) / 255 - mean) / std).view(4, 1, 3, 1).expand(4, 4, 3, 256).reshape(16, 768)
    assert float((got.double() - want).abs().max()) < 3e-5


def test_table_entries_outside_the_bank_are_clamped_in_the_kernel_and_refused_on_the_host(ops):
    Hs, Ws, S, R = 45, 80, 40, 32
    bank = noise_bank(Hs, Ws, 13).cuda()
    bad = torch.tensor([-5, BANK + 7, 2, 3, 0, 1, BANK, -1], dtype=torch.int32)
    clamped = bad.clamp(0, BANK - 1)
    a = ops.patch_gather_eval(bank, bad.cuda(), 4, 16, 3, S, R)
    b = ops.patch_gather_eval(bank, clamped.cuda(), 4, 16, 3, S, R)
    torch.cuda.synchronize()
    assert torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)
    with pytest.raises(ValueError):
        ops.patch_gather_eval(bank, bad, 4, 16, 3, S, R)                       # the host can see this table: refused
    with pytest.raises(ValueError):
        ops.patch_gather_eval(bank.float(), None, 4, 16, 3, S, R)


def test_launcher_refuses_what_it_cannot_do(ops):
    from egovlp_amd import _lib
    lib = _lib.lib()
    bank = noise_bank(45, 80, 14).cuda()
    pl = ops.empty_planes(BANK * 4, 768, 3, bank.device)
    mean, std = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5), (C.c_float * 4)(0.25, 0.25, 0.25, 0.25)
    st = ops._stream(bank)

    def call(F_=BANK, BT=BANK, Cc=3, Hs=45, Ws=80, S=40, R=32, P=16, frames=bank.data_ptr(), hi=pl.hi.data_ptr(), lda=768, sd=std):
        return lib.egv_patch_gather_u8_eval(frames, F_, None, BT, Cc, Hs, Ws, S, R, P, mean, sd, hi, pl.lo.data_ptr(), lda, st)

    assert call() == 0
    assert call(R=40) == 1                 # R % P != 0
    assert call(R=30, P=10) == 1           # R % 4 != 0
    assert call(Cc=5) == 1                 # C > 4
    assert call(F_=0) == 1 and call(F_=-3) == 1
    assert call(BT=BANK + 1) == 1          # index == NULL reads frame bt: more output frames than the bank holds
    assert call(BT=0) == 1 and call(Hs=0) == 1 and call(Ws=-1) == 1 and call(S=0) == 1
    assert call(frames=None) == 1 and call(hi=None) == 1
    assert call(lda=512) == 1              # narrower than K = 768
    assert call(sd=(C.c_float * 4)(0.25, 0.0, 0.25, 0.25)) == 1
    torch.cuda.synchronize()
