"""A refused attention call enqueues nothing: egv_divided_attn_fwd / _bwd called through the C ABI with every output and workspace
buffer holding a sentinel; the call returns EGV_ERR_ARG and every buffer is bit-intact after a synchronize.  (Before
csrc/attn_dispatch.h the time backward at T > 64 ran the CLS delta kernel -- which writes delta and zeroes dcls in `work` -- and
only then looked at T.)  B = 1, H = 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from egovlp_amd import _lib  # noqa: E402
from egovlp_amd.ops import _p, _stream  # noqa: E402

EGV_ERR_ARG = 1
SENTINEL = 0x5A5A5A5A


def _buf(nbytes, value=SENTINEL):
    return torch.full(((nbytes + 3) // 4,), value, dtype=torch.int32, device="cuda")


def _call(direction, T, n, mode, passes, missing=()):
    """One call with every plane present except `missing`; -> (rc, {name: (buffer, copy made before the call)})."""
    B = H = 1
    S = 1 + T * n
    lib = _lib.lib()
    bufs = {"qkv_hi": _buf(S * 192 * 2, 0), "qkv_lo": _buf(S * 192 * 2, 0), "out_hi": _buf(S * 64 * 2), "out_lo": _buf(S * 64 * 2),
            "lse": _buf(S * 4)}
    if direction == "fwd":
        bufs["work"] = _buf(4 * lib.egv_divided_attn_fwd_work_floats(B, T, n, H, mode & 1))
    else:
        bufs.update({"dout_hi": _buf(S * 64 * 2, 0), "dout_lo": _buf(S * 64 * 2, 0), "dqkv_hi": _buf(S * 192 * 2), "dqkv_lo": _buf(S * 192 * 2),
                     "work": _buf(4 * lib.egv_divided_attn_bwd_work_floats(B, T, n, H))})
    before = {k: v.clone() for k, v in bufs.items()}
    a = {k: (None if k in missing else _p(v)) for k, v in bufs.items()}
    s = _stream(bufs["qkv_hi"])
    if direction == "fwd":
        rc = lib.egv_divided_attn_fwd(a["qkv_hi"], a["qkv_lo"], B, T, n, H, mode, passes, a["out_hi"], a["out_lo"], a["lse"], a["work"], s)
    else:
        rc = lib.egv_divided_attn_bwd(a["qkv_hi"], a["qkv_lo"], a["out_hi"], a["out_lo"], a["dout_hi"], a["dout_lo"], a["lse"], B, T, n, H,
                                      mode, passes, a["dqkv_hi"], a["dqkv_lo"], a["work"], s)
    torch.cuda.synchronize()
    return rc, {k: (bufs[k], before[k]) for k in bufs}


REFUSED = [
    ("time-backward-65-frames", "bwd", 65, 1, 1, 1, ()),
    ("time-backward-65-frames-three-products", "bwd", 65, 1, 1, 3, ()),
    ("time-forward-65-frames", "fwd", 65, 1, 1, 3, ()),
    ("time-forward-65-frames-one-product", "fwd", 65, 1, 1, 1, ()),
    ("fp16-operands-one-product-forward", "fwd", 2, 3, 8, 1, ()),
    ("fp16-operands-one-product-time-forward", "fwd", 2, 3, 9, 1, ()),
    ("output-format-1-one-product-forward", "fwd", 2, 3, 2, 1, ()),
    ("output-format-3-one-product-forward", "fwd", 2, 3, 6, 1, ()),
    ("three-products-no-out-lo-n64-streaming", "fwd", 1, 64, 0, 3, ("out_lo",)),
    ("three-products-no-out-lo-n224-streaming", "fwd", 1, 224, 0, 3, ("out_lo",)),
    ("three-products-no-out-lo-n288-key-tiled", "fwd", 1, 288, 0, 3, ("out_lo",)),
    ("backward-bit4-without-bit3", "bwd", 2, 3, 16, 1, ()),
    ("backward-bit4-without-bit3-time", "bwd", 2, 3, 17, 1, ()),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_call_enqueues_nothing(case):
    _, direction, T, n, mode, passes, missing = case
    rc, bufs = _call(direction, T, n, mode, passes, missing)
    assert rc == EGV_ERR_ARG
    for name, (now, before) in bufs.items():
        assert torch.equal(now, before), name


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_accepted_call_writes_its_outputs(direction):
    """The harness above passes the arguments where the entry points expect them: the neighbouring valid call returns 0 and leaves no
    sentinel in its output plane."""
    rc, bufs = _call(direction, 2, 3, 1, 1)
    assert rc == 0
    now, before = bufs["out_hi" if direction == "fwd" else "dqkv_hi"]
    assert not bool((now == SENTINEL).any()) and bool((before == SENTINEL).all())
    for name in ("qkv_hi", "qkv_lo", "out_lo" if direction == "fwd" else "dqkv_lo"):       # inputs, and the plane a one-product call does not have
        assert torch.equal(*bufs[name]), name
