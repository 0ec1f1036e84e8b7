"""A refused GEMM call enqueues nothing: egv_gemm_nt called through the C ABI with every output, `partial` and `colsum` buffer holding a
sentinel; the call returns EGV_ERR_ARG and every buffer is bit-intact after a synchronize.  (Before csrc/gemm_dispatch.h four
split-K rules were looked at behind the kernel's launch: the refused call had already written its `partial` slab.  Run against that
library, the first four cases below fail on `partial`; the other seven and the accepted call pass.)"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from egovlp_amd import _lib  # noqa: E402
from egovlp_amd.ops import _p, _stream  # noqa: E402

EGV_ERR_ARG = 1
SENTINEL = 0x5A5A5A5A
OPERANDS = ("a_hi", "a_lo", "b_hi", "b_lo")


def _buf(nbytes, value=SENTINEL):
    return torch.full(((nbytes + 3) // 4,), value, dtype=torch.int32, device="cuda")


def _call(M, N, K, passes=1, trans=0, ksplit=1, accumulate=0, ldo=None, outputs=("out_f32",), aux_bf16=0, out_fmt=0, grid_cap=0):
    """One call: zero operands, `outputs` (and `partial` under split-K) passed, every output buffer there and holding the sentinel, each
    as large as the kernels of the call could write it.  -> (rc, {name: (buffer, copy made before the call)})."""
    ldo = N if ldo is None else ldo
    ks = max(ksplit, 1)
    bufs = {k: _buf(M * K * 2, 0) for k in OPERANDS[:2]}
    bufs.update({k: _buf(N * K * 2, 0) for k in OPERANDS[2:]})
    bufs.update({"out_f32": _buf(M * ldo * 4), "out_hi": _buf(M * N * 2), "out_lo": _buf(M * N * 2), "aux_out": _buf(M * N * 4),
                 "partial": _buf((ks * M * N + ks * M) * 4), "colsum": _buf(M * 4)})
    before = {k: v.clone() for k, v in bufs.items()}
    given = set(OPERANDS) | set(outputs) | ({"partial"} if ks > 1 else set())
    a = {k: (_p(v) if k in given else None) for k, v in bufs.items()}
    d = _lib.GemmDesc(a["a_hi"], a["a_lo"], (M if trans else K), a["b_hi"], a["b_lo"], (N if trans else K), M, N, K, passes, 1.0, 0, None,
                      None, 0, None, a["aux_out"], N, a["out_f32"], ldo, a["out_hi"], a["out_lo"], N, ksplit, accumulate, a["partial"],
                      trans, aux_bf16, a["colsum"], grid_cap, out_fmt, None)
    rc = _lib.lib().egv_gemm_nt(C.byref(d), _stream(bufs["a_hi"]))
    torch.cuda.synchronize()
    return rc, {k: (bufs[k], before[k]) for k in bufs}


REFUSED = [
    # the parent launched the kernel, which wrote `partial`, and refused behind it
    ("small-split-k-accumulate", dict(M=128, N=128, K=64, ksplit=2, accumulate=1)),
    ("tn-split-k-padded-ldo", dict(M=256, N=256, K=128, trans=1, ksplit=2, ldo=264)),
    ("tn-split-k-padded-ldo-slabs-left", dict(M=256, N=256, K=128, trans=1, ksplit=2, ldo=264, accumulate=2)),
    ("big-split-k-without-out-f32", dict(M=256, N=256, K=8192, ksplit=128, outputs=("out_hi",))),
    # refused before any launch then as now
    ("f16x2-split-k", dict(M=256, N=256, K=64, passes=2, ksplit=2)),
    ("fp16-planes-of-a-bf16x3-product", dict(M=256, N=256, K=64, passes=3, out_fmt=1, outputs=("out_hi", "out_lo"))),
    ("bf16-aux-on-the-small-kernel", dict(M=128, N=128, K=64, aux_bf16=1, outputs=("out_f32", "aux_out"))),
    ("grid-cap-12", dict(M=256, N=256, K=64, grid_cap=12)),
    ("k-48", dict(M=128, N=128, K=48)),
    ("fp16-nt-split-k", dict(M=256, N=256, K=64, passes=4, ksplit=2)),
    ("tn-m-248", dict(M=248, N=256, K=128, trans=1)),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_call_enqueues_nothing(case):
    rc, bufs = _call(**case[1])
    assert rc == EGV_ERR_ARG
    for name, (now, before) in bufs.items():
        assert torch.equal(now, before), name


def test_accepted_call_writes_its_outputs():
    """The harness above passes the arguments where egv_gemm_nt expects them and sees a write: the first refused case without its
    `accumulate` returns 0, overwrites out_f32 and the slabs, and leaves the buffers it was not given alone."""
    rc, bufs = _call(M=128, N=128, K=64, ksplit=2, accumulate=0)
    assert rc == 0
    for name in ("out_f32", "partial"):
        now, before = bufs[name]
        assert bool((before == SENTINEL).all()) and bool((now[:128 * 128] == 0).all()), name
    for name in OPERANDS + ("out_hi", "out_lo", "aux_out", "colsum"):
        assert torch.equal(*bufs[name]), name
