"""egv_gemm_nt element by element: every case of tests/gemm_ref.py -- one per instance of the big kernel, the small kernel, every
split-K reduce, the tile, stride and k-slice edges -- called through the C ABI on guarded buffers and compared with the reference, bit
for bit wherever the inputs make every sum exact and within a derived element-wise bound where they do not (gemm_ref's docstring).

Order of the assertions: the return code; every output arena intact outside the rows the call may write, every input arena untouched;
then each output.  A failure names the first bad element, the tile and k-slices that compute it, and how many elements are bad.
The fused f16x2 instances (PROD 2) need EGV_X2_SEG=0, which the library reads once per process: they run in ONE fresh child process.

Each test prints `ratio <case> <output> <largest err / bound>` for its bounded outputs (profiles/gemm_elements_ratios.txt keeps them)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import gemm_ref as G
from layernorm_ref import Guarded
from multi_tensor_ref import split_bf16_ref

pytestmark = pytest.mark.gpu

from egovlp_amd import _lib  # noqa: E402

EGV_ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN_CHILD = os.environ.get("EGV_GEMM_ELEMENTS_CHILD") == "1" and os.environ.get("EGV_X2_SEG") == "0"
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


class Buffers:
    """Every operand and output of a case in Guarded arenas, one per (inputs | outputs, dtype)."""

    def __init__(self, c, x):
        d = c.d
        self.groups, self.where = {}, {}
        ks = c.ks
        pd, od, ad = G.plane_dtype(c), G.out_plane_dtype(c), G.aux_dtype(c)
        sa, sb = ((d.K, d.M), (d.K, d.N)) if d.trans else ((d.M, d.K), (d.N, d.K))
        for n in G.OPERANDS:
            rows, cols = sa if n[0] == "a" else sb
            self._add("in", pd, n, rows, cols, d.ld("lda" if n[0] == "a" else "ldb"), x[n])
        if d.bias:
            self._add("in", torch.float32, "bias", 1, d.N, d.N, x["bias"])
        if d.residual:
            self._add("in", torch.float32, "residual", d.M, d.N, c.ldr, x["residual"])
        if d.aux_in:
            self._add("in", ad, "aux_in", d.M, d.N, c.ldaux, x["aux_in"])
        if d.out_f32:
            self._add("out", torch.float32, "out_f32", d.M, d.N, d.ldo, x.get("prev"))
        if d.aux_out:
            self._add("out", ad, "aux_out", d.M, d.N, c.ldaux)
        for n in ("out_hi", "out_lo"):
            if getattr(d, n):
                self._add("out", od, n, d.M, d.N, d.ld("ldoh"))
        if c.out_bf:
            self._add("out", torch.bfloat16, "out_bf", d.M, d.N, d.ld("ldoh"))
        if d.partial:
            self._add("out", torch.float32, "partial", 1, ks * d.M * d.N + (ks * d.M if d.colsum else 0), None)
        if d.colsum:
            self._add("out", torch.float32, "colsum", 1, d.M, d.M)
        for g in self.groups.values():
            g.build("cuda")

    def _add(self, kind, dtype, name, rows, cols, ld, data=None):
        g = self.groups.setdefault((kind, dtype), Guarded(dtype))
        g.add(name, rows, cols, ld, data)
        self.where[name] = g

    def ptr(self, name):
        return self.where[name].ptr(name) if name in self.where else None

    def get(self, name):
        return self.where[name].get(name)

    def assert_guards(self, what):
        for (kind, _), g in self.groups.items():
            if kind == "out":
                g.assert_intact(what)
        for (kind, _), g in self.groups.items():
            if kind == "in":
                g.assert_untouched(what)

    def outputs_all_sentinel(self, names):
        for n in names:
            if n in self.where:
                g = self.where[n]
                got = g.get(n).view(_INT[g.dtype])
                if not bool((got == g.arena.sentinel).all()):
                    return False
        return True


def desc_of(c, b):
    d = c.d
    return _lib.GemmDesc(a_hi=b.ptr("a_hi"), a_lo=b.ptr("a_lo"), lda=d.ld("lda"), b_hi=b.ptr("b_hi"), b_lo=b.ptr("b_lo"), ldb=d.ld("ldb"),
                         M=d.M, N=d.N, K=d.K, passes=d.passes, alpha=d.alpha, act=d.act, bias=b.ptr("bias"), residual=b.ptr("residual"),
                         ldr=c.ldr, aux_in=b.ptr("aux_in"), aux_out=b.ptr("aux_out"), ldaux=c.ldaux, out_f32=b.ptr("out_f32"), ldo=d.ldo,
                         out_hi=b.ptr("out_hi"), out_lo=b.ptr("out_lo"), ldoh=d.ld("ldoh"), ksplit=d.ksplit, accumulate=d.accumulate,
                         partial=b.ptr("partial"), trans=d.trans, aux_bf16=d.aux_bf16, colsum=b.ptr("colsum"), grid_cap=d.grid_cap,
                         out_fmt=d.out_fmt, out_bf=b.ptr("out_bf"))


def _first_bad(c, name, bad):
    idx = torch.nonzero(bad)
    first = idx[0].tolist()
    m, n = (first[0], 0) if len(first) == 1 else (first[0], first[1])
    return "%s: %s: %d of %d elements bad, the first at (m %d, n %d): %s" % (c.id, name, int(bad.sum()), bad.numel(), m, n, G.locate(c, m, n))


def assert_bits(c, name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (c.id, name, got.dtype, want.dtype, got.shape, want.shape)
    bad = got.view(_INT[got.dtype]) != want.view(_INT[want.dtype])
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(_first_bad(c, name, bad) + "; got %r, expected %r" % (float(got[i]), float(want[i])))


def assert_bound(c, name, got64, ref, bound):
    err = (got64 - ref).abs()
    bad = ~(err <= bound)                       # a NaN is out of every bound
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    print("ratio %s %s %.4f" % (c.id, name, float(ratio.max())))
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(_first_bad(c, name, bad) + "; got %r, reference %r, |err| %.3e, bound %.3e" % (
            float(got64[i]), float(ref[i]), float(err[i]), float(bound[i])))


def _sync(c):
    """A device fault ends the whole run: nothing more is started on a card that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault behind case %s: %s" % (c.id, e), returncode=3)


def run_case(c):
    x = G.make_inputs(c)
    b = Buffers(c, x)
    h = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    desc = desc_of(c, b)
    rc = h.egv_gemm_nt(C.byref(desc), stream)
    _sync(c)
    if c.want is None:
        assert rc == EGV_ERR_ARG, (c.id, rc)
        for g in b.groups.values():
            g.assert_untouched(c.id)            # a refused call enqueues nothing: outputs, slabs and inputs alike
        return
    assert rc == 0, (c.id, rc)
    b.assert_guards(c.id)
    d = c.d
    if d.accumulate == 2:
        # the slabs stay for the caller; nothing else is written.  egv_splitk_reduce_multi finishes them.
        assert b.outputs_all_sentinel(("out_f32", "colsum")), c.id + ": accumulate == 2 wrote an output"
        arr = lambda t, *v: (t * len(v))(*v)                                           # noqa: E731
        rc = h.egv_splitk_reduce_multi(1, arr(C.c_void_p, b.ptr("partial")), arr(C.c_void_p, b.ptr("out_f32")), arr(C.c_int64, d.M * d.N),
                                       arr(C.c_int32, d.ksplit), arr(C.c_void_p, b.ptr("colsum")), arr(C.c_int32, d.M), stream)
        _sync(c)
        assert rc == 0, (c.id, rc)
        b.assert_guards(c.id + " (reduce)")
    for chk in G.reference(c, x):
        if chk.bits is not None:
            got = b.get(chk.name)
            assert_bits(c, chk.name, got.reshape(chk.bits.shape), chk.bits)
        elif chk.planes == ("split-of-out_f32",):
            hi, lo = split_bf16_ref(b.get("out_f32"))
            assert_bits(c, "out_hi", b.get("out_hi"), hi)
            if d.out_lo:
                assert_bits(c, "out_lo", b.get("out_lo"), lo)
        else:
            got = sum(b.get(n).double() for n in (chk.planes or (chk.name,)))
            assert_bound(c, chk.name, got.reshape(chk.ref.shape), chk.ref, chk.bound)


if not IN_CHILD:
    @pytest.mark.parametrize("c", G.CASES, ids=[c.id for c in G.CASES])
    def test_gemm_case(c):
        run_case(c)

    def test_fused_f16x2_instances_in_a_child_process():
        """The PROD 2 list (EGV_X2_SEG=0): one child, one pytest run over that list alone; only its exit status is looked at."""
        env = dict(os.environ, EGV_X2_SEG="0", EGV_GEMM_ELEMENTS_CHILD="1")
        cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider",
               os.path.join("tests", "test_gpu_gemm_elements.py") + "::test_fused_f16x2_case"]
        try:
            p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
        except subprocess.TimeoutExpired:
            pytest.exit("the EGV_X2_SEG=0 child hung: nothing more is started on that card", returncode=3)
        print(p.stdout[-6000:])
        if p.returncode == 3 or p.returncode < 0 or p.returncode in (134, 139):
            # its own pytest.exit behind a device fault, or killed by a signal: the card may have faulted -- the run ends here
            pytest.exit("the EGV_X2_SEG=0 child ended with status %d: %s" % (p.returncode, p.stdout[-1500:]), returncode=3)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
else:
    @pytest.mark.parametrize("c", G.X2_CASES, ids=[c.id for c in G.X2_CASES])
    def test_fused_f16x2_case(c):
        run_case(c)
