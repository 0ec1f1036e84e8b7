"""csrc/block_plan.h on the CPU: the header is compiled on its own (g++, address + undefined-behaviour sanitizers) into a driver that
prints the result of the check, every field of the plan and every offset of the three layouts, one geometry per input line;
tests/block_plan_ref.py, a restatement of the code the header replaced, says what the lines have to be.  model/layer_common.py's
block_plan, which the Python host side reads, is pinned to the header here as well.  Second half: the calls egv_block_fwd / _bwd and
egv_text_layer_fwd / _bwd make (tools/block_call_census.py, a recording stub behind the host-only objects of the two files) against
the digests recorded from the tree before the plan header, tests/golden/block_call_census.sha256."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import pytest

import block_plan_ref as R
from block_plan_ref import Geom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include <iostream>
#include "block_plan.h"

// the library's workspace formulas: fixed stand-ins (tests/block_plan_ref.py has the same)
extern "C" int64_t egv_divided_attn_fwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H, int32_t mode) {
  return (int64_t)B * H * (1 + (int64_t)T * n) * (mode ? 3 : 5) + 7;
}
extern "C" int64_t egv_divided_attn_bwd_work_floats(int32_t B, int32_t T, int32_t n, int32_t H) { return (int64_t)B * H * (1 + (int64_t)T * n) * 2 + 64 * H; }
extern "C" int egv_layernorm_bwd_parts(int32_t rows) { return rows < 64 * 256 ? (rows + 63) / 64 : 256; }
extern "C" int64_t egv_cls_linear_work_floats(int32_t R, int32_t N, int32_t K) { return (int64_t)R * K * 8 + N; }

static void out(const char* tag, const int64_t* v, int n) {
  printf("%s", tag);
  for (int i = 0; i < n; ++i) printf(" %lld", (long long)v[i]);
  printf("\n");
}

// one geometry per input line: B T n H Hd fwd_passes bwd_passes train z_bf16 f16_single ksplit x 6
int main() {
  long long w[16];
  for (;;) {
    for (auto& x : w) if (!(std::cin >> x)) return 0;
    egv_block_geom g = {};
    g.B = w[0]; g.T = w[1]; g.n = w[2]; g.H = w[3]; g.D = 64 * g.H; g.Hd = w[4];
    g.fwd_passes = w[5]; g.bwd_passes = w[6]; g.train = w[7]; g.z_bf16 = w[8]; g.f16_single = w[9]; g.eps = 1e-6f;
    int32_t ks[6];
    for (int i = 0; i < 6; ++i) ks[i] = (int32_t)w[10 + i];
    if (block_check(g) != EGV_OK) { printf("refused\n"); continue; }
    const BlockPlan p = block_plan(g);
    printf("plan %d %d", p.train, p.tail);
    for (int i = 0; i < 6; ++i) printf(" %d", p.passes[i]);
    for (int i = 0; i < 6; ++i) printf(" %d", p.operand[i]);
    for (int i = 0; i < 6; ++i) printf(" %d", p.w_fmt[i]);
    for (int i = 0; i < 6; ++i) printf(" %.9g", (double)p.walpha[i]);
    printf(" %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.w_lo, p.ln_f16, p.lnq_lo, p.ln2_lo, p.qkv_lo, p.attn_lo,
           p.h_lo, p.bf, p.qkv_fmt, p.attn_passes, p.attn_fmt, p.attn_mode_fwd, p.attn_mode_bwd, p.kv_fmt, p.h_fmt, p.z_code, p.z_bytes, p.bwd_passes,
           p.bwd_lo, p.saved_bf, p.grad_fmt, p.ln_fmt, p.attn_bwd_passes, p.attn_bwd_o_lo, p.cls_dx_mode);
    const FwdLayout F = fwd_layout(g, p);
    const int64_t f[] = {F.t.n_hi, F.t.n_lo, F.t.mean, F.t.rstd, F.t.qkv_hi, F.t.qkv_lo, F.t.a_hi, F.t.a_lo, F.t.lse, F.t.work, F.tr,
                         F.s.n_hi, F.s.n_lo, F.s.mean, F.s.rstd, F.s.qkv_hi, F.s.qkv_lo, F.s.a_hi, F.s.a_lo, F.s.lse, F.s.work, F.sr,
                         F.n2_hi, F.n2_lo, F.mean2, F.rstd2, F.h_hi, F.h_lo, F.z, F.t.n_bf, F.s.n_bf, F.n2_bf, F.h_bf,
                         F.n1c, F.mean1c, F.rstd1c, F.qc, F.oc, F.n2c, F.hc, F.total};
    out("fwd", f, sizeof f / sizeof f[0]);
    const BwdLayout L = bwd_layout(g, p, ks);
    const int64_t b[] = {L.g_hi, L.g_lo, L.dz_hi, L.dz_lo, L.d_n2, L.s.d_res, L.s.dres_hi, L.s.dres_lo, L.s.do_hi, L.s.do_lo, L.s.dqkv_hi, L.s.dqkv_lo,
                         L.s.d_n, L.t.d_res, L.t.dres_hi, L.t.dres_lo, L.t.do_hi, L.t.do_lo, L.t.dqkv_hi, L.t.dqkv_lo, L.t.d_n,
                         L.ln_work[0], L.ln_work[1], L.ln_work[2], L.attn_work, L.partial[0], L.partial[1], L.partial[2], L.partial[3], L.partial[4],
                         L.partial[5], L.dzc, L.dn2c, L.dsrc, L.doc, L.dqc, L.lin_work, L.total};
    out("bwd", b, sizeof b / sizeof b[0]);
    int64_t go[19];
    grad_layout(g, go, go[18]);
    out("grad", go, 19);
  }
}
"""

# (B, T, n, H, Hd): the smallest block, the benchmark's, and one whose arena offsets pass 2^31
GEOMETRIES = ((2, 2, 4, 4, 1024), (32, 4, 196, 12, 3072), (64, 16, 196, 12, 3072))
KSPLIT = (1, 2, 4, 1, 3, 2)


def sweep():
    return [Geom(*geo, P, Pb, train, z, single) for geo in GEOMETRIES
            for P, Pb, train, z, single in itertools.product(range(5), range(6), range(-1, 5), (0, 1), range(-1, 17))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("block_plan_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "egovlp_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def answers(driver):
    """[(geometry, None | the driver's four lines)] over the sweep, from ONE driver process."""
    cases = sweep()
    text = "".join(" ".join(map(str, g + KSPLIT)) + "\n" for g in cases)
    run = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    it = iter(run.stdout.splitlines())
    got = []
    for g in cases:
        first = next(it)
        got.append((g, None if first == "refused" else [first, next(it), next(it), next(it)]))
    assert next(it, None) is None
    return got


def test_block_check_accepts_what_geom_ok_accepted(answers):
    for g, got in answers:
        assert (got is not None) == R.geom_ok(g), g
    ok = [g for g, got in answers if got is not None]
    assert len(ok) == 3 * 216 and len(answers) == 3 * 5 * 6 * 6 * 2 * 18
    assert {(g.P, g.Pb) for g in ok} == {(1, 1), (3, 1), (3, 3), (2, 1), (2, 4)}
    assert {g.single for g in ok if g.P == 2} == set(range(16)) and {g.train for g in ok} == {0, 1, 2, 3}


def test_plan_and_layouts_follow_the_code_they_replaced(answers):
    """Every field of the plan, every offset of the forward and backward arenas (with a split-K table that has 1, 2, 3 and 4 in it) and
    the gradient layout equal what the former inline derivations gave, geometry by geometry."""
    big = 0
    for g, got in answers:
        if got is not None:
            want = R.lines(g, KSPLIT)
            for a, b in zip(got, want):
                assert a == b, (g, a, b)
            big += int(got[1].split()[-1]) > 2 ** 31
    assert big >= 216                                   # the third geometry's offsets pass 2^31


def test_python_plan_follows_the_header(answers):
    """layer_common.block_plan(P, Pb, single, train, z_bf16) is the header's plan, field by field, on every accepted case."""
    from egovlp_amd.model.layer_common import BlockPlan, block_plan
    assert len(BlockPlan._fields) == 31
    n = 0
    for g, got in answers:
        if got is not None:
            pl = block_plan(g.P, g.Pb, g.single, g.train, bool(g.z_bf16))
            flat = [x for v in pl for x in (v if isinstance(v, tuple) else (v,))]
            assert "plan " + " ".join(R.fmt(v) for v in flat) == got[0], (g, pl)
            n += 1
    assert n == 3 * 216


def test_pinned_plans():
    """The modes the trainers run, written out by hand from the format descriptions of include/egovlp_hip.h."""
    from egovlp_amd.model.layer_common import A1_INV, block_plan
    x3 = block_plan(3, 1, 0, 1)                          # 'mixed': split-bf16 three-product forward, one bf16 product backward
    assert x3.passes == (3,) * 6 and x3.operand == (0,) * 6 and x3.w_fmt == (0,) * 6 and x3.walpha == (1.0,) * 6
    assert (x3.attn_fmt, x3.attn_mode_fwd, x3.attn_mode_bwd, x3.grad_fmt, x3.ln_fmt, x3.bf, x3.attn_bwd_o_lo) == (0, 0, 0, 0, 0, False, True)
    x2 = block_plan(2, 1, 0, 1, True)                    # 'f16x2' / bf16: two fp16 products in qkv, fc1, fc2; bf16 copies for the backward
    assert x2.passes == (2, 3, 2, 3, 2, 2) and x2.w_fmt == (1, 0, 1, 0, 1, 1) and x2.bf and x2.saved_bf and (x2.h_fmt, x2.z_code) == (1, 2)
    # 'f16mix' / f16, every bit set: ONE fp16 product everywhere; the proj Linears read the attention's one fp16(value) plane
    f = block_plan(2, 4, 15, 1, True)
    assert f.passes == (4,) * 6 and f.operand == (1,) * 6 and f.w_fmt == (1,) * 6 and f.walpha == (1.0,) * 6
    assert (f.attn_fmt, f.attn_mode_fwd, f.attn_mode_bwd) == (3, 6 | 8, 6 | 24) and not f.attn_lo and not f.bf and not f.saved_bf
    assert (f.qkv_fmt, f.h_fmt, f.z_code, f.grad_fmt, f.ln_fmt, f.attn_bwd_passes, f.wt_fmt) == (3, 2, 3, 4, 3, 1, "f16")
    n = block_plan(2, 4, 0, 1, True)                     # the same backward behind two-product Linears: X is a1 of an f16x2 encoding
    assert n.passes == (2,) * 6 and n.walpha == (A1_INV,) * 6 and n.attn_fmt == 2 and n.attn_lo
    p = block_plan(2, 1, 8, 1, True)                     # one-product proj, bf16 backward: fp16(value) as the attention's SECOND plane
    assert p.passes[1] == 4 and p.operand[1] == 2 and p.w_fmt[1] == 1 and p.attn_fmt == 1 and not p.attn_bwd_o_lo


# ---------------------------------------------------------------------------------------------------------------- the call census
def _census():
    spec = importlib.util.spec_from_file_location("block_call_census", os.path.join(ROOT, "tools", "block_call_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_block_and_text_layer_calls_are_the_recorded_ones(tmp_path):
    """Every call of the four entry points, with every argument, over the census sweep: one digest per (entry point, fwd_passes,
    bwd_passes, train) against tests/golden/block_call_census.sha256."""
    census = _census()
    hipcc = census.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    per, cases, lines, _ = census.groups(census.build(ROOT, str(tmp_path), hipcc))
    golden = census.read_golden()
    assert len(golden) > 60 and cases > 30000 and lines > 250000
    bad = census.mismatches(per, golden)
    assert not bad, "calls differ from the recorded ones in %s: compare `python tools/block_call_census.py run` with its output on the " \
                    "parent tree (--root)" % ", ".join(bad)
