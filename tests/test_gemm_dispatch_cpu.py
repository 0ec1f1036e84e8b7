"""csrc/gemm_dispatch.h on the CPU: the header is compiled on its own (g++, address + undefined-behaviour sanitizers) into a driver that
prints the result of the check and every field of the pick, one descriptor per input line; tests/gemm_dispatch_ref.py, a restatement
of the launchers the header replaced, says what the lines have to be.  ops.uses_big_gemm / ops.f16x2_gemm_ok, which the trainers route
on, are pinned to the header here as well."""
import itertools
import os
import random
import shutil
import subprocess
from dataclasses import replace

import pytest

import gemm_dispatch_ref as R
from gemm_dispatch_ref import Desc

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "gemm_dispatch.h"

// one descriptor per input line, the words of tests/gemm_dispatch_ref.py Desc.words(); pointers are present (any address) or null
int main() {
  static uint16_t there[8];
  std::string w[19];
  for (;;) {
    for (auto& x : w) if (!(std::cin >> x)) return 0;
    auto I = [&](int i) { return atoll(w[i].c_str()); };
    auto P = [&](int bit) -> void* { return (I(16) >> bit) & 1 ? (void*)there : nullptr; };
    egv_gemm_desc d = {};
    d.M = I(0); d.N = I(1); d.K = I(2); d.passes = I(3); d.trans = I(4); d.ksplit = I(5); d.accumulate = I(6); d.act = I(7);
    d.out_fmt = I(8); d.aux_bf16 = I(9); d.alpha = (float)strtod(w[10].c_str(), nullptr); d.grid_cap = I(11);
    d.lda = I(12); d.ldb = I(13); d.ldo = I(14); d.ldoh = I(15);
    d.a_hi = (egv_bf16*)P(0); d.a_lo = (egv_bf16*)P(1); d.b_hi = (egv_bf16*)P(2); d.b_lo = (egv_bf16*)P(3);
    d.bias = (float*)P(4); d.residual = (float*)P(5); d.aux_in = (float*)P(6); d.aux_out = (float*)P(7); d.out_f32 = (float*)P(8);
    d.out_hi = (egv_bf16*)P(9); d.out_lo = (egv_bf16*)P(10); d.partial = (float*)P(11); d.colsum = (float*)P(12);
    const int x2_seg = I(17), f3 = I(18);
    if (gemm_check(d, x2_seg)) { printf("1\n"); continue; }
    const GemmPick g = gemm_pick(d, x2_seg, f3);
    printf("0 %d %d %d %d %d %d %d %d %lld %lld %d %d %d %lld %lld %d\n", g.family, g.mf, g.tn, g.epi, g.prod, g.mixed, g.nb5, g.passes,
           (long long)g.grid_x, (long long)g.grid_y, g.block, g.lds, g.reduce, (long long)g.reduce_grid, (long long)g.reduce_blocks1,
           g.family == GEMM_BIG ? (int)gemm_big_instance(g.mf, g.tn, g.epi, g.prod, g.mixed) : 1);
  }
}
"""

MS = (1, 127, 128, 129, 248, 255, 256, 264, 319, 320, 328, 639, 640, 5376, 5384, 7176, 25120)
NS = (4, 6, 252, 256, 260, 768, 2304, 3072)
KS = (32, 48, 64, 96, 768)
PASSES, TRANS, KSPLIT, ACC, ACT = range(6), (0, 1), (0, 1, 2, 128, 65535, 65536), (0, 1, 2), range(4)
OUT_FMT, AUX16 = range(-1, 6), range(-1, 5)
ALPHA = (1.0, 0.5, 0.0, -1.0, float("nan"))
CAP = (0, 7, 8, 12, 248, 256, 264)
X2, F3 = (0, 1, 2), (0, 1)
BIG_INSTANCES = 43                      # the kernels of profiles/gemm_dispatch_regs.txt

OPERANDS = frozenset(("a_hi", "a_lo", "b_hi", "b_lo"))
F32 = OPERANDS | {"out_f32", "partial"}                                   # plain fp32 output
PLANES = OPERANDS | {"bias", "out_hi", "out_lo", "partial"}               # qkv: bias -> planes
FC1 = PLANES | {"aux_out"}
DZ = OPERANDS | {"aux_in", "out_hi", "out_lo", "partial"}
RESID = F32 | {"bias", "residual"}
EVERY = frozenset(R.POINTERS)
SHAPES = ((128, 128, 64), (256, 256, 64), (640, 2304, 768), (5376, 3072, 64), (5384, 3072, 64), (7176, 2304, 64), (25120, 768, 768))


def sweep_shapes():
    """Every M x N x K x passes, NT and TN, into fp32 and (NT) through the bias into planes, (TN) with the column sums."""
    out = []
    for M, N, K, passes, trans in itertools.product(MS, NS, KS, PASSES, TRANS):
        d = Desc(M=M, N=N, K=K, passes=passes, trans=trans)
        out += [d, replace(d, ptrs=F32 | {"colsum"}) if trans else replace(d, ptrs=PLANES)]
    return out


def sweep_splitk():
    out = []
    for (M, N, K), passes, trans, ks, acc, pad in itertools.product(SHAPES + ((1, 4, 32), (256, 256, 8192)), (1, 2, 3, 4), TRANS, KSPLIT, ACC, (0, 8)):
        for drop in ((), ("out_f32",), ("partial",), ("out_f32", "out_hi+")):
            ptrs = (F32 | {"colsum"} if trans else F32) - set(drop) | ({"out_hi"} if "out_hi+" in drop else set())
            out.append(Desc(M=M, N=N, K=K, passes=passes, trans=trans, ksplit=ks, accumulate=acc, ldo_pad=pad, ptrs=frozenset(ptrs)))
    return out


def sweep_epilogues():
    """Every act x out_fmt x aux_bf16 under every product kind, with the pointer sets of the step's launches and with everything there."""
    out = []
    for (M, N, K), passes, act, fmt, aux, x2, alpha in itertools.product(SHAPES, (1, 2, 3, 4), ACT, OUT_FMT, AUX16, X2, (1.0, 0.5)):
        if x2 != 2 and passes != 2:
            continue
        for ptrs in (F32, PLANES, FC1, DZ, RESID, EVERY - {"colsum"}):
            out.append(Desc(M=M, N=N, K=K, passes=passes, act=act, out_fmt=fmt, aux_bf16=aux, x2_seg=x2, alpha=alpha, ptrs=ptrs))
    for fmt, ldoh, act, passes in itertools.product((1, 2, 3, 4), (256, 260), ACT, (2, 4)):
        out.append(Desc(passes=passes, act=act, out_fmt=fmt, ldoh=ldoh, aux_bf16=2, ptrs=DZ))
    return out


def sweep_pointers():
    """Each pointer taken away from, and added to, a valid launch of every kind."""
    bases = [Desc(ptrs=F32), Desc(passes=3, ptrs=PLANES), Desc(passes=2, act=1, out_fmt=1, aux_bf16=2, ptrs=FC1),
             Desc(passes=4, act=2, out_fmt=4, aux_bf16=3, ptrs=DZ), Desc(passes=4, out_fmt=3, ptrs=PLANES), Desc(passes=4, out_fmt=4, ptrs=DZ),
             Desc(M=128, N=128, passes=3, ksplit=2, ptrs=RESID), Desc(trans=1, K=100, ksplit=2, ptrs=F32 | {"colsum"}),
             Desc(trans=1, passes=4, ksplit=2, accumulate=2, ptrs=F32), Desc(M=7176, N=2304, passes=3, grid_cap=8, ptrs=PLANES),
             Desc(M=7176, N=2304, passes=2, x2_seg=0, act=1, grid_cap=8, ptrs=FC1), Desc(M=5384, N=3072, passes=3, act=3, ptrs=DZ)]
    out = []
    for d in bases:
        out.append(d)
        for p in R.POINTERS:
            out.append(replace(d, ptrs=d.ptrs ^ {p}))
            out.append(replace(d, ptrs=(d.ptrs | {"bias", "residual", "out_f32"}) ^ {p}))
    return out


def sweep_alpha_and_strides():
    out = []
    for alpha, act, passes, trans, (M, N, K), ptrs in itertools.product(ALPHA, ACT, (1, 2, 3, 4), TRANS, SHAPES[:3], (F32, RESID)):
        out.append(Desc(M=M, N=N, K=K, passes=passes, trans=trans, act=act, alpha=alpha, ptrs=ptrs))
    for lda, ldb, passes, trans, (M, N, K) in itertools.product((0, 772, 776), (0, 772, 776), (1, 4), TRANS, SHAPES[:2]):
        out.append(Desc(M=M, N=N, K=K, passes=passes, trans=trans, lda=lda, ldb=ldb))
    return out


def sweep_grid_cap_and_knobs():
    """grid_cap on both sides of its range and of the mixed-band threshold (8 workgroups), the two process knobs, all tall shapes."""
    out = []
    for cap, M, N, passes, x2, f3, (act, fmt, aux, ptrs) in itertools.product(CAP, MS[8:], (768, 2304, 3072), (1, 2, 3, 4), X2, F3,
                                                                        ((0, 0, 0, PLANES), (1, 0, 0, FC1), (1, 1, 2, FC1), (0, 0, 0, F32), (0, 0, 0, OPERANDS))):
        if (x2 != 2 and passes != 2) or (f3 != 1 and passes != 3):
            continue
        out.append(Desc(M=M, N=N, K=64, passes=passes, act=act, out_fmt=fmt, aux_bf16=aux, grid_cap=cap, x2_seg=x2, f3=f3, ptrs=ptrs))
    for K, N, x2, act in itertools.product((64, 768, 832), (256, 768, 772), X2 + (3,), (0, 1)):
        out.append(Desc(M=640, N=N, K=K, passes=2, x2_seg=x2, act=act, ptrs=PLANES))
    return out


def sweep_grids():
    """Block counts, work ids and k-slices on both sides of what a launch can carry."""
    out = []
    for M, N, K, ks in ((2 ** 27, 2 ** 18, 32, 1), (2 ** 27, 2 ** 18 - 128, 32, 1), (2 ** 27, 2 ** 18 - 128, 32, 2), (2 ** 31 - 1, 2 ** 31 - 4, 32, 1),
                        (2 ** 31 - 1, 4, 32, 65535), (2 ** 31 - 1, 4, 32, 65536), (2 ** 20, 2 ** 20, 64, 127), (2 ** 20, 2 ** 20, 64, 128),
                        (2 ** 20, 2 ** 20, 64, 2 ** 31 - 1), (2 ** 31 - 8, 2 ** 31 - 8, 64, 1), (2 ** 31 - 8, 2 ** 31 - 8, 64, 2 ** 31 - 1),
                        (2 ** 23, 2 ** 18, 64, 1), (2 ** 23, 2 ** 18, 64, 2), (2 ** 16, 2 ** 15, 64, 2 ** 17), (128, 128, 2 ** 31 - 32, 65535)):
        for passes, trans in ((1, 0), (3, 0), (4, 0), (1, 1)):
            out.append(Desc(M=M, N=N, K=K, passes=passes, trans=trans, ksplit=ks, ptrs=F32 | ({"colsum"} if trans else set())))
    return out


def sweep_random():
    """A seeded sample over the whole descriptor: every field from its table, every pointer there or not."""
    rng = random.Random(20260)
    out = []
    for _ in range(40000):
        M, N, K = rng.choice(MS), rng.choice(NS), rng.choice(KS)
        if rng.random() < 0.5:                      # half the sample where most rules have something to decide: at least one big tile
            M, N, K = max(M, 256), max(N, 256), rng.choice((64, 768))
        ptrs = frozenset(p for p in R.POINTERS if rng.random() < (0.95 if p in OPERANDS else 0.5))
        relaxed = rng.random() < 0.6                # ... and the range rules satisfied
        out.append(Desc(M=M, N=N, K=K, passes=rng.choice((1, 2, 3, 4) if relaxed else PASSES), trans=rng.choice(TRANS), ksplit=rng.choice(KSPLIT),
                        accumulate=rng.choice(ACC), act=rng.choice(ACT), out_fmt=rng.choice((0, 0, 1, 2, 3, 4) if relaxed else OUT_FMT),
                        aux_bf16=rng.choice((0, 1, 2, 3) if relaxed else AUX16), alpha=rng.choice((1.0,) if relaxed else ALPHA),
                        grid_cap=rng.choice((0, 8, 248, 256) if relaxed else CAP), lda=rng.choice((0, 0, 0, 3080, 3076)),
                        ldb=rng.choice((0, 0, 0, 3080, 3076)), ldo_pad=rng.choice((0, 0, 8)), ldoh=rng.choice((0, 0, 3080, 3076)), ptrs=ptrs,
                        x2_seg=rng.choice(X2), f3=rng.choice(F3)))
    return out


SWEEPS = {"shapes": sweep_shapes, "split-k": sweep_splitk, "epilogues": sweep_epilogues, "pointers": sweep_pointers,
          "alpha-and-strides": sweep_alpha_and_strides, "grid-cap-and-knobs": sweep_grid_cap_and_knobs, "grids": sweep_grids,
          "random": sweep_random}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gemm_dispatch_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                           os.path.join(root, "egovlp_amd", "csrc"), "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def lines(driver):
    """Every sweep through ONE driver process: {sweep: [(desc, the driver's line)]}."""
    cases = {name: fn() for name, fn in SWEEPS.items()}
    flat = [d for name in SWEEPS for d in cases[name]]
    run = subprocess.run([driver], input="".join(d.words() + "\n" for d in flat), capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    got = run.stdout.splitlines()
    assert len(got) == len(flat)
    it = iter(zip(flat, got))
    return {name: [next(it) for _ in cases[name]] for name in SWEEPS}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_gemm_dispatch_follows_the_launchers_it_replaced(lines, name):
    """The check's result and every field of the pick (family, instance, grids, block, LDS bytes, the reduce and its grid) equal what the
    former launchers did, descriptor by descriptor; every accepted pick names an instance that exists (the line's last word)."""
    for d, got in lines[name]:
        want = R.line(R.expected(d))
        assert got == want, (d, got, want)
        assert got == "1" or got.endswith(" 1")


def test_sweeps_cover_what_they_promise(lines):
    ok = [(d, g.split()) for name in SWEEPS for d, g in lines[name] if g != "1"]
    refused = sum(g == "1" for name in SWEEPS for _, g in lines[name])
    assert len(ok) > 10000 and refused > 20000
    big = {tuple(g[2:7]) for _, g in ok if g[1] == str(R.BIG)}
    assert len(big) == BIG_INSTANCES                                  # every instance of the library is picked somewhere, and nothing else
    assert {g[8] for _, g in ok if g[1] == str(R.SMALL)} == {"1", "3"}
    assert {g[13] for _, g in ok} == {str(x) for x in (R.RED_NONE, R.RED_EPILOGUE, R.RED_SLAB, R.RED_CALLER)}
    assert any(g[13] == str(R.RED_SLAB) and g[14] != g[15] for _, g in ok)          # a column-sum tail
    for name in ("split-k", "random"):                                # the refusals that used to come behind the launch
        assert sum(R.expected(d) is None and R.expected(d, late=False) is not None for d, _ in lines[name]) > 20
    grids = [int(g[9]) for _, g in ok]
    assert max(grids) > 2 ** 30 and 65535 in {int(g[10]) for _, g in ok}
    assert sum(g == "1" for _, g in lines["grids"]) >= 20 and sum(g != "1" for _, g in lines["grids"]) >= 10


def pick(d):
    r = R.expected(d)
    assert r is not None, d
    return dict(zip(("family", "mf", "tn", "epi", "prod", "mixed", "nb5", "passes", "grid_x", "grid_y", "block", "lds", "reduce", "reduce_grid",
                     "reduce_blocks1"), r))


def test_pinned_picks(driver):
    """Numbers worked out from the kernels' own comments, asked of the reference and of the header."""
    qkv = Desc(M=25120, N=2304, K=768, passes=3, ptrs=PLANES)
    fc1 = Desc(M=25120, N=3072, K=768, passes=3, act=1, ptrs=FC1)
    small3 = Desc(M=7176, N=2304, K=64, passes=3, grid_cap=8, ptrs=PLANES)
    tall = Desc(M=5384, N=3072, K=64, passes=3, ptrs=PLANES)
    want = {
        # the two documented splits: 53 bands of 320 rows + 32 of 256
        qkv: dict(mixed=1, nb5=53, mf=5, epi=R.LINEAR, prod=3, grid_x=256, lds=147456, block=512),
        fc1: dict(mixed=1, nb5=53, mf=5, epi=R.GELU, prod=3, grid_x=256),
        # the smallest three-product shape that picks mixed bands: 23 bands of 320 = 207 tiles = 26 rounds of 8 workgroups hold 23 bands
        small3: dict(mixed=1, nb5=21, mf=5, grid_x=8),
        replace(small3, grid_cap=0): dict(mixed=0, nb5=0, mf=5, grid_x=207),
        # 17 bands of 320 = 204 tiles, one round, against 22 of 256 = 264 tiles, two
        tall: dict(mf=5, mixed=0, nb5=0, grid_x=204),
        replace(tall, M=5376): dict(mf=4, mixed=0, grid_x=252, lds=131072),
        # N = 768 at 25 120 tokens: 79 x 3 tiles of 320 rows, one round
        Desc(M=25120, N=768, K=768, passes=3, ptrs=RESID): dict(mf=5, mixed=0, epi=R.LINEAR, grid_x=237),
        # DistilBERT: M = 1024 stays on the 128x128 kernel: 8 x 6 tiles, two k-slices, a reduce over 1024 * 768 / 1024 blocks
        Desc(M=1024, N=768, K=768, passes=3, ksplit=2, ptrs=RESID): dict(family=R.SMALL, passes=3, grid_x=48, grid_y=2, lds=65536, block=256,
                                                                         reduce=R.RED_EPILOGUE, reduce_grid=768),
        # a weight gradient with its bias gradient: 3 x 12 tiles x 7 slices on 256 workgroups; 768 * 3072 / 1024 + 1 reduce blocks
        Desc(M=768, N=3072, K=25120, trans=1, ksplit=7, ptrs=F32 | {"colsum"}): dict(family=R.BIG, tn=1, mf=4, epi=R.RAW, prod=0, grid_x=252,
                                                                                     reduce=R.RED_SLAB, reduce_grid=2305, reduce_blocks1=2304),
    }
    for d, fields in want.items():
        p = pick(d)
        assert {k: p[k] for k in fields} == fields, (d, p)
    run = subprocess.run([driver], input="".join(d.words() + "\n" for d in want), capture_output=True, text=True)
    assert run.stdout.splitlines() == [R.line(R.expected(d)) for d in want]


def test_python_mirror_follows_the_header(lines):
    """ops.uses_big_gemm says which family an un-split NT launch takes and ops.f16x2_gemm_ok whether an fp16 NT launch is accepted."""
    from egovlp_amd import ops
    seen = {True: 0, False: 0}
    for name in SWEEPS:
        for d, g in lines[name]:
            if g != "1" and not d.trans and d.ksplit <= 1:
                big = g.split()[1] == str(R.BIG)
                assert ops.uses_big_gemm(d.M, d.N, d.K, d.passes) == big, d
                seen[big] += 1
    assert min(seen.values()) > 1000
    n = 0
    for d, g in lines["shapes"]:
        if d.passes in (2, 4) and not d.trans:                         # valid in everything but, perhaps, the shape
            assert ops.f16x2_gemm_ok(d.M, d.N, d.K) == (g != "1"), d
            n += g != "1"
    assert n > 100
