"""The case table of tests/gemm_ref.py on the CPU: every case's inputs really sum exactly, its expected pick is what csrc/gemm_dispatch.h
answers (the compiled header, through the driver of tests/test_gemm_dispatch_cpu.py) and what the mirror answers, the table covers
what it promises, the erf polynomial has the error the bounds assume, and the tile-walk model -- which reproduces the references bit
for bit -- is rejected by the bit comparison, on the table's own inputs, for each kernel-shaped mutant."""
import subprocess
from dataclasses import replace

import numpy as np
import pytest
import torch

import gemm_dispatch_ref as R
import gemm_ref as G
from multi_tensor_ref import U
from test_gemm_dispatch_cpu import driver  # noqa: F401  (the fixture: the header compiled on its own, sanitizers on)

ALL = G.CASES + G.X2_CASES
GRID = [c for c in ALL if c.klass == "grid" and c.want is not None]
_inputs = {}


def inputs(c):
    """make_inputs once per case and module run (the exactness, model and mutant tests share them, unchanged)."""
    if c.id not in _inputs:
        _inputs.clear()                 # one case at a time: the tall cases are tens of MB
        _inputs[c.id] = G.make_inputs(c)
    return _inputs[c.id]


def with_out_f32(c):
    """The same case with an fp32 output, whatever it stores: the linear value as the reference has it."""
    return replace(c, d=replace(c.d, ptrs=c.d.ptrs | {"out_f32"}))


def linear_bits(c, x):
    """The reference's out_f32 where it is a bit-for-bit one (None otherwise: GELU, GELU', a non-power-of-two alpha behind slabs)."""
    for chk in G.reference(with_out_f32(c), x):
        if chk.name == "out_f32" and chk.bits is not None:
            return chk.bits
    return None


# ------------------------------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("c", GRID, ids=[c.id for c in GRID])
def test_every_partial_sum_is_exact(c):
    """max |partial sum| / granularity < 2^24 from the case's K, value ranges, bias, residual and previous contents; every input is a
    multiple of the grain and inside the range the magnitude assumes; and, for sampled elements, an fp32 accumulation of the element's
    terms in several shuffled orders equals their fp64 sum."""
    d = c.d
    for what, mag, grain in c.exactness():
        assert mag / grain < 2 ** 24, (what, mag, grain)
    x = inputs(c)
    prod_grain = c.exactness()[0][2]
    for n in G.OPERANDS:
        lim = c.amax * 2.0 ** -(c.a_exp if n[0] == "a" else 0) * (2.0 ** -c.lo_exp if n.endswith("lo") else 1.0)
        assert float(x[n].abs().max()) <= lim
        assert x[n].to(G.plane_dtype(c)).double().equal(x[n]), n            # exact in the format it travels in
    for n in ("bias", "residual", "prev"):
        if n in x:
            assert float(x[n].abs().max()) <= c.amax * 2.0 ** -c.e_exp and bool((x[n] / prod_grain == (x[n] / prod_grain).round()).all())
    rng = np.random.RandomState(len(c.id))
    ms, ns = rng.randint(0, d.M, 6), rng.randint(0, d.N, 6)
    ms[0], ns[0] = d.M - 1, d.N - 1
    for m, n in zip(ms, ns):
        a = {k: (x[k][:, m] if d.trans else x[k][m]).numpy() for k in ("a_hi", "a_lo")}
        b = {k: (x[k][:, n] if d.trans else x[k][n]).numpy() for k in ("b_hi", "b_lo")}
        pairs = {1: [("a_hi", "b_hi")], 4: [("a_hi", "b_hi")], 2: [("a_hi", "b_hi"), ("a_lo", "b_lo")],
                 3: [("a_hi", "b_lo"), ("a_lo", "b_hi"), ("a_hi", "b_hi")]}[d.passes]
        alpha = d.alpha if c.alpha_pow2 else 1.0
        terms = np.concatenate([a[p] * b[q] * alpha for p, q in pairs] +
                               [np.array([float(x[k][n] if k == "bias" else x[k][m, n])]) for k in ("bias", "residual", "prev") if k in x])
        assert np.all(terms / prod_grain == np.round(terms / prod_grain))
        want = terms.sum()                                                   # fp64: exact, far below 2^53 grains
        for _ in range(4):
            rng.shuffle(terms)
            got = np.add.accumulate(terms.astype(np.float32), dtype=np.float32)
            assert float(got[-1]) == want and np.all(got.astype(np.float64) == np.add.accumulate(terms))
        if d.colsum:
            col = (x["a_hi"][:, m] + (x["a_lo"][:, m] if d.passes == 3 else 0.0)).numpy()
            assert float(np.add.accumulate(col.astype(np.float32), dtype=np.float32)[-1]) == col.sum()


# ------------------------------------------------------------------------------------------------------------------------- picks
def test_expected_picks_are_the_headers(driver):  # noqa: F811
    """Every case's expected pick -- written into the table, not derived from the mirror -- equals what the mirror and the compiled
    header answer; a refused case is refused by both; the PROD 2 list under EGV_X2_SEG = 0, the rest under the default."""
    run = subprocess.run([driver], input="".join(c.d.words() + "\n" for c in ALL), capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(ALL)
    for c, line in zip(ALL, got):
        assert c.d.x2_seg == (0 if c in G.X2_CASES else 2) and c.d.f3 == 1
        assert line == R.line(R.expected(c.d)), (c.id, line)
        assert G.pick_of(c) == c.want, (c.id, G.pick_of(c), c.want)
        if c.want is None:
            assert line == "1", c.id
        else:
            w = line.split()
            assert (int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]), int(w[6]), int(w[13])) == c.want, (c.id, line)
            assert w[-1] == "1"                                              # the instance exists
            if c.want[0] == G.SMALL:
                assert int(w[8]) == (3 if c.d.passes == 3 else 1)


# ------------------------------------------------------------------------------------------------------------------------- coverage
def _ids(cases):
    return {G.big_id(c.want) for c in cases if c.want is not None and c.want[0] == G.BIG}


def test_table_covers_every_instance_and_edge():
    every = {(mf, tn, epi, prod, mixed) for mf in (4, 5) for tn in (0, 1) for epi in range(6) for prod in range(4) for mixed in (0, 1)
             if G.big_instance(mf, tn, epi, prod, mixed)}
    assert len(every) == 43
    ids = {G.big_id((G.BIG,) + k + (0,)): k for k in every}
    prod2 = {i for i, k in ids.items() if k[3] == 2}
    # every instance id: the PROD 2 ones in the EGV_X2_SEG = 0 list and nowhere else, every other one under the default knobs
    assert _ids(G.CASES) == set(ids) - prod2 and _ids(G.X2_CASES) == prod2 and len(prod2) == 11
    ok = [c for c in G.CASES if c.want is not None]
    assert {c.d.passes for c in ok if c.want[0] == G.SMALL} == {1, 3}
    assert {c.want[6] for c in ok} == {G.RED_NONE, G.RED_EPILOGUE, G.RED_SLAB, G.RED_CALLER}
    assert not any(c.d.passes == 3 and c.want[0] == G.BIG and c.want[4] == 0 and not c.d.trans for c in ok)      # diagnostics build only
    assert sum(c.want is None for c in G.CASES) >= 5 and sum(c.klass == "randn" for c in G.CASES) == 3

    # ---- gemm_big NT
    nt = [c for c in ok if c.want[0] == G.BIG and not c.d.trans and c.klass == "grid"]
    assert {4, 8, 252} <= {c.d.N % 256 for c in nt}
    def beyond(c):
        """Rows by which the (shifted) last band lies past the end of the band before it, from the pick's own bands."""
        b = G.bands(c)
        return c.d.M - (b[-2][0] + b[-2][1])

    for mf, mixed in ((4, 0), (5, 0), (5, 1)):
        some = [c for c in nt if c.want[1] == mf and c.want[5] == mixed]
        last = {beyond(c) for c in some}
        assert {1, 8, G.bands(some[0])[-1][1] - 1} <= last, (mf, mixed, sorted(last))
    # mixed bands with 320-row bands in front (nb5 > 0) end 193 .. 256 rows past the band before: both ends of what exists
    assert {193, 255} <= {beyond(c) for c in nt if c.want[5] == 1 and R.expected(c.d)[6] > 0}
    for mf, mixed in ((4, 0), (5, 0), (5, 1)):
        some = [c for c in nt if c.want[1] == mf and c.want[5] == mixed]
        assert {64, 128} <= {c.d.K for c in some}
    assert 768 in {c.d.K for c in nt if c.ks == 1} and 768 in {c.d.K for c in nt if c.ks > 1}
    assert any(c.d.ldo_pad == 4 and c.d.out_f32 for c in nt) and any(c.d.out_hi and c.d.ldoh == c.d.N + 8 for c in nt)
    assert any(c.d.out_hi and c.d.ldoh > c.d.N for c in nt) and any(c.ldaux_pad and (c.d.aux_in or c.d.aux_out) for c in nt)
    assert any(c.ldr_pad and c.d.residual for c in nt) and any(c.d.lda == c.d.K + 8 and c.d.ldb == c.d.K + 8 for c in nt)
    walked = [c for c in nt if c.d.grid_cap == 8 and len(G.bands(c)) * len(G.columns(c)) >= 200]
    assert len(walked) >= 3 and all(R.expected(c.d)[8] == 8 for c in walked)             # 8 workgroups, >= 25 tiles each
    slab = [c for c in nt if c.want[6] == G.RED_SLAB]
    assert {0, 1} <= {c.d.accumulate for c in slab}
    uneven = [c for c in slab if len({k1 - k0 for k0, k1 in G.k_slices(c)}) > 1]
    assert uneven and {c.want[4] for c in uneven} == {0, 3}

    # ---- TN
    tn = [c for c in ok if c.d.trans and c.klass == "grid"]
    for passes in (1, 3, 4):
        assert any(c.d.passes == passes and c.ks > 1 for c in tn) and any(c.d.passes == passes and c.ks == 1 for c in tn)
    assert {256, 264, 504, 520} <= {c.d.M for c in tn} and {256, 264, 504, 520} <= {c.d.N for c in tn}
    assert {1, 63, 64, 65, 130} <= {c.d.K for c in tn}
    assert {1, 2, 3} <= {c.ks for c in tn} and any(c.ks > (c.d.K + 63) // 64 for c in tn)       # more slices than k-tiles
    for cs in (False, True):
        assert {0, 1, 2} <= {c.d.accumulate for c in tn if bool(c.d.colsum) == cs and c.ks > 1}
    assert {1.0, 0.5, G.ALPHA_X2} <= {c.d.alpha for c in tn} and any(c.d.lda > c.d.M for c in tn)
    assert any(c.d.alpha == G.ALPHA_X2 and c.ks == 1 for c in tn) and any(c.d.alpha == G.ALPHA_X2 and c.ks > 1 for c in tn)

    # ---- the small kernel, un-split and through the reduce-with-epilogue
    sm = [c for c in ok if c.want[0] == G.SMALL and c.klass == "grid"]
    assert {1, 127, 128, 129, 200} <= {c.d.M for c in sm} and {4, 72, 124, 128, 132} <= {c.d.N for c in sm} and {32, 96} <= {c.d.K for c in sm}
    assert {1, 2, 5} <= {c.ks for c in sm}
    assert any(c.ks == 2 and c.d.K == 96 for c in sm) and any(c.ks == 5 and c.d.K == 96 for c in sm)        # uneven; more slices than k-steps
    for red in (G.RED_NONE, G.RED_EPILOGUE):
        some = [c for c in sm if c.want[6] == red]
        assert any(c.d.alpha != 1.0 for c in some) and any(c.d.bias for c in some) and any(c.d.residual for c in some)
        assert any(c.d.act == G.ACT_GELU and c.d.aux_out for c in some) and any(c.d.act == G.ACT_GELU_BWD for c in some)
        assert any(c.d.act == G.ACT_RELU_BWD for c in some)
        assert any(c.d.out_f32 and c.d.out_hi for c in some) and any(c.d.out_hi and not c.d.out_f32 and c.d.ldoh > c.d.N for c in some)


# ------------------------------------------------------------------------------------------------------------------------- erf
def test_erf_polynomial_error():
    """E: A&S 7.1.26 is within ERF_E of erf in exact arithmetic, and the fp32 evaluation of gelu_parts within K_CDF u + E / 2 of Phi and
    its gelu / gelu' within the bounds the GPU test uses, over a dense grid of z and over the grid values a GELU case can produce."""
    u64 = np.linspace(0.0, 6.0, 600001)
    erf = torch.erf(torch.from_numpy(u64)).numpy()
    assert np.abs(G.erf_poly64(u64) - erf).max() <= G.ERF_E
    z = np.concatenate([np.linspace(-9.0, 9.0, 1800001), np.arange(-2 ** 15, 2 ** 15 + 1) * 2.0 ** -11]).astype(np.float32)
    zt = torch.from_numpy(z.astype(np.float64))
    cdf, pdf = G.emu_gelu_parts(z)
    assert float((torch.from_numpy(cdf.astype(np.float64)) - G.phi64(zt)).abs().max()) <= G.K_CDF * U + G.ERF_E / 2
    gelu = torch.from_numpy((z * cdf).astype(np.float64))
    grad = torch.from_numpy((cdf + z * pdf).astype(np.float64))
    assert bool(((gelu - G.gelu64(zt)).abs() <= G.gelu_bound(zt)).all())
    assert bool(((grad - G.gelu_grad64(zt)).abs() <= G.gelu_grad_bound(zt)).all())


# ------------------------------------------------------------------------------------------------------------------------- model, mutants
LINEAR_CASES = [c for c in GRID if c.d.act in (G.ACT_NONE, G.ACT_RELU_BWD)]


@pytest.mark.parametrize("c", LINEAR_CASES, ids=[c.id for c in LINEAR_CASES])
def test_tile_walk_model_and_its_mutants(c):
    """The numpy model of the launch -- k-slices, bands, shifted origins, slabs, reduce, the linear epilogue, all sums in fp32 -- gives
    the reference's bits; each mutant that applies to the case changes bits of the case's own outputs."""
    x = inputs(c)
    want = linear_bits(c, x)
    cs = next((chk.bits for chk in G.reference(with_out_f32(c), x) if chk.name == "colsum"), None)
    good = G.walk(c, x)
    if want is not None:
        assert torch.equal(good["out_f32"], want)
    if cs is not None:
        assert torch.equal(good["colsum"], cs)
    for m in G.MUTANTS:
        if not G.applies(c, m):
            continue
        bad = G.walk(c, x, m)
        if m == "colsum_twice":
            assert not torch.equal(bad["colsum"], cs), m
        elif want is not None:
            assert not torch.equal(bad["out_f32"], want), m


def test_every_mutant_meets_cases():
    """... and none of them is vacuous: each applies to several cases whose comparison is bit for bit."""
    for m in G.MUTANTS:
        n = sum(G.applies(c, m) and (m == "colsum_twice" or c.alpha_pow2 or c.ks == 1) for c in LINEAR_CASES)
        assert n >= 3, (m, n)


def test_locate_names_tile_and_slices():
    c = G.BY_ID["nt-splitk5-p3-K768"]
    s = G.locate(c, c.d.M - 1, c.d.N - 1)
    assert "origin [%d]" % (c.d.M - 256) in s and "origin [4]" in s and "(640, 768)" in s
    assert G.k_slices(c) == [(0, 160), (160, 320), (320, 480), (480, 640), (640, 768)]
    assert G.k_slices(G.BY_ID["small-alpha-bias-200x132x96-p3-ks5"])[2:] == [(64, 96), (96, 96), (96, 96)]
