"""The references of tests/multi_tensor_ref.py judged on their own, without a GPU: adamw_ref64 against the oracle's AdamW in fp64, the
fp32 oracle inside the element-wise bound the GPU test applies (on the GPU test's own inputs), loss_scale_ref against traces written
out by hand, the arena helper, the table sizes the GPU tests hard-code against the .hip sources, and the host half of csrc/multi_tensor.h
(a stand-alone program under the address and undefined-behaviour sanitizers) against the plan of R.mt_plan."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multi_tensor_ref as R
from oracle import egovlp_oracle as O


def _oracle(ps, gs, ms, vs, dtype, wd, cb, step, gscale):
    lr, (b1, b2), eps = R.f32(R.ADAMW_LR), tuple(R.f32(b) for b in R.ADAMW_BETAS), R.f32(R.ADAMW_EPS)
    out = []
    for p, g, m, v in zip(ps, gs, ms, vs):
        p, m, v = p.clone().to(dtype), m.clone().to(dtype), v.clone().to(dtype)
        ge = g.to(dtype) * torch.tensor(R.f32(gscale), dtype=dtype)         # the un-scaling the kernel does first, in the same format
        O.adamw_step(p, ge, m, v, step, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=R.f32(wd), correct_bias=bool(cb))
        out.append((p, m, v))
    return out


_WORST = {"p": 0.0, "m": 0.0, "v": 0.0}


@pytest.mark.parametrize("case", R.adamw_cases(), ids=[c[0] for c in R.adamw_cases()])
def test_adamw_ref64_agrees_with_the_oracle_and_the_fp32_oracle_is_inside_the_bound(case):
    """On the inputs of tests/test_gpu_multi_tensor.py::test_adamw_multi: (a) the oracle in fp64 and adamw_ref64 (step size and lr * wd left
    un-rounded, as the oracle has them) agree to 1e-12 of the error scale; (b) the oracle in fp32 -- the same operations in the same
    format as the kernel -- stays inside K u s for p, m and v.  Largest err / (u s) of the fp32 oracle over all cases, measured: p 3.55,
    m 1.93, v 1.98 (allowed 13 / 16, 4, 6)."""
    cid, count, wd, cb, step, gscale, seed = case
    numels, _ = R.adamw_case_layout(count, seed)
    ps, gs, ms, vs = R.adamw_inputs(numels, step, gscale, seed)
    lr, (b1, b2) = R.ADAMW_LR, R.ADAMW_BETAS
    o64 = _oracle(ps, gs, ms, vs, torch.float64, wd, cb, step, gscale)
    o32 = _oracle(ps, gs, ms, vs, torch.float32, wd, cb, step, gscale)
    from egovlp_amd.optim import adamw_step_size
    ss = R.f32(adamw_step_size(R.f32(lr), R.f32(b1), R.f32(b2), step, bool(cb)))
    for i, n in enumerate(numels):
        args = (ps[i], gs[i], ms[i], vs[i], lr, b1, b2, R.ADAMW_EPS, wd, step, cb, gscale)
        exact = R.adamw_ref64(*args, round_scalars=False)
        for x, r, s in zip(o64[i], exact[:3], exact[3:]):
            assert bool(((x - r).abs() <= 1e-12 * s).all()), (cid, i, n)
        ref = R.adamw_ref64(*args)
        ratios = R.check_adamw(o32[i], ref, ps[i], wd, ss, "%s tensor %d (numel %d), fp32 oracle" % (cid, i, n))
        for k, r in zip("pmv", ratios):
            _WORST[k] = max(_WORST[k], r)
    print("fp32 oracle, largest err / (u s) so far: p %.2f m %.2f v %.2f" % (_WORST["p"], _WORST["m"], _WORST["v"]))


def test_adamw_bound_sees_one_wrong_element():
    """One element one fp32 ulp-of-its-scale too far, in a 130 000-element tensor, fails the element-wise bound (a relative L2 norm at
    1e-6 would not move)."""
    ps, gs, ms, vs = R.adamw_inputs([130000], 1000, 1.0, 3)
    lr, (b1, b2) = R.ADAMW_LR, R.ADAMW_BETAS
    ref = R.adamw_ref64(ps[0], gs[0], ms[0], vs[0], lr, b1, b2, R.ADAMW_EPS, 0.01, 1000)
    got = [ref[0].float(), ref[1].float(), ref[2].float()]
    R.check_adamw(got, ref, ps[0], 0.01, 1e-2)
    got[0][77777] += 20 * R.U * float(ref[3][77777])
    assert float((got[0].double() - ref[0]).norm() / ref[0].norm()) < 1e-6
    with pytest.raises(AssertionError):
        R.check_adamw(got, ref, ps[0], 0.01, 1e-2)


# ------------------------------------------------------------------------------------------------------------------------- loss scale
def _run_trace(init_scale, overflows, steps=None, growth=2.0, backoff=0.5, interval=3, max_scale=2.0 ** 24, correct_bias=1):
    st = {"scale": np.float32(init_scale), "good": 0, "skipped": 0, "inv": np.float32(1.0 / init_scale), "skip": 0.0}
    rows = []
    for i, ov in enumerate(overflows):
        step = steps[i] if steps is not None else i + 1
        st, hyper = R.loss_scale_ref(st, ov, 1e-2, 0.9, 0.999, step, correct_bias, growth, backoff, interval, max_scale)
        rows.append((float(st["scale"]), st["good"], st["skipped"], hyper[2], hyper[3], max(step - st["skipped"], 1)))
    return rows


def test_loss_scale_ref_overflow_at_the_first_step():
    #        S after, good, skipped, 1/S of this step, skip, t of the bias correction
    assert _run_trace(1024.0, [True, False]) == [
        (512.0, 0, 1, 1.0 / 1024, 1.0, 1),          # skipped; step 1 - 1 skipped = 0 -> clamped to t = 1
        (512.0, 1, 1, 1.0 / 512, 0.0, 1),           # the first APPLIED step is t = 1
    ]


def test_loss_scale_ref_grows_exactly_at_the_interval():
    assert _run_trace(1024.0, [False] * 7, interval=3) == [
        (1024.0, 1, 0, 1.0 / 1024, 0.0, 1),
        (1024.0, 2, 0, 1.0 / 1024, 0.0, 2),
        (2048.0, 0, 0, 1.0 / 1024, 0.0, 3),         # the third good step in a row: S doubles AFTER this step's gradients used 1 / 1024
        (2048.0, 1, 0, 1.0 / 2048, 0.0, 4),
        (2048.0, 2, 0, 1.0 / 2048, 0.0, 5),
        (4096.0, 0, 0, 1.0 / 2048, 0.0, 6),
        (4096.0, 1, 0, 1.0 / 4096, 0.0, 7),
    ]


def test_loss_scale_ref_is_capped_at_max_scale():
    assert _run_trace(1024.0, [False] * 4, interval=1, growth=4.0, max_scale=5000.0) == [
        (4096.0, 0, 0, 1.0 / 1024, 0.0, 1),
        (5000.0, 0, 0, 1.0 / 4096, 0.0, 2),         # 16384 > max_scale
        (5000.0, 0, 0, float(np.float32(1.0) / np.float32(5000.0)), 0.0, 3),
        (5000.0, 0, 0, float(np.float32(1.0) / np.float32(5000.0)), 0.0, 4),
    ]


def test_loss_scale_ref_floor_is_one():
    assert _run_trace(4.0, [True, True, True], backoff=0.25) == [
        (1.0, 0, 1, 0.25, 1.0, 1),
        (1.0, 0, 2, 1.0, 1.0, 1),                   # 0.25 -> floor 1.0
        (1.0, 0, 3, 1.0, 1.0, 1),
    ]


def test_loss_scale_ref_two_overflows_in_a_row_reset_the_good_count():
    assert _run_trace(1024.0, [False, False, True, True, False, False, False], interval=3) == [
        (1024.0, 1, 0, 1.0 / 1024, 0.0, 1),
        (1024.0, 2, 0, 1.0 / 1024, 0.0, 2),
        (512.0, 0, 1, 1.0 / 1024, 1.0, 2),          # one short of the interval: back to zero
        (256.0, 0, 2, 1.0 / 512, 1.0, 2),
        (256.0, 1, 2, 1.0 / 256, 0.0, 3),
        (256.0, 2, 2, 1.0 / 256, 0.0, 4),
        (512.0, 0, 2, 1.0 / 256, 0.0, 5),
    ]


def test_loss_scale_ref_more_skipped_steps_than_the_step_count_clamps_t():
    """A restored state with 5 skipped steps and an optimizer at step 2: t = max(2 - 5, 1) = 1, and the step size is that of t = 1."""
    from egovlp_amd.optim import adamw_step_size
    st = {"scale": np.float32(64.0), "good": 0, "skipped": 5, "inv": np.float32(1.0 / 64), "skip": 0.0}
    new, hyper = R.loss_scale_ref(st, False, 1e-2, 0.9, 0.999, 2, 1, 2.0, 0.5, 3, 2.0 ** 24)
    assert (float(new["scale"]), new["good"], new["skipped"]) == (64.0, 1, 5)
    assert hyper == [R.f32(1e-2), adamw_step_size(R.f32(1e-2), R.f32(0.9), R.f32(0.999), 1), 1.0 / 64, 0.0]
    new2, hyper2 = R.loss_scale_ref(new, True, 1e-2, 0.9, 0.999, 3, 0, 2.0, 0.5, 3, 2.0 ** 24)
    assert (float(new2["scale"]), new2["good"], new2["skipped"]) == (32.0, 0, 6)
    assert hyper2 == [R.f32(1e-2), R.f32(1e-2), 1.0 / 64, 1.0]          # correct_bias = 0: the step size is lr


def test_loss_scale_ref_without_advance_changes_only_the_hyper_block():
    st = {"scale": np.float32(100.0), "good": 2, "skipped": 1, "inv": np.float32(0.125), "skip": 1.0}
    new, hyper = R.loss_scale_ref(st, True, 3e-3, 0.9, 0.999, 4, 0, 2.0, 0.5, 3, 2.0 ** 24, advance=0)
    assert new == st
    assert hyper == [R.f32(3e-3), R.f32(3e-3), 0.125, 1.0]              # 1 / S and skip as the advancing call of this step left them


def test_loss_scale_ref_rounds_the_scale_to_fp32():
    rows = _run_trace(1000.0, [False, True], interval=1, growth=1.7, backoff=0.3)
    s1 = np.float32(1000.0) * np.float32(1.7)
    s2 = np.float32(s1) * np.float32(0.3)
    assert rows[0][0] == float(s1) and rows[1][0] == float(s2)
    assert float(s1) != 1000.0 * R.f32(1.7)                             # the fp64 product of the same fp32 factors is another number


# ------------------------------------------------------------------------------------------------------------------------- helpers
def test_split_bf16_ref():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -9, 3.14159274, -1e-30, 0.0, 65504.0])
    hi, lo = R.split_bf16_ref(x)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16
    assert float(hi[1]) == 1.0 and float(lo[1]) == 2.0 ** -9            # the half-way case goes to the even neighbour, lo holds the rest
    assert bool(((hi.float() + lo.float() - x).abs() <= 2.0 ** -17 * x.abs()).all())


def test_arena_guards_alignment_and_detection():
    specs = [(5, 0), (0, 0), (16385, 1), (4, 3), (1, 2), (1024, 0)]
    a = R.Arena(specs)
    base = a.bits.data_ptr()
    for (n, mis), v, off in zip(specs, a.views, a.offsets):
        assert v.numel() == n
        if n:
            assert (v.data_ptr() - base) == 4 * off and v.data_ptr() % 16 == 4 * mis
        assert bool((a.bits[off - R.GUARD:off] == a.sentinel).all()) and bool((a.bits[off + n:off + n + R.GUARD] == a.sentinel).all())
    for i in range(len(specs) - 1):
        assert a.offsets[i + 1] - (a.offsets[i] + a.numels[i]) >= R.GUARD
    a.fill([torch.arange(n, dtype=torch.float32) for n, _ in specs])
    a.assert_guards()
    assert torch.equal(a.tensors_cpu()[2], torch.arange(16385, dtype=torch.float32))
    a.flat[a.offsets[2] + 16385] = 0.0                                  # one element behind tensor 2
    with pytest.raises(AssertionError, match="guard"):
        a.assert_guards()
    b = R.Arena([(7, 1), (8, 0)], dtype=torch.bfloat16)
    assert b.views[0].data_ptr() % 8 == 2 and b.views[1].data_ptr() % 16 == 0
    assert bool(torch.isnan(b.flat[:R.GUARD].float()).all())            # the sentinel is a NaN: an over-reading scan trips on it


def test_case_generator_covers_what_it_promises():
    for name, T in (("adamw", 48), ("nonfinite", 96)):
        for count in (T - 1, T, T + 1, 2 * T + 1):
            numels = R.layout_sizes(count, T, 5)
            nz = [n for n in numels if n]
            assert len(nz) == count and numels.count(0) >= 3 and numels[0] == 0
            assert set(R.SIZES) <= set(nz)
            if count > T:
                assert nz[T] == 65536 + 4096 + 4 and nz[T - 1] == 16388            # a big tensor on each side of the flush
            plan = R.misalign_plan(numels, "pgmv", 5)
            if count >= T - 1:
                for s in "pgmv":                                                   # every stream misaligned on its own somewhere
                    others = [t for t in "pgmv" if t != s]
                    assert any(plan[s][i] and not any(plan[o][i] for o in others) for i in range(len(numels))), (count, s)
                assert any(all(plan[s][i] for s in "pgmv") for i in range(len(numels)))


def test_table_sizes_and_chunk_match_the_sources():
    """The boundary cases of tests/test_gpu_multi_tensor.py are built from R.TABLE / R.CHUNK: if a kernel's table size changes, this
    fails instead of the GPU cases quietly testing the interior."""
    for fname, want in R.SOURCE_CONSTANTS.items():
        have = R.source_constants(fname)
        for name, value in want.items():
            assert have.get(name) == value, (fname, name, have.get(name), value)
    assert R.TABLE == {"adamw": 48, "nonfinite": 96, "accumulate": 120, "gradsync": 96, "split": 40, "f16x2": 48, "splitk_reduce": 8}
    assert R.CHUNK == 16384


# ------------------------------------------------------------------------------------------------------------------------- work list
MT_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "multi_tensor.h"

struct Table {
  int item[3];
  MtIndex<3> ix;
};

// argv: <launch call that fails, 0 = none> <what it returns> <block count of every item ...>
int main(int argc, char** argv) {
  const int fail_at = atoi(argv[1]), fail_rc = atoi(argv[2]);
  std::vector<long long> blocks;
  for (int a = 3; a < argc; ++a) blocks.push_back(atoll(argv[a]));
  int calls = 0;
  const int rc = mt_for_each_launch<Table>(
      (int)blocks.size(), [&](int i) -> int64_t { return blocks[i]; }, [&](Table& t, int slot, int i) { t.item[slot] = i; },
      [&](const Table& t, int nb) -> int {
        printf("launch nb %d count %d items", nb, t.ix.count);
        for (int k = 0; k < t.ix.count; ++k) printf(" %d", t.item[k]);
        printf(" blk_start");
        for (int k = 0; k <= t.ix.count; ++k) printf(" %d", t.ix.blk_start[k]);
        printf("\n");
        return ++calls == fail_at ? fail_rc : 0;
      });
  printf("result %d\n", rc);
  return 0;
}
"""

G = R.MT_MAX_GRID
MT_CASES = [                                                        # (id, block counts, launch call that fails, its result)
    ("empty", [], 0, 0),
    ("only-zeros", [0, 0], 0, 0),
    ("zeros-front-middle-end", [0, 0, 5, 0, 2, 0, 0, 9, 4, 0, 0], 0, 0),
    ("3-items-one-launch", [4, 1, 7], 0, 0),
    ("4-items-two-launches", [4, 1, 7, 2], 0, 0),
    ("7-items-three-launches", [1, 2, 3, 4, 5, 6, 7], 0, 0),
    ("negative-first", [-1, 1, 1, 1, 1], 0, 0),
    ("negative-behind-the-first-table", [1, 1, 1, -1, 1], 0, 0),
    ("negative-last", [1, 1, 1, 1, 1, 1, -5], 0, 0),
    ("one-item-of-2^31-blocks", [1, G + 1], 0, 0),
    ("two-items-of-2^31-1-blocks", [G, G], 0, 0),
    ("sum-past-2^31-1-with-room-in-the-table", [G - 1, 1, 1], 0, 0),
    ("second-launch-returns-7", [1, 2, 3, 4, 5, 6, 7], 2, 7),
]


@pytest.fixture(scope="module")
def mt_driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("mt_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(MT_DRIVER)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egovlp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", csrc,
                           str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("case", MT_CASES, ids=[c[0] for c in MT_CASES])
def test_mt_for_each_launch_follows_the_plan(mt_driver, case):
    """mt_for_each_launch with a table of 3 items and a recording `launch`: the grid, the count, the item of every slot and the
    blk_start row of every launch, and the result, equal R.mt_plan's -- an invalid item anywhere launches nothing."""
    _, blocks, fail_at, fail_rc = case
    run = subprocess.run([mt_driver, str(fail_at), str(fail_rc)] + [str(b) for b in blocks], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
    result, launches = R.mt_plan(blocks, 3, [fail_rc if k + 1 == fail_at else 0 for k in range(fail_at)])
    want = ["launch nb %d count %d items %s blk_start %s" % (nb, len(items), " ".join(map(str, items)), " ".join(map(str, starts)))
            for nb, items, starts in launches] + ["result %d" % result]
    assert run.stdout.splitlines() == want


def test_mt_plan_on_cases_written_out_by_hand():
    assert R.mt_plan([], 3) == (0, [])
    assert R.mt_plan([0, 5, 0, 2], 3) == (0, [(7, [1, 3], [0, 5, 7])])
    assert R.mt_plan([4, 1, 7, 2], 3) == (0, [(12, [0, 1, 2], [0, 4, 5, 12]), (2, [3], [0, 2])])
    assert len(R.mt_plan([1] * 7, 3)[1]) == 3
    assert R.mt_plan([1, 1, 1, -1], 3) == (1, []) and R.mt_plan([G + 1], 3) == (1, [])
    assert R.mt_plan([G, G], 3) == (0, [(G, [0], [0, G]), (G, [1], [0, G])])
    assert R.mt_plan([1] * 7, 3, [0, 7]) == (7, [(3, [0, 1, 2], [0, 1, 2, 3]), (3, [3, 4, 5], [0, 1, 2, 3])])
