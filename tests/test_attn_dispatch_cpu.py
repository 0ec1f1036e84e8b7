"""csrc/attn_dispatch.h on the CPU: the header is compiled on its own (g++, address + undefined-behaviour sanitizers) into a driver that
prints the result of every check and every field of every pick over a sweep of the boundaries; tests/attn_dispatch_ref.py, a
restatement of the launchers the header replaced, says what the lines have to be."""
import itertools
import os
import shutil
import subprocess

import pytest

import attn_dispatch_ref as R

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "attn_dispatch.h"

static void print_pick(int rc, const AttPick& p) {
  if (rc) { printf("%d\n", rc); return; }
  printf("0 %d %d %d %d %d %d %d %d %d\n", p.family, p.frags, p.products, p.f16, p.waves, p.threads, p.lds, p.grid, p.nblk);
}

// one case per input line: <kind> <arguments as tests/attn_dispatch_ref.py orders them>
int main() {
  std::string kind;
  while (std::cin >> kind) {
    long long a[11];
    double prob = 0.0;
    const int na = kind == "check_dfwd" ? 9 : kind == "check_dbwd" ? 11 : kind == "check_tfwd" ? 7 : kind == "check_tbwd" ? 7 : kind == "pick_time" ? 7 : 6;
    for (int i = 0; i < na; ++i) std::cin >> a[i];
    if (kind == "check_tfwd" || kind == "check_tbwd") {      // strtod: "nan" is a case
      std::string word;
      std::cin >> word;
      prob = strtod(word.c_str(), nullptr);
    }
    AttPick p = {};
    if (kind == "check_dfwd") {
      AttDividedFwd d = {};
      const int rc = att_check_divided_fwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6] != 0, a[7] != 0, a[8] != 0, &d);
      if (rc) printf("%d\n", rc); else printf("0 %d %d %d %d %d\n", d.time, d.out_fmt, d.f16, (int)d.qkv_lo, (int)d.out_lo);
    } else if (kind == "check_dbwd") {
      AttDividedBwd d = {};
      const int rc = att_check_divided_bwd(a[0], a[1], a[2], a[3], a[4], a[5], a[6] != 0, a[7] != 0, a[8] != 0, a[9] != 0, a[10] != 0, &d);
      if (rc) printf("%d\n", rc);
      else printf("0 %d %d %d %d %d %d %d %d\n", d.time, d.o_fmt, d.g_fmt, d.f16, (int)d.qkv_lo, (int)d.out_lo, (int)d.dout_lo, (int)d.dqkv_lo);
    } else if (kind == "check_tfwd") {
      bool out_lo = a[5] != 0;
      const int rc = att_check_text_fwd(a[0], a[1], a[2], a[3], a[4] != 0, &out_lo, a[6], (float)prob);
      if (rc) printf("%d\n", rc); else printf("0 %d\n", (int)out_lo);
    } else if (kind == "check_tbwd") {
      printf("%d\n", att_check_text_bwd(a[0], a[1], a[2], a[3], a[4] != 0, a[5], a[6], (float)prob));
    } else if (kind == "pick_fwd") {
      print_pick(att_pick_fwd(a[0] != 0, a[1], a[2], a[3], a[4], a[5], &p), p);
    } else if (kind == "pick_dq") {
      print_pick(att_pick_dq(a[0] != 0, a[1], a[2], a[3], a[4], a[5], &p), p);
    } else if (kind == "pick_dkv") {
      print_pick(att_pick_dkv(a[0] != 0, a[1], a[2], a[3], a[4], a[5], &p), p);
    } else if (kind == "pick_time") {
      print_pick(att_pick_time(a[0] != 0, a[1], a[2], a[3], a[4], a[5], a[6], &p), p);
    } else {
      return 2;
    }
  }
  return 0;
}
"""

ROWS = (1, 32, 33, 64, 65, 224, 225, 288, 289, 785)                 # keys / queries on both sides of every ladder step
FRAMES = (1, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65)
G = R.MAX_GRID
VARIANTS = ((1, 0), (3, 0), (3, 1), (1, 1))                         # (products, fp16 operands)


def sweep_space_text():
    """Every row count, space (n locations: n + 1 keys and n + 1 query rows with the CLS query) and text (L x L), every variant, on both
    sides of the 256-workgroup persistent grid; the backward with the query extent above the key extent's ladder step; grids at
    2^31 - 1 and 2^31."""
    cases = []
    for kind, rows, (products, f16), groups in itertools.product(("pick_fwd", "pick_dq", "pick_dkv"), ROWS, VARIANTS, (1, 255, 256, 257)):
        cases.append((kind, 1, groups, rows + 1, rows + 1, products, f16))
        cases.append((kind, 0, groups, rows, rows, products, 0))
    for kind, space, (nq, nk), products in itertools.product(("pick_dq", "pick_dkv", "pick_fwd"), (0, 1),
                                                             ((33, 20), (65, 64), (225, 100), (289, 288), (288, 289), (500, 30)), (1, 3)):
        cases.append((kind, space, 12, nq, nk, products, 0))
    for kind, space, rows in itertools.product(("pick_fwd", "pick_dq", "pick_dkv"), (0, 1), (32, 200, 785)):
        nblk = (rows + 127) // 128 if rows > 288 else 1
        for groups in (0, -1, G // nblk, G // nblk + 1, G, G + 1, 2 ** 40):
            cases.append((kind, space, groups, rows, rows, 3, 0))
    return cases


def sweep_time():
    cases = []
    for bwd, T, (products, f16), n in itertools.product((0, 1), FRAMES + (0,), VARIANTS, (1, 3, 4, 5, 196)):
        cases.append(("pick_time", bwd, 2, T, n, 12, products, f16))
    for bwd, T, products in itertools.product((0, 1), (4, 8, 16, 17, 64), (1, 3)):
        locs = {4: 4, 8: 2}.get(T, 1)
        wpb = 4 if not bwd or products == 1 else 2
        # the block count reaches 2^31 - 1 / 2^31: forward T <= 16 packs 4 waves of any (clip, head), the backward WPB units of one
        for B, n, H in ((G, 1, 1), (G, 4 * locs, 1), (G, 4 * locs + 1, 1), (2 ** 16, wpb * locs * 2 ** 15, 1),
                        (2 ** 16, wpb * locs * 2 ** 15 - 1, 1), (2 ** 20, 1, 2 ** 11), (2 ** 20, 1, 2 ** 13), (46341, 1, 46341)):
            cases.append(("pick_time", bwd, B, T, n, H, products, 0))
    return cases


def sweep_checks():
    """Every (passes, mode word, which second planes exist) combination of the divided entry points, accepted or not, in space and time
    (the mode's bit 0) at a valid and a refused T; the size, pointer and stride rules one at a time."""
    cases = []
    for passes, mode, qkv_lo, out_lo, T in itertools.product((1, 3, 2), range(-1, 17), (0, 1), (0, 1), (64, 65)):
        cases.append(("check_dfwd", 2, T, 5, 3, mode, passes, 1, qkv_lo, out_lo))
    for passes, mode, lo in itertools.product((1, 3, 2), range(-1, 33), range(16)):
        cases.append(("check_dbwd", 2, 9, 5, 3, mode, passes, 1, lo & 1, (lo >> 1) & 1, (lo >> 2) & 1, (lo >> 3) & 1))
    for mode, T in itertools.product((0, 1, 16, 25), FRAMES):
        cases.append(("check_dbwd", 1, T, 1, 1, mode, 1, 1, 0, 0, 0, 0))
    for kind, tail in (("check_dfwd", (1, 1)), ("check_dbwd", (1, 1, 1, 1))):
        for B, T, n, H, required in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (-3, 1, 1, 1, 1), (1, 1, 1, 1, 0),
                                     (1, 2 ** 16, 2 ** 15 - 1, 1, 1), (1, 2 ** 16, 2 ** 15, 1, 1), (2 ** 16, 1, 1, 2 ** 15, 1),
                                     (2 ** 16, 1, 1, 2 ** 15 - 1, 1), (46341, 1, 1, 46341, 1)):
            cases.append((kind, B, T, n, H, 0, 3, required) + tail)
    for passes, required, out_lo, ld, p in itertools.product((1, 3, 0), (0, 1), (0, 1), (767, 768, 770, 772, 2304), (0.0, 0.1, 1.0, -0.1, float("nan"))):
        cases.append(("check_tfwd", 2, 7, 12, passes, required, out_lo, ld, p))
        cases.append(("check_tbwd", 2, 7, 12, passes, required, ld, 768, p))
        cases.append(("check_tbwd", 2, 7, 12, passes, required, 768, ld, p))
    for B, L, H in ((0, 7, 12), (2, 0, 12), (2, 7, 0), (-1, 7, 12)):
        cases.append(("check_tfwd", B, L, H, 3, 1, 1, 2304, 0.0))
        cases.append(("check_tbwd", B, L, H, 3, 1, 2304, 2304, 0.0))
    return cases


SWEEPS = {"space-and-text-picks": sweep_space_text, "time-picks": sweep_time, "checks": sweep_checks}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("attn_dispatch_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egovlp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", csrc,
                           str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("name", list(SWEEPS))
def test_attn_dispatch_follows_the_launchers_it_replaced(driver, name):
    """Every check result and every field of every pick (family, fragments, products, fp16, waves, threads, LDS bytes, grid, blocks per
    group) equals what the former launchers did -- line by line over the sweep."""
    cases = SWEEPS[name]()
    text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    run = subprocess.run([driver], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
    got = run.stdout.splitlines()
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == R.expected(c), (c, g, R.expected(c))


def test_sweeps_cover_what_they_promise():
    picks = sweep_space_text()
    fams = {(c[0], R.expected(c).split()[1]) for c in picks if R.expected(c) != "1"}
    assert {f for _, f in fams} == {str(x) for x in (R.RESIDENT, R.STREAM, R.TEXT_STREAM, R.KEY_TILED)}
    assert {R.expected(c).split()[2] for c in picks if R.expected(c) != "1"} == {"0", "2", "4", "14", "18"}
    step = lambda rows: sum(rows > x for x in (32, 64, 224, 288))
    assert any(step(c[3]) > step(c[4]) for c in picks if c[0] == "pick_dq")      # the query extent, not the key extent, picks the count
    grids = [int(R.expected(c).split()[8]) for c in picks + sweep_time() if R.expected(c) != "1"]
    assert G in grids and 256 in grids and 255 in grids
    assert sum(R.expected(c) == "1" for c in picks) >= 9 and sum(R.expected(c) == "1" for c in sweep_time()) >= 20
    t = {(R.expected(c).split()[1], R.expected(c).split()[2]) for c in sweep_time() if R.expected(c) != "1"}
    assert t == {(str(R.TIME_TILE), "4"), (str(R.TIME_TILE), "8"), (str(R.TIME_TILE), "16"), (str(R.TIME_LONG), "2"), (str(R.TIME_LONG), "3"),
                 (str(R.TIME_LONG), "4")}
    checks = [R.expected(c) for c in sweep_checks()]
    assert 200 < sum(x != "1" for x in checks) < len(checks) - 1000


def test_ref_on_cases_written_out_by_hand():
    """(family, frags, products, f16, waves, threads, LDS bytes, grid, blocks per group), worked out from the kernels' own comments."""
    # ViT-B/16 space forward, three products, B T H = 16 * 4 * 12: the persistent streaming kernel, 4 planes of 224 rows + the key bias
    assert R.pick_fwd(1, 768, 197, 197, 3, 0) == (R.STREAM, 14, 3, 0, 16, 1024, 4 * 224 * 128 + 224 * 4, 256, 1)
    assert R.pick_fwd(1, 100, 197, 197, 3, 1) == (R.STREAM, 14, 3, 1, 16, 1024, 115584, 100, 1)
    assert R.pick_fwd(1, 768, 197, 197, 1, 0) == (R.RESIDENT, 14, 1, 0, 8, 512, 2 * 224 * 128 + 224 * 4, 768, 1)
    # DistilBERT, L = 32: two fragments
    assert R.pick_fwd(0, 384, 32, 32, 3, 0) == (R.RESIDENT, 2, 3, 0, 8, 512, 16512, 384, 1)
    # 448^2 input: 785 keys, 7 blocks of 128 query rows; the ring is two tiles of four 8 KiB planes + 256 B of key bias
    assert R.pick_fwd(1, 10, 785, 785, 3, 0) == (R.KEY_TILED, 0, 3, 0, 8, 512, 2 * (32768 + 256), 70, 7)
    dq, dkv = R.pick_bwd(1, 768, 197, 197, 1, 1)
    assert dq == (R.STREAM, 14, 1, 1, 8, 512, 2 * 224 * 128 + 224 * 4, 768, 1) and dkv == (R.RESIDENT, 14, 1, 1, 8, 512, 2 * 224 * 128 + 2 * 224 * 4, 768, 1)
    dq, dkv = R.pick_bwd(0, 24, 100, 100, 3, 0)
    assert dq == (R.TEXT_STREAM, 14, 3, 0, 8, 512, 116480, 24, 1) and dkv == (R.RESIDENT, 14, 3, 0, 4, 256, 116480, 24, 1)
    assert R.pick_bwd(0, 24, 33, 20, 1, 0)[0][1] == 4 and R.pick_bwd(0, 24, 20, 20, 1, 0)[0][1] == 2
    # time: T = 4 packs four locations into a wave: 196 locations = 49 units; forward 4 waves per block over 16 * 49 * 12 waves
    assert R.pick_time(0, 16, 4, 196, 12, 3, 0) == (R.TIME_TILE, 4, 3, 0, 4, 256, 0, 2352, 1)
    assert R.pick_time(1, 16, 4, 196, 12, 3, 0) == (R.TIME_TILE, 4, 3, 0, 2, 128, 0, 16 * 12 * 25, 1)
    assert R.pick_time(1, 16, 16, 196, 12, 1, 1) == (R.TIME_TILE, 16, 1, 1, 4, 256, 0, 16 * 12 * 49, 1)
    assert R.pick_time(0, 2, 33, 196, 12, 1, 0) == (R.TIME_LONG, 3, 1, 0, 3, 192, 0, 2 * 196 * 12, 1)
    assert R.pick_time(1, 1, 65, 1, 1, 1, 0) is None and R.pick_fwd(1, 2 ** 31, 197, 197, 3, 0) is None
    # the divided forward: mode = 2 fmt + time + 8 fp16
    assert R.check_divided_fwd(2, 4, 196, 12, 6, 3, True, True, False) == (0, 3, 0, 1, 0)          # ONE fp16 plane: no second plane needed
    assert R.check_divided_fwd(2, 4, 196, 12, 0, 3, True, True, False) is None
    assert R.check_divided_fwd(2, 4, 196, 12, 8, 1, True, True, True) is None                      # fp16 operands: three products
    assert R.check_divided_fwd(2, 4, 196, 12, 1, 1, True, True, True) == (1, 0, 0, 0, 0)
    assert R.check_divided_bwd(1, 65, 1, 1, 1, 1, True, False, False, False, False) is None
    assert R.check_divided_bwd(1, 4, 1, 1, 16, 1, True, False, False, False, False) is None         # bit 4 without bit 3
    assert R.check_divided_bwd(1, 4, 1, 1, 24 + 6, 1, True, True, True, True, True) == (0, 3, 4, 1, 0, 0, 0, 0)
    assert R.line(None) == "1" and R.line((0, 3)) == "0 0 3"
