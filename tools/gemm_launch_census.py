"""Which GEMM kernels a library launches, with what grid, block and LDS: one egv_gemm_nt call per case over a fixed list that reaches
every instance of the product library, to be traced and compared between two builds.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o census -- python tools/gemm_launch_census.py run [--lib LIBRARY]
    python tools/gemm_launch_census.py parse DIR/.../census_kernel_trace.csv > this.txt
    python tools/gemm_launch_census.py compare parent.txt this.txt          (-> the report kept as profiles/gemm_dispatch_census.txt)

Run it twice per library, at the default environment and with EGV_X2_SEG=0 (f16x2 operands on the fused two-product instances, PROD 2,
instead of two k-segments of the fp16 loop, PROD 1).  The cases:
  small    128x128x64, passes 1 and 3, un-split and ksplit 2 (+ the epilogue reduce)
  tn       256x256x128 weight gradients, bf16 and fp16: ksplit 1, ksplit 2 (+ the slab reduce with its column sums), accumulate 2
  mf4      256x256x64, every NT epilogue of every product kind that one tile reaches: the fp16 kinds (PROD 1, 2) take the big kernel
           at any tile count; a bf16 / bf16x3 product (PROD 0, 3) of one tile reaches the big kernel only as 128 k-slices (RAW)
  mf4-tall 5376x3072x64: the PROD 0 / 3 epilogues at MF 4 that 256x256x64 cannot reach
  mf5      5384x3072x64, every NT epilogue of every product kind
  mixed    7176x2304x64 with grid_cap 8: LINEAR and GELU for PROD 3 and, EGV_X2_SEG=0, LINEAR, GELU and GELU_X2 for PROD 2"""
import argparse
import csv
import ctypes as C
import os
import re
import sys

NONE, GELU, GELU_BWD, RELU_BWD = range(4)
# epilogue -> the descriptor fields that select it
EPILOGUES = {
    "RAW": dict(outputs=("out_f32",)),
    "LINEAR": dict(outputs=("out_f32", "bias", "residual")),
    "GELU": dict(act=GELU, outputs=("out_hi", "out_lo", "bias", "aux_out")),
    "GELU_BWD": dict(act=GELU_BWD, outputs=("out_f32", "aux_in")),
    "GENERIC": dict(act=RELU_BWD, outputs=("out_f32", "aux_in")),
    "GELU_X2": dict(act=GELU, out_fmt=1, aux_bf16=2, outputs=("out_hi", "out_lo", "bias", "aux_out")),
    "GELU_X2-one-plane": dict(act=GELU, out_fmt=2, aux_bf16=2, outputs=("out_hi", "bias", "aux_out")),
}
# passes -> its epilogues at the default environment (passes 2 = PROD 1) / with EGV_X2_SEG=0 (passes 2 = PROD 2)
BY_PASSES = {1: ("RAW", "LINEAR", "GELU", "GELU_BWD", "GENERIC"), 3: ("RAW", "LINEAR", "GELU", "GELU_BWD", "GENERIC"),
             4: ("RAW", "LINEAR", "GELU_X2-one-plane", "GELU_BWD")}
F16X2 = {False: ("RAW", "LINEAR", "GELU_X2", "GELU_BWD"), True: ("RAW", "LINEAR", "GELU", "GELU_X2")}


def cases(fused_x2):
    out = []
    for passes in (1, 3):
        out.append(("small x%d" % passes, dict(M=128, N=128, K=64, passes=passes)))
        out.append(("small x%d ksplit 2" % passes, dict(M=128, N=128, K=64, passes=passes, ksplit=2)))
    for passes in (1, 4):
        tn = dict(M=256, N=256, K=128, passes=passes, trans=1, outputs=("out_f32", "colsum"))
        out += [("tn x%d" % passes, tn), ("tn x%d ksplit 2" % passes, dict(tn, ksplit=2)),
                ("tn x%d ksplit 2 slabs left" % passes, dict(tn, ksplit=2, accumulate=2))]
    eps = {**BY_PASSES, 2: F16X2[fused_x2]}
    for passes in (2, 4):
        out += [("mf4 x%d %s" % (passes, e), dict(M=256, N=256, K=64, passes=passes, **EPILOGUES[e])) for e in eps[passes]]
    for passes in (1, 3):
        out.append(("mf4 x%d RAW 128 k-slices" % passes, dict(M=256, N=256, K=8192, passes=passes, ksplit=128)))
        out += [("mf4-tall x%d %s" % (passes, e), dict(M=5376, N=3072, K=64, passes=passes, **EPILOGUES[e])) for e in eps[passes]]
    for passes in (1, 2, 3, 4):
        out += [("mf5 x%d %s" % (passes, e), dict(M=5384, N=3072, K=64, passes=passes, **EPILOGUES[e])) for e in eps[passes]]
    for passes, names in ((3, ("LINEAR", "GELU")), (2, ("LINEAR", "GELU", "GELU_X2") if fused_x2 else ())):
        out += [("mixed x%d %s" % (passes, e), dict(M=7176, N=2304, K=64, passes=passes, grid_cap=8, **EPILOGUES[e])) for e in names]
    return out


def run(lib):
    if lib:
        os.environ["EGOVLP_HIP_LIB"] = os.path.abspath(lib)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from egovlp_amd import _lib
    h = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    fused_x2 = (int(os.environ.get("EGV_X2_SEG", "2")) & 2) == 0
    for name, c in cases(fused_x2):
        M, N, K, ks = c["M"], c["N"], c["K"], c.get("ksplit", 1)
        outputs = c.get("outputs", ("out_f32",))
        zeros = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
        t = {k: zeros((M if k[0] == "a" else N) * K, torch.int16) for k in ("a_hi", "a_lo", "b_hi", "b_lo")}
        t.update({k: zeros(M * N) for k in ("out_f32", "residual", "aux_in", "aux_out")})
        t.update({"out_hi": zeros(M * N, torch.int16), "out_lo": zeros(M * N, torch.int16), "bias": zeros(N), "colsum": zeros(M),
                  "partial": zeros(ks * M * N + ks * M) if ks > 1 else None})
        p = lambda k: t[k].data_ptr() if (k in outputs or k[:2] in ("a_", "b_") or (k == "partial" and ks > 1)) else None  # noqa: E731
        trans = c.get("trans", 0)
        d = _lib.GemmDesc(p("a_hi"), p("a_lo"), (M if trans else K), p("b_hi"), p("b_lo"), (N if trans else K), M, N, K, c["passes"], 1.0,
                          c.get("act", NONE), p("bias"), p("residual"), N, p("aux_in"), p("aux_out"), N, p("out_f32"), N, p("out_hi"),
                          p("out_lo"), N, ks, c.get("accumulate", 0), p("partial"), trans, c.get("aux_bf16", 0), p("colsum"),
                          c.get("grid_cap", 0), c.get("out_fmt", 0), None)
        rc = h.egv_gemm_nt(C.byref(d), stream)
        torch.cuda.synchronize()
        print("case %-28s rc %d" % (name, rc), flush=True)
        if rc:
            return 1
    return 0


def parse(path):
    rows = [r for r in csv.DictReader(open(path)) if "gemm_" in r["Kernel_Name"] or "splitk_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))

    def col(r, *names):
        for nm in names:
            if nm in r:
                return r[nm]
        raise SystemExit("no column of %s in %s" % (names, sorted(r)))

    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        name = re.sub(r"^void ", "", name).split("(")[0]
        print("%s grid %s,%s block %s lds %s" % (name, col(r, "Grid_Size_X", "Grid_Size"), r.get("Grid_Size_Y", "-"),
                                                 col(r, "Workgroup_Size_X", "Workgroup_Size"),
                                                 col(r, "LDS_Block_Size", "LDS_Block_Size_v", "Lds_Block_Size")))


def compare(parent, this):
    a, b = open(parent).read().splitlines(), open(this).read().splitlines()
    print("GEMM launches over the case list of tools/gemm_launch_census.py: (kernel, grid in threads x, y, block, LDS bytes) in launch order")
    print("(LDS as the trace's LDS_Block_Size column has it: the kernel's static LDS -- dynamic LDS shows 0; the dynamic byte counts of every")
    print(" pick are pinned on the CPU, tests/test_gemm_dispatch_cpu.py)")
    print("parent: %d launches, this tree: %d launches: %s" % (len(a), len(b), "identical" if a == b else "DIFFERENT"))
    for i in range(max(len(a), len(b)) if a != b else 0):
        x, y = (a[i] if i < len(a) else "-"), (b[i] if i < len(b) else "-")
        if x != y:
            print("!! %4d parent: %s\n        this:   %s" % (i, x, y))
    print("distinct kernels: %d" % len({x.split(" grid ")[0] for x in b}))
    print("---- parent\n%s\n---- this tree\n%s" % ("\n".join(a), "\n".join(b)))
    return 0 if a == b else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["run", "parse", "compare"])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--lib", default=None, help="the library whose launches are counted (default: this tree's)")
    args = ap.parse_args()
    if args.what == "run":
        return run(args.lib)
    if args.what == "parse":
        return parse(args.files[0])
    return compare(*args.files)


if __name__ == "__main__":
    sys.exit(main())
