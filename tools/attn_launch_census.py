"""Which attention kernels a tree launches, with what grid, block and LDS: one forward and one backward call per case over a fixed
list that reaches every kernel family and instance, to be traced and compared between two trees.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o census -- python tools/attn_launch_census.py run [--root TREE]
    python tools/attn_launch_census.py parse DIR/.../census_kernel_trace.csv > this.txt
    python tools/attn_launch_census.py compare parent.txt this.txt          (-> the report kept as profiles/attn_dispatch_census.txt)

Space: n = 3, 40, 64, 224, 288 locations at T = 2; time: T = 2, 5, 9, 17, 33, 49 frames at n = 3; text: L = 8, 40, 65, 225, 289 tokens.
Each in bf16x3 (three products), in single bf16 (one product) and -- space and time -- in the fp16 pairing (fp16-split qkv through
the three-product forward into ONE fp16 output plane, fp16 dO / dqkv through the one-product backward).  B = 1, H = 1."""
import argparse
import csv
import os
import re
import sys

SPACE_N, TIME_T, TEXT_L = (3, 40, 64, 224, 288), (2, 5, 9, 17, 33, 49), (8, 40, 65, 225, 289)


def run(root):
    sys.path.insert(0, root)
    import torch
    from egovlp_amd import ops
    B = H = 1
    g = torch.Generator().manual_seed(5)

    def bf16_planes(rows, cols, passes):
        x = torch.randn((rows, cols), generator=g) * 0.5
        hi = x.to(torch.bfloat16)
        return ops.Planes(hi.cuda(), (x - hi.float()).to(torch.bfloat16).cuda() if passes == 3 else None, rows, cols)

    def f16_planes(rows, cols, single):
        x = torch.randn((rows, cols), generator=g) * 0.5
        hi = x.to(torch.float16)
        return ops.Planes(hi.cuda(), None if single else (x - hi.float()).to(torch.float16).cuda(), rows, cols, "f16" if single else "f16s")

    for mode, cases in ((0, [(2, n) for n in SPACE_N]), (1, [(T, 3) for T in TIME_T])):
        for T, n in cases:
            S = 1 + T * n
            for passes in (3, 1):
                qkv = bf16_planes(B * S, 3 * H * 64, passes)
                out, lse = ops.divided_attn_fwd(qkv, B, T, n, H, mode, passes)
                ops.divided_attn_bwd(qkv, out, bf16_planes(B * S, H * 64, passes), lse, B, T, n, H, mode, passes)
            qkv = f16_planes(B * S, 3 * H * 64, False)
            out, lse = ops.divided_attn_fwd(qkv, B, T, n, H, mode, 3, out_fmt="f16")
            ops.divided_attn_bwd(qkv, out, f16_planes(B * S, H * 64, True), lse, B, T, n, H, mode, 1, grad_f16=True)
    for L in TEXT_L:
        q, k, v, d_out = (torch.randn((B * L, H * 64), generator=g).cuda() for _ in range(4))
        mask = torch.ones((B, L), dtype=torch.int64, device="cuda")
        for passes in (3, 1):
            _, lse = ops.text_attn_fwd(q, k, v, mask, B, L, H, passes)
            ops.text_attn_bwd(q, k, v, mask, d_out, lse, B, L, H, passes)
    torch.cuda.synchronize()


def parse(path):
    rows = [r for r in csv.DictReader(open(path)) if "attn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))

    def col(r, *names):
        for nm in names:
            if nm in r:
                return r[nm]
        raise SystemExit("no column of %s in %s" % (names, sorted(r)))

    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        name = re.sub(r"^void ", "", name).split("(")[0]
        print("%s grid %s block %s lds %s" % (name, col(r, "Grid_Size_X", "Grid_Size"), col(r, "Workgroup_Size_X", "Workgroup_Size"),
                                              col(r, "LDS_Block_Size", "LDS_Block_Size_v", "Lds_Block_Size")))


def compare(parent, this):
    a, b = open(parent).read().splitlines(), open(this).read().splitlines()
    print("attention launches over the case list of tools/attn_launch_census.py: (kernel, grid in threads, block, LDS bytes) in launch order")
    print("(LDS as the trace's LDS_Block_Size column has it: the kernel's static LDS -- a kernel whose LDS is dynamic shows 0; the dynamic")
    print(" byte counts of every pick are pinned on the CPU, tests/test_attn_dispatch_cpu.py)")
    print("parent: %d launches, this tree: %d launches: %s" % (len(a), len(b), "identical" if a == b else "DIFFERENT"))
    for i in range(max(len(a), len(b)) if a != b else 0):
        x, y = (a[i] if i < len(a) else "-"), (b[i] if i < len(b) else "-")
        if x != y:
            print("!! %4d parent: %s\n        this:   %s" % (i, x, y))
    print("---- parent\n%s\n---- this tree\n%s" % ("\n".join(a), "\n".join(b)))
    return 0 if a == b else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["run", "parse", "compare"])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the built tree whose package makes the calls")
    args = ap.parse_args()
    if args.what == "run":
        return run(args.root)
    if args.what == "parse":
        return parse(args.files[0])
    return compare(*args.files)


if __name__ == "__main__":
    sys.exit(main())
