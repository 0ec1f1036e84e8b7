"""Every call egv_block_fwd / _bwd and egv_text_layer_fwd / _bwd make, with every argument, without a GPU.

csrc/block.hip and csrc/text_layer.hip hold no device code: `hipcc --cuda-host-only -c` compiles them on any machine, and what they
leave undefined is the library's own entry points plus hipEventRecord / hipStreamWaitEvent.  tools/block_call_census.cpp answers
those with a recording stub (each call printed with its scalars, every field of every egv_gemm_desc, every pointer as region + byte
offset) and sweeps the geometries: every (fwd_passes, bwd_passes, train, z_bf16, f16_single) at three block sizes, the backward with
and without gradient planes, three split-K tables and three side-stream deals, a sample of refused geometries and of missing
pointers, the arena sizes, offsets and gradient layouts, and a small sweep of the text layer.

    python tools/block_call_census.py run [--root TREE] > census.txt     the full text (some 100 MB)
    python tools/block_call_census.py digests [--root TREE]              one sha256 per group (entry point, passes, train)
    python tools/block_call_census.py check                              digests of this tree against tests/golden/block_call_census.sha256

A refactor of the two files leaves the full text byte-identical: run it on both trees and compare (profiles/block_plan_census.txt).
"""
import argparse
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_call_census.sha256")


def find_hipcc():
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.path.exists(p)), None)


def build(root, workdir, hipcc=None):
    """Compile the two host files of the tree at `root` and the recording stub of THIS tree into workdir/census."""
    hipcc = hipcc or find_hipcc()
    if hipcc is None:
        raise RuntimeError("no hipcc")
    csrc, inc = os.path.join(root, "egovlp_amd", "csrc"), os.path.join(root, "include")
    flags = [hipcc, "--cuda-host-only", "-O1", "-fPIC", "-std=c++17", "-Wno-unused-value", "-I", inc, "-I", csrc, "-c"]
    objs = []
    for src in (os.path.join(csrc, "block.hip"), os.path.join(csrc, "text_layer.hip"), os.path.join(HERE, "block_call_census.cpp")):
        obj = os.path.join(workdir, os.path.basename(src) + ".o")
        subprocess.check_call(flags + (["-x", "hip"] if src.endswith(".cpp") else []) + [src, "-o", obj])
        objs.append(obj)
    exe = os.path.join(workdir, "census")
    # a plain C++ link: nothing of the HIP runtime is needed (or wanted) behind the stub
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    linker = shutil.which("g++") or shutil.which("c++") or clang
    subprocess.check_call([linker] + objs + ["-o", exe])
    return exe


def groups(exe):
    """-> ({group: sha256 over its cases' text}, cases, lines, sha256 of everything) of one run of the census program."""
    proc = subprocess.Popen([exe], stdout=subprocess.PIPE)
    per, whole, cur, cases, lines = {}, hashlib.sha256(), None, 0, 0
    for line in proc.stdout:
        whole.update(line)
        lines += 1
        if line.startswith(b"@ "):
            cases += 1
            cur = per.setdefault(line[2:].split(b" | ")[0].decode(), hashlib.sha256())
        cur.update(line)
    if proc.wait() != 0:
        raise RuntimeError("census program failed: %d" % proc.returncode)
    return {k: h.hexdigest() for k, h in per.items()}, cases, lines, whole.hexdigest()


def digest_text(per):
    return "".join("%s  %s\n" % (per[k], k) for k in sorted(per))


def read_golden(path=GOLDEN):
    return {name: dg for dg, name in (ln.rstrip("\n").split("  ", 1) for ln in open(path) if ln.strip())}


def mismatches(per, golden):
    """The groups whose digest differs from, is missing in, or is not known to the golden file."""
    return sorted(k for k in set(per) | set(golden) if per.get(k) != golden.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=["run", "digests", "check"])
    ap.add_argument("--root", default=ROOT, help="the tree whose block.hip / text_layer.hip are compiled (default: this one)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(os.path.abspath(args.root), tmp)
        if args.what == "run":
            return subprocess.call([exe])
        per, cases, lines, whole = groups(exe)
    if args.what == "digests":
        sys.stdout.write(digest_text(per))
        print("# %d cases, %d lines, sha256 %s" % (cases, lines, whole), file=sys.stderr)
        return 0
    bad = mismatches(per, read_golden())
    for k in bad:
        print("DIFFERENT: %s" % k)
    print("%d groups, %d cases, %d lines: %s" % (len(per), cases, lines, "as recorded" if not bad else "%d groups differ" % len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
