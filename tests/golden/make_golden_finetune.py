"""Generate the goldens of the ranking-loss head by RUNNING THE REFERENCE ITSELF (model/model.py sim_matrix, model/loss.py
MaxMarginRankingLoss / AdaptiveMaxMarginRankingLoss, torch autograd), in fp32 and again on the same inputs cast to fp64.
Run once where the reference is available:
    python tests/golden/make_golden_finetune.py
Writes finetune_head.npz next to this file.  Per case `c` of tests/finetune_ref.py CASES:
  c_seed                      the inputs are finetune_ref.make_inputs(c, seed); stored in full (c_text, c_video, c_weight) for n <= 48
  c_loss32, c_loss64          the reference's loss in the two precisions
  c_e, c_tau                  e = max |x_fp32 - x_fp64| of the reference's own sim_matrix, tau = 10 e
  c_n_amb, c_n_kept, c_active ambiguous hinge terms (fp64 argument within tau of zero), kept terms, share of active hinges
  c_err32_dt, c_err32_dv      relative Frobenius error of the reference's fp32 gradients against its fp64 ones
  n <= 48:  c_dt64, c_dv64, c_sim64  the fp64 gradients and similarity, stored rounded to fp32 (2^-24 relative, far below the bars)
  n >  48:  c_dt64_proj, c_dv64_proj  the fp64 gradients times finetune_ref.projection(D) [n, 8] (fp64), c_dt64_norm, c_dv64_norm,
            c_dt64_rows, c_dv64_rows (per-row norms): what tests/finetune_ref.py's fp64 head is pinned to, so that the tests can
            compare FULL gradients against it without a multi-megabyte file.
A hinge has no gradient at its corner: for n <= 200 seeds are searched until NO term is ambiguous and 0.15 <= active <= 0.6, so
these cases compare in full.  At n = 1024 no seed is clean; the first seed with fewer than 1e-4 ambiguous terms is taken and
the tests allow exactly the fp64 gradient those terms contribute (finetune_ref.ambiguous_allowance)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))

import finetune_ref as FR  # noqa: E402
from oracle import ref_import  # noqa: E402


def reference_run(mm, ml, name, text, video, weight, dtype):
    n, D, adaptive, fix_norm, _ = FR.CASES[name]
    t = text.detach().to(dtype).clone().requires_grad_(True)
    v = video.detach().to(dtype).clone().requires_grad_(True)
    x = mm.sim_matrix(t, v)
    if adaptive:
        loss = ml.AdaptiveMaxMarginRankingLoss(margin=FR.margin_of(True), fix_norm=fix_norm)(x, weight.to(dtype))
    else:
        loss = ml.MaxMarginRankingLoss(margin=FR.margin_of(False), fix_norm=fix_norm)(x)
    loss.backward()
    return loss.detach(), x.detach(), t.grad, v.grad


def main():
    assert ref_import.available(), "needs the reference checkout"
    mm, ml, _, _ = ref_import.load_reference()
    torch.set_num_threads(8)
    out = {}
    for name, (n, D, adaptive, fix_norm, _) in FR.CASES.items():
        margin = FR.margin_of(adaptive)
        for seed in range(1, 400):
            text, video, weight = FR.make_inputs(name, seed)
            l32, x32, dt32, dv32 = reference_run(mm, ml, name, text, video, weight, torch.float32)
            l64, x64, dt64, dv64 = reference_run(mm, ml, name, text, video, weight, torch.float64)
            e = float((x32.double() - x64).abs().max())
            tau = 10.0 * e
            w64 = None if weight is None else weight.double()
            ar, ac, active = FR.ambiguous(x64, w64, margin, fix_norm, tau)
            n_amb = int(ar.sum() + ac.sum())
            n_kept = int(2 * FR.kept(n, fix_norm).sum())
            ok_share = 0.15 <= active <= 0.6
            if ok_share and (n_amb == 0 if n <= 200 else n_amb < 1e-4 * n_kept):
                break
        else:
            raise RuntimeError(f"{name}: no seed found")
        print(f"{name}: seed {seed} e {e:.2e} tau {tau:.2e} ambiguous {n_amb}/{n_kept} active {active:.3f} loss32 {float(l32):.8f} "
              f"loss64 {float(l64):.10f} err32 dt {FR.rel_fro(dt32, dt64):.2e} dv {FR.rel_fro(dv32, dv64):.2e}")
        out[name + "_seed"] = np.int64(seed)
        out[name + "_loss32"] = np.float32(float(l32))
        out[name + "_loss64"] = np.float64(float(l64))
        out[name + "_e"] = np.float64(e)
        out[name + "_tau"] = np.float64(tau)
        out[name + "_n_amb"] = np.int64(n_amb)
        out[name + "_n_kept"] = np.int64(n_kept)
        out[name + "_active"] = np.float64(active)
        out[name + "_err32_dt"] = np.float64(FR.rel_fro(dt32, dt64))
        out[name + "_err32_dv"] = np.float64(FR.rel_fro(dv32, dv64))
        if n <= FR.FULL_MAX_N:
            out[name + "_text"] = text.numpy()
            out[name + "_video"] = video.numpy()
            if weight is not None:
                out[name + "_weight"] = weight.numpy()
            out[name + "_dt64"] = dt64.float().numpy()
            out[name + "_dv64"] = dv64.float().numpy()
            out[name + "_sim64"] = x64.float().numpy()
        else:
            P = FR.projection(D)
            out[name + "_dt64_proj"] = (dt64 @ P).numpy()
            out[name + "_dv64_proj"] = (dv64 @ P).numpy()
            out[name + "_dt64_norm"] = np.float64(float(dt64.norm()))
            out[name + "_dv64_norm"] = np.float64(float(dv64.norm()))
            out[name + "_dt64_rows"] = dt64.norm(dim=1).numpy()
            out[name + "_dv64_rows"] = dv64.norm(dim=1).numpy()
    path = os.path.join(HERE, "finetune_head.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
