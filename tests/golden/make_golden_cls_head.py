"""Generate the goldens of the classification head by RUNNING THE REFERENCE ITSELF: model/loss.py CrossEntropy, the literal loss
expressions of trainer/trainer_oscc.py:338 and trainer/trainer_pnr.py:350, model/metric.py oscc_metrics / pnr_metrics, on
torch.nn.functional.linear heads, in fp32 and again on the same inputs cast to fp64.  Run once where the reference is available:
    python tests/golden/make_golden_cls_head.py
Writes cls_head.npz next to this file.  Per case `c` of tests/cls_head_ref.py CASES (inputs are cls_head_ref.make_inputs(c, seed)):
  c_seed, c_loss32, c_loss64            the reference's loss in the two precisions
  c_dW64, c_db64, c_dfeats64, c_scores64  fp64 gradients (the local slice for dfeats) and scores, stored rounded to fp32
  c_pred                                 argmax of every fp64 score row (torch.argmax on the CPU: lowest index on ties); equal in fp32
  c_err32_loss / _dW / _db / _dfeats     relative (Frobenius) error of the reference's own fp32 run against its fp64 run
  c_gap                                  smallest top-2 gap of the fp64 score rows (the tied pair of the tie case counted once)
Seeds are searched until (a) every score row keeps a top-2 gap of MIN_GAP in fp64, so that argmax is not decided by rounding, and
(b) every recorded err32 is 0 with an exactly zero fp64 value (the all-state-0 case) or at least ERR_FLOOR = 2^-25.  The tests
hold an fp32 implementation to 10 x err32; a value correctly rounded to fp32 is already off by up to 2^-24 (2^-25.5 on average),
so a recorded error below 2^-25 would only say that the reference's roundings happened to cancel on that seed, not what fp32
arithmetic can do.
Metric sets `m` of METRIC_SETS: m_seed and m_value = the reference's accuracy / keyframe_distance (NaN without positives)."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HERE = os.path.dirname(os.path.abspath(__file__))

import cls_head_ref as CR  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    assert ref_import.available(), "needs the reference checkout"
    _, ml, _, _ = ref_import.load_reference()
    import model.metric as ref_metric
    ce = ml.CrossEntropy()

    def loss_of(scores, target, state):
        if state is None:
            return ce(scores, target)                                            # trainer/trainer_oscc.py:338
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                      # .T of a 1-D tensor, as the reference writes it
            return torch.mean(state.T * ce(scores.squeeze(dim=-1), target))      # trainer/trainer_pnr.py:350

    out = {}
    for name, (task, n, K, C, world, rank, kind) in CR.CASES.items():
        for seed in range(1, 400):
            inp = CR.make_inputs(name, seed)
            r32, r64 = CR.head(name, inp, torch.float32, loss_of), CR.head(name, inp, torch.float64, loss_of)
            gap = CR.min_gap(r64["scores"], (1, 2) if kind == "tie" else None)
            errs = {k: CR.rel(r32[k], r64[k]) for k in ("loss", "dW", "db", "dfeats")}
            zero = float(r64["loss"]) == 0.0
            ok = gap >= CR.MIN_GAP and torch.equal(r32["pred"], r64["pred"])
            ok = ok and all((e == 0.0 and zero) or e >= CR.ERR_FLOOR for e in errs.values())
            if ok:
                break
        else:
            raise RuntimeError(f"{name}: no seed found")
        print(f"{name}: seed {seed} loss32 {float(r32['loss']):.8f} loss64 {float(r64['loss']):.12f} gap {gap:.2e} err32 "
              + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        out[name + "_seed"] = np.int64(seed)
        out[name + "_loss32"] = np.float32(float(r32["loss"]))
        out[name + "_loss64"] = np.float64(float(r64["loss"]))
        out[name + "_gap"] = np.float64(gap)
        out[name + "_pred"] = r64["pred"].to(torch.int32).numpy()
        for k in ("dW", "db", "dfeats", "scores"):
            out[f"{name}_{k}64"] = r64[k].float().numpy()
        for k, v in errs.items():
            out[f"{name}_err32_{k}"] = np.float64(v)
    for name, (task, rows, C, fps, kind) in CR.METRIC_SETS.items():
        seed = 7
        m = CR.make_metric_inputs(name, seed)
        if task == "oscc":
            val = ref_metric.oscc_metrics(m["preds"], m["state"])["accuracy"]
        else:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                                  # np.mean([]) of the no-positive set
                val = ref_metric.pnr_metrics(m["preds"], m["labels"], m["state"], m["fps"], m["start"], m["end"], m["pnr"])["keyframe_distance"]
        print(f"{name}: {val!r}")
        out[name + "_seed"] = np.int64(seed)
        out[name + "_value"] = np.float64(val)
    path = os.path.join(HERE, "cls_head.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
