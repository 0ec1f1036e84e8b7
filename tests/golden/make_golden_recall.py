"""Generate the Recall@K goldens by RUNNING THE REFERENCE ITSELF (model/metric.py t2v_metrics :20-124, v2t_metrics :127-216).
Run once where the reference is available:
    python tests/golden/make_golden_recall.py
Writes tests/golden/recall_ranks.npz.

The reference calls `cols2metrics(cols, num_queries)` (:124, :216) and defines it nowhere, so the two functions cannot finish
as they stand.  Here `cols2metrics` is set in the namespace of the reference's module, at run time, to a recorder that returns
its arguments: what is stored is exactly what the reference computed, the rank vector and the number of queries.  Every call
gets copies of its inputs: the reference's v2t writes MISSING_VAL into the matrix it is handed (:167).

Cases (<tag>_sims fp32 [Nq, Nv], <tag>_mask uint8 [Nq] where the case has one, <tag>_t2v_cols / _t2v_n / _v2t_cols / _v2t_n):
  rand     40 x 40 random fp32
  first    195 x 65 (qpv 3), the mask keeps every video's first caption and a random half of the others
  novid    195 x 65, one video fully masked (its v2t rank is +inf)
  ties     96 x 32 integer-valued in [-3, 3]: massive ties
  const    60 x 20, a constant matrix, with a mask"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle import ref_import  # noqa: E402


def main():
    ref_import.load_reference()                                   # stubs what the reference imports and is not installed
    import model.metric as metric_mod
    if not hasattr(np, "bool"):
        np.bool = np.bool_                                        # the alias the reference uses (:112)
    metric_mod.cols2metrics = lambda cols, num_queries: (np.array(cols, dtype=np.float64), int(num_queries))
    rng = np.random.default_rng(20241019)

    def first_mask(nq, qpv):
        m = (rng.random(nq) < 0.5).astype(np.uint8)
        m[::qpv] = 1
        return m

    novid = np.ones(195, dtype=np.uint8)
    novid[3 * 17:3 * 18] = 0
    novid[[4, 100]] = 0
    cases = {
        "rand": (rng.standard_normal((40, 40)).astype(np.float32), None),
        "first": (rng.standard_normal((195, 65)).astype(np.float32), first_mask(195, 3)),
        "novid": (rng.standard_normal((195, 65)).astype(np.float32), novid),
        "ties": (rng.integers(-3, 4, size=(96, 32)).astype(np.float32), None),
        "const": (np.full((60, 20), 0.25, dtype=np.float32), first_mask(60, 3)),
    }
    out = {}
    for tag, (sims, mask) in cases.items():
        out[tag + "_sims"] = sims
        if mask is not None:
            out[tag + "_mask"] = mask
        for name, fn in (("t2v", metric_mod.t2v_metrics), ("v2t", metric_mod.v2t_metrics)):
            cols, n = fn(sims.copy(), None if mask is None else mask.copy())
            out[f"{tag}_{name}_cols"], out[f"{tag}_{name}_n"] = cols, np.int64(n)
            print(tag, name, "n =", n, "ranks", cols[:6], "inf:", int(np.isinf(cols).sum()))
    path = os.path.join(HERE, "recall_ranks.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
