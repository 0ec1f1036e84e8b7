"""CPU tests of Recall@K (no GPU):

1. tests/recall_ref.py -- the count form of the reference's ranks -- equals, exactly, the rank vectors the reference's own
   t2v_metrics / v2t_metrics produced (tests/golden/make_golden_recall.py).  This shows nothing about the device path; it makes
   the helper a trustworthy stand-in at sizes where no golden is stored.
2. cols2metrics (the product's, on host tensors) on hand-made vectors: the median of an even and an odd count, half-integer
   ranks, an inf, a zero recall.
3. The chunk plan of RecallEvaluator covers every row exactly once.
4. The ValueErrors that need no device, and the public surface through the mock C ABI (tests/mock_hip.py): keys and C-ABI calls."""
import os

import numpy as np
import pytest
import torch

import recall_ref as RF
from mock_hip import mock_hip

CASES = ["rand", "first", "novid", "ties", "const"]
KEYS = ["R1", "R5", "R10", "R50", "MedR", "MeanR", "geometric_mean_R1-R5-R10"]


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "recall_ranks.npz"))


def mask_of(G, tag):
    return G[tag + "_mask"] if tag + "_mask" in G.files else None


# ------------------------------------------------------------------------------------------------ 1. the helper against the reference
@pytest.mark.parametrize("tag", CASES)
def test_count_form_equals_the_reference_ranks(G, tag):
    sims, mask = G[tag + "_sims"], mask_of(G, tag)
    _, cols = RF.t2v_metrics(sims, mask)
    assert np.array_equal(cols, G[tag + "_t2v_cols"])
    assert cols.size == int(G[tag + "_t2v_n"]) == (sims.shape[0] if mask is None else int(mask.sum()))
    _, cols = RF.v2t_metrics(sims, mask)
    assert np.array_equal(cols, G[tag + "_v2t_cols"])             # inf == inf
    assert int(G[tag + "_v2t_n"]) == sims.shape[1]


def test_goldens_hold_the_cases_they_are_meant_to(G):
    assert np.isinf(G["novid_v2t_cols"]).sum() == 1 and np.isinf(G["novid_v2t_cols"][17])
    assert (G["ties_v2t_cols"] % 1 == 0.5).any()                  # averaged ties: half-integer ranks
    assert (G["const_t2v_cols"] == 0).all()
    assert (G["const_v2t_cols"] == (int(G["const_mask"].sum()) - 1) / 2).all()
    assert (G["first_mask"].reshape(-1, 3)[:, 0] == 1).all() and G["first_mask"].sum() < 195


# ------------------------------------------------------------------------------------------------ 2. cols2metrics
def check_cols2metrics(cols, n):
    from egovlp_amd.model.metric import cols2metrics
    want = RF.cols2metrics(np.asarray(cols, dtype=np.float64), n)
    for given in (np.asarray(cols, dtype=np.float64), torch.tensor(cols, dtype=torch.float64)):
        got = cols2metrics(given, n)
        assert list(got) == KEYS
        for k in KEYS:
            assert isinstance(got[k], float)
            assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])
    return got


def test_cols2metrics_hand_made():
    m = check_cols2metrics([0, 3, 7, 60], 4)                      # even count: the mean of the two middle values
    assert m == {"R1": 25.0, "R5": 50.0, "R10": 75.0, "R50": 75.0, "MedR": 6.0, "MeanR": 18.5,
                 "geometric_mean_R1-R5-R10": float(np.exp(np.mean(np.log([25.0, 50.0, 75.0]))))}
    m = check_cols2metrics([4, 0, 12], 3)                         # odd count
    assert m["MedR"] == 5.0 and m["R1"] == 100 / 3 and m["R5"] == 200 / 3
    m = check_cols2metrics([0.5, 1.5, 0, 9.5, 4.5, 49.5], 6)      # half-integer ranks (averaged ties)
    assert m["MedR"] == 4.0 and m["R1"] == 100 / 6 and m["R5"] == 400 / 6 and m["R10"] == 500 / 6 and m["R50"] == 100.0
    m = check_cols2metrics([0, 2, float("inf")], 3)               # a video without a caption
    assert m["MedR"] == 3.0 and m["MeanR"] == float("inf") and m["R50"] == 200 / 3
    m = check_cols2metrics([0, float("inf"), float("inf"), 1], 4)
    assert m["MedR"] == float("inf")
    m = check_cols2metrics([3, 4, 20], 3)                         # R1 = 0: the geometric mean is 0
    assert m["R1"] == 0.0 and m["geometric_mean_R1-R5-R10"] == 0.0
    m = check_cols2metrics([0, 1, 2], 5)                          # num_queries is the caller's number, not the vector's length
    assert m["R1"] == 20.0 and m["R5"] == 60.0


@pytest.mark.parametrize("tag", CASES)
def test_cols2metrics_on_the_golden_ranks(G, tag):
    for d in ("t2v", "v2t"):
        check_cols2metrics(G[f"{tag}_{d}_cols"].tolist(), int(G[f"{tag}_{d}_n"]))


def test_masked_summary_equals_the_compacted_one():
    """t2v's query mask is applied inside the summary without compacting the vector on the device."""
    from egovlp_amd.model.metric import _recall_summary
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 40):
        cols = rng.integers(0, 60, size=n).astype(np.float64)
        keep = rng.random(n) < 0.6
        keep[0] = True
        got = _recall_summary(torch.from_numpy(cols), torch.from_numpy(keep).sum(), keep=torch.from_numpy(keep))
        assert got == RF.cols2metrics(cols[keep], int(keep.sum()))


# ------------------------------------------------------------------------------------------------ 3. the chunk plan
def test_chunk_plan_covers_every_row_once():
    from egovlp_amd.trainer.retrieval_eval import chunk_plan
    n_rows, n_cols = 37, 50
    row = 4 * n_cols
    for chunk_bytes, per in ((1, 1), (row - 1, 1), (row, 1), (row + 1, 1), (2 * row, 2), (7 * row + 3, 7), (36 * row, 36),
                             (37 * row - 1, 36), (37 * row, 37), (1 << 40, 37)):
        plan = chunk_plan(n_rows, n_cols, chunk_bytes)
        assert plan[0] == 0 and plan[-1] == n_rows and all(a < b for a, b in zip(plan[:-1], plan[1:]))
        sizes = [b - a for a, b in zip(plan[:-1], plan[1:])]
        assert sum(sizes) == n_rows and max(sizes) == per and all(s == per for s in sizes[:-1])
        assert per == 1 or per * row <= chunk_bytes               # a chunk never exceeds the budget, except the one-row minimum
    assert chunk_plan(1, 1, 1) == [0, 1]
    assert chunk_plan(5, 3, 24) == [0, 2, 4, 5]
    with pytest.raises(ValueError):
        chunk_plan(0, 3, 24)


# ------------------------------------------------------------------------------------------------ 4. errors and the public surface
def test_value_errors_that_need_no_device():
    from egovlp_amd import retrieval_ops as RO
    from egovlp_amd.model.metric import t2v_metrics, v2t_metrics
    from egovlp_amd.trainer.retrieval_eval import RecallEvaluator
    s = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="64"):
        RO.topk_rows(s, 65)
    with pytest.raises(ValueError, match="64"):
        RO.topk_rows(s, 0)
    with pytest.raises(ValueError, match="empty"):
        RO.topk_rows(torch.zeros(0, 3), 1)
    with pytest.raises(ValueError, match="empty"):
        RO.gt_ranks(torch.zeros(3, 0), 1, "t2v")
    with pytest.raises(ValueError, match="multiple of Nv"):
        RO.gt_ranks(torch.zeros(7, 3), 2, "t2v")                  # 7 captions > 2 * 3
    with pytest.raises(ValueError, match="multiple of Nv"):
        RO.gt_ranks(torch.zeros(7, 3), 2, "v2t")
    with pytest.raises(ValueError, match="multiple of Nv"):
        RO.gt_ranks(torch.zeros(3, 7), 2, "v2t", transposed=False)
    with pytest.raises(ValueError, match="6 are needed"):
        RO.gt_ranks(s, 2, "v2t", query_masks=torch.ones(5))
    with pytest.raises(ValueError, match="6 are needed"):
        RO.gt_ranks(s, 2, "t2v", query_masks=torch.ones(7))
    with pytest.raises(ValueError, match="3 are needed"):
        RO.topk_rows(s, 2, col_valid=torch.ones(6))
    with pytest.raises(ValueError, match="direction"):
        RO.gt_ranks(s, 2, "t2t")
    with pytest.raises(ValueError):
        RO.row_normalize(torch.zeros(0, 4))
    for fn in (t2v_metrics, v2t_metrics):
        with pytest.raises(ValueError, match="multiple of Nv"):
            fn(np.zeros((7, 3), dtype=np.float32))
        with pytest.raises(ValueError, match="mask"):
            fn(np.zeros((6, 3), dtype=np.float32), np.ones(5))
        with pytest.raises(ValueError, match="empty"):
            fn(np.zeros((0, 3), dtype=np.float32))
    ev = RecallEvaluator(queries_per_video=2)
    with pytest.raises(ValueError, match="Nq"):
        ev.update(torch.zeros(5, 8), torch.zeros(3, 8))
    with pytest.raises(ValueError, match="mask"):
        ev.update(torch.zeros(6, 8), torch.zeros(3, 8), query_mask=torch.ones(5))
    with pytest.raises(ValueError, match="64"):
        ev.topk(65)


def test_no_cpu_path():
    from egovlp_amd import _lib, retrieval_ops as RO
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    for call in (lambda: RO.gt_ranks(torch.zeros(4, 4), 1, "t2v"), lambda: RO.topk_rows(torch.zeros(4, 4), 2),
                 lambda: RO.row_normalize(torch.zeros(4, 4))):
        with pytest.raises(_lib.EgovlpHipError):
            call()


def test_public_surface_through_the_mock_abi():
    from egovlp_amd.model import metric as M
    from egovlp_amd.trainer.retrieval_eval import RecallEvaluator, chunk_plan
    sims = np.zeros((6, 3), dtype=np.float32)
    with mock_hip() as calls:
        for fn in (M.t2v_metrics, M.v2t_metrics):
            res, per = fn(sims, np.array([1, 1, 0, 1, 1, 1]), per_query=True)
            assert list(res) == KEYS and per.dtype == torch.float64
        assert calls == ["egv_gt_ranks", "egv_gt_ranks_work_bytes", "egv_gt_ranks"]
        del calls[:]
        ev = RecallEvaluator(queries_per_video=2, chunk_bytes=4 * 7 * 2, n_loaders=2)     # two rows of seven videos per chunk
        ev.update(torch.zeros(8, 32), torch.zeros(4, 32), dl_idx=1)
        ev.update(torch.zeros(6, 32), torch.zeros(3, 32), query_mask=torch.tensor([1, 0, 1, 1, 1, 1]), dl_idx=1)
        out = ev.compute()
        assert out[0] == {} and list(out[1]) == ["t2v_metrics", "v2t_metrics"] and list(out[1]["t2v_metrics"]) == KEYS
        n_t2v, n_v2t = len(chunk_plan(14, 7, 56)) - 1, len(chunk_plan(7, 14, 56)) - 1
        assert (n_t2v, n_v2t) == (7, 7)
        assert calls.count("egv_row_normalize") == 2 and calls.count("egv_gt_ranks") == n_t2v + n_v2t
        assert calls.count("egv_gemm_nt") == n_t2v + n_v2t and "egv_sim_matrix_fwd" not in calls
        assert ev._text == [[], []]                               # compute() forgets the batches
