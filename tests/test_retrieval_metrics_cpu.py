"""CPU tests of the retrieval metrics (no GPU):

1. tests/retrieval_ref.py -- the numpy statement of DCG / AP with the index tie rule -- against every golden the reference
   produced (tests/golden/make_golden_retrieval.py).  Bars: 1e-8 on the percent-scale scalars, 1e-10 on per-query values.
   Derivation: every term carries a few ulps of fp64 (2.2e-16), a row sums at most 16 384 positive terms, so the relative error
   of a sum stays below 4e-12, 4e-10 after the x 100; the bars are 25 times that.  This shows nothing about the device path; it
   makes the helper a trustworthy stand-in at sizes where no golden is stored.
2. The public surface through the mock C ABI (tests/mock_hip.py): mir_metrics / mir_scores / charades_metrics / map and the
   RetrievalEvaluator run on CPU tensors, return the reference's keys, make exactly the expected C-ABI calls and cache the IDCG."""
import os

import numpy as np
import pytest
import torch

import retrieval_ref as RR
from mock_hip import mock_hip

SCALAR_BAR = 1e-8      # percent scale
QUERY_BAR = 1e-10
MIR_KEYS = ["nDCG_V2T", "nDCG_T2V", "nDCG_AVG", "mAP_V2T", "mAP_T2V", "mAP_AVG"]


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "retrieval_metrics.npz"))


@pytest.fixture(scope="module")
def GC(golden_dir):
    return np.load(os.path.join(golden_dir, "retrieval_metrics_charades.npz"))


def relevancy(G, prefix):
    return RR.sparse_to_dense(G[prefix + "_rel_shape"], G[prefix + "_rel_index"], G[prefix + "_rel_value"])


def check_queries(per, G, prefix):
    for k in ("nDCG_V2T", "nDCG_T2V", "AP_V2T", "AP_T2V"):
        want = G[f"{prefix}_q_{k}"]
        err = np.abs(per[k] - want).max()
        print(prefix, k, "max abs err per query %.3e" % err)
        assert per[k].shape == want.shape and err <= QUERY_BAR, (prefix, k, err)


@pytest.mark.parametrize("tag", ["s", "m"])
def test_ref_helper_matches_reference_mir(G, tag):
    p = f"mir_{tag}"
    rel = relevancy(G, p)
    M = RR.prepare_mir(G[p + "_sims"], G[p + "_idx_arr"], G[p + "_video_id"], G[p + "_text_id"])
    assert M.shape == rel.shape
    Mh = RR.transform(M, affine_half=True)
    assert not RR.tie_conflicts(Mh, rel).any() and not RR.tie_conflicts(Mh.T, rel.T).any()      # the fixtures' condition on ties
    scal, per = RR.mir(M, rel, affine_half=True)
    for k in MIR_KEYS:
        err = abs(scal[k] - float(G[f"{p}_{k}"]))
        print(p, k, scal[k], "err %.3e" % err)
        assert err <= SCALAR_BAR, (k, err)
    check_queries(per, G, p)


def test_ref_helper_ties_among_irrelevant_items_change_nothing(G):
    rel = relevancy(G, "mirtie")
    M = G["mirtie_M"]
    srt = np.sort(M, axis=1)
    assert (srt[:, 1:] == srt[:, :-1]).any(axis=1).all()                                      # ties in every row ...
    assert not RR.tie_conflicts(M, rel).any() and not RR.tie_conflicts(M.T, rel.T).any()      # ... none between different relevancies
    _, per = RR.mir(M, rel)
    check_queries(per, G, "mirtie")


def charades_inputs(GC, tag):
    nv, nc = (int(x) for x in GC["charades_gt_shape"])
    gt = np.zeros(nv * nc)
    gt[GC[f"charades_{tag}_gt_index"]] = 1
    return GC["charades_sub"], gt.reshape(nv, nc)


def charades_ref(sub, gt):
    aps = RR.rank_scores(np.ascontiguousarray(sub.T), np.ascontiguousarray(gt.T))[1]
    return aps.mean(), aps * gt.sum(axis=0) / gt.sum(), aps


@pytest.mark.parametrize("tag", ["a", "b"])
def test_ref_helper_matches_reference_charades(GC, tag):
    sub, gt = charades_inputs(GC, tag)
    m_ap, w_ap, aps = charades_ref(sub, gt)
    want = GC[f"charades_{tag}_map_m_aps"]
    assert np.array_equal(np.isnan(aps), np.isnan(want)) and int(np.isnan(want).sum()) == (1 if tag == "b" else 0)
    ok = ~np.isnan(want)
    assert np.abs(aps[ok] - want[ok]).max() <= QUERY_BAR
    assert np.abs(w_ap[ok] - GC[f"charades_{tag}_map_w_ap"][ok]).max() <= QUERY_BAR
    fix = np.where((gt.sum(axis=1) == 0)[:, None], -np.inf, sub).astype(np.float32)
    got, want_fix, want_raw = charades_ref(fix, gt)[0], float(GC[f"charades_{tag}_mAP"]), float(GC[f"charades_{tag}_map_m_ap"])
    if tag == "b":
        assert np.isnan(got) and np.isnan(want_fix) and np.isnan(m_ap) and np.isnan(want_raw)
    else:
        assert abs(got - want_fix) <= QUERY_BAR and abs(m_ap - want_raw) <= QUERY_BAR


def test_oscc_metrics_matches_reference(G):
    from egovlp_amd.model.metric import oscc_metrics
    got = oscc_metrics(torch.from_numpy(G["oscc_preds"]), torch.from_numpy(G["oscc_labels"]))
    assert list(got) == ["accuracy"] and abs(got["accuracy"] - float(G["oscc_accuracy"])) <= SCALAR_BAR


# ------------------------------------------------------------------------------------------------ through the mock C ABI
def annotations(G, tag="s"):
    from egovlp_amd.model.metric import RetrievalAnnotations
    p = f"mir_{tag}"
    return RetrievalAnnotations(G[p + "_video_id"], G[p + "_text_id"], relevancy(G, p))


def test_config_metric_names_resolve():
    """The reference's run scripts do `getattr(module_metric, met)` for the names in configs/{ft,eval}/{epic,charades}.json."""
    import egovlp_amd.model.metric as module_metric
    for name in ("mir_metrics", "charades_metrics", "oscc_metrics"):
        assert callable(getattr(module_metric, name))
        assert getattr(module_metric, name).__name__ == name


def test_mir_metrics_calls_and_idcg_cache(G):
    from egovlp_amd.model.metric import mir_metrics, mir_scores
    ann = annotations(G)
    sims, idx = G["mir_s_sims"], G["mir_s_idx_arr"]
    with mock_hip() as calls:
        res = mir_metrics(sims, idx, ann)
        assert list(res) == MIR_KEYS and all(isinstance(v, float) for v in res.values())
        # IDCG of both directions + the two scored directions; each column-direction call asks for its workspace size first
        assert calls == ["egv_rank_scores", "egv_rank_scores_work_bytes", "egv_rank_scores"] * 2
        del calls[:]
        res = mir_metrics(torch.from_numpy(sims), torch.from_numpy(idx), ann)               # second call: no IDCG launch
        assert list(res) == MIR_KEYS
        assert calls == ["egv_rank_scores", "egv_rank_scores_work_bytes", "egv_rank_scores"]
        del calls[:]
        res, per = mir_scores(torch.rand(40, 96), ann, per_query=True)                      # [sentences, videos], cache shared
        assert list(res) == MIR_KEYS and per["AP_V2T"].shape == (96,) and per["nDCG_T2V"].shape == (40,)
        assert calls == ["egv_rank_scores_work_bytes", "egv_rank_scores", "egv_rank_scores"]
        del calls[:]
        mir_metrics(sims, idx, annotations(G))                                              # another annotations object: its own IDCG
        assert calls.count("egv_rank_scores") == 4


def test_mir_metrics_rejects_incomplete_idx(G):
    from egovlp_amd.model.metric import mir_metrics
    idx = G["mir_s_idx_arr"].copy()
    idx[0] = idx[1]
    with mock_hip():
        with pytest.raises(ValueError):
            mir_metrics(G["mir_s_sims"], idx, annotations(G))


def test_mir_metrics_default_annotations_from_the_reference_paths(G, tmp_path, monkeypatch):
    """The two-argument call of trainer_epic.py:240 reads the csv files and the pickle from the reference's hard-coded paths."""
    import pickle
    import egovlp_amd.model.metric as module_metric
    d = tmp_path / module_metric.EPIC_RETRIEVAL_DIR
    (d / "relevancy").mkdir(parents=True)
    (d / "EPIC_100_retrieval_test.csv").write_text("narration_id,narration\n" + "".join("%d,x\n" % v for v in G["mir_s_video_id"]))
    (d / "EPIC_100_retrieval_test_sentence.csv").write_text("narration_id,narration\n" + "".join("%d,x\n" % v for v in G["mir_s_text_id"]))
    with open(d / "relevancy" / "caption_relevancy_EPIC_100_retrieval_test.pkl", "wb") as f:
        pickle.dump(relevancy(G, "mir_s"), f)
    monkeypatch.chdir(tmp_path)
    with mock_hip() as calls:
        res = module_metric.mir_metrics(G["mir_s_sims"], G["mir_s_idx_arr"])
        assert list(res) == MIR_KEYS and calls.count("egv_rank_scores") == 4
        ann = module_metric._default_annotations()
        assert [str(v) for v in G["mir_s_video_id"]] == list(ann.video_id) and ann.relevancy.shape == (96, 40)


def test_charades_metrics_and_map_calls(GC):
    from egovlp_amd.model.metric import charades_metrics, map as map_
    sub, gt = charades_inputs(GC, "a")
    with mock_hip() as calls:
        res = charades_metrics(sub, gt)
        assert list(res) == ["mAP"] and isinstance(res["mAP"], float)
        assert calls == ["egv_rank_scores_work_bytes", "egv_rank_scores"]
        del calls[:]
        m_ap, w_ap, m_aps = map_(torch.from_numpy(sub), torch.from_numpy(gt))
        assert isinstance(m_ap, float) and w_ap.shape == (157,) and m_aps.shape == (157,) and m_aps.dtype == np.float64
        assert calls == ["egv_rank_scores_work_bytes", "egv_rank_scores"]


def test_rank_scores_argument_checks():
    from egovlp_amd.retrieval_ops import rank_scores
    with mock_hip():
        with pytest.raises(ValueError):
            rank_scores(torch.rand(3, 4), torch.rand(3, 5))
        with pytest.raises(ValueError):
            rank_scores(torch.rand(3, 4), torch.rand(3, 4).half())
        with pytest.raises(ValueError):
            rank_scores(torch.rand(3, 4), torch.rand(3, 4), want_dcg=False, want_ap=False)
        dcg, ap = rank_scores(torch.rand(3, 4), torch.rand(3, 4).double(), transposed=True)
        assert dcg.shape == (4,) and ap.shape == (4,) and dcg.dtype == torch.float64
        dcg, ap = rank_scores(None, torch.rand(3, 4), want_ap=False)
        assert dcg.shape == (3,) and ap is None


def test_rank_scores_has_no_cpu_path():
    from egovlp_amd._lib import EgovlpHipError
    from egovlp_amd.retrieval_ops import rank_scores
    with pytest.raises(EgovlpHipError):
        rank_scores(torch.rand(3, 4), torch.rand(3, 4))


def test_retrieval_evaluator_call_census(G):
    """Per-batch embeddings in, nested metrics out: one similarity launch, the rank-score calls, nothing else."""
    from egovlp_amd.trainer.retrieval_eval import RetrievalEvaluator
    ann = annotations(G)
    ev = RetrievalEvaluator(["mir_metrics"], annotations=ann)
    idx = torch.from_numpy(G["mir_s_idx_arr"])
    with mock_hip() as calls:
        for a in range(0, 96, 32):
            ev.update(torch.rand(32, 16), torch.rand(32, 16), idx[a:a + 32])
        out = ev.compute()
        assert list(out) == [0] and list(out[0]) == ["mir_metrics"] and list(out[0]["mir_metrics"]) == MIR_KEYS
        assert calls == ["egv_sim_matrix_fwd"] + ["egv_rank_scores", "egv_rank_scores_work_bytes", "egv_rank_scores"] * 2
        del calls[:]
        ev.update(torch.rand(96, 16), torch.rand(96, 16), idx)                               # next epoch: the IDCG is kept
        ev.compute()
        assert calls == ["egv_sim_matrix_fwd", "egv_rank_scores", "egv_rank_scores_work_bytes", "egv_rank_scores"]
    assert ev.compute() == {0: {}}
