"""Retrieval scoring on the device (egv_rank_scores, egovlp_amd.model.metric mir_metrics / mir_scores / map / charades_metrics /
oscc_metrics, egovlp_amd.trainer.retrieval_eval.RetrievalEvaluator) against the goldens the reference produced and, at sizes
where no golden is stored, against tests/retrieval_ref.py (pinned to those goldens by tests/test_retrieval_metrics_cpu.py).

Bars (derived in tests/test_retrieval_metrics_cpu.py): 1e-8 on percent-scale scalars, 1e-10 on per-query values.  The raw IDCG
sums of the geometry sweep are not normalised and grow with the row length (hundreds for a dense row of 16 384), so they are
held to the same RELATIVE bar, 1e-10 * max(1, |value|); nDCG = DCG / IDCG and AP lie in [0, 1] and are held to 1e-10 absolute.

EPIC-sized end-to-end test, observed on an MI355X: see the docstring of test_epic_sized_end_to_end."""
import os

import numpy as np
import pytest
import torch

import retrieval_ref as RR

pytestmark = pytest.mark.gpu

SCALAR_BAR = 1e-8
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


def annotations(G, tag):
    from egovlp_amd.model.metric import RetrievalAnnotations
    p = f"mir_{tag}"
    return RetrievalAnnotations(G[p + "_video_id"], G[p + "_text_id"], relevancy(G, p))


def close(got, want, bar, what, relative=False):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions differ")
    ok = ~np.isnan(want)
    if not ok.any():
        return
    err = np.abs(got[ok] - want[ok]) / (np.maximum(1.0, np.abs(want[ok])) if relative else 1.0)
    print(what, "max err %.3e (bar %.0e)" % (err.max(), bar))
    assert err.max() <= bar, (what, err.max())


# ------------------------------------------------------------------------------------------------ goldens of the reference
@pytest.mark.parametrize("as_cuda", [True, False])
@pytest.mark.parametrize("tag", ["s", "m"])
def test_mir_metrics_golden(G, tag, as_cuda):
    from egovlp_amd.model.metric import mir_metrics
    p = f"mir_{tag}"
    sims, idx = G[p + "_sims"], G[p + "_idx_arr"]
    if as_cuda:
        sims, idx = torch.from_numpy(sims).cuda(), torch.from_numpy(idx).cuda()
    res, per = mir_metrics(sims, idx, annotations(G, tag), per_query=True)
    assert list(res) == MIR_KEYS
    for k in MIR_KEYS:
        close(np.float64(res[k]), G[f"{p}_{k}"], SCALAR_BAR, f"{p} {k}")
    for k in ("nDCG_V2T", "nDCG_T2V", "AP_V2T", "AP_T2V"):
        assert per[k].is_cuda
        close(per[k], G[f"{p}_q_{k}"], QUERY_BAR, f"{p} per query {k}")


def test_mir_scores_golden_prepared_matrix(G):
    """run/test_epic.py's path: the [sentences, videos] matrix prepared by the caller, its own (s + 1) / 2 applied."""
    from egovlp_amd.model.metric import mir_scores
    p = "mir_m"
    M = RR.transform(RR.prepare_mir(G[p + "_sims"], G[p + "_idx_arr"], G[p + "_video_id"], G[p + "_text_id"]), affine_half=True)
    res = mir_scores(torch.from_numpy(np.ascontiguousarray(M.T)).cuda(), annotations(G, "m"))
    for k in MIR_KEYS:
        close(np.float64(res[k]), G[f"{p}_{k}"], SCALAR_BAR, f"mir_scores {k}")


def test_ties_among_irrelevant_items_change_nothing(G):
    from egovlp_amd.retrieval_ops import rank_scores
    rel = torch.from_numpy(relevancy(G, "mirtie")).cuda()
    M = torch.from_numpy(G["mirtie_M"]).cuda()
    for transposed, d in ((False, "V2T"), (True, "T2V")):
        dcg, ap = rank_scores(M, rel, transposed=transposed)
        idcg, _ = rank_scores(None, rel, transposed=transposed)
        close(dcg / idcg, G[f"mirtie_q_nDCG_{d}"], QUERY_BAR, f"mirtie nDCG {d}")
        close(ap, G[f"mirtie_q_AP_{d}"], QUERY_BAR, f"mirtie AP {d}")


def charades_inputs(GC, tag):
    nv, nc = (int(x) for x in GC["charades_gt_shape"])
    gt = np.zeros(nv * nc)
    gt[GC[f"charades_{tag}_gt_index"]] = 1
    return GC["charades_sub"], gt.reshape(nv, nc)


@pytest.mark.parametrize("as_cuda", [True, False])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_charades_golden(GC, tag, as_cuda):
    from egovlp_amd.model.metric import charades_metrics, map as map_
    sub, gt = charades_inputs(GC, tag)
    if as_cuda:
        sub, gt = torch.from_numpy(sub).cuda(), torch.from_numpy(gt).cuda()
    res = charades_metrics(sub, gt)
    assert list(res) == ["mAP"]
    close(np.float64(res["mAP"]), GC[f"charades_{tag}_mAP"], QUERY_BAR, f"charades_{tag} mAP")          # a fraction, not x 100
    m_ap, w_ap, m_aps = map_(sub, gt)
    close(np.float64(m_ap), GC[f"charades_{tag}_map_m_ap"], QUERY_BAR, f"charades_{tag} map m_ap")
    close(m_aps, GC[f"charades_{tag}_map_m_aps"], QUERY_BAR, f"charades_{tag} map m_aps")
    close(w_ap, GC[f"charades_{tag}_map_w_ap"], QUERY_BAR, f"charades_{tag} map w_ap")
    assert int(np.isnan(m_aps).sum()) == (1 if tag == "b" else 0)


def test_oscc_golden(G):
    from egovlp_amd.model.metric import oscc_metrics
    got = oscc_metrics(torch.from_numpy(G["oscc_preds"]).cuda(), torch.from_numpy(G["oscc_labels"]).cuda())
    assert abs(got["accuracy"] - float(G["oscc_accuracy"])) <= SCALAR_BAR


# ------------------------------------------------------------------------------------------------ geometry sweep
def sweep_inputs(nq, L, dense, seed):
    """Tie-free by construction: the similarities are nq * L DISTINCT fp32 values (a permutation of a 2^-23 grid), so neither
    direction holds equal values.  The relevancies are fp32-representable, so the fp32 and the fp64 hand-over agree exactly."""
    rng = np.random.default_rng(seed)
    n = nq * L
    S = ((rng.permutation(n).astype(np.float64) - n // 2) / 2.0 ** 23).astype(np.float32).reshape(nq, L)
    assert np.unique(S).size == n
    if dense:
        R = rng.uniform(0.01, 1.0, size=(nq, L)).astype(np.float32)
        R[rng.random((nq, L)) < 0.1] = 1.0
    else:
        R = np.zeros((nq, L), dtype=np.float32)
        R[rng.random((nq, L)) < 0.02] = 1.0
        frac = rng.random((nq, L)) < 0.02
        R[frac] = (rng.integers(1, 8, size=(nq, L)) / 8.0).astype(np.float32)[frac]
        R[::3][R[::3] == 1.0] = 0.5                               # every third query has no relevancy == 1: AP is NaN
    return S, R


@pytest.mark.parametrize("nq", [1, 7, 300])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 1000, 4097, 16384])
def test_geometry_sweep(nq, L):
    from egovlp_amd.retrieval_ops import rank_scores
    for dense in (True, False):
        S, R = sweep_inputs(nq, L, dense, seed=1000 * nq + L + int(dense))
        dcg_ref, ap_ref = RR.rank_scores(S, R)
        idcg_ref, _ = RR.rank_scores(None, R)
        with np.errstate(invalid="ignore", divide="ignore"):
            ndcg_ref = dcg_ref / idcg_ref
        if not dense:
            assert np.isnan(ap_ref[::3]).all()
        for transposed in (False, True):
            # stored [nq, L] with the queries in the rows, or [L, nq] with the queries in the columns
            Sd = torch.from_numpy(np.ascontiguousarray(S.T) if transposed else S).cuda()
            for r64 in (False, True):
                Rh = R.astype(np.float64) if r64 else R
                Rd = torch.from_numpy(np.ascontiguousarray(Rh.T) if transposed else Rh).cuda()
                dcg, ap = rank_scores(Sd, Rd, transposed=transposed)
                idcg, _ = rank_scores(None, Rd, transposed=transposed, want_ap=False)
                what = f"nq={nq} L={L} dense={dense} transposed={transposed} r64={r64}"
                close(idcg, idcg_ref, QUERY_BAR, what + " IDCG", relative=True)
                close(dcg / idcg, ndcg_ref, QUERY_BAR, what + " nDCG")
                close(ap, ap_ref, QUERY_BAR, what + " AP")


def test_affine_half_ranks_the_transformed_values():
    """(s + 1) / 2 in fp32 merges neighbouring fp32 values: the ranking must be that of the transformed values (ties by index)."""
    from egovlp_amd.retrieval_ops import rank_scores
    rng = np.random.default_rng(7)
    base = rng.uniform(-0.9, 0.9, size=(5, 50)).astype(np.float32)
    S = np.repeat(base, 4, axis=1)
    S[:, 1::4] = np.nextafter(S[:, 1::4], np.float32(2))          # one ulp apart: equal after the transformation for most
    R = rng.uniform(0.1, 1.0, size=S.shape)
    R[rng.random(S.shape) < 0.2] = 1.0
    assert (RR.transform(S, True)[:, 1::4] == RR.transform(S, True)[:, 0::4]).any()
    dcg_ref, ap_ref = RR.rank_scores(S, R, affine_half=True)
    dcg, ap = rank_scores(torch.from_numpy(S).cuda(), torch.from_numpy(R).cuda(), affine_half=True)
    close(dcg, dcg_ref, QUERY_BAR, "affine DCG", relative=True)
    close(ap, ap_ref, QUERY_BAR, "affine AP")


def test_all_equal_row_is_ranked_by_column_index():
    from egovlp_amd.retrieval_ops import rank_scores
    rng = np.random.default_rng(3)
    L = 777
    R = rng.uniform(0.1, 1.0, size=(2, L))
    R[rng.random((2, L)) < 0.1] = 1.0
    S = np.full((2, L), 0.25, dtype=np.float32)
    S[1, ::2] = -0.0                                              # -0 and +0 are equal similarities
    S[1, 1::2] = 0.0
    pos = np.arange(L)
    for i in range(2):                                            # order = column index: the scores of R's own order
        K = (R[i] > 0).sum()
        want_dcg = (R[i] * (pos < K) / np.log2(pos + 2.0)).sum()
        hit = R[i] == 1
        want_ap = (np.where(hit, np.cumsum(R[i]), 0) / (pos + 1.0)).sum() / hit.sum()
        dcg, ap = rank_scores(torch.from_numpy(S[i:i + 1]).cuda(), torch.from_numpy(R[i:i + 1]).cuda())
        close(dcg, [want_dcg], QUERY_BAR, "all-equal DCG", relative=True)
        close(ap, [want_ap], QUERY_BAR, "all-equal AP")


def test_row_above_the_limit_is_refused_and_writes_nothing():
    from egovlp_amd import _lib, ops, retrieval_ops
    L = retrieval_ops.MAX_ROW + 1
    S = torch.rand(2, L, device="cuda")
    R = torch.rand(2, L, device="cuda")
    with pytest.raises(_lib.EgovlpHipError, match="invalid argument"):
        retrieval_ops.rank_scores(S, R)
    with pytest.raises(_lib.EgovlpHipError, match="invalid argument"):
        retrieval_ops.rank_scores(S.t().contiguous(), R.t().contiguous(), transposed=True)
    dcg = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    ap = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    rc = _lib.lib().egv_rank_scores(S.data_ptr(), L, 0, R.data_ptr(), 0, L, 2, L, 0, dcg.data_ptr(), ap.data_ptr(), None, ops._stream())
    torch.cuda.synchronize()
    assert rc == 1 and bool((dcg == -7.0).all()) and bool((ap == -7.0).all())
    dcg, ap = retrieval_ops.rank_scores(S[:, :retrieval_ops.MAX_ROW], R[:, :retrieval_ops.MAX_ROW])     # the limit itself is served (strided rows)
    assert bool(torch.isfinite(dcg).all())


# ------------------------------------------------------------------------------------------------ EPIC-sized, end to end
def test_epic_sized_end_to_end():
    """9 668 clips x 3 842 sentences (EPIC-Kitchens-100 test): embeddings from egovlp_amd.synth -> RetrievalEvaluator (sim_matrix
    and both scoring directions on the device) against tests/retrieval_ref.py on the SAME device-computed similarity matrix
    copied to the host, so last-bit differences of the similarity kernel do not enter.

    Ties: 9 668 fp32 cosines in one row collide (after (s + 1) / 2 the values near 0.5 sit on a 2^-24 grid), and a collision
    between items of different relevancy makes the order matter.  A host simulation with random 256-wide embeddings and ONE
    relevant sentence per clip gave such a conflict in 0.2 % of the V2T queries and 0.9 % of the T2V queries -- above the cap of
    0.1 % of the queries that may be left out.  So the inputs are perturbed, not the cap: the text embeddings whose similarities
    take part in a conflict are nudged (relative 1e-3, seeded) and the similarities recomputed, at most four times; what then remains
    is left out of the per-query comparison and must stay within the cap.
    Observed on an MI355X (V2T / T2V queries with a conflict): 128 / 297 as drawn (1.3 % / 7.7 %), 25 / 37 after one nudge,
    3 / 2 after two (0.03 % / 0.05 %), 0 / 0 after three: no query is left out; largest per-query error 8.3e-17."""
    from egovlp_amd.model.metric import RetrievalAnnotations
    from egovlp_amd.synth import synth_tensor
    from egovlp_amd.trainer.retrieval_eval import RetrievalEvaluator
    nv, ns, D = 9668, 3842, 256
    rng = np.random.default_rng(100)
    text = synth_tensor("retrieval.text_embed", (nv, D), seed=5)
    vid = synth_tensor("retrieval.video_embed", (nv, D), seed=6).cuda()
    idx = rng.permutation(nv)
    text_rows = np.sort(rng.permutation(nv)[:ns])                   # csv positions of the clips whose caption is a unique sentence
    rel = np.zeros((nv, ns))
    sentence_of = rng.integers(0, ns, size=nv)
    sentence_of[rng.permutation(nv)[:ns]] = np.arange(ns)
    rel[np.arange(nv), sentence_of] = 1.0
    frac = (rng.random((nv, ns)) < 0.002) & (rel == 0)
    rel[frac] = (rng.integers(1, 8, size=(nv, ns)) / 8.0)[frac]
    ann = RetrievalAnnotations(np.arange(nv), text_rows, rel)
    order = np.argsort(idx)                                         # order[i] = position of clip i in the loader's order
    ev = RetrievalEvaluator(["mir_metrics"], annotations=ann)

    def similarities(text_embed):
        ev.reset()
        for a in range(0, nv, 2048):                                # per-batch hand-over, as the validation loop does
            ev.update(text_embed[a:a + 2048].cuda(), vid[a:a + 2048], torch.from_numpy(idx[a:a + 2048]))
        sims = ev.similarity().cpu().numpy()
        return RR.prepare_mir_fast(sims, order, text_rows)

    def conflicts(Mh):
        return RR.tie_conflict_entries(Mh, rel), RR.tie_conflict_entries(np.ascontiguousarray(Mh.T), np.ascontiguousarray(rel.T))

    for attempt in range(5):
        M = similarities(text)
        Mh = RR.transform(M, affine_half=True)
        (vi, vj), (tj, ti) = conflicts(Mh)
        bad_v, bad_t = np.unique(vi), np.unique(tj)
        print(f"attempt {attempt}: tie conflicts in {bad_v.size} of {nv} V2T queries, {bad_t.size} of {ns} T2V queries")
        if (bad_v.size == 0 and bad_t.size == 0) or attempt == 4:
            break
        # column t of M is the row order[text_rows[t]] of the loader-order similarity matrix: nudge those text embeddings
        rows = np.unique(order[text_rows[np.concatenate([vj, tj])]])
        g = torch.Generator().manual_seed(attempt)
        text = text.clone()
        rows = torch.from_numpy(rows)
        text[rows] += 1e-3 * text[rows].norm(dim=1, keepdim=True) * torch.randn(rows.numel(), D, generator=g) / D ** 0.5
    assert bad_v.size <= 0.001 * nv and bad_t.size <= 0.001 * ns, "more than 0.1 % of the queries hold a tie between different relevancies"

    out = ev.compute()[0]["mir_metrics"]                            # the batches of the last similarities() call
    assert list(out) == MIR_KEYS
    ev.reset()
    for a in range(0, nv, 2048):
        ev.update(text[a:a + 2048].cuda(), vid[a:a + 2048], torch.from_numpy(idx[a:a + 2048]))
    from egovlp_amd.model.metric import mir_metrics
    sims_dev = ev.similarity()
    assert sims_dev.is_cuda and np.array_equal(RR.prepare_mir_fast(sims_dev.cpu().numpy(), order, text_rows), M)   # deterministic kernel
    res, per = mir_metrics(sims_dev, torch.from_numpy(idx).cuda(), ann, per_query=True)
    assert res == out
    scal, per_ref = RR.mir(M, rel, affine_half=True)
    keep = {"V2T": np.setdiff1d(np.arange(nv), bad_v), "T2V": np.setdiff1d(np.arange(ns), bad_t)}
    for k in ("nDCG_V2T", "nDCG_T2V", "AP_V2T", "AP_T2V"):
        kk = keep[k[-3:]]
        close(per[k].cpu().numpy()[kk], per_ref[k][kk], QUERY_BAR, f"EPIC-sized per query {k}")
    if bad_v.size == 0 and bad_t.size == 0:
        for k in MIR_KEYS:
            close(np.float64(res[k]), np.float64(scal[k]), SCALAR_BAR, f"EPIC-sized {k}")
    else:                                                            # the means over the queries that were compared
        for k in ("nDCG_V2T", "nDCG_T2V", "AP_V2T", "AP_T2V"):
            kk = keep[k[-3:]]
            close(np.float64(100 * per[k].cpu().numpy()[kk].mean()), np.float64(100 * per_ref[k][kk].mean()), SCALAR_BAR, f"EPIC-sized mean {k}")
