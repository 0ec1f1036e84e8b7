"""Recall@K on the device (egv_gt_ranks, egv_topk_rows, egv_row_normalize; egovlp_amd.model.metric t2v_metrics / v2t_metrics /
cols2metrics; egovlp_amd.trainer.retrieval_eval.RecallEvaluator) against the rank vectors the reference produced
(tests/golden/recall_ranks.npz) and, at sizes where no golden is stored, against tests/recall_ref.py (pinned to those goldens by
tests/test_recall_cpu.py).

Ranks and top-k lists are compared EXACTLY: they are counts and selections of fp32 comparisons.  The only tolerances:
  * MedR / MeanR of the metric dicts: 1e-12 (sums of integers and half-integers, exact in fp64 in any order; the bar is slack).
  * the normalised evaluator: an interval from fp64 scores, derived at test_evaluator_normalised.
  * row_normalize: derived at test_row_normalize.

Step widths of the kernels (csrc/recall.hip), each tested one below, at and one above:"""
import os

import numpy as np
import pytest
import torch

import recall_ref as RF

pytestmark = pytest.mark.gpu

WAVE = 64                    # lanes of a wave
WORKGROUP = 256              # RC_THREADS; also TK_SAMPLE, the columns behind the head (0..3) that set the top-k kernel's first bar
VECTOR = 4                   # RC_VEC: floats of a 16-byte load
TRIP = 1024                  # RC_TRIP: one 16-byte load per thread
TOPK_TILE = 2048             # TK_TILE: columns between two looks at the candidate count
RANK_TILE = 4096             # RC_TILE: one trip of the rank kernel's unrolled loop; also TK_CAP, the candidate buffer
LENGTHS = sorted({1, 63, 64, 65, 255, 256, 257, 258, 259, 260, 1025} |
                 {w + d for w in (WAVE, WORKGROUP, VECTOR, TRIP, TOPK_TILE, RANK_TILE) for d in (-1, 0, 1)})
CASES = ["rand", "first", "novid", "ties", "const"]
RECALLS = ["R1", "R5", "R10", "R50", "geometric_mean_R1-R5-R10"]


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "recall_ranks.npz"))


def mask_of(G, tag):
    return G[tag + "_mask"] if tag + "_mask" in G.files else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def same(got, want, what):
    got = host(got) if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, np.flatnonzero((got != want).reshape(-1))[:8])


def int_matrix(rng, rows, cols, span=4):
    return rng.integers(-span, span + 1, size=(rows, cols)).astype(np.float32)


def layouts(M):
    """The matrix as a dense device tensor and as a column-sliced view of a wider one with an odd leading dimension, so that its
    rows start at every alignment and 16-byte loads cannot be assumed."""
    rows, cols = M.shape
    ld = cols + 5 - (cols % 2)                                   # odd, > cols
    big = torch.full((rows, ld), 99.0, device="cuda")            # what lies beside the view would win every comparison
    big[:, 1:1 + cols] = dev(M)
    view = big[:, 1:1 + cols]
    assert view.stride(0) % 2 == 1 and view.stride(0) > cols
    return [("dense", dev(M)), ("view", view)]


# ------------------------------------------------------------------------------------------------ goldens of the reference
@pytest.mark.parametrize("as_cuda", [True, False])
@pytest.mark.parametrize("tag", CASES)
def test_metrics_golden(G, tag, as_cuda):
    from egovlp_amd.model.metric import t2v_metrics, v2t_metrics
    sims, mask = G[tag + "_sims"], mask_of(G, tag)
    a, m = (dev(sims), None if mask is None else dev(mask)) if as_cuda else (sims.copy(), mask)
    for name, fn in (("t2v", t2v_metrics), ("v2t", v2t_metrics)):
        res, per = fn(a, m, per_query=True)
        want_cols, n = G[f"{tag}_{name}_cols"], int(G[f"{tag}_{name}_n"])
        assert per.is_cuda
        same(per, want_cols, f"{tag} {name} ranks")
        want = RF.cols2metrics(want_cols, n)
        assert list(res) == list(want)
        for k in RECALLS:
            assert res[k] == want[k], (tag, name, k, res[k], want[k])
        for k in ("MedR", "MeanR"):
            assert res[k] == want[k] or abs(res[k] - want[k]) <= 1e-12, (tag, name, k, res[k], want[k])
        assert fn(a, m) == res                                   # without per_query: the dict alone
    if not as_cuda:
        assert np.array_equal(sims, G[tag + "_sims"])            # the caller's matrix is not written to


@pytest.mark.parametrize("tag", CASES)
def test_v2t_transposed_and_row_form_golden(G, tag):
    from egovlp_amd.retrieval_ops import gt_ranks
    sims, mask = G[tag + "_sims"], mask_of(G, tag)
    qpv = sims.shape[0] // sims.shape[1]
    m = None if mask is None else dev(mask)
    same(gt_ranks(dev(sims), qpv, "v2t", query_masks=m), G[tag + "_v2t_cols"], "transposed")
    same(gt_ranks(dev(sims.T), qpv, "v2t", query_masks=m, transposed=False), G[tag + "_v2t_cols"], "row form")
    same(gt_ranks(dev(sims), qpv, "t2v", query_masks=m), RF.t2v_ranks(sims), "t2v unfiltered")


def test_cols2metrics_on_the_device():
    from egovlp_amd.model.metric import cols2metrics
    cols = np.array([0, 0.5, 3, 7.5, 60, np.inf, 2, 11])
    assert cols2metrics(dev(cols), 8) == RF.cols2metrics(cols, 8)
    assert cols2metrics(cols, 9) == RF.cols2metrics(cols, 9)


# ------------------------------------------------------------------------------------------------ row-length edges
@pytest.mark.parametrize("L", LENGTHS)
def test_row_lengths(L):
    """Every step width of the kernels, dense and from an odd-ld view; the ground-truth segments lie in the LAST columns (row0 > 0)."""
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    rng = np.random.default_rng(1000 + L)
    R = min(5, L)
    M = int_matrix(rng, R, L)
    valid = (rng.random(L) < 0.7).astype(np.uint8)
    valid[rng.integers(0, L)] = 1
    row0 = L - R
    want_t2v = RF.t2v_ranks(M, 1, row0)
    want_v2t = RF.v2t_ranks_rows(M, 1, valid, row0)
    want_v2t_all = RF.v2t_ranks_rows(M, 1, None, row0)
    for name, S in layouts(M):
        same(gt_ranks(S, 1, "t2v", row0=row0, n_videos=L), want_t2v, f"t2v {name}")
        same(gt_ranks(S, 1, "v2t", query_masks=dev(valid), row0=row0, n_videos=L, transposed=False), want_v2t, f"v2t {name}")
        same(gt_ranks(S, 1, "v2t", row0=row0, n_videos=L, transposed=False), want_v2t_all, f"v2t unmasked {name}")
        same(gt_ranks(S, 1, "v2t", row0=row0, n_videos=L, transposed=False, tie="optimistic"),
             RF.v2t_ranks_rows(M, 1, None, row0, tie="optimistic"), f"optimistic {name}")
        for k in (1, 5, 64):
            for cv, v in ((None, None), (dev(valid), valid)):
                vals, idx = topk_rows(S, k, col_valid=cv)
                wv, wi = RF.topk_rows(M, k, v)
                same(idx, wi, f"top-{k} idx {name} masked={v is not None}")
                same(vals, wv, f"top-{k} values {name}")


def test_many_trips():
    """3 x 70 001: the column loops run many trips (17 of the rank kernel's, 35 of the top-k kernel's)."""
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    rng = np.random.default_rng(7)
    L = 70001
    M = int_matrix(rng, 3, L)
    valid = (rng.random(L) < 0.5).astype(np.uint8)
    valid[-3:] = [1, 0, 1]
    for name, S in layouts(M):
        same(gt_ranks(S, 1, "t2v", row0=L - 3, n_videos=L), RF.t2v_ranks(M, 1, L - 3), name)
        same(gt_ranks(S, 1, "v2t", query_masks=dev(valid), row0=L - 3, n_videos=L, transposed=False),
             RF.v2t_ranks_rows(M, 1, valid, L - 3), name)
        for k in (5, 64):
            vals, idx = topk_rows(S, k, col_valid=dev(valid))
            wv, wi = RF.topk_rows(M, k, valid)
            same(idx, wi, name)
            same(vals, wv, name)


def test_topk_ascending_row():
    """The worst case of the candidate buffer: every column beats the bar, so every tile ends in a sort."""
    from egovlp_amd.retrieval_ops import topk_rows
    M = np.stack([np.arange(10000, dtype=np.float32), -np.arange(10000, dtype=np.float32), np.zeros(10000, dtype=np.float32)])
    vals, idx = topk_rows(dev(M), 64)
    wv, wi = RF.topk_rows(M, 64)
    same(idx, wi, "idx")
    same(vals, wv, "values")


@pytest.mark.parametrize("qpv", [1, 3, 20])
def test_queries_per_video(qpv):
    from egovlp_amd.retrieval_ops import gt_ranks
    rng = np.random.default_rng(40 + qpv)
    nv = 13
    sims = int_matrix(rng, qpv * nv, nv)
    mask = (rng.random(qpv * nv) < 0.6).astype(np.uint8)
    mask[::qpv] = 1
    for m in (None, mask):
        md = None if m is None else dev(m)
        want = RF.v2t_ranks(sims, m)
        same(gt_ranks(dev(sims), qpv, "v2t", query_masks=md), want, "transposed")
        same(gt_ranks(dev(sims.T), qpv, "v2t", query_masks=md, transposed=False), want, "row form")
        same(gt_ranks(dev(sims.T)[5:9], qpv, "v2t", query_masks=md, row0=5, n_videos=nv, transposed=False), want[5:9], "chunk")
    want = RF.t2v_ranks(sims)
    same(gt_ranks(dev(sims), qpv, "t2v"), want, "t2v")
    c0 = qpv * nv - 7
    same(gt_ranks(dev(sims)[c0:], qpv, "t2v", row0=c0, n_videos=nv), want[c0:], "t2v chunk")


# ------------------------------------------------------------------------------------------------ values
def test_special_values():
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    rng = np.random.default_rng(3)
    sims = int_matrix(rng, 60, 30)
    sims[rng.random(sims.shape) < 0.1] = np.inf
    sims[rng.random(sims.shape) < 0.1] = -np.inf
    sims[0, 0], sims[3, 1] = np.inf, -np.inf                     # a ground truth at each end
    zeros = np.where(rng.random((60, 30)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    for M in (sims, zeros):
        same(gt_ranks(dev(M), 2, "t2v"), RF.t2v_ranks(M), "t2v")
        same(gt_ranks(dev(M), 2, "v2t"), RF.v2t_ranks(M), "v2t")
        vals, idx = topk_rows(dev(M), 5)
        wv, wi = RF.topk_rows(M, 5)
        same(idx, wi, "top-5 idx")
        same(vals, wv, "top-5 values")
    same(gt_ranks(dev(zeros), 2, "t2v"), np.zeros(60), "-0.0 ties +0.0")
    same(gt_ranks(dev(zeros), 2, "v2t"), np.full(30, 59 / 2), "-0.0 ties +0.0")


def test_all_equal_matrix():
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    sims = np.full((90, 30), 0.375, dtype=np.float32)
    mask = np.ones(90, dtype=np.uint8)
    mask[[1, 2, 50, 77]] = 0
    same(gt_ranks(dev(sims), 3, "t2v"), np.zeros(90), "t2v")
    same(gt_ranks(dev(sims), 3, "v2t"), np.full(30, (90 - 1) / 2), "v2t")
    same(gt_ranks(dev(sims), 3, "v2t", query_masks=dev(mask)), np.full(30, (86 - 1) / 2), "v2t masked")
    vals, idx = topk_rows(dev(sims), 7)
    same(idx, np.tile(np.arange(7, dtype=np.int64), (90, 1)), "ties by ascending column")


# ------------------------------------------------------------------------------------------------ masks
def test_masks():
    from egovlp_amd.model.metric import t2v_metrics, v2t_metrics
    from egovlp_amd.retrieval_ops import topk_rows
    rng = np.random.default_rng(11)
    nv, qpv = 21, 4
    sims = int_matrix(rng, nv * qpv, nv)
    first = np.zeros((nv, qpv), dtype=np.uint8)
    first[:, 0] = 1
    last = np.zeros((nv, qpv), dtype=np.uint8)
    last[:, -1] = 1
    gone = np.ones((nv, qpv), dtype=np.uint8)
    gone[6] = 0
    for mask in (first, last, gone):                             # query_masks in any shape with Nq elements
        res, per = v2t_metrics(dev(sims), dev(mask), per_query=True)
        want = RF.v2t_ranks(sims, mask)
        same(per, want, "v2t")
        assert res == RF.cols2metrics(want, nv)
        res, per = t2v_metrics(dev(sims), mask, per_query=True)
        want_res, want = RF.t2v_metrics(sims, mask)
        assert per.numel() == int(mask.sum()) and res == want_res
        same(per, want, "t2v")
    assert np.isinf(host(v2t_metrics(dev(sims), dev(gone), per_query=True)[1])).tolist() == [v == 6 for v in range(nv)]
    # fewer valid columns than k: the tail is -inf / -1
    rows = np.ascontiguousarray(sims.T)
    vals, idx = topk_rows(dev(rows), 64, col_valid=dev(first.reshape(-1)))
    wv, wi = RF.topk_rows(rows, 64, first.reshape(-1))
    assert (wi[:, nv:] == -1).all() and np.isneginf(wv[:, nv:]).all() and (wi[:, :nv] >= 0).all()
    same(idx, wi, "idx")
    same(vals, wv, "values")


# ------------------------------------------------------------------------------------------------ the evaluator
def feed(ev, t, v, mask, qpv):
    """Two batches, the captions of a batch grouped per video."""
    b = v.shape[0] // 2
    for v0, v1 in ((0, b), (b, v.shape[0])):
        ev.update(dev(t[v0 * qpv:v1 * qpv]), dev(v[v0:v1]), None if mask is None else mask[v0 * qpv:v1 * qpv])


@pytest.mark.parametrize("D", [4, 64, 132, 256, 768])
def test_evaluator_exact(D):
    """Integer embeddings in [-8, 8]: every dot product is an integer of magnitude <= 64 D < 2^24, exact in any summation order and
    in the split-bf16 product, so ranks and top-k lists equal those of the integer matrix, whatever the chunking."""
    from egovlp_amd.trainer.retrieval_eval import RecallEvaluator
    rng = np.random.default_rng(D)
    for nv, qpv in ((130, 1), (65, 3)):
        nq = nv * qpv
        t, v = rng.integers(-8, 9, size=(nq, D)), rng.integers(-8, 9, size=(nv, D))
        S = (t @ v.T).astype(np.float32)
        assert np.abs(t @ v.T).max() < 2 ** 24
        mask = (rng.random(nq) < 0.7).astype(np.uint8)
        mask[::qpv] = 1
        mask[qpv * 9:qpv * 10] = 0                               # one video without a caption
        t32, v32 = t.astype(np.float32), v.astype(np.float32)
        want_t2v, want_v2t = RF.t2v_metrics(S, mask), RF.v2t_metrics(S, mask)
        row_t2v, row_v2t = 4 * nv, 4 * nq
        for rows in (1, 7, None):
            for m in ((mask, None) if rows == 7 else (mask,)):
                # one budget serves both walks: sized for the longer row (v2t), the t2v walk then takes more rows per chunk
                ev = RecallEvaluator(queries_per_video=qpv, normalize=False,
                                     chunk_bytes=1 << 40 if rows is None else rows * max(row_t2v, row_v2t))
                feed(ev, t32, v32, m, qpv)
                r_t, r_v, _ = ev.ranks()
                same(r_t, RF.t2v_ranks(S), "t2v ranks")
                same(r_v, RF.v2t_ranks(S, m), "v2t ranks")
                for k, d, want in ((5, "t2v", RF.topk_rows(S, 5)), (5, "v2t", RF.topk_rows(S.T, 5, m))):
                    vals, idx = ev.topk(k, d)
                    same(idx, want[1], f"top-{k} {d}")
                    same(vals, want[0], f"top-{k} {d}")
                out = ev.compute()
                if m is not None:
                    assert out == {0: {"t2v_metrics": want_t2v[0], "v2t_metrics": want_v2t[0]}}
                assert ev._text == [[]]
        # a budget below one row: one row per chunk, in both walks
        ev = RecallEvaluator(queries_per_video=qpv, normalize=False, chunk_bytes=1)
        feed(ev, t32, v32, mask, qpv)
        assert ev.compute() == {0: {"t2v_metrics": want_t2v[0], "v2t_metrics": want_v2t[0]}}


NORMALISED = [(256, 65, 3, 1), (64, 130, 1, 2), (768, 129, 2, 3), (256, 1100, 1, 1)]     # D, Nv, qpv, seed


def normalised_case(D, nv, qpv, seed):
    """Embeddings in an 8-dimensional subspace, the fp64 scores of their fp64 normalisation, and per query the interval of ranks
    those scores allow when every device score may be off by delta."""
    g = torch.Generator().manual_seed(seed)
    nq = nv * qpv
    basis = torch.randn(8, D, generator=g)                       # one subspace for both sets: the cosines spread over [-1, 1]
    t = (torch.randn(nq, 8, generator=g) @ basis).numpy()
    v = (torch.randn(nv, 8, generator=g) @ basis).numpy()
    mask = None
    if qpv > 1:
        mask = (torch.rand(nq, generator=g) < 0.7).numpy().astype(np.uint8)
        mask[::qpv] = 1
    t64, v64 = t.astype(np.float64), v.astype(np.float64)
    S = (t64 / np.linalg.norm(t64, axis=1, keepdims=True)) @ (v64 / np.linalg.norm(v64, axis=1, keepdims=True)).T
    # twice the worst-case error of a unit-vector dot product on the split-bf16 GEMM: the dropped lo.lo term and the two plane
    # roundings (3 * 2^-18), fp32 accumulation over D and the normalisation ((D + 8) * 2^-24)
    delta = 2 * (3 * 2.0 ** -18 + (D + 8) * 2.0 ** -24)
    g_t = S[np.arange(nq), np.arange(nq) // qpv][:, None]
    t2v = ((S > g_t + delta).sum(1), (S >= g_t - delta).sum(1) - 1)
    valid = np.ones(nq, dtype=bool) if mask is None else mask != 0
    Sv = S.T[:, valid]                                           # [videos, valid captions]
    own = (np.arange(nq) // qpv)[valid][None, :] == np.arange(nv)[:, None]
    g_v = np.where(own, Sv, -np.inf).max(1)[:, None]
    v2t = ((Sv > g_v + delta).sum(1), (Sv >= g_v - delta).sum(1) - 1)
    return t, v, mask, t2v, v2t


@pytest.mark.parametrize("D,nv,qpv,seed", NORMALISED)
def test_evaluator_normalised(D, nv, qpv, seed):
    """normalize=True on real-valued embeddings: every rank must lie in the interval the fp64 scores allow,
    #{s > g + delta} <= rank <= #{s >= g - delta} - 1 (v2t: g the fp64 maximum over the video's valid captions), and -- so that the
    interval cannot hide a failure -- at least 85 % of the queries of each case have a one-point interval (asserted on the host
    side, from the fp64 scores alone)."""
    from egovlp_amd.trainer.retrieval_eval import RecallEvaluator
    t, v, mask, t2v, v2t = normalised_case(D, nv, qpv, seed)
    for lo, hi in (t2v, v2t):
        assert (lo <= hi).all()
        share = float((lo == hi).mean())
        print("one-point intervals: %.1f %%" % (100 * share))
        assert share >= 0.85
    ev = RecallEvaluator(queries_per_video=qpv, normalize=True, chunk_bytes=4 * nv * qpv * 50)
    feed(ev, t, v, mask, qpv)
    r_t, r_v, _ = ev.ranks()
    for name, r, (lo, hi) in (("t2v", host(r_t), t2v), ("v2t", host(r_v), v2t)):
        bad = np.flatnonzero((r < lo) | (r > hi))
        assert bad.size == 0, (name, bad[:8], r[bad[:8]], lo[bad[:8]], hi[bad[:8]])
    res = ev.compute()[0]
    keep = slice(None) if mask is None else mask != 0
    assert res["t2v_metrics"] == RF.cols2metrics(host(r_t)[keep], int(host(r_t)[keep].size))
    assert res["v2t_metrics"] == RF.cols2metrics(host(r_v), nv)


def test_row_normalize():
    """x / max(|x|, eps) against fp64.  The kernel sums D squares in fp32 (relative error of the sum <= (D + 1) * 2^-24 in any
    order), takes a square root (halves it, adds 2^-24) and divides (2^-24): the bar is (D + 8) * 2^-24 relative to the largest
    entry of a unit vector, 1."""
    from egovlp_amd.retrieval_ops import row_normalize
    g = torch.Generator().manual_seed(5)
    for D in (1, 3, 64, 257, 768):
        x = torch.randn(37, D, generator=g)
        x[5] = 0                                                 # |x| < eps: 0 / eps = 0
        x[6] *= 1e-10
        want = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-8)
        big = torch.zeros(37, D + 3).cuda()
        big[:, 2:2 + D] = x.cuda()
        for xin in (x.cuda(), big[:, 2:2 + D]):
            got = row_normalize(xin)
            assert got.shape == x.shape and got.is_contiguous()
            err = float((got.double().cpu() - want).abs().max())
            assert err <= (D + 8) * 2.0 ** -24, (D, err)
        assert float(got[5].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bits():
    from egovlp_amd.retrieval_ops import gt_ranks, topk_rows
    S = torch.randn(64, 5000, generator=torch.Generator().manual_seed(1)).cuda()
    S[:, ::7] = S[:, 1:2]                                        # ties
    Q = S[:, :64 * 3].reshape(192, 64).contiguous()              # [captions, videos], qpv 3: the transposed form
    valid = (torch.rand(5000, generator=torch.Generator().manual_seed(2)) < 0.8).cuda()

    def run():
        return [gt_ranks(S, 1, "t2v", n_videos=5000), gt_ranks(S, 1, "v2t", query_masks=valid, n_videos=5000, transposed=False),
                gt_ranks(Q, 3, "v2t", query_masks=valid[:192]), *topk_rows(S, 10), *topk_rows(S, 64, col_valid=valid)]
    for x, y in zip(run(), run()):
        assert torch.equal(x, y)
