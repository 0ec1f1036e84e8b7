"""TEST INFRASTRUCTURE: plain-torch restatement of the classification head of the OSCC / PNR fine-tunes (Linear + CrossEntropy,
the PNR weighting by mean(state), the local gradient slice of AllGather_multi.backward, oscc_metrics / pnr_metrics), the case
table of tests/golden/cls_head.npz and the input generators both the fixture generator and the tests draw from.  Works in any
dtype (the goldens are fp64).  Never imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

# name: (task, n gathered rows, K features, C classes, world, rank, kind)     B = n / world local rows
CASES = {
    "oscc_n32": ("oscc", 32, 768, 2, 1, 0, ""),              # configs/ft/oscc.json: 8 ranks x 4 clips, seen from one gathered block
    "pnr_n32_some0": ("pnr", 32, 768, 16, 8, 5, "some0"),    # configs/ft/pnr.json geometry, rank 5 of 8; some clips without a change
    "pnr_c17": ("pnr", 8, 768, 17, 2, 1, ""),                # projection_dim 17 against 16 label columns
    "pnr_k1024": ("pnr", 16, 1024, 16, 8, 5, ""),
    "oscc_n4096": ("oscc", 4096, 64, 16, 16, 9, ""),         # the limits: n = 4096, B = 256
    "pnr_all0": ("pnr", 8, 64, 16, 2, 1, "all0"),            # no clip with a state change: loss 0, gradients 0
    "oscc_tie": ("oscc", 8, 64, 4, 1, 0, "tie"),             # classes 1 and 2 score identically in every row
    "oscc_w2": ("oscc", 8, 768, 2, 2, 1, ""),
}
LABEL_COLS = 16           # the PNR loader's one-hot width (16 sampled frames)
MIN_GAP = 1e-4            # top-2 gap every (non-tied) score row must keep in fp64, so that argmax is not a rounding question
ERR_FLOOR = 2.0 ** -25    # see make_golden_cls_head.py


def local_rows(name):
    _, n, _, _, world, rank, _ = CASES[name]
    B = n // world
    return rank * B, B


def make_inputs(name, seed):
    """-> dict: feats [n, K], W [C, K], b [C] fp32; OSCC: state [n] int64 in [0, C); PNR: labels [n, 16] int64 (one-hot, or all
    zero for clips with state 0) and state [n] int64 in {0, 1}."""
    task, n, K, C, _, _, kind = CASES[name]
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((n, K)).astype(np.float32)
    W = (rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    if kind == "tie":
        W[0] *= 0.05
        W[3] *= 0.05
        W[2] = W[1]
        b[2] = b[1]
    out = {"feats": torch.from_numpy(feats), "W": torch.from_numpy(W), "b": torch.from_numpy(b)}
    if task == "oscc":
        out["state"] = torch.from_numpy(rng.integers(0, C, size=n).astype(np.int64))
        return out
    state = np.ones(n, dtype=np.int64)
    if kind == "some0":
        state[rng.permutation(n)[: n // 3]] = 0
        state[5 * (n // 8)] = 0             # one of them among rank 5's rows
    elif kind == "all0":
        state[:] = 0
    else:
        state[rng.permutation(n)[: max(1, n // 8)]] = 0
    labels = np.zeros((n, LABEL_COLS), dtype=np.int64)
    frame = rng.integers(0, LABEL_COLS, size=n)
    labels[np.arange(n), frame] = 1
    labels[state == 0] = 0
    out["labels"], out["state"] = torch.from_numpy(labels), torch.from_numpy(state)
    return out


def targets(name, inp):
    """-> (target [n] int64, state [n] or None) as the trainers form them (trainer_oscc.py:331,337, trainer_pnr.py:346-350)."""
    if CASES[name][0] == "oscc":
        return inp["state"], None
    return torch.argmax(inp["labels"].long(), dim=1), inp["state"]


def head(name, inp, dtype, loss_of=None):
    """Linear head + loss + autograd in `dtype` with this rank's view of the gather: its own rows carry gradient, the other ranks'
    rows are constants (AllGather_multi.backward keeps the local slice).  -> dict loss, scores [n, C], pred [n], dW, db,
    dfeats [B, K].  `loss_of(scores, target, state)`: the loss expression (default: the restatement below)."""
    lo, B = local_rows(name)
    feats_all = inp["feats"].to(dtype)
    W = inp["W"].to(dtype).clone().requires_grad_(True)
    b = inp["b"].to(dtype).clone().requires_grad_(True)
    mine = feats_all[lo:lo + B].clone().requires_grad_(True)
    with torch.no_grad():
        others = F.linear(feats_all, W, b)
    scores = torch.cat([others[:lo], F.linear(mine, W, b), others[lo + B:]])
    target, state = targets(name, inp)
    if loss_of is None:
        loss = F.cross_entropy(scores, target)
        if state is not None:
            loss = torch.mean(state * loss)
    else:
        loss = loss_of(scores, target, state)
    loss.backward()
    return {"loss": loss.detach(), "scores": scores.detach(), "pred": torch.argmax(scores.detach(), dim=1),
            "dW": W.grad, "db": b.grad, "dfeats": mine.grad}


def rel(a, b):
    """Relative Frobenius error; 0 when both are exactly zero (the all-state-0 case)."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    d, nb = float((a - b).norm()), float(b.norm())
    if nb == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / nb


def min_gap(scores, tie_cols=None):
    """Smallest top-2 gap over the rows (a tied pair of columns counts once)."""
    s = scores.double().clone()
    if tie_cols is not None:
        s[:, tie_cols[1]] = -float("inf")
    top = s.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


# ------------------------------------------------------------------------------------------------ metric sets
# name: (task, rows, C, fps or None, kind)
METRIC_SETS = {
    "oscc_set": ("oscc", 203, 2, None, ""),
    "pnr_2997": ("pnr", 150, 16, 29.97, ""),
    "pnr_30": ("pnr", 97, 16, 30.0, ""),
    "pnr_nopos": ("pnr", 21, 16, 30.0, "nopos"),
}


def make_metric_inputs(name, seed):
    """-> dict preds [rows, C] fp32 and the columns the metric functions take.  PNR: int64 frame numbers of 8-second parent clips,
    fps as fp64 (what the default collate makes of the loader's Python floats)."""
    task, rows, C, fps, kind = METRIC_SETS[name]
    rng = np.random.default_rng(seed)
    out = {"preds": torch.from_numpy(rng.standard_normal((rows, C)).astype(np.float32))}
    if task == "oscc":
        out["state"] = torch.from_numpy(rng.integers(0, C, size=rows).astype(np.int64))
        return out
    state = (rng.uniform(size=rows) < 0.6).astype(np.int64)
    if kind == "nopos":
        state[:] = 0
    start = rng.integers(0, 200000, size=rows).astype(np.int64)
    length = rng.integers(int(6 * fps), int(9 * fps), size=rows).astype(np.int64)
    pnr = start + (rng.uniform(0.1, 0.9, size=rows) * length).astype(np.int64)
    labels = np.zeros((rows, LABEL_COLS), dtype=np.int64)
    labels[np.arange(rows), rng.integers(0, LABEL_COLS, size=rows)] = 1
    labels[state == 0] = 0
    out.update(labels=torch.from_numpy(labels), state=torch.from_numpy(state),
               fps=torch.full((rows,), fps, dtype=torch.float64), start=torch.from_numpy(start),
               end=torch.from_numpy(start + length), pnr=torch.from_numpy(pnr))
    return out


def oscc_accuracy(preds, state):
    """model/metric.py:342-353 restated."""
    hits = sum(int(torch.argmax(p)) == int(s) for p, s in zip(preds, state))
    return hits / len(state) * 100


def pnr_distance(m):
    """model/metric.py:355-397 restated: fp32 tensor arithmetic for the mapped frame, fp64 for the error."""
    dist = []
    for i in range(m["preds"].shape[0]):
        if int(m["state"][i]) != 1:
            continue
        k = int(torch.argmax(m["preds"][i]))
        mapped = float(((m["end"][i] - m["start"][i]) / 16 * k).item())
        gt = int(m["pnr"][i]) - int(m["start"][i])
        dist.append(abs(mapped - gt) / float(m["fps"][i]))
    return float(np.mean(dist)) if dist else float("nan")
