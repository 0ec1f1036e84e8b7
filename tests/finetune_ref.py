"""TEST INFRASTRUCTURE: plain-torch restatement of the ranking-loss head (sim_matrix + MaxMarginRankingLoss /
AdaptiveMaxMarginRankingLoss + autograd), the case table of tests/golden/finetune_head.npz and the input generator both the
fixture generator and the tests draw from.  Works in any dtype (the goldens are fp64).  Never imported by the product."""
import numpy as np
import torch

PROJ_COLS = 8
# name: (n, D, adaptive, fix_norm, zero_row)          margins are the classes' defaults: 0.2 / 0.4
CASES = {
    "mm_n4": (4, 256, False, True, False),
    "ada_n4_nofix": (4, 256, True, False, False),
    "mm_n32_nofix": (32, 256, False, False, False),
    "ada_n32": (32, 256, True, True, False),
    "mm_n48_zero": (48, 256, False, True, True),
    "ada_n48_d64_nofix": (48, 64, True, False, False),
    "mm_n200": (200, 256, False, True, False),
    "ada_n200_nofix": (200, 256, True, False, False),
    "mm_n1024": (1024, 256, False, True, False),
    "ada_n1024": (1024, 256, True, True, False),
}
FULL_MAX_N = 48          # up to here the fixture holds inputs and gradients in full; above it a seed and recorded statistics


def margin_of(adaptive):
    return 0.4 if adaptive else 0.2


def make_inputs(name, seed):
    """-> text, video [n, D] fp32, weight [n] fp32 or None.  video = 0.25 * text + noise: a fifth to a half of the hinges active."""
    n, D, adaptive, _, zero_row = CASES[name]
    rng = np.random.default_rng(seed)
    text = rng.standard_normal((n, D)).astype(np.float32)
    video = (0.25 * text + rng.standard_normal((n, D)).astype(np.float32)).astype(np.float32)
    weight = rng.uniform(0.25, 1.0, size=n).astype(np.float32) if adaptive else None
    if zero_row:
        text[1] = 0.0           # |t_1| = 0: the eps clamp of sim_matrix and the g / eps branch of its backward
    return torch.from_numpy(text), torch.from_numpy(video), None if weight is None else torch.from_numpy(weight)


def projection(D, dtype=torch.float64):
    g = np.random.default_rng(4242)
    return torch.from_numpy(g.standard_normal((D, PROJ_COLS))).to(dtype)


def sim_matrix(a, b, eps=1e-8):
    an = a / a.norm(dim=1, keepdim=True).clamp_min(eps)
    bn = b / b.norm(dim=1, keepdim=True).clamp_min(eps)
    return an @ bn.t()


def hinge_args(x, weight, margin):
    """rows[i, j] = w_i m - x_ii + x_ij,  cols[i, j] = w_i m - x_ii + x_ji."""
    d = torch.diag(x).unsqueeze(1)
    m = margin if weight is None else weight.to(x.dtype).unsqueeze(1) * margin
    return m - d + x, m - d + x.t()


def kept(n, fix_norm, dtype=torch.bool):
    k = torch.ones(n, n, dtype=torch.bool)
    if fix_norm:
        k &= ~torch.eye(n, dtype=torch.bool)
    return k.to(dtype)


def loss_from_sim(x, weight, margin, fix_norm):
    rows, cols = hinge_args(x, weight, margin)
    k = kept(x.shape[0], fix_norm, x.dtype)
    return ((torch.relu(rows) + torch.relu(cols)) * k).sum() / (2 * k.sum())


def head(text, video, weight, margin, fix_norm, eps=1e-8):
    """-> loss, sim, d_text, d_video in the dtype of `text`."""
    t = text.detach().clone().requires_grad_(True)
    v = video.detach().clone().requires_grad_(True)
    x = sim_matrix(t, v, eps)
    loss = loss_from_sim(x, weight, margin, fix_norm)
    loss.backward()
    return loss.detach(), x.detach(), t.grad, v.grad


def ambiguous(x64, weight, margin, fix_norm, tau):
    """Boolean masks (rows, cols) of the kept hinge terms whose fp64 argument lies within tau of the corner, and the active share."""
    rows, cols = hinge_args(x64, weight, margin)
    k = kept(x64.shape[0], fix_norm)
    off = ~torch.eye(x64.shape[0], dtype=torch.bool)     # the diagonal terms are the constant w_i m: never ambiguous in x
    ar, ac = (rows.abs() <= tau) & k & off, (cols.abs() <= tau) & k & off
    active = float((((rows > 0) & k).sum() + ((cols > 0) & k).sum()) / (2.0 * k.sum()))
    return ar, ac, active


def ambiguous_allowance(text64, video64, weight, margin, fix_norm, tau, eps=1e-8):
    """The gradient the ambiguous hinge terms contribute when they count as active, exactly in fp64: an implementation whose
    similarity differs from the fp64 one by rounding may switch these terms, and only these, on or off.
    -> (|d_text part|_F, |d_video part|_F, number of ambiguous terms, number of kept terms)."""
    t = text64.detach().clone().requires_grad_(True)
    v = video64.detach().clone().requires_grad_(True)
    x = sim_matrix(t, v, eps)
    rows, cols = hinge_args(x, weight, margin)
    ar, ac, _ = ambiguous(x.detach(), weight, margin, fix_norm, tau)
    count = 2 * kept(x.shape[0], fix_norm, x.dtype).sum()
    n_amb = int(ar.sum() + ac.sum())
    if n_amb == 0:
        return 0.0, 0.0, 0, int(count)
    ((rows * ar).sum() / count + (cols * ac).sum() / count).backward()
    return float(t.grad.norm()), float(v.grad.norm()), n_amb, int(count)


def rel_fro(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
