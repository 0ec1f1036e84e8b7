"""TEST INFRASTRUCTURE: plain-torch restatement of Mixup / CutMix and of the soft-target classification head (label smoothing and
mixed targets), in any dtype (the tests' yardstick is fp64).  The reference has no counterpart: torch's own
`F.cross_entropy(x, probabilities)` and `F.cross_entropy(x, t, label_smoothing=)` are the independent yardsticks the CPU tests hold
this restatement to.  Never imported by the product."""
import torch


def soft_targets(t, t2, lam, eps, C, dtype=torch.float64):
    """q [n, C] = (1 - eps) (lam e(t) + (1 - lam) e(t2)) + eps / C;  t2 None: t2 = t;  lam None: lam = 1."""
    t = torch.as_tensor(t).long()
    n = t.shape[0]
    t2 = t if t2 is None else torch.as_tensor(t2).long()
    lam = torch.ones(n, dtype=dtype) if lam is None else torch.as_tensor(lam).to(dtype)
    e1 = torch.zeros(n, C, dtype=dtype).scatter_(1, t.view(-1, 1), 1.0)
    e2 = torch.zeros(n, C, dtype=dtype).scatter_(1, t2.view(-1, 1), 1.0)
    return (1.0 - eps) * (lam.view(-1, 1) * e1 + (1.0 - lam).view(-1, 1) * e2) + eps / C


def soft_loss(x, q, s=1.0):
    """-> (loss, dlogits): loss = s mean_r(logsumexp(x_r) - sum_c q_rc x_rc), dlogits = s (softmax(x) - q) / n, written out."""
    n = x.shape[0]
    lse = torch.logsumexp(x, dim=1)
    loss = s * (lse - (q * x).sum(dim=1)).sum() / n
    return loss, s * (torch.exp(x - lse.view(-1, 1)) - q) / n


def soft_head(feats, W, b, t, t2, lam, eps, state=None, row0=0, B=None, dtype=torch.float64):
    """The soft head chain on a gathered block of n rows, seen from the rank that owns rows [row0, row0 + B): scores = feats W^T + b,
    loss = s mean(logsumexp - sum q x) with s = mean(state) (PNR) or 1, and the gradients the LOCAL rows leave: dW = g^T feats_local,
    db = sum g, dfeats = g W, g = the local rows of dlogits.  Every operation in `dtype`.  -> dict scores, loss, dW, db, dfeats."""
    feats, W, b = feats.to(dtype), W.to(dtype), b.to(dtype)
    n, C = feats.shape[0], W.shape[0]
    B = n if B is None else B
    x = feats @ W.t() + b
    q = soft_targets(t, t2, lam, eps, C, dtype)
    s = 1.0 if state is None else torch.as_tensor(state).to(dtype).mean()
    loss, dlogits = soft_loss(x, q, s)
    g = dlogits[row0:row0 + B]
    return {"scores": x, "loss": loss, "dW": g.t() @ feats[row0:row0 + B], "db": g.sum(dim=0), "dfeats": g @ W}


def clamp_tables(mix_idx, B, H, W):
    """The table as the kernels read it: partner clamped into [0, B), the box into the frame, op & 3."""
    m = torch.as_tensor(mix_idx).long().clone()
    m[:, 0] = m[:, 0].clamp(0, B - 1)
    m[:, 1] = m[:, 1] & 3
    m[:, 2:4] = m[:, 2:4].clamp(0, H)
    m[:, 4:6] = m[:, 4:6].clamp(0, W)
    return m


def mix_clips(A, mix_idx, mix_lam):
    """A [B, T, C, H, W], the fully transformed clips -> the mixed batch, in A's dtype.  op 1: lam A_b + (1 - lam) A_p with (1 - lam)
    formed in fp32 (the kernels' order); op 2: A_p inside rows [y0, y1) x columns [x0, x1) of every frame; the partner enters unmixed."""
    B, _, _, H, W = A.shape
    m = clamp_tables(mix_idx, B, H, W)
    lam32 = torch.as_tensor(mix_lam).to(torch.float32)
    out = A.clone()
    for b in range(B):
        p, op, y0, y1, x0, x1 = [int(v) for v in m[b]]
        if op == 1:
            out[b] = lam32[b].to(A.dtype) * A[b] + (1.0 - lam32[b]).to(A.dtype) * A[p]
        elif op == 2 and y1 > y0 and x1 > x0:
            out[b, :, :, y0:y1, x0:x1] = A[p, :, :, y0:y1, x0:x1]
    return out
