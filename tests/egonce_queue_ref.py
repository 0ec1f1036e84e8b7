"""TEST INFRASTRUCTURE of the EgoNCE head with a queue of past embeddings (egovlp_amd/csrc/egonce_long.hip):

  * `oracle`: the loss in fp64 with autograd.  The K valid queue rows are constant extra columns of both softmaxes,
        Z_i = sum_j a_ij + sum_q a_iq,  P_i = sum_j m_ij a_ij + sum_q m_iq a_iq   (columns: the same with b_jq = exp(v_j . tq_q / tau)),
    m_iq the noun / verb sharing rule between batch row i and queue row q WITHOUT a diagonal; K = 0 is egonce_long_ref.oracle_head.
  * `Ring`: a host model of the ring -- slot arrays, head, filled, and the rule that a loss that is not finite pushes nothing.
  * `queue_head_ref`: the tiled algorithm of the kernels restated in torch (bit words, 64 x 64 tiles, online statistics, the own term
    alone on queue tiles, sum G X from both walks); at K = 0 it performs the operations of egonce_long_ref.long_head_ref.
  * `split_inputs`: egonce_long_ref.make_inputs(n + Q, D, seed), the first n rows as the batch and the rest, normalised, as the queue.

Never imported by the product."""
import math

import torch

import egonce_long_ref as R

TILE = R.TILE


# ---- the workspace layout, restated from the host code as it stood when the queue head had a layout function of its own
# (egq_split, egq_layout, egq_args_ok, egv_egonce_queue_layout)
def queue_args_ok(n, D, dn, dv, Q):
    return R.args_ok(n, D, dn, dv) and TILE <= Q <= 65536 and Q % TILE == 0 and n <= Q


def rect_split(rtiles, ctiles, target):
    """`rtiles` row tiles against `ctiles` column tiles -> (tiles per column range, ranges)"""
    want = min((target + rtiles - 1) // rtiles, ctiles)
    tps = (ctiles + want - 1) // want
    return tps, (ctiles + tps - 1) // tps


def queue_work_floats(n, D, dn, dv, Q):
    """egv_egonce_queue_work_floats"""
    if not queue_args_ok(n, D, dn, dv, Q):
        return 0
    L = R.prep_layout(n, D, dn, dv)
    ctiles = L["ntiles"] + Q // TILE
    ns_s, ns_g = rect_split(L["ntiles"], ctiles, R.STAT_WGS)[1], rect_split(L["ntiles"], ctiles, R.GRAD_WGS)[1]
    return L["total"] + 2 * ns_s * 3 * L["np"] + 6 * L["np"] + ns_g * L["np"] * L["Dp"] + 2 * ns_g * L["ntiles"]


def queue_layout(D, dn, dv):
    """egv_egonce_queue_layout -> (Dp, W), or None where it returns an error"""
    if not R.args_ok(1, D, dn, dv):
        return None
    L = R.prep_layout(1, D, dn, dv)
    return L["Dp"], L["W"]


def normalise(x, eps=1e-8):
    return x / x.norm(dim=1, keepdim=True).clamp_min(eps)


def split_inputs(n, Q, D=256, seed=0):
    """-> (text, video, noun, verb) of the batch [n, ..] and (q_text, q_video, q_noun, q_verb) [Q, ..], the queue rows normalised"""
    text, video, noun, verb = R.make_inputs(n + Q, D, seed)
    batch = (text[:n].clone(), video[:n].clone(), noun[:n].clone(), verb[:n].clone())
    queue = (normalise(text[n:]), normalise(video[n:]), noun[n:].clone(), verb[n:].clone())
    return batch, queue


def share(noun_a, verb_a, noun_b, verb_b, use_noun=True, use_verb=True):
    """bool [a, b]: rows share a noun AND a verb (use_noun only: a noun; else: a verb -- the reference's else-branch); no diagonal"""
    sn = ((noun_a > 0).double() @ (noun_b > 0).double().t()) > 0
    sv = ((verb_a > 0).double() @ (verb_b > 0).double().t()) > 0
    return (sn & sv) if (use_noun and use_verb) else (sn if use_noun else sv)


def oracle(O, text, video, noun, verb, q_text, q_video, q_noun, q_verb, K, temperature=0.05, use_noun=True, use_verb=True,
           eps=1e-8, logit_scale=None):
    """fp64 with autograd -> (loss, d_text, d_video, d_logit_scale or None, batch x queue mask [n, K] bool).  q_text / q_video: rows
    as the ring holds them (normalised; used as they stand); only the first K rows of the four queue tensors count.  `logit_scale`
    (a float s): 1 / tau = exp(s) and dL/ds is returned."""
    n = text.shape[0]
    td, vd = text.double().requires_grad_(True), video.double().requires_grad_(True)
    s = None
    if logit_scale is not None:
        s = torch.tensor(float(logit_scale), dtype=torch.float64, requires_grad=True)
    scale = (lambda z: z * s.exp()) if s is not None else (lambda z: z / temperature)
    x = O.sim_matrix(td, vd)
    eye = torch.eye(n, dtype=torch.bool)
    if noun is None:
        m, mq = eye, torch.zeros(n, K, dtype=torch.bool)
    else:
        m = share(noun, verb, noun, verb, use_noun, use_verb) | eye
        mq = share(noun, verb, q_noun[:K], q_verb[:K], use_noun, use_verb)
    tn = td / torch.max(td.norm(dim=1)[:, None], eps * torch.ones(n, 1, dtype=torch.float64))
    vn = vd / torch.max(vd.norm(dim=1)[:, None], eps * torch.ones(n, 1, dtype=torch.float64))
    xq_t = tn @ q_video[:K].double().t()            # text anchors against queued videos
    xq_v = vn @ q_text[:K].double().t()             # video anchors against queued texts
    i_sm = torch.softmax(scale(torch.cat([x, xq_t], 1)), dim=1)
    j_sm = torch.softmax(scale(torch.cat([x.t(), xq_v], 1)), dim=1)
    idiag = torch.log(torch.sum(i_sm * torch.cat([m, mq], 1), dim=1))
    jdiag = torch.log(torch.sum(j_sm * torch.cat([m.t(), mq], 1), dim=1))
    loss = -idiag.sum() / n - jdiag.sum() / n
    loss.backward()
    return loss.detach(), td.grad, vd.grad, (None if s is None else s.grad), mq


class Ring:
    """The ring on the host: slots [Q, ..] of normalised text / video rows and raw noun / verb rows, `head`, `filled`."""

    def __init__(self, Q, D, dn=582, dv=118, dtype=torch.float64):
        self.Q, self.head, self.filled = Q, 0, 0
        self.text, self.video = torch.zeros(Q, D, dtype=dtype), torch.zeros(Q, D, dtype=dtype)
        self.noun, self.verb = torch.zeros(Q, dn), torch.zeros(Q, dv)

    def push(self, text, video, noun, verb, loss, eps=1e-8):
        """the batch's rows, normalised here, go to slots (head + i) mod Q -- unless `loss` is not finite"""
        if not math.isfinite(float(loss)):
            return self
        n = text.shape[0]
        assert n <= self.Q
        slots = (self.head + torch.arange(n)) % self.Q
        self.text[slots] = normalise(text.to(self.text.dtype), eps)
        self.video[slots] = normalise(video.to(self.video.dtype), eps)
        if noun is not None:
            self.noun[slots], self.verb[slots] = noun.float(), verb.float()
        self.head = (self.head + n) % self.Q
        self.filled = min(self.Q, self.filled + n)
        return self

    def fill(self, q_text, q_video, q_noun, q_verb, K):
        "slots 0 .. K - 1 <- the given rows (already normalised); head = K mod Q, filled = K"
        self.text[:K], self.video[:K] = q_text[:K].to(self.text.dtype), q_video[:K].to(self.video.dtype)
        self.noun[:K], self.verb[:K] = q_noun[:K], q_verb[:K]
        self.head, self.filled = K % self.Q, K
        return self

    def columns(self):
        "what the head reads: (q_text, q_video, q_noun, q_verb, K), the valid slots in slot order"
        return self.text, self.video, self.noun, self.verb, self.filled


# ---------------------------------------------------------------------------------------------- the tiled algorithm
def _share_tile(wn_i, wv_i, wn_j, wv_j, mode):
    "egonce_long_ref._mask_tile without the diagonal"
    if mode == 0:
        return torch.zeros(wn_i.shape[0], wn_j.shape[0], dtype=torch.bool)
    sn = ((wn_i[:, None, :] & wn_j[None, :, :]) != 0).any(-1)
    sv = ((wv_i[:, None, :] & wv_j[None, :, :]) != 0).any(-1)
    return (sn & sv) if mode == 1 else (sn if mode == 2 else sv)


def _pad_rows(x, rows):
    out = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype)
    out[:x.shape[0]] = x
    return out


def _tiles(n, np_, K, Bb, Bq, wn, wv, qwn, qwv):
    """the column tiles of a walk in order: batch tiles of Bb (valid j < n, diagonal), then the queue tiles that hold a valid slot
    (valid slot < K, rows from K on read as zeros, no diagonal) -> (rows, words_n, words_v, valid [64] bool, j0 or None)"""
    for j0 in range(0, np_, TILE):
        yield Bb[j0:j0 + TILE], wn[j0:j0 + TILE], wv[j0:j0 + TILE], torch.arange(j0, j0 + TILE) < n, j0
    for q0 in range(0, K, TILE):
        valid = torch.arange(q0, q0 + TILE) < K
        yield Bq[q0:q0 + TILE] * valid[:, None].to(Bq.dtype), qwn[q0:q0 + TILE], qwv[q0:q0 + TILE], valid, None


def _stats(A, Bb, Bq, wn, wv, qwn, qwv, mode, n, K, inv_tau):
    np_ = A.shape[0]
    out = torch.zeros(3, np_, dtype=A.dtype)
    for i0 in range(0, np_, TILE):
        m = torch.full((TILE,), -3e38, dtype=A.dtype)
        Z = torch.zeros(TILE, dtype=A.dtype)
        P = torch.zeros(TILE, dtype=A.dtype)
        for B, bwn, bwv, valid, j0 in _tiles(n, np_, K, Bb, Bq, wn, wv, qwn, qwv):
            X = A[i0:i0 + TILE] @ B.t()
            mk = R._mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], bwn, bwv, mode, i0, j0) if j0 is not None else \
                _share_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], bwn, bwv, mode)
            valid = valid[None, :]
            cm = torch.where(valid, X, torch.full_like(X, -3e38)).max(dim=1).values
            mn = torch.maximum(m, cm)
            alpha = torch.exp(torch.clamp((m - mn) * inv_tau, min=-1e4))
            e = torch.where(valid, torch.exp((X - mn[:, None]) * inv_tau), torch.zeros_like(X))
            Z = Z * alpha + e.sum(1)
            P = P * alpha + (e * mk).sum(1)
            m = mn
        out[0, i0:i0 + TILE], out[1, i0:i0 + TILE], out[2, i0:i0 + TILE] = m, Z, P
    return out


def _grad(A, Bb, Bq, wn, wv, qwn, qwv, mode, n, K, inv_tau, own, oth, gx_batch):
    """-> (dA, sum G X over the queue tiles and, with gx_batch, the batch tiles)"""
    np_ = A.shape[0]
    dA = torch.zeros_like(A)
    sc = -inv_tau / n
    gx = torch.zeros((), dtype=torch.float64)
    for i0 in range(0, np_, TILE):
        live = (torch.arange(i0, i0 + TILE) < n)[:, None]
        for B, bwn, bwv, valid, j0 in _tiles(n, np_, K, Bb, Bq, wn, wv, qwn, qwv):
            X = A[i0:i0 + TILE] @ B.t()
            eo = torch.exp((X - own[0, i0:i0 + TILE, None]) * inv_tau)
            if j0 is not None:
                mk = R._mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], bwn, bwv, mode, i0, j0).to(A.dtype)
                ec = torch.exp((X - oth[0, None, j0:j0 + TILE]) * inv_tau)
                G = sc * (eo * (mk / own[2, i0:i0 + TILE, None] - 1.0 / own[1, i0:i0 + TILE, None]) +
                          ec * (mk / oth[2, None, j0:j0 + TILE] - 1.0 / oth[1, None, j0:j0 + TILE]))
            else:
                mk = _share_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], bwn, bwv, mode).to(A.dtype)
                G = sc * (eo * (mk / own[2, i0:i0 + TILE, None] - 1.0 / own[1, i0:i0 + TILE, None]))
            G = torch.where(valid[None, :] & live, G, torch.zeros_like(G))
            dA[i0:i0 + TILE] += G @ B
            if gx_batch or j0 is None:
                gx = gx + (G * X).double().sum()
    return dA, gx


def queue_head_ref(text, video, noun, verb, q_text, q_video, q_noun, q_verb, K, temperature=0.05, eps=1e-8, use_noun=True,
                   use_verb=True, dtype=torch.float32):
    """-> (loss, d_text, d_video, dL/ds): the steps of egv_egonce_queue_fwd_bwd on the batch and the first K queue rows"""
    n, D = text.shape
    np_ = (n + TILE - 1) // TILE * TILE
    Kp = (K + TILE - 1) // TILE * TILE
    text, video = text.to(dtype), video.to(dtype)
    inv_tau = 1.0 / temperature
    mode = 0 if noun is None else (1 if (use_noun and use_verb) else (2 if use_noun else 3))
    # prep (the long head's)
    nt, nv = text.norm(dim=1), video.norm(dim=1)
    tn = torch.zeros(np_, D, dtype=dtype)
    vn = torch.zeros(np_, D, dtype=dtype)
    tn[:n] = text / nt.clamp_min(eps)[:, None]
    vn[:n] = video / nv.clamp_min(eps)[:, None]
    bad = False
    wn = torch.zeros(np_, 4, dtype=torch.int64)
    wv = torch.zeros(np_, 4, dtype=torch.int64)
    qwn = torch.zeros(Kp, 4, dtype=torch.int64)
    qwv = torch.zeros(Kp, 4, dtype=torch.int64)
    if noun is not None:
        bad = bool((~(noun >= 0)).any() or (~(verb >= 0)).any())
        pn, pv = R.pack_bits(noun), R.pack_bits(verb)
        wn = torch.zeros(np_, pn.shape[1], dtype=torch.int64)
        wv = torch.zeros(np_, pv.shape[1], dtype=torch.int64)
        wn[:n], wv[:n] = pn, pv
        qwn, qwv = _pad_rows(R.pack_bits(q_noun[:K]), Kp), _pad_rows(R.pack_bits(q_verb[:K]), Kp)
    qt, qv = _pad_rows(q_text[:K].to(dtype), Kp), _pad_rows(q_video[:K].to(dtype), Kp)
    # statistics: text anchors against videos + queued videos, then video anchors against texts + queued texts
    rs = _stats(tn, vn, qv, wn, wv, qwn, qwv, mode, n, K, inv_tau)
    cs = _stats(vn, tn, qt, wn, wv, qwn, qwv, mode, n, K, inv_tau)
    terms = (torch.log(rs[2, :n]) - torch.log(rs[1, :n])) + (torch.log(cs[2, :n]) - torch.log(cs[1, :n]))
    loss = -(terms.double().sum() / n)
    if bad:
        loss = torch.tensor(float('nan'), dtype=torch.float64)
    out, dls = [], torch.zeros((), dtype=torch.float64)
    for A, Bb, Bq, own, oth, nrm, gx_batch in ((tn, vn, qv, rs, cs, nt, True), (vn, tn, qt, cs, rs, nv, False)):
        g, gx = _grad(A, Bb, Bq, wn, wv, qwn, qwv, mode, n, K, inv_tau, own, oth, gx_batch)
        g = g[:n]
        dls = dls + gx
        th = A[:n]
        proj = (th * g).sum(1, keepdim=True)
        out.append(torch.where((nrm > eps)[:, None], (g - th * proj) / nrm.clamp_min(1e-30)[:, None], g / eps))
    return loss, out[0], out[1], dls


rel = R.rel
