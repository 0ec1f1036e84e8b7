"""TEST INFRASTRUCTURE: the algorithm of egovlp_amd/csrc/egonce_long.hip restated in torch, and the inputs the long-head tests
share.  Nothing n x n is formed: noun / verb rows become bit words, the similarity is walked in 64 x 64 tiles with online
(max, Z, P) statistics, the column statistics are the row statistics of the swapped problem (the mask is symmetric), and the
gradient tile G comes from the two sets of statistics.  tests/test_egonce_long_cpu.py compares it with the fp64 oracle, which
pins the bit-mask and symmetry identities without a GPU.

Never imported by the product."""
import torch

TILE = 64


def make_inputs(n, D=256, seed=0):
    """randn embeddings; per row 0-3 nouns of the first 8 classes and 0-2 verbs of the first 4 (so empty rows occur); class
    581 / 117 -- the last bit of the last word -- on every 97th / 89th row."""
    g = torch.Generator().manual_seed(1000 + seed)
    text = torch.randn(n, D, generator=g)
    video = torch.randn(n, D, generator=g)
    noun = torch.zeros(n, 582)
    verb = torch.zeros(n, 118)
    kn = torch.randint(0, 4, (n,), generator=g)
    kv = torch.randint(0, 3, (n,), generator=g)
    cn = torch.randint(0, 8, (n, 3), generator=g)
    cv = torch.randint(0, 4, (n, 2), generator=g)
    for i in range(n):
        for k in range(int(kn[i])):
            noun[i, int(cn[i, k])] = 1.0
        for k in range(int(kv[i])):
            verb[i, int(cv[i, k])] = 1.0
    noun[::97, 581] = 1.0
    verb[::89, 117] = 1.0
    return text, video, noun, verb


def offdiag_density(mask_bool):
    n = mask_bool.shape[0]
    if n < 2:
        return 0.0
    return float((mask_bool.sum() - mask_bool.diagonal().sum()).item()) / (n * (n - 1))


def pack_bits(m):
    """[n, d] -> int64 [n, W] holding 32 bits per word (bit = entry > 0), W a multiple of 4 as in the kernel's layout"""
    n, d = m.shape
    W = ((d + 31) // 32 + 3) // 4 * 4
    bits = torch.zeros(n, W * 32, dtype=torch.int64)
    bits[:, :d] = (m > 0).to(torch.int64)
    weights = (1 << torch.arange(32, dtype=torch.int64))
    return (bits.view(n, W, 32) * weights).sum(-1)


def _mask_tile(wn_i, wv_i, wn_j, wv_j, mode, i0, j0):
    ni, nj = wn_i.shape[0], wn_j.shape[0]
    diag = (torch.arange(i0, i0 + ni)[:, None] == torch.arange(j0, j0 + nj)[None, :])
    if mode == 0:
        return diag
    sn = ((wn_i[:, None, :] & wn_j[None, :, :]) != 0).any(-1)
    sv = ((wv_i[:, None, :] & wv_j[None, :, :]) != 0).any(-1)
    m = (sn & sv) if mode == 1 else (sn if mode == 2 else sv)
    return m | diag


def _stats(A, B, wn, wv, mode, n, inv_tau):
    """per row of A: running max, Z = sum a, P = sum m a over the column tiles of B, rescaled online"""
    np_ = A.shape[0]
    out = torch.zeros(3, np_, dtype=A.dtype)
    for i0 in range(0, np_, TILE):
        m = torch.full((TILE,), -3e38, dtype=A.dtype)
        Z = torch.zeros(TILE, dtype=A.dtype)
        P = torch.zeros(TILE, dtype=A.dtype)
        for j0 in range(0, np_, TILE):
            X = A[i0:i0 + TILE] @ B[j0:j0 + TILE].t()
            mk = _mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], wn[j0:j0 + TILE], wv[j0:j0 + TILE], mode, i0, j0)
            valid = (torch.arange(j0, j0 + TILE) < n)[None, :]
            cm = torch.where(valid, X, torch.full_like(X, -3e38)).max(dim=1).values
            mn = torch.maximum(m, cm)
            alpha = torch.exp(torch.clamp((m - mn) * inv_tau, min=-1e4))
            e = torch.where(valid, torch.exp((X - mn[:, None]) * inv_tau), torch.zeros_like(X))
            Z = Z * alpha + e.sum(1)
            P = P * alpha + (e * mk).sum(1)
            m = mn
        out[0, i0:i0 + TILE], out[1, i0:i0 + TILE], out[2, i0:i0 + TILE] = m, Z, P
    return out


def _grad(A, B, wn, wv, mode, n, inv_tau, own, oth):
    np_ = A.shape[0]
    dA = torch.zeros_like(A)
    sc = -inv_tau / n
    for i0 in range(0, np_, TILE):
        live = (torch.arange(i0, i0 + TILE) < n)[:, None]
        for j0 in range(0, np_, TILE):
            X = A[i0:i0 + TILE] @ B[j0:j0 + TILE].t()
            mk = _mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], wn[j0:j0 + TILE], wv[j0:j0 + TILE], mode, i0, j0).to(A.dtype)
            valid = (torch.arange(j0, j0 + TILE) < n)[None, :] & live
            eo = torch.exp((X - own[0, i0:i0 + TILE, None]) * inv_tau)
            ec = torch.exp((X - oth[0, None, j0:j0 + TILE]) * inv_tau)
            G = sc * (eo * (mk / own[2, i0:i0 + TILE, None] - 1.0 / own[1, i0:i0 + TILE, None]) +
                      ec * (mk / oth[2, None, j0:j0 + TILE] - 1.0 / oth[1, None, j0:j0 + TILE]))
            G = torch.where(valid, G, torch.zeros_like(G))
            dA[i0:i0 + TILE] += G @ B[j0:j0 + TILE]
    return dA


def long_head_ref(text, video, noun, verb, temperature=0.05, eps=1e-8, use_noun=True, use_verb=True, dtype=torch.float32):
    """-> (loss, d_text, d_video), the five steps of egv_egonce_long_fwd_bwd"""
    n, D = text.shape
    np_ = (n + TILE - 1) // TILE * TILE
    text, video = text.to(dtype), video.to(dtype)
    inv_tau = 1.0 / temperature
    mode = 0 if noun is None else (1 if (use_noun and use_verb) else (2 if use_noun else 3))
    # prep
    nt, nv = text.norm(dim=1), video.norm(dim=1)
    tn = torch.zeros(np_, D, dtype=dtype)
    vn = torch.zeros(np_, D, dtype=dtype)
    tn[:n] = text / nt.clamp_min(eps)[:, None]
    vn[:n] = video / nv.clamp_min(eps)[:, None]
    bad = False
    wn = torch.zeros(np_, 4, dtype=torch.int64)
    wv = torch.zeros(np_, 4, dtype=torch.int64)
    if noun is not None:
        bad = bool((~(noun >= 0)).any() or (~(verb >= 0)).any())
        pn, pv = pack_bits(noun), pack_bits(verb)
        wn = torch.zeros(np_, pn.shape[1], dtype=torch.int64)
        wv = torch.zeros(np_, pv.shape[1], dtype=torch.int64)
        wn[:n], wv[:n] = pn, pv
    # statistics: rows, then the swapped problem for the columns
    rs = _stats(tn, vn, wn, wv, mode, n, inv_tau)
    cs = _stats(vn, tn, wn, wv, mode, n, inv_tau)
    # loss
    terms = (torch.log(rs[2, :n]) - torch.log(rs[1, :n])) + (torch.log(cs[2, :n]) - torch.log(cs[1, :n]))
    loss = -(terms.double().sum() / n)
    if bad:
        loss = torch.tensor(float('nan'), dtype=torch.float64)
    # gradient, twice with the roles swapped, + the backward of the normalisation
    out = []
    for A, B, own, oth, nrm in ((tn, vn, rs, cs, nt), (vn, tn, cs, rs, nv)):
        g = _grad(A, B, wn, wv, mode, n, inv_tau, own, oth)[:n]
        th = A[:n]
        proj = (th * g).sum(1, keepdim=True)
        out.append(torch.where((nrm > eps)[:, None], (g - th * proj) / nrm.clamp_min(1e-30)[:, None], g / eps))
    return loss, out[0], out[1]


def oracle_head(O, text, video, noun, verb, temperature=0.05, use_noun=True, use_verb=True):
    """fp64 oracle with autograd -> (loss, d_text, d_video, mask_bool or None)"""
    td, vd = text.double().requires_grad_(True), video.double().requires_grad_(True)
    x = O.sim_matrix(td, vd)
    mask = None
    if noun is None:
        loss = O.norm_softmax_loss(x, temperature)
    else:
        sv, sn = O.sim_matrix(verb.double(), verb.double()), O.sim_matrix(noun.double(), noun.double())
        loss = O.egonce(x, sv, sn, temperature, noun=use_noun, verb=use_verb)
        eye = torch.eye(len(x), dtype=torch.float64)
        mask = ((sv * sn + eye) if (use_noun and use_verb) else ((sn + eye) if use_noun else (sv + eye))) > 0
    loss.backward()
    return loss.detach(), td.grad, vd.grad, mask


# ---- the workspace layout, restated from the host code as it stood before the long and the queue head shared one layout function
# (egl_prep_layout, egl_split, egl_layout, sig_layout, egl_args_ok): sizes in floats; a refused size is 0.
STAT_WGS, GRAD_WGS, SIG_WALK_WGS = 512, 256, 512


def args_ok(n, D, dn, dv):
    return 1 <= n <= 65536 and 4 <= D <= 256 and D % 4 == 0 and 0 <= dn <= 65536 and 0 <= dv <= 65536


def prep_layout(n, D, dn, dv):
    """-> dict(np, Dp, wn, W, ntiles, total): what prep writes at the front of a tiled head's workspace"""
    np_ = (n + TILE - 1) // TILE * TILE
    Dp = 64 if D <= 64 else 256
    wn = ((dn + 31) // 32 + 3) // 4 * 4
    W = wn + ((dv + 31) // 32 + 3) // 4 * 4
    return dict(np=np_, Dp=Dp, wn=wn, W=W, ntiles=np_ // TILE, total=2 * np_ * Dp + np_ * W + 2 * np_ + np_)


def split(ntiles, target):
    """the square split of the long and sigmoid heads -> (tiles per column range, ranges)"""
    want = min((target + ntiles - 1) // ntiles, ntiles)
    tps = (ntiles + want - 1) // want
    return tps, (ntiles + tps - 1) // tps


def long_work_floats(n, D, dn, dv):
    """egv_egonce_long_work_floats"""
    if not args_ok(n, D, dn, dv):
        return 0
    L = prep_layout(n, D, dn, dv)
    ns_s, ns_g = split(L["ntiles"], STAT_WGS)[1], split(L["ntiles"], GRAD_WGS)[1]
    return L["total"] + 2 * ns_s * 3 * L["np"] + 6 * L["np"] + ns_g * L["np"] * L["Dp"] + ns_g * L["ntiles"]


def sigmoid_work_floats(n, D, dn, dv):
    """egv_sigmoid_head_work_floats"""
    if not args_ok(n, D, dn, dv):
        return 0
    L = prep_layout(n, D, dn, dv)
    ns = split(L["ntiles"], SIG_WALK_WGS)[1]
    return L["total"] + ns * L["np"] * L["Dp"] + 3 * ns * L["ntiles"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
