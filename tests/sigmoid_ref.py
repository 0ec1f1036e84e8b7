"""TEST INFRASTRUCTURE of the sigmoid-head tests: the fp64 oracle of the pairwise sigmoid loss with EgoNCE's positives (autograd through
the formulas, `s` and `b` requiring grad, the mask from noun @ noun^T > 0 and so on), the closed-form gradients, and the partial
scheme of egovlp_amd/csrc/sigmoid_head.hip restated in torch (row tiles x column ranges, padding masked, summed in the fixed order).

  tn_i = text_i / max(|text_i|, eps), vn_j likewise;  x_ij = tn_i . vn_j;  u_ij = exp(s) x_ij + b;  z_ij = +1 where m_ij else -1
  L = (1 / n) sum_ij softplus(-z_ij u_ij)

Never imported by the product."""
import math

import torch

import egonce_long_ref as R

TILE = R.TILE
WALK_WGS = 512          # SIG_WALK_WGS of the kernel file: the walk aims at this many workgroups
LN10, LN20, LN100 = math.log(10.0), math.log(20.0), math.log(100.0)


def make_inputs(n, D=256, seed=0, dn=16, dv=12):
    """video = 0.5 text + 0.5 noise; noun / verb multi-hots at densities 0.15 / 0.2 (so rows without any noun or verb occur)"""
    g = torch.Generator().manual_seed(7000 + seed)
    text = torch.randn(n, D, generator=g)
    video = 0.5 * text + 0.5 * torch.randn(n, D, generator=g)
    noun = (torch.rand(n, dn, generator=g) < 0.15).float()
    verb = (torch.rand(n, dv, generator=g) < 0.2).float()
    return text, video, noun, verb


def mask_of(n, noun, verb, use_noun=True, use_verb=True):
    """bool [n, n]: share a noun AND a verb, OR i == j; use_noun only: share a noun; else: share a verb; no vectors: I"""
    eye = torch.eye(n, dtype=torch.bool)
    if noun is None:
        return eye
    sn = (noun.double() @ noun.double().t()) > 0
    sv = (verb.double() @ verb.double().t()) > 0
    m = (sn & sv) if (use_noun and use_verb) else (sn if use_noun else sv)
    return m | eye


def _normalise(a, eps):
    return a / a.norm(dim=1).clamp_min(eps)[:, None]


def oracle(text, video, noun, verb, s, b, use_noun=True, use_verb=True, eps=1e-8):
    """fp64, autograd -> dict(loss, d_text, d_video, d_scale, d_bias, abs_scale = sum |G x|, abs_bias = sum |z p| / n, x, G, mask)"""
    n = text.shape[0]
    td, vd = text.double().requires_grad_(True), video.double().requires_grad_(True)
    sd = torch.tensor([float(s)], dtype=torch.float64, requires_grad=True)
    bd = torch.tensor([float(b)], dtype=torch.float64, requires_grad=True)
    x = _normalise(td, eps) @ _normalise(vd, eps).t()
    x.retain_grad()
    mask = mask_of(n, noun, verb, use_noun, use_verb)
    z = torch.where(mask, 1.0, -1.0).double()
    u = torch.exp(sd) * x + bd
    loss = torch.nn.functional.softplus(-z * u, beta=1.0, threshold=1e30).sum() / n
    loss.backward()
    G, xd = x.grad.detach(), x.detach()
    p = torch.sigmoid(-z * u.detach())
    return dict(loss=loss.detach(), d_text=td.grad, d_video=vd.grad, d_scale=float(sd.grad), d_bias=float(bd.grad),
                abs_scale=float((G * xd).abs().sum()), abs_bias=float((z * p).abs().sum() / n), x=xd, G=G, mask=mask)


def closed_form(x, mask, s, b):
    """The issue's formulas on a given x [n, n] (any dtype) -> (loss, G, d_scale, d_bias)"""
    n = x.shape[0]
    z = torch.where(mask, 1.0, -1.0).to(x.dtype)
    t = math.exp(s)
    a = -z * (t * x + b)
    loss = (a.clamp_min(0) + torch.log1p(torch.exp(-a.abs()))).sum() / n
    p = torch.sigmoid(a)
    G = -(t / n) * z * p
    return loss, G, (G * x).sum(), -(z * p).sum() / n


def walk_split(ntiles, target=WALK_WGS):
    """egl_split: tiles per column range and the number of ranges (no empty range)"""
    want = min((target + ntiles - 1) // ntiles, ntiles)
    tps = (ntiles + want - 1) // want
    return tps, (ntiles + tps - 1) // tps


def tile_scheme(text, video, noun, verb, s, b, use_noun=True, use_verb=True, eps=1e-8, dtype=torch.float64, mask_padding=True):
    """The kernels' scheme: prep (normalised rows zero-padded to a multiple of 64, packed words), the walk with roles (tn, vn) and
    (vn, tn) -- per (row tile, column range) a gradient partial and, in the first walk, one partial each of sum softplus, sum G x and
    sum z p, rows and columns >= n masked out -- finish (partials summed range by range + the backward of the normalisation) and
    reduce (partials summed in double).  mask_padding=False leaves the padded pairs in: what the padding test must tell apart.
    -> dict(loss, d_text, d_video, d_scale, d_bias, partials [3, ranges, tiles])"""
    n, D = text.shape
    np_ = (n + TILE - 1) // TILE * TILE
    ntiles = np_ // TILE
    text, video = text.to(dtype), video.to(dtype)
    mode = 0 if noun is None else (1 if (use_noun and use_verb) else (2 if use_noun else 3))
    nt, nv = text.norm(dim=1), video.norm(dim=1)
    tn = torch.zeros(np_, D, dtype=dtype)
    vn = torch.zeros(np_, D, dtype=dtype)
    tn[:n] = text / nt.clamp_min(eps)[:, None]
    vn[:n] = video / nv.clamp_min(eps)[:, None]
    wn = torch.zeros(np_, 4, dtype=torch.int64)
    wv = torch.zeros(np_, 4, dtype=torch.int64)
    if noun is not None:
        pn, pv = R.pack_bits(noun), R.pack_bits(verb)
        wn = torch.zeros(np_, pn.shape[1], dtype=torch.int64)
        wv = torch.zeros(np_, pv.shape[1], dtype=torch.int64)
        wn[:n], wv[:n] = pn, pv
    t = torch.exp(torch.tensor(float(s), dtype=dtype))
    sc = -t / n
    tps, ns = walk_split(ntiles)
    part = torch.zeros(3, ns, ntiles, dtype=dtype)
    grads = []
    for role, (A, B, nrm) in enumerate(((tn, vn, nt), (vn, tn, nv))):
        gpart = torch.zeros(ns, np_, D, dtype=dtype)
        for it in range(ntiles):
            i0 = it * TILE
            live = (torch.arange(i0, i0 + TILE) < n)[:, None]
            for r in range(ns):
                for jt in range(r * tps, min(ntiles, (r + 1) * tps)):
                    j0 = jt * TILE
                    X = A[i0:i0 + TILE] @ B[j0:j0 + TILE].t()
                    mk = R._mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], wn[j0:j0 + TILE], wv[j0:j0 + TILE], mode, i0, j0)
                    ok = (torch.arange(j0, j0 + TILE) < n)[None, :] & live
                    if not mask_padding:
                        ok = torch.ones_like(ok)
                    a = torch.where(mk, -1.0, 1.0).to(dtype) * (t * X + b)
                    e = torch.exp(-a.abs())
                    sp = a.clamp_min(0) + torch.log1p(e)
                    p = torch.where(a >= 0, torch.ones_like(e), e) / (1.0 + e)
                    zp = torch.where(mk, p, -p)
                    G = torch.where(ok, sc * zp, torch.zeros_like(zp))
                    gpart[r, i0:i0 + TILE] += G @ B[j0:j0 + TILE]
                    if role == 0:
                        part[0, r, it] += torch.where(ok, sp, torch.zeros_like(sp)).sum()
                        part[1, r, it] += (G * X).sum()
                        part[2, r, it] += torch.where(ok, zp, torch.zeros_like(zp)).sum()
        g = torch.zeros(np_, D, dtype=dtype)
        for r in range(ns):
            g = g + gpart[r]
        g, th = g[:n], A[:n]
        proj = (th * g).sum(1, keepdim=True)
        grads.append(torch.where((nrm > eps)[:, None], (g - th * proj) / nrm.clamp_min(1e-30)[:, None], g / eps))
    sums = part.double().reshape(3, -1).sum(1)
    return dict(loss=float(sums[0] / n), d_text=grads[0], d_video=grads[1], d_scale=float(sums[1]), d_bias=float(-sums[2] / n),
                partials=part)


def rel(a, b):
    return R.rel(a, b)
