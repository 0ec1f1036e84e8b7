"""TEST INFRASTRUCTURE of the learnable-temperature tests: the fp64 oracle of dL/d(logit scale) by autograd, and the long head's
partial scheme (egovlp_amd/csrc/egonce_long.hip, `scale`) restated in torch on top of tests/egonce_long_ref.py.

With s = log(1 / tau) the heads compute L(x e^s), so dL/ds = sum_ij G_ij x_ij with G = dL/dx.  The oracle does not use that
identity: it makes `temperature = exp(-s)` with `s.requires_grad` and lets autograd differentiate the reference's own formulas.

Never imported by the product."""
import math

import torch

import egonce_long_ref as R

TILE = R.TILE
GRAD_WGS = 256          # EGL_GRAD_WGS of the kernel file: the grad walk aims at this many workgroups


def oracle_scale(O, text, video, noun, verb, temperature=0.05, use_noun=True, use_verb=True):
    """fp64 oracle with autograd through temperature = exp(-s)
    -> dict(loss, d_text, d_video, d_scale, x, G, abs_sum = sum |G_ij x_ij|, identity = sum G_ij x_ij)"""
    td, vd = text.double().requires_grad_(True), video.double().requires_grad_(True)
    s = torch.tensor([math.log(1.0 / temperature)], dtype=torch.float64, requires_grad=True)
    x = O.sim_matrix(td, vd)
    x.retain_grad()
    tau = torch.exp(-s)
    if noun is None:
        loss = O.norm_softmax_loss(x, tau)
    else:
        sv, sn = O.sim_matrix(verb.double(), verb.double()), O.sim_matrix(noun.double(), noun.double())
        loss = O.egonce(x, sv, sn, tau, noun=use_noun, verb=use_verb)
    loss.backward()
    G, xd = x.grad.detach(), x.detach()
    return dict(loss=loss.detach(), d_text=td.grad, d_video=vd.grad, d_scale=float(s.grad), x=xd, G=G,
                abs_sum=float((G * xd).abs().sum()), identity=float((G * xd).sum()))


def grad_split(ntiles, target=GRAD_WGS):
    """egl_split: tiles per column range and the number of ranges (no empty range)"""
    want = min((target + ntiles - 1) // ntiles, ntiles)
    tps = (ntiles + want - 1) // want
    return tps, (ntiles + tps - 1) // tps


def long_scale_partials(text, video, noun, verb, temperature=0.05, eps=1e-8, use_noun=True, use_verb=True, dtype=torch.float64):
    """The grad walk with roles (tn, vn): one partial sum of G X per (row tile, column range), rows and columns >= n masked out
    exactly as G is -> (partials [ranges, tiles], their sum in a fixed order)."""
    n, D = text.shape
    np_ = (n + TILE - 1) // TILE * TILE
    ntiles = np_ // TILE
    text, video = text.to(dtype), video.to(dtype)
    inv_tau = math.exp(math.log(1.0 / temperature))
    mode = 0 if noun is None else (1 if (use_noun and use_verb) else (2 if use_noun else 3))
    tn = torch.zeros(np_, D, dtype=dtype)
    vn = torch.zeros(np_, D, dtype=dtype)
    tn[:n] = text / text.norm(dim=1).clamp_min(eps)[:, None]
    vn[:n] = video / video.norm(dim=1).clamp_min(eps)[:, None]
    wn = torch.zeros(np_, 4, dtype=torch.int64)
    wv = torch.zeros(np_, 4, dtype=torch.int64)
    if noun is not None:
        pn, pv = R.pack_bits(noun), R.pack_bits(verb)
        wn = torch.zeros(np_, pn.shape[1], dtype=torch.int64)
        wv = torch.zeros(np_, pv.shape[1], dtype=torch.int64)
        wn[:n], wv[:n] = pn, pv
    own = R._stats(tn, vn, wn, wv, mode, n, inv_tau)
    oth = R._stats(vn, tn, wn, wv, mode, n, inv_tau)
    tps, ns = grad_split(ntiles)
    part = torch.zeros(ns, ntiles, dtype=dtype)
    sc = -inv_tau / n
    for it in range(ntiles):
        i0 = it * TILE
        live = (torch.arange(i0, i0 + TILE) < n)[:, None]
        for r in range(ns):
            for jt in range(r * tps, min(ntiles, (r + 1) * tps)):
                j0 = jt * TILE
                X = tn[i0:i0 + TILE] @ vn[j0:j0 + TILE].t()
                mk = R._mask_tile(wn[i0:i0 + TILE], wv[i0:i0 + TILE], wn[j0:j0 + TILE], wv[j0:j0 + TILE], mode, i0, j0).to(dtype)
                valid = (torch.arange(j0, j0 + TILE) < n)[None, :] & live
                eo = torch.exp((X - own[0, i0:i0 + TILE, None]) * inv_tau)
                ec = torch.exp((X - oth[0, None, j0:j0 + TILE]) * inv_tau)
                G = sc * (eo * (mk / own[2, i0:i0 + TILE, None] - 1.0 / own[1, i0:i0 + TILE, None]) +
                          ec * (mk / oth[2, None, j0:j0 + TILE] - 1.0 / oth[1, None, j0:j0 + TILE]))
                G = torch.where(valid, G, torch.zeros_like(G))      # the padded rows' statistics are 0: G is inf / nan there
                part[r, it] += (G * X).sum()
    return part, float(part.double().flatten().sum())
