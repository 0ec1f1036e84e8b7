"""The text tower's input kernels and the text projection's relu + split on a real MI355X (`pytest -m gpu`): egv_embed_fwd,
egv_embed_bwd and egv_relu_split (csrc/format.hip) through the C ABI, every buffer inside sentinel guards
(tests/layernorm_ref.py: Guarded), against plain references of the same operations.

egv_embed_fwd is one rounding per element: bit-exact.  egv_embed_bwd adds c terms per element with atomics in any order: within
(c - 1) u sum |terms| (u = 2^-24), bit-exact for c <= 2, exactly zero where nothing lands (absent ids, the pad row, positions >= L).
egv_relu_split is relu then two roundings to bf16: bit-exact, NaN stays NaN as under nn.ReLU.

Largest err / ((c - 1) u sum |terms|) observed on an MI355X: d_word 0.87, d_pos 0.91 (sums of three terms: two roundings to nearest,
each of which can reach its half ulp).  egv_relu_split returned 0 for a NaN while it used fmaxf; `x <= 0 ? 0 : x` hands it on."""
import pytest
import torch

import layernorm_ref as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
V, P = 11, 40              # vocabulary, position table

_WORST = {}


@pytest.fixture(scope="module")
def ops():
    from egovlp_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _ops


def _h():
    from egovlp_amd import _lib
    return _lib.lib()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ids(B, Ln, seed, all_same=None):
    """int64 [B, Ln] with repeats, 0 and V - 1 (the last table row sits against the guard)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, Ln), generator=g)
    flat = ids.view(-1)
    flat[0] = V - 1
    flat[-1] = 0
    if flat.numel() > 2:
        flat[1] = V - 1
    if all_same is not None:
        ids.fill_(all_same)
    return ids


SHAPES = [(1, 1, 4), (3, 5, 8), (2, 32, 768), (3, 7, 772)]


@pytest.mark.parametrize("B,Ln,D", SHAPES)
def test_embed_fwd(ops, B, Ln, D):
    """e[b, l] = word[ids[b, l]] + pos[l], bit for bit; the tables and the ids unchanged; nothing outside e written."""
    g = torch.Generator().manual_seed(D + B)
    ids = _ids(B, Ln, D)
    word, pos = torch.randn(V, D, generator=g), torch.randn(P, D, generator=g)
    gi = L.Guarded(F32).add("word", V, D, data=word).add("pos", P, D, data=pos).build(DEV)
    go = L.Guarded(F32).add("e", B * Ln, D).build(DEV)
    ids_d = ids.to(DEV)
    assert _h().egv_embed_fwd(ids_d.data_ptr(), gi.ptr("word"), gi.ptr("pos"), B, Ln, D, go.ptr("e"), ops._stream()) == 0
    torch.cuda.synchronize()
    gi.assert_untouched("embed_fwd")
    go.assert_intact("embed_fwd")
    assert torch.equal(ids_d.cpu(), ids)
    assert _same(go.get("e"), L.embed_fwd_ref(ids, word, pos))


def _embed_bwd(ops, ids, de, D, pad_id, what):
    B, Ln = ids.shape
    gi = L.Guarded(F32).add("de", B * Ln, D, data=de).build(DEV)
    go = L.Guarded(F32).add("d_word", V, D, data=torch.zeros(V, D)).add("d_pos", P, D, data=torch.zeros(P, D)).build(DEV)
    ids_d = ids.to(DEV)
    assert _h().egv_embed_bwd(ids_d.data_ptr(), gi.ptr("de"), B, Ln, D, int(pad_id), go.ptr("d_word"), go.ptr("d_pos"), ops._stream()) == 0
    torch.cuda.synchronize()
    gi.assert_untouched(what)
    go.assert_intact(what)
    assert torch.equal(ids_d.cpu(), ids)
    d_word, d_pos = go.get("d_word"), go.get("d_pos")
    rw, rp, sw, sp, nw, npos = L.embed_bwd_ref64(ids, de, V, P, pad_id)
    worst = {}
    for name, got, ref, s, n in (("d_word", d_word, rw, sw, nw), ("d_pos", d_pos, rp, sp, npos)):
        none, few = n == 0, (n >= 1) & (n <= 2)
        assert bool((_bits(got[none]) == 0).all()), (what, name, "a row nothing lands on is not exactly zero")
        assert _same(got[few], ref[few].float()), (what, name, "a sum of at most two terms is not exact")
        many = n > 2
        if bool(many.any()):
            k = (n[many] - 1).double()[:, None]
            worst[name] = float(((got[many].double() - ref[many]).abs() / (k * L.U * s[many]).clamp(min=1e-300)).max())
    for k, r in worst.items():
        _WORST[k] = max(_WORST.get(k, 0.0), r)
    print("%s: largest err / ((c - 1) u sum |terms|): %s   (all cases so far: %s)" % (what, worst, _WORST))
    assert all(r <= 1.0 for r in worst.values()), (what, worst)
    return d_word, d_pos


@pytest.mark.parametrize("pad_id", [0, -1])
@pytest.mark.parametrize("B,Ln,D", SHAPES)
def test_embed_bwd(ops, B, Ln, D, pad_id):
    """d_pos[l] = sum_b de[b, l] (rows >= L exactly zero), d_word[id] = the sum over its occurrences (absent ids exactly zero); the
    pad_id row stays exactly zero although id 0 occurs, and pad_id = -1 switches that off."""
    g = torch.Generator().manual_seed(D + B)
    ids = _ids(B, Ln, D + 1)
    de = torch.randn(B * Ln, D, generator=g)
    d_word, _ = _embed_bwd(ops, ids, de, D, pad_id, "embed_bwd B %d L %d D %d pad %d" % (B, Ln, D, pad_id))
    assert int((ids == 0).sum()) >= 1
    assert bool((d_word[0] != 0).any()) == (pad_id == -1)


@pytest.mark.parametrize("pad_id", [-1, 3])
def test_embed_bwd_every_token_the_same_id(ops, pad_id):
    """B L atomics land on ONE row of d_word (and, with that id as pad_id, on none)."""
    B, Ln, D = 3, 7, 772
    g = torch.Generator().manual_seed(9)
    de = torch.randn(B * Ln, D, generator=g)
    d_word, _ = _embed_bwd(ops, _ids(B, Ln, 1, all_same=3), de, D, pad_id, "embed_bwd all tokens id 3, pad %d" % pad_id)
    assert bool((d_word[3] != 0).any()) == (pad_id == -1)


def _special(rows, cols, seed):
    """N(0, 1) with -0.0, +0.0, denormals of both signs, +-inf, NaN and the largest / smallest normals sprinkled over every row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    vals = [-0.0, 0.0, 1e-40, -1e-40, float("inf"), float("-inf"), float("nan"), 3.4e38, -3.4e38, 1.1754944e-38, -1.1754944e-38]
    flat = x.view(-1)
    for i, v in enumerate(vals):
        flat[(i * 7 + 1) % flat.numel()] = v
        flat[flat.numel() - 1 - (i * 5) % flat.numel()] = v
    if flat.numel() <= len(vals):                    # the 1 x 4 case: the values that matter most
        flat[:4] = torch.tensor([float("nan"), -0.0, 1e-40, -3.0])
    return x


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("rows,cols", [(1, 4), (3, 8), (5, 260), (9, 768)])
def test_relu_split(ops, rows, cols, strided):
    """Planes bit-identical to split_bf16(relu(x)), contiguous and as the strided CLS view of the text projection (ldx = L D, ldo >
    cols with sentinel gaps); x holds -0.0, denormals, +-inf and NaN, and NaN comes out as NaN: nn.ReLU propagates it."""
    Ln = 6
    x = _special(rows, cols, rows + cols)
    ldx, ldo = (Ln * cols, cols + 8) if strided else (cols, cols)
    gi = L.Guarded(F32).add("x", rows, cols, ldx, x).build(DEV)
    for passes in (3, 1):
        go = L.Guarded(BF16).add("hi", rows, cols, ldo).add("lo", rows, cols, ldo).build(DEV)
        assert _h().egv_relu_split(gi.ptr("x"), ldx, rows, cols, go.ptr("hi"), go.ptr("lo") if passes == 3 else None, ldo, ops._stream()) == 0
        torch.cuda.synchronize()
        gi.assert_untouched("relu_split")
        go.assert_intact("relu_split %dx%d strided %s" % (rows, cols, strided))
        want_hi, want_lo = L.split_bf16_ref(L.relu_ref(x))
        hi, lo = go.get("hi"), go.get("lo")
        nan = torch.isnan(x)
        assert bool(nan.any()) and bool(torch.isnan(hi[nan]).all()), "relu(NaN) must be NaN (nn.ReLU), not 0"
        assert torch.equal(torch.isnan(hi), torch.isnan(want_hi))
        assert _same(hi[~nan], want_hi[~nan]), "hi != bf16(relu(x))"
        if passes == 3:
            ln = torch.isnan(want_lo)                       # NaN inputs, and inf - inf behind an infinite hi
            assert torch.equal(torch.isnan(lo), ln) and _same(lo[~ln], want_lo[~ln]), "lo != bf16(relu(x) - hi)"
        else:
            assert go.get("lo").view(torch.int16).eq(L.SENTINEL[BF16]).all(), "lo written though NULL"


def test_relu_split_wrapper_takes_the_strided_view(ops):
    """ops.relu_split on x[:, 0] of a [B, L, D] tensor, as model/model.py calls it."""
    B, Ln, D = 5, 6, 260
    x = _special(B * Ln, D, 3).view(B, Ln, D)
    pl = ops.relu_split(x.to(DEV)[:, 0], 3)
    want_hi, want_lo = L.split_bf16_ref(L.relu_ref(x[:, 0].contiguous()))
    hi, lo = pl.hi.cpu(), pl.lo.cpu()
    ok_h, ok_l = ~torch.isnan(want_hi), ~torch.isnan(want_lo)
    assert torch.equal(torch.isnan(hi), ~ok_h) and torch.equal(torch.isnan(lo), ~ok_l)
    assert _same(hi[ok_h], want_hi[ok_h]) and _same(lo[ok_l], want_lo[ok_l])
