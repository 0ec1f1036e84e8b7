"""TEST INFRASTRUCTURE for stochastic depth in the video tower (tests/test_drop_path_cpu.py, tests/test_gpu_drop_path.py):

  * a numpy uint32 mirror of the counter-based mask of csrc/common.h (egv_mix32 / egv_make_drop / egv_drop_scale) with the element
    index set to the sample number -- what egv_drop_path_scales writes;
  * the reference's rule (model/video_transformer.py:155,171,175 with timm's DropPath, scale_by_keep=True) on the CPU oracle's
    pieces, in whatever dtype its inputs have (the tests use fp64), with the per-sample scale vectors as INPUTS:
        tr = x + timeattn(norm3(x));  sr = x + s1[b] * attn(norm1(tr));  out = sr + s2[b] * mlp(norm2(sr))
    At all-ones scales it is oracle.egovlp_oracle.space_time_block / video_encoder (tests/test_drop_path_cpu.py checks that first).

Never imported by the product.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import egovlp_oracle as O

M32 = 0xFFFFFFFF


def mix32(x):
    """egv_mix32 on a uint32 array."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x = (x.astype(np.uint64) * np.uint64(0x7FEB352D) & np.uint64(M32)).astype(np.uint32)
    x ^= x >> np.uint32(15)
    x = (x.astype(np.uint64) * np.uint64(0x846CA68B) & np.uint64(M32)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    return x


def drop_params(p):
    """egv_make_drop: (threshold, fp32 scale) of probability p, which the C ABI takes as a float."""
    p32 = np.float32(p)
    if not p32 > 0:
        return 0, np.float32(1.0)
    t = float(p32) * 4294967296.0
    thresh = M32 if t >= 4294967295.0 else int(t)
    return thresh, np.float32(1.0) / (np.float32(1.0) - p32)


def drop_path_scales(B, p, seed, seed_dev=0):
    """fp32 [B]: s[b] = egv_drop_scale(egv_drop_resolve(egv_make_drop(p, seed, &seed_dev)), b)."""
    seed = (int(seed) ^ int(seed_dev)) & (2 ** 64 - 1)
    s0, s1 = np.uint32(seed & M32), np.uint32(seed >> 32)
    thresh, scale = drop_params(p)
    idx = np.arange(B, dtype=np.uint32)                 # b < 2^32: the high index word is 0
    h = mix32(mix32(idx ^ s0) ^ s1)
    return np.where(h >= np.uint32(thresh), scale, np.float32(0.0)).astype(np.float32)


def block(x, sd, p, cfg, n, f, s1=None, s2=None):
    """One SpaceTimeBlock with the space / MLP branches scaled per sample by s1 / s2 ([B] tensors of x's dtype; None = ones)."""
    D = cfg.embed_dim

    def ln(t, name):
        return F.layer_norm(t, (D,), sd[p + name + ".weight"], sd[p + name + ".bias"], cfg.ln_eps)
    one = torch.ones(x.shape[0], dtype=x.dtype)
    s1 = one if s1 is None else s1.to(x.dtype)
    s2 = one if s2 is None else s2.to(x.dtype)
    tr = x + O.var_attention(ln(x, "norm3"), sd, p + "timeattn.", cfg.num_heads, "time", n, f)          # :166-167, never dropped
    sr = x + s1[:, None, None] * O.var_attention(ln(tr, "norm1"), sd, p + "attn.", cfg.num_heads, "space", n, f)     # :168-171
    h = F.gelu(F.linear(ln(sr, "norm2"), sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
    return sr + s2[:, None, None] * F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])       # :175


def tower(video, sd, cfg, scales=None, prefix="video_model."):
    """SpaceTimeTransformer.forward_features -> [B, D]; scales[i] = (s1, s2) of block i (None entries / None = ones)."""
    T = video.shape[1]
    x = O.video_tokens(video, sd, cfg, prefix)
    for i in range(cfg.depth):
        s1, s2 = (scales[i] if scales is not None and scales[i] is not None else (None, None))
        x = block(x, sd, f"{prefix}blocks.{i}.", cfg, cfg.patches_per_frame, T, s1, s2)
    x = F.layer_norm(x, (cfg.embed_dim,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"], cfg.ln_eps)
    return x[:, 0]


def other_seed(s):
    """A second seed far from `s` in both words (seeds that differ by a small XOR of the low word draw permuted copies of one
    another's scales: the index is XOR-ed with that word)."""
    return (s * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & (2 ** 64 - 1)


def find_seeds(B, p, start, need_both_dropped=True, limit=4096):
    """The first seed pair (seed_space, seed_mlp) = (s, other_seed(s)), s >= start, whose draws have a kept and a dropped sample on
    either branch and (optionally) a sample dropped on both.  Used once, on the CPU, to CHOOSE the constants of the GPU tests, which
    assert the conditions themselves."""
    for s in range(start, start + limit):
        a, b = drop_path_scales(B, p, s), drop_path_scales(B, p, other_seed(s))
        if all(0 < int((v == 0).sum()) < B for v in (a, b)) and (not need_both_dropped or bool(((a == 0) & (b == 0)).any())):
            return s, other_seed(s)
    raise RuntimeError("no seed pair found")
