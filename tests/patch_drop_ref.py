"""TEST INFRASTRUCTURE for patch dropout in the video tower (tests/test_patch_drop_cpu.py, tests/test_gpu_patch_drop.py):

  * a numpy mirror of egv_patch_keep_draw (include/egovlp_hip.h): the key of (clip b, position j) is the counter-based hash of
    csrc/common.h at element index b * n + j, the K positions with the smallest (key, j) pairs are kept, listed in ascending order;
  * the rule on the CPU oracle's pieces, in whatever dtype its inputs have (the tests use fp64), with the table as an INPUT: the
    full token sequence of oracle.video_tokens, index_select of [CLS] + [1 + f * n + keep[b]] per clip, then the oracle's own
    SpaceTimeBlock at n = K (optionally with drop-path scales: drop_path_ref.block), the final LayerNorm, row 0.
    At keep = arange(n) it is oracle.video_encoder (tests/test_patch_drop_cpu.py checks that first).

Never imported by the product.
"""
import numpy as np
import torch
import torch.nn.functional as F

import drop_path_ref as DR
from drop_path_ref import M32, mix32  # noqa: F401
from oracle import egovlp_oracle as O


def keep_count(n, rate):
    """timm's rule: K = max(1, int(n * (1 - rate)))."""
    return max(1, int(n * (1. - rate)))


def keys(B, n, seed, seed_dev=0):
    """uint32 [B, n]: h = mix32(mix32((uint32)idx ^ s0) ^ (uint32)(idx >> 32) ^ s1), idx = b * n + j."""
    seed = (int(seed) ^ int(seed_dev)) & (2 ** 64 - 1)
    s0, s1 = np.uint32(seed & M32), np.uint32(seed >> 32)
    idx = np.arange(B * n, dtype=np.uint64)
    lo, hi = (idx & np.uint64(M32)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
    return mix32(mix32(lo ^ s0) ^ hi ^ s1).reshape(B, n)


def patch_keep(B, n, K, seed, seed_dev=0):
    """int32 [B, K]: what egv_patch_keep_draw writes."""
    h = keys(B, n, seed, seed_dev)
    j = np.arange(n)
    out = np.empty((B, K), dtype=np.int32)
    for b in range(B):
        order = np.lexsort((j, h[b]))              # by key, ties by position
        out[b] = np.sort(order[:K])
    return out


def token_index(keep, T, n):
    """int64 [B, 1 + T*K]: rows of the full [1 + T*n] token sequence a clip keeps, in the order the tower runs them."""
    keep = torch.as_tensor(np.asarray(keep), dtype=torch.int64)
    B, K = keep.shape
    body = (1 + torch.arange(T)[None, :, None] * n + keep[:, None, :]).reshape(B, T * K)
    return torch.cat([torch.zeros(B, 1, dtype=torch.int64), body], dim=1)


def select_tokens(x, keep, T, n):
    """x [B, 1 + T*n, D] -> [B, 1 + T*K, D]."""
    idx = token_index(keep, T, n)
    return torch.stack([x[b].index_select(0, idx[b]) for b in range(x.shape[0])])


def tower(video, sd, cfg, keep, scales=None, prefix="video_model."):
    """SpaceTimeTransformer.forward_features on the kept patches -> [B, D].  scales[i] = (s1, s2): drop-path scales of block i
    (None entries / None = nothing dropped, the oracle's block)."""
    T = video.shape[1]
    n = cfg.patches_per_frame
    K = np.asarray(keep).shape[1]
    x = select_tokens(O.video_tokens(video, sd, cfg, prefix), keep, T, n)
    for i in range(cfg.depth):
        p = f"{prefix}blocks.{i}."
        if scales is not None and scales[i] is not None:
            x = DR.block(x, sd, p, cfg, K, T, *scales[i])
        else:
            x = O.space_time_block(x, sd, p, cfg, K, T)
    x = F.layer_norm(x, (cfg.embed_dim,), sd[prefix + "norm.weight"], sd[prefix + "norm.bias"], cfg.ln_eps)
    return x[:, 0]
