"""Time Mixup / CutMix in the train-transform gather and the soft-target classification head on one GPU (DESIGN.md sections 4.8
and 4.5d).

    python tools/bench_mix.py [--batch 32] [--frames 4] [--source 256x341] [--res 224] [--reps 30] [--rounds 5] [--lib FILE] [--out FILE]

The benchmark's input shape: B clips of T decoded uint8 frames, crop boxes from `train_transform_params`, three-product planes,
ViT-B/16.  HIP events, median of --reps launches after 5, the legs alternating over --rounds rounds (median and min - max of the round
medians); every figure is also given as a ratio to the plain gather / the hard head of the same run:
  gather  (1) egv_patch_gather_u8_aug, no mix -- the entry a step without the recipe calls;
          (2) egv_patch_gather_u8_aug_mix with op 0 in every row (what the mixed entry costs when nothing is mixed);
          (3) the same with a cutmix box per clip (`mix_params(..., switch_prob=1)`): by construction the bytes of (1);
          (4) the same with mixup in every clip: two clips are sampled per output pixel;
  head    (5) egv_cls_head_loss_bwd on [B, 768] features, C = 2;
          (6) egv_cls_head_loss_bwd_soft with the target2 / lam columns and label smoothing 0.1.
--lib FILE: load another build of the library (e.g. the parent commit's) and time the legs that build has, for an A/B of (1) and (5)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=5):
    """Median microseconds of fn() by HIP events."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--source", default="256x341")
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from egovlp_amd import _lib
    if a.lib:
        import ctypes
        _lib.LIB_PATH = os.path.abspath(a.lib)
        older = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.PROTOTYPES if not hasattr(older, n)]:
            del _lib.PROTOTYPES[name]               # an older build: only the legs it has are timed
    from egovlp_amd import loss_ops, ops
    from egovlp_amd.data_loader.transforms import mix_params, train_transform_params
    has_mix = "egv_patch_gather_u8_aug_mix" in _lib.PROTOTYPES
    B, T, R, P = a.batch, a.frames, a.res, a.patch
    Hs, Ws = (int(v) for v in a.source.split("x"))
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, T, 3, Hs, Ws), generator=g, dtype=torch.uint8).cuda()
    boxes = train_transform_params(B, Hs, Ws, (0.5, 1.0), generator=g).cuda()
    cut = tuple(t.cuda() for t in mix_params(B, R, R, switch_prob=1.0, mode="elem", generator=g))
    mup = tuple(t.cuda() for t in mix_params(B, R, R, switch_prob=0.0, mode="elem", generator=g))
    off = (torch.tensor([[b, 0, 0, 0, 0, 0] for b in range(B)], dtype=torch.int32).cuda(), torch.ones(B).cuda())
    legs = {"gather plain": lambda: ops.patch_gather(u8, P, 3, aug=(boxes, R))}
    if has_mix:
        legs.update({"gather mix op 0": lambda: ops.patch_gather(u8, P, 3, aug=(boxes, R), mix=off),
                     "gather cutmix": lambda: ops.patch_gather(u8, P, 3, aug=(boxes, R), mix=cut),
                     "gather mixup": lambda: ops.patch_gather(u8, P, 3, aug=(boxes, R), mix=mup)})
    K, C = 768, 2
    feats, W = torch.randn(B, K, generator=g).cuda(), (torch.randn(C, K, generator=g) / K ** 0.5).cuda()
    target = torch.randint(0, C, (B,), generator=g).cuda()
    hard_lay = loss_ops.ClsLayout(C, "oscc")
    hard_blk = hard_lay.fill(loss_ops.cls_head_fwd(feats, W, None, out=torch.empty(B, hard_lay.ld, device="cuda")), target)
    legs["head hard"] = lambda: loss_ops.cls_head_loss_bwd(hard_blk, C, hard_lay.target, feats=feats, weight=W)
    if has_mix:
        soft_lay = loss_ops.ClsLayout(C, "oscc", soft=True)
        soft_blk = soft_lay.fill(loss_ops.cls_head_fwd(feats, W, None, out=torch.empty(B, soft_lay.ld, device="cuda")), target,
                                 target2=target.flip(0), lam=mup[1])
        legs["head soft"] = lambda: loss_ops.cls_head_loss_bwd(soft_blk, C, soft_lay.target, feats=feats, weight=W,
                                                               col_target2=soft_lay.target2, col_lam=soft_lay.lam, label_smoothing=0.1)
    rounds = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            rounds[k].append(timed(fn, a.reps))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    lines = ["Mixup / CutMix in the train-transform gather and the soft-target head on %s: B = %d, T = %d, %d x %d -> %d, P = %d, "
             "three-product planes; library %s" % (torch.cuda.get_device_name(0), B, T, Hs, Ws, R, P, _lib.LIB_PATH),
             "  cutmix boxes cover %.0f %% of the frame on average; mean mixup lam %.2f" % (100.0 * (1.0 - float(cut[1].mean())),
                                                                                          float(mup[1].mean()))]
    for k, v in rounds.items():
        base = med["gather plain"] if k.startswith("gather") else med["head hard"]
        lines.append("  %-16s %8.1f us (%.1f - %.1f)   x %.2f of %s" % (k, med[k], min(v), max(v), med[k] / base,
                                                                       "the plain gather" if k.startswith("gather") else "the hard head"))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
