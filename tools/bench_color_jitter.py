"""Time the train-transform gather with the colour jitter on one GPU.

    python tools/bench_color_jitter.py [--batch 32] [--frames 4] [--source 256x341] [--res 224] [--reps 30] [--rounds 5] [--out FILE]

B clips of T decoded uint8 frames, crop boxes and a jitter table with all three ops on (`train_transform_params_color`, the
(0.4, 0.4, 0.1) recipe), three-product planes, ViT-B/16.  Three things, HIP events, median of --reps launches after 5, the three
alternating over --rounds rounds (median and min - max of the round medians):
  (1) egv_patch_gather_u8_aug_color: crop, resize, flip, jitter, Normalize and im2col in one kernel;
  (2) egv_patch_gather_u8_aug on the same clips and boxes: the same without the jitter;
  (3) the host-shaped alternative on the device: the uint8 clip (as if it had been uploaded as such) cropped, x / 255, resized by
      F.interpolate, flipped, jittered with the torch ops of tests/color_jitter_ref.py, normalised, written as one fp32 clip, then
      egv_patch_gather.  One box per clip, so this is a loop over the clips, as the reference's loader runs it per sample.
The result of (1) is checked against (3) before anything is timed."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import color_jitter_ref as CJ
    from egovlp_amd import ops
    from egovlp_amd.data_loader.transforms import train_transform_params_color
    B, T, R, P = a.batch, a.frames, a.res, a.patch
    Hs, Ws = (int(v) for v in a.source.split("x"))
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, T, 3, Hs, Ws), generator=g, dtype=torch.uint8).cuda()
    boxes, color = train_transform_params_color(B, Hs, Ws, (0.5, 1.0), (0.4, 0.4, 0.1), generator=g)
    assert all(len(CJ.ops_of(c)) == 3 for c in color[:, 3].tolist())
    rows_h, color_h = boxes.tolist(), color.tolist()
    boxes, color = boxes.cuda(), color.cuda()
    mean = torch.tensor(ops.IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(ops.IMAGENET_STD, device="cuda").view(1, 3, 1, 1)

    def fused():
        return ops.patch_gather(u8, P, 3, aug=(boxes, R), color=color)

    def plain():
        return ops.patch_gather(u8, P, 3, aug=(boxes, R))

    def host_shaped():
        clip32 = torch.empty((B, T, 3, R, R), dtype=torch.float32, device="cuda")
        for b in range(B):
            i, j, h, w, flip = rows_h[b]
            x = F.interpolate(u8[b, :, :, i:i + h, j:j + w].float() / 255, size=(R, R), mode="bilinear", align_corners=False)
            if flip:
                x = x.flip(-1)
            clip32[b] = (CJ.apply(x, color_h[b]) - mean) / std
        return ops.patch_gather(clip32, P, 3)

    err = float((fused().float() - host_shaped().float()).abs().max())
    assert err < 2e-3, err
    rounds = {"fused": [], "plain": [], "host": []}
    for _ in range(a.rounds):
        rounds["fused"].append(timed(fused, a.reps))
        rounds["plain"].append(timed(plain, a.reps))
        rounds["host"].append(timed(host_shaped, max(3, a.reps // 10), warm=2))

    def fmt(v):
        return "%.1f us (%.1f - %.1f)" % (statistics.median(v), min(v), max(v))
    mf, mp, mh = (statistics.median(rounds[k]) for k in ("fused", "plain", "host"))
    frames = B * T
    lines = ["Colour jitter in the train-transform gather on %s: B = %d, T = %d, %d x %d -> %d, P = %d, three-product planes" % (
                 torch.cuda.get_device_name(0), B, T, Hs, Ws, R, P),
             "  max |fused - host-shaped| over the planes: %.2e" % err,
             "  (1) egv_patch_gather_u8_aug_color          %s  = %.2f us per frame" % (fmt(rounds["fused"]), mf / frames),
             "  (2) egv_patch_gather_u8_aug (no jitter)     %s  = %.2f us per frame" % (fmt(rounds["plain"]), mp / frames),
             "  (3) torch ops on an fp32 clip + egv_patch_gather  %s" % fmt(rounds["host"]),
             "  the jitter costs %.1f us (x %.2f of the plain gather); the fused gather is x %.1f faster than (3)" % (mf - mp, mf / mp, mh / mf)]
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
