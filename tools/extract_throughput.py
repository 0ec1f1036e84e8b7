"""Throughput of the NLQ / MQ clip-feature extraction:

    python tools/extract_throughput.py [--out profiles/extract_throughput.json]

(a) the reference-shaped loop through the plain API (host transform to fp32, compute_video at batch 4, a host copy per batch)
against (b) ClipFeatureExtractor.video_features at batch 32, on one synthetic 600-frame 256 x 341 uint8 clip in pinned host memory,
base_patch16_224, in the library's default precision and in f16mix; then egv_patch_gather_u8_eval on its own (HIP events, 128
frames per launch) next to the plain fp32 gather.  A warm-up, then 5 (kernels: 10) repetitions: median, min, max."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egovlp_amd import ops  # noqa: E402
from egovlp_amd.data_loader.transforms import eval_transform_geometry  # noqa: E402
from egovlp_amd.extract import ClipFeatureExtractor  # noqa: E402
from egovlp_amd.model.model import FrozenInTime  # noqa: E402
from egovlp_amd.synth import synth_state_dict  # noqa: E402

REPEATS = 5


def host_transform(u8, S=256, R=224):
    H1, W1, top, left = eval_transform_geometry(u8.shape[-2], u8.shape[-1], S)
    x = u8.float() / 255
    x = F.interpolate(x, size=(H1, W1), mode="bilinear", align_corners=False)
    x = x[:, :, top:top + S, left:left + S]
    x = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False)
    return (x - torch.tensor(ops.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(ops.IMAGENET_STD).view(1, 3, 1, 1)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result JSON here as well")
    args = ap.parse_args()
    out = {"torch_threads": torch.get_num_threads()}
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0))
    m = m.cuda().eval()
    clip = torch.randint(0, 256, (600, 3, 256, 341), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).pin_memory()
    W = 150

    def run_a():
        t0 = time.perf_counter()
        x = host_transform(clip).reshape(-1, 4, 3, 224, 224)
        t1 = time.perf_counter()
        with torch.no_grad():
            x = x.cuda()
            outs = torch.zeros(W, 256)
            for j in range((W + 3) // 4):
                outs[4 * j:4 * j + 4] = m.compute_video(x[4 * j:4 * j + 4])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return t1 - t0, t2 - t0, outs

    for prec in (("bf16x3",), ("f16mix", "f16")):
        m.exec_ctx.set_precision(*prec)
        ext = ClipFeatureExtractor(m, num_frames=4, batch=32)
        name = "/".join(prec)
        run_a()
        ta = [run_a() for _ in range(REPEATS)]
        ext.video_features(clip)
        tb, fb = [], None
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fb = ext.video_features(clip)
            tb.append(time.perf_counter() - t0)
        dev_clip = clip.cuda()
        ext.video_features(dev_clip)
        tc = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ext.video_features(dev_clip)
            tc.append(time.perf_counter() - t0)
        rel = float((fb.double() - ta[-1][2].double()).norm() / ta[-1][2].double().norm())
        out[name] = {"a_windows_per_s": spread([W / t[1] for t in ta]), "a_host_transform_share": spread([t[0] / t[1] for t in ta]),
                     "a_seconds": spread([t[1] for t in ta]), "b_windows_per_s": spread([W / t for t in tb]),
                     "b_seconds": spread(tb), "b_device_frames_windows_per_s": spread([W / t for t in tc]), "rel_b_vs_a": rel}
        print(name, json.dumps(out[name]), flush=True)

    # the kernel alone: 128 output frames (32 windows), identity and non-identity stage 1
    for hs, ws in ((256, 341), (270, 480)):
        bank = torch.randint(0, 256, (128, 3, hs, ws), dtype=torch.uint8).cuda()
        for passes in (3, 1):
            for _ in range(3):
                ops.patch_gather_eval(bank, None, 4, 16, passes, 256, 224)
            ts = []
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.patch_gather_eval(bank, None, 4, 16, passes, 256, 224)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            out["kernel_us_128frames_%dx%d_passes%d" % (hs, ws, passes)] = spread(ts)
            print(hs, ws, passes, spread(ts), flush=True)
    # for scale: the plain fp32 gather of the same 128 frames
    x = torch.randn(32, 4, 3, 224, 224).cuda()
    ts = []
    for _ in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.patch_gather(x, 16, 3)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    out["kernel_us_128frames_plain_fp32_passes3"] = spread(ts[3:])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
