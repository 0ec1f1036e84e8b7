"""Device-side counterpart of the reference's TRAIN transform (data_loader/transforms.py:14-19):

    RandomResizedCrop(input_res, scale=randcrop_scale) -> RandomHorizontalFlip()
        -> ColorJitter(brightness=color_jitter[0], saturation=color_jitter[1], hue=color_jitter[2]) -> Normalize(mean, std)

The reference runs it on the host, on float frames, and ships 4 x 3 x 224 x 224 floats per clip to the GPU.  Here only the
RANDOM DRAWS stay on the host -- `train_transform_params` returns, per clip, the crop box and the flip flag -- and the pixels
are produced by `egv_patch_gather_u8_aug` straight from the decoded uint8 clip inside the patch gather of the video encoder
(`SpaceTimeTransformer.set_input_augmentation`).  One box per clip, as in the reference (the transform is applied to the
[T, C, H, W] tensor as a whole).

The colour jitter is the identity in the pre-training config (`color_jitter` = (0, 0, 0)) and a real stage in fine-tuning
configs such as (0.4, 0.4, 0.1).  `train_transform_params_color` draws, next to the boxes, one row per clip of (brightness
factor, saturation factor, hue shift, op code) in torchvision 0.13's order -- `randperm(4)` over (brightness, contrast,
saturation, hue), then the factors of the enabled ops -- and `egv_patch_gather_u8_aug_color` applies the ops between the flip
and Normalize (`set_input_augmentation(boxes, out_res, color)`).  A scalar b means the range [max(0, 1 - b), 1 + b] for
brightness and saturation and [-h, h], 0 <= h <= 0.5, for hue; a (min, max) pair is taken as it is; a range that collapses onto
the identity value disables the op (skipped, not run with factor 1: the hue round trip is not the identity in fp32).  Contrast
cannot be set through the reference's `init_transform_dict` and is skipped wherever it lands in the permutation.

Mixup / CutMix (an extension, timm's `Mixup` restated; the reference mixes nothing) keeps the same division of labour: `mix_params`
draws, per clip, the partner, the op, the cutmix box and lam, and the patch gather blends or selects the pixels of the two transformed
clips (`SpaceTimeTransformer.set_input_mix`, `egv_patch_gather_mix` / `egv_patch_gather_u8_aug_mix`).

The 'val' / 'test' transform (data_loader/transforms.py:49-60) is deterministic:

    Resize(center_crop) -> CenterCrop(center_crop) -> Resize(input_res) -> Normalize(mean, std)

It has a device-side counterpart too: `egv_patch_gather_u8_eval` computes it from decoded uint8 frames inside the patch gather
(`SpaceTimeTransformer.set_input_eval_transform`, `egovlp_amd.extract`).  Its only host half is arithmetic on sizes,
`eval_transform_geometry`: the size of the first resize and the offsets of the centre crop.

The box sampling restates torchvision 0.13's `RandomResizedCrop.get_params` (third-party, pinned in the reference's
environment.yml): ten tries of (area fraction ~ U(scale), log-aspect ~ U(log ratio)), then the central fallback crop.
"""
import math

import torch


def random_resized_crop_box(height, width, scale=(0.5, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * float(torch.empty(1).uniform_(scale[0], scale[1], generator=generator))
        aspect = math.exp(float(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, (1,), generator=generator))
            j = int(torch.randint(0, width - w + 1, (1,), generator=generator))
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def train_transform_params(batch, height, width, randcrop_scale=(0.5, 1.0), flip_p=0.5, generator=None):
    """-> int32 [batch, 5] (top, left, h, w, flip): the host half of the fused train transform."""
    rows = []
    for _ in range(batch):
        i, j, h, w = random_resized_crop_box(height, width, randcrop_scale, generator=generator)
        flip = int(float(torch.rand(1, generator=generator)) < flip_p)
        rows.append([i, j, h, w, flip])
    return torch.tensor(rows, dtype=torch.int32)


def _jitter_range(value, name, center, bound, clip_first_on_zero=True):
    """torchvision 0.13 `ColorJitter._check_input`: -> (min, max), or None where the range is the identity value alone."""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"color_jitter: a scalar {name} is non-negative")
        lo, hi = center - float(value), center + float(value)
        if clip_first_on_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise TypeError(f"color_jitter: {name} is a number or a (min, max) pair")
    if not bound[0] <= lo <= hi <= bound[1]:
        raise ValueError(f"color_jitter: {name} values lie in {bound}, got ({lo}, {hi})")
    return None if lo == hi == center else (lo, hi)


def train_transform_params_color(batch, height, width, randcrop_scale, color_jitter, flip_p=0.5, generator=None):
    """-> (boxes int32 [batch, 5], color float32 [batch, 4] or None): the host half of the fused train transform with
    ColorJitter(brightness=color_jitter[0], saturation=color_jitter[1], hue=color_jitter[2]).  Per clip, in this order: the box,
    the flip, `randperm(4)`, then the brightness, saturation and hue draws of the enabled ops (torchvision's `get_params`).
    color[b] = (brightness factor, saturation factor, hue shift, code); code is three base-4 digits stored exactly in the float,
    the first applied op lowest (0 nothing, 1 brightness, 2 saturation, 3 hue).  With every op disabled: color is None and the
    boxes are those of `train_transform_params` from the same generator state."""
    if len(color_jitter) != 3:
        raise ValueError("color_jitter: (brightness, saturation, hue)")
    ranges = (_jitter_range(color_jitter[0], "brightness", 1.0, (0.0, float("inf"))),
              _jitter_range(color_jitter[1], "saturation", 1.0, (0.0, float("inf"))),
              _jitter_range(color_jitter[2], "hue", 0.0, (-0.5, 0.5), clip_first_on_zero=False))
    if all(r is None for r in ranges):
        return train_transform_params(batch, height, width, randcrop_scale, flip_p, generator), None
    digit = {0: 1, 2: 2, 3: 3}                        # randperm index (1 = contrast: skipped) -> op digit
    identity = (1.0, 1.0, 0.0)
    boxes, color = [], []
    for _ in range(batch):
        i, j, h, w = random_resized_crop_box(height, width, randcrop_scale, generator=generator)
        flip = int(float(torch.rand(1, generator=generator)) < flip_p)
        boxes.append([i, j, h, w, flip])
        order = torch.randperm(4, generator=generator).tolist()
        factors = [identity[k] if r is None else float(torch.empty(1).uniform_(r[0], r[1], generator=generator))
                   for k, r in enumerate(ranges)]
        code = shift = 0
        for fn in order:
            d = digit.get(fn, 0)
            if d and ranges[d - 1] is not None:
                code |= d << shift
                shift += 2
        color.append(factors + [float(code)])
    return torch.tensor(boxes, dtype=torch.int32), torch.tensor(color, dtype=torch.float32)


def eval_transform_geometry(height, width, center_crop=256):
    """-> (H1, W1, top, left) of the val / test transform on a height x width frame: `Resize(center_crop)` takes the short side
    to center_crop and the long side to int(center_crop * long / short) (torchvision 0.13 `_compute_resized_output_size`), and
    `CenterCrop(center_crop)` then cuts rows top .. top + center_crop and columns left .. left + center_crop with
    int(round((size - center_crop) / 2.0)) offsets (`functional.center_crop`; Python's round: halves go to the even neighbour)."""
    S = int(center_crop)
    if height < 1 or width < 1 or S < 1:
        raise ValueError("eval_transform_geometry: sizes are positive")
    if height <= width:
        H1, W1 = S, int(S * width / height)
    else:
        H1, W1 = int(S * height / width), S
    return H1, W1, int(round((H1 - S) / 2.0)), int(round((W1 - S) / 2.0))


def _beta(alpha, generator):
    """One draw of Beta(alpha, alpha) from `generator`: X / (X + Y) with X, Y ~ Gamma(alpha, 1)."""
    g = torch._standard_gamma(torch.full((2,), float(alpha), dtype=torch.float64), generator=generator)
    total = float(g[0] + g[1])
    return float(g[0]) / total if total > 0.0 else 0.5


def _mix_draw(height, width, mixup_alpha, cutmix_alpha, prob, switch_prob, generator):
    """One decision of timm's Mixup -> (op, lam, y0, y1, x0, x1)."""
    if not float(torch.rand(1, generator=generator)) < prob:
        return 0, 1.0, 0, 0, 0, 0
    if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
        cut = float(torch.rand(1, generator=generator)) < switch_prob
    else:
        cut = cutmix_alpha > 0.0
    lam = _beta(cutmix_alpha if cut else mixup_alpha, generator)
    if not cut:
        return 1, lam, 0, 0, 0, 0
    ratio = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(height * ratio), int(width * ratio)
    cy = int(torch.randint(0, height, (1,), generator=generator))
    cx = int(torch.randint(0, width, (1,), generator=generator))
    y0, y1 = min(max(cy - cut_h // 2, 0), height), min(max(cy + cut_h // 2, 0), height)
    x0, x1 = min(max(cx - cut_w // 2, 0), width), min(max(cx + cut_w // 2, 0), width)
    return 2, 1.0 - (y1 - y0) * (x1 - x0) / float(height * width), y0, y1, x0, x1


def mix_params(batch, height, width, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode='batch', generator=None):
    """The host half of Mixup / CutMix inside the patch gather (an extension: timm's `Mixup` restated, the recipe of the VideoMAE /
    MViT fine-tunes; the reference mixes nothing) -> (mix_idx int32 [batch, 6], mix_lam float32 [batch]), or (None, None) when it
    is off (both alphas 0, or prob 0): every caller then makes the calls it made before.
    mix_idx[b] = (partner, op, y0, y1, x0, x1): op 0 nothing, 1 mixup, 2 cutmix; the box covers rows [y0, y1) and columns [x0, x1)
    of the OUTPUT frame of `height` x `width` pixels (input_res x input_res under the fused train transform), the same in every
    frame of the clip.  With probability `prob` the batch (mode 'batch': one op, one lam, one box for all clips) or the clip (mode
    'elem': its own draw) is mixed; cutmix is chosen with probability `switch_prob` when both alphas are > 0; lam ~ Beta(alpha,
    alpha); the cutmix box has extents int(height * cut), int(width * cut), cut = sqrt(1 - lam), a centre uniform over the frame,
    is clipped to the frame, and lam is then REPLACED by 1 - area / (height * width) of the clipped box.  The partner is the flipped
    batch, batch - 1 - b (the middle clip of an odd batch pairs with itself); rows that are not mixed are (b, 0, 0, 0, 0, 0), lam 1.
    The target of clip b is lam * target[b] + (1 - lam) * target[partner] (`classification_step(mix=...)`)."""
    if mode not in ('batch', 'elem'):
        raise ValueError("mix_params: mode is 'batch' or 'elem'")
    if batch < 1 or height < 1 or width < 1:
        raise ValueError("mix_params: batch, height and width are positive")
    if mixup_alpha < 0.0 or cutmix_alpha < 0.0 or not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
        raise ValueError("mix_params: alphas are non-negative, prob and switch_prob lie in [0, 1]")
    if (mixup_alpha == 0.0 and cutmix_alpha == 0.0) or prob == 0.0:
        return None, None
    draws = [_mix_draw(height, width, mixup_alpha, cutmix_alpha, prob, switch_prob, generator)
             for _ in range(batch if mode == 'elem' else 1)]
    rows, lams = [], []
    for b in range(batch):
        op, lam, y0, y1, x0, x1 = draws[b if mode == 'elem' else 0]
        rows.append([batch - 1 - b if op else b, op, y0, y1, x0, x1])
        lams.append(lam)
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(lams, dtype=torch.float32)
