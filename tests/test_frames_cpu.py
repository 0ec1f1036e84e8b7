"""More than 16 frames, the parts that need no GPU (modules are parameter containers until `forward`): the bound of the time attention
(64 frames, csrc/attn_time_long.hip) as the model and `ops` state it, and a 16-frame checkpoint's temporal embedding inflated to 32 frames.
Values on the device: tests/test_gpu_attn_time_long.py, tests/test_gpu_frames_model.py."""
import pytest
import torch
import torch.nn.functional as F

TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
TINY = dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)


def test_the_bound_is_64_frames():
    from egovlp_amd import ops
    from egovlp_amd.model.video_transformer import SpaceTimeTransformer
    assert ops.TIME_ATTN_MAX_FRAMES == 64
    m = SpaceTimeTransformer(num_frames=64, **TINY)
    assert m.temporal_embed.shape == (1, 64, 128) and m.num_frames == 64
    with pytest.raises(ValueError, match="64"):
        SpaceTimeTransformer(num_frames=65, **TINY)


@pytest.mark.parametrize("arch", ["custom", "base_patch16_224"])
def test_num_frames_of_video_params_reaches_the_tower_and_its_bound(arch):
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": arch, "num_frames": 65, "pretrained": True, "time_init": "zeros"}
    if arch == "custom":
        vp["arch_kwargs"] = dict(TINY)
    with pytest.raises(ValueError, match="64"):
        FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
    if arch == "custom":
        m = FrozenInTime(video_params={**vp, "num_frames": 32}, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="")
        assert m.video_model.num_frames == 32 and m.video_model.temporal_embed.shape == (1, 32, 128)


@pytest.mark.parametrize("fix", ["zeros", "interp", "bilinear"])
def test_a_16_frame_checkpoint_inflates_to_32_frames(fix):
    """`_inflate_positional_embeds` (the reference's load_temporal_fix rules, model/model.py:145-187) against F.interpolate written
    here: 'zeros' keeps the 16 rows and appends zero rows, 'interp' is nearest (every checkpoint frame twice), 'bilinear' is bilinear with
    align_corners=True, both over the (frames, channels) plane."""
    from egovlp_amd.model.model import FrozenInTime
    vp = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 32, "pretrained": True, "time_init": "zeros",
          "arch_kwargs": dict(TINY)}
    m = FrozenInTime(video_params=vp, text_params=dict(TINY_TEXT), projection="minimal", load_checkpoint="", load_temporal_fix=fix)
    old = torch.randn(1, 16, 128, generator=torch.Generator().manual_seed(3))
    sd = {"video_model.temporal_embed": old.clone(), "video_model.pos_embed": torch.zeros(1, 5, 128)}
    new = m._inflate_positional_embeds(sd)["video_model.temporal_embed"]
    assert new.shape == (1, 32, 128)
    if fix == "zeros":
        want = torch.cat([old, torch.zeros(1, 16, 128)], dim=1)
    elif fix == "interp":
        want = F.interpolate(old[None], size=(32, 128), mode="nearest")[0]
        assert torch.equal(want, old.repeat_interleave(2, dim=1))
    else:
        want = F.interpolate(old[None], size=(32, 128), mode="bilinear", align_corners=True)[0]
    assert torch.equal(new, want)
    if fix == "bilinear":       # the end frames are kept, the ones between are blends of their two neighbours
        assert torch.allclose(new[0, 0], old[0, 0]) and torch.allclose(new[0, -1], old[0, -1])
