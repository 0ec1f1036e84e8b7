"""The NLQ / MQ feature-dump flow (egovlp_amd/extract.py) on a real MI355X (`pytest -m gpu`): window features from decoded uint8
frames through the fused val / test transform against the reference-shaped loop (host transform -> reshape to [-1, 4, C, H, W] ->
compute_video four windows at a time, run/test_nlq.py:71-88) and against the CPU oracle, at the project's parity bar (rel-L2 1e-3,
tests/test_gpu_model.py PARITY); query features of a padded batch against per-sentence calls; and the sync census of the window
loop."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from egovlp_amd.data_loader.transforms import eval_transform_geometry  # noqa: E402
from egovlp_amd.synth import synth_batch, synth_state_dict  # noqa: E402
from oracle import egovlp_oracle as O  # noqa: E402

PARITY = 1e-3
TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
N_FRAMES = 4 * 9 + 3


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def host_transform(u8, S, R):
    """init_video_transform_dict()['test'] on [N, C, Hs, Ws] uint8 frames -> fp32 [N, C, R, R]: what the reference loader yields"""
    from egovlp_amd import ops
    H1, W1, top, left = eval_transform_geometry(u8.shape[-2], u8.shape[-1], S)
    x = u8.float() / 255
    x = F.interpolate(x, size=(H1, W1), mode="bilinear", align_corners=False)
    x = x[:, :, top:top + S, left:left + S]
    x = F.interpolate(x, size=(R, R), mode="bilinear", align_corners=False)
    return (x - torch.tensor(ops.IMAGENET_MEAN).view(1, 3, 1, 1)) / torch.tensor(ops.IMAGENET_STD).view(1, 3, 1, 1)


def reference_loop(model, windows5d):
    """run/test_nlq.py:76-88 with every window computed: compute_video four windows at a time, a host copy per batch"""
    outs = []
    with torch.no_grad():
        for s in range(0, windows5d.shape[0], 4):
            outs.append(model.compute_video(windows5d[s:s + 4].cuda()).float().cpu())
    return torch.cat(outs)


@pytest.fixture(scope="module")
def tiny():
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m = FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection_dim=64, projection="minimal",
                     load_checkpoint="")
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=4), strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def full():
    from egovlp_amd.model.model import FrozenInTime
    from egovlp_amd.ops import Precision
    Precision.set("bf16x3")
    m = FrozenInTime(video_params={"model": "SpaceTimeTransformer", "arch_config": "base_patch16_224", "num_frames": 4,
                                   "pretrained": True, "time_init": "rand"},
                     text_params={"model": "distilbert-base-uncased", "pretrained": True, "input": "text"},
                     projection="minimal", load_checkpoint="")
    sd = synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict(sd, strict=True)
    m.text_model.set_dropout(0.0, 0.0)
    return m.cuda().eval(), sd


@pytest.fixture(scope="module")
def tiny_clip():
    return torch.randint(0, 256, (N_FRAMES, 3, 45, 80), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)


def test_window_features_match_the_reference_shaped_loop(tiny, tiny_clip):
    from egovlp_amd.extract import ClipFeatureExtractor
    S, R = 40, 32
    host = host_transform(tiny_clip, S, R)                                          # [39, 3, 32, 32]
    want = reference_loop(tiny, host[:36].reshape(-1, 4, 3, R, R))
    assert tuple(want.shape) == (9, 64)
    for batch in (2, 4, 32):                                                        # 32: one ragged batch of 9
        ext = ClipFeatureExtractor(tiny, num_frames=4, batch=batch, center_crop=S, input_res=R)
        for where, frames in (("host", tiny_clip), ("pinned", tiny_clip.pin_memory()), ("device", tiny_clip.cuda())):
            got = ext.video_features(frames)
            assert tuple(got.shape) == (9, 64) and got.dtype == torch.float32 and got.device.type == "cpu"
            r = rel(got, want)
            print("extract tiny: batch %2d frames on %-6s rel %.2e" % (batch, where, r))
            assert r < PARITY, (batch, where, r)
        for where, frames in (("host", host), ("device", host.cuda())):             # float = already transformed: the plain path
            r = rel(ext.video_features(frames), want)
            print("extract tiny: batch %2d float frames on %-6s rel %.2e" % (batch, where, r))
            assert r < PARITY, (batch, where, r)
    assert not tiny.training
    tiny.train()
    ClipFeatureExtractor(tiny, batch=4, center_crop=S, input_res=R).video_features(tiny_clip)
    assert tiny.training                                                            # the previous mode is restored
    tiny.eval()


def test_reference_tail_zeroes_exactly_the_rows_the_reference_leaves(tiny, tiny_clip):
    from egovlp_amd.extract import ClipFeatureExtractor
    S, R = 40, 32
    full_rows = ClipFeatureExtractor(tiny, batch=4, center_crop=S, input_res=R).video_features(tiny_clip)
    tail = ClipFeatureExtractor(tiny, batch=4, center_crop=S, input_res=R, reference_tail=True).video_features(tiny_clip)
    assert tuple(tail.shape) == (9, 64)
    assert bool((tail[8] == 0).all()) and bool((full_rows[8] != 0).any())
    assert rel(tail[:8], full_rows[:8]) < PARITY and bool((tail[:8].abs().sum(1) > 0).all())


def test_strided_windows_equal_the_loop_over_gathered_windows(tiny, tiny_clip):
    from egovlp_amd.extract import ClipFeatureExtractor
    S, R = 40, 32
    ext = ClipFeatureExtractor(tiny, batch=4, center_crop=S, input_res=R)
    idx = ext.windows(N_FRAMES, stride=2)
    assert tuple(idx.shape) == (18, 4)
    host = host_transform(tiny_clip, S, R)
    want = reference_loop(tiny, host[idx.reshape(-1).long()].reshape(18, 4, 3, R, R))
    for where, frames in (("host", tiny_clip), ("device", tiny_clip.cuda()), ("float", host)):
        got = ext.video_features(frames, stride=2)
        r = rel(got, want)
        print("extract tiny stride 2: %-6s rel %.2e" % (where, r))
        assert tuple(got.shape) == (18, 64) and r < PARITY, (where, r)


def test_real_geometry_matches_the_cpu_oracle(full):
    from egovlp_amd.extract import ClipFeatureExtractor
    m, sd = full
    frames = torch.randint(0, 256, (20, 3, 256, 341), generator=torch.Generator().manual_seed(22), dtype=torch.uint8)
    got = ClipFeatureExtractor(m, num_frames=4, batch=32).video_features(frames)
    assert tuple(got.shape) == (5, 256)
    host = host_transform(frames, 256, 224).reshape(5, 4, 3, 224, 224)
    with torch.no_grad():
        v = O.video_encoder(host, sd, O.VideoCfg(num_frames=4))
        want = F.linear(v, sd["vid_proj.0.weight"], sd["vid_proj.0.bias"])
    r = rel(got, want)
    print("extract base_patch16_224, 256 x 341 frames, 5 windows: rel %.2e vs the CPU oracle" % r)
    assert r < PARITY, r


def test_text_features_of_a_padded_batch_match_per_sentence_calls(full):
    from egovlp_amd.extract import ClipFeatureExtractor
    m, _ = full
    ext = ClipFeatureExtractor(m)
    text = synth_batch(4, T=4, L=24, seed=31, ragged=True)["text"]
    words = text["attention_mask"].sum(1).tolist()
    assert len(set(words)) > 1, words                                               # sentences of different lengths
    for token in (False, True):
        batch = ext.text_features(text, token=token)
        assert len(batch) == 4
        for i, n in enumerate(words):
            one = ext.text_features({k: v[i:i + 1, :n] for k, v in text.items()}, token=token)[0]
            assert tuple(batch[i].shape) == ((n - 2, 256) if token else (256,)) and batch[i].device.type == "cpu"
            r = rel(batch[i], one)
            print("extract text token=%s sentence %d (%d words): rel %.2e" % (token, i, n, r))
            assert r < PARITY, (token, i, r)
    # token rows are compute_text_tokens(...)[i][1 : num_words - 1]
    with torch.no_grad():
        tok = m.compute_text_tokens({k: v.cuda() for k, v in text.items()}).float().cpu()
    got = ext.text_features(text, token=True)
    for i, n in enumerate(words):
        assert rel(got[i], tok[i, 1:n - 1]) < 1e-6


def test_no_host_sync_inside_the_window_loop(tiny, tiny_clip, monkeypatch):
    """The call census of one clip (5 window batches): ONE Tensor.cpu() -- the copy of the finished [W, dim] matrix -- and no
    .item() / .tolist() / synchronize of the device, a stream or an event."""
    from egovlp_amd.extract import ClipFeatureExtractor
    ext = ClipFeatureExtractor(tiny, batch=2, center_crop=40, input_res=32)
    frames = tiny_clip.pin_memory()
    ext.video_features(frames)                                                      # warm: weight planes, workspaces, the copy stream
    census = {}

    def count(owner, name):
        real = getattr(owner, name)

        def wrapped(*a, **k):
            census[name] = census.get(name, 0) + 1
            return real(*a, **k)

        monkeypatch.setattr(owner, name, wrapped)

    for owner, name in ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"),
                        (torch.cuda, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
        count(owner, name)
    got = ext.video_features(frames)
    monkeypatch.undo()
    print("extract sync census of a 5-batch clip:", census)
    assert census == {"cpu": 1}, census
    assert tuple(got.shape) == (9, 64)
