"""Host side of the NLQ / MQ feature dumps (egovlp_amd/extract.py) on CPU tensors over the do-nothing HIP stand-in
(tests/mock_hip.py): window arithmetic, the census of C-ABI calls of a clip, the file formats, resuming, the text cache, and the
one-shot contract of SpaceTimeTransformer.set_input_eval_transform.  No numerics here: those are tests/test_gpu_extract.py and
tests/test_gpu_eval_transform.py."""
import collections
import os

import numpy as np
import pytest
import torch

from mock_hip import mock_hip

TINY_VIDEO = {"model": "SpaceTimeTransformer", "arch_config": "custom", "num_frames": 4, "pretrained": True, "time_init": "rand",
              "arch_kwargs": dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2)}
TINY_TEXT = {"model": "distilbert-base-uncased", "pretrained": True, "input": "text",
             "config": dict(vocab_size=30522, dim=128, n_layers=2, n_heads=2, hidden_dim=256)}
DIM = 64
GATHERS = ("egv_patch_gather", "egv_patch_gather_u8", "egv_patch_gather_u8_aug", "egv_patch_gather_u8_eval")


@pytest.fixture(scope="module")
def model():
    from egovlp_amd.model.model import FrozenInTime
    torch.manual_seed(0)
    return FrozenInTime(video_params=dict(TINY_VIDEO), text_params=dict(TINY_TEXT), projection_dim=DIM, projection="minimal",
                        load_checkpoint="").train()


def tokenizer(texts, return_tensors="pt", padding=True, truncation=True):
    """[CLS] word ids [SEP], padded with 0 -- the shape of a HF tokenizer's output"""
    rows = [[101] + [1000 + sum(map(ord, w)) % 5000 for w in t.split()] + [102] for t in texts]
    L = max(map(len, rows))
    ids = torch.tensor([r + [0] * (L - len(r)) for r in rows])
    mask = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows])
    return {"input_ids": ids, "attention_mask": mask}


def clip(n_frames, seed=0, h=45, w=80):
    return torch.randint(0, 256, (n_frames, 3, h, w), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_window_arithmetic(model):
    from egovlp_amd.extract import ClipFeatureExtractor
    ext = ClipFeatureExtractor(model, num_frames=4)
    w = ext.windows(3)
    assert w.dtype == torch.int32 and tuple(w.shape) == (0, 4)                     # F < T: no window
    w = ext.windows(39)
    assert w.dtype == torch.int32 and tuple(w.shape) == (9, 4)                     # 39 // 4, the last 3 frames dropped
    assert w.reshape(-1).tolist() == list(range(36))
    assert torch.equal(ext.windows(39, stride=4), w)
    w2 = ext.windows(39, stride=2)                                                 # starts 0, 2, ..., 34 (34 + 4 <= 39, 36 + 4 > 39)
    assert tuple(w2.shape) == (18, 4) and w2[:, 0].tolist() == list(range(0, 36, 2)) and w2[-1].tolist() == [34, 35, 36, 37]
    w7 = ext.windows(39, stride=7)                                                 # stride > T: sub-sampled windows
    assert w7[:, 0].tolist() == [0, 7, 14, 21, 28, 35] and w7[-1].tolist() == [35, 36, 37, 38]
    assert tuple(ext.windows(4).shape) == (1, 4) and tuple(ext.windows(4, stride=100).shape) == (1, 4)
    with pytest.raises(ValueError):
        ext.windows(39, stride=0)


def test_geometry_helper_restates_resize_and_center_crop():
    from egovlp_amd.data_loader.transforms import eval_transform_geometry
    assert eval_transform_geometry(256, 341) == (256, 341, 0, 42)                  # (341 - 256) / 2 = 42.5 -> 42 (half to even)
    assert eval_transform_geometry(270, 480) == (256, 455, 0, 100)                 # 99.5 -> 100
    assert eval_transform_geometry(480, 270) == (455, 256, 100, 0)
    assert eval_transform_geometry(180, 240) == (256, 341, 0, 42)
    assert eval_transform_geometry(45, 80, 40) == (40, 71, 0, 16)                  # 15.5 -> 16
    assert eval_transform_geometry(224, 224, 256) == (256, 256, 0, 0)


def test_video_features_census_one_fused_gather_per_window_batch(model):
    from egovlp_amd.extract import ClipFeatureExtractor
    frames = clip(39)
    with mock_hip() as calls:
        for batch, n_batches in ((2, 5), (4, 3), (32, 1)):
            ext = ClipFeatureExtractor(model, num_frames=4, batch=batch, center_crop=40, input_res=32)
            calls.clear()
            feats = ext.video_features(frames)
            c = collections.Counter(calls)
            assert tuple(feats.shape) == (9, DIM) and feats.dtype == torch.float32 and feats.device.type == "cpu"
            assert c["egv_patch_gather_u8_eval"] == n_batches, (batch, c)
            assert all(c[g] == 0 for g in GATHERS[:3]), c
        # the reference's tail: 9 windows -> 8 computed (two batches of 4), row 8 stays zero
        ext = ClipFeatureExtractor(model, num_frames=4, batch=4, center_crop=40, input_res=32, reference_tail=True)
        calls.clear()
        feats = ext.video_features(frames)
        assert collections.Counter(calls)["egv_patch_gather_u8_eval"] == 2 and bool((feats[8] == 0).all())
        # float frames = the loader's transformed output: the plain gather, nothing fused
        calls.clear()
        feats = ClipFeatureExtractor(model, num_frames=4, batch=4).video_features(torch.randn(39, 3, 32, 32), stride=2)
        c = collections.Counter(calls)
        assert tuple(feats.shape) == (18, DIM) and c["egv_patch_gather"] == 5 and c["egv_patch_gather_u8_eval"] == 0
        # a clip shorter than a window: no row, no call
        calls.clear()
        assert tuple(ext.video_features(clip(3)).shape) == (0, DIM) and not calls
    assert model.training                                                           # the previous mode is back


def test_extract_mq_files_resume_and_no_half_files(model, tmp_path):
    from egovlp_amd.extract import extract_mq
    loader = [{"video": clip(39, 1)[None], "meta": {"clip_uid": ["clip_a"]}},
              {"video": clip(17, 2)[None], "meta": {"clip_uid": ["clip_b"]}}]
    out = str(tmp_path / "mq")
    with mock_hip() as calls:
        written = extract_mq(model, loader, out, center_crop=40, input_res=32, log=lambda s: None)
        assert sorted(os.listdir(out)) == ["clip_a.pt", "clip_b.pt"]               # and no temporary file
        assert [os.path.basename(p) for p in written] == ["clip_a.pt", "clip_b.pt"]
        for name, rows in (("clip_a.pt", 9), ("clip_b.pt", 4)):
            t = torch.load(os.path.join(out, name))
            assert tuple(t.shape) == (rows, DIM) and t.dtype == torch.float32
        # both files exist: a second run touches no device
        calls.clear()
        assert extract_mq(model, loader, out, center_crop=40, input_res=32, log=lambda s: None) == []
        assert not calls
        # one file missing: only that clip is encoded
        os.remove(os.path.join(out, "clip_b.pt"))
        calls.clear()
        written = extract_mq(model, loader, out, center_crop=40, input_res=32, log=lambda s: None)
        assert [os.path.basename(p) for p in written] == ["clip_b.pt"]
        assert collections.Counter(calls)["egv_patch_gather_u8_eval"] == 1
        # a run that dies while writing leaves nothing under the final name and no temporary file
        os.remove(os.path.join(out, "clip_b.pt"))
        real_save = torch.save

        def dying_save(obj, f, *a, **k):
            f.write(b"half")
            raise KeyboardInterrupt

        torch.save = dying_save
        try:
            with pytest.raises(KeyboardInterrupt):
                extract_mq(model, loader, out, center_crop=40, input_res=32, log=lambda s: None)
        finally:
            torch.save = real_save
        assert sorted(os.listdir(out)) == ["clip_a.pt"]


def test_extract_nlq_video_and_text_dumps(model, tmp_path):
    from egovlp_amd.extract import extract_nlq
    out = str(tmp_path / "nlq")
    vloader = [{"video": clip(16, 3)[None], "meta": {"clip_uid": ["clip_c"]}}]
    queries = ["where is the red cup", "what did i put in the drawer before lunch", "where is the red cup", "who"]
    tloader = [{"text": [q]} for q in queries]
    with mock_hip() as calls:
        extract_nlq(model, vloader, tokenizer, out, "video", center_crop=40, input_res=32, log=lambda s: None)
        assert tuple(torch.load(os.path.join(out, "clip_c.pt")).shape) == (4, DIM)
        calls.clear()
        extract_nlq(model, tloader, tokenizer, out, "text")
        n_text_forwards = collections.Counter(calls)["egv_embed_fwd"]
        assert n_text_forwards == 3                                                 # the duplicate query is not encoded again
        cache = np.load(os.path.join(out, "sentence.npy"), allow_pickle=True).item()
        assert isinstance(cache, dict) and sorted(cache) == sorted(set(queries))
        assert all(tuple(v.shape) == (1, DIM) and v.device.type == "cpu" for v in cache.values())
        # token features: [CLS] / [SEP] / padding are cut per sentence, also inside one padded batch
        extract_nlq(model, [{"text": queries}], tokenizer, out, "text", token=True)
        cache = np.load(os.path.join(out, "sentence.npy"), allow_pickle=True).item()
        assert sorted(cache) == sorted(set(queries))
        for q in set(queries):
            assert tuple(cache[q].shape) == (len(q.split()), DIM), q
        with pytest.raises(ValueError):
            extract_nlq(model, tloader, tokenizer, out, "audio")
    assert sorted(os.listdir(out)) == ["clip_c.pt", "sentence.npy"]


def test_set_input_eval_transform_is_one_shot_and_exclusive(model):
    net = model.video_model
    u8 = clip(8).view(2, 4, 3, 45, 80)
    with mock_hip() as calls:
        net.set_input_eval_transform(center_crop=40, out_res=32)
        net.forward_features(u8)
        assert calls.count("egv_patch_gather_u8_eval") == 1
        calls.clear()
        net.forward_features(torch.randn(2, 4, 3, 32, 32))                         # consumed: the next forward is the plain one
        assert calls.count("egv_patch_gather_u8_eval") == 0 and calls.count("egv_patch_gather") == 1
        # a frame bank with a table: [F, C, Hs, Ws] in, b x T from the table
        calls.clear()
        net.set_input_eval_transform(40, 32, frame_index=torch.tensor([[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7]]))
        assert tuple(net.forward_features(clip(8)).shape) == (3, 128) and calls.count("egv_patch_gather_u8_eval") == 1
        # a host table that leaves the bank is refused
        net.set_input_eval_transform(40, 32, frame_index=torch.tensor([[0, 1, 2, 8]]))
        with pytest.raises(ValueError):
            net.forward_features(clip(8))
        net.set_input_eval_transform(40, 32, frame_index=torch.tensor([[-1, 1, 2, 3]]))
        with pytest.raises(ValueError):
            net.forward_features(clip(8))
        # float frames are refused (and the request is consumed by the refusal)
        net.set_input_eval_transform(40, 32)
        with pytest.raises(ValueError):
            net.forward_features(torch.randn(2, 4, 3, 45, 80))
        calls.clear()
        net.forward_features(torch.randn(2, 4, 3, 32, 32))
        assert calls.count("egv_patch_gather") == 1
        # not combinable with the train augmentation, in either order
        net.set_input_eval_transform(40, 32)
        with pytest.raises(ValueError):
            net.set_input_augmentation(torch.tensor([[0, 0, 40, 40, 0], [0, 0, 40, 40, 1]]))
        net.forward_features(u8)
        net.set_input_augmentation(torch.tensor([[0, 0, 40, 40, 0], [0, 0, 40, 40, 1]]), out_res=32)
        with pytest.raises(ValueError):
            net.set_input_eval_transform(40, 32)
        with pytest.raises(ValueError):
            net.forward_features(u8)                   # consumes the augmentation (its boxes must live on the device: refused here)
        with pytest.raises(ValueError):
            net.set_input_eval_transform(40, 32, frame_index=torch.tensor([0, 1, 2, 3]))       # not [b, T]
        with pytest.raises(ValueError):
            net.set_input_eval_transform(40, 32, frame_index=torch.tensor([[0.0, 1.0, 2.0, 3.0]]))


def test_ops_wrapper_refuses_what_it_can_see():
    from egovlp_amd import ops
    bank = clip(8)
    with mock_hip() as calls:
        pl = ops.patch_gather_eval(bank, None, 4, 16, 3, 40, 32)
        assert (pl.rows, pl.cols) == (8 * 4, 768) and pl.lo is not None
        pl = ops.patch_gather_eval(bank, torch.tensor([3, 3, 0, 7], dtype=torch.int32), 4, 14, 1, 40, 28)
        assert (pl.rows, pl.cols) == (4 * 4, 640) and pl.lo is None                # K = 588 padded to the 64-deep k-tile
        assert calls.count("egv_patch_gather_u8_eval") == 2
        calls.clear()
        for bad in (torch.tensor([0, 1, 2, 8]), torch.tensor([0, -1, 2, 3]), torch.tensor([0, 1, 2]), torch.tensor([0.0, 1.0, 2.0, 3.0]),
                    torch.zeros(0, dtype=torch.int32), [0, 1, 2, 3]):
            with pytest.raises(ValueError):
                ops.patch_gather_eval(bank, bad, 4, 16, 3, 40, 32)
        with pytest.raises(ValueError):
            ops.patch_gather_eval(bank.float(), None, 4, 16, 3, 40, 32)
        with pytest.raises(ValueError):
            ops.patch_gather_eval(bank, None, 3, 16, 3, 40, 32)                    # 8 frames are not windows of 3
        assert not calls
