"""NLQ / MQ feature dumps -- the bodies of the reference's run/test_nlq.py and run/test_mq.py.

The reference encodes a whole clip in consecutive 4-frame windows with `compute_video` and writes the [windows, projection_dim]
matrix as `<clip_uid>.pt`; the queries go to `sentence.npy`, a dict raw text -> embedding (or token embeddings).  VSLNet (NLQ) and
VSGN (MQ) train on these files.  Here the same files are produced with the clip kept as DECODED uint8 frames:

  * the val / test transform (Resize -> CenterCrop -> Resize -> Normalize) runs inside the patch gather
    (`egv_patch_gather_u8_eval`, `SpaceTimeTransformer.set_input_eval_transform`): no fp32 clip exists on the host or the device;
  * a window is a row of a frame table, so overlapping (stride < T) or sub-sampled windows and a ragged last batch copy nothing;
  * `batch` windows run per forward, the features stay on the device and come back in ONE copy per clip (the reference runs four
    windows per forward and copies -- synchronises -- after each);
  * host frames are uploaded in window batches on a copy stream, the upload of batch i + 1 under the forward of batch i.

Data loading and video decoding are the caller's (the reference's loader, or any decoder that yields uint8 frames).
"""
from __future__ import annotations

import os

import numpy as np
import torch

REFERENCE_BATCH = 4          # run/test_nlq.py:78, run/test_mq.py:76: windows per compute_video call of the reference


def _core(model):
    return getattr(model, "module", model)


class ClipFeatureExtractor:
    """Window-level video features and query features of one model.

    num_frames: frames per window (T of the video encoder call).  batch: windows per forward.  center_crop / input_res: the two
    sizes of the val / test transform.  reference_tail: the reference loop runs `windows // 4` batches of four and leaves the last
    `windows % 4` rows of its output at their initial zeros (run/test_nlq.py:76-88); True reproduces those zero rows (rows >=
    4 * (windows // 4)) bit for bit, the default (False) computes every window."""

    def __init__(self, model, num_frames=4, batch=32, center_crop=256, input_res=224, reference_tail=False):
        if num_frames < 1 or batch < 1:
            raise ValueError("ClipFeatureExtractor: num_frames and batch are positive")
        self.model = model
        self.num_frames, self.batch = int(num_frames), int(batch)
        self.center_crop, self.input_res = int(center_crop), int(input_res)
        self.reference_tail = bool(reference_tail)
        self._copy_stream = None

    # ------------------------------------------------------------------------------------------------------------ windows
    def window_starts(self, n_frames, stride=None):
        T = self.num_frames
        stride = T if stride is None else int(stride)
        if stride < 1:
            raise ValueError("windows: stride is a positive number of frames")
        return list(range(0, n_frames - T + 1, stride))

    def windows(self, n_frames, stride=None):
        """-> int32 [W, T]: the frame numbers of every window of an n_frames clip.  stride=None: the reference's n_frames // T
        consecutive windows (the trailing n_frames % T frames are dropped, run/test_nlq.py:72); stride s: windows start at
        0, s, 2s, ... while start + T <= n_frames."""
        starts = torch.tensor(self.window_starts(n_frames, stride), dtype=torch.int32)
        return starts.view(-1, 1) + torch.arange(self.num_frames, dtype=torch.int32).view(1, -1)

    # ------------------------------------------------------------------------------------------------------------- video
    def _device(self):
        return next(_core(self.model).parameters()).device

    def _dim(self):
        core = _core(self.model)
        proj = core.vid_proj
        return core.video_model.embed_dim if isinstance(proj, torch.nn.Identity) else proj[0].out_features

    def video_features(self, frames, stride=None):
        """frames [F, C, Hs, Ws] of one clip -> fp32 [W, projection_dim] on the CPU, row w = compute_video of window w.

        uint8 frames (decoded, on the host or the device) go through the fused val / test transform; floating-point frames
        [F, C, input_res, input_res] are taken as the output of the reference loader's transform and go through the plain path.
        Runs under no_grad with the model in eval mode (the previous mode is restored).  Nothing in the loop waits for the
        device: features accumulate there and leave in one copy.  Host frames overlap their upload with the previous forward
        when they are in pinned memory.  With reference_tail=True rows >= 4 * (W // 4) are the reference's zeros and are not
        computed; by default every row is computed."""
        if frames.dim() != 4:
            raise ValueError("video_features: frames of one clip are [F, C, H, W]")
        fused = frames.dtype == torch.uint8
        if not fused and not frames.is_floating_point():
            raise ValueError("video_features: decoded uint8 frames or transformed floating-point frames")
        T, core = self.num_frames, _core(self.model)
        starts = self.window_starts(frames.shape[0], stride)
        W = len(starts)
        run = W // REFERENCE_BATCH * REFERENCE_BATCH if self.reference_tail else W
        dev = self._device()
        out = torch.zeros((W, self._dim()), dtype=torch.float32, device=dev)
        if run == 0:
            return out.cpu()
        on_gpu = dev.type == "cuda"
        table = self.windows(frames.shape[0], stride).to(dev)                      # [W, T], the only upload besides the frames
        spans = [(s, min(s + self.batch, run)) for s in range(0, run, self.batch)]
        consecutive = (stride is None or int(stride) == T)
        if on_gpu and not frames.is_cuda and self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        main = torch.cuda.current_stream(dev) if on_gpu else None
        done = []                                                                   # event behind the forward of every batch

        def stage(k):
            """frames lo .. hi of window batch k on the device (+ the event of their upload)"""
            s, e = spans[k]
            lo, hi = starts[s], starts[e - 1] + T
            if frames.device == dev:
                return frames[lo:hi], lo, None
            if not on_gpu:
                return frames[lo:hi].to(dev), lo, None
            cp = self._copy_stream
            if k >= 2:
                cp.wait_event(done[k - 2])                                          # two staged batches at a time, no more
            with torch.cuda.stream(cp):
                chunk = frames[lo:hi].to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cp)
            return chunk, lo, ev

        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                core.exec_ctx.begin_step()
                nxt = stage(0)
                for k, (s, e) in enumerate(spans):
                    chunk, lo, ev = nxt
                    if k + 1 < len(spans):
                        nxt = stage(k + 1)                                          # uploads under the forward below
                    if ev is not None:
                        main.wait_event(ev)
                        chunk.record_stream(main)
                    if fused:
                        core.video_model.set_input_eval_transform(self.center_crop, self.input_res, frame_index=table[s:e] - lo)
                        feats = self.model.compute_video(chunk)
                    else:
                        if consecutive:
                            clips = chunk.reshape(e - s, T, *chunk.shape[1:])
                        else:
                            clips = chunk.index_select(0, (table[s:e] - lo).reshape(-1).long()).view(e - s, T, *chunk.shape[1:])
                        feats = self.model.compute_video(clips.float())
                    out[s:e].copy_(feats)
                    if on_gpu:
                        d = torch.cuda.Event()
                        d.record(main)
                        done.append(d)
                return out.cpu()                                                    # the one device-to-host copy of the clip
        finally:
            self.model.train(was_training)

    # -------------------------------------------------------------------------------------------------------------- text
    def text_features(self, tokenized, token=False):
        """tokenized: the tokenizer's output for a (padded) batch of sentences, `input_ids` / `attention_mask` [B, L].
        -> a list of B CPU tensors.  token=False: the sentence embedding [dim] (`compute_text`).  token=True: the embeddings of
        the sentence's own tokens, [num_words_i - 2, dim] = compute_text_tokens(...)[i][1 : num_words_i - 1] with num_words_i the
        attention-mask sum (run/test_nlq.py:103-106: [CLS] and [SEP] are cut off, padding never enters)."""
        dev = self._device()
        mask_host = tokenized["attention_mask"].cpu()
        text = {k: v.to(dev) for k, v in tokenized.items()}
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                _core(self.model).exec_ctx.begin_step()
                emb = (self.model.compute_text_tokens(text) if token else self.model.compute_text(text)).float().cpu()
        finally:
            self.model.train(was_training)
        if not token:
            return [emb[i].clone() for i in range(emb.shape[0])]
        words = mask_host.sum(dim=1).tolist()
        return [emb[i, 1:max(int(n) - 1, 1)].clone() for i, n in enumerate(words)]


def _atomic_write(path, write):
    """write(file object) into a temporary neighbour of `path`, then rename: an interrupted run leaves no file under the final
    name (which a later run would take for finished work)."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _clip_uid(data):
    uid = data["meta"]["clip_uid"]
    return uid if isinstance(uid, str) else uid[0]


def _dump_videos(ext, data_loader, save_dir, stride, log):
    os.makedirs(save_dir, exist_ok=True)
    written = []
    for data in data_loader:
        uid = _clip_uid(data)
        path = os.path.join(save_dir, uid + ".pt")
        if os.path.exists(path):                       # resume: before any device work (run/test_mq.py:65-67)
            log(f"{uid} is already.")
            continue
        video = data["video"]
        frames = video[0] if video.dim() == 5 else video           # the loader's batch of one clip: [1, F, C, H, W]
        feats = ext.video_features(frames, stride=stride)
        _atomic_write(path, lambda f: torch.save(feats, f))
        written.append(path)
        log(f"Saved {uid}.")
    return written


def extract_mq(model, data_loader, save_dir, num_frames=4, batch=32, center_crop=256, input_res=224, reference_tail=False,
               stride=None, log=print):
    """run/test_mq.py over the batches of the reference's loader (batch_size 1: `data['video']` [1, F, C, H, W] -- decoded uint8 or
    transformed float frames --, `data['meta']['clip_uid']`): every clip becomes `<save_dir>/<clip_uid>.pt`, a torch.save of the fp32
    [windows, projection_dim] features; a clip whose file exists is skipped.  -> the paths written."""
    ext = ClipFeatureExtractor(model, num_frames, batch, center_crop, input_res, reference_tail)
    return _dump_videos(ext, data_loader, save_dir, stride, log)


def extract_nlq(model, data_loader, tokenizer, save_dir, subsample, token=False, num_frames=4, batch=32, center_crop=256,
                input_res=224, reference_tail=False, stride=None, log=print):
    """run/test_nlq.py.  subsample='video': the clip dump of extract_mq.  subsample='text': every batch's `data['text']` (raw
    sentences) is tokenized (`tokenizer(texts, return_tensors='pt', padding=True, truncation=True)`) and encoded, and
    `<save_dir>/sentence.npy` is np.save of the dict raw text -> CPU tensor: [1, dim] sentence embeddings as the reference stores
    them, or with token=True the [num_words - 2, dim] token embeddings.  The first occurrence of a text is kept (:110-111); later
    ones are not encoded again.  -> the paths written."""
    ext = ClipFeatureExtractor(model, num_frames, batch, center_crop, input_res, reference_tail)
    if subsample == "video":
        return _dump_videos(ext, data_loader, save_dir, stride, log)
    if subsample != "text":
        raise ValueError("extract_nlq: subsample is 'video' or 'text'")
    os.makedirs(save_dir, exist_ok=True)
    cache = {}
    for data in data_loader:
        texts = [data["text"]] if isinstance(data["text"], str) else list(data["text"])
        new = [t for t in dict.fromkeys(texts) if t not in cache]
        if not new:
            continue
        feats = ext.text_features(tokenizer(new, return_tensors="pt", padding=True, truncation=True), token=token)
        for t, f in zip(new, feats):
            cache[t] = f if token else f.unsqueeze(0)
    path = os.path.join(save_dir, "sentence.npy")
    _atomic_write(path, lambda f: np.save(f, cache, allow_pickle=True))
    return [path]
