"""Charades-Ego fine-tuning -- drop-in for the reference's trainer/trainer_charades.py (`Multi_Trainer_dist_Charades`).

Training is the retrieval step of the EPIC-MIR trainer (the two reference files share it line for line); validation is
zero-shot action classification (:182-262): the 157 class sentences are encoded once per validation, every clip is scored
against them and the multi-label mAP of `charades_metrics` is taken on the device.
"""
from __future__ import annotations

import csv
import os

import torch

from ..gather import _gather_rows, _world
from ..model.model import sim_matrix
from .trainer_epic import RetrievalTrainerBase, format_nested_metrics_for_writer  # noqa: F401  (re-exported, as the reference file has it)

CHARADES_CLASSES_FILE = 'dataset/charades/CharadesEgo/Charades_v1_classes.txt'      # trainer/trainer_charades.py:187


def read_class_sentences(path=CHARADES_CLASSES_FILE):
    """Charades_v1_classes.txt: one 'c012 Holding a box' per line -> the sentence after the 5-character class id (:186-190)."""
    with open(path, 'r') as f:
        return [line[0][5:] for line in csv.reader(f) if line]


class Multi_Trainer_dist_Charades(RetrievalTrainerBase):
    """Same constructor as the reference plus `class_sentences` (list of str, also settable as an attribute): the class
    descriptions the clips are scored against; None reads them from `classes_file` at validation time."""

    classes_file = CHARADES_CLASSES_FILE

    def __init__(self, args, model, loss, metrics, optimizer, config, data_loader, valid_data_loader=None,
                 lr_scheduler=None, len_epoch=None, writer=None, visualizer=None, tokenizer=None,
                 max_samples_per_epoch=50000, class_sentences=None):
        super().__init__(args, model, loss, metrics, optimizer, config, data_loader, valid_data_loader, lr_scheduler,
                         len_epoch, writer, visualizer, tokenizer, max_samples_per_epoch)
        self.class_sentences = class_sentences

    def _class_embeds(self):
        sentences = self.class_sentences if self.class_sentences is not None else read_class_sentences(self.classes_file)
        os.environ["TOKENIZERS_PARALLELISM"] = "false"
        tokens = self.tokenizer(list(sentences), return_tensors='pt', padding=True, truncation=True)
        tokens = {key: val.to(self.device) for key, val in tokens.items()}
        core = getattr(self.model, 'module', self.model)
        # the reference pushes a dummy clip through the whole model to get at the text tower (:197-198); here the tower is called
        core.exec_ctx.begin_step()
        return core.compute_text(tokens)

    def _valid_epoch(self, epoch):
        """:182-262: class sentences once, videos per batch, targets gathered; `sim_matrix(text, video).T` [videos, classes]
        against the multi-hot targets through the configured metrics.  Embeddings and targets stay on the device."""
        self.model.eval()
        n_loaders = len(self.valid_data_loader)
        vid_arr = {x: [] for x in range(n_loaders)}
        target_arr = {x: [] for x in range(n_loaders)}
        world = _world()
        with torch.no_grad():
            text_embeds = self._class_embeds()
            for dl_idx, dl in enumerate(self.valid_data_loader):
                for data in dl:
                    data_target = data['target'].to(self.device)
                    # the reference also encodes the clips' own captions and drops the result (:213): only the video tower runs
                    vid_embed = self.model({'video': data['video'].to(self.device)}, video_only=True)
                    vid_arr[dl_idx].append(_gather_rows(vid_embed, world))                       # :215-218
                    target_arr[dl_idx].append(_gather_rows(data_target, world))                  # :220-223
            nested_metrics = {x: {} for x in range(n_loaders)}
            for dl_idx in range(n_loaders):
                if not vid_arr[dl_idx]:
                    continue
                sims = sim_matrix(text_embeds, torch.cat(vid_arr[dl_idx])).t()                   # :240
                targets = torch.cat(target_arr[dl_idx])
                self.last_val_similarity = sims
                for metric in self.metrics:
                    res = metric(sims, targets)
                    nested_metrics[dl_idx][metric.__name__] = res
                    self._report(epoch, dl_idx, metric.__name__, res, verbose)
        return self._val_result(nested_metrics)


def verbose(epoch, metrics, mode, name="TEST"):
    """The validation log line of trainer/trainer_charades.py:264-268."""
    msg = f"[{mode}]{name:s} epoch {epoch}, mAP: {metrics['mAP']:.3f}"
    print(msg)
    return msg
