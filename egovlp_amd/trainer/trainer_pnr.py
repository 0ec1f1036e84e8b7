"""Ego4D point-of-no-return (PNR) keyframe localisation fine-tuning -- drop-in for the reference's trainer/trainer_pnr.py.

Training is `classification_step(task='pnr')` of trainer_oscc.py: the head scores the 16 sampled frames, the target is the argmax
of the one-hot `labels` (0 for the all-zero rows of clips without a state change) and the loss is
`mean(state.T * CrossEntropy(scores, target))` over the gathered batch (trainer/trainer_pnr.py:341-350).  Validation (:400-519)
sends scores, target, state, fps and the three parent frame numbers of a batch in ONE row block (the reference: seven
collectives and seven host copies) and egv_cls_eval_update adds the keyframe errors of `pnr_metrics` on the device; fps crosses
as two floats so that an fp64 frame rate such as 29.97 keeps 48 bits.
"""
from __future__ import annotations

from .trainer_oscc import ClassificationTrainerBase, classification_step, format_nested_metrics_for_writer  # noqa: F401


def verbose(epoch, metrics, name="TEST"):
    """The validation log line of trainer/trainer_pnr.py:531-535."""
    msg = f"{name:s} epoch {epoch}, keyframe_distance: {metrics['keyframe_distance']:.1f}"
    print(msg)
    return msg


class Multi_Trainer_dist_PNR(ClassificationTrainerBase):
    """Drop-in for trainer/trainer_pnr.py:238-529 (configs/ft/pnr.json: CrossEntropy, pnr_metrics)."""

    task = 'pnr'
    _verbose = staticmethod(verbose)

    def __init__(self, args, *rest, **kw):
        self.args = args
        if self._mix_on():          # a blended clip has no keyframe: refused here, before anything is built
            raise ValueError("Multi_Trainer_dist_PNR: Mixup / CutMix (args.mixup_alpha / args.cutmix_alpha) does not apply to keyframe "
                             "localisation; PNR takes label smoothing only (CrossEntropy(label_smoothing=...))")
        super().__init__(args, *rest, **kw)

    def _val_columns(self, data):
        cols = super()._val_columns(data)
        for key, name in (('fps', 'fps'), ('start', 'parent_start_frame'), ('end', 'parent_end_frame'), ('pnr', 'parent_pnr_frame')):
            cols[key] = data[name].to(self.device).reshape(-1)                                   # :431-435
        return cols
