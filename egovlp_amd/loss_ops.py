"""Tensor-level wrappers of the loss heads (include/egovlp_hip.h): the one-call heads egv_egonce_fwd_bwd, egv_egonce_long_fwd_bwd
(and their *_ls variants), egv_sigmoid_head_fwd_bwd and egv_maxmargin_head_fwd_bwd; the API-compatible pieces egv_sim_matrix_*,
egv_egonce_from_sim(_ls), egv_sigmoid_from_sim, egv_maxmargin_fwd_bwd, egv_dual_softmax, egv_cross_entropy_fwd_bwd; and the
classification head of the OSCC / PNR fine-tunes (egv_cls_head_fwd, egv_cls_head_loss_bwd, egv_cls_eval_update)."""
import ctypes

import torch

from . import _lib, ops
from ._lib import check
from .ops import _p


def _one_fp32_arg(value, like, name):
    """A head parameter read on the device (the logit scale s = log(1 / tau), the logit bias): one fp32 on the inputs' device.
    Returns a view of `value` (one element is always contiguous): its address stays valid as long as the caller's tensor."""
    v = value.detach()
    if v.dtype != torch.float32 or v.numel() != 1 or v.device != like.device:
        raise ValueError("%s must be one fp32 value on the device of the embeddings" % name)
    return v


def _head_buffers(text, video, work_floats, want_grads, param_grads=0, want_param_grads=True):
    """What every one-call head writes: loss[1], its workspace, d_text / d_video and a list of `param_grads` parameter gradients
    of [1] each; the gradients are None without want_grads, those of the parameters also without want_param_grads."""
    dev = text.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    work = torch.empty(work_floats, dtype=torch.float32, device=dev)
    dt = torch.empty_like(text) if want_grads else None
    dv = torch.empty_like(video) if want_grads else None
    want_param_grads = want_grads and want_param_grads
    return loss, work, dt, dv, [torch.empty(1, dtype=torch.float32, device=dev) if want_param_grads else None
                                for _ in range(param_grads)]


def _nv_widths(noun, verb):
    return (noun.shape[1] if noun is not None else 0), (verb.shape[1] if verb is not None else 0)


EGONCE_SHORT_MAX = 1024      # rows of egv_egonce_fwd_bwd; egonce_fwd_bwd switches to the long head past it
EGONCE_LONG_MAX = 65536      # rows of egv_egonce_long_fwd_bwd


def egonce_fwd_bwd(text, video, noun, verb, temperature, eps=1e-8, use_noun=True, use_verb=True, want_grads=True,
                   want_sim=False, logit_scale=None):
    """The contrastive head in one call -> (loss[1], sim or None, d_text, d_video).  Up to EGONCE_SHORT_MAX rows: the latency-bound
    kernels of csrc/egonce.hip; beyond: egonce_long_fwd_bwd (no n x n matrix exists there, so `want_sim` is refused).
    `logit_scale` (a device tensor holding s = log(1 / tau); `temperature` is then unused): the kernels form 1 / tau = exp(s) on the
    device and the call returns a fifth value, d_logit_scale [1] = dL/ds (None without want_grads) -- egv_egonce_fwd_bwd_ls."""
    ops._need_cuda(text, video, noun, verb)
    n, D = text.shape
    if n > EGONCE_SHORT_MAX:
        if want_sim:
            raise ValueError("egonce_fwd_bwd: want_sim needs n <= %d (the long head materialises no n x n matrix), got n = %d"
                             % (EGONCE_SHORT_MAX, n))
        out = egonce_long_fwd_bwd(text, video, noun, verb, temperature, eps=eps, use_noun=use_noun, use_verb=use_verb,
                                  want_grads=want_grads, logit_scale=logit_scale)
        return (out[0], None) + tuple(out[1:])
    dn, dv = _nv_widths(noun, verb)
    learn = logit_scale is not None
    entry = "egv_egonce_fwd_bwd_ls" if learn else "egv_egonce_fwd_bwd"
    tau = _p(_one_fp32_arg(logit_scale, text, "logit_scale")) if learn else float(temperature)
    loss, work, dt, dvv, dls = _head_buffers(text, video, _lib.lib().egv_egonce_work_floats(n, D), want_grads, int(learn))
    sim = torch.empty((n, n), dtype=torch.float32, device=text.device) if want_sim else None
    check(getattr(_lib.lib(), entry)(_p(text), _p(video), _p(noun), _p(verb), n, D, dn, dv, tau, float(eps), int(use_noun),
                                     int(use_verb), _p(loss), _p(sim), _p(dt), _p(dvv), *map(_p, dls), _p(work),
                                     ops._stream(text)), entry)
    return (loss, sim, dt, dvv, *dls)


def egonce_long_fwd_bwd(text, video, noun, verb, temperature, eps=1e-8, use_noun=True, use_verb=True, want_grads=True,
                        logit_scale=None):
    """egv_egonce_long_fwd_bwd for ANY n in [1, 65536] -> (loss[1], d_text, d_video): the tiled fp32-MFMA head with a workspace
    linear in n.  noun / verb: non-negative multi-hots (only entry > 0 is used); a negative or NaN entry makes the loss NaN.
    `logit_scale`: as in egonce_fwd_bwd -> (loss[1], d_text, d_video, d_logit_scale [1]) -- egv_egonce_long_fwd_bwd_ls."""
    ops._need_cuda(text, video, noun, verb)
    n, D = text.shape
    dn, dv = _nv_widths(noun, verb)
    learn = logit_scale is not None
    entry = "egv_egonce_long_fwd_bwd_ls" if learn else "egv_egonce_long_fwd_bwd"
    tau = _p(_one_fp32_arg(logit_scale, text, "logit_scale")) if learn else float(temperature)
    loss, work, dt, dvv, dls = _head_buffers(text, video, _lib.lib().egv_egonce_long_work_floats(n, D, dn, dv), want_grads,
                                             int(learn))
    check(getattr(_lib.lib(), entry)(_p(text), _p(video), _p(noun), _p(verb), n, D, dn, dv, tau, float(eps), int(use_noun),
                                     int(use_verb), _p(loss), _p(dt), _p(dvv), *map(_p, dls), _p(work), ops._stream(text)), entry)
    return (loss, dt, dvv, *dls)


EGONCE_QUEUE_MIN, EGONCE_QUEUE_MAX = 64, 65536     # capacity of an EgonceQueue: a multiple of 64 in this range


def egonce_queue_size_ok(Q):
    return isinstance(Q, int) and EGONCE_QUEUE_MIN <= Q <= EGONCE_QUEUE_MAX and Q % 64 == 0


class EgonceQueue:
    """The device buffers of egv_egonce_queue_fwd_bwd / _push, in the kernels' own layout (egv_egonce_queue_layout: Dp floats per
    embedding row, W words per noun / verb row): text, video [Q, Dp] fp32, words [Q, W] int32, state int32 {head, filled}.  All
    zeros: an empty queue.  `dn`, `dv`: the noun / verb widths (0, 0 for NormSoftmaxLoss)."""

    def __init__(self, Q, D, dn, dv, device):
        if not egonce_queue_size_ok(Q):
            raise ValueError("queue size must be a multiple of 64 in [%d, %d], got %r" % (EGONCE_QUEUE_MIN, EGONCE_QUEUE_MAX, Q))
        Dp, W = ctypes.c_int32(0), ctypes.c_int32(0)
        check(_lib.lib().egv_egonce_queue_layout(D, dn, dv, ctypes.byref(Dp), ctypes.byref(W)), "egv_egonce_queue_layout")
        self.Q, self.D, self.dn, self.dv, self.Dp, self.W = Q, D, dn, dv, Dp.value, W.value
        self.text = torch.zeros((Q, self.Dp), dtype=torch.float32, device=device)
        self.video = torch.zeros((Q, self.Dp), dtype=torch.float32, device=device)
        self.words = torch.zeros((Q, self.W), dtype=torch.int32, device=device)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)

    def check_batch(self, text, dn, dv):
        if text.shape[1] != self.D or (dn, dv) != (self.dn, self.dv) or text.device != self.text.device:
            raise ValueError("the queue was allocated for D = %d, noun / verb widths %d / %d on %s; got D = %d, %d / %d on %s"
                             % (self.D, self.dn, self.dv, self.text.device, text.shape[1], dn, dv, text.device))
        if text.shape[0] > self.Q:
            raise ValueError("a batch of %d rows does not fit a queue of %d" % (text.shape[0], self.Q))

    def reset(self):
        self.state.zero_()

    def filled(self):
        "valid slots, read back from the device (synchronises)"
        return int(self.state[1].item())

    def head(self):
        return int(self.state[0].item())


def egonce_queue_fwd_bwd(text, video, noun, verb, temperature, queue, eps=1e-8, use_noun=True, use_verb=True, want_grads=True,
                         logit_scale=None):
    """egv_egonce_queue_fwd_bwd: EgoNCE / NormSoftmaxLoss (noun = verb = None) of the batch with the valid slots of `queue` (an
    EgonceQueue) as extra constant columns -> (loss[1], d_text, d_video, work); with `logit_scale` (as in egonce_fwd_bwd)
    -> (loss[1], d_text, d_video, d_logit_scale [1], work).  Any n in [1, min(65536, queue.Q)].  The queue is only read; `work`
    holds what egonce_queue_push enqueues."""
    ops._need_cuda(text, video, noun, verb)
    n, D = text.shape
    dn, dv = _nv_widths(noun, verb)
    queue.check_batch(text, dn, dv)
    learn = logit_scale is not None
    ls = _p(_one_fp32_arg(logit_scale, text, "logit_scale")) if learn else None
    loss, work, dt, dvv, dls = _head_buffers(text, video, _lib.lib().egv_egonce_queue_work_floats(n, D, dn, dv, queue.Q),
                                             want_grads, int(learn))
    check(_lib.lib().egv_egonce_queue_fwd_bwd(_p(text), _p(video), _p(noun), _p(verb), n, D, dn, dv, _p(queue.text), _p(queue.video),
                                              _p(queue.words), queue.Q, _p(queue.state), 0.0 if learn else float(temperature), ls,
                                              float(eps), int(use_noun), int(use_verb), _p(loss), _p(dt), _p(dvv),
                                              _p(dls[0]) if learn else None, _p(work), ops._stream(text)), "egv_egonce_queue_fwd_bwd")
    return (loss, dt, dvv, *dls, work)


def egonce_queue_push(work, loss, n, queue):
    """egv_egonce_queue_push: the n rows the head just normalised and packed (`work`, `loss`: what egonce_queue_fwd_bwd returned)
    go into the ring; a loss that is not finite enqueues nothing.  No host read."""
    check(_lib.lib().egv_egonce_queue_push(_p(work), _p(loss), n, queue.D, queue.dn, queue.dv, _p(queue.text), _p(queue.video),
                                           _p(queue.words), queue.Q, _p(queue.state), ops._stream(work)), "egv_egonce_queue_push")


def sigmoid_head_fwd_bwd(text, video, noun, verb, logit_scale, logit_bias, eps=1e-8, use_noun=True, use_verb=True, want_grads=True,
                         want_param_grads=True):
    """egv_sigmoid_head_fwd_bwd, the pairwise sigmoid head with EgoNCE's positives (noun / verb None: mask = I, plain SigLIP), for
    ANY n in [1, 65536] -> (loss[1], d_text, d_video, d_scale[1], d_bias[1]).  `logit_scale` (s) and `logit_bias` (b) are device
    tensors of one fp32 each: u = exp(s) x + b is formed on the device.  want_grads=False: the loss alone, the four gradients are
    None; want_param_grads=False (fixed s and b): d_scale and d_bias are None.  noun / verb: non-negative multi-hots (only
    entry > 0 is used); a negative or NaN entry makes the loss NaN."""
    ops._need_cuda(text, video, noun, verb)
    n, D = text.shape
    dn, dv = _nv_widths(noun, verb)
    ls = _one_fp32_arg(logit_scale, text, "logit_scale")
    lb = _one_fp32_arg(logit_bias, text, "logit_bias")
    loss, work, dt, dvv, (dls, dlb) = _head_buffers(text, video, _lib.lib().egv_sigmoid_head_work_floats(n, D, dn, dv),
                                                    want_grads, 2, want_param_grads)
    check(_lib.lib().egv_sigmoid_head_fwd_bwd(_p(text), _p(video), _p(noun), _p(verb), n, D, dn, dv, _p(ls), _p(lb), float(eps),
                                              int(use_noun), int(use_verb), _p(loss), _p(dt), _p(dvv), _p(dls), _p(dlb), _p(work),
                                              ops._stream(text)), "egv_sigmoid_head_fwd_bwd")
    return loss, dt, dvv, dls, dlb


def sim_fwd(a, b, eps):
    ops._need_cuda(a, b)
    a = a.contiguous().float()
    b = b.contiguous().float()
    n, D = a.shape
    m = b.shape[0]
    dev = a.device
    an = torch.empty_like(a)
    bn = torch.empty_like(b)
    norms = torch.empty(n + m, dtype=torch.float32, device=dev)
    out = torch.empty((n, m), dtype=torch.float32, device=dev)
    check(_lib.lib().egv_sim_matrix_fwd(_p(a), _p(b), n, m, D, float(eps), _p(an), _p(bn), _p(norms), _p(out),
                                        ops._stream()), "egv_sim_matrix_fwd")
    return out, (an, bn, norms, n, m, D, float(eps))


def sim_bwd(data, g):
    an, bn, norms, n, m, D, eps = data
    g = g.contiguous()
    da = torch.empty_like(an)
    db = torch.empty_like(bn)
    check(_lib.lib().egv_sim_matrix_bwd(_p(g), _p(an), _p(bn), _p(norms), n, m, D, eps, _p(da), _p(db), ops._stream()),
          "egv_sim_matrix_bwd")
    return da, db


def egonce_from_sim(x, sim_v, sim_n, temperature, use_noun, use_verb, want_grad=True, logit_scale=None):
    """EgoNCE / NormSoftmaxLoss on a given similarity matrix -> (loss[1], dx).  `logit_scale` (a device tensor holding
    s = log(1 / tau); `temperature` is then unused) -> (loss[1], dx, d_logit_scale [1]) -- egv_egonce_from_sim_ls."""
    ops._need_cuda(x)
    x = x.contiguous()
    n = x.shape[0]
    if x.shape[1] != n:
        raise ValueError("EgoNCE / NormSoftmaxLoss need a square similarity matrix")
    dev = x.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x) if want_grad else None
    sv = sim_v.contiguous() if sim_v is not None else None
    sn = sim_n.contiguous() if sim_n is not None else None
    learn = logit_scale is not None
    entry = "egv_egonce_from_sim_ls" if learn else "egv_egonce_from_sim"
    tau = _p(_one_fp32_arg(logit_scale, x, "logit_scale")) if learn else float(temperature)
    work = torch.empty(n * n + (7 if learn else 6) * n, dtype=torch.float32, device=dev)
    dls = [torch.empty(1, dtype=torch.float32, device=dev) if want_grad else None] if learn else []
    check(getattr(_lib.lib(), entry)(_p(x), _p(sv), _p(sn), n, tau, int(use_noun), int(use_verb), _p(loss), _p(dx), *map(_p, dls),
                                     _p(work), ops._stream()), entry)
    return (loss, dx, *dls)


def sigmoid_from_sim(x, sim_v, sim_n, logit_scale, logit_bias, use_noun, use_verb, want_grad=True, want_param_grads=True):
    """SigmoidLoss / EgoSigmoidLoss on a given similarity matrix -> (loss[1], dx, d_scale [1], d_bias [1]) -- egv_sigmoid_from_sim.
    `logit_scale`, `logit_bias`: device tensors of one fp32 each.  want_grad=False: the loss alone; want_param_grads=False: no
    d_scale / d_bias."""
    ops._need_cuda(x, sim_v, sim_n)
    x = x.contiguous()
    n = x.shape[0]
    if x.dim() != 2 or x.shape[1] != n:
        raise ValueError("SigmoidLoss / EgoSigmoidLoss need a square similarity matrix")
    dev = x.device
    ls = _one_fp32_arg(logit_scale, x, "logit_scale")
    lb = _one_fp32_arg(logit_bias, x, "logit_bias")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dx = torch.empty_like(x) if want_grad else None
    dls = torch.empty(1, dtype=torch.float32, device=dev) if want_grad and want_param_grads else None
    dlb = torch.empty(1, dtype=torch.float32, device=dev) if want_grad and want_param_grads else None
    sv = sim_v.contiguous() if sim_v is not None else None
    sn = sim_n.contiguous() if sim_n is not None else None
    work = torch.empty(3072, dtype=torch.float32, device=dev)
    check(_lib.lib().egv_sigmoid_from_sim(_p(x), _p(sv), _p(sn), n, _p(ls), _p(lb), int(use_noun), int(use_verb), _p(loss), _p(dx),
                                          _p(dls), _p(dlb), _p(work), ops._stream()), "egv_sigmoid_from_sim")
    return loss, dx, dls, dlb


def maxmargin(x, weight, margin, fix_norm, want_grad=True):
    """MaxMarginRankingLoss (weight None) / AdaptiveMaxMarginRankingLoss on a square similarity matrix -> (loss[1], dx)."""
    ops._need_cuda(x, weight)
    x = x.contiguous().float()
    n = x.shape[0]
    if x.dim() != 2 or x.shape[1] != n:
        raise ValueError("the ranking losses need a square similarity matrix")
    w = None if weight is None else weight.contiguous().float()
    if w is not None and w.numel() != n:
        raise ValueError("weight must have one entry per row")
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if want_grad else None
    check(_lib.lib().egv_maxmargin_fwd_bwd(_p(x), _p(w), n, float(margin), int(bool(fix_norm)), _p(loss), _p(dx), ops._stream()),
          "egv_maxmargin_fwd_bwd")
    return loss, dx


MAXMARGIN_HEAD_MAX_N, MAXMARGIN_HEAD_MAX_D = 1024, 256


def maxmargin_head_ok(n, D):
    """The limits of egv_maxmargin_head_fwd_bwd (the EgoNCE head's): n <= 1024 rows of D <= 256 features, D % 4 == 0."""
    return 0 < n <= MAXMARGIN_HEAD_MAX_N and 0 < D <= MAXMARGIN_HEAD_MAX_D and D % 4 == 0


def maxmargin_head(text, video, weight, margin, fix_norm, eps=1e-8, want_sim=False):
    """sim_matrix + MaxMarginRankingLoss (weight None) / AdaptiveMaxMarginRankingLoss + backward in one call, on the global batch
    text, video [n, D] -> (loss[1], sim [n, n] or None, d_text, d_video).  Deterministic; nothing n x n is written unless
    want_sim."""
    ops._need_cuda(text, video, weight)
    if text.dim() != 2 or video.dim() != 2 or text.shape != video.shape:
        raise ValueError("maxmargin_head: text and video must both be [n, D]")
    text = text.contiguous().float()
    video = video.contiguous().float()
    n, D = text.shape
    w = None if weight is None else weight.contiguous().float()
    if w is not None and w.numel() != n:
        raise ValueError("weight must have one entry per row")
    dev = text.device
    wf = max(int(_lib.lib().egv_maxmargin_head_work_floats(n, D)), 1)
    work = torch.empty(wf, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    sim = torch.empty((n, n), dtype=torch.float32, device=dev) if want_sim else None
    dt = torch.empty_like(text)
    dv = torch.empty_like(video)
    check(_lib.lib().egv_maxmargin_head_fwd_bwd(_p(text), _p(video), _p(w), n, D, float(margin), int(bool(fix_norm)), float(eps),
                                                _p(loss), _p(sim), _p(dt), _p(dv), _p(work), ops._stream(text)),
          "egv_maxmargin_head_fwd_bwd")
    return loss, sim, dt, dv


def dual_softmax(x, temp=500.0):
    """softmax(softmax(x / temp, dim=1) * x, dim=0) of a [texts, videos] similarity matrix (run/test_epic.py:137-143)."""
    ops._need_cuda(x)
    x = x.contiguous().float()
    if x.dim() != 2:
        raise ValueError("dual_softmax needs a [texts, videos] matrix")
    n, m = x.shape
    work = torch.empty_like(x)
    out = torch.empty_like(x)
    check(_lib.lib().egv_dual_softmax(_p(x), n, m, float(temp), _p(work), _p(out), ops._stream()), "egv_dual_softmax")
    return out


def cross_entropy(logits, target, ignore_index=-100, want_grad=True, target2=None, lam=None, label_smoothing=0.0):
    """nn.CrossEntropyLoss (mean over targets != ignore_index) on [rows, classes] fp32 scores and int64 labels -> (loss[1], dlogits).
    target2 [rows] / lam [rows] / label_smoothing (Mixup / CutMix and label smoothing): the soft targets
    (1 - eps) (lam e(t) + (1 - lam) e(t2)) + eps / classes of egv_cross_entropy_soft_fwd_bwd; without any of them the call made before."""
    if lam is not None and target2 is None:
        raise ValueError("cross_entropy: lam mixes target with target2")
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError("cross_entropy: label_smoothing lies in [0, 1]")
    ops._need_cuda(logits, target, target2, lam)
    if logits.dim() != 2 or target.dim() != 1 or target.shape[0] != logits.shape[0]:
        raise ValueError("cross_entropy: logits [rows, classes], target [rows]")
    x = logits.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    t = target.to(torch.int64).contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dx = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device) if want_grad else None
    if target2 is not None or float(label_smoothing) != 0.0:
        rows = x.shape[0]
        if (target2 is not None and tuple(target2.shape) != (rows,)) or (lam is not None and tuple(lam.shape) != (rows,)):
            raise ValueError("cross_entropy: target2 [rows], lam [rows]")
        t2 = None if target2 is None else target2.to(torch.int64).contiguous()
        lm = None if lam is None else lam.to(torch.float32).contiguous()
        check(_lib.lib().egv_cross_entropy_soft_fwd_bwd(_p(x), x.stride(0), _p(t), _p(t2), _p(lm), float(label_smoothing), rows, x.shape[1],
                                                        int(ignore_index), _p(loss), _p(dx), x.shape[1], ops._stream(x)),
              "egv_cross_entropy_soft_fwd_bwd")
        return loss, dx
    check(_lib.lib().egv_cross_entropy_fwd_bwd(_p(x), x.stride(0), _p(t), x.shape[0], x.shape[1], int(ignore_index), _p(loss),
                                               _p(dx), x.shape[1], ops._stream(x)), "egv_cross_entropy_fwd_bwd")
    return loss, dx


CLS_MAX_N, CLS_MAX_B, CLS_MAX_K, CLS_MAX_C = 4096, 256, 1024, 64


def cls_head_ok(n, B, K, C):
    """The limits of egv_cls_head_fwd / egv_cls_head_loss_bwd: n <= 4096 gathered rows, B <= 256 local rows, K <= 1024 features with
    K % 4 == 0, C <= 64 classes."""
    return 0 < B <= CLS_MAX_B and B <= n <= CLS_MAX_N and 0 < K <= CLS_MAX_K and K % 4 == 0 and 0 < C <= CLS_MAX_C


class ClsLayout:
    """Columns of the fp32 row block that crosses the ranks in the classification fine-tunes: [0, C) the scores, then the class
    index, then (PNR) the state, then (PNR validation) fps as two floats (hi + lo of the fp64 value), parent_start_frame,
    parent_end_frame, parent_pnr_frame.  Integer columns are exact below 2^24.  `soft` (Mixup / CutMix) appends, AFTER all of these,
    the partner's class index and the mixing weight: a layout without it is the layout it always was."""

    def __init__(self, C, task='oscc', evaluate=False, soft=False):
        if task not in ('oscc', 'pnr'):
            raise ValueError("task is 'oscc' or 'pnr'")
        self.C, self.task = C, task
        self.target = C
        self.state = C + 1 if task == 'pnr' else -1
        self.fps = self.start = self.end = self.pnr = -1
        self.ld = C + (2 if task == 'pnr' else 1)
        if task == 'pnr' and evaluate:
            self.fps, self.start, self.end, self.pnr = C + 2, C + 4, C + 5, C + 6
            self.ld = C + 7
        self.target2 = self.lam = -1
        if soft:
            self.target2, self.lam = self.ld, self.ld + 1
            self.ld += 2

    def fill(self, packed, target, state=None, fps=None, start=None, end=None, pnr=None, target2=None, lam=None):
        """Write everything but the scores into packed [B, ld]."""
        packed[:, self.target] = target
        if self.target2 >= 0:
            packed[:, self.target2] = target2
            packed[:, self.lam] = lam
        if self.state >= 0:
            packed[:, self.state] = state
        if self.fps >= 0:
            f64 = fps.to(torch.float64)
            hi = f64.to(torch.float32)
            packed[:, self.fps] = hi
            packed[:, self.fps + 1] = f64 - hi.to(torch.float64)
            packed[:, self.start] = start
            packed[:, self.end] = end
            packed[:, self.pnr] = pnr
        return packed


def _rows_f32(x):
    """[rows, K] fp32 with unit column stride, 16-byte aligned rows (a strided view such as the CLS rows is read in place)."""
    x = x.float()
    if x.dim() != 2:
        raise ValueError("expected a [rows, K] matrix")
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.stride(0) < x.shape[1] or x.data_ptr() % 16 != 0:
        x = x.contiguous()
    return x


def cls_head_fwd(feats, weight, bias, out=None):
    """scores = feats W^T + b for feats [B, K], weight [C, K], bias [C] or None (egv_cls_head_fwd).  `out` [B, ld >= C] fp32:
    the scores go to its first C columns (the block the collective sends) and `out` is returned; else a new [B, C]."""
    ops._need_cuda(feats, weight)
    x = _rows_f32(feats.detach())
    w = weight.detach().float().contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    B, K = x.shape
    C = w.shape[0]
    if w.shape[1] != K:
        raise ValueError("cls_head_fwd: feats [B, K] and weight [C, K]")
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < C or out.stride(1) != 1:
        raise ValueError("cls_head_fwd: out must be fp32 [B, >= C] with unit column stride")
    check(_lib.lib().egv_cls_head_fwd(_p(x), x.stride(0), _p(w), _p(b), B, K, C, _p(out), out.stride(0), ops._stream(x)),
          "egv_cls_head_fwd")
    return out


def cls_head_loss_bwd(packed, C, col_target, col_state=-1, row0=0, B=None, feats=None, weight=None, want_grad=True, want_pred=False,
                      col_target2=-1, col_lam=-1, label_smoothing=0.0):
    """Loss (and backward) of the classification head on the gathered block packed [n, ld] (egv_cls_head_loss_bwd)
    -> (loss[1], dW [C, K], db [C], dfeats [B, K], pred int32 [n]); entries not asked for are None.  feats [B, K]: the LOCAL rows
    row0 .. row0 + B of the batch.  col_target2 / col_lam (columns of the partner's class and of the mixing weight; -1: none) or
    label_smoothing > 0: the soft-target head, egv_cls_head_loss_bwd_soft; without any of them the call made before."""
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError("cls_head_loss_bwd: label_smoothing lies in [0, 1]")
    ops._need_cuda(packed)
    if packed.dim() != 2 or packed.dtype != torch.float32 or packed.stride(1) != 1:
        raise ValueError("cls_head_loss_bwd: packed must be fp32 [n, ld] with unit column stride")
    n = packed.shape[0]
    dev = packed.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    work = torch.empty(n + 1, dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev) if want_pred else None
    x = w = dW = db = dx = None
    B = n if B is None else B
    K = 4
    if not want_grad:
        row0, B = 0, 1                       # no local rows are read
    else:
        x = _rows_f32(feats.detach())
        w = weight.detach().float().contiguous()
        if x.shape[0] != B or w.shape != (C, x.shape[1]):
            raise ValueError("cls_head_loss_bwd: feats [B, K] and weight [C, K]")
        K = x.shape[1]
        dW = torch.empty((C, K), dtype=torch.float32, device=dev)
        db = torch.empty(C, dtype=torch.float32, device=dev)
        dx = torch.empty((B, K), dtype=torch.float32, device=dev)
    if int(col_target2) >= 0 or int(col_lam) >= 0 or float(label_smoothing) != 0.0:
        check(_lib.lib().egv_cls_head_loss_bwd_soft(_p(packed), packed.stride(0), n, C, int(col_target), int(col_state), int(col_target2),
                                                    int(col_lam), float(label_smoothing), int(row0), B, _p(x),
                                                    0 if x is None else x.stride(0), _p(w), K, _p(loss), _p(dW), _p(db), _p(dx), K,
                                                    _p(pred), _p(work), ops._stream(packed)), "egv_cls_head_loss_bwd_soft")
        return loss, dW, db, dx, pred
    check(_lib.lib().egv_cls_head_loss_bwd(_p(packed), packed.stride(0), n, C, int(col_target), int(col_state), int(row0), B,
                                           _p(x), 0 if x is None else x.stride(0), _p(w), K, _p(loss), _p(dW), _p(db), _p(dx), K,
                                           _p(pred), _p(work), ops._stream(packed)), "egv_cls_head_loss_bwd")
    return loss, dW, db, dx, pred


def cls_eval_update(packed, layout, accum):
    """Add the rows of a gathered validation block packed [n, layout.ld] to accum (float64 [4] on the device: hits, rows, sum of
    err_sec, positives) -- egv_cls_eval_update.  Blocks of more than 4096 rows are fed in pieces."""
    ops._need_cuda(packed, accum)
    if packed.dim() != 2 or packed.dtype != torch.float32 or packed.stride(1) != 1 or packed.shape[1] < layout.ld:
        raise ValueError("cls_eval_update: packed must be fp32 [n, >= layout.ld] with unit column stride")
    if accum.dtype != torch.float64 or accum.numel() != 4 or not accum.is_contiguous():
        raise ValueError("cls_eval_update: accum is a contiguous float64 [4]")
    for lo in range(0, packed.shape[0], CLS_MAX_N):
        part = packed[lo:lo + CLS_MAX_N]
        check(_lib.lib().egv_cls_eval_update(_p(part), part.stride(0), part.shape[0], layout.C, layout.target, layout.state,
                                             layout.fps, layout.start, layout.end, layout.pnr, _p(accum), ops._stream(packed)),
              "egv_cls_eval_update")
    return accum
