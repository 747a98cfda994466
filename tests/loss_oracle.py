"""The validation loss restated in float64 NumPy from its formulas (reference loss.py:119-212 as it runs): the yardstick of
the device kernel.  Nothing here is shared with the package's code.

  decode      xy = (sigmoid(t_xy) + grid) * stride (no xyscale), wh = exp(t_wh) * anchor
  box         respond * (2 - w h / input_area) * (1 - GIoU(pred, label)), IoU denominator + 1e-7, enclosing term divide_no_nan
  class       respond * sum_c BCE-with-logits(t_c, label_c),   BCE = max(x, 0) - x z + log1p(exp(-|x|))
  confidence  (respond - sigmoid(t_conf))^2 * BCE(t_conf, respond) * (respond + respond_bgd),
              respond_bgd = (1 - respond) * [max over all true-box rows of IoU(pred, row) < iou_loss_thresh]
"""
import numpy as np

EPS = float(np.float32(1e-7))             # K.epsilon() as the float32 the reference adds
WEIGHTS = (3.54, 64.3, 1.0)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _bce(x, z):
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def _corners(b):
    return b[..., 0:2] - b[..., 2:4] * 0.5, b[..., 0:2] + b[..., 2:4] * 0.5


def _iou_parts(b1, b2):
    a1, a2 = b1[..., 2] * b1[..., 3], b2[..., 2] * b2[..., 3]
    lo1, hi1 = _corners(b1)
    lo2, hi2 = _corners(b2)
    inter = np.prod(np.maximum(np.minimum(hi1, hi2) - np.maximum(lo1, lo2), 0.0), axis=-1)
    union = a1 + a2 - inter
    return inter / (union + EPS), union, np.prod(np.maximum(hi1, hi2) - np.minimum(lo1, lo2), axis=-1)


def decode(head, anchors_s, stride, ncls, dtype=np.float64):
    n, gh, gw, _ = head.shape
    t = np.asarray(head, dtype=dtype).reshape(n, gh, gw, 3, 5 + ncls)
    grid = np.stack(np.meshgrid(np.arange(gw), np.arange(gh)), axis=-1)[None, :, :, None, :].astype(dtype)
    xy = (_sigmoid(t[..., 0:2]) + grid) * dtype(stride)
    wh = np.exp(t[..., 2:4]) * np.asarray(anchors_s, dtype=dtype)
    return t, np.concatenate([xy, wh], axis=-1)


def scale_terms(head, label, true_xywh, anchors_s, stride, ncls, thresh, input_area):
    """One scale -> (terms [n, 3] float64: box, confidence, class sums per image; max_iou [n, gh, gw, 3]; respond)."""
    t, pred = decode(head, anchors_s, stride, ncls)
    label = np.asarray(label, dtype=np.float64)
    respond = label[..., 4]
    iou, union, enclose = _iou_parts(pred, label[..., 0:4])
    with np.errstate(divide="ignore", invalid="ignore"):
        giou = iou - np.where(enclose == 0.0, 0.0, (enclose - union) / enclose)
    box = respond * (2.0 - label[..., 2] * label[..., 3] / input_area) * (1.0 - giou)
    cls = respond * _bce(t[..., 5:], label[..., 5:]).sum(axis=-1)
    rows = np.asarray(true_xywh, dtype=np.float64)[:, None, None, None, :, :]
    max_iou = _iou_parts(pred[..., None, :], rows)[0].max(axis=-1)
    bgd = (1.0 - respond) * (max_iou < thresh)
    bce = _bce(t[..., 4], respond)
    conf = (respond - _sigmoid(t[..., 4])) ** 2 * (respond * bce + bgd * bce)
    return np.stack([x.sum(axis=(1, 2, 3)) for x in (box, conf, cls)], axis=-1), max_iou, respond


def loss_terms(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw):
    """-> float64 [n, 3 scales, 3 terms]."""
    anchors = np.asarray(anchors, dtype=np.float64).reshape(3, 3, 2)
    area = float(input_hw[0]) * float(input_hw[1])
    return np.stack([scale_terms(heads[s], labels[s], true_xywh, anchors[s], strides[s], ncls, thresh, area)[0]
                     for s in range(3)], axis=1)


def total(terms):
    """The reference's scalar (loss.py:136-140): weighted sum over terms and scales, mean over the batch."""
    return float((np.asarray(terms, dtype=np.float64).sum(axis=1) * np.array(WEIGHTS)).sum(axis=1).mean())


def rel_dist(a, b):
    """|a - b| / |b| elementwise (0 where both are 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    return np.where(d == 0.0, 0.0, d / np.maximum(np.abs(b), np.finfo(np.float64).tiny))
