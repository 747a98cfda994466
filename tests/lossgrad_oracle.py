"""The gradient of the validation loss w.r.t. the raw heads, restated in float64 NumPy from its formulas (beside loss_oracle.py;
nothing here is shared with the package's code), the head convs' weight gradient, and Keras' Adam rule.

Objective:  sum_i img_weight[i] * (3.54 box_i + 64.3 conf_i + class_i)   (reference loss.py:131-135; 1 / N gives the batch mean)

  class       respond * (sigmoid(t_c) - label_c)
  confidence  with q = sigmoid(t), r = respond, m = r + respond_bgd (the ignore mask is a cast: no gradient through max IoU):
              m * [ -2 (r - q) q (1 - q) BCE(t, r) + (r - q)^2 (q - r) ]
  box         GIoU = iou - 1 + union / enclose (without the last term where enclose == 0), iou = inter / (union + eps),
              union = area_p + area_l - inter:
              d giou = (A - B) d inter + B d area_p + E d enclose,  A = 1 / (union + eps), B = -inter / (union + eps)^2 + 1 / enclose,
              E = -union / enclose^2;  the corners x1 = px - pw / 2, x2 = px + pw / 2 carry it to px and pw,
              d px / d tx = stride q_x (1 - q_x),  d pw / d tw = pw.  Ties of a maximum / minimum: the strict comparison decides.
"""
import numpy as np

import loss_oracle as LO


def scale_grad(head, label, true_xywh, anchors_s, stride, ncls, thresh, input_area, img_weight, dtype=np.float64):
    """One scale -> `dtype` [n, gh, gw, 3 (5 + C)] (float32: every operation in single precision, which measures what it costs)."""
    t, pred = LO.decode(head, anchors_s, stride, ncls, dtype)
    label = np.asarray(label, dtype=dtype)
    w_img = np.asarray(img_weight, dtype=dtype)[:, None, None, None]
    r = label[..., 4]
    g = np.zeros_like(t)
    # class
    g[..., 5:] = r[..., None] * (LO._sigmoid(t[..., 5:]) - label[..., 5:])
    # confidence
    rows = np.asarray(true_xywh, dtype=dtype)[:, None, None, None, :, :]
    max_iou = LO._iou_parts(pred[..., None, :], rows)[0].max(axis=-1)
    m = r + (1.0 - r) * (max_iou < dtype(thresh))
    q = LO._sigmoid(t[..., 4])
    d = r - q
    g[..., 4] = LO.WEIGHTS[1] * m * (-2.0 * d * q * (1.0 - q) * LO._bce(t[..., 4], r) + d * d * (q - r))
    # box
    lab = label[..., 0:4]
    plo, phi = LO._corners(pred)
    llo, lhi = LO._corners(lab)
    raw = np.minimum(phi, lhi) - np.maximum(plo, llo)                     # [..., 2]: x, y
    iwh = np.maximum(raw, 0.0)
    inter = iwh[..., 0] * iwh[..., 1]
    uni = pred[..., 2] * pred[..., 3] + lab[..., 2] * lab[..., 3] - inter
    ewh = np.maximum(phi, lhi) - np.minimum(plo, llo)
    enc = ewh[..., 0] * ewh[..., 1]
    ok = enc != 0.0
    safe = np.where(ok, enc, 1.0)
    A = 1.0 / (uni + LO.EPS)
    B = -inter * A * A + np.where(ok, 1.0 / safe, 0.0)
    E = np.where(ok, -uni / (safe * safe), 0.0)
    AB = A - B
    other_i, other_e = iwh[..., ::-1], ewh[..., ::-1]                     # d (iw ih) / d iw = ih, ...
    pos = raw > 0.0
    g_lo = AB[..., None] * np.where(pos & (plo > llo), -other_i, 0.0) + E[..., None] * np.where(plo < llo, -other_e, 0.0)
    g_hi = AB[..., None] * np.where(pos & (phi < lhi), other_i, 0.0) + E[..., None] * np.where(phi > lhi, other_e, 0.0)
    g_ctr = g_lo + g_hi
    g_wh = 0.5 * (g_hi - g_lo) + B[..., None] * pred[..., 3:1:-1]
    k = -LO.WEIGHTS[0] * r * (2.0 - lab[..., 2] * lab[..., 3] / input_area)
    sxy = LO._sigmoid(t[..., 0:2])
    g[..., 0:2] = k[..., None] * g_ctr * stride * sxy * (1.0 - sxy)
    g[..., 2:4] = k[..., None] * g_wh * pred[..., 2:4]
    g *= w_img[..., None]
    return g.reshape(head.shape)


def loss_grad(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw, img_weight=None, dtype=np.float64):
    """-> three `dtype` arrays [n, gh, gw, 3 (5 + C)]: d(sum_i img_weight[i] * loss_i) / d head (img_weight: 1 / n by default)."""
    anchors = np.asarray(anchors, dtype=np.float64).reshape(3, 3, 2)
    n = heads[0].shape[0]
    w = np.full(n, 1.0 / n) if img_weight is None else np.asarray(img_weight, dtype=np.float64)
    area = float(input_hw[0]) * float(input_hw[1])
    return [scale_grad(heads[s], labels[s], true_xywh, anchors[s], strides[s], ncls, thresh, area, w, dtype) for s in range(3)]


def head_wgrad(g, x, dtype=np.float64):
    """g [n, gh, gw, cout] and the head conv's input x [n, gh, gw, cin] -> (db [cout], dW [cout, cin]) summed in `dtype`."""
    g = np.asarray(g, dtype=dtype).reshape(-1, g.shape[-1])
    x = np.asarray(x, dtype=dtype).reshape(-1, x.shape[-1])
    return g.sum(axis=0, dtype=dtype), np.einsum("po,pc->oc", g, x).astype(dtype)


def adam_step(w, m, v, g, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-7, dtype=np.float64):
    """Keras' Adam (reference models.py:83): -> (w, m, v) after step t = 1, 2, ..., every operation in `dtype`."""
    f = dtype
    w, m, v, g = (np.asarray(a, dtype=f) for a in (w, m, v, g))
    lr_t = f(f(lr) * np.sqrt(f(1) - f(b2) ** f(t)) / (f(1) - f(b1) ** f(t)))
    m = f(b1) * m + (f(1) - f(b1)) * g
    v = f(b2) * v + (f(1) - f(b2)) * (g * g)
    return w - lr_t * m / (np.sqrt(v) + f(eps)), m, v


def rel_to_max(a, b):
    """max |a - b| / max |b|: the distance the gradient budgets are stated in."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(np.float64).tiny))
