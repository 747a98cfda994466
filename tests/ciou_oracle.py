"""The CIoU box term (box_loss='ciou': reference loss.py:63-113, bbox_ciou, in place of bbox_giou in loss.py:156) and its gradient
w.r.t. the raw (tx, ty, tw, th), restated in NumPy from the formulas, per responsible lane.  Nothing here is shared with the
package's code.  The confidence and class parts come from loss_oracle / lossgrad_oracle unchanged: `loss_terms` and `loss_grad`
here replace the box columns of theirs.

  forward   ciou = iou - p2 / c2 - a v
            iou = inter / (union + 1e-9), both areas from the corners (min / max normalised, the identity for positive sizes)
            p2 = |centre_p - centre_l|^2,  c2 = ew^2 + eh^2 of the enclosing box (a plain division)
            v = 4 (atan(pw / (ph + 1e-9)) - atan(lw / (lh + 1e-9)))^2 / pi^2,  a = v / D,  D = 1 - iou + v
            term = (2 - lw lh / input_area) (1 - ciou), weight 3.54
  gradient  there is no stop_gradient: a v = v^2 / D is differentiated as a whole
            d ciou = (1 - a^2) d iou - (2 a - a^2) d v - d p2 / c2 + p2 / c2^2 d c2
            d iou = (A + inter A^2) d inter - inter A^2 d area_p,  A = 1 / (union + 1e-9)
            d c2 = 2 ew d ew + 2 eh d eh,  d p2 = 2 (px - lx) d px + 2 (py - ly) d py
            d v = 8 / pi^2 (atan q - atan q_l) / (1 + q^2) d q,  q = pw / (ph + 1e-9)
            d px / d tx = stride s_x (1 - s_x),  d pw / d tw = pw.  Ties of a maximum / minimum: the strict comparison decides.

`forward(..., xp=torch)` runs the same text on torch tensors, for autograd (tests/test_ciou_cpu.py); `dtype=np.float32` evaluates
everything in float32, from which the GPU tests take d_ref where no reference run exists.
"""
import math

import numpy as np

import loss_oracle as LO
import lossgrad_oracle as GO

PI2 = math.pi ** 2
E9 = 1e-9


def lanes(head, label, anchors_s, ncls, dtype=np.float64):
    """The responsible lanes of one scale -> (idx: the (image, row, col, anchor) index arrays, t4 [m, 4], grid [m, 2] (col, row),
    anchor [m, 2], lab [m, 4]) in `dtype`."""
    n, gh, gw, _ = head.shape
    t = np.asarray(head).reshape(n, gh, gw, 3, 5 + ncls)
    label = np.asarray(label)
    idx = np.nonzero(label[..., 4] == 1)
    t4 = t[idx][:, 0:4].astype(dtype)
    grid = np.stack([idx[2], idx[1]], axis=-1).astype(dtype)
    anc = np.asarray(anchors_s, dtype=dtype).reshape(3, 2)[idx[3]]
    return idx, t4, grid, anc, label[idx][:, 0:4].astype(dtype)


def forward(t4, grid, anc, lab, stride, input_area, xp=np):
    """-> dict of every intermediate of the lanes; 'term' is (2 - lw lh / input_area) (1 - ciou), unweighted."""
    f = {}
    f["sxy"] = 1.0 / (1.0 + xp.exp(-t4[:, 0:2]))
    f["pxy"] = (f["sxy"] + grid) * stride
    f["pwh"] = xp.exp(t4[:, 2:4]) * anc
    c0, c1 = f["pxy"] - f["pwh"] * 0.5, f["pxy"] + f["pwh"] * 0.5
    f["plo"], f["phi"] = xp.minimum(c0, c1), xp.maximum(c0, c1)
    l0, l1 = lab[:, 0:2] - lab[:, 2:4] * 0.5, lab[:, 0:2] + lab[:, 2:4] * 0.5
    f["llo"], f["lhi"] = xp.minimum(l0, l1), xp.maximum(l0, l1)
    f["cwh"] = f["phi"] - f["plo"]
    lwh = f["lhi"] - f["llo"]
    f["raw"] = xp.minimum(f["phi"], f["lhi"]) - xp.maximum(f["plo"], f["llo"])
    f["iwh"] = xp.clip(f["raw"], 0.0, None)
    f["inter"] = f["iwh"][:, 0] * f["iwh"][:, 1]
    f["den"] = f["cwh"][:, 0] * f["cwh"][:, 1] + lwh[:, 0] * lwh[:, 1] - f["inter"] + E9
    f["iou"] = f["inter"] / f["den"]
    f["ewh"] = xp.maximum(f["phi"], f["lhi"]) - xp.minimum(f["plo"], f["llo"])
    f["c2"] = f["ewh"][:, 0] ** 2 + f["ewh"][:, 1] ** 2
    f["dxy"] = f["pxy"] - lab[:, 0:2]
    f["p2"] = f["dxy"][:, 0] ** 2 + f["dxy"][:, 1] ** 2
    f["hq"] = f["pwh"][:, 1] + E9
    f["q"] = f["pwh"][:, 0] / f["hq"]
    f["dat"] = xp.arctan(f["q"]) - xp.arctan(lab[:, 2] / (lab[:, 3] + E9))
    f["v"] = 4.0 * f["dat"] ** 2 / PI2
    f["D"] = 1.0 - f["iou"] + f["v"]
    f["a"] = f["v"] / f["D"]
    f["ciou"] = f["iou"] - f["p2"] / f["c2"] - f["a"] * f["v"]
    f["scale"] = 2.0 - lab[:, 2] * lab[:, 3] / input_area
    f["term"] = f["scale"] * (1.0 - f["ciou"])
    return f


def lane_grad(t4, grid, anc, lab, stride, input_area):
    """d term / d (tx, ty, tw, th) of every lane, [m, 4], analytic (unweighted: without 3.54 and the image weight)."""
    f = forward(t4, grid, anc, lab, stride, input_area)
    a2 = f["a"] ** 2
    k_iou, k_v = 1.0 - a2, a2 - 2.0 * f["a"]
    A = 1.0 / f["den"]
    b_i = -f["inter"] * A * A
    c_inter, c_area = (k_iou * (A - b_i))[:, None], (k_iou * b_i)[:, None]
    e = 2.0 * f["ewh"] * (f["p2"] / f["c2"] ** 2)[:, None]                # p2 / c2^2 d c2 / d (ew, eh)
    other = f["iwh"][:, ::-1]                                             # d (iw ih) / d iw = ih, ...
    pos = f["raw"] > 0.0
    g_lo = c_inter * np.where(pos & (f["plo"] > f["llo"]), -other, 0.0) + np.where(f["plo"] < f["llo"], -e, 0.0)
    g_hi = c_inter * np.where(pos & (f["phi"] < f["lhi"]), other, 0.0) + np.where(f["phi"] > f["lhi"], e, 0.0)
    g_ctr = g_lo + g_hi - 2.0 * f["dxy"] / f["c2"][:, None]
    dvq = k_v * (8.0 / PI2) * f["dat"] / (1.0 + f["q"] ** 2)              # (d ciou / d v) (d v / d q)
    dq = np.stack([1.0 / f["hq"], -f["pwh"][:, 0] / f["hq"] ** 2], axis=-1)
    g_wh = 0.5 * (g_hi - g_lo) + c_area * f["cwh"][:, ::-1] + dvq[:, None] * dq
    k = -f["scale"][:, None]                                              # d term = -scale d ciou
    return np.concatenate([k * g_ctr * stride * f["sxy"] * (1.0 - f["sxy"]), k * g_wh * f["pwh"]], axis=-1)


def box_sums(head, label, anchors_s, stride, ncls, input_area, dtype=np.float64):
    """One scale -> the box term's sum per image [n] (unweighted, as y4_loss returns it), accumulated in `dtype`."""
    idx, t4, grid, anc, lab = lanes(head, label, anchors_s, ncls, dtype)
    term = forward(t4, grid, anc, lab, dtype(stride), dtype(input_area))["term"]
    out = np.zeros(head.shape[0], dtype=dtype)
    np.add.at(out, idx[0], term)
    return out


def loss_terms(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw, dtype=np.float64):
    """loss_oracle.loss_terms with the box column replaced by the CIoU term -> float64 [n, 3 scales, 3 terms] (with dtype =
    np.float32 the box column is the float32 evaluation; the other columns stay float64)."""
    out = LO.loss_terms(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw)
    anchors3 = np.asarray(anchors, dtype=np.float64).reshape(3, 3, 2)
    area = float(input_hw[0]) * float(input_hw[1])
    for s in range(3):
        out[:, s, 0] = box_sums(heads[s], labels[s], anchors3[s], strides[s], ncls, area, dtype)
    return out


def lane_conditions(heads, labels, anchors, strides, ncls, input_hw):
    """-> (the smallest 1 - iou + v, the smallest c2) over the responsible lanes of all scales: what the comparison needs to be
    away from 0 (the reference itself is non-finite there)."""
    anchors3 = np.asarray(anchors, dtype=np.float64).reshape(3, 3, 2)
    area = float(input_hw[0]) * float(input_hw[1])
    d_min, c2_min = np.inf, np.inf
    for s in range(3):
        _, t4, grid, anc, lab = lanes(heads[s], labels[s], anchors3[s], ncls)
        f = forward(t4, grid, anc, lab, float(strides[s]), area)
        if f["D"].size:
            d_min, c2_min = min(d_min, float(f["D"].min())), min(c2_min, float(f["c2"].min()))
    return d_min, c2_min


def loss_grad(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw, img_weight=None, dtype=np.float64):
    """lossgrad_oracle.loss_grad with the four box columns of every responsible lane replaced by the CIoU term's gradient
    -> three float64 arrays [n, gh, gw, 3 (5 + C)] (with dtype = np.float32 the box columns hold the float32 evaluation; the
    other columns stay float64)."""
    g = GO.loss_grad(heads, labels, true_xywh, anchors, strides, ncls, thresh, input_hw, img_weight)
    anchors3 = np.asarray(anchors, dtype=np.float64).reshape(3, 3, 2)
    n = heads[0].shape[0]
    w = np.full(n, 1.0 / n) if img_weight is None else np.asarray(img_weight, dtype=np.float64)
    area = float(input_hw[0]) * float(input_hw[1])
    out = []
    for s in range(3):
        idx, t4, grid, anc, lab = lanes(heads[s], labels[s], anchors3[s], ncls, dtype)
        g5 = g[s].reshape(heads[s].shape[:3] + (3, 5 + ncls)).copy()
        box = np.zeros(g5.shape[:4] + (4,))
        box[idx] = dtype(LO.WEIGHTS[0]) * w.astype(dtype)[idx[0]][:, None] * lane_grad(t4, grid, anc, lab, dtype(strides[s]), dtype(area))
        g5[..., 0:4] = box
        out.append(g5.reshape(heads[s].shape))
    return out
