"""Test oracle for the NMS pair rule (y4_set_nms_rule): `oracle.decode_nms.combined_nms` restated as ONE greedy pass over the
globally ordered candidates, with the measure and the class scope of the rule.  NumPy only.

Candidates are every (box, class) with score > score_threshold (strict), in the order both sides define: score descending, box
index ascending, class ascending.  A candidate whose class already holds `per_class` kept boxes is turned away: it is not kept
and suppresses nothing.  Otherwise it is kept unless an earlier KEPT candidate -- of its class, or with `agnostic` of any class
-- has a measure m > iou_threshold (strict); the pass ends with `total` kept boxes.  For ('iou', agnostic=False) that is
combined_nms exactly: a class's candidates are visited in that class's own descending order and tested against that class's
kept boxes only, and a class's (per_class + 1)-th survivor could never be among the best `total`.

The measure, in float32 in the kernel's operation order (decode_nms.hip nms_measure), on the normalised canvas boxes:
    iou = TensorFlow's IOU(): corners min / max-normalised per axis, 0 if either area <= 0
    d2  = (cya - cyb)^2 + (cxa - cxb)^2,  centres = 0.5 * (lo + hi) of the normalised corners
    c2  = (max(hi) - min(lo))_y^2 + (..)_x^2
    m   = iou                                   kind 'iou'
        = c2 == 0 ? iou : iou - (d2 / c2)^beta  kind 'diou'   (beta == 1: the quotient itself)

`min_margin` is the smallest |m - iou_threshold| over every pair the pass tested, evaluated in float32 and again in float64 (the
same formulas on the same float32 boxes), the smaller of the two: a test that asserts it is well above float32 rounding knows
that no decision hangs on the last bits of a powf or a division."""
import numpy as np

F32 = np.float32
KINDS = ("iou", "diou")


def measure(b, others, kind="iou", beta=1.0, dtype=F32):
    """m of box b [4] against others [k, 4], computed in `dtype` -> [k]."""
    assert kind in KINDS
    T = dtype
    b = np.asarray(b, F32).astype(T)
    o = np.asarray(others, F32).astype(T).reshape(-1, 4)
    y0 = np.minimum(b[0], b[2]); x0 = np.minimum(b[1], b[3])
    y1 = np.maximum(b[0], b[2]); x1 = np.maximum(b[1], b[3])
    oy0 = np.minimum(o[:, 0], o[:, 2]); ox0 = np.minimum(o[:, 1], o[:, 3])
    oy1 = np.maximum(o[:, 0], o[:, 2]); ox1 = np.maximum(o[:, 1], o[:, 3])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        area_i = T((y1 - y0) * (x1 - x0))
        area_j = ((oy1 - oy0) * (ox1 - ox0)).astype(T)
        iy0 = np.maximum(y0, oy0); ix0 = np.maximum(x0, ox0)
        iy1 = np.minimum(y1, oy1); ix1 = np.minimum(x1, ox1)
        inter = (np.maximum(iy1 - iy0, T(0)) * np.maximum(ix1 - ix0, T(0))).astype(T)
        iou = (inter / (area_i + area_j - inter)).astype(T)
        iou = np.where((area_i <= 0) | (area_j <= 0), T(0), iou).astype(T)
        if kind == "iou":
            return iou
        dy = (T(0.5) * (y0 + y1) - T(0.5) * (oy0 + oy1)).astype(T)
        dx = (T(0.5) * (x0 + x1) - T(0.5) * (ox0 + ox1)).astype(T)
        d2 = (dy * dy + dx * dx).astype(T)
        ey = (np.maximum(y1, oy1) - np.minimum(y0, oy0)).astype(T)
        ex = (np.maximum(x1, ox1) - np.minimum(x0, ox0)).astype(T)
        c2 = (ey * ey + ex * ex).astype(T)
        q = (d2 / c2).astype(T)
        pen = q if float(beta) == 1.0 else np.power(q, T(beta)).astype(T)
        return np.where(c2 == 0, iou, (iou - pen).astype(T)).astype(T)


def combined_nms_rule(boxes, scores, per_class=100, total=100, iou_thr=0.413, score_thr=0.3, kind="iou", beta=1.0,
                      agnostic=False):
    """boxes [N, nbox, 4] normalised, scores [N, nbox, C] -> (nmsed_boxes [N, T, 4] clipped, nmsed_scores [N, T], nmsed_classes
    [N, T], valid [N] int32, kept_idx [N, T] int32 (-1 padded), min_margin)."""
    assert kind in KINDS and np.isfinite(beta) and beta > 0
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    n, nbox, ncls = scores.shape
    T = total
    thr32, sthr = F32(iou_thr), F32(score_thr)
    thr64 = np.float64(thr32)
    out_b = np.zeros((n, T, 4), F32); out_s = np.zeros((n, T), F32)
    out_c = np.zeros((n, T), F32); out_v = np.zeros((n,), np.int32)
    out_i = np.full((n, T), -1, np.int32)
    margin = np.inf
    for b in range(n):
        sc = scores[b]
        bi, ci = np.nonzero(sc > sthr)
        order = np.lexsort((ci, bi, -sc[bi, ci].astype(np.float64)))
        kept_box, kept_cls = [], []
        count = np.zeros(ncls, np.int64)
        k = 0
        for i, c in zip(bi[order], ci[order]):
            if k >= T:
                break
            if count[c] >= per_class:
                continue                                   # turned away by its class's cap: not kept, suppresses nothing
            against = kept_box if agnostic else [kb for kb, kc in zip(kept_box, kept_cls) if kc == c]
            if against:
                m32 = measure(boxes[b, i], boxes[b, against], kind, beta, F32)
                m64 = measure(boxes[b, i], boxes[b, against], kind, beta, np.float64)
                with np.errstate(invalid="ignore"):
                    d = np.concatenate([np.abs(m32.astype(np.float64) - thr64), np.abs(m64 - thr64)])
                d = d[np.isfinite(d)]
                if d.size:
                    margin = min(margin, float(d.min()))
                if np.any(m32 > thr32):
                    continue
            kept_box.append(int(i)); kept_cls.append(int(c))
            count[c] += 1
            out_b[b, k] = np.clip(boxes[b, i], F32(0), F32(1))
            out_s[b, k] = sc[i, c]; out_c[b, k] = c; out_i[b, k] = i
            k += 1
        out_v[b] = k
    return out_b, out_s, out_c, out_v, out_i, margin
