"""The matching rule of `evalmap.eval_map` (reference models.py:282-330) restated per image, as `y4_map_match` is specified:
float32 inputs widened exactly to Python floats, Python float arithmetic in `_iou_inclusive`'s own expression order.

`match_image` is what one workgroup of the kernel computes for one image; `eval_map` itself walks the detections of a CLASS
over all images, but a detection only ever meets the ground truth of its own image and class, and within one image the walk
order of a class is confidence descending with ties in line (= slot) order -- so the per-image walk below visits every
(image, class) subsequence in `eval_map`'s order and takes the same decisions."""
import numpy as np


def pixel_boxes(boxes_norm, scale):
    """[k, 4] normalised float32 boxes and (w, h) -> float32 pixel boxes: export_prediction's `boxes[:, [0, 2]] *= w`, a float32
    product."""
    b = np.array(boxes_norm, dtype=np.float32).reshape(-1, 4).copy()
    b[:, [0, 2]] *= np.float32(scale[0])
    b[:, [1, 3]] *= np.float32(scale[1])
    return b


def iou_inclusive(bb, gt):
    iw = min(bb[2], gt[2]) - max(bb[0], gt[0]) + 1
    ih = min(bb[3], gt[3]) - max(bb[1], gt[1]) + 1
    if iw <= 0 or ih <= 0:
        return -1.0
    union = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (gt[2] - gt[0] + 1) * (gt[3] - gt[1] + 1) - iw * ih
    return iw * ih / union


def match_image(boxes_px, scores, classes, gt, thresholds):
    """boxes_px float32 [k, 4], scores [k], classes [k] (the valid slots only); gt float32 [m, 5] (the counted rows only);
    thresholds: floats.  -> (tp_mask uint32 [k], best_iou float64 [k], match int32 [k], gt_used uint32 [m])."""
    k, m = len(scores), len(gt)
    bb = [[float(v) for v in row] for row in np.asarray(boxes_px, dtype=np.float32).reshape(k, 4)]
    gg = [[float(v) for v in row[:4]] for row in np.asarray(gt, dtype=np.float32).reshape(m, 5)]
    gcls = [int(row[4]) for row in np.asarray(gt, dtype=np.float32).reshape(m, 5)]
    conf = [float(np.float32(s)) for s in scores]
    best_iou, match = np.full(k, -1.0, dtype=np.float64), np.full(k, -1, dtype=np.int32)
    for d in range(k):
        best, hit = -1.0, -1
        for g in range(m):
            if gcls[g] != int(classes[d]):
                continue
            ov = iou_inclusive(bb[d], gg[g])
            if ov > best:
                best, hit = ov, g
        best_iou[d], match[d] = best, hit
    order = sorted(range(k), key=lambda d: conf[d], reverse=True)          # stable: slot order on ties
    tp_mask, gt_used = np.zeros(k, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    for t, thr in enumerate(thresholds):
        used = [False] * m
        for d in order:
            if best_iou[d] >= thr and not used[match[d]]:
                used[match[d]] = True
                tp_mask[d] |= np.uint32(1 << t)
        for g in range(m):
            if used[g]:
                gt_used[g] |= np.uint32(1 << t)
    return tp_mask, best_iou, match, gt_used
