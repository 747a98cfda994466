"""Test oracle of the gathered decode + NMS (y4_decode_gather, y4_nms_gathered): NumPy only.

A group is a list of rows (slots), each with its raw heads and a map {ax, bx, ay, by}.  Every row is decoded with the project's
decode oracle (decode_nms_cases.boxes_and_scores), its boxes are mapped to the group's coordinates -- x1, x2 -> float32(float64(x)
* ax + bx), y likewise: the product of two float32 values is exact in float64, so this is the device's fmaf up to one double
rounding of the sum --, the slots are concatenated along the box axis into [1, T * nbox, ...], and the NMS pair-rule oracle
(nms_rule_oracle.combined_nms_rule) runs on that: candidates by score descending, then slot * nbox + box, then class; the measure
on the MAPPED boxes; kept_idx = slot * nbox + box."""
import numpy as np

import decode_nms_cases as DC
import nms_rule_oracle as NR


def map_boxes(boxes, m):
    """boxes [..., 4] float32 (x1, y1, x2, y2), m = (ax, bx, ay, by) float32 -> float32(float64(v) * a + b), unclipped."""
    b = np.asarray(boxes, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    out = np.empty_like(b)
    out[..., 0::2] = b[..., 0::2] * m[0] + m[1]
    out[..., 1::2] = b[..., 1::2] * m[2] + m[3]
    return out.astype(np.float32)


def group_tables(heads, maps, ncls, cfg, size):
    """heads: 3 arrays [T, g, g, 3 (5 + C)] (one row per slot), maps [T, 4] -> (boxes [1, T * nbox, 4] mapped, scores [1, T * nbox, C])."""
    with np.errstate(over="ignore", invalid="ignore"):
        b, s = DC.boxes_and_scores(heads, ncls, cfg, size)
    b = np.stack([map_boxes(b[t], maps[t]) for t in range(b.shape[0])])
    return b.reshape(1, -1, 4), np.asarray(s, np.float32).reshape(1, -1, ncls)


def candidate_count(scores, score_thr):
    return int((np.asarray(scores, np.float32) > np.float32(score_thr)).sum())


def gathered_nms(groups, ncls, cfg, size, iou_thr, score_thr, kind="iou", beta=1.0, agnostic=False, per_class=100, total=100):
    """groups: a list of (heads of the group's rows in slot order, maps [T, 4]) -> (boxes [G, total, 4], scores, classes, valid,
    kept_idx, min_margin over all groups, candidate count per group [G])."""
    outs, counts, margin = [], [], np.inf
    for heads, maps in groups:
        b, s = group_tables(heads, maps, ncls, cfg, size)
        r = NR.combined_nms_rule(b, s, per_class, total, iou_thr, score_thr, kind, beta, agnostic)
        outs.append(r[:5])
        margin = min(margin, r[5])
        counts.append(candidate_count(s, score_thr))
    return tuple(np.concatenate([o[i] for o in outs], axis=0) for i in range(5)) + (margin, np.asarray(counts, np.int64))
