"""Test oracle of test-time augmentation (y4_view_u8_ragged, y4_decode_gather_views, Engine.predict_tta): NumPy only, built on
tests/tiled_oracle.py and tests/merge_oracle.py by import.

A view's map may have a negative scale (the canvas is mirrored).  `map_boxes_oriented` is tiled_oracle.map_boxes behind the corner
swap y4_decode_gather_views makes: an axis whose scale is negative reads its two corners exchanged, so a box with x1 <= x2 keeps
x1' <= x2'.  `gathered_nms` is tiled_oracle.gathered_nms on tables mapped that way; `merged` hands such tables to
merge_oracle.merged_nms.  `view_host` is the host restatement of one slot of y4_view_u8_ragged: the row of marker_photos.place_row
(prepost.resize_bilinear onto a pad canvas), then np.flip of the whole canvas along the flipped axes."""
import numpy as np

import decode_nms_cases as DC
import marker_photos as MP
import merge_oracle as MO
import nms_rule_oracle as NR
import tiled_oracle as TO


def oriented(boxes, m):
    """boxes [..., 4] with the corners an axis of negative scale reads exchanged (m = ax, bx, ay, by)."""
    b = np.array(boxes, np.float32, copy=True)
    m = np.asarray(m, np.float32)
    if m[0] < 0:
        b[..., [0, 2]] = b[..., [2, 0]]
    if m[2] < 0:
        b[..., [1, 3]] = b[..., [3, 1]]
    return b


def map_boxes_oriented(boxes, m):
    return TO.map_boxes(oriented(boxes, m), m)


def unoriented(boxes, m):
    """The negative control: the plain map of y4_decode_gather, which stores x1 > x2 under a negative scale."""
    return TO.map_boxes(boxes, m)


def group_tables(heads, maps, ncls, cfg, size, mapper=map_boxes_oriented):
    """tiled_oracle.group_tables with the oriented map: -> (boxes [1, T * nbox, 4], scores [1, T * nbox, C])."""
    with np.errstate(over="ignore", invalid="ignore"):
        b, s = DC.boxes_and_scores(heads, ncls, cfg, size)
    b = np.stack([mapper(b[t], maps[t]) for t in range(b.shape[0])])
    return b.reshape(1, -1, 4), np.asarray(s, np.float32).reshape(1, -1, ncls)


def gathered_nms(groups, ncls, cfg, size, iou_thr, score_thr, kind="iou", beta=1.0, agnostic=False, per_class=100, total=100):
    """tiled_oracle.gathered_nms under oriented maps: -> (boxes, scores, classes, valid, kept_idx, min_margin, counts [G])."""
    outs, counts, margin = [], [], np.inf
    for heads, maps in groups:
        b, s = group_tables(heads, maps, ncls, cfg, size)
        r = NR.combined_nms_rule(b, s, per_class, total, iou_thr, score_thr, kind, beta, agnostic)
        outs.append(r[:5])
        margin = min(margin, r[5])
        counts.append(TO.candidate_count(s, score_thr))
    return tuple(np.concatenate([o[i] for o in outs], axis=0) for i in range(5)) + (margin, np.asarray(counts, np.int64))


def merged(tables_b, tables_s, iou_thr, score_thr, kind="iou", beta=1.0, agnostic=False):
    """merge_oracle.merged_nms over group tables [G, T * nbox, 4 / C] (the oracle's, or the device's own read back)."""
    return MO.merged_nms(tables_b, tables_s, 100, 100, iou_thr, score_thr, kind, beta, agnostic)


def cross_view_suppressions(boxes, scores, result, nbox, iou_thr, score_thr, kind="iou", beta=1.0, agnostic=False):
    """For one group's table (boxes [T * nbox, 4], scores [T * nbox, C]) and its NMS result (the five arrays, one group): the
    number of candidates above the lowest kept score that are not kept and whose every suppressor -- a kept box of higher score,
    of its class (any class when agnostic), with measure > threshold -- comes from ANOTHER slot."""
    b, s, c, v, k = (np.asarray(a)[0] for a in result[:5])
    v = int(v)
    kept = [(int(k[i]), int(c[i]), np.float32(s[i])) for i in range(v)]
    kept_ids = {(bi, ci) for bi, ci, _ in kept}
    bi, ci = np.nonzero(np.asarray(scores, np.float32) > np.float32(score_thr))
    count = 0
    for j, cj in zip(bi.tolist(), ci.tolist()):
        sj = np.float32(scores[j, cj])
        if (j, cj) in kept_ids or v == 0 or sj <= kept[-1][2]:
            continue
        sup = [kb for kb, kc, ks in kept if ks > sj and (agnostic or kc == cj)]
        if not sup:
            continue
        m = NR.measure(boxes[j], boxes[sup], kind, beta, np.float32)
        hit = [kb for kb, mm in zip(sup, m) if mm > np.float32(iou_thr)]
        if hit and all(kb // nbox != j // nbox for kb in hit):
            count += 1
    return count


def view_host(photo, window, rect, flip_bits, canvas_hw, pad=MP.PAD):
    """One slot of y4_view_u8_ragged on the host: marker_photos.place_row, then np.flip along the flipped axes (bit 0: columns,
    bit 1: rows) of the whole canvas, padding included."""
    canvas = MP.place_row(photo, window, rect, canvas_hw, pad)
    if flip_bits & 1:
        canvas = canvas[:, ::-1]
    if flip_bits & 2:
        canvas = canvas[::-1]
    return np.ascontiguousarray(canvas)


def canvas_box(box_px, window, rect, flip_bits, canvas_hw):
    """A box (x1, y1, x2, y2) in photo pixels -> canvas pixels under a view, in float64, corners ordered: x -> (x - x0) out_w / ww +
    pad_left, mirrored to W - x under bit 0; y likewise."""
    H, W = canvas_hw
    y0, x0, wh, ww = window
    out_h, out_w, top, left = rect
    xs = [(float(v) - x0) * out_w / ww + left for v in (box_px[0], box_px[2])]
    ys = [(float(v) - y0) * out_h / wh + top for v in (box_px[1], box_px[3])]
    if flip_bits & 1:
        xs = [W - v for v in xs]
    if flip_bits & 2:
        ys = [H - v for v in ys]
    return np.array([min(xs), min(ys), max(xs), max(ys)], np.float64)


def photo_box(rect_px, canvas_hw, m, photo_hw):
    """A rectangle in canvas pixel edges -> photo pixels through a view's map with the corner swap (marker_photos.mapped_rect for
    maps that may mirror)."""
    H, W = canvas_hw
    b = np.array([rect_px[0] / W, rect_px[1] / H, rect_px[2] / W, rect_px[3] / H], np.float32)
    return map_boxes_oriented(b, m).astype(np.float64) * np.array([photo_hw[1], photo_hw[0], photo_hw[1], photo_hw[0]], np.float64)
