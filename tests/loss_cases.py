"""Inputs of the loss tests, from seeds (shared by tests/golden/make_loss_fixtures.py and the tests, so that the fixture
files hold results only).  Heads look like a detector's: confidence shifted negative, narrow wh logits, about half of the
responsible cells near their labels and some neighbouring anchors predicting a labelled box too (the ignore region).  Every
generated value is snapped to a multiple of 2^-10, so that a last-bit difference of some libm does not move an input."""
import hashlib

import numpy as np

ANCHORS = np.array([12, 16, 19, 36, 40, 28, 36, 75, 76, 55, 72, 146, 142, 110, 192, 243, 459, 401]).reshape(9, 2)
STRIDES = (8, 16, 32)
MAX_BOXES = 100
IOU_LOSS_THRESH = 0.5
# name -> input (H, W), classes, images, seed.  The seeds are the first ones whose case passes every assertion of the
# generator (check_case there), the 1e-4 clearance of the ignore threshold included.
CASES = {
    "416_bccd": dict(hw=(416, 416), ncls=3, n=4, seed=1),
    "160_coco": dict(hw=(160, 160), ncls=80, n=4, seed=2),
    # heads far outside the range a freshly initialised detector produces (make_heads(wide=True)): saturating confidence and class
    # logits, xy at the cell borders, boxes from a fraction of a pixel to thousands of pixels
    "160_wide": dict(hw=(160, 160), ncls=3, n=4, seed=1, wide=True),
}


def _snap(x):
    return (np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0).astype(np.float32)


def _random_boxes(rng, m, hw, ncls):
    H, W = hw
    side = np.exp(rng.uniform(np.log(8.0), np.log(0.9 * min(H, W)), size=(m, 1)))
    wh = np.minimum(side * np.exp(rng.uniform(-0.5, 0.5, size=(m, 2))), [W - 2.0, H - 2.0])
    ctr = rng.uniform(0.0, 1.0, size=(m, 2)) * ([W, H] - wh) + wh / 2
    out = np.zeros((m, 5), dtype=np.float32)
    out[:, 0:2] = _snap(ctr - wh / 2)
    out[:, 2:4] = _snap(ctr + wh / 2)
    out[:, 4] = rng.integers(0, ncls, size=m)
    return out


def make_boxes(hw, ncls, n, seed, max_boxes=MAX_BOXES):
    """[n, max_boxes, 5] float32.  Image 0 has no box, image 1 exactly max_boxes, image 2 a degenerate (w = 0) row between
    valid rows, image 3 two boxes of different classes on one cell and anchor; further images a few boxes each."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((n, max_boxes, 5), dtype=np.float32)
    for i in range(1, n):
        m = max_boxes if i == 1 else int(rng.integers(6, 16))
        boxes[i, :m] = _random_boxes(rng, m, hw, ncls)
        if i == 2:
            boxes[i, 3, 2] = boxes[i, 3, 0]                              # w = 0, the rows behind it stay valid
        if i == 3:
            boxes[i, m] = boxes[i, 1]                                    # the same box once more ...
            boxes[i, m, 4] = (boxes[i, 1, 4] + 1) % ncls                 # ... as another class
            boxes[i, m, 2] += 1.0                                        # (the later one's xywh differs and must win)
    return boxes


def _make_heads_wide(hw, ncls, n, seed, records):
    """The heads of a net whose logits left the range of order 1: confidence and class logits uniform over +-40 on every lane, the
    responsible ones included (so both the right and the wrong sign occur there, saturated), xy logits over +-20 and wh logits over
    +-8 -- around the label's value on the lanes that predict a labelled box, half of which stay near their label as in make_heads
    (the ignore region and a box term that is not all saturation)."""
    rng = np.random.default_rng(seed + 1000)
    heads = []
    for s, stride in enumerate(STRIDES):
        gh, gw = hw[0] // stride, hw[1] // stride
        t = np.empty((n, gh, gw, 3, 5 + ncls))
        t[..., 0:2] = rng.uniform(-20.0, 20.0, size=t[..., 0:2].shape)
        t[..., 2:4] = rng.uniform(-8.0, 8.0, size=t[..., 2:4].shape)
        t[..., 4:] = rng.uniform(-40.0, 40.0, size=t[..., 4:].shape)
        heads.append(t)
    for b, rec in enumerate(records):
        for r in rec:
            s, row, col, a = (int(v) for v in r[0:4])
            x, y, w, h = r[4:8].view(np.float32).astype(np.float64)
            if w <= 0 or h <= 0:
                continue
            u = rng.uniform(size=3)
            picks = [a] if u[0] < 0.75 else []
            if u[1] < 0.5:
                picks.append((a + 1) % 3)
            for q in picks:
                t = heads[s][b, row, col, q]
                off = np.clip(np.array([x / STRIDES[s] - col, y / STRIDES[s] - row]), 0.05, 0.95)
                near = u[2] < 0.5
                t[0:2] = np.log(off / (1 - off)) + rng.normal(0.0, 0.3, size=2) if near else rng.uniform(-20.0, 20.0, size=2)
                t[2:4] = np.log(np.array([w, h]) / ANCHORS[3 * s + q]) + (rng.normal(0.0, 0.15, size=2) if near else rng.uniform(-8.0, 8.0, size=2))
    out = []
    for t in heads:
        t[..., 0:2] = np.clip(t[..., 0:2], -20.0, 20.0)
        t[..., 4:] = np.clip(t[..., 4:], -40.0, 40.0)
        out.append(_snap(t).reshape(t.shape[:3] + (3 * (5 + ncls),)))
    return out


def make_heads(hw, ncls, n, seed, records, wide=False):
    """Three float32 heads [n, gh, gw, 3 (5 + C)]; `records` (per image, yolo4hip.data format) say where the labels are."""
    if wide:
        return _make_heads_wide(hw, ncls, n, seed, records)
    rng = np.random.default_rng(seed + 1000)
    heads = []
    for s, stride in enumerate(STRIDES):
        gh, gw = hw[0] // stride, hw[1] // stride
        t = rng.normal(0.0, 1.0, size=(n, gh, gw, 3, 5 + ncls))
        t[..., 2:4] *= 0.3
        t[..., 4] = t[..., 4] * 1.5 - 4.0
        t[..., 5:] = t[..., 5:] * 1.5 - 2.0
        heads.append(t)
    for b, rec in enumerate(records):
        for r in rec:
            s, row, col, a = (int(v) for v in r[0:4])
            x, y, w, h = r[4:8].view(np.float32).astype(np.float64)
            if w <= 0 or h <= 0:
                continue
            u = rng.uniform(size=2)
            picks = [a] if u[0] < 0.5 else []
            if u[1] < 0.5:
                picks.append((a + 1) % 3)                                # a neighbouring anchor that predicts the labelled box
            for q in picks:
                t = heads[s][b, row, col, q]
                off = np.clip(np.array([x / STRIDES[s] - col, y / STRIDES[s] - row]), 0.05, 0.95)
                t[0:2] = np.log(off / (1 - off)) + rng.normal(0.0, 0.3, size=2)
                t[2:4] = np.log(np.array([w, h]) / ANCHORS[3 * s + q]) + rng.normal(0.0, 0.15, size=2)
                if q == a:
                    t[4] = rng.normal(1.0, 1.0)
                    t[5:][np.nonzero([(int(r[8 + c // 32]) >> (c % 32)) & 1 for c in range(ncls)])[0]] += 3.0
    return [_snap(np.clip(t, -12.0, 12.0)).reshape(t.shape[:3] + (3 * (5 + ncls),)) for t in heads]


def make_case(name):
    """-> dict(hw, ncls, n, boxes [n, 100, 5], heads [3 arrays], sha: a checksum of the inputs)."""
    import sys
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolo-v4-tf.keras_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from yolo4hip.data import records_from_boxes
    c = CASES[name]
    boxes = make_boxes(c["hw"], c["ncls"], c["n"], c["seed"])
    records, _ = records_from_boxes(boxes, c["hw"], ANCHORS, c["ncls"])
    heads = make_heads(c["hw"], c["ncls"], c["n"], c["seed"], records, c.get("wide", False))
    sha = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in [boxes] + heads)).hexdigest()
    return dict(hw=c["hw"], ncls=c["ncls"], n=c["n"], boxes=boxes, heads=heads, sha=sha)
