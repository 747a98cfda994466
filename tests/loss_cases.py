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


def _random_boxes(rng, m, hw, ncls, side_range=None):
    H, W = hw
    lo, hi = side_range or (8.0, 0.9 * min(H, W))
    side = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(m, 1)))
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


def _package_on_path():
    import sys
    import os
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolo-v4-tf.keras_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)


def make_case(name):
    """-> dict(hw, ncls, n, boxes [n, 100, 5], heads [3 arrays], sha: a checksum of the inputs)."""
    _package_on_path()
    from yolo4hip.data import records_from_boxes
    c = CASES[name]
    boxes = make_boxes(c["hw"], c["ncls"], c["n"], c["seed"])
    records, _ = records_from_boxes(boxes, c["hw"], ANCHORS, c["ncls"])
    heads = make_heads(c["hw"], c["ncls"], c["n"], c["seed"], records, c.get("wide", False))
    sha = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in [boxes] + heads)).hexdigest()
    return dict(hw=c["hw"], ncls=c["ncls"], n=c["n"], boxes=boxes, heads=heads, sha=sha)


# ---- label geometry: max_boxes and class counts beside 100 and {3, 80} (tests/test_label_shapes_cpu.py, tests/test_gpu_label_shapes.py)
WAVE = 64                                                                 # rows of one wave of the label kernels (one row per thread)
# name -> input (H, W), classes, images, max_boxes, seed; `classes`: class ids some record must carry (the first rows of the full
# image get them); `trio`: the classes of the three rows on one (scale, cell, anchor) of image 3.  The seeds are the first ones
# whose case passes check_case (tests/golden/make_loss_fixtures.py --seeds).
LABEL_CASES = {
    "mb1_c1": dict(hw=(160, 160), ncls=1, n=4, max_boxes=1, seed=1, classes=(0,)),
    "mb64_c32": dict(hw=(160, 160), ncls=32, n=4, max_boxes=64, seed=1, classes=(31,)),
    "mb65_c33": dict(hw=(160, 160), ncls=33, n=4, max_boxes=65, seed=1, classes=(32,)),
    "mb129_c64": dict(hw=(160, 160), ncls=64, n=4, max_boxes=129, seed=6, classes=(31, 32, 63), trio=(31, 32, 63)),
    "mb256_c65": dict(hw=(160, 160), ncls=65, n=4, max_boxes=256, seed=16, classes=(63, 64), trio=(0, 63, 64)),
}
# box sides that the anchors of scale 0 / 1 / 2 win (the one-row case puts one box on every scale)
SCALE_SIDES = ((8.0, 28.0), (48.0, 80.0), (112.0, 140.0))


def degenerate_rows(max_boxes):
    """The rows of image 2 that get w = 0: row 7 of every wave that holds a row in front of the array's last one (a degenerate
    LAST row would have no valid row behind it); none below 65 rows."""
    return [] if max_boxes <= WAVE else [w * WAVE + 7 for w in range((max_boxes - 2) // WAVE + 1)]


def trio_rows(max_boxes):
    """The three rows of image 3 that share one (scale, cell, anchor): in the first wave, the last but one wave and the last wave
    (-> None below three waves)."""
    waves = (max_boxes - 1) // WAVE + 1
    if waves < 3:
        return None
    last = max_boxes - 1
    return (5, (waves - 2) * WAVE + 5, last - min(5, last % WAVE))


def make_label_boxes(hw, ncls, n, seed, max_boxes, classes=(), trio=None):
    """[n, max_boxes, 5] float32.  Image 0 has no box; image 1 exactly max_boxes, its first rows of the classes `classes`; image 2
    (65 rows and more) every row filled and the rows degenerate_rows() degenerate (w = 0), so that the k-th valid row lies further
    behind row k wave by wave and the last valid rows are dropped; image 3 (three waves and more) every row filled and the rows
    trio_rows() one box of three classes, the last one a pixel wider -- with fewer rows the two-class collision of make_boxes, the
    first of them of the last class.  One row: images 1 .. 3 carry one box each, sized for scale 0, 1 and 2."""
    assert n == 4
    rng = np.random.default_rng(seed)
    mb = max_boxes
    boxes = np.zeros((n, mb, 5), dtype=np.float32)
    if mb == 1:
        for i in (1, 2, 3):
            boxes[i] = _random_boxes(rng, 1, hw, ncls, SCALE_SIDES[i - 1])
        return boxes
    boxes[1] = _random_boxes(rng, mb, hw, ncls)
    boxes[1, :len(classes), 4] = classes
    deg = degenerate_rows(mb)
    if deg:
        boxes[2] = _random_boxes(rng, mb, hw, ncls)
        boxes[2, deg, 2] = boxes[2, deg, 0]
    else:
        m = int(rng.integers(6, 16))
        boxes[2, :m] = _random_boxes(rng, m, hw, ncls)
        boxes[2, 3, 2] = boxes[2, 3, 0]
    rows = trio_rows(mb)
    if rows:
        boxes[3] = _random_boxes(rng, mb, hw, ncls)
        for k, cls in zip(rows, trio):
            boxes[3, k] = boxes[3, rows[0]]
            boxes[3, k, 4] = cls
        boxes[3, rows[2], 2] += 1.0                                       # (the last one's xywh differs and must win)
    else:
        m = int(rng.integers(6, 16))
        boxes[3, :m] = _random_boxes(rng, m, hw, ncls)
        boxes[3, 1, 4] = ncls - 1
        boxes[3, m] = boxes[3, 1]
        boxes[3, m, 4] = 0
        boxes[3, m, 2] += 1.0
    return boxes


def make_label_case(name, seed=None):
    """-> dict(hw, ncls, n, max_boxes, boxes [n, max_boxes, 5], records (host assignment per image), true_xywh, heads, sha)."""
    _package_on_path()
    from yolo4hip.data import records_from_boxes
    c = LABEL_CASES[name]
    seed = c["seed"] if seed is None else seed
    boxes = make_label_boxes(c["hw"], c["ncls"], c["n"], seed, c["max_boxes"], c["classes"], c.get("trio"))
    records, xywh = records_from_boxes(boxes, c["hw"], ANCHORS, c["ncls"])
    heads = make_heads(c["hw"], c["ncls"], c["n"], seed, records)
    sha = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in [boxes] + heads)).hexdigest()
    return dict(hw=c["hw"], ncls=c["ncls"], n=c["n"], max_boxes=c["max_boxes"], boxes=boxes, records=records, true_xywh=xywh,
                heads=heads, sha=sha)


def _has_class(rec, cls):
    return bool(((rec[:, 8 + cls // 32].view(np.uint32) >> np.uint32(cls % 32)) & 1).any()) if len(rec) else False


def _key_of_row(row, hw, ncls):
    """(scale, row, col, anchor) a box gets when it is alone in its image"""
    from yolo4hip.data import records_from_boxes
    rec, _ = records_from_boxes(row.reshape(1, 1, 5), hw, ANCHORS, ncls)
    return tuple(int(v) for v in rec[0][0, 0:4])


def check_case(name, case=None):
    """Every condition a label case is there for, as assertions -> facts about it (for the tests' notes)."""
    import loss_oracle as LO
    from yolo4hip.data import dense_from_records
    c = LABEL_CASES[name]
    case = make_label_case(name) if case is None else case
    hw, ncls, n, mb = c["hw"], c["ncls"], c["n"], c["max_boxes"]
    boxes, recs = case["boxes"], case["records"]
    assert boxes.shape == (n, mb, 5) and boxes.dtype == np.float32
    assert np.array_equal(boxes[..., 0:4] * 1024.0, np.round(boxes[..., 0:4] * 1024.0))      # snapped to 2^-10
    assert all(np.array_equal(h * 1024.0, np.round(h * 1024.0)) for h in case["heads"])
    valid = boxes[..., 2] - boxes[..., 0] > 0
    # full image, empty image
    assert not valid[0].any() and len(recs[0]) == 0
    assert valid[1].all() and all(len(r) <= mb for r in recs)
    waves = (mb - 1) // WAVE + 1
    assert sorted(set(np.flatnonzero(valid[1]) // WAVE)) == list(range(waves))              # valid rows in every wave
    # the class bits
    for cls in c["classes"]:
        assert 0 <= cls < ncls and any(_has_class(r, cls) for r in recs), cls
    # many records: they reach wave 3 of map_records
    if name == "mb256_c65":
        assert len(recs[1]) >= 3 * WAVE + 1, len(recs[1])
    # degenerate rows
    deg = degenerate_rows(mb)
    if mb > WAVE:
        v = valid[2]
        assert deg and [k // WAVE for k in deg] == list(range((mb - 2) // WAVE + 1))
        assert not v[deg].any() and int(v.sum()) == mb - len(deg) and v[deg[-1] + 1:].any() and v[0]
        vidx = np.flatnonzero(v)                                             # thread k reads the (w, h) of row vidx[k]
        shift = vidx - np.arange(len(vidx))
        assert sorted(set(shift.tolist())) == list(range(len(deg) + 1))     # the shift grows by one behind every degenerate row
        assert (vidx // WAVE > np.arange(len(vidx)) // WAVE).any()          # ... and across a wave border
        assert len(recs[2]) <= len(vidx) and len(vidx) < mb                 # the last rows are dropped
    # equal keys across waves
    rows = trio_rows(mb)
    assert (rows is not None) == (mb > 2 * WAVE)
    if rows:
        assert valid[3].all() and len({k // WAVE for k in rows}) == 3
        keys = [_key_of_row(boxes[3, k], hw, ncls) for k in rows]
        assert keys[0] == keys[1] == keys[2], keys
        assert len({int(boxes[3, k, 4]) for k in rows}) == 3 and tuple(int(boxes[3, k, 4]) for k in rows) == c["trio"]
        assert not np.array_equal(boxes[3, rows[2], 0:4], boxes[3, rows[0], 0:4])
        hit = [r for r in recs[3] if tuple(int(x) for x in r[0:4]) == keys[0]]
        assert len(hit) == 1
        want = np.concatenate(((boxes[3, rows[2], 0:2] + boxes[3, rows[2], 2:4]) // 2, boxes[3, rows[2], 2:4] - boxes[3, rows[2], 0:2]))
        assert np.array_equal(hit[0][4:8].view(np.float32), want.astype(np.float32))        # the last row's xywh ...
        assert all(_has_class(hit[0][None], cls) for cls in c["trio"])                        # ... and every row's class
    elif mb > 1:
        assert any((np.array([bin(int(w) & 0xFFFFFFFF).count("1") for w in r[8:]]).sum() > 1) for r in recs[3])
    # wide grids: a width that is no multiple of the strips of the gradient kernels
    assert any((hw[1] // s) % 16 and (hw[1] // s) % 64 for s in STRIDES)
    # every scale is used, has an ignore region, and no lane is within 1e-4 of the ignore threshold
    labels = dense_from_records(recs, hw, ncls)
    anchors3 = ANCHORS.reshape(3, 3, 2)
    ignore = []
    for s in range(3):
        _, max_iou, respond = LO.scale_terms(case["heads"][s], labels[s], case["true_xywh"], anchors3[s], STRIDES[s], ncls,
                                             IOU_LOSS_THRESH, float(hw[0] * hw[1]))
        assert respond.sum() > 0, f"scale {s} has no responsible cell"
        ignore.append(int(((respond == 0) & (max_iou >= IOU_LOSS_THRESH)).sum()))
        assert ignore[-1] > 0, f"scale {s}: empty ignore region"
        near = int((np.abs(max_iou - IOU_LOSS_THRESH) < 1e-4).sum())
        assert near == 0, f"scale {s}: {near} lanes within 1e-4 of the ignore threshold"
    return dict(records=[len(r) for r in recs], valid=valid.sum(axis=1).tolist(), ignore=ignore, degenerate=deg, trio=rows)
