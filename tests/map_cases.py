"""Crafted images for the VOC mAP matching (`y4_map_match`, `mapeval.MapAccumulator`), as one small dataset.

Every pixel coordinate is a multiple of 0.25 below 4096 and every score a multiple of 1/1024: their shortest decimal form is
exact, so a trip through the text files of `export_gt` / `export_prediction` changes no value and the file pipeline
(`evalmap.eval_map`) sees exactly the numbers the device sees.  All images share max_total = 100 slots and max_gt = 256 rows;
slots >= valid and rows >= gt_count are NaN.  An image's name is its stem in that pipeline; "a-b" and "a" pin the image order
(`sorted(glob)` orders "a-b.txt" before "a.txt")."""
import numpy as np

MAX_TOTAL, MAX_GT = 100, 256
# ids 0..2 carry most ground truth; 3 ("kiwi") has ground truth in one image only; 4 ("date") has none anywhere.  The names are
# out of id order on purpose: the classes are walked sorted by NAME
CLASS_NAMES = ["pear", "apple", "fig", "kiwi", "date"]
THRESHOLD_SETS = {1: (0.5,), 10: tuple(float(t) for t in np.arange(0.5, 1.0, 0.05)),
                  16: tuple(float(t) for t in np.linspace(0.2, 0.95, 16))}


def _case(stem, dets, gts, scale=(1.0, 1.0), normalised=False):
    """dets: rows (x1, y1, x2, y2, score, class) in pixels (or already normalised); gts: rows (x1, y1, x2, y2, class)."""
    boxes = np.full((MAX_TOTAL, 4), np.nan, dtype=np.float32)
    scores = np.full(MAX_TOTAL, np.nan, dtype=np.float32)
    classes = np.full(MAX_TOTAL, np.nan, dtype=np.float32)
    gt = np.full((MAX_GT, 5), np.nan, dtype=np.float32)
    d = np.array(dets, dtype=np.float64).reshape(-1, 6)
    g = np.array(gts, dtype=np.float64).reshape(-1, 5)
    assert len(d) <= MAX_TOTAL and len(g) <= MAX_GT
    if not normalised:
        assert scale == (1.0, 1.0)
    boxes[:len(d)], scores[:len(d)], classes[:len(d)] = d[:, :4], d[:, 4], d[:, 5]
    gt[:len(g)] = g
    px = boxes[:len(d)] * np.array([scale[0], scale[1], scale[0], scale[1]], dtype=np.float32)
    for a in (px * 4, gt[:len(g), :4] * 4, scores[:len(d)] * 1024):        # the exactness the docstring promises
        assert np.all(a == np.round(a)) and np.all(np.abs(a) < 4096 * 4)
    return {"stem": stem, "boxes": boxes, "scores": scores, "classes": classes, "valid": len(d), "gt": gt, "gt_count": len(g),
            "scale": (float(scale[0]), float(scale[1]))}


def _full():
    """valid = max_total = 100 on 256 ground-truth rows of 3 classes in a 600 x 600 field: crowded rows, several detections
    per row, many score ties, some detections of the wrong class."""
    rng = np.random.default_rng(20240)
    gts = []
    for _ in range(MAX_GT):
        x1, y1 = 8 + rng.integers(0, 2400, 2) / 4
        w, h = rng.integers(40, 800, 2) / 4
        gts.append((x1, y1, x1 + w, y1 + h, int(rng.integers(0, 3))))
    dets = []
    for _ in range(MAX_TOTAL):
        x1, y1, x2, y2, c = gts[int(rng.integers(0, MAX_GT))]
        j = rng.integers(-16, 17, 4) / 4
        cls = c if rng.random() < 0.8 else int(rng.integers(0, 3))
        dets.append((x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3], int(rng.integers(1, 64)) / 64, cls))
    return _case("full", dets, gts)


def cases():
    out = [
        _case("no_det", [], [(10, 10, 50, 50, 0), (60, 60, 90, 90, 1)]),
        _case("no_gt", [(10, 10, 50, 50, 0.75, 0), (12, 10, 50, 50, 0.5, 1), (0, 0, 5, 5, 0.25, 2)], []),
        _case("nothing", [], []),
        _full(),
        # scores out of slot order, with ties: the walk is by score, then slot.  Slots 1 and 3 tie on one box: slot 1 wins it
        _case("a-b", [(100, 100, 150, 150, 0.25, 0), (10, 10, 49, 49, 0.75, 0), (200, 200, 260, 260, 0.875, 1),
                      (10, 10, 50, 50, 0.75, 0), (100, 100, 149, 151, 0.25, 0), (199, 200, 260, 260, 0.875, 1)],
              [(10, 10, 50, 50, 0), (100, 100, 150, 150, 0), (200, 200, 260, 260, 1)]),
        # two detections on one box: the second is a false positive
        _case("a", [(20, 20, 80, 80, 0.9375, 2), (21, 20, 80, 80, 0.5, 2)], [(20, 20, 80, 80, 2)]),
        # the best box (row 0) is used, the second-best (row 1, IoU 0.85) is free: still a false positive
        _case("used_best", [(0, 0, 99, 99, 0.875, 0), (0, 0, 99, 101, 0.75, 0)], [(0, 0, 99, 99, 0), (0, 0, 99, 119, 0)]),
        # two identical ground-truth boxes: both detections pick the first (first on ties); the second finds it used
        _case("twins", [(30, 30, 70, 70, 0.625, 1), (30, 30, 70, 70, 0.5, 1)], [(30, 30, 70, 70, 1), (30, 30, 70, 70, 1)]),
        # IoU exactly 0.5: 100 / (100 + 200 - 100); a true positive at 0.5
        _case("exact_half", [(0, 0, 9, 9, 0.5, 0)], [(0, 0, 9, 19, 0)]),
        # touching: x2 = 9 against x1' = 10 is no overlap (iw = 0); against x1' = 9 one pixel column (IoU 10 / 190)
        _case("touching", [(0, 0, 9, 9, 0.5, 0), (0, 0, 9, 9, 0.5, 1)], [(10, 0, 19, 9, 0), (9, 0, 18, 9, 1)]),
        # a detection whose class (3) has no ground truth in ITS image (it has in "kiwi_here"), beside one that matches
        _case("no_class_gt", [(5, 5, 40, 40, 0.75, 3), (5, 5, 40, 40, 0.5, 0)], [(5, 5, 40, 40, 0)]),
        _case("kiwi_here", [(50, 50, 90, 90, 0.625, 3)], [(50, 50, 90, 90.25, 3)]),
        # class 4 is absent from the whole ground truth
        _case("absent_class", [(5, 5, 40, 40, 0.875, 4), (6, 5, 40, 40, 0.25, 1)], [(5, 5, 40, 40, 1)]),
        # normalised boxes k / 64 with scale (640, 480): pixel = 10 k and 7.5 k, exact float32 products
        _case("scaled", [(4 / 64, 8 / 64, 20 / 64, 40 / 64, 0.75, 2), (5 / 64, 8 / 64, 21 / 64, 40 / 64, 0.625, 2),
                         (32 / 64, 2 / 64, 60 / 64, 30 / 64, 0.5, 0)],
              [(40, 60, 200, 300, 2), (330, 15, 600, 225, 0), (50, 60, 210, 300, 2)], scale=(640.0, 480.0), normalised=True),
    ]
    assert len({c["stem"] for c in out}) == len(out)
    return out


def batch(case_list):
    """The cases stacked into the arrays y4_map_match takes: boxes [n,100,4], scores, classes [n,100], valid [n], scale [n,2],
    gt [n,256,5], gt_count [n]."""
    return (np.stack([c["boxes"] for c in case_list]), np.stack([c["scores"] for c in case_list]),
            np.stack([c["classes"] for c in case_list]), np.array([c["valid"] for c in case_list], dtype=np.int32),
            np.array([c["scale"] for c in case_list], dtype=np.float32), np.stack([c["gt"] for c in case_list]),
            np.array([c["gt_count"] for c in case_list], dtype=np.int32))


def oracle(case, thresholds):
    """`map_oracle.match_image` on one case -> (tp_mask [100], best_iou [100], match [100], gt_used [256]) padded the way
    y4_map_match pads: 0 / -1 / -1 in slots >= valid, 0 in rows >= gt_count."""
    import map_oracle
    k, m = case["valid"], case["gt_count"]
    px = map_oracle.pixel_boxes(case["boxes"][:k], case["scale"])
    tp, best, match, used = map_oracle.match_image(px, case["scores"][:k], case["classes"][:k], case["gt"][:m], thresholds)
    tp_mask = np.zeros(MAX_TOTAL, dtype=np.uint32); tp_mask[:k] = tp
    best_iou = np.full(MAX_TOTAL, -1.0, dtype=np.float64); best_iou[:k] = best
    match_full = np.full(MAX_TOTAL, -1, dtype=np.int32); match_full[:k] = match
    gt_used = np.zeros(MAX_GT, dtype=np.uint32); gt_used[:m] = used
    return tp_mask, best_iou, match_full, gt_used
