"""Crafted images for the COCO matching (`y4_coco_match`, `cocoeval.CocoAccumulator`), as one small dataset in the style of
tests/map_cases.py (whose `_case` and `batch` are used as they are): every pixel coordinate a multiple of 0.25, every score a
multiple of 1/1024, max_total = 100 slots and max_gt = 256 rows, NaN beyond valid / gt_count.

A witness case carries `expect`: for some (range name, threshold index of THRESHOLD_SETS[10]) the decision per detection SLOT,
written out by hand as (matched row or -1, ignored).  tests/test_coco_cpu.py holds the oracle to them; the device is held to
the oracle on everything."""
import numpy as np

from map_cases import MAX_GT, MAX_TOTAL, _case, batch  # noqa: F401

CLASS_NAMES = ["pear", "apple", "fig", "kiwi", "date"]
COCO_AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
AREA_INDEX = {"all": 0, "small": 1, "medium": 2, "large": 3}
# (thresholds, area ranges) by (T, A)
PARAM_SETS = {(1, 1): ((0.5,), COCO_AREAS[:1]),
              (10, 4): (tuple(float(t) for t in np.linspace(.5, .95, 10)), COCO_AREAS),
              (16, 4): (tuple(float(t) for t in np.linspace(0.2, 0.95, 16)), COCO_AREAS)}


def _full():
    """valid = max_total = 100 on 256 rows of 3 classes in a 700 x 700 field, sides 8 .. 200: rows in every size bucket, crowded,
    several detections per row, score ties, detections of the wrong class; about 33 detections per class, so cls_rank passes
    maxDets 1 and 10."""
    rng = np.random.default_rng(20261)
    gts = []
    for _ in range(MAX_GT):
        x1, y1 = 8 + rng.integers(0, 2000, 2) / 4
        w, h = rng.integers(32, 800, 2) / 4
        gts.append((x1, y1, x1 + w, y1 + h, int(rng.integers(0, 3))))
    dets = []
    for _ in range(MAX_TOTAL):
        x1, y1, x2, y2, c = gts[int(rng.integers(0, MAX_GT))]
        j = rng.integers(-12, 13, 4) / 4
        cls = c if rng.random() < 0.8 else int(rng.integers(0, 3))
        dets.append((x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3], int(rng.integers(1, 64)) / 64, cls))
    return _case("full", dets, gts)


def _with(case, **extra):
    case.update(extra)
    return case


def _nan_score():
    """Slot 1 of three valid slots has a NaN score: it is never walked, takes no rank and no row; slot 2 gets the row."""
    c = _case("nan_score", [(200, 200, 260, 260, 0.25, 0), (10, 10, 50, 50, 0.5, 0), (10, 10, 50, 50, 0.125, 0)],
              [(10, 10, 50, 50, 0), (200, 200, 260, 260, 0)])
    c["scores"][1] = np.nan
    c["expect"] = {("all", 0): [(1, False), (-1, False), (0, False)]}
    c["expect_rank"] = [0, -1, 1]
    return c


def cases():
    every = range(10)
    out = [
        _case("no_det", [], [(10, 10, 50, 50, 0), (60, 60, 90, 90, 1)]),
        _case("no_gt", [(10, 10, 50, 50, 0.75, 0), (12, 10, 50, 50, 0.5, 1), (0, 0, 5, 5, 0.25, 2)], []),
        _case("nothing", [], []),                                                     # an image with nothing
        _full(),
        # IoU exactly 0.5 without `+ 1`: 100 / (100 + 200 - 100) (the devkit's widths give 121 / 231).  Matched at 0.5, not at
        # 0.55.  The row (area 200) is ignored under medium: the detection matched to it is ignored; unmatched at 0.55 it is
        # ignored as well, its own area 100 being out of range
        _with(_case("exact_half", [(0, 0, 10, 10, 0.5, 0)], [(0, 0, 10, 20, 0)]),
              expect={("all", 0): [(0, False)], ("all", 1): [(-1, False)], ("small", 0): [(0, False)],
                      ("medium", 0): [(0, True)], ("medium", 1): [(-1, True)]}),
        # touching boxes: x2 = 10 against x1' = 10 gives iw = 0, IoU 0 (with `+ 1` a pixel column would overlap): unmatched at
        # every threshold; a false positive under all and small, ignored under medium (area 100 out of range)
        _with(_case("touching", [(0, 0, 10, 10, 0.5, 0)], [(10, 0, 20, 10, 0)]),
              expect={**{("all", t): [(-1, False)] for t in every}, ("small", 0): [(-1, False)], ("medium", 0): [(-1, True)]}),
        # twin rows: the first detection takes the LAST twin (`iou >= best`), the second takes the other one -- VOC gives both
        # the first twin and makes the second detection a false positive
        _with(_case("twins", [(30, 30, 70, 70, 0.625, 1), (30, 30, 70, 70, 0.5, 1)], [(30, 30, 70, 70, 1), (30, 30, 70, 70, 1)]),
              expect={("all", t): [(1, False), (0, False)] for t in every}),
        # one detection (area 10000), row 0 (area 9200, IoU 0.92) and row 1 (area 16000, IoU 0.625).  Under large row 0 is
        # ignored and row 1 is not: the detection takes row 1 up to 0.6, then row 0 and is itself ignored up to 0.9, and is an
        # in-range false positive at 0.95.  Under all it takes row 0, the larger IoU; under medium row 0 is the regular one and
        # at 0.95 the unmatched detection is out of range; under small both rows are ignored and it takes the better one
        _with(_case("ignored_or_not", [(0, 0, 100, 100, 0.5, 0)], [(0, 0, 92, 100, 0), (0, 0, 100, 160, 0)]),
              expect={**{("large", t): [(1, False)] for t in (0, 1, 2)}, **{("large", t): [(0, True)] for t in range(3, 9)},
                      ("large", 9): [(-1, False)],
                      **{("all", t): [(0, False)] for t in range(9)}, ("all", 9): [(-1, False)],
                      **{("medium", t): [(0, False)] for t in range(9)}, ("medium", 9): [(-1, True)],
                      **{("small", t): [(0, True)] for t in range(9)}, ("small", 9): [(-1, True)]}),
        # two unmatched detections, areas 400 and 10000: under small the first is a false positive and the second ignored,
        # under large the other way round, under medium both ignored, under all both false positives
        _with(_case("unmatched_range", [(0, 0, 20, 20, 0.75, 2), (300, 300, 400, 400, 0.5, 2)], [(600, 600, 650, 650, 2)]),
              expect={("all", 0): [(-1, False), (-1, False)], ("small", 0): [(-1, False), (-1, True)],
                      ("medium", 0): [(-1, True), (-1, True)], ("large", 0): [(-1, True), (-1, False)]}),
        # a row of area exactly 1024 counts under small AND medium (both tests strict), not under large
        _with(_case("area_1024", [(0, 0, 32, 32, 0.5, 1)], [(0, 0, 32, 32, 1)]),
              expect={("small", 9): [(0, False)], ("medium", 9): [(0, False)], ("large", 9): [(0, True)], ("all", 9): [(0, False)]},
              expect_gt_ignore=[0b1000]),
        # score ties across slots: slots 1 and 2 tie at 0.75 on row 0; slot 1 walks first and takes it (IoU 1521 / 1600 = 0.950625,
        # past every threshold), slot 2 (IoU 1) finds it matched; slot 0 walks last
        _with(_case("ties", [(100, 100, 150, 150, 0.25, 0), (10, 10, 49, 49, 0.75, 0), (10, 10, 50, 50, 0.75, 0)],
                    [(10, 10, 50, 50, 0), (100, 100, 150, 150, 0)]),
              expect={("all", t): [(1, False), (0, False), (-1, False)] for t in every}, expect_rank=[2, 0, 1]),
        # a class (3) with a detection and no rows in its image, beside one that matches; class 3 has rows in "kiwi_here" only
        _with(_case("no_class_gt", [(5, 5, 40, 40, 0.75, 3), (5, 5, 40, 40, 0.5, 0)], [(5, 5, 40, 40, 0)]),
              expect={("all", 0): [(-1, False), (0, False)]}, expect_rank=[0, 0]),
        _case("kiwi_here", [(50, 50, 90, 90, 0.625, 3)], [(50, 50, 90, 90.25, 3)]),
        # the scaled case: normalised boxes k / 64 with scale (640, 480), pixel = 10 k and 7.5 k, exact float32 products.  Slot 0
        # takes row 0 (IoU 1), slot 1 row 2 (IoU 1), slot 2 row 1 (280 x 210 in 270 x 210: IoU 56700 / 58800 = 0.964)
        _with(_case("scaled", [(4 / 64, 8 / 64, 20 / 64, 40 / 64, 0.75, 2), (5 / 64, 8 / 64, 21 / 64, 40 / 64, 0.625, 2),
                               (32 / 64, 2 / 64, 60 / 64, 30 / 64, 0.5, 0)],
                    [(40, 60, 200, 300, 2), (330, 15, 600, 225, 0), (50, 60, 210, 300, 2)], scale=(640.0, 480.0), normalised=True),
              expect={("all", 9): [(0, False), (2, False), (1, False)]}),
        _nan_score(),
    ]
    assert len({c["stem"] for c in out}) == len(out)
    return out


def oracle(case, thresholds, area_ranges):
    """`coco_oracle.match_image` on one case, padded the way y4_coco_match pads -> (dt_match uint32 [A,100], dt_ignore uint32
    [A,100], cls_rank int32 [100], gt_ignore uint32 [256], match_row int32 [A,T,100])."""
    import coco_oracle
    k, m = case["valid"], case["gt_count"]
    A, T = len(area_ranges), len(thresholds)
    px = coco_oracle.pixel_boxes(case["boxes"][:k], case["scale"])
    dm, di, rank, gi, row = coco_oracle.match_image(px, case["scores"][:k], case["classes"][:k], case["gt"][:m], area_ranges, thresholds)
    dt_match, dt_ignore = np.zeros((A, MAX_TOTAL), dtype=np.uint32), np.zeros((A, MAX_TOTAL), dtype=np.uint32)
    dt_match[:, :k], dt_ignore[:, :k] = dm, di
    cls_rank = np.full(MAX_TOTAL, -1, dtype=np.int32); cls_rank[:k] = rank
    gt_ignore = np.zeros(MAX_GT, dtype=np.uint32); gt_ignore[:m] = gi
    match_row = np.full((A, T, MAX_TOTAL), -1, dtype=np.int32); match_row[:, :, :k] = row
    return dt_match, dt_ignore, cls_rank, gt_ignore, match_row


def dataset_images(case_list):
    """The cases as `coco_oracle.evaluate` takes a dataset: per image (pixel boxes, scores, classes, rows)."""
    import coco_oracle
    return [(coco_oracle.pixel_boxes(c["boxes"][:c["valid"]], c["scale"]), c["scores"][:c["valid"]], c["classes"][:c["valid"]],
             c["gt"][:c["gt_count"]]) for c in case_list]
