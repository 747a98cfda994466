"""Inputs of the loss-gradient tests, from seeds (shared by tests/golden/make_lossgrad_fixtures.py and the tests, so that the
fixture files hold results only).  The cases of loss_cases.py cannot serve: image 2 there carries a degenerate row (w = 0)
between valid rows, whose label has zero width -- max(0, 0) inside GIoU is an exact tie, where autodiff's choice is unspecified --
and seed 2 of 160_coco leaves one responsible lane 3.7e-4 px from a tie.  Same generators, the degenerate row given a width, and
the first seeds that pass every assertion of the fixture generator (ties further than 1e-3 px, 1e-4 clearance of the ignore
threshold)."""
import hashlib

import numpy as np

import loss_cases as LC

# name -> input (H, W), classes, images, seed
CASES = {
    "416_bccd_g": dict(hw=(416, 416), ncls=3, n=4, seed=2),
    "160_coco_g": dict(hw=(160, 160), ncls=80, n=4, seed=6),
    "160_wide_g": dict(hw=(160, 160), ncls=3, n=4, seed=1, wide=True),         # loss_cases._make_heads_wide
}


def make_boxes(hw, ncls, n, seed):
    boxes = LC.make_boxes(hw, ncls, n, seed)
    if n > 2:
        boxes[2, 3, 2] = min(boxes[2, 3, 0] + 24.0, hw[1] - 1.0)       # the degenerate row of loss_cases: 24 px wide here
    return boxes


def make_case(name):
    """-> dict(hw, ncls, n, boxes [n, 100, 5], heads [3 arrays], sha: a checksum of the inputs), as loss_cases.make_case."""
    LC.make_case("160_coco")                                             # (puts the package on sys.path)
    from yolo4hip.data import records_from_boxes
    c = CASES[name]
    boxes = make_boxes(c["hw"], c["ncls"], c["n"], c["seed"])
    records, _ = records_from_boxes(boxes, c["hw"], LC.ANCHORS, c["ncls"])
    heads = LC.make_heads(c["hw"], c["ncls"], c["n"], c["seed"], records, c.get("wide", False))
    sha = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in [boxes] + heads)).hexdigest()
    return dict(hw=c["hw"], ncls=c["ncls"], n=c["n"], boxes=boxes, heads=heads, sha=sha)
