"""Inputs of the gathered decode + NMS tests (tiled inference), with their oracle results.  NumPy only; the GPU tests
(tests/test_gpu_tiled.py) hold the kernels to these, tests/test_tiling_cpu.py asserts the witnesses without a GPU.

The geometry: two photos of 200 x 260 and 96 x 120 pixels on a 96^2 network, tile 96^2, overlap 0.25, with the full image: window
starts y {0, 72, 104} x x {0, 72, 144, 164} and y {0} x x {0, 24}, 13 + 3 = 16 rows.  With max_batch = 4 the first photo's rows span
four forward chunks and the last chunk holds rows of both photos.

The heads are random (decode_nms_cases._random_heads): C = 3 with some 4 k / 0.85 k candidates per photo, C = 80 with some 12 k /
2.8 k -- the later-chunk paths of nms_kernel beyond NMS_THREADS and SORT_CAP.  MARGINS records the oracle's min_margin of every
(classes, seed, rule): the smallest distance of a tested pair's measure from the threshold; the tests assert the recorded figure
and that it is far above float32 rounding, so no decision hangs on the last bit of a mapped box."""
import functools

import numpy as np

import decode_nms_cases as DC
import tiled_oracle as TO

SIZE = 96
PHOTOS = ((200, 260), (96, 120))
TILE, OVERLAP = 96, 0.25
CHUNK = 4                                  # max_batch of the test engine: rows per forward chunk
IOU_THR, SCORE_THR = 0.413, 0.3            # config.py's thresholds (make_config)
BIAS = {3: (-1.0, 0.0), 80: (-2.0, -1.5)}  # C -> (objectness bias, class bias)
SEEDS = (0, 1, 2)
RULES = {"iou": ("iou", 1.0, False), "diou06": ("diou", 0.6, False), "agn_iou": ("iou", 1.0, True)}
# (classes, seed, rule) -> the oracle's min_margin over both photos, computed on the CPU
MARGINS = {
    (3, 0, "iou"): 3.56e-3, (3, 0, "diou06"): 4.91e-4, (3, 0, "agn_iou"): 9.09e-4,
    (3, 1, "iou"): 5.08e-3, (3, 1, "diou06"): 2.00e-2, (3, 1, "agn_iou"): 1.23e-3,
    (3, 2, "iou"): 2.70e-3, (3, 2, "diou06"): 2.47e-2, (3, 2, "agn_iou"): 7.67e-4,
    (80, 0, "iou"): 6.95e-2, (80, 0, "diou06"): 2.46e-1, (80, 0, "agn_iou"): 1.72e-3,
    (80, 1, "iou"): 3.48e-2, (80, 1, "diou06"): 6.42e-2, (80, 1, "agn_iou"): 6.21e-4,
    (80, 2, "iou"): 7.69e-2, (80, 2, "diou06"): 1.57e-1, (80, 2, "agn_iou"): 1.67e-3,
}
MIN_MARGIN = 2.1e-4                        # every case is at least this far from a coin toss (and >= 1e-5, the boxes' bar)


@functools.lru_cache(maxsize=None)
def geometry():
    """-> (rows, row_group [R], row_slot [R], row_map [R, 4] float32, slots per group): `rows` the (window, rect, map) of
    yolo4hip.tiling.tile_rows for every photo, in batch order."""
    from yolo4hip import tiling
    rows, group, slot = [], [], []
    for p, (h, w) in enumerate(PHOTOS):
        r = tiling.tile_rows(h, w, (SIZE, SIZE), (TILE, TILE), OVERLAP, full_image=True, letterbox=False)
        rows += r
        group += [p] * len(r)
        slot += list(range(len(r)))
    maps = np.stack([m for _, _, m in rows]).astype(np.float32)
    per_group = [group.count(p) for p in range(len(PHOTOS))]
    return rows, np.asarray(group, np.int32), np.asarray(slot, np.int32), maps, per_group


@functools.lru_cache(maxsize=None)
def heads(ncls, seed):
    """The raw heads of the 16 rows (arrays shared by every test: do not write to them)."""
    ob, cb = BIAS[ncls]
    return DC._random_heads(np.random.default_rng(seed), len(geometry()[1]), SIZE, ncls, ob, cb)


def groups_of(hd, group, maps):
    """Split batch-ordered heads and maps into the oracle's per-group (heads, maps) lists."""
    out = []
    for g in range(int(group.max()) + 1):
        sel = np.nonzero(group == g)[0]
        out.append(([h[sel] for h in hd], maps[sel]))
    return out


@functools.lru_cache(maxsize=None)
def reference(ncls, seed, rule):
    """-> the tiled oracle's (boxes, scores, classes, valid, kept_idx, min_margin, candidate counts) of a case."""
    from yolo4hip.config import make_config
    _, group, _, maps, _ = geometry()
    kind, beta, agn = RULES[rule]
    return TO.gathered_nms(groups_of(heads(ncls, seed), group, maps), ncls, make_config(SIZE), SIZE, IOU_THR, SCORE_THR, kind, beta, agn)


def kept_slots(ref, g, nbox):
    """The slots the kept boxes of group g come from."""
    return set(int(i) // nbox for i in ref[4][g][:int(ref[3][g])])
