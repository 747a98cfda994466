"""Inputs of the oriented gather tests (test-time augmentation), with their oracle results.  NumPy only; tests/test_gpu_views.py
holds y4_decode_gather_views to these, tests/test_views_cpu.py asserts the recorded figures without a GPU.

The geometry: a 96^2 network, max_batch 4.  Group 0 is a 131 x 97 photo, stretched, under the views of VIEW_SETS[geometry] (4, 5 or
6 slots); group 1 a 96 x 120 photo, letterboxed, under ((1.0, 'lr'), (0.75, '')) (2 slots): 6 to 8 rows in two forward chunks, the
second chunk with rows of both photos.  Every geometry has an 'lr', a 'ud', an 'lrud' and a scaled map.  The maps are those of
yolo4hip.tiling.view_rows on each photo's full-image row.

The heads are random (decode_nms_cases._random_heads, tiled_cases.BIAS).  CASES maps (classes, geometry, rule) to the head seed
and the oracle's figures on the CPU: the min_margin of the NMS decisions, the min_margin of the merge's membership decisions, the
kept boxes that come from a flipped slot, and the suppressions that only another view's box explains
(views_oracle.cross_view_suppressions).  Seeds were picked (`python tests/views_cases.py`) so that both margins are at least 1e-4
-- the parity rule asks for 1e-5 -- and the two counts are positive; no case is skipped at run time."""
import functools

import numpy as np

import decode_nms_cases as DC
import tiled_cases as TC
import views_oracle as VO

SIZE, CHUNK = TC.SIZE, TC.CHUNK
IOU_THR, SCORE_THR = TC.IOU_THR, TC.SCORE_THR
RULES = TC.RULES
PHOTOS = ((131, 97, False), (96, 120, True))                    # (h, w, letterbox)
VIEW_SETS = {
    0: ((1.0, ""), (0.83, "lr"), (1.0, "ud"), (0.67, "lrud")),
    1: ((1.0, "lrud"), (0.83, "lr"), (0.67, ""), (0.9, "ud"), (1.0, "")),
    2: ((1.0, ""), (0.83, "lr"), (0.67, ""), (1.0, "ud"), (0.5, "lrud"), (1.0, "lr")),
}
SECOND = ((1.0, "lr"), (0.75, ""))
NBOX = 3 * sum((SIZE // s) ** 2 for s in (8, 16, 32))

# (classes, geometry, rule) -> (head seed, NMS min_margin, membership min_margin, kept boxes from flipped slots, cross-view
# suppressions), the oracle's on the CPU
CASES = {
    (3, 0, "iou"): (0, 4.09e-04, 4.09e-04, 127, 9),
    (3, 0, "diou06"): (0, 2.20e-03, 1.52e-04, 130, 5),
    (3, 0, "agn_iou"): (0, 4.09e-04, 1.34e-04, 127, 44),
    (3, 1, "iou"): (0, 2.86e-03, 1.82e-04, 121, 17),
    (3, 1, "diou06"): (0, 1.78e-03, 9.98e-04, 120, 8),
    (3, 1, "agn_iou"): (0, 5.46e-04, 1.06e-04, 118, 72),
    (3, 2, "iou"): (1, 1.96e-03, 1.01e-04, 125, 20),
    (3, 2, "diou06"): (0, 8.16e-03, 6.50e-04, 112, 7),
    (3, 2, "agn_iou"): (1, 1.01e-04, 1.01e-04, 126, 56),
    (80, 0, "iou"): (1, 4.31e-03, 1.77e-03, 164, 1),
    (80, 0, "diou06"): (3, 1.51e-01, 5.71e-03, 102, 1),
    (80, 0, "agn_iou"): (2, 1.05e-04, 1.05e-04, 120, 137),
    (80, 1, "iou"): (1, 1.69e-02, 1.32e-03, 93, 1),
    (80, 1, "diou06"): (3, 7.62e-02, 9.06e-03, 132, 1),
    (80, 1, "agn_iou"): (2, 1.92e-04, 1.92e-04, 123, 127),
    (80, 2, "iou"): (1, 1.50e-02, 4.85e-04, 122, 1),
    (80, 2, "diou06"): (6, 1.28e-02, 1.28e-02, 98, 1),
    (80, 2, "agn_iou"): (1, 2.24e-04, 1.82e-04, 126, 140),
}
MIN_MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def geometry(geo):
    """-> (rows: (window, rect, flip bits, map) in batch order, row_group [R], row_slot [R], row_map [R, 4], slots per group)."""
    from yolo4hip import tiling
    rows, group, slot = [], [], []
    for p, ((h, w, lb), views) in enumerate(zip(PHOTOS, (VIEW_SETS[geo], SECOND))):
        base = tiling.tile_rows(h, w, (SIZE, SIZE), None, 0.0, True, lb)[-1:]
        r = tiling.view_rows(base, views, (h, w), (SIZE, SIZE))
        rows += r
        group += [p] * len(r)
        slot += list(range(len(r)))
    maps = np.stack([r[3] for r in rows]).astype(np.float32)
    return rows, np.asarray(group, np.int32), np.asarray(slot, np.int32), maps, [group.count(p) for p in range(len(PHOTOS))]


@functools.lru_cache(maxsize=None)
def heads(ncls, geo, seed):
    """The raw heads of the case's rows (shared: do not write to them)."""
    ob, cb = TC.BIAS[ncls]
    return DC._random_heads(np.random.default_rng([seed, geo, ncls]), len(geometry(geo)[1]), SIZE, ncls, ob, cb)


@functools.lru_cache(maxsize=None)
def tables(ncls, geo, seed):
    """The oracle's group tables: per group (boxes [1, T * nbox, 4] under the oriented maps, scores [1, T * nbox, C])."""
    from yolo4hip.config import make_config
    _, group, _, maps, _ = geometry(geo)
    return [VO.group_tables(h, m, ncls, make_config(SIZE), SIZE) for h, m in TC.groups_of(heads(ncls, geo, seed), group, maps)]


@functools.lru_cache(maxsize=None)
def reference(ncls, geo, rule, seed=None):
    """-> the oracle's (boxes, scores, classes, valid, kept_idx, min_margin, candidate counts) of a case, merge off."""
    from yolo4hip.config import make_config
    seed = CASES[(ncls, geo, rule)][0] if seed is None else seed
    _, group, _, maps, _ = geometry(geo)
    return VO.gathered_nms(TC.groups_of(heads(ncls, geo, seed), group, maps), ncls, make_config(SIZE), SIZE, IOU_THR, SCORE_THR,
                           *RULES[rule])


def figures(ncls, geo, rule, seed):
    """-> (NMS min_margin, membership min_margin, kept boxes from flipped slots, cross-view suppressions) on the CPU."""
    ref = reference(ncls, geo, rule, seed)
    _, group, slot, maps, _ = geometry(geo)
    member, flipped, cross = np.inf, 0, 0
    for g, (b, s) in enumerate(tables(ncls, geo, seed)):
        member = min(member, VO.merged(b, s, IOU_THR, SCORE_THR, *RULES[rule])[6])
        gmaps = maps[group == g]
        v = int(ref[3][g])
        flipped += sum(1 for i in ref[4][g][:v] if (gmaps[int(i) // NBOX][[0, 2]] < 0).any())
        cross += VO.cross_view_suppressions(b[0], s[0], [a[g:g + 1] for a in ref[:5]], NBOX, IOU_THR, SCORE_THR, *RULES[rule])
    return float(ref[5]), float(member), flipped, cross


if __name__ == "__main__":                                       # the seed picker: prints a CASES table
    for ncls in (3, 80):
        for geo in sorted(VIEW_SETS):
            for rule in RULES:
                for seed in range(50):
                    f = figures(ncls, geo, rule, seed)
                    if f[0] >= MIN_MARGIN and f[1] >= MIN_MARGIN and f[2] >= 1 and f[3] >= 1:
                        print(f"    ({ncls}, {geo}, {rule!r}): ({seed}, {f[0]:.2e}, {f[1]:.2e}, {f[2]}, {f[3]}),", flush=True)
                        break
                else:
                    raise SystemExit(f"no seed for {(ncls, geo, rule)}")
