"""Inputs for the Soft-NMS tests (y4_set_nms_soft): hand-made witnesses, each of which fails for one specific wrong kernel, the list
lengths at which the kernel changes its path, and seeded random heads.  NumPy only: tests/test_soft_nms_cpu.py asserts every
witness and every margin on the oracle (tests/soft_nms_oracle.py) without a GPU, tests/test_gpu_soft_nms.py holds the kernel to the
oracle on the same inputs.

Geometry of the witnesses: anchor 0 of stride-8 cells with t_xy = 0, so a box is centred on its cell ((col + 0.5) * 8, (row + 0.5) * 8)
and t_wh sets its size in pixels; objectness logit 8, the class logit sets the score.  Two boxes w x h on horizontally adjacent
cells have IoU (w - 8) / (w + 8):  32 x 20 -> 0.6,  20 x 20 -> 3/7,  12 x 20 -> 0.2."""
import functools

import numpy as np

import decode_nms_cases as DC

IOU_THR, SCORE_THR = 0.413, 0.3            # config.py's thresholds (make_config)
ANCHOR0 = (12.0, 16.0)                     # anchor 0 of scale 0 (config.py)
SIGMA = 0.5
TOP_K_MAX = 4096                           # soft_nms.hip: SORT_CAP


def t_of(w, h):
    return (0.0, 0.0, float(np.log(w / ANCHOR0[0])), float(np.log(h / ANCHOR0[1])))


def logit_for(score, lo=8.0):
    """The class logit that gives sigmoid(lo) * sigmoid(logit) = score."""
    p = score * (1.0 + np.exp(-lo))
    return float(np.log(p / (1.0 - p)))


def entry(gy, gx, cls, score, w=20.0, h=20.0, anchor=0, image=0):
    return (image, 0, gy, gx, anchor, cls, 8.0, logit_for(score), t_of(w, h))


def box_index(size, gy, gx, anchor=0):
    return 3 * (gy * (size // 8) + gx) + anchor


def iou_adjacent(w):
    return (w - 8.0) / (w + 8.0)


# name -> (size, ncls, entries, engine caps, soft keywords).  What each one shows is asserted in tests/test_soft_nms_cpu.py
# (`test_witness_*`) on the oracle, and again on the device's outputs.
SIZE = 96
WITNESSES = {
    # A (0.9), B (0.8, IoU 0.6 with A), C (0.5, disjoint): B' = 0.8 * exp(-0.72) = 0.389 -> A, C, B'.  A walk in original order gives A, B', C
    "order": (SIZE, 3, [entry(5, 4, 1, 0.9, 32), entry(5, 5, 1, 0.8, 32), entry(1, 9, 1, 0.5)], {}, {}),
    # D between A and E (20 x 20 on three adjacent cells): D carries f(3/7) of A and f(3/7) of E; E carries f(1/9) of A first
    "two_factors": (SIZE, 3, [entry(5, 4, 1, 0.9), entry(5, 5, 1, 0.7), entry(5, 6, 1, 0.85)], {}, {}),
    # the pair of `order` in two classes: no decay; `agnostic` decays
    "classes": (SIZE, 3, [entry(5, 4, 1, 0.9, 32), entry(5, 5, 2, 0.8, 32), entry(1, 9, 1, 0.5)], {}, {}),
    # min_score 0.45: B' = 0.389 is gone, valid = 2
    "floor": (SIZE, 3, [entry(5, 4, 1, 0.9, 32), entry(5, 5, 1, 0.8, 32), entry(1, 9, 1, 0.5)], {}, {"min_score": 0.45}),
    # max_per_class = 1 under an agnostic rule: A (class 0) kept, A2 (class 0, disjoint from A) turned away, X (class 1, IoU 0.6 with
    # A2) keeps its score: a turned-away candidate decays nothing
    "turned_away": (SIZE, 3, [entry(1, 1, 0, 0.9), entry(8, 4, 0, 0.8, 32), entry(8, 5, 1, 0.7, 32)], {"max_per_class": 1}, {}),
    # three disjoint boxes, max_total = 2
    "max_total": (SIZE, 3, [entry(1, 1, 0, 0.9), entry(5, 5, 1, 0.8), entry(9, 9, 2, 0.7)], {"max_total": 2}, {}),
    # exact score ties on disjoint boxes, two classes per box: out by box index, then class
    "ties": (SIZE, 3, [entry(gy, gx, c, 0.6, 6.0, 6.0) for gy, gx in ((7, 2), (1, 9), (4, 4), (1, 3)) for c in (2, 0)], {}, {}),
    "empty": (SIZE, 3, [], {}, {}),
}


@functools.lru_cache(maxsize=None)
def witness(name):
    """-> (size, ncls, heads, boxes, scores, caps, soft): one image."""
    from yolo4hip.config import make_config
    size, ncls, entries, caps, soft = WITNESSES[name]
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    return size, ncls, heads, b, s, dict(caps), dict(soft)


# ---- list lengths: exactly L candidates at 160^2, C = 80.  A CROWD of up to six 32 x 20 boxes of class 0 on adjacent cells of row 10
# (IoU 0.6 between neighbours; scores 0.99 .. 0.965), whose decayed scores are what the kernel has to get right, among a BULK of
# 6 x 6 boxes on anchor 0 of the cells of the other rows (rows 9 .. 11 stay free), any class: disjoint across cells, and the same
# box in several classes does not interact under a class-aware rule.  The bulk's 80 best scores are spread over 0.75 .. 0.955 and the
# rest lies in 0.31 .. 0.38, under every decayed crowd score: the 100 results are the bulk's best, the crowd -- some of its
# boxes decayed once or twice, others pushed under the floor -- and then the best of the rest.  Where a candidate sits in the list the decode stage decides anew
# in every run.  The seeds are chosen like those of RANDOM_SEEDS, for the class-aware 'iou' modes.
SIZE_LEN = 160
NCLS_LEN = 80
LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
LENGTH_MODES = ("gauss_iou", "lin_iou")
LENGTH_SEEDS = {L: 0 for L in LENGTHS}      # (every length clears the bar with the first seed tried)


@functools.lru_cache(maxsize=None)
def length_case(L, seed=None):
    """-> (heads, boxes, scores): one image with exactly L candidates."""
    from yolo4hip.config import make_config
    size, ncls = SIZE_LEN, NCLS_LEN
    seed = LENGTH_SEEDS.get(L, 0) if seed is None else seed
    rng = np.random.default_rng([seed, L])
    n_crowd = min(6, L)
    entries = [entry(10, 2 + j, 0, 0.99 - 0.005 * j, 32.0) for j in range(n_crowd)]
    slots = [(gy, gx, c) for gy in range(20) if not 9 <= gy <= 11 for gx in range(20) for c in range(ncls)]
    n_bulk = L - n_crowd
    pick = rng.permutation(len(slots))[:n_bulk]
    n_top = min(80, n_bulk)
    scores = np.concatenate([np.sort(rng.uniform(0.75, 0.955, n_top))[::-1], rng.uniform(0.31, 0.38, n_bulk - n_top)])
    for j, sc in zip(pick, scores):
        gy, gx, c = slots[j]
        entries.append(entry(gy, gx, c, float(sc), 6.0, 6.0))
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    assert int((s > np.float32(SCORE_THR)).sum()) == L
    return heads, b, s


# ---- exactly top_k participants: a STACK of L - 1 keys -- boxes that cover the whole image (t_wh = 6; any two overlap with
# IoU > 0.9), anchor 1 of the stride-8 cells, several classes per box -- and one small box of its own, the LONER, with the
# lowest score of all.  Under the agnostic 'hard' method the best stack key suppresses the rest of the stack: with L <= top_k the
# loner is kept second, with L = top_k + 1 it is no participant and valid is 1.
EDGE_LENGTHS = (4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def edge_case(L):
    """-> (heads, boxes, scores, box index of the loner): one image with exactly L candidates at 160^2, C = 80."""
    from yolo4hip.config import make_config
    size, ncls = SIZE_LEN, NCLS_LEN
    rng = np.random.default_rng([7, L])
    slots = [(gy, gx, a, c) for gy in range(20) for gx in range(20) for a in (1,) for c in range(ncls)]
    pick = rng.permutation(len(slots))[:L - 1]
    entries = [(0, 0, slots[j][0], slots[j][1], slots[j][2], slots[j][3], 8.0, float(rng.uniform(0.0, 3.0)), (0.0, 0.0, 6.0, 6.0)) for j in pick]
    entries.append(entry(3, 3, 5, 0.31, 6.0, 6.0))
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    assert int((s > np.float32(SCORE_THR)).sum()) == L
    return heads, b, s, box_index(size, 3, 3)


# ---- top_k = 64 on a 200-key list: 64 boxes of class 0 in the left half, crowded (scores 0.60 .. 0.95); the 65th key is one
# box of class 1 alone in the right half (0.55); 135 more of class 0 in the left half below it (0.32 .. 0.50)
TOPK_SMALL = 64
TOPK_LONER = (2, 17)                       # its cell (row, column) at 160^2


@functools.lru_cache(maxsize=None)
def topk_case():
    from yolo4hip.config import make_config
    size, ncls = SIZE_LEN, 3
    rng = np.random.default_rng(68)                 # (chosen like the seeds of RANDOM_SEEDS)
    cells = [(gy, gx, a) for gy in range(20) for gx in range(10) for a in range(3)]
    order = rng.permutation(len(cells))[:199]
    scores = np.concatenate([np.linspace(0.95, 0.60, 64), np.linspace(0.50, 0.32, 135)])
    entries = []
    for j, sc in zip(order, scores):
        gy, gx, a = cells[j]
        entries.append((0, 0, gy, gx, a, 0, 8.0, logit_for(float(sc)), (0.0, 0.0, float(rng.normal(0.4, 0.2)), float(rng.normal(0.4, 0.2)))))
    entries.append(entry(TOPK_LONER[0], TOPK_LONER[1], 1, 0.55, 8.0, 8.0))
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    assert int((s > np.float32(SCORE_THR)).sum()) == 200
    return heads, b, s, box_index(size, *TOPK_LONER)


# ---- seeded random heads, one image each.  MODES: the (method, kind, beta, agnostic) every input runs under.  A seed is in the
# table because the float64 face reports a margin of at least MARGIN_BAR for it under that mode (tests/test_soft_nms_cpu.py asserts
# it); one that misses is replaced HERE, never skipped at run time.
MARGIN_BAR = 1e-4
MODES = {
    "gauss_iou": ("gaussian", "iou", 1.0, False), "gauss_iou_agn": ("gaussian", "iou", 1.0, True),
    "gauss_diou": ("gaussian", "diou", 0.6, False), "gauss_diou_agn": ("gaussian", "diou", 0.6, True),
    "lin_iou": ("linear", "iou", 1.0, False), "lin_iou_agn": ("linear", "iou", 1.0, True),
    "lin_diou": ("linear", "diou", 0.6, False), "lin_diou_agn": ("linear", "diou", 0.6, True),
}
# (size, classes) -> (objectness bias, class bias) of DC._random_heads: some tens to a few hundred candidates per image, crowded
# enough that most boxes are decayed several times
RANDOM_BIAS = {(96, 3): (-1.0, -1.0), (160, 3): (-2.0, -1.5), (96, 80): (-1.5, -3.5), (160, 80): (-2.5, -3.5)}
# (size, classes, mode) -> seed
RANDOM_SEEDS = {
    (96, 3, "gauss_iou"): 141,    # 145 candidates, valid 89, margin 2.81e-04
    (96, 3, "gauss_iou_agn"): 18,    # 171 candidates, valid 48, margin 2.09e-04
    (96, 3, "gauss_diou"): 2,    # 181 candidates, valid 100, margin 2.34e-04
    (96, 3, "gauss_diou_agn"): 1,    # 161 candidates, valid 82, margin 2.68e-04
    (96, 3, "lin_iou"): 22,    # 153 candidates, valid 100, margin 5.28e-04
    (96, 3, "lin_iou_agn"): 5,    # 171 candidates, valid 87, margin 2.01e-04
    (96, 3, "lin_diou"): 5,    # 171 candidates, valid 100, margin 1.07e-03
    (96, 3, "lin_diou_agn"): 2,    # 181 candidates, valid 100, margin 2.71e-04
    (160, 3, "gauss_iou"): 14,    # 104 candidates, valid 84, margin 2.50e-04
    (160, 3, "gauss_iou_agn"): 51,    # 108 candidates, valid 57, margin 2.16e-04
    (160, 3, "gauss_diou"): 1,    # 112 candidates, valid 100, margin 3.51e-04
    (160, 3, "gauss_diou_agn"): 11,    # 113 candidates, valid 85, margin 2.26e-04
    (160, 3, "lin_iou"): 1,    # 112 candidates, valid 98, margin 3.74e-04
    (160, 3, "lin_iou_agn"): 1,    # 112 candidates, valid 85, margin 3.74e-04
    (160, 3, "lin_diou"): 2,    # 125 candidates, valid 100, margin 5.82e-04
    (160, 3, "lin_diou_agn"): 2,    # 125 candidates, valid 100, margin 3.03e-04
    (96, 80, "gauss_iou"): 2,    # 132 candidates, valid 100, margin 2.87e-04
    (96, 80, "gauss_iou_agn"): 27,    # 141 candidates, valid 37, margin 2.10e-04
    (96, 80, "gauss_diou"): 1,    # 119 candidates, valid 100, margin 7.89e-04
    (96, 80, "gauss_diou_agn"): 1,    # 119 candidates, valid 61, margin 3.42e-04
    (96, 80, "lin_iou"): 4,    # 117 candidates, valid 100, margin 8.22e-04
    (96, 80, "lin_iou_agn"): 5,    # 145 candidates, valid 74, margin 5.48e-04
    (96, 80, "lin_diou"): 4,    # 117 candidates, valid 100, margin 7.51e-04
    (96, 80, "lin_diou_agn"): 1,    # 119 candidates, valid 76, margin 2.72e-03
    (160, 80, "gauss_iou"): 6,    # 110 candidates, valid 100, margin 4.29e-04
    (160, 80, "gauss_iou_agn"): 6,    # 110 candidates, valid 47, margin 3.01e-04
    (160, 80, "gauss_diou"): 3,    # 99 candidates, valid 99, margin 4.75e-04
    (160, 80, "gauss_diou_agn"): 2,    # 100 candidates, valid 64, margin 2.52e-04
    (160, 80, "lin_iou"): 1,    # 104 candidates, valid 99, margin 7.69e-04
    (160, 80, "lin_iou_agn"): 1,    # 104 candidates, valid 67, margin 7.69e-04
    (160, 80, "lin_diou"): 2,    # 100 candidates, valid 99, margin 2.38e-04
    (160, 80, "lin_diou_agn"): 2,    # 100 candidates, valid 74, margin 2.38e-04
}
RANDOM_CASES = [(size, ncls, mode, seed) for (size, ncls, mode), seed in RANDOM_SEEDS.items()]


@functools.lru_cache(maxsize=None)
def random_case(size, ncls, seed):
    from yolo4hip.config import make_config
    ob, cb = RANDOM_BIAS[(size, ncls)]
    rng = np.random.default_rng([seed, size, ncls])
    heads = DC._random_heads(rng, 1, size, ncls, ob, cb)
    # twelve planted groups of two or three boxes of one class on horizontally adjacent stride-8 cells (anchor 0, centred), 24 .. 36
    # pixels wide -- IoU 0.5 .. 0.64 between neighbours -- with scores 0.55 .. 0.95: the pairs above iou_threshold that sparse
    # random heads lack, so that 'linear' has something to decay and the results hold decayed scores
    g = size // 8
    h0 = heads[0].reshape(1, g, g, 3, 5 + ncls)
    for _ in range(12):
        gy, gx, c, k = int(rng.integers(1, g - 1)), int(rng.integers(1, g - 3)), int(rng.integers(ncls)), int(rng.integers(2, 4))
        for j in range(k):
            h0[0, gy, gx + j, 0, :] = -20.0
            h0[0, gy, gx + j, 0, :4] = t_of(float(rng.uniform(24.0, 36.0)), float(rng.uniform(18.0, 26.0)))
            h0[0, gy, gx + j, 0, 4] = 8.0
            h0[0, gy, gx + j, 0, 5 + c] = logit_for(float(rng.uniform(0.55, 0.95)))
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    return heads, b, s
