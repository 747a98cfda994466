"""Inputs for the Matrix-NMS tests (y4_set_nms_matrix): hand-made witnesses on the geometry of tests/soft_nms_cases.py, each of which
fails for one specific wrong kernel, two lists that tie the kernel to the ones that ship, and seeded random heads.  NumPy only:
tests/test_matrix_nms_cpu.py asserts every witness and every margin on the oracle (tests/matrix_nms_oracle.py) without a GPU,
tests/test_gpu_matrix_nms.py holds the kernel to the oracle on the same inputs.  The list lengths, the top_k = 64 list and the
4096-of-4097 stacks are soft_nms_cases' own (LENGTHS, topk_case, edge_case)."""
import functools

import numpy as np

import decode_nms_cases as DC
import soft_nms_cases as SC
from soft_nms_cases import entry

SIZE = SC.SIZE
# name -> (size, ncls, entries, engine caps, matrix keywords).  What each one shows is asserted in tests/test_matrix_nms_cpu.py
WITNESSES = {
    # A (0.9), E (0.85, IoU 1/9 with A), D (0.7, IoU 3/7 with both): D carries the SMALLER of its two terms, not their product
    "two_factors": SC.WITNESSES["two_factors"],
    # A (0.9), B (0.8, IoU 0.6 with A), C (0.7, 12 x 20: IoU 0.375 with B, 0.158 with A): B's own decay compensates what B does to C
    "chain": (SIZE, 3, [entry(5, 4, 1, 0.9, 32), entry(5, 5, 1, 0.8, 32), entry(5, 6, 1, 0.7, 12)], {}, {}),
    # A, B (IoU 0.6), C disjoint, one class: B' is Soft-NMS's B' bit for bit
    "order": SC.WITNESSES["order"],
    # the pair of `order` in two classes: no decay; `agnostic` decays
    "classes": SC.WITNESSES["classes"],
    # min_score 0.45: B' = 0.389 is gone; min_score = B' exactly: gone too (strict)
    "floor": SC.WITNESSES["floor"],
    # max_per_class = 1 under an agnostic rule: A (class 0) kept, A2 (class 0, disjoint from A) skipped, X (class 1, IoU 0.6 with A2) is
    # decayed by A2 all the same: decay is one-shot (Soft-NMS leaves X at 0.7)
    "skipped_still_decays": (SIZE, 3, SC.WITNESSES["turned_away"][2], {"max_per_class": 1}, {"min_score": 0.1}),
    "max_total": SC.WITNESSES["max_total"],
    "ties": SC.WITNESSES["ties"],
    "empty": SC.WITNESSES["empty"],
    # one box in three classes under an agnostic linear rule: IoU 1, c = 1 for the second -- its term for the third is left out, and the
    # first one's term (1 - 1) / (1 - 0) makes the third score 0
    "identical": (SIZE, 3, [entry(5, 5, 0, 0.9), entry(5, 5, 1, 0.8), entry(5, 5, 2, 0.7)], {}, {"min_score": 0.0}),
}


@functools.lru_cache(maxsize=None)
def witness(name):
    """-> (size, ncls, heads, boxes, scores, caps, matrix keywords): one image."""
    from yolo4hip.config import make_config
    size, ncls, entries, caps, kw = WITNESSES[name]
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    return size, ncls, heads, b, s, dict(caps), dict(kw)


# ---- every interacting pair disjoint: 300 boxes of 6 x 6 pixels on distinct stride-8 cells at 160^2, 80 classes, scores 0.31 .. 0.95.
# Nothing decays: all five outputs are the hard kernel's.
@functools.lru_cache(maxsize=None)
def disjoint_case():
    from yolo4hip.config import make_config
    size, ncls = SC.SIZE_LEN, SC.NCLS_LEN
    rng = np.random.default_rng(11)
    cells = rng.permutation(400)[:300]
    entries = [entry(int(c) // 20, int(c) % 20, int(rng.integers(ncls)), float(rng.uniform(0.31, 0.95)), 6.0, 6.0) for c in cells]
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    assert int((s > np.float32(SC.SCORE_THR)).sum()) == 300
    return heads, b, s


# ---- two candidates per class, 80 classes at 160^2: the pair of class c on two adjacent cells, 24 .. 36 pixels wide (IoU 0.5 .. 0.64),
# scores 0.5 .. 0.95.  c = 0 for both, so gaussian Matrix-NMS is gaussian Soft-NMS: all five outputs bit for bit.
PAIRS_SEED = 2                             # (chosen like the seeds of RANDOM_SEEDS, for gaussian and linear 'iou')


@functools.lru_cache(maxsize=None)
def pairs_case(seed=None):
    from yolo4hip.config import make_config
    size, ncls = SC.SIZE_LEN, SC.NCLS_LEN
    rng = np.random.default_rng([12, PAIRS_SEED if seed is None else seed])
    entries = []
    for c in range(ncls):
        gy, gx = c // 4, 5 * (c % 4) + 1
        for j in range(2):
            entries.append(entry(gy, gx + j, c, float(rng.uniform(0.5, 0.95)), float(rng.uniform(24.0, 36.0)), float(rng.uniform(18.0, 26.0))))
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    assert int((s > np.float32(SC.SCORE_THR)).sum()) == 2 * ncls
    return heads, b, s


# ---- seeded random heads, one image each (soft_nms_cases.random_case: random heads with planted overlapping groups).  MODES: the
# (method, kind, beta, agnostic) every input runs under.  A seed is in the table because the float64 face reports a margin of at least
# MARGIN_BAR for it under that mode (tests/test_matrix_nms_cpu.py asserts it); one that misses is replaced HERE, never skipped at run time.
MARGIN_BAR = SC.MARGIN_BAR
MODES = {k: v for k, v in SC.MODES.items()}
LENGTH_MODES = SC.LENGTH_MODES
# soft_nms_cases.length_case(L, seed): the seed under which both LENGTH_MODES clear the bar for this rule
LENGTH_SEEDS = {L: (1 if L == 1023 else 0) for L in SC.LENGTHS}
SHAPES = ((96, 3), (160, 80))
# (size, classes, mode) -> seed
RANDOM_SEEDS = {
    (96, 3, "gauss_iou"): 0,    # 170 candidates, valid 100, 73 decayed, margin 1.14e-04
    (96, 3, "gauss_iou_agn"): 1,    # 161 candidates, valid 100, 89 decayed, margin 1.94e-04
    (96, 3, "gauss_diou"): 0,    # 170 candidates, valid 100, 52 decayed, margin 2.89e-04
    (96, 3, "gauss_diou_agn"): 0,    # 170 candidates, valid 100, 69 decayed, margin 2.86e-04
    (96, 3, "lin_iou"): 0,    # 170 candidates, valid 100, 71 decayed, margin 3.61e-04
    (96, 3, "lin_iou_agn"): 5,    # 171 candidates, valid 83, 72 decayed, margin 1.61e-04
    (96, 3, "lin_diou"): 1,    # 161 candidates, valid 100, 50 decayed, margin 1.07e-04
    (96, 3, "lin_diou_agn"): 0,    # 170 candidates, valid 100, 67 decayed, margin 1.30e-04
    (160, 80, "gauss_iou"): 0,    # 104 candidates, valid 100, 19 decayed, margin 1.74e-04
    (160, 80, "gauss_iou_agn"): 0,    # 104 candidates, valid 64, 50 decayed, margin 4.70e-04
    (160, 80, "gauss_diou"): 0,    # 104 candidates, valid 100, 18 decayed, margin 6.75e-04
    (160, 80, "gauss_diou_agn"): 0,    # 104 candidates, valid 70, 35 decayed, margin 6.88e-04
    (160, 80, "lin_iou"): 1,    # 104 candidates, valid 99, 19 decayed, margin 7.69e-04
    (160, 80, "lin_iou_agn"): 0,    # 104 candidates, valid 55, 41 decayed, margin 1.70e-04
    (160, 80, "lin_diou"): 0,    # 104 candidates, valid 100, 18 decayed, margin 2.86e-04
    (160, 80, "lin_diou_agn"): 1,    # 104 candidates, valid 65, 31 decayed, margin 1.35e-03
}
RANDOM_CASES = [(size, ncls, mode, seed) for (size, ncls, mode), seed in RANDOM_SEEDS.items()]
random_case = SC.random_case


# ---- the class cap (max_per_class below max_total takes a pass of its own).  Random heads at (96, 3) under caps, seeds chosen like
# RANDOM_SEEDS: (max_per_class, max_total, mode) -> seed; and decode_nms_cases' later-chunk stack and disjoint grid under its cap pairs
CAP_SEEDS = {
    (3, 100, "gauss_iou"): 12,    # valid 9, 2 decayed, margin 1.14e-04
    (3, 100, "lin_iou_agn"): 5,    # valid 9, 3 decayed, margin 1.61e-04
    (2, 10, "lin_iou_agn"): 5,    # valid 6, 2 decayed, margin 1.61e-04
    (8, 20, "gauss_iou"): 0,    # valid 20, 7 decayed, margin 1.80e-03
    (8, 20, "lin_iou_agn"): 0,    # valid 20, 12 decayed, margin 1.89e-03
}
CAP_RANDOM = [(pc, t, mode, seed) for (pc, t, mode), seed in CAP_SEEDS.items()]
CAP_INPUTS = ("s2500", "grid2704")
CAP_MODES = ("gauss_iou", "lin_iou_agn")
