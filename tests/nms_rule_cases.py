"""Inputs for the NMS pair-rule tests (y4_set_nms_rule), each with a witness -- a property of the input, computed from the oracle
alone -- that its deciding pair is tested at the place of nms_kernel it is meant for.  Built on tests/decode_nms_cases.py; NumPy
only (tests/test_nms_rule_cpu.py asserts the witnesses without a GPU, tests/test_gpu_nms_rule.py holds the kernel to the oracle).

The WITNESS PAIR is the worked example of tests/test_nms_rule_cpu.py: anchor 0 of two horizontally adjacent stride-8 cells,
t_xy = 0 (centres 8 px apart), t_wh such that both boxes are 20 x 20 px: iou = 12/28 = 0.4286 > 0.413, iou - d2/c2 = 0.3745 and
iou - (d2/c2)^0.6 = 0.2550, both < 0.413.  'iou' keeps one box of a same-class pair, 'diou' keeps both.

The places (decode_nms.hip):
  par         first chunk, C <= PAR_MAX_C, class-aware: the round-parallel pass;
  wave0_first first chunk through wave 0: C > PAR_MAX_C, or any agnostic rule; the pair at positions 0 and 1 shares a batch;
  later_prev  a later chunk, the earlier box kept in a PREVIOUS 64-candidate batch (the loop over the kept list): the pair is ranked
              behind the first chunk's 1024 candidates at most and its two boxes lie at least 64 positions apart, so wherever a
              batch starts they are not in one;
  later_same  a later chunk, both boxes in ONE batch (the survivors loop): TWO pairs on the last four positions p .. p + 3, as
              (p, p + 1) and (p + 2, p + 3): a batch boundary can part one of them, never both, so at least one pair is decided
              inside a batch, and either pair decided wrongly changes the result."""
import functools

import numpy as np

import decode_nms_cases as DC
import nms_rule_oracle as NR

IOU_THR, SCORE_THR = 0.413, 0.3            # config.py's thresholds (make_config)
ANCHOR0 = (12.0, 16.0)                     # anchor 0 of scale 0 (config.py)
T_WH = (float(np.log(20.0 / ANCHOR0[0])), float(np.log(20.0 / ANCHOR0[1])))
T_PAIR = (0.0, 0.0) + T_WH


def pair(image, gy, gx, cls_a, cls_b, lc_a, lc_b, lo=8.0):
    """Two entries for `_heads_with`: the witness pair on cells (gy, gx) and (gy, gx + 1), class logits lc_a > lc_b."""
    return [(image, 0, gy, gx, 0, cls_a, lo, lc_a, T_PAIR), (image, 0, gy, gx + 1, 0, cls_b, lo, lc_b, T_PAIR)]


PLACES = ("par", "later_prev", "later_same", "wave0_first")


@functools.lru_cache(maxsize=None)
def witness_case(place, other_class=False):
    """-> (size, ncls, heads, boxes, scores, pairs): one image; `pairs` lists the (box index a, box index b) of its witness pairs.
    other_class: the second box of every pair is of another class than the first (the agnostic witnesses)."""
    from yolo4hip.config import make_config
    extra, spots = [], []                      # spots: (gy, gx, class logit of a, of b) of every witness pair
    if place == "par":
        size, ncls = 160, 3
        ca, cb = 1, (2 if other_class else 1)
        spots = [(5, 7, 2.0, 1.0)]
        extra = [(0, 0, 15, 2, 0, 0, 8.0, 3.0, T_PAIR), (0, 1, 2, 2, 1, 1, 8.0, 0.5, (0.0, 0.0, 0.0, 0.0))]
    elif place == "wave0_first":
        size, ncls = 96, DC.PAR_MAX_C + 1
        ca, cb = ncls - 1, (3 if other_class else ncls - 1)
        spots = [(4, 5, 2.0, 1.0)]
    else:
        size, ncls = DC.SIZE_CHUNK, 3
        ca, cb = 1, (2 if other_class else 1)
        extra = DC.stack_boxes(size, 1300, seed=1300, ncls=ncls, stack_cls=0)
        # the stack's class logits are uniform in [0, 3] under objectness logit 8.  later_prev: box a (logit 0.25) has about a
        # twelfth of the stack behind it, box b (logit -0.5) all of it.  later_same: all four behind the stack
        spots = [(30, 20, 0.25, -0.5)] if place == "later_prev" else [(30, 20, -0.5, -0.6), (10, 40, -0.7, -0.8)]
    entries = list(extra)
    for gy, gx, la, lb in spots:
        entries += pair(0, gy, gx, ca, cb, la, lb)
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    g = size // 8
    pairs = [(3 * (gy * g + gx), 3 * (gy * g + gx + 1)) for gy, gx, _, _ in spots]      # box index: scale 0, anchor 0
    return size, ncls, heads, b, s, pairs


def pair_ranks(place, other_class=False):
    """-> (T, [(rank of a, rank of b) per witness pair]) in the candidate order."""
    _, _, _, _, s, pairs = witness_case(place, other_class)
    order = DC.candidate_order(s[0], SCORE_THR)
    first = {}
    for i, (bi, _) in enumerate(order):
        first.setdefault(int(bi), i)            # (a witness box has one candidate)
    return len(order), [(first[a], first[b]) for a, b in pairs]


def place_holds(place, other_class=False):
    """The witness of `witness_case(place)`: True when the ranks put the deciding test where the place says."""
    _, ncls, _, _, _, _ = witness_case(place, other_class)
    T, ranks = pair_ranks(place, other_class)
    if place == "par":
        return T <= DC.NMS_THREADS and ncls <= DC.PAR_MAX_C
    if place == "wave0_first":
        return ncls > DC.PAR_MAX_C and ranks == [(0, 1)]
    later = T > DC.NMS_THREADS and all(ra >= DC.NMS_THREADS for ra, _ in ranks)       # behind any first chunk
    if place == "later_prev":
        return later and all(rb - ra >= 64 for ra, rb in ranks)
    return later and sorted(r for p in ranks for r in p) == [T - 4, T - 3, T - 2, T - 1] and all(rb == ra + 1 for ra, rb in ranks)


@functools.lru_cache(maxsize=None)
def witness_reference(place, other_class, kind, beta, agnostic, per_class=100, total=100):
    _, _, _, b, s, _ = witness_case(place, other_class)
    return NR.combined_nms_rule(b, s, per_class, total, IOU_THR, SCORE_THR, kind, beta, agnostic)


def kept_boxes(ref):
    """The set of kept box indices of image 0."""
    return set(int(i) for i in ref[4][0][:int(ref[3][0])])


# ---- the class cap under an agnostic rule: class 0's second candidate is turned away by max_per_class = 1 and must not suppress the
# class-1 box that overlaps it
@functools.lru_cache(maxsize=None)
def cap_case():
    from yolo4hip.config import make_config
    size, ncls = 160, 3
    entries = [(0, 0, 15, 2, 0, 0, 8.0, 3.0, T_PAIR)] + pair(0, 5, 7, 0, 1, 2.0, 1.0)
    heads = DC._heads_with(size, ncls, 1, entries)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(size), size)
    return size, ncls, heads, b, s


# ---- random heads.  (ncls, seed, rule, min_margin the oracle reports): the seeds were chosen so that no tested pair of any image
# lies within 1e-5 of the threshold under that rule -- the tests assert it
RULES = {"diou1": ("diou", 1.0, False), "diou06": ("diou", 0.6, False), "agn_iou": ("iou", 1.0, True), "agn_diou06": ("diou", 0.6, True)}
# (classes, seed, rule, the oracle's min_margin over both images): seeds chosen on the CPU so that min_margin >= 1e-5
RANDOM_CASES = [
    (3, 3, "diou1", 1.49e-3), (3, 3, "diou06", 1.88e-2), (3, 3, "agn_iou", 8.34e-4), (3, 3, "agn_diou06", 9.78e-3),
    (3, 6, "diou1", 3.65e-3), (3, 6, "diou06", 1.24e-3), (3, 6, "agn_iou", 5.10e-3), (3, 6, "agn_diou06", 1.24e-3),
    (80, 3, "diou1", 3.12e-2), (80, 3, "diou06", 1.14e-3), (80, 3, "agn_iou", 2.55e-3), (80, 3, "agn_diou06", 1.14e-3),
    (80, 4, "diou1", 1.56e-1), (80, 4, "diou06", 2.85e-1), (80, 4, "agn_iou", 2.50e-3), (80, 4, "agn_diou06", 1.15e-2),
]


# ---- a rule that goes on in a LATER chunk: the stack-and-disjoint images of decode_nms_cases under a non-default rule.  The first
# chunk leaves its kept lists through the DIoU round-parallel pass, or through the agnostic wave-0 pass; the later chunk is sorted
# (rank sort for s1300, nms_sort_regs for s2500) and decided by the wave-0 pass of that rule, continuing from those lists.
LATER_CHUNK_CASES = [(name, rule) for name in ("s1300", "s2500") for rule in ("diou06", "agn_iou")]


@functools.lru_cache(maxsize=None)
def later_chunk_reference(name, rule):
    _, b, s = DC.chunk_case(name)
    kind, beta, agn = RULES[rule]
    return NR.combined_nms_rule(b, s, 100, 100, IOU_THR, SCORE_THR, kind, beta, agn)


def rank_of_last_kept_under(scores, ref):
    """Position of the last kept box of `ref` (image 0) in the candidate order of `scores` [nbox, C]."""
    return DC.rank_of_last_kept(DC.candidate_order(scores, SCORE_THR), ref[4][0], ref[2][0], ref[3][0])


def later_chunk_witness(name, rule):
    """`DC.chunk_witness` of the input under the rule, with the ranks of all kept boxes."""
    _, _, s = DC.chunk_case(name)
    ref = later_chunk_reference(name, rule)
    w = DC.chunk_witness(s[0], SCORE_THR, (ref[4][0], ref[2][0], ref[3][0]))
    w["ranks"] = DC.ranks_of_kept(DC.candidate_order(s[0], SCORE_THR), ref[4][0], ref[2][0], ref[3][0])
    return w


RANDOM_N, RANDOM_SIZE = 2, 160
RANDOM_BIAS = {3: (1.0, 0.0), 80: (-0.5, -1.5)}       # C -> (objectness bias, class bias): crowded classes at either count


@functools.lru_cache(maxsize=None)
def random_case(ncls, seed):
    from yolo4hip.config import make_config
    ob, cb = RANDOM_BIAS[ncls]
    heads = DC._random_heads(np.random.default_rng(seed), RANDOM_N, RANDOM_SIZE, ncls, ob, cb)
    b, s = DC.boxes_and_scores(heads, ncls, make_config(RANDOM_SIZE), RANDOM_SIZE)
    return heads, b, s


@functools.lru_cache(maxsize=None)
def random_reference(ncls, seed, rule):
    _, b, s = random_case(ncls, seed)
    kind, beta, agn = RULES[rule]
    return NR.combined_nms_rule(b, s, 100, 100, IOU_THR, SCORE_THR, kind, beta, agn)
