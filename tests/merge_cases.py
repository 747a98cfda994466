"""Inputs of the merge-NMS tests (y4_decode_nms_merged, y4_nms_gathered_merged) with what the oracle (tests/merge_oracle.py) says
about them on the CPU.  NumPy only: tests/test_nms_merge_cpu.py asserts the recorded figures and witnesses without a GPU,
tests/test_gpu_nms_merge.py holds the kernel to the oracle, bit for bit on boxes, on the same inputs.

Every recorded margin is the oracle's smallest |m - iou_threshold| over the MEMBERSHIP decisions of the case (all images), with the
oracle's own decode in front; the seeds were chosen so that it is at least 3e-5 -- the device's decode differs from NumPy's in the
last bit or two of a box (its expf), which moves a measure by ~1e-7, so the same decisions fall the same way on the device's boxes,
where the GPU tests assert >= 1e-5 again."""
import functools

import numpy as np

import decode_nms_cases as DC
import merge_oracle as MO
import nms_rule_cases as RC

IOU_THR, SCORE_THR = RC.IOU_THR, RC.SCORE_THR
RULES = {"iou": ("iou", 1.0, False), "diou06": ("diou", 0.6, False), "agn_iou": ("iou", 1.0, True)}
MIN_MARGIN = 3e-5

# ---- (a) the random heads of nms_rule_cases.random_case (2 images at 160^2): (classes, seed, rule, membership margin)
RANDOM_CASES = [
    (3, 3, "iou", 1.04e-4), (3, 3, "diou06", 2.57e-4), (3, 3, "agn_iou", 1.04e-4),
    (3, 8, "iou", 1.47e-4), (3, 8, "diou06", 2.22e-4), (3, 8, "agn_iou", 1.47e-4),
    (80, 4, "iou", 3.98e-3), (80, 4, "diou06", 3.88e-3), (80, 4, "agn_iou", 4.17e-4),
    (80, 2, "iou", 1.75e-3), (80, 2, "diou06", 1.52e-3), (80, 2, "agn_iou", 3.13e-4),
]


@functools.lru_cache(maxsize=None)
def random_reference(ncls, seed, rule):
    _, b, s = RC.random_case(ncls, seed)
    return MO.merged_nms(b, s, 100, 100, IOU_THR, SCORE_THR, *RULES[rule])


# ---- (c) later chunks: the stack-and-disjoint images of decode_nms_cases (416^2, C = 2).  The stack's boxes are some 18 image
# sides wide, so the test maps them into view: x -> x / 64 + 0.5 keeps the mean of the stack inside [0, 1], where the clip does not
# hide it.  (name, max_total): with max_total = 55 NMS has its boxes after 55 candidates -- the 54 disjoint boxes above the stack and
# the stack's best -- and never takes a second chunk; with 100 it walks the whole stack.
CHUNK_MAP = np.array([[1.0 / 64, 0.5, 1.0 / 64, 0.5]], np.float32)
CHUNK_CASES = [("s1300", 55), ("s2500", 100)]


@functools.lru_cache(maxsize=None)
def chunk_reference(name, total):
    _, b, s = DC.chunk_case(name)
    return MO.merged_nms(b, s, 100, total, IOU_THR, SCORE_THR, box_maps=CHUNK_MAP)


def chunk_witness(boxes, scores, ref, total):
    """From the oracle alone, for the kept STACK box (class 0) of a chunk case: its slot, the candidate ranks of its members, the
    rank of the last kept box, and its merged box when only the first NMS_THREADS candidates count."""
    order = DC.candidate_order(scores[0], SCORE_THR)
    rank = {(int(b), int(c)): i for i, (b, c) in enumerate(order)}
    v = int(ref[3][0])
    slot = [k for k in range(v) if ref[2][0][k] == 0.0]
    assert len(slot) == 1
    k = slot[0]
    _, masks, _ = MO.merge_image(boxes[0], scores[0], ref[4][0], ref[2][0], v, IOU_THR, SCORE_THR, total=total)
    bi, ci, ids, sc = MO.candidates(scores[0], SCORE_THR)
    ranks = np.array([rank[(int(b), int(c))] for b, c in zip(bi, ci)])
    member_ranks = ranks[masks[k]]
    last_kept = DC.rank_of_last_kept(order, ref[4][0], ref[2][0], v)
    head = ranks < DC.NMS_THREADS
    kb, kc = int(ref[4][0][k]), 0
    only_head, _, _ = MO.merge_one(boxes[0, kb], kc, kb * scores.shape[2] + kc, boxes[0][bi[head]], ci[head], ids[head], sc[head], IOU_THR)
    return {"slot": k, "member_ranks": member_ranks, "last_kept": last_kept,
            "head_only": MO.map_and_clip(only_head, CHUNK_MAP[0])}


# ---- (d) caps: (input of decode_nms_cases.cap_input, max_per_class, max_total)
CAP_CASES = [("small6", 3, 10), ("small6", 5, 7)]


@functools.lru_cache(maxsize=None)
def cap_reference(name, per_class, total):
    _, _, _, b, s = DC.cap_input(name)
    return MO.merged_nms(b, s, per_class, total, IOU_THR, SCORE_THR)


# ---- (e) the box maps of tests/test_gpu_nms_rule.py's mapped test, on random case (3, 3)
MAPS = np.array([[1.25, -0.125, 1.0, 0.0], [1.0, 0.0, 1.6, -0.3]], np.float32)

# ---- (f) gathered: (classes, seed, rule of tiled_cases.RULES) of tiled_cases, membership margins over both photos
TILED_CASES = [(3, 0, "iou", 1.14e-4), (3, 0, "diou06", 4.91e-4), (80, 0, "iou", 1.41e-3), (80, 1, "agn_iou", 2.37e-4)]


@functools.lru_cache(maxsize=None)
def tiled_reference(ncls, seed, rule):
    """-> per photo of tiled_cases, the merged oracle on the oracle's group tables."""
    import tiled_cases as TC
    import tiled_oracle as TO
    from yolo4hip.config import make_config
    _, group, _, maps, _ = TC.geometry()
    out = []
    for hd, mp in TC.groups_of(TC.heads(ncls, seed), group, maps):
        gb, gs = TO.group_tables(hd, mp, ncls, make_config(TC.SIZE), TC.SIZE)
        out.append(MO.merged_nms(gb, gs, 100, 100, TC.IOU_THR, TC.SCORE_THR, *TC.RULES[rule]))
    return out
