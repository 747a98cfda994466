"""Test oracle of merge-NMS (y4_decode_nms_merged, y4_nms_gathered_merged; box_merge.hip): NumPy only.

After the NMS pair-rule oracle (nms_rule_oracle.combined_nms_rule) has decided the kept set, each kept box k -- unclipped box B_k,
class c_k, candidate id (box, class) -- is replaced by the score-weighted mean of its MEMBERS: the candidates j of the image's
whole list (every (box, class) with score > score_threshold, visited by NMS or not) with
    class_j == c_k (any class when `agnostic`)   and   measure(B_j, B_k) > iou_threshold      (float32, strict)
plus candidate k itself, recognised by its id.  A candidate with a component that is not finite or of magnitude above 2^8 is never
a member; a kept box with such a component is left as it is.

`nms_rule_oracle.measure(b, others)` is called with b = B_k and others = the candidates, the arguments the other way round than the
kernel's nms_measure(B_j, B_k): the measure is symmetric bit for bit on finite boxes (float addition, min and max commute, the
centre distance is squared), which tests/test_nms_merge_cpu.py asserts.

Accumulation is in integers and therefore independent of the order of the list:
    wq_j = rint(float64(score_j) * 2^30),  t_j[c] = rint(float64(score_j) * float64(B_j[c]) * 2^30)   as int64
    B'_k[c] = float32(float64(sum t_j[c]) / float64(sum wq_j))           (sum wq == 0: the box stays)
then the box map x -> float32(float64(x) * a + b) (the device's fmaf up to one double rounding of the sum, as tiled_oracle.map_boxes)
and the clip to [0, 1].

`min_margin` is the smallest |m - iou_threshold| over every membership decision that was made with the measure, in float32 and
again in float64 on the same float32 boxes, the smaller of the two."""
import numpy as np

import nms_rule_oracle as NR

F32 = np.float32
SCALE = float(2 ** 30)
MAX_ABS = F32(256.0)


def usable(boxes):
    """boxes [..., 4] -> bool [...]: every component finite and of magnitude at most 2^8."""
    b = np.asarray(boxes, F32)
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(b) <= MAX_ABS, axis=-1)           # (a NaN fails the comparison)


def fixed_sums(cand_boxes, cand_scores):
    """The int64 sums (S_w, S[4]) of a member list: boxes [M, 4] float32, scores [M] float32."""
    w = np.asarray(cand_scores, F32).astype(np.float64)
    b = np.asarray(cand_boxes, F32).astype(np.float64).reshape(-1, 4)
    wq = np.rint(w * SCALE).astype(np.int64)
    t = np.rint(w[:, None] * b * SCALE).astype(np.int64)
    return int(wq.sum(dtype=np.int64)), t.sum(axis=0, dtype=np.int64)


def mean_of_sums(sw, sc):
    return (np.asarray(sc, np.int64).astype(np.float64) / np.float64(np.int64(sw))).astype(F32)


def merge_one(kbox, kcls, kid, cand_boxes, cand_cls, cand_id, cand_scores, iou_thr, kind="iou", beta=1.0, agnostic=False):
    """One kept box against an explicit candidate list (any order): kbox [4] unclipped, its class and id; cand_* arrays of length M
    (boxes [M, 4], class, id = box * C + class, score).  -> (box' [4] float32 unclipped, member mask [M], min_margin)."""
    kbox = np.asarray(kbox, F32)
    cand_boxes = np.asarray(cand_boxes, F32).reshape(-1, 4)
    cand_cls, cand_id = np.asarray(cand_cls), np.asarray(cand_id)
    member = np.zeros(len(cand_id), bool)
    if not usable(kbox):
        return kbox.copy(), member, np.inf
    thr32 = F32(iou_thr)
    thr64 = np.float64(thr32)
    is_self = cand_id == kid
    elig = usable(cand_boxes) & (np.ones_like(is_self) if agnostic else cand_cls == kcls)
    test = elig & ~is_self
    margin = np.inf
    if test.any():
        m32 = NR.measure(kbox, cand_boxes[test], kind, beta, F32)
        m64 = NR.measure(kbox, cand_boxes[test], kind, beta, np.float64)
        with np.errstate(invalid="ignore"):
            d = np.concatenate([np.abs(m32.astype(np.float64) - thr64), np.abs(m64 - thr64)])
            member[test] = m32 > thr32
        d = d[np.isfinite(d)]
        if d.size:
            margin = float(d.min())
    member |= elig & is_self
    sw, sc = fixed_sums(cand_boxes[member], np.asarray(cand_scores, F32)[member])
    if sw == 0:
        return kbox.copy(), member, margin
    return mean_of_sums(sw, sc), member, margin


def map_and_clip(box, m=None):
    b = np.asarray(box, F32)
    if m is not None:
        m = np.asarray(m, F32).astype(np.float64)
        d = b.astype(np.float64)
        b = np.stack([d[..., 0] * m[0] + m[1], d[..., 1] * m[2] + m[3], d[..., 2] * m[0] + m[1], d[..., 3] * m[2] + m[3]], axis=-1).astype(F32)
    return np.clip(b, F32(0), F32(1))


def candidates(scores, score_thr):
    """scores [nbox, C] -> (box index [M], class [M], id [M], score [M]) of the image's list, in index order."""
    sc = np.asarray(scores, F32)
    bi, ci = np.nonzero(sc > F32(score_thr))
    return bi, ci, bi.astype(np.int64) * sc.shape[1] + ci, sc[bi, ci]


def merge_image(boxes, scores, kept_idx, kept_cls, valid, iou_thr, score_thr, kind="iou", beta=1.0, agnostic=False, box_map=None,
                total=None):
    """boxes [nbox, 4] unclipped, scores [nbox, C] of one image and its kept list -> (out boxes [total, 4] mapped and clipped, zero
    padded; member masks per kept box; min_margin)."""
    boxes = np.asarray(boxes, F32)
    T = len(kept_idx) if total is None else total
    bi, ci, ids, sc = candidates(scores, score_thr)
    C = np.asarray(scores).shape[1]
    out = np.zeros((T, 4), F32)
    masks, margin = [], np.inf
    for k in range(int(valid)):
        kb, kc = int(kept_idx[k]), int(kept_cls[k])
        merged, member, mg = merge_one(boxes[kb], kc, kb * C + kc, boxes[bi], ci, ids, sc, iou_thr, kind, beta, agnostic)
        out[k] = map_and_clip(merged, box_map)
        masks.append(member)
        margin = min(margin, mg)
    return out, masks, margin


def merged_nms(boxes, scores, per_class=100, total=100, iou_thr=0.413, score_thr=0.3, kind="iou", beta=1.0, agnostic=False,
               box_maps=None):
    """nms_rule_oracle.combined_nms_rule, then the merge: boxes [N, nbox, 4], scores [N, nbox, C] -> (boxes [N, T, 4], scores,
    classes, valid, kept_idx, min_margin of the NMS decisions, min_margin of the membership decisions, the plain NMS boxes --
    with box_maps applied to them as y4_decode_nms_mapped does)."""
    boxes = np.asarray(boxes, F32)
    pb, ps, pc, pv, pi, nms_margin = NR.combined_nms_rule(boxes, scores, per_class, total, iou_thr, score_thr, kind, beta, agnostic)
    out = np.zeros_like(pb)
    plain = pb.copy()
    margin = np.inf
    for n in range(boxes.shape[0]):
        bm = None if box_maps is None else box_maps[n]
        out[n], _, mg = merge_image(boxes[n], scores[n], pi[n], pc[n], pv[n], iou_thr, score_thr, kind, beta, agnostic, bm, total)
        margin = min(margin, mg)
        if bm is not None:
            v = int(pv[n])
            plain[n, :v] = map_and_clip(boxes[n, pi[n, :v]], bm)
    return out, ps, pc, pv, pi, nms_margin, margin, plain
