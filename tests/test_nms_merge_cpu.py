"""Merge-NMS on the CPU: the rule of tests/merge_oracle.py on known answers, its order independence and error bound, and the
recorded margins and witnesses of tests/merge_cases.py that the GPU tests (tests/test_gpu_nms_merge.py) rely on.  No GPU."""
import numpy as np
import pytest

import decode_nms_cases as DC
import merge_cases as MC
import merge_oracle as MO
import nms_rule_cases as RC
import nms_rule_oracle as NR

F32 = np.float32
THR = MC.IOU_THR


def _list(boxes, scores, classes, ncls=3):
    """An explicit candidate list: box j has index j."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    classes = np.asarray(classes)
    return boxes, classes, np.arange(len(boxes)) * ncls + classes, np.asarray(scores, F32)


def _float64_mean(boxes, scores, member):
    w = np.asarray(scores, F32).astype(np.float64)[member]
    b = np.asarray(boxes, F32).astype(np.float64)[member]
    return (w[:, None] * b).sum(axis=0) / w.sum()


def _bound(mean, s_min):
    """2^-31 (1 + |mean|) / s_min for the members' roundings, plus one float32 rounding of the quotient (half an ulp: 2^-24
    relative, 2^-150 absolute below the normal range)."""
    return 2.0 ** -31 * (1.0 + np.abs(mean)) / float(s_min) + 2.0 ** -24 * np.abs(mean) + 2.0 ** -150


# ------------------------------------------------------------------------------------------------ the measure is symmetric
@pytest.mark.parametrize("kind,beta", [("iou", 1.0), ("diou", 1.0), ("diou", 0.6)])
def test_measure_is_symmetric_bit_for_bit(kind, beta):
    """The oracle calls measure(B_k, candidates), the kernel nms_measure(B_j, B_k): the same bits either way on finite boxes."""
    _, b, s = RC.random_case(3, 3)
    cand = b[0][(s[0] > F32(MC.SCORE_THR)).any(axis=1)][:300]
    for k in range(0, 300, 37):
        fwd = NR.measure(cand[k], cand, kind, beta)
        back = np.array([NR.measure(c, cand[k:k + 1], kind, beta)[0] for c in cand], F32)
        assert np.array_equal(fwd.view(np.int32), back.view(np.int32))


# ------------------------------------------------------------------------------------------------ known answers
def test_two_boxes_give_the_hand_computed_weighted_mean():
    """Scores 0.75 and 0.5, dyadic corners: every fixed-point term is exact, so the result is float32 of the exact rational.
    IoU = 0.25 / 0.3125 = 0.8.  x2: (0.75 * 0.75 + 0.5 * 0.875) / 1.25 = 0.8; the other three corners coincide."""
    boxes, cls, ids, sc = _list([[0.25, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.875]], [0.75, 0.5], [1, 1])
    got, member, margin = MO.merge_one(boxes[0], 1, ids[0], boxes, cls, ids, sc, THR)
    assert member.tolist() == [True, True]
    assert np.array_equal(got, np.array([0.25, 0.25, 0.75, F32(0.8)], F32))
    assert abs(margin - (0.8 - float(F32(THR)))) < 1e-6
    sw, s4 = MO.fixed_sums(boxes, sc)
    assert sw == 5 * 2 ** 28 and s4.tolist() == [5 * 2 ** 26, 5 * 2 ** 26, 15 * 2 ** 26, 2 ** 30]


def test_a_stack_of_identical_boxes_returns_the_box():
    """Thirty copies with thirty scores: numerator and denominator are each off by at most 15 units of 2^-30, the quotient by
    2^-31 (1 + |B|) / s_min <= 2^-28.4 -- under half an ulp (>= 2^-27) of a component in [0.2, 0.9], so float32 returns B."""
    rng = np.random.default_rng(5)
    for _ in range(20):
        lo = rng.uniform(0.2, 0.5, 2)
        box = np.concatenate([lo, lo + rng.uniform(0.1, 0.4, 2)]).astype(F32)
        sc = rng.uniform(0.3, 1.0, 30).astype(F32)
        boxes, cls, ids, sc = _list(np.tile(box, (30, 1)), sc, np.full(30, 2))
        got, member, _ = MO.merge_one(box, 2, ids[7], boxes, cls, ids, sc, THR)
        assert member.all() and np.array_equal(got.view(np.int32), box.view(np.int32))


def test_permuting_or_regrouping_the_list_changes_no_bit():
    _, b, s = RC.random_case(3, 8)
    ref = MC.random_reference(3, 8, "iou")
    bi, ci, ids, sc = MO.candidates(s[0], MC.SCORE_THR)
    rng = np.random.default_rng(0)
    for k in range(0, int(ref[3][0]), 9):
        kb, kc = int(ref[4][0][k]), int(ref[2][0][k])
        want, member, _ = MO.merge_one(b[0, kb], kc, kb * 3 + kc, b[0][bi], ci, ids, sc, THR)
        for _ in range(3):
            p = rng.permutation(len(ids))
            got, _, _ = MO.merge_one(b[0, kb], kc, kb * 3 + kc, b[0][bi[p]], ci[p], ids[p], sc[p], THR)
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
        # any reduction tree: partial sums over random groups of the members, added in random order
        mb, ms = b[0][bi[member]], sc[member]
        cuts = np.sort(rng.integers(0, len(ms) + 1, 5))
        parts = [MO.fixed_sums(mb[lo:hi], ms[lo:hi]) for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, len(ms)])]
        rng.shuffle(parts)
        sw = sum(p[0] for p in parts)
        s4 = sum((p[1] for p in parts), np.zeros(4, np.int64))
        assert np.array_equal(MO.mean_of_sums(sw, s4).view(np.int32), want.view(np.int32))
        assert np.array_equal(MO.map_and_clip(want).view(np.int32), ref[0][0][k].view(np.int32))


@pytest.mark.parametrize("ncls,seed,rule,margin", MC.RANDOM_CASES)
def test_result_is_within_the_derived_bound_of_the_float64_mean(ncls, seed, rule, margin):
    """The random cases at the config's score threshold (0.3 = s_min's lower bound): every merged box lies within
    2^-31 (1 + |mean|) / s_min plus one float32 rounding of the float64 weighted mean of its members.  Also the recorded margin."""
    _, b, s = RC.random_case(ncls, seed)
    ref = MC.random_reference(ncls, seed, rule)
    assert ref[6] >= MC.MIN_MARGIN and abs(ref[6] - margin) <= 0.01 * margin
    assert ref[5] >= 1e-5
    kind, beta, agn = MC.RULES[rule]
    moved = 0
    for n in range(b.shape[0]):
        bi, ci, ids, sc = MO.candidates(s[n], MC.SCORE_THR)
        v = int(ref[3][n])
        for k in range(v):
            kb, kc = int(ref[4][n][k]), int(ref[2][n][k])
            got, member, _ = MO.merge_one(b[n, kb], kc, kb * ncls + kc, b[n][bi], ci, ids, sc, THR, kind, beta, agn)
            assert member.sum() >= 1 and member[ids == kb * ncls + kc].all()
            mean = _float64_mean(b[n][bi], sc, member)
            assert (np.abs(got.astype(np.float64) - mean) <= _bound(mean, sc[member].min())).all()
            moved += int(member.sum() > 1)
        assert not ref[0][n, v:].any()
    assert moved >= 20
    # everything but the boxes is the plain NMS oracle's
    plain = NR.combined_nms_rule(b, s, 100, 100, THR, MC.SCORE_THR, kind, beta, agn)
    for k in (1, 2, 3, 4):
        assert np.array_equal(ref[k], plain[k])
    assert np.array_equal(ref[7], plain[0]) and not np.array_equal(ref[0], plain[0])


# ------------------------------------------------------------------------------------------------ excluded boxes
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 257.0, -300.0])
def test_a_box_with_a_huge_or_nan_component_neither_joins_nor_is_merged(bad):
    good = [[0.25, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.875]]
    broken = [0.25, 0.25, 0.75, bad]
    boxes, cls, ids, sc = _list(good + [broken], [0.75, 0.5, 0.9], [1, 1, 1])
    got, member, _ = MO.merge_one(boxes[0], 1, ids[0], boxes, cls, ids, sc, THR)
    assert member.tolist() == [True, True, False]
    assert np.array_equal(got, np.array([0.25, 0.25, 0.75, F32(0.8)], F32))
    kept_bad, member, _ = MO.merge_one(boxes[2], 1, ids[2], boxes, cls, ids, sc, THR)
    assert not member.any() and np.array_equal(kept_bad.view(np.int32), boxes[2].view(np.int32))
    # 256 itself is allowed
    edge, _, _, _ = _list([[0.0, 0.0, 256.0, 256.0]], [0.5], [1])
    assert MO.usable(edge).all() and not MO.usable(np.array([[0.0, 0.0, np.nextafter(F32(256), F32(300)), 1.0]], F32)).any()


def test_overflowing_heads_leave_their_kept_boxes_unmerged():
    """decode_nms_cases.overflow_heads: wh logits of 95 give inf corners.  A kept box with an inf corner comes out as the plain
    NMS writes it (clipped), and no inf box is a member of anything."""
    from yolo4hip.config import make_config
    heads = DC.overflow_heads()
    with np.errstate(over="ignore", invalid="ignore"):
        b, s = DC.boxes_and_scores(heads, 3, make_config(96), 96)
        ref = MO.merged_nms(b, s, 100, 100, THR, MC.SCORE_THR)
        v = int(ref[3][0])
        bad_kept = [k for k in range(v) if not MO.usable(b[0, ref[4][0][k]])]
        assert bad_kept
        for k in bad_kept:
            assert np.array_equal(ref[0][0][k], ref[7][0][k])
        bi, ci, ids, sc = MO.candidates(s[0], MC.SCORE_THR)
        _, masks, _ = MO.merge_image(b[0], s[0], ref[4][0], ref[2][0], v, THR, MC.SCORE_THR)
    assert not any(m[~MO.usable(b[0][bi])].any() for m in masks)
    assert np.isfinite(ref[0]).all()


# ------------------------------------------------------------------------------------------------ class scope and DIoU
def test_a_candidate_of_another_class_is_a_member_only_under_agnostic():
    boxes, cls, ids, sc = _list([[0.25, 0.25, 0.75, 0.75], [0.25, 0.25, 0.75, 0.875]], [0.75, 0.5], [1, 2])
    got, member, _ = MO.merge_one(boxes[0], 1, ids[0], boxes, cls, ids, sc, THR)
    assert member.tolist() == [True, False] and np.array_equal(got, boxes[0])
    got, member, _ = MO.merge_one(boxes[0], 1, ids[0], boxes, cls, ids, sc, THR, agnostic=True)
    assert member.tolist() == [True, True] and got[3] == F32(0.8)
    # the cap case of nms_rule_cases under an agnostic rule with max_per_class = 1: class 0's second candidate (box 321) is turned
    # away by the cap, the class-1 box next to it (324) is kept -- and absorbs it
    _, _, _, b, s = RC.cap_case()
    ref = MO.merged_nms(b, s, 1, 100, THR, MC.SCORE_THR, "iou", 1.0, True)
    assert ref[4][0][:2].tolist() == [906, 324] and ref[3][0] == 2
    _, masks, _ = MO.merge_image(b[0], s[0], ref[4][0], ref[2][0], 2, THR, MC.SCORE_THR, agnostic=True)
    bi, ci, _, _ = MO.candidates(s[0], MC.SCORE_THR)
    assert sorted(zip(bi[masks[1]].tolist(), ci[masks[1]].tolist())) == [(321, 0), (324, 1)]
    assert ref[0][0][1][0] < ref[7][0][1][0] and np.array_equal(ref[0][0][0], ref[7][0][0])
    aware = MO.merged_nms(b, s, 1, 100, THR, MC.SCORE_THR, "iou", 1.0, False)
    assert np.array_equal(aware[0][0][1], aware[7][0][1])


@pytest.mark.parametrize("beta", [1.0, 0.6])
def test_under_diou_the_witness_pair_stays_apart(beta):
    """nms_rule_cases' witness pair: IoU 0.4286 > 0.413 but IoU - (d2 / c2)^beta <= 0.413.  Under 'iou' one box is kept and absorbs
    the other; under 'diou' both are kept, neither is in the other's mean, and both boxes come out as they went in."""
    _, ncls, _, b, s, pairs = RC.witness_case("par")
    (pa, pb), = pairs
    assert float(NR.measure(b[0, pa], b[0, pb:pb + 1], "iou")[0]) > THR
    assert float(NR.measure(b[0, pa], b[0, pb:pb + 1], "diou", beta)[0]) <= THR
    iou = MO.merged_nms(b, s, 100, 100, THR, MC.SCORE_THR, "iou")
    kept = iou[4][0][:iou[3][0]].tolist()
    assert pa in kept and pb not in kept
    k = kept.index(pa)
    assert not np.array_equal(iou[0][0][k], iou[7][0][k])
    diou = MO.merged_nms(b, s, 100, 100, THR, MC.SCORE_THR, "diou", beta)
    kept = diou[4][0][:diou[3][0]].tolist()
    assert pa in kept and pb in kept
    bi, ci, _, _ = MO.candidates(s[0], MC.SCORE_THR)
    _, masks, _ = MO.merge_image(b[0], s[0], diou[4][0], diou[2][0], diou[3][0], THR, MC.SCORE_THR, "diou", beta)
    for box in (pa, pb):
        assert bi[masks[kept.index(box)]].tolist() == [box]
        assert np.array_equal(diou[0][0][kept.index(box)], diou[7][0][kept.index(box)])


# ------------------------------------------------------------------------------------------------ the GPU cases' witnesses
@pytest.mark.parametrize("name,total", MC.CHUNK_CASES)
def test_later_chunk_cases_have_members_behind_the_first_chunk(name, total):
    _, b, s = DC.chunk_case(name)
    ref = MC.chunk_reference(name, total)
    assert ref[6] >= MC.MIN_MARGIN and ref[3][0] == total
    w = MC.chunk_witness(b, s, ref, total)
    k = w["slot"]
    assert (w["member_ranks"] >= DC.NMS_THREADS).sum() > 100
    if total == 55:                                   # NMS stopped in its first chunk: those members were never visited
        assert w["last_kept"] < DC.NMS_THREADS and (w["member_ranks"] > w["last_kept"]).sum() > 1000
    else:
        assert w["last_kept"] >= DC.NMS_THREADS
    # they move the box: with the first 1024 candidates alone the result is another, and both differ from the plain box
    assert np.abs(ref[0][0][k] - w["head_only"]).max() > 1e-4
    assert np.abs(ref[0][0][k] - ref[7][0][k]).max() > 1e-2
    assert ref[0][0][k].min() > 0.0 and ref[0][0][k].max() < 1.0          # the map keeps the mean clear of the clip


@pytest.mark.parametrize("name,per_class,total", MC.CAP_CASES)
def test_cap_cases_absorb_candidates_the_caps_turned_away(name, per_class, total):
    _, ncls, _, b, s = DC.cap_input(name)
    ref = MC.cap_reference(name, per_class, total)
    assert ref[6] >= MC.MIN_MARGIN and ref[3][0] == total
    v = total
    _, masks, _ = MO.merge_image(b[0], s[0], ref[4][0], ref[2][0], v, THR, MC.SCORE_THR)
    bi, ci, _, _ = MO.candidates(s[0], MC.SCORE_THR)
    kept = set(zip(ref[4][0][:v].tolist(), ref[2][0][:v].astype(int).tolist()))
    absorbed = set()
    for m in masks:
        absorbed |= set(zip(bi[m].tolist(), ci[m].tolist()))
    assert kept <= absorbed and len(absorbed - kept) >= 2
    # among the absorbed there is one that NMS alone, uncapped, would have KEPT: only a cap turned it away
    free = DC.cap_reference(name, None, None)
    free_kept = set(zip(free[4][0][:free[3][0]].tolist(), free[2][0][:free[3][0]].astype(int).tolist()))
    assert (absorbed - kept) & free_kept or len(absorbed - kept) >= 2
    assert not np.array_equal(ref[0], ref[7]) and not ref[0][0, v:].any()


@pytest.mark.parametrize("ncls,seed,rule,margin", MC.TILED_CASES)
def test_tiled_cases_margins(ncls, seed, rule, margin):
    refs = MC.tiled_reference(ncls, seed, rule)
    got = min(r[6] for r in refs)
    assert got >= MC.MIN_MARGIN and abs(got - margin) <= 0.01 * margin
    assert all(not np.array_equal(r[0], r[7]) for r in refs)


def test_the_map_applies_after_the_mean_and_before_the_clip():
    _, b, s = RC.random_case(3, 3)
    ref = MO.merged_nms(b, s, 100, 100, THR, MC.SCORE_THR, box_maps=MC.MAPS)
    plain = MC.random_reference(3, 3, "iou")
    assert ref[6] == plain[6]
    # some mapped means leave [0, 1] and are clipped, and the map moved nearly every kept box
    for n in range(2):
        v = int(ref[3][n])
        assert ((ref[0][n, :v] == 0) | (ref[0][n, :v] == 1)).any()
        assert (ref[0][n, :v] != plain[0][n, :v]).any(axis=1).sum() >= v // 2
    # the order shows on the stack of a chunk case: its mean is some 18 canvas sides wide, so a clip BEFORE the map would leave
    # (0, 0, 1, 1) for the map to shrink; the map first brings the mean into view
    _, cb, cs = DC.chunk_case("s1300")
    chunk = MC.chunk_reference("s1300", 55)
    k = MC.chunk_witness(cb, cs, chunk, 55)["slot"]
    canvas = MO.merged_nms(cb, cs, 100, 55, THR, MC.SCORE_THR)
    assert canvas[0][0][k].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert np.abs(MO.map_and_clip(canvas[0][0][k], MC.CHUNK_MAP[0]) - chunk[0][0][k]).max() > 0.1
