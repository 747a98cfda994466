"""The NMS pair rule's test oracle (tests/nms_rule_oracle.py) without a GPU: with the default rule it IS
oracle.decode_nms.combined_nms, its DIoU measure has the hand values of a worked example, and the agnostic pass and the class cap
behave as include/yolo4hip.h (y4_set_nms_rule) says."""
import os

import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_cases as RC
import nms_rule_oracle as NR
from oracle import decode_nms as OD

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F32 = np.float32


def _same5(got, ref):
    for a, b in zip(got[:5], ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_default_rule_is_combined_nms_on_golden(case):
    g = np.load(os.path.join(GOLDEN, "nms_cases.npz"))
    b, s = g[case + "_boxes"], g[case + "_scores"]
    ref = OD.combined_nms(b, s)
    _same5(NR.combined_nms_rule(b, s, kind="iou", agnostic=False), ref)
    for a, k in zip(ref, ("ob", "os", "oc", "ov", "oi")):       # (and both equal what the fixture recorded)
        assert np.array_equal(a, g[f"{case}_{k}"])


@pytest.mark.parametrize("name,caps", [("small6", (100, 100)), ("small6", (3, 10)), ("small6", (1, 100)),
                                       ("s2500", (100, 100)), ("s2500", (2, 1024))])
def test_default_rule_is_combined_nms_on_cap_inputs(name, caps):
    from yolo4hip.config import make_config
    size, ncls, _, b, s = DC.cap_input(name)
    cfg = make_config(size)
    ref = DC.cap_reference(name, *caps)
    got = NR.combined_nms_rule(b, s, caps[0], caps[1], cfg["iou_threshold"], cfg["score_threshold"], "iou", 1.0, False)
    _same5(got, ref)


# ---- the worked example: two 20 x 20 boxes whose centres are 8 apart (pixels of a 160 canvas, normalised)
def _pair(gap=8.0, side=20.0, canvas=160.0, axis=0):
    a = np.array([40.0, 40.0, 40.0 + side, 40.0 + side], np.float64)
    b = a.copy()
    b[[axis, axis + 2]] += gap
    return (a / canvas).astype(F32), (b / canvas).astype(F32)


def test_hand_values():
    a, b = _pair()
    iou = NR.measure(a, b[None], "iou")[0]
    assert abs(float(iou) - 12.0 / 28.0) < 1e-6
    m1 = NR.measure(a, b[None], "diou", 1.0)[0]
    m06 = NR.measure(a, b[None], "diou", 0.6)[0]
    assert abs(float(m1) - (12.0 / 28.0 - 64.0 / 1184.0)) < 1e-6 and abs(float(m1) - 0.37452) < 1e-5
    assert abs(float(m06) - (12.0 / 28.0 - (64.0 / 1184.0) ** 0.6)) < 1e-6 and abs(float(m06) - 0.2550) < 1e-4
    assert m1.dtype == F32 and m06.dtype == F32
    # float64 evaluation of the same formulas agrees to float32 rounding
    assert abs(float(NR.measure(a, b[None], "diou", 0.6, np.float64)[0]) - float(m06)) < 1e-6
    # the other axis gives the same values
    a2, b2 = _pair(axis=1)
    assert NR.measure(a2, b2[None], "diou", 0.6)[0] == m06


@pytest.mark.parametrize("kind,beta,kept", [("iou", 1.0, 1), ("diou", 1.0, 2), ("diou", 0.6, 2)])
def test_hand_pair_through_nms(kind, beta, kept):
    a, b = _pair()
    boxes = np.stack([a, b])[None]
    scores = np.array([[[0.9], [0.8]]], F32)
    out = NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, kind, beta, False)
    assert out[3][0] == kept and list(out[4][0][:kept]) == [0, 1][:kept]
    m = {"iou": 12.0 / 28.0, "diou": 12.0 / 28.0 - (64.0 / 1184.0) ** beta}[kind]
    assert abs(out[5] - abs(m - float(F32(0.413)))) < 1e-6          # min_margin is this one pair's


def test_measure_properties():
    rng = np.random.default_rng(5)
    lo = rng.uniform(0.0, 0.8, (400, 2))
    wh = rng.uniform(0.0, 0.4, (400, 2))
    bx = np.concatenate([lo, lo + wh], axis=1).astype(F32)
    bx[::7] = bx[::7][:, [2, 3, 0, 1]]                    # some with swapped corners: the measure normalises them
    for beta in (1.0, 0.6, 2.0):
        for i in range(0, 400, 40):
            iou = NR.measure(bx[i], bx, "iou")
            m = NR.measure(bx[i], bx, "diou", beta)
            assert np.all(m <= iou)
            assert m[i] == iou[i]                          # a box against itself: equal centres
    # equal centres, different sizes: m == iou exactly
    a = np.array([0.2, 0.2, 0.6, 0.6], F32)
    b = np.array([0.3, 0.1, 0.5, 0.7], F32)
    assert NR.measure(a, b[None], "diou", 0.6)[0] == NR.measure(a, b[None], "iou")[0] > 0
    # a degenerate pair, both boxes the same point: c2 == 0 -> iou (which is 0: no area), not NaN
    p = np.array([0.5, 0.5, 0.5, 0.5], F32)
    assert NR.measure(p, p[None], "diou", 0.6)[0] == 0.0
    # swapping the two boxes changes nothing
    assert NR.measure(a, bx, "diou", 0.6)[3] == NR.measure(bx[3], a[None], "diou", 0.6)[0]


def test_agnostic_one_box_three_classes_keeps_its_best():
    a, _ = _pair()
    far = np.array([0.7, 0.7, 0.8, 0.8], F32)
    boxes = np.stack([a, far])[None]
    scores = np.array([[[0.5, 0.9, 0.7, 0.1], [0.2, 0.1, 0.6, 0.1]]], F32)
    aware = NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, "iou", 1.0, False)
    assert aware[3][0] == 4 and list(aware[2][0][:4]) == [1.0, 2.0, 2.0, 0.0]
    for kind in NR.KINDS:
        ag = NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, kind, 0.6, True)
        assert ag[3][0] == 2
        assert list(ag[4][0][:2]) == [0, 1] and list(ag[2][0][:2]) == [1.0, 2.0]
        assert np.all(ag[1][0][2:] == 0) and np.all(ag[4][0][2:] == -1)


def test_agnostic_two_boxes_of_different_classes_keep_one():
    a, b = _pair()
    boxes = np.stack([a, b])[None]
    scores = np.array([[[0.9, 0.0], [0.0, 0.8]]], F32)
    assert NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, "iou", 1.0, False)[3][0] == 2
    ag = NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, "iou", 1.0, True)
    assert ag[3][0] == 1 and ag[4][0][0] == 0 and ag[2][0][0] == 0.0
    # DIoU leaves this pair alone also across classes
    assert NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, "diou", 0.6, True)[3][0] == 2


def test_capped_class_suppresses_nothing():
    """Class 0 has two disjoint candidates and per_class = 1: the second is turned away.  A class-1 box that overlaps the
    turned-away one (and nothing else) comes later: it is kept, because a candidate that was not kept suppresses nothing."""
    a, b = _pair()
    first = np.array([0.7, 0.7, 0.8, 0.8], F32)
    boxes = np.stack([first, a, b])[None]
    scores = np.array([[[0.9, 0.0], [0.8, 0.0], [0.0, 0.7]]], F32)
    out = NR.combined_nms_rule(boxes, scores, 1, 100, 0.413, 0.3, "iou", 1.0, True)
    assert out[3][0] == 2 and list(out[4][0][:2]) == [0, 2] and list(out[2][0][:2]) == [0.0, 1.0]
    # without the cap the middle box is kept and, agnostic, suppresses the third
    out = NR.combined_nms_rule(boxes, scores, 100, 100, 0.413, 0.3, "iou", 1.0, True)
    assert out[3][0] == 2 and list(out[4][0][:2]) == [0, 1]


def test_min_margin_takes_the_float64_value_too():
    a, b = _pair()
    boxes = np.stack([a, b])[None]
    scores = np.array([[[0.9], [0.8]]], F32)
    m32 = float(NR.measure(a, b[None], "diou", 0.6)[0])
    m64 = float(NR.measure(a, b[None], "diou", 0.6, np.float64)[0])
    thr = float(F32(0.25))
    out = NR.combined_nms_rule(boxes, scores, 100, 100, 0.25, 0.3, "diou", 0.6, False)
    assert out[5] == min(abs(m32 - thr), abs(m64 - thr))


# ---- the witnesses of tests/nms_rule_cases.py, which the GPU tests rely on
@pytest.mark.parametrize("other_class", [False, True])
@pytest.mark.parametrize("place", RC.PLACES)
def test_witness_places_hold(place, other_class):
    assert RC.place_holds(place, other_class)
    _, _, _, _, _, pairs = RC.witness_case(place, other_class)
    assert len(pairs) == (2 if place == "later_same" else 1)

    def outcome(kind, beta, agnostic):
        kept = RC.kept_boxes(RC.witness_reference(place, other_class, kind, beta, agnostic))
        return [(a in kept, b in kept) for a, b in pairs]
    one, both = [(True, False)] * len(pairs), [(True, True)] * len(pairs)
    assert outcome("iou", 1.0, False) == (both if other_class else one)
    assert outcome("iou", 1.0, True) == one
    for beta in (1.0, 0.6):
        assert outcome("diou", beta, False) == both and outcome("diou", beta, True) == both
    if place.startswith("later"):              # fewer than max_total boxes are kept in front of the pair
        assert RC.witness_reference(place, other_class, "diou", 0.6, False)[3][0] < 100


@pytest.mark.parametrize("ncls,seed,rule,margin", RC.RANDOM_CASES)
def test_random_case_margins(ncls, seed, rule, margin):
    ref = RC.random_reference(ncls, seed, rule)
    assert ref[5] >= 1e-5 and abs(ref[5] - margin) <= 0.01 * margin
    assert ref[3].tolist() == [100, 100]
