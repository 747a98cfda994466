"""The COCO rule on the CPU: the loop-form oracle (tests/coco_oracle.py) against the decisions written out by hand in
tests/coco_cases.py, `cocoeval.CocoAccumulator` against the oracle's accumulate / summarize with == over the case set as one
dataset, the sanity values of the rule, and the argument checks.  No GPU."""
import numpy as np
import pytest

import coco_cases
import coco_oracle

THR, AREAS = coco_cases.PARAM_SETS[(10, 4)]


@pytest.fixture(scope="module")
def cases():
    return coco_cases.cases()


@pytest.fixture(scope="module")
def flags(cases):
    """The per-image oracle in the kernel's output form, once for the module."""
    return [coco_cases.oracle(c, THR, AREAS) for c in cases]


def test_parameters_are_cocos():
    from yolo4hip import cocoeval
    assert np.array_equal(cocoeval.IOU_THRESHOLDS, coco_oracle.IOU_THRS) and np.array_equal(cocoeval.IOU_THRESHOLDS, THR)
    assert np.array_equal(cocoeval.REC_THRESHOLDS, coco_oracle.REC_THRS) and len(cocoeval.REC_THRESHOLDS) == 101
    assert np.array_equal(np.array(cocoeval.AREA_RANGES), np.array(coco_oracle.AREA_RNG, dtype=np.float64))
    assert tuple(cocoeval.MAX_DETS) == coco_oracle.MAX_DETS == (1, 10, 100)
    assert THR[0] == 0.5 and THR[5] == 0.75


def test_the_oracle_takes_the_decisions_written_out_by_hand(cases, flags):
    witnesses = 0
    for c, (dm, di, rank, gi, row) in zip(cases, flags):
        for (name, t), want in c.get("expect", {}).items():
            a = coco_cases.AREA_INDEX[name]
            assert len(want) == c["valid"]
            for slot, (m, ignored) in enumerate(want):
                got = (int(row[a, t, slot]), bool((di[a, slot] >> t) & 1))
                assert got == (m, ignored), (c["stem"], name, t, slot, got, (m, ignored))
                assert bool((dm[a, slot] >> t) & 1) == (m >= 0)
                witnesses += 1
        if "expect_rank" in c:
            assert rank[:c["valid"]].tolist() == c["expect_rank"], c["stem"]
        if "expect_gt_ignore" in c:
            assert gi[:c["gt_count"]].tolist() == c["expect_gt_ignore"], c["stem"]
    assert witnesses >= 100
    by = {c["stem"]: f for c, f in zip(cases, flags)}
    assert not by["nothing"][0].any() and (by["nothing"][2] == -1).all() and (by["nothing"][4] == -1).all()
    # the full image: every size bucket has rows, some class has more than 10 detections
    full = by["full"]
    assert all(((full[3] >> a) & 1 == 0).sum() >= 10 for a in range(4)) and full[2].max() > 10 and full[0].any() and full[1].any()


def _accumulate(cases, flags, **kw):
    from yolo4hip.cocoeval import CocoAccumulator
    acc = CocoAccumulator(coco_cases.CLASS_NAMES, **kw)
    for i0 in range(0, len(cases), 4):                                 # batches of 4, as the facade adds them
        part, f = cases[i0:i0 + 4], flags[i0:i0 + 4]
        acc.add(np.stack([c["scores"] for c in part]), np.stack([c["classes"] for c in part]),
                np.array([c["valid"] for c in part], dtype=np.int32), np.stack([x[2] for x in f]), np.stack([x[0] for x in f]),
                np.stack([x[1] for x in f]), [c["gt"][:c["gt_count"], 4] for c in part], np.stack([x[3] for x in f]))
    return acc.result()


def test_accumulator_equals_the_oracle_on_the_case_set(cases, flags):
    from yolo4hip.cocoeval import STAT_NAMES
    got = _accumulate(cases, flags)
    precision, recall, stats = coco_oracle.evaluate(coco_cases.dataset_images(cases), len(coco_cases.CLASS_NAMES))
    assert got["precision"].shape == (10, 101, 5, 4, 3) and got["recall"].shape == (10, 5, 4, 3)
    assert np.array_equal(got["precision"], precision) and np.array_equal(got["recall"], recall)
    assert got["stats"] == stats and [got[k] for k in STAT_NAMES] == stats
    print(dict(zip(STAT_NAMES, stats)))
    # the data bite: every number is defined, maxDets matter, the size buckets differ
    assert all(0.0 < v < 1.0 for v in stats) and stats[6] < stats[7] < stats[8] and len({stats[3], stats[4], stats[5]}) == 3
    for k, name in enumerate(coco_cases.CLASS_NAMES):
        s = precision[:, :, k, 0, 2]
        assert got["per_class"][name] == (float(np.mean(s[s > -1])) if (s > -1).any() else -1.0)
    # "date" has no rows anywhere; "kiwi" is [FP (no_class_gt), TP (kiwi_here)] on one row: the first sanity value
    assert got["per_class"]["date"] == -1.0 and abs(got["per_class"]["kiwi"] - 0.5) <= 1e-12
    n_gt = {}
    for c in cases:
        for v in c["gt"][:c["gt_count"], 4]:
            n_gt[coco_cases.CLASS_NAMES[int(v)]] = n_gt.get(coco_cases.CLASS_NAMES[int(v)], 0) + 1
    assert got["n_gt"] == n_gt and sum(got["n_det"].values()) == sum(c["valid"] for c in cases) - 1      # (the NaN score)


def test_other_parameters_equal_the_oracle_too(cases):
    thr, areas = coco_cases.PARAM_SETS[(16, 4)]
    flags = [coco_cases.oracle(c, thr, areas[:2]) for c in cases]
    got = _accumulate(cases, flags, iou_thresholds=thr, area_ranges=areas[:2], max_dets=(3, 20))
    precision, recall = coco_oracle.tables(coco_cases.dataset_images(cases), 5, np.array(thr), [list(a) for a in areas[:2]],
                                           (3, 20, 10 ** 6))
    assert np.array_equal(got["precision"], precision[..., :2]) and np.array_equal(got["recall"], recall[..., :2])
    # what was not asked for is -1.0: no medium / large range, no third maxDet
    assert got["APm"] == got["APl"] == got["ARm"] == got["ARl"] == got["AR100"] == -1.0
    assert got["AP50"] > 0 and got["APs"] > 0 and got["AR10"] > 0
    only = [coco_cases.oracle(c, (0.6,), areas[:1]) for c in cases]
    res = _accumulate(cases, only, iou_thresholds=(0.6,), area_ranges=areas[:1], max_dets=(100,))
    assert res["AP50"] == res["AP75"] == -1.0 and res["AP"] > 0 and res["AR1"] > 0 and res["AR10"] == -1.0


def _one_class(dets, rows):
    """AP at 0.5 of one image of one class: dets (score, hits row or None), boxes built so that a hit is IoU 1."""
    from yolo4hip.cocoeval import CocoAccumulator
    gt = [(100.0 * g, 0.0, 100.0 * g + 50.0, 50.0, 0) for g in range(rows)]
    d = [((100.0 * r, 0.0, 100.0 * r + 50.0, 50.0) if r is not None else (0.0, 500.0, 50.0, 550.0)) + (s, 0) for s, r in dets]
    case = coco_cases._case("sanity", d, gt)
    f = coco_cases.oracle(case, THR, AREAS)
    acc = CocoAccumulator(["x"])
    acc.add(case["scores"][None], case["classes"][None], np.array([case["valid"]]), f[2][None], f[0][None], f[1][None],
            [case["gt"][:rows, 4]], f[3][None])
    res = acc.result()
    images = coco_cases.dataset_images([case])
    assert np.array_equal(res["precision"], coco_oracle.evaluate(images, 1)[0])
    return float(np.mean(res["precision"][0, :, 0, 0, 2])), res


def test_sanity_values_of_the_rule():
    ap, _ = _one_class([(0.75, None), (0.5, 0)], 1)                    # [FP, TP] on one row
    assert abs(ap - 0.5) <= 1e-12
    ap, res = _one_class([(0.75, 0), (0.5, None)], 1)                  # [TP, FP]
    assert abs(ap - 0.9999999999999999) <= 1e-12 and abs(res["AP50"] - ap) <= 1e-12
    ap, _ = _one_class([(0.75, 0)], 2)                                 # two rows, one TP
    assert abs(ap - 51 / 101) <= 1e-12


def test_a_summary_over_an_empty_range_is_minus_one():
    _, res = _one_class([(0.75, 0)], 1)                                # one 50 x 50 row: medium only
    assert res["APs"] == -1.0 and res["APl"] == -1.0 and res["ARs"] == -1.0 and res["ARl"] == -1.0
    assert res["APm"] > 0.99 and res["AP"] > 0.99 and res["AR1"] > 0.99
    from yolo4hip.cocoeval import CocoAccumulator
    empty = CocoAccumulator(["x"]).result()
    assert empty["stats"] == [-1.0] * 12 and empty["n_gt"] == {} and empty["n_det"] == {}


@pytest.mark.parametrize("kw", [{"iou_thresholds": ()}, {"iou_thresholds": [0.5] * 17}, {"iou_thresholds": [float("nan")]},
                                {"area_ranges": []}, {"area_ranges": [[0, 1]] * 5}, {"area_ranges": [[2, 1]]},
                                {"area_ranges": [0, 1]}, {"max_dets": ()}, {"max_dets": (0, 10)}, {"max_dets": (10, 10)},
                                {"max_dets": (1.5, 10)}])
def test_bad_parameters_raise(kw):
    from yolo4hip.cocoeval import CocoAccumulator
    with pytest.raises(ValueError):
        CocoAccumulator(["x"], **kw)
