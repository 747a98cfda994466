"""y4_map_match on the GPU against the per-image oracle (tests/map_oracle.py) on the crafted cases (tests/map_cases.py): all
four outputs, `best_iou` with ==; batch-position independence; run-to-run identity; the refused arguments.  No model."""
import ctypes as C

import numpy as np
import pytest

import map_cases

pytestmark = pytest.mark.gpu


def _run(case_list, thresholds, max_total=map_cases.MAX_TOTAL, max_gt=map_cases.MAX_GT, n=None, n_thr=None):
    """-> (rc, tp_mask uint32 [n,100], best_iou float64 [n,100], match int32 [n,100], gt_used uint32 [n,256]); the output
    buffers start poisoned, so every element the kernel must write shows."""
    import torch
    from yolo4hip import ext
    lib = ext.load()
    dev = "cuda:0"
    arrays = map_cases.batch(case_list)
    boxes, scores, classes, valid, scale, gt, gt_count = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)
    k = len(case_list)
    tp = torch.full((k, map_cases.MAX_TOTAL), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    best = torch.full((k, map_cases.MAX_TOTAL), 123.0, dtype=torch.float64, device=dev)
    match = torch.full((k, map_cases.MAX_TOTAL), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    used = torch.full((k, map_cases.MAX_GT), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    thr = (C.c_double * 17)(*thresholds)
    rc = lib.y4_map_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), ext.ptr(valid), k if n is None else n, max_total,
                          ext.ptr(scale), ext.ptr(gt), ext.ptr(gt_count), max_gt, thr, len(thresholds) if n_thr is None else n_thr,
                          ext.ptr(tp), ext.ptr(best), ext.ptr(match), ext.ptr(used), ext.stream_ptr())
    torch.cuda.synchronize()
    return (rc, tp.cpu().numpy().view(np.uint32), best.cpu().numpy(), match.cpu().numpy(), used.cpu().numpy().view(np.uint32))


@pytest.fixture(scope="module")
def cases():
    return map_cases.cases()


@pytest.mark.parametrize("n_thr", [1, 10, 16])
def test_map_match_equals_oracle(cases, n_thr):
    thresholds = map_cases.THRESHOLD_SETS[n_thr]
    rc, tp, best, match, used = _run(cases, thresholds)
    assert rc == 0
    for i, c in enumerate(cases):
        rtp, rbest, rmatch, rused = map_cases.oracle(c, thresholds)
        assert np.array_equal(match[i], rmatch), (c["stem"], match[i][:c["valid"]], rmatch[:c["valid"]])
        assert np.all(best[i] == rbest), (c["stem"], np.abs(best[i] - rbest).max())
        assert np.array_equal(tp[i], rtp), (c["stem"], tp[i][:c["valid"]], rtp[:c["valid"]])
        assert np.array_equal(used[i], rused), c["stem"]


def test_image_alone_and_as_image_3_of_5(cases):
    thresholds = map_cases.THRESHOLD_SETS[10]
    by = {c["stem"]: c for c in cases}
    around = [by["full"], by["no_gt"], by["a-b"], by["scaled"]]
    for c in cases:
        alone = _run([c], thresholds)
        five = _run(around[:3] + [c] + around[3:], thresholds)
        assert alone[0] == 0 and five[0] == 0
        for a, b in zip(alone[1:], five[1:]):
            assert a[0].tobytes() == b[3].tobytes(), c["stem"]


def test_two_runs_give_the_same_bits(cases):
    thresholds = map_cases.THRESHOLD_SETS[16]
    a, b = _run(cases, thresholds), _run(cases, thresholds)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_optional_outputs_may_be_null(cases):
    import torch
    from yolo4hip import ext
    lib = ext.load()
    thresholds = map_cases.THRESHOLD_SETS[10]
    arrays = map_cases.batch(cases)
    boxes, scores, classes, valid, scale, gt, gt_count = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)
    tp = torch.full((len(cases), map_cases.MAX_TOTAL), -1, dtype=torch.int32, device="cuda:0")
    thr = (C.c_double * len(thresholds))(*thresholds)
    ext.check(lib.y4_map_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), ext.ptr(valid), len(cases), map_cases.MAX_TOTAL,
                               ext.ptr(scale), ext.ptr(gt), ext.ptr(gt_count), map_cases.MAX_GT, thr, len(thresholds), ext.ptr(tp),
                               None, None, None, ext.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(tp.cpu().numpy().view(np.uint32), _run(cases, thresholds)[1])


@pytest.mark.parametrize("kw, word", [({"max_total": 257}, b"max_total"), ({"max_gt": 257}, b"max_gt"), ({"n_thr": 0}, b"n_thresholds"),
                                      ({"n_thr": 17}, b"n_thresholds"), ({"n": -1}, b"negative"), ({"max_total": -1}, b"negative"),
                                      ({"max_gt": -1}, b"negative")])
def test_refused_arguments(cases, kw, word):
    from yolo4hip import ext
    rc = _run(cases[:2], map_cases.THRESHOLD_SETS[1], **kw)[0]
    assert rc == -22
    assert word in ext.load().y4_last_error()
