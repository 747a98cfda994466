"""y4_coco_match on the GPU against the loop-form oracle (tests/coco_oracle.py) on the crafted cases (tests/coco_cases.py): all
five outputs with array_equal on poisoned buffers at (T, A) = (1, 1), (10, 4) and (16, 4); batch-position independence;
run-to-run identity; the nullable output; the refused arguments.  No model."""
import ctypes as C

import numpy as np
import pytest

import coco_cases

pytestmark = pytest.mark.gpu
POISON = 0x7F7F7F7F


def _run(case_list, thresholds, areas, max_total=coco_cases.MAX_TOTAL, max_gt=coco_cases.MAX_GT, n=None, n_thr=None, n_areas=None,
         with_rows=True):
    """-> (rc, dt_match uint32 [n,A,100], dt_ignore uint32 [n,A,100], cls_rank int32 [n,100], gt_ignore uint32 [n,256],
    match_row int32 [n,A,T,100] or None); the output buffers start poisoned, so every element the kernel must write shows."""
    import torch
    from yolo4hip import ext
    lib = ext.load()
    dev = "cuda:0"
    arrays = coco_cases.batch(case_list)
    boxes, scores, classes, valid, scale, gt, gt_count = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)
    k, T, A = len(case_list), len(thresholds), len(areas)
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device=dev)      # noqa: E731
    dm, di = full(k, A, coco_cases.MAX_TOTAL), full(k, A, coco_cases.MAX_TOTAL)
    rank, gi = full(k, coco_cases.MAX_TOTAL), full(k, coco_cases.MAX_GT)
    rows = full(k, A, T, coco_cases.MAX_TOTAL) if with_rows else None
    thr = (C.c_double * 17)(*thresholds)
    rng = (C.c_double * 10)(*[v for r in areas for v in r])
    rc = lib.y4_coco_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), ext.ptr(valid), k if n is None else n, max_total,
                           ext.ptr(scale), ext.ptr(gt), ext.ptr(gt_count), max_gt, rng, A if n_areas is None else n_areas, thr,
                           T if n_thr is None else n_thr, ext.ptr(dm), ext.ptr(di), ext.ptr(rank), ext.ptr(gi), ext.ptr(rows),
                           ext.stream_ptr())
    torch.cuda.synchronize()
    return (rc, dm.cpu().numpy().view(np.uint32), di.cpu().numpy().view(np.uint32), rank.cpu().numpy(),
            gi.cpu().numpy().view(np.uint32), rows.cpu().numpy() if with_rows else None)


@pytest.fixture(scope="module")
def cases():
    return coco_cases.cases()


@pytest.mark.parametrize("shape", [(1, 1), (10, 4), (16, 4)])
def test_coco_match_equals_oracle(cases, shape):
    thresholds, areas = coco_cases.PARAM_SETS[shape]
    rc, dm, di, rank, gi, rows = _run(cases, thresholds, areas)
    assert rc == 0
    for i, c in enumerate(cases):
        rdm, rdi, rrank, rgi, rrows = coco_cases.oracle(c, thresholds, areas)
        assert np.array_equal(rows[i], rrows), (c["stem"], np.argwhere(rows[i] != rrows)[:5])
        assert np.array_equal(dm[i], rdm), (c["stem"], dm[i][:, :c["valid"]], rdm[:, :c["valid"]])
        assert np.array_equal(di[i], rdi), (c["stem"], di[i][:, :c["valid"]], rdi[:, :c["valid"]])
        assert np.array_equal(rank[i], rrank), (c["stem"], rank[i][:c["valid"]], rrank[:c["valid"]])
        assert np.array_equal(gi[i], rgi), c["stem"]


def test_image_alone_and_as_image_3_of_5(cases):
    thresholds, areas = coco_cases.PARAM_SETS[(10, 4)]
    by = {c["stem"]: c for c in cases}
    around = [by["full"], by["no_gt"], by["ties"], by["scaled"]]
    for c in cases:
        alone = _run([c], thresholds, areas)
        five = _run(around[:3] + [c] + around[3:], thresholds, areas)
        assert alone[0] == 0 and five[0] == 0
        for a, b in zip(alone[1:], five[1:]):
            assert a[0].tobytes() == b[3].tobytes(), c["stem"]


def test_two_runs_give_the_same_bits(cases):
    thresholds, areas = coco_cases.PARAM_SETS[(16, 4)]
    a, b = _run(cases, thresholds, areas), _run(cases, thresholds, areas)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_match_row_may_be_null(cases):
    thresholds, areas = coco_cases.PARAM_SETS[(10, 4)]
    a, b = _run(cases, thresholds, areas, with_rows=False), _run(cases, thresholds, areas)
    assert a[0] == 0 and b[0] == 0 and a[5] is None
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kw, word", [({"max_total": 257}, b"max_total"), ({"max_gt": 257}, b"max_gt"), ({"n_thr": 0}, b"n_thresholds"),
                                      ({"n_thr": 17}, b"n_thresholds"), ({"n_areas": 0}, b"n_areas"), ({"n_areas": 5}, b"n_areas"),
                                      ({"n": -1}, b"negative"), ({"max_total": -1}, b"negative"), ({"max_gt": -1}, b"negative")])
def test_refused_arguments(cases, kw, word):
    from yolo4hip import ext
    out = _run(cases[:2], *coco_cases.PARAM_SETS[(1, 1)], **kw)
    assert out[0] == -22
    assert word in ext.load().y4_last_error()
    assert all((o.view(np.uint32) == POISON).all() for o in out[1:])           # refused before any launch


@pytest.mark.parametrize("null", ["iou_thresholds", "area_ranges", "dt_match", "dt_ignore", "cls_rank", "gt_ignore", "valid", "gt"])
def test_null_pointers_are_refused(cases, null):
    import torch
    from yolo4hip import ext
    lib = ext.load()
    arrays = coco_cases.batch(cases[:2])
    boxes, scores, classes, valid, scale, gt, gt_count = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)
    outs = {k: torch.zeros(2 * 4 * 256, dtype=torch.int32, device="cuda:0") for k in ("dt_match", "dt_ignore", "cls_rank", "gt_ignore")}
    p = {"valid": ext.ptr(valid), "gt": ext.ptr(gt), "iou_thresholds": (C.c_double * 1)(0.5),
         "area_ranges": (C.c_double * 2)(0.0, 1e10), **{k: ext.ptr(v) for k, v in outs.items()}}
    p[null] = None
    rc = lib.y4_coco_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), p["valid"], 2, coco_cases.MAX_TOTAL, ext.ptr(scale),
                           p["gt"], ext.ptr(gt_count), coco_cases.MAX_GT, p["area_ranges"], 1, p["iou_thresholds"], 1,
                           p["dt_match"], p["dt_ignore"], p["cls_rank"], p["gt_ignore"], None, ext.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -22 and b"null" in lib.y4_last_error()
