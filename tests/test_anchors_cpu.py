"""The data-set anchor rule on the host: hand-written witnesses of the NumPy oracle (tests/anchors_oracle.py), the oracle's best
anchor against `data._assign`, `dataset_wh` against the label path on a written data set, the host part of `rebase_anchors`, and
`AnchorFit.config()` through `_cfg_struct`.  No GPU."""
import os

import numpy as np
import pytest

import anchors_oracle as AO
from helpers import CLASS_DIR

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


# ---------------------------------------------------------------- witnesses of the rule
def test_k1_next_anchor_is_the_fixed_point_mean():
    wh = np.array([[10, 20], [30, 40], [20.5, 3.25]], dtype=F32)
    nxt, stats, assign = AO.step(wh, [[5, 5]])
    sw, sh = int(60.5 * 65536), int(63.25 * 65536)
    assert stats.tolist()[1:] == [3, sw, sh] and assign.tolist() == [0, 0, 0]
    assert _bits(nxt) == _bits([[F32(sw / 3 / 65536.0), F32(sh / 3 / 65536.0)]])
    # the sides are summed in 16.16 fixed point: a fraction below 2^-17 is rounded away before the mean
    w = F32(1 + 2.0 ** -20)
    nxt, stats, _ = AO.step(np.array([[w, 2]], dtype=F32), [[1, 1]])
    assert stats[2] == 65536 and nxt[0, 0] == F32(1.0) and nxt[0, 0] != w
    # F: one box inside its anchor, IoU = 200 / 400 = 0.5 exactly
    assert AO.fitness(np.array([[10, 20]], dtype=F32), [[20, 20]]) == 2 ** 29


def test_equal_iou_goes_to_the_first_anchor():
    box = np.array([[10, 10]], dtype=F32)
    for anchors in ([[20, 5], [5, 20]], [[5, 20], [20, 5]]):
        ious = [AO.iou64(box, a)[0] for a in anchors]
        assert ious[0] == ious[1] == 50.0 / 150.0
        idx, best = AO.best_anchor(box, anchors)
        assert idx.tolist() == [0] and best[0] == ious[0]
    idx, _ = AO.best_anchor(box, [[3, 3], [20, 5], [5, 20]])        # ... and to the first of the two best, not to index 0
    assert idx.tolist() == [1]


def test_empty_cluster_keeps_its_anchor():
    wh = np.array([[9, 11], [10, 10], [12, 9]], dtype=F32)
    nxt, stats, assign = AO.step(wh, [[10, 10], [1000, 1000]])
    assert assign.tolist() == [0, 0, 0] and stats[1:3].tolist() == [3, 0] and stats[4] == 0 and stats[6] == 0
    assert _bits(nxt[1]) == _bits([1000, 1000])
    assert _bits(nxt[0]) == _bits([F32(31 / 3), F32(10)])


def test_one_box_and_fewer_boxes_than_anchors():
    one = np.array([[33.5, 17.25]], dtype=F32)
    a0 = AO.start(one, 9)
    assert _bits(a0) == _bits(np.repeat(one, 9, axis=0))
    res = AO.fit(one, None)
    assert res["converged"] and res["iterations"] == 1 and res["fitness"] == 2 ** 30 and res["avg_iou"] == 1.0
    assert res["counts"].tolist() == [1] + [0] * 8 and res["assign"].tolist() == [0]
    two = np.array([[100, 50], [10, 20]], dtype=F32)
    a0 = AO.start(two, 9)                                           # ranks ((2j + 1) * 2) // 18 = 0 0 0 0 1 1 1 1 1
    assert _bits(a0) == _bits([[10, 20]] * 4 + [[100, 50]] * 5)
    res = AO.fit(two, None)
    assert res["converged"] and res["avg_iou"] == 1.0 and res["counts"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0]
    assert res["assign"].tolist() == [4, 0]


def test_start_orders_by_area_then_w_then_h():
    wh = np.array([[4, 4], [2, 8], [8, 2], [1, 1], [2, 8.5]], dtype=F32)      # areas 16 16 16 1 17
    assert AO.by_size(wh).tolist() == [3, 1, 0, 2, 4]
    assert _bits(AO.start(wh, 2)) == _bits([wh[1], wh[2]])         # ranks (1 * 5) // 4 = 1 and (3 * 5) // 4 = 3


def test_candidate_is_clamped_to_one_pixel():
    wh = np.array([[1.5, 30], [1, 20]], dtype=F32)
    best = np.array([[1.2, 50]], dtype=F32)
    mult = np.array([0.5, 0.5], dtype=F32).reshape(1, 1, 1, 2)
    f0 = AO.fitness(wh, best)
    nb, fb, hist, acc = AO.evolve(wh, best, f0, mult)
    assert hist[0, 0] == AO.fitness(wh, [[1.0, 25.0]]) and hist[0, 0] > f0           # 0.6 -> 1.0, not 0.6
    assert hist[0, 0] != AO.fitness(wh, [[0.6, 25.0]])
    assert acc.tolist() == [0] and fb == hist[0, 0] and _bits(nb) == _bits([[1.0, 25.0]])


def test_a_tie_with_the_best_is_not_accepted():
    wh = AO.mixture(50, 3)
    best = AO.start(wh, 9)
    f0 = AO.fitness(wh, best)
    mult = np.ones((2, 3, 9, 2), dtype=F32)
    mult[1, 2] = 3.0                                                # generation 1: two ties and a worse set
    nb, fb, hist, acc = AO.evolve(wh, best, f0, mult)
    assert hist[0].tolist() == [f0] * 3 and hist[1, :2].tolist() == [f0] * 2 and hist[1, 2] < f0
    assert acc.tolist() == [-1, -1] and fb == f0 and _bits(nb) == _bits(best)
    # among equal winners the first index is taken
    worse = (best * F32(3.0)).astype(F32)
    mult = np.full((1, 3, 9, 2), 1 / 3, dtype=F32)
    mult[0, 0] = 1.0
    cand = np.maximum(worse * mult[0, 1], F32(1.0))
    _nb, fb, hist, acc = AO.evolve(wh, worse, AO.fitness(wh, worse), mult)
    assert hist[0, 1] == hist[0, 2] == AO.fitness(wh, cand) > hist[0, 0] and acc.tolist() == [1] and fb == hist[0, 1]


def test_draw_mult_is_the_stated_draw():
    from yolo4hip.anchors import draw_mult
    rng = np.random.default_rng(7)
    mask = rng.random((3, 5, 9, 2)) < 0.9
    ref = np.clip(1 + mask * rng.standard_normal((3, 5, 9, 2)) * 0.1, 0.3, 3.0).astype(F32)
    got = draw_mult(7, 3, 5)
    assert got.dtype == F32 and got.tobytes() == ref.tobytes()
    assert 0.05 < float((got == 1).mean()) < 0.15


def test_host_start_and_order_equal_the_oracle():
    from yolo4hip import anchors as A
    for n in (1, 5, 9, 100, 1025):
        wh = AO.mixture(n, n)
        assert _bits(A.start_anchors(wh)) == _bits(AO.start(wh, 9))
        assert A.by_size(wh).tolist() == AO.by_size(wh).tolist()


# ---------------------------------------------------------------- the label path
def test_oracle_best_anchor_is_the_label_assignment():
    from yolo4hip.config import yolo_config
    from yolo4hip.data import _assign
    rng = np.random.default_rng(11)
    wh = AO.mixture(600, 5, size=300.0)
    fitted = AO.fit(wh, None)["anchors"]
    for anchors in (np.array(yolo_config["anchors"]).reshape(9, 2), np.array([float(v) for v in fitted.reshape(-1)]).reshape(9, 2)):
        boxes = np.zeros((6, 100, 5), dtype=F32)
        cx = rng.uniform(160, 256, size=(6, 100)).astype(F32)
        cy = rng.uniform(160, 256, size=(6, 100)).astype(F32)
        w, h = wh[:, 0].reshape(6, 100), wh[:, 1].reshape(6, 100)
        boxes[..., 0], boxes[..., 1], boxes[..., 2], boxes[..., 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
        _xy, awh, _grids, hits = _assign(boxes, (416, 416), anchors, 3)
        got = np.array([[s * 3 + a for s, _r, _c, a, _k, _cls in rows] for rows in hits])
        idx, _best = AO.best_anchor(awh.reshape(-1, 2), anchors)
        assert got.shape == (6, 100) and np.array_equal(got.reshape(-1), idx)
        assert len(set(idx.tolist())) >= 6


def _write_dataset(tmp_path):
    from PIL import Image
    sizes = {"a.png": (37, 53), "b.jpg": (640, 480), "c.png": (200, 601)}              # (w, h)
    for name, (w, h) in sizes.items():
        Image.fromarray(np.full((h, w, 3), 90, dtype=np.uint8)).save(str(tmp_path / name))
    lines = ["a.png 3,4,30,41,0 10.5,2.25,20.75,50,1\n",
             "b.jpg 0,0,640,480,2 100,50,333,77,0 5,5,7.5,470,1 600,400,639,479,2\n",
             "c.png 20,30,180,590,1 7,7,11,13,0\n"]
    return sizes, lines


@pytest.mark.parametrize("size", [(416, 416, 3), (352, 608, 3)])
def test_dataset_wh_stretch_equals_the_label_path(tmp_path, monkeypatch, size):
    from yolo4hip.anchors import dataset_wh
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator, _assign
    _sizes, lines = _write_dataset(tmp_path)
    monkeypatch.setattr(np.random, "shuffle", lambda x: None)      # get_data shuffles an image's boxes; dataset_wh keeps the order
    cfg = make_config(size[:2])
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), max_boxes=8, shuffle=False, config=cfg)
    ref = []
    for line in lines:
        _img, boxes = gen.get_data(line)
        _xy, wh, _g, _hits = _assign(boxes[None], size[:2], gen.anchors, 3)
        ref.append(wh[0][wh[0, :, 0] > 0])
    ref = np.concatenate(ref)
    got = dataset_wh(lines, str(tmp_path), size)
    assert got.dtype == F32 and got.shape == (8, 2) and got.tobytes() == ref.tobytes()
    assert dataset_wh(lines, str(tmp_path), size[:2]).tobytes() == got.tobytes()


def test_dataset_wh_letterbox_equals_the_canvas_label_path(tmp_path):
    from yolo4hip import prepost
    from yolo4hip.anchors import dataset_wh
    from yolo4hip.augment import transform_boxes
    from yolo4hip.data import _assign
    sizes, lines = _write_dataset(tmp_path)
    H, W = 352, 608
    ref = []
    for line in lines:
        fields = line.split()
        iw, ih = sizes[fields[0]]
        raw = np.array([[float(v) for v in f.split(',')] for f in fields[1:]], dtype=F32)
        out_h, out_w, top, left = prepost.letterbox_rect(ih, iw, H, W)
        param = {"out_h": out_h, "out_w": out_w, "pad_top": top, "pad_left": left, "flip": 0}
        boxes = transform_boxes(raw, (ih, iw), param, (H, W), 8)
        _xy, wh, _g, _hits = _assign(boxes[None], (H, W), np.arange(1, 19).reshape(9, 2), 3)
        ref.append(wh[0][wh[0, :, 0] > 0])
    ref = np.concatenate(ref)
    got = dataset_wh(lines, str(tmp_path), (H, W, 3), letterbox=True)
    assert got.shape == (8, 2) and got.tobytes() == ref.tobytes()
    assert got.tobytes() != dataset_wh(lines, str(tmp_path), (H, W, 3)).tobytes()


def test_dataset_wh_keeps_every_box_and_refuses_bad_sides(tmp_path):
    from PIL import Image
    from yolo4hip.anchors import dataset_wh
    Image.fromarray(np.zeros((10, 10, 3), dtype=np.uint8)).save(str(tmp_path / "s.png"))
    many = " ".join(f"{i % 5},{i % 3},{i % 5 + 2},{i % 3 + 4},0" for i in range(300))
    lines = ["s.png " + many + "\n", "\n", "s.png\n", "s.png 5,5,5,9,0 1,8,3,8,0 6,6,4,9,0 1,1,2,3,0\n"]
    got = dataset_wh(lines, str(tmp_path), 320)
    assert got.shape == (301, 2)                                   # no cut to max_boxes; w <= 0 and h <= 0 rows dropped
    assert _bits(got[-1]) == _bits([F32(2) * F32(32.0) - F32(1) * F32(32.0), F32(96) - F32(32)])
    with pytest.raises(ValueError, match="16384"):
        dataset_wh(["s.png 0,0,600,5,0\n"], str(tmp_path), 320)
    with pytest.raises(ValueError, match="finite"):
        dataset_wh(["s.png 0,0,inf,5,0\n"], str(tmp_path), 320)
    assert dataset_wh([], str(tmp_path), 320).shape == (0, 2)


# ---------------------------------------------------------------- rebase_anchors (host part) and config()
def test_rebase_moves_exactly_the_eighteen_wh_biases():
    from yolo4hip import weights as W
    from yolo4hip.anchors import anchor_log_shift, rebase_flat
    from yolo4hip.config import yolo_config
    from yolo4hip.plan import build_plan
    ncls = 3
    plan = build_plan((64, 64), ncls)
    flat = W.flatten(W.synth_weights(plan, 2))
    old = np.array(yolo_config["anchors"], dtype=np.float64).reshape(9, 2)
    new = AO.fit(AO.mixture(400, 9), None)["anchors"]
    keep = flat.copy()
    out = rebase_flat(flat, plan, ncls, old, new)
    assert flat.tobytes() == keep.tobytes() and out.dtype == F32 and out.shape == flat.shape
    moved = np.nonzero(out.view(np.uint32) != flat.view(np.uint32))[0]
    assert len(moved) == 18
    shift = anchor_log_shift(old, new)
    assert shift.dtype == F32 and np.array_equal(shift, np.log(old / new.astype(np.float64)).astype(F32))
    a, b = W.unflatten(plan, flat), W.unflatten(plan, out)
    nf = 5 + ncls
    for s, idx in enumerate((93, 101, 109)):
        assert a[idx].w.tobytes() == b[idx].w.tobytes()
        for an in range(3):
            for c in (0, 1):
                ch = an * nf + 2 + c
                assert b[idx].bias[ch] == F32(a[idx].bias[ch] + shift[3 * s + an, c]) != a[idx].bias[ch]
        rest = np.ones(3 * nf, dtype=bool)
        rest[[an * nf + 2 + c for an in range(3) for c in (0, 1)]] = False
        assert a[idx].bias[rest].tobytes() == b[idx].bias[rest].tobytes()
    # exp(t') * new == exp(t) * old up to rounding
    t = a[93].bias[2].astype(np.float64)
    assert abs(np.exp(np.float64(b[93].bias[2])) * np.float64(new[0, 0]) / (np.exp(t) * old[0, 0]) - 1) < 1e-6
    assert rebase_flat(flat, plan, ncls, new, new).tobytes() == flat.tobytes()
    with pytest.raises(ValueError):
        rebase_flat(flat, plan, ncls, old[:8], new)


def test_config_round_trips_through_the_config_struct():
    from yolo4hip.anchors import AnchorFit
    from yolo4hip.config import make_config, yolo_config
    from yolo4hip.engine import _cfg_struct
    anchors = AO.fit(AO.mixture(300, 4), None)["anchors"]
    fit = AnchorFit(None, anchors=anchors)
    base = make_config(160, max_boxes=25)
    cfg = fit.config(base)
    assert cfg is not base and base["anchors"] == yolo_config["anchors"] and cfg["max_boxes"] == 25 and cfg["img_size"] == (160, 160, 3)
    assert len(cfg["anchors"]) == 18 and all(type(v) is float for v in cfg["anchors"])
    c = _cfg_struct(cfg, 3, 1, "f32")
    assert np.array([c.anchors[i] for i in range(18)], dtype=F32).tobytes() == anchors.tobytes()
    assert np.array(cfg["anchors"]).reshape(9, 2).astype(F32).tobytes() == anchors.tobytes()      # what DataGenerator keeps
    assert fit.config()["img_size"] == yolo_config["img_size"]
