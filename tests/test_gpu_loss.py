"""The validation loss on the device (y4_loss_assign, y4_loss; csrc/loss.hip) against the reference-generated fixtures, the
float64 restatement (tests/loss_oracle.py) and itself (records, determinism, the two fronts, evaluate).

Budget of every comparison with the float64 restatement: 4 x d_ref with a floor of 1e-6, relative, where d_ref (stored in
the fixture, per scale and term) is the distance of the reference's OWN float32 result from the same restatement -- the device
and the reference run one formula in float32 and differ from float64 by the exp / log implementation and the summation tree
only.  The measured distances are written to profiles/loss/parity_measured.json."""
import json
import os

import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
from helpers import CLASS_DIR, ROOT
from test_loss_cpu import CASE_NAMES, _write_dataset, load_fixture

pytestmark = pytest.mark.gpu
FLOOR = 1e-6


def _engine(hw, ncls, n, dtype="f32"):
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    from yolo4hip import weights as W
    cfg = make_config(hw if hw[0] != hw[1] else hw[0])
    eng = Engine(ncls, cfg, max_batch=n, dtype=dtype, device="cuda:0")
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(hw, ncls), seed=2)))
    return eng


def _note(key, value):
    path = os.path.join(ROOT, "profiles", "loss", "parity_measured.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc[key] = value
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


def _within_budget(key, got, oracle, d_ref):
    dist = LO.rel_dist(got, oracle)
    budget = np.maximum(4.0 * np.asarray(d_ref, dtype=np.float64), FLOOR)
    _note(key, {"max_rel_dist": dist.max(axis=0).tolist(), "budget": np.broadcast_to(budget, dist.shape[1:]).tolist()})
    print(key, "max rel dist per (scale, term):", dist.max(axis=0).tolist(), "budget:", budget.tolist())
    assert np.all(dist <= budget), (key, dist.max(axis=0), budget)


def _device_records(eng, boxes):
    import torch
    rec, cnt, xywh = eng.assign_device(torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(eng.device))
    return rec.cpu().numpy(), cnt.cpu().numpy(), xywh.cpu().numpy()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_loss_of_fixture_heads_vs_reference(name):
    case, fx, labels = load_fixture(name)
    from yolo4hip.data import records_from_dense
    from yolo4hip.engine import combine_loss
    eng = _engine(case["hw"], case["ncls"], case["n"])
    n = eng.set_heads(case["heads"])
    triple = eng.upload_records(records_from_dense(labels, case["ncls"]), fx["true_xywh"])
    got = eng.loss_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert got.shape == (n, 3, 3) and got.dtype == np.float32
    oracle = LO.loss_terms(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH,
                           case["hw"])
    _within_budget(f"fixture_{name}", got, oracle, fx["d_ref"])
    # ... and so near the reference's own float32 numbers: both lie within their budgets of the float64 values
    assert np.all(LO.rel_dist(got, fx["ref_img"]) <= 5.0 * np.maximum(fx["d_ref"], FLOOR))
    total = combine_loss(got)[0].mean()
    assert abs(total - float(fx["ref_total"])) <= 5e-6 * float(fx["ref_total"])
    # labels assigned on the device give the same bits
    import torch
    got_b = eng.loss_device(n, boxes_dev=torch.from_numpy(case["boxes"]).to(eng.device),
                            iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert np.array_equal(got.view(np.int32), got_b.view(np.int32))
    eng.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_assign_gives_the_host_records_exactly(name):
    from yolo4hip.data import pad_records, records_from_boxes
    case, fx, labels = load_fixture(name)
    eng = _engine(case["hw"], case["ncls"], case["n"])
    rec, cnt, xywh = _device_records(eng, case["boxes"])
    host, _ = records_from_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
    want, want_cnt = pad_records(host, LC.MAX_BOXES, case["ncls"])
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(rec, want)                                         # integers and float bits, zero padding included
    assert np.array_equal(xywh.view(np.int32), fx["true_xywh"].view(np.int32))
    # an off-grid centre / an unknown class is flagged (count -1), not written anywhere
    bad = case["boxes"][1:3].copy()
    bad[0, 0] = [400, 10, 460, 50, 0] if case["hw"][1] == 416 else [150, 10, 180, 50, 0]
    bad[1, 0, 4] = case["ncls"]
    _, cnt_bad, _ = _device_records(eng, bad)
    assert cnt_bad.tolist() == [-1, -1]
    with pytest.raises(ValueError, match="outside"):
        eng.loss(np.zeros((1,) + tuple(case["hw"]) + (3,), np.float32), boxes=bad[0:1])
    with pytest.raises(ValueError, match="class id"):
        eng.loss(np.zeros((1,) + tuple(case["hw"]) + (3,), np.float32), boxes=bad[1:2])
    with pytest.raises(ValueError, match="max_boxes"):
        eng.loss(np.zeros((1,) + tuple(case["hw"]) + (3,), np.float32), boxes=bad[0:1, :50])
    eng.close()


def test_loss_is_deterministic_and_independent_of_batch_and_position():
    import torch
    case, fx, labels = load_fixture("160_coco")
    eng = _engine(case["hw"], case["ncls"], 4)
    boxes = torch.from_numpy(case["boxes"]).to(eng.device)

    def run(order):
        eng.set_heads([h[order] for h in case["heads"]])
        return eng.loss_device(len(order), boxes_dev=boxes[order].contiguous()).cpu().numpy().view(np.int32)
    full = run([0, 1, 2, 3])
    assert np.array_equal(full, run([0, 1, 2, 3]))
    assert np.array_equal(full[[3, 2, 1, 0]], run([3, 2, 1, 0]))
    for i in range(4):
        assert np.array_equal(full[i:i + 1], run([i]))
    assert np.array_equal(full[[1, 1, 3]], run([1, 1, 3]))
    eng.close()


def _facade(hw, ncls_file, dtype, max_batch=4):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = make_config(hw if hw[0] != hw[1] else hw[0], batch_size=3)
    return Yolov4(None, os.path.join(CLASS_DIR, ncls_file), cfg, dtype=dtype, max_batch=max_batch, synth_seed=3, tune=False)


# (box seeds: ones whose boxes leave every lane of these heads more than 1e-4 away from the ignore threshold, asserted below)
@pytest.mark.parametrize("hw,dtype,seed", [((160, 160), "f32", 9), ((160, 160), "bf16", 9), ((96, 160), "f32", 14)])
def test_training_model_predict_end_to_end(hw, dtype, seed):
    from yolo4hip.data import preprocess_true_boxes, records_from_dense
    from yolo4hip.engine import combine_loss
    m = _facade(hw, "bccd_classes.txt", dtype)
    assert m.training_model is not None and m.training_model.name == "training_model"
    n, ncls = 6, m.num_classes                                               # 6 images through max_batch 4: two chunks
    rng = np.random.default_rng(4)
    imgs = rng.uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)
    boxes = np.concatenate([LC.make_boxes(hw, ncls, 4, seed=seed), LC.make_boxes(hw, ncls, 4, seed=seed + 1)[2:]])
    y_true, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    loss = m.training_model.predict([imgs, *y_true, xywh])
    assert np.ndim(loss) == 0 and np.isfinite(loss)
    heads = m.yolo_model.predict(imgs)
    oracle = LO.loss_terms(heads, y_true, xywh, LC.ANCHORS, LC.STRIDES, ncls, m.iou_loss_thresh, hw)
    # the ignore threshold is a step: the synthetic heads must keep clear of it for the comparison to mean anything
    for s in range(3):
        _, max_iou, _ = LO.scale_terms(heads[s], y_true[s], xywh, LC.ANCHORS.reshape(3, 3, 2)[s], LC.STRIDES[s], ncls,
                                       m.iou_loss_thresh, float(hw[0] * hw[1]))
        assert not (np.abs(max_iou - m.iou_loss_thresh) < 1e-4).any()
    dense = m.engine.loss(imgs, records=records_from_dense(y_true, ncls), true_xywh=xywh)
    box_front = m.engine.loss(imgs, boxes=boxes)
    assert np.array_equal(dense.view(np.int32), box_front.view(np.int32))     # the dense front and the box front: same bits
    # no reference run exists for these heads: d_ref is the reference's own error where it was measured, the larger of the
    # two fixture sets with heads of order 1 per (scale, term)
    d_ref = np.maximum(*(load_fixture(name)[1]["d_ref"] for name in ("160_coco", "416_bccd")))
    _within_budget(f"e2e_{hw[0]}x{hw[1]}_{dtype}", dense, oracle, d_ref)
    assert abs(float(loss) - LO.total(oracle)) <= 5e-6 * LO.total(oracle)
    assert np.float32(combine_loss(dense)[0].mean()) == loss
    smooth = [y.copy() for y in y_true]
    smooth[0][..., 5:] = smooth[0][..., 5:] * 0.99 + 0.01 / ncls
    with pytest.raises(ValueError, match="smoothed"):
        m.training_model.predict([imgs, *smooth, xywh])
    with pytest.raises(NotImplementedError):
        m.fit(None, 1)
    m.engine.close()


def test_evaluate_over_a_generator_with_a_ragged_last_batch(tmp_path):
    from yolo4hip.data import DataGenerator
    from yolo4hip.engine import combine_loss
    hw = (160, 160)
    m = _facade(hw, "bccd_classes.txt", "f32")
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 8, 1])
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False, config=m.config)
    assert len(gen) == 2                                                     # batches of 3 and 2
    np.random.seed(11)
    res = m.evaluate(gen)
    assert set(res) == {"loss", "box", "conf", "class", "images"} and res["images"] == 5
    np.random.seed(11)                                                       # (get_data shuffles each image's boxes)
    singles = []
    for i in range(len(gen)):
        X, boxes = gen.boxes(i)
        for k in range(len(X)):
            singles.append(m.engine.loss(X[k:k + 1], boxes=boxes[k:k + 1])[0])
    total, box, conf, cls = combine_loss(np.stack(singles))
    assert res["loss"] == pytest.approx(total.mean(), rel=1e-12) and res["box"] == pytest.approx(box.mean(), rel=1e-12)
    assert res["conf"] == pytest.approx(conf.mean(), rel=1e-12) and res["class"] == pytest.approx(cls.mean(), rel=1e-12)
    assert res["loss"] == pytest.approx(res["box"] + res["conf"] + res["class"], rel=1e-12)
    m.engine.close()
