"""Host side of the validation loss: the labels (`preprocess_true_boxes`, records, `DataGenerator`) against fixtures the
reference's own functions wrote (tests/golden/make_loss_fixtures.py), and the float64 restatement of the loss
(tests/loss_oracle.py) against the reference's float32 components."""
import os

import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
from helpers import CLASS_DIR, GOLDEN, PKG_DIR

CASE_NAMES = sorted(LC.CASES)


def load_fixture(name):
    """-> (case inputs, fixture arrays, dense labels rebuilt from the stored sparse form)."""
    case = LC.make_case(name)
    fx = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
    assert str(fx["sha"]) == case["sha"], "the seeded inputs drifted from the ones the fixture was generated with"
    labels = []
    for s, stride in enumerate(LC.STRIDES):
        y = np.zeros((case["n"], case["hw"][0] // stride, case["hw"][1] // stride, 3, 5 + case["ncls"]), dtype=np.float32)
        y.reshape(-1)[fx[f"label{s}_idx"]] = fx[f"label{s}_val"]
        labels.append(y)
    return case, fx, labels


@pytest.mark.parametrize("name", CASE_NAMES)
def test_preprocess_true_boxes_equals_reference(name):
    from yolo4hip.data import preprocess_true_boxes
    case, fx, labels = load_fixture(name)
    y_true, xywh = preprocess_true_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
    assert xywh.dtype == np.float32 and np.array_equal(xywh, fx["true_xywh"])
    for y, ref in zip(y_true, labels):
        assert y.dtype == np.float32 and y.shape == ref.shape and np.array_equal(y, ref)
    # the cases hold what they are meant to hold
    assert any(((y[..., 4] == 1) & (y[..., 5:].sum(axis=-1) > 1)).any() for y in y_true)          # a two-class collision
    assert all((y[..., 4] == 1).any() for y in y_true)                                             # every scale is used


def test_preprocess_true_boxes_rectangle_self_consistent():
    from yolo4hip.data import preprocess_true_boxes, records_from_boxes
    hw, ncls = (96, 160), 5
    boxes = LC.make_boxes(hw, ncls, 4, seed=7)
    y_true, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    assert [y.shape for y in y_true] == [(4, 12, 20, 3, 10), (4, 6, 10, 3, 10), (4, 3, 5, 3, 10)]
    assert np.array_equal(xywh[..., 0:2], (boxes[..., 0:2] + boxes[..., 2:4]) // 2)
    assert np.array_equal(xywh[..., 2:4], boxes[..., 2:4] - boxes[..., 0:2])
    recs, xywh2 = records_from_boxes(boxes, hw, LC.ANCHORS, ncls)
    assert np.array_equal(xywh, xywh2)
    for b, rec in enumerate(recs):
        assert len(rec) == sum(int((y[b, ..., 4] == 1).sum()) for y in y_true)
        for r in rec:
            cell = y_true[r[0]][b, r[1], r[2], r[3]]
            assert cell[4] == 1 and np.array_equal(cell[0:4].view(np.int32), r[4:8])
            # the cell is floor(float32(centre / side) * grid), which can lie one below centre // stride (40 / 96 * 12 < 5);
            # a degenerate row (image 2) shifts which row's centre is used, so that image is left to the fixtures
            if b != 2:
                g = y_true[r[0]].shape[1:3]
                assert r[2] == int(np.floor(np.float64(np.float32(cell[0] / np.float64(hw[1]))) * g[1]))
                assert r[1] == int(np.floor(np.float64(np.float32(cell[1] / np.float64(hw[0]))) * g[0]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_restatement_reproduces_reference_components(name):
    case, fx, labels = load_fixture(name)
    terms = LO.loss_terms(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH,
                          case["hw"])
    # float32 results of sums of up to 8112 x 85 float32 terms: 2e-6 relative is ~16 ulp
    assert LO.rel_dist(fx["ref_img"], terms).max() < 2e-6
    assert np.array_equal(LO.rel_dist(fx["ref_img"], terms).max(axis=0), fx["d_ref"])
    assert LO.rel_dist(fx["ref_batch"], terms.mean(axis=0)).max() < 2e-6
    assert abs(LO.total(terms) - float(fx["ref_total"])) < 2e-6 * float(fx["ref_total"])
    assert np.all(terms[0, :, 0] == 0) and np.all(terms[0, :, 2] == 0) and np.all(terms[0, :, 1] > 0)   # the image without boxes
    assert np.all(fx["ignore_count"] > 0)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_records_round_trip(name):
    from yolo4hip.data import dense_from_records, pad_records, record_words, records_from_boxes, records_from_dense
    case, fx, labels = load_fixture(name)
    recs = records_from_dense(labels, case["ncls"])
    recs_b, xywh = records_from_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
    assert np.array_equal(xywh, fx["true_xywh"])
    for a, b in zip(recs, recs_b):
        assert a.dtype == np.int32 and a.shape[1] == record_words(case["ncls"]) and np.array_equal(a, b)
        keys = [tuple(r[0:4]) for r in a]
        assert keys == sorted(set(keys))
    back = dense_from_records(recs, case["hw"], case["ncls"])
    for y, ref in zip(back, labels):
        assert np.array_equal(y, ref)
    padded, counts = pad_records(recs, LC.MAX_BOXES, case["ncls"])
    assert padded.shape == (case["n"], LC.MAX_BOXES, record_words(case["ncls"])) and counts[0] == 0
    assert record_words(80) == 11 and record_words(3) == 9


def test_refused_inputs():
    from yolo4hip.data import pad_records, preprocess_true_boxes, records_from_boxes, records_from_dense
    boxes = np.zeros((1, 100, 5), dtype=np.float32)
    boxes[0, 0] = [400, 10, 440, 50, 0]                                   # centre x = 420 >= 416
    with pytest.raises(ValueError, match="outside"):
        preprocess_true_boxes(boxes, (416, 416), LC.ANCHORS, 3)
    boxes[0, 0] = [-60, 10, 20, 50, 0]                                    # centre x = -20: numpy would wrap the index
    with pytest.raises(ValueError, match="outside"):
        records_from_boxes(boxes, (416, 416), LC.ANCHORS, 3)
    boxes[0, 0] = [10, 10, 50, 50, 3]
    with pytest.raises(ValueError, match="class id 3"):
        preprocess_true_boxes(boxes, (416, 416), LC.ANCHORS, 3)
    boxes[0, 0] = [10, 10, 50, 50, -1]
    with pytest.raises(ValueError, match="class id -1"):
        preprocess_true_boxes(boxes, (416, 416), LC.ANCHORS, 3)
    boxes[0, 0] = [10, 10, 50, 50, 2]
    y_true, _ = preprocess_true_boxes(boxes, (416, 416), LC.ANCHORS, 3)
    smooth = [y.copy() for y in y_true]
    s = [i for i, y in enumerate(smooth) if (y[..., 4] == 1).any()][0]
    smooth[s][smooth[s][..., 4] == 1, 5:] = [0.005, 0.005, 0.99]
    with pytest.raises(ValueError, match="smoothed"):
        records_from_dense(smooth, 3)
    recs = records_from_dense(y_true, 3)
    with pytest.raises(ValueError, match="max_boxes"):
        pad_records([np.zeros((101, 9), dtype=np.int32)], 100, 3)
    with pytest.raises(ValueError):
        preprocess_true_boxes(boxes[:, :, :4], (416, 416), LC.ANCHORS, 3)
    assert len(recs[0]) == 1


def _write_dataset(tmp_path, sizes, boxes_per_image):
    from PIL import Image
    rng = np.random.default_rng(3)
    lines = []
    for i, ((h, w), m) in enumerate(zip(sizes, boxes_per_image)):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / f"im{i}.png")
        objs = []
        for _ in range(m):
            x1, y1 = rng.integers(0, w // 2), rng.integers(0, h // 2)
            objs.append(f"{x1},{y1},{x1 + rng.integers(8, w // 2)},{y1 + rng.integers(8, h // 2)},{rng.integers(0, 3)}")
        lines.append(f"im{i}.png " + " ".join(objs) + "\n")
    return lines


def test_data_generator_shapes_scaling_and_labels(tmp_path):
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator, preprocess_true_boxes, read_annotation_lines
    lines = _write_dataset(tmp_path, [(120, 200), (160, 160), (90, 64)], [3, 0, 5])
    ann = tmp_path / "ann.txt"
    ann.write_text("".join(lines))
    assert read_annotation_lines(str(ann)) == lines
    train, test = read_annotation_lines(str(ann), test_size=1)
    assert len(train) == 2 and len(test) == 1
    cfg = make_config((96, 160), batch_size=2)
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False, config=cfg)
    assert len(gen) == 2 and gen.num_classes == 3 and gen.batch_size == 2 and gen.max_boxes == 100
    (X, y_s, y_m, y_l, xywh), zeros = gen[0]
    assert X.shape == (2, 96, 160, 3) and X.dtype == np.float32 and 0 <= X.min() and X.max() <= 1
    assert y_s.shape == (2, 12, 20, 3, 8) and y_m.shape == (2, 6, 10, 3, 8) and y_l.shape == (2, 3, 5, 3, 8)
    assert xywh.shape == (2, 100, 4) and zeros.shape == (2,) and not zeros.any()
    Xb, boxes = gen.boxes(0)
    assert np.array_equal(X, Xb) and boxes.shape == (2, 100, 5) and boxes.dtype == np.float32
    # the first image is 120 x 200 -> 96 x 160: x scales by 0.8, y by 0.8; its 3 boxes are a shuffle of the annotated ones
    want = np.array([[float(v) for v in o.split(",")] for o in lines[0].split()[1:]], dtype=np.float32)
    want[:, [0, 2]] *= 160 / 200
    want[:, [1, 3]] *= 96 / 120
    got = boxes[0, :3]
    assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())) and not boxes[0, 3:].any()
    assert not boxes[1].any()
    y_true, xywh2 = preprocess_true_boxes(boxes, (96, 160), gen.anchors, 3)
    # (gen[0] drew its own shuffle of the rows: compare the label sets through a second, seeded draw)
    np.random.seed(5)
    (_, a_s, a_m, a_l, a_xywh), _ = gen[0]
    np.random.seed(5)
    _, boxes5 = gen.boxes(0)
    y5, xywh5 = preprocess_true_boxes(boxes5, (96, 160), gen.anchors, 3)
    assert np.array_equal(a_xywh, xywh5) and all(np.array_equal(a, b) for a, b in zip((a_s, a_m, a_l), y5))
    (X1, *_), z1 = gen[1]
    assert X1.shape == (1, 96, 160, 3) and z1.shape == (1,)
    default = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False)
    assert default.target_img_size == (416, 416, 3) and default.batch_size == 8 and default.anchors.shape == (9, 2)


def test_drop_in_utils_exports_the_label_names():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_utils", os.path.join(PKG_DIR, "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from yolo4hip import data
    assert mod.DataGenerator is data.DataGenerator and mod.preprocess_true_boxes is data.preprocess_true_boxes
    assert mod.read_annotation_lines is data.read_annotation_lines
    assert callable(mod.load_weights) and callable(mod.draw_bbox)
