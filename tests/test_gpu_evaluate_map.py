"""`Yolov4.evaluate_map` (matching on the device, one copy per batch) against the file pipeline `export_gt` +
`export_prediction` + `eval_map` on the model of test_export_then_eval_map_pipeline: 160^2, bccd classes, f32, max_batch 2,
three copies of street.jpeg.  Also `fit(..., val_map=True)`."""
import math
import os
import shutil

import numpy as np
import pytest

from helpers import CLASS_DIR, GOLDEN

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.5, 0.75)
MARGIN = 1e-3


def _ground_truth_from(dets, k):
    """Annotation boxes of image k from its predictions (class id, x1, y1, x2, y2): coordinates rounded to integers; detection
    k + 1 dropped; every third remaining box shifted along x by 0.235 of its width, a few pixels, which puts its IoU with
    the detection near (1 - 0.235) / (1 + 0.235) = 0.62 -- past 0.5, short of 0.75; and one box far outside the image, which
    nothing detects."""
    rows = []
    for j, (cls, x1, y1, x2, y2) in enumerate(dets):
        if j == k + 1:
            continue
        x1, y1, x2, y2 = (int(round(v)) for v in (x1, y1, x2, y2))
        if j % 3 == k % 3:
            dx = max(1, int(round(0.235 * (x2 - x1 + 1))))
            x1, x2 = x1 + dx, x2 + dx
        rows.append((x1, y1, x2, y2, cls))
    rows.append((5000, 5000, 5040, 5040, 0))
    return rows


@pytest.fixture(scope="module")
def pipeline(tmp_path_factory):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    root = tmp_path_factory.mktemp("evalmap")
    imgdir, pred, gt = (str(root / d) for d in ("img", "pred", "gt"))
    for d in (imgdir, pred, gt):
        os.makedirs(d)
    names = [f"s{k}.jpeg" for k in range(3)]
    for name in names:
        shutil.copy(os.path.join(GOLDEN, "street.jpeg"), os.path.join(imgdir, name))
    ann0 = str(root / "ann0.txt")
    with open(ann0, "w") as fh:
        fh.write("".join(f"/data/{name}\n" for name in names))
    cfg = make_config(160)
    cfg["batch_size"] = 2
    m = Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), cfg, dtype="f32", max_batch=2)
    m.export_prediction(ann0, pred, imgdir, bs=2)
    ann = str(root / "ann.txt")
    n_det = 0
    with open(ann, "w") as fh:
        for k, name in enumerate(names):
            dets = []
            for line in open(os.path.join(pred, f"s{k}.txt")).read().splitlines():
                cls, _conf, x1, y1, x2, y2 = line.split(" ")
                dets.append((m.class_names.index(cls), float(x1), float(y1), float(x2), float(y2)))
            n_det += len(dets)
            fh.write(" ".join([f"/data/{name}"] + [",".join(str(v) for v in row) for row in _ground_truth_from(dets, k)]) + "\n")
    assert n_det >= 9, "the synthetic weights must produce detections on street.jpeg"
    m.export_gt(ann, gt)
    return {"model": m, "cfg": cfg, "root": root, "imgdir": imgdir, "pred": pred, "gt": gt, "ann": ann}


def _precondition(p):
    """From the files alone: every detection's best IoU keeps MARGIN from both thresholds and from the runner-up box.  The file
    pipeline reads the shortest decimal form of each float32 coordinate, the device the float32 itself: up to half a float32
    ulp apart (3.1e-5 px below 1024 px), which on boxes of 8 px and more a side moves an IoU by about 3e-5 -- MARGIN is 30
    times that.  A condition on the inputs, not on the code under test.  -> (detections, how many sit between the thresholds)."""
    from yolo4hip.evalmap import _iou_inclusive
    n, between, closest = 0, 0, math.inf
    for k in range(3):
        gts = [line.split() for line in open(os.path.join(p["gt"], f"s{k}.txt")).read().splitlines()]
        for line in open(os.path.join(p["pred"], f"s{k}.txt")).read().splitlines():
            cls, _conf, *bb = line.split()
            bb = [float(v) for v in bb]
            assert max(bb) < 1024 and bb[2] - bb[0] + 1 >= 8 and bb[3] - bb[1] + 1 >= 8, line
            ious = sorted((_iou_inclusive(bb, [float(v) for v in g[1:]]) for g in gts if g[0] == cls), reverse=True)
            ious = [v for v in ious if v > -1.0]
            n += 1
            if not ious:
                continue
            gaps = [abs(ious[0] - t) for t in THRESHOLDS] + ([ious[0] - ious[1]] if len(ious) > 1 else [])
            closest = min(closest, *gaps)
            between += THRESHOLDS[0] < ious[0] < THRESHOLDS[1]
    print(f"precondition: {n} detections, {between} between the thresholds, closest gap {closest:.3e}")
    assert closest >= MARGIN, closest
    return n, between


def _file_pipeline(p, thr, tag):
    from yolo4hip import evalmap
    tmp, out = str(p["root"] / f"tmp_{tag}"), str(p["root"] / f"out_{tag}")
    os.makedirs(tmp), os.makedirs(out)
    return evalmap.eval_map(p["gt"], p["pred"], tmp, out, min_overlap=thr, verbose=False)


def test_evaluate_map_equals_the_file_pipeline(pipeline):
    p = pipeline
    n, between = _precondition(p)
    got = p["model"].evaluate_map(p["ann"], p["imgdir"], bs=2, iou_thresholds=THRESHOLDS, channel_order="bgr")
    refs = [_file_pipeline(p, thr, f"path{t}") for t, thr in enumerate(THRESHOLDS)]
    for t, thr in enumerate(THRESHOLDS):
        for key in ("mAP", "ap", "tp", "fp"):
            assert got["per_threshold"][thr][key] == refs[t][key], (thr, key, got["per_threshold"][thr][key], refs[t][key])
        for key in ("n_gt", "n_images", "n_det"):
            assert got[key] == refs[t][key], (key, got[key], refs[t][key])
    for key in ("mAP", "ap", "tp", "fp"):
        assert got[key] == refs[0][key]
    assert got["mAP_mean"] == (refs[0]["mAP"] + refs[1]["mAP"]) / 2
    # the construction did what it was for: the shifted boxes count at 0.5 and not at 0.75, the dropped ones nowhere
    assert between >= 3
    assert sum(refs[0]["tp"].values()) - sum(refs[1]["tp"].values()) >= 3 and sum(refs[1]["tp"].values()) >= 3
    assert sum(refs[0]["fp"].values()) >= 3 and sum(got["n_det"].values()) == n


def test_generator_form_gives_the_numbers_of_the_path_form(pipeline):
    from yolo4hip.data import DataGenerator, read_annotation_lines
    p = pipeline
    m = p["model"]
    lines = [line.replace("/data/", "") for line in read_annotation_lines(p["ann"])]
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), p["imgdir"], shuffle=True, config=p["cfg"])
    for order in ("rgb", "bgr"):
        a = m.evaluate_map(p["ann"], p["imgdir"], bs=2, iou_thresholds=THRESHOLDS, channel_order=order)
        b = m.evaluate_map(gen, iou_thresholds=THRESHOLDS, channel_order=order)
        assert a == b
    assert m.evaluate_map(p["ann"], p["imgdir"], iou_thresholds=THRESHOLDS) == m.evaluate_map(gen, iou_thresholds=THRESHOLDS)
    with pytest.raises(ValueError, match="img_folder_path"):
        m.evaluate_map(p["ann"])
    with pytest.raises(ValueError, match="channel_order"):
        m.evaluate_map(gen, channel_order="gbr")


def test_fit_val_map(pipeline):
    from yolo4hip.data import DataGenerator, read_annotation_lines
    p = pipeline
    m = p["model"]
    # labels the loss accepts: the annotation's boxes clipped to the 273 x 185 image, without the one outside it
    lines = []
    for line in read_annotation_lines(p["ann"]):
        name, *objs = line.replace("/data/", "").split()
        rows = [[int(v) for v in obj.split(",")] for obj in objs if not obj.startswith("5000,")]
        rows = [(max(x1, 0), max(y1, 0), min(x2, 272), min(y2, 184), c) for x1, y1, x2, y2, c in rows]
        lines.append(" ".join([name] + [",".join(str(v) for v in r) for r in rows if r[2] > r[0] and r[3] > r[1]]))
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), p["imgdir"], shuffle=False, config=p["cfg"])
    with pytest.raises(ValueError, match="val_data_gen"):
        m.fit(gen, 1, trainable="heads", val_map=True)
    flat0 = m._flat.copy()
    state = np.random.get_state()       # DataGenerator shuffles each image's boxes on the global stream: the same draws per fit
    np.random.seed(1234)
    plain = m.fit(gen, 1, trainable="heads", val_data_gen=gen)
    assert sorted(plain.history) == ["loss", "val_loss"]
    flat1 = m._flat.copy()
    m._set_weights(flat0.copy())                     # (fit updates the array it is given in place)
    np.random.seed(1234)
    hist = m.fit(gen, 2, trainable="heads", val_data_gen=gen, val_map=True).history
    assert sorted(hist) == ["loss", "val_loss", "val_mAP"] and len(hist["val_mAP"]) == 2
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in hist["val_mAP"])
    assert hist["val_mAP"][-1] == m.evaluate_map(gen)["mAP"]
    # val_map changes nothing else (evaluate_map draws nothing from that stream either): the first epoch's loss and weights
    # are those of the plain run
    assert hist["loss"][0] == plain.history["loss"][0] and hist["val_loss"][0] == plain.history["val_loss"][0]
    m._set_weights(flat0.copy())
    np.random.seed(1234)
    again = m.fit(gen, 1, trainable="heads", val_data_gen=gen, val_map=True)
    assert np.array_equal(m._flat, flat1) and again.history["loss"] == plain.history["loss"]
    m._set_weights(flat0.copy())
    np.random.set_state(state)


def test_engine_map_match_on_the_models_own_boxes(pipeline):
    """`Engine.map_match_device(debug=True)` and the flat output block on real decode + NMS outputs -- float32 products that are
    no round decimals -- against the oracle: all four outputs with ==, and the block's host copy equal to the tensors."""
    import torch
    import map_oracle
    from yolo4hip import prepost
    from yolo4hip.data import read_map_annotations
    p = pipeline
    eng = p["model"].engine
    items = read_map_annotations(open(p["ann"]).readlines(), 3)[:2]
    raws = [prepost.imread_rgb(os.path.join(p["imgdir"], name.split("/")[-1]))[:, :, ::-1] for name, _, _ in items]
    imgs, _ = eng.preprocess_u8_batch(raws)
    gt = np.full((2, 130, 5), np.nan, dtype=np.float32)
    for k, (_, _, boxes) in enumerate(items):
        gt[k, :len(boxes)] = boxes
    count = torch.tensor([len(b) for _, _, b in items], dtype=torch.int32, device=eng.device)
    scale = torch.tensor([[r.shape[1], r.shape[0]] for r in raws], dtype=torch.float32, device=eng.device)
    flat, outs, tp_view = eng.alloc_map_outputs_flat(2)
    eng.forward_device(imgs)
    eng.decode_nms_device(2, outs)
    thresholds = (0.5, 0.6, 0.75, 0.9)
    tp, best, match, used = eng.map_match_device(outs, scale, torch.from_numpy(gt).to(eng.device), count, thresholds, debug=True,
                                                 tp_mask=tp_view)
    scores, classes, valid, tp_host = eng.map_outputs_to_host(flat, 2)
    assert tp is tp_view and np.array_equal(tp_host, tp.cpu().numpy().view(np.uint32))
    assert np.array_equal(scores, outs[1].cpu().numpy()) and np.array_equal(classes, outs[2].cpu().numpy())
    assert np.array_equal(valid, outs[3].cpu().numpy()) and valid.min() >= 3
    boxes = outs[0].cpu().numpy()
    for k, (_, _, rows) in enumerate(items):
        nb = int(valid[k])
        px = map_oracle.pixel_boxes(boxes[k, :nb], (raws[k].shape[1], raws[k].shape[0]))
        rtp, rbest, rmatch, rused = map_oracle.match_image(px, scores[k, :nb], classes[k, :nb], rows, thresholds)
        assert np.array_equal(match[k, :nb].cpu().numpy(), rmatch) and np.all(best[k, :nb].cpu().numpy() == rbest)
        assert np.array_equal(tp_host[k, :nb], rtp) and not tp_host[k, nb:].any()
        assert np.array_equal(used[k, :len(rows)].cpu().numpy().view(np.uint32), rused) and not used[k, len(rows):].any()
        assert rtp.any()
