"""`Yolov4.evaluate_coco` (matching on the device, one copy per batch) over the plain, the test-time-view and the tiled inference
path against the loop-form oracle (tests/coco_oracle.py) fed with what `inference_model.predict` / `predict_tta` / `predict_tiled`
return, on the model of test_gpu_evaluate_map.py: 160^2, bccd classes, f32, max_batch 2, three copies of street.jpeg.  The pixel
boxes are float32 products on both sides, so the comparison is ==.  Also the labels-follow-pixels check of the tiled path on
the marker photos and stand-in detector of tests/marker_photos.py."""
import os
import shutil

import numpy as np
import pytest

import coco_oracle
import marker_photos as MP
from helpers import CLASS_DIR, GOLDEN

pytestmark = pytest.mark.gpu

VIEWS = [(1.0, ''), (0.75, 'lr')]
PATHS = {"plain": {}, "views": {"views": VIEWS}, "tiled": {"tiled": True}}
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def _ground_truth_from(dets, k):
    """Annotation boxes of image k from its detections (x1, y1, x2, y2, class) in pixels: coordinates rounded to integers;
    detection (k + 1) mod count dropped (a false positive); every third remaining box shifted along x by 0.235 of its width,
    which puts its IoU near (1 - 0.235) / (1 + 0.235) = 0.62 -- matched at 0.5 .. 0.6, not above; and two boxes far outside the
    image, a small and a large one, which nothing detects (misses in two size buckets)."""
    rows = []
    for j, (x1, y1, x2, y2, cls) in enumerate(dets):
        if j == (k + 1) % len(dets):
            continue
        x1, y1, x2, y2 = (int(round(v)) for v in (x1, y1, x2, y2))
        if j % 3 == k % 3:
            dx = max(1, int(round(0.235 * (x2 - x1))))
            x1, x2 = x1 + dx, x2 + dx
        rows.append((x1, y1, x2, y2, int(cls)))
    rows += [(5000, 5000, 5020, 5020, 0), (6000, 6000, 6200, 6200, 1)]
    return rows


def _predict(m, path, raws):
    """What the facade's own predict calls return for the raw images -> (boxes [3,100,4], scores, classes, valid)."""
    if path == "views":
        return m.predict_tta(raws, views=VIEWS)
    if path == "tiled":
        return m.predict_tiled(raws)
    parts = []
    for i0 in range(0, len(raws), 2):
        if path == "letterbox":
            parts.append(m._predict_mapped(*m._letterboxed(raws[i0:i0 + 2])))
        else:
            parts.append(m.inference_model.predict(m.engine.preprocess_u8_batch(raws[i0:i0 + 2])[0]))
    return [np.concatenate([p[f] for p in parts]) for f in range(4)]


def _images(pred, raws, gts):
    """The oracle's dataset: per image (float32 pixel boxes, scores, classes, rows)."""
    boxes, scores, classes, valid = pred
    out = []
    for k, raw in enumerate(raws):
        nb = int(valid[k])
        px = coco_oracle.pixel_boxes(boxes[k, :nb], (raw.shape[1], raw.shape[0]))
        out.append((px, scores[k, :nb], classes[k, :nb], np.array(gts[k], dtype=np.float32).reshape(-1, 5)))
    return out


def _write_annotation(path, names, gts):
    with open(path, "w") as fh:
        for name, rows in zip(names, gts):
            fh.write(" ".join([f"/data/{name}"] + [",".join(str(v) for v in row) for row in rows]) + "\n")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from yolo4hip import prepost
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    root = tmp_path_factory.mktemp("evalcoco")
    imgdir = str(root / "img")
    os.makedirs(imgdir)
    names = [f"s{k}.jpeg" for k in range(3)]
    for name in names:
        shutil.copy(os.path.join(GOLDEN, "street.jpeg"), os.path.join(imgdir, name))
    cfg = make_config(160)
    cfg["batch_size"] = 2
    m = Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), cfg, dtype="f32", max_batch=2)
    raws = [prepost.imread_rgb(os.path.join(imgdir, name)) for name in names]
    per_path = {}
    for path in PATHS:
        pred = _predict(m, path, raws)
        gts = []
        for k, raw in enumerate(raws):
            nb = int(pred[3][k])
            px = coco_oracle.pixel_boxes(pred[0][k, :nb], (raw.shape[1], raw.shape[0]))
            gts.append(_ground_truth_from([tuple(px[j]) + (pred[2][k, j],) for j in range(nb)], k))
        ann = str(root / f"ann_{path}.txt")
        _write_annotation(ann, names, gts)
        per_path[path] = {"pred": pred, "gts": gts, "ann": ann, "images": _images(pred, raws, gts)}
    return {"model": m, "cfg": cfg, "imgdir": imgdir, "names": names, "raws": raws, "paths": per_path, "root": root}


def _assert_equals_oracle(res, images, what):
    precision, recall, stats = coco_oracle.evaluate(images, 3)
    print(what, dict(zip(STAT_NAMES, stats)))
    assert np.array_equal(res["precision"], precision), what
    assert np.array_equal(res["recall"], recall), what
    assert res["stats"] == stats and [res[k] for k in STAT_NAMES] == stats, (what, res["stats"], stats)
    return stats


@pytest.mark.parametrize("path", list(PATHS))
def test_evaluate_coco_equals_the_oracle(setup, path):
    m, p = setup["model"], setup["paths"][path]
    res = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, **PATHS[path])
    stats = _assert_equals_oracle(res, p["images"], path)
    # the construction did what it was for, read off the oracle's per-image flags under `all` at 0.5 and 0.75: true positives,
    # shifted boxes that count at 0.5 only, false positives; and ground truth in at least two size buckets
    tp50 = tp75 = fp50 = 0
    buckets = set()
    for px, scores, classes, rows in p["images"]:
        dm, di, _, gi, _ = coco_oracle.match_image(px, scores, classes, rows, coco_oracle.AREA_RNG, coco_oracle.IOU_THRS)
        assert len(scores) >= 3 and not di[0].any()
        tp50 += int((dm[0] & 1).sum()); tp75 += int(((dm[0] >> 5) & 1).sum()); fp50 += int((1 - (dm[0] & 1)).sum())
        buckets |= {a for a in (1, 2, 3) if (((gi >> a) & 1) == 0).any()}
    print(path, "tp@.5", tp50, "tp@.75", tp75, "fp@.5", fp50, "buckets", sorted(buckets))
    assert tp75 >= 3 and tp50 - tp75 >= 2 and fp50 >= 3 and len(buckets) >= 2
    assert sum(v > -1 for v in (res["APs"], res["APm"], res["APl"])) >= 2 and 0 < stats[0] < stats[1] < 1
    n_det = sum(len(im[1]) for im in p["images"])
    assert sum(res["n_det"].values()) == n_det and sum(res["n_gt"].values()) == sum(len(g) for g in p["gts"])
    assert set(res["per_class"]) == set(m.class_names)
    if path == "tiled":                                        # several rows per photo and one NMS over them were in play
        from yolo4hip import tiling
        h, w = setup["raws"][0].shape[:2]
        assert len(tiling.tile_rows(h, w, (160, 160), None, 0.2, True, False)) >= 4


@pytest.mark.parametrize("path", list(PATHS))
def test_bs_1_and_bs_2_give_the_same_result(setup, path):
    m, p = setup["model"], setup["paths"][path]
    a = m.evaluate_coco(p["ann"], setup["imgdir"], bs=1, **PATHS[path])
    b = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, **PATHS[path])
    assert a["stats"] == b["stats"] and np.array_equal(a["precision"], b["precision"]) and np.array_equal(a["recall"], b["recall"])
    assert a["n_det"] == b["n_det"] and a["per_class"] == b["per_class"]


def test_generator_form_and_channel_order(setup):
    from yolo4hip.data import DataGenerator, read_annotation_lines
    m, p = setup["model"], setup["paths"]["plain"]
    lines = [line.replace("/data/", "") for line in read_annotation_lines(p["ann"])]
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), setup["imgdir"], shuffle=True, config=setup["cfg"])
    a, b = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2), m.evaluate_coco(gen)
    assert a["stats"] == b["stats"] and np.array_equal(a["precision"], b["precision"])
    bgr = m.evaluate_coco(gen, channel_order="bgr")
    pred = _predict(m, "plain", [r[:, :, ::-1] for r in setup["raws"]])
    _assert_equals_oracle(bgr, _images(pred, setup["raws"], p["gts"]), "bgr")


def test_letterbox(setup, monkeypatch):
    m, p = setup["model"], setup["paths"]["plain"]
    monkeypatch.setattr(m, "_letterbox", True)
    pred = _predict(m, "letterbox", setup["raws"])
    assert not np.array_equal(pred[0], p["pred"][0]) and int(pred[3].min()) >= 1
    res = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2)
    _assert_equals_oracle(res, _images(pred, setup["raws"], p["gts"]), "letterbox")
    tiled = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, tiled=True, tile=128, overlap=0.25)
    pred = m.predict_tiled(setup["raws"], tile=128, overlap=0.25)
    _assert_equals_oracle(tiled, _images(pred, setup["raws"], p["gts"]), "letterbox tiled")


def test_other_ranges_and_max_dets(setup):
    m, p = setup["model"], setup["paths"]["plain"]
    ranges, max_dets = [[0, 1e10], [0, 2000]], (2, 5)
    res = m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, area_ranges=ranges, max_dets=max_dets)
    precision, recall = coco_oracle.tables(p["images"], 3, coco_oracle.IOU_THRS, ranges, max_dets + (10 ** 6,))
    assert res["precision"].shape == (10, 101, 3, 2, 2)
    assert np.array_equal(res["precision"], precision[..., :2]) and np.array_equal(res["recall"], recall[..., :2])
    assert res["APm"] == res["APl"] == res["AR100"] == -1.0 and res["APs"] > -1


def test_one_copy_per_batch_and_no_box_crosses(setup, monkeypatch):
    m = setup["model"]
    eng = m.engine
    blocks, copies = [], []
    alloc, to_host = eng.alloc_coco_outputs_flat, eng.coco_outputs_to_host

    def forbidden(*a, **k):
        raise AssertionError("evaluate_coco brings a batch back in the one copy of its flat block")

    monkeypatch.setattr(eng, "alloc_coco_outputs_flat", lambda *a: blocks.append(alloc(*a)) or blocks[-1])
    monkeypatch.setattr(eng, "coco_outputs_to_host", lambda flat, *a: copies.append(flat) or to_host(flat, *a))
    for name in ("tiled_outputs_to_host", "map_outputs_to_host", "alloc_tiled_outputs_flat", "alloc_outputs", "alloc_outputs_flat"):
        monkeypatch.setattr(eng, name, forbidden)
    for path, kw in PATHS.items():
        blocks.clear(); copies.clear()
        m.evaluate_coco(setup["paths"][path]["ann"], setup["imgdir"], bs=2, **kw)
        assert len(blocks) == 2 and len(copies) == 2 and all(c is b[0] for c, b in zip(copies, blocks)), path     # 2 + 1 images
        for flat, outs, cand, match_out in blocks:
            n = outs[1].shape[0]
            base = flat.untyped_storage().data_ptr()
            assert flat.numel() == n * (100 + 100 + 1 + 1 + 100 + 4 * 100 + 4 * 100 + 256)          # no [n,100,4] boxes in it
            assert outs[0].untyped_storage().data_ptr() != base                                   # the boxes stay behind
            for t in (outs[1], outs[2], outs[3], cand) + tuple(match_out):
                assert t.untyped_storage().data_ptr() == base


def test_argument_errors(setup, monkeypatch):
    m, p = setup["model"], setup["paths"]["plain"]
    ann, imgdir = p["ann"], setup["imgdir"]

    def no_upload(*a, **k):
        raise AssertionError("a bad argument must be refused before anything is uploaded")

    for name in ("preprocess_u8_batch", "_upload_ragged", "forward_device"):
        monkeypatch.setattr(m.engine, name, no_upload)
    monkeypatch.setattr(m, "_eval_batches", no_upload)
    for kw, word in [({"img_folder_path": None}, "img_folder_path"), ({"channel_order": "gbr"}, "channel_order"),
                     ({"bs": 0}, "bs"), ({"views": [(1.5, '')]}, "scale"), ({"views": []}, "view"),
                     ({"max_dets": (10, 1)}, "max_dets"), ({"max_dets": ()}, "max_dets"), ({"area_ranges": [[5, 1]]}, "area_ranges"),
                     ({"area_ranges": [[0, 1]] * 5}, "area_ranges"), ({"tile": 64}, "tiled=True"),
                     ({"tiled": True, "overlap": 1.0}, "overlap"), ({"tiled": True, "tile": 0}, "tile"),
                     ({"tiled": True, "tile_candidates": 0}, "tile_candidates")]:
        args = {"img_folder_path": imgdir, **kw}
        with pytest.raises(ValueError, match=word):
            m.evaluate_coco(ann, **args)
    with pytest.raises(TypeError):
        m.evaluate_coco(ann, imgdir, 2, 'rgb')                 # the options are keyword-only


def test_tile_candidates_overflow_is_reported(setup):
    m, p = setup["model"], setup["paths"]["tiled"]
    with pytest.raises(RuntimeError, match="tile_candidates"):
        m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, tiled=True, tile_candidates=1)
    with pytest.raises(RuntimeError, match="tile_candidates"):
        m.evaluate_coco(p["ann"], setup["imgdir"], bs=2, views=VIEWS, tile_candidates=1)


# ------------------------------------------------------------------------------------------------ labels follow pixels, tiled path
MARKER_SIZES = [(240, 320), (200, 260), (160, 300)]           # (h, w), every side >= the 160^2 canvas: every window is a 1:1 copy
MARKER_SEED, MARKER_OVERLAP = 3, 0.5                            # a seed whose markers all lie whole in some window (asserted)


def _tiled_stand_in(m, served, truth, bs, monkeypatch):
    """forward_device of m.engine replaced for the tiled path: every marker that lies WHOLE in the row's window becomes a head
    cell (a marker cut by the window's edge is what a real detector would box badly; the stand-in leaves it to the window that
    shows it whole).  served: the photos in the order the images are read.  The windows arrive in `_rows_device`'s order: per
    chunk of max_batch photos, photo by photo, every window of `tiling.tile_rows`."""
    from yolo4hip import tiling
    eng = m.engine
    hw = tuple(m.img_size[:2])
    step = min(bs, eng.max_batch)
    queue = []
    for start in range(0, len(served), bs):
        for i0 in range(start, min(start + bs, len(served)), step):
            for a in served[i0:min(i0 + step, start + bs)]:
                rows = tiling.tile_rows(a.shape[0], a.shape[1], hw, None, MARKER_OVERLAP, False, False)
                assert all(rect == (hw[0], hw[1], 0, 0) for _, rect, _ in rows)
                queue.extend(win for win, _, _ in rows)
    seen = []

    def forward(imgs_dev):
        canvases = imgs_dev.cpu().numpy()
        assert canvases.dtype == np.uint8
        wins = [queue.pop(0) for _ in canvases]
        heads, _, found = MP.detect_markers(canvases, lambda q: truth[q], hw, 3, m.config["anchors"], m.config["xyscale"],
                                            accept=lambda i, q, j: j in MP.whole_markers(truth[q], wins[i]))
        seen.extend(found)
        assert eng.set_heads(heads) == len(canvases)

    monkeypatch.setattr(eng, "forward_device", forward)
    return queue, seen


def test_tiled_labels_follow_pixels_on_marker_photos(tmp_path_factory, monkeypatch):
    from PIL import Image
    from test_gpu_labels_follow_pixels import _model
    from yolo4hip import tiling
    import test_labels_follow_pixels_cpu as LC
    hw = (160, 160)
    m = _model(hw)
    monkeypatch.setattr(m, "_letterbox", False)
    ds = LC.dataset(tmp_path_factory.mktemp("coco_markers"), MARKER_SIZES, MARKER_SEED, min_side=20)
    photos, truth = ds["photos"], ds["truth"]
    for a, t in zip(photos, truth):                            # the condition on the inputs: every marker whole in some window
        rows = tiling.tile_rows(a.shape[0], a.shape[1], hw, None, MARKER_OVERLAP, False, False)
        assert len(rows) >= 3 and set().union(*(MP.whole_markers(t, win) for win, _, _ in rows)) == set(range(len(t)))
    ann = os.path.join(ds["folder"], "ann.txt")
    with open(ann, "w") as fh:
        fh.writelines(ds["lines"])
    kw = dict(bs=3, tiled=True, overlap=MARKER_OVERLAP, full_image=False)
    queue, seen = _tiled_stand_in(m, photos, truth, 3, monkeypatch)
    res = m.evaluate_coco(ann, ds["folder"], **kw)
    assert not queue and sum(len(f) for f in seen) >= sum(len(t) for t in truth)
    perfect = coco_oracle.evaluate([(t[:, :4], np.ones(len(t), np.float32), t[:, 4], t) for t in truth], 3)[2]
    print("markers, tiled:", {k: res[k] for k in STAT_NAMES}, "perfect boxes:", perfect[0])
    assert abs(res["AP"] - perfect[0]) <= 1e-12 and perfect[0] > 0.99
    assert sum(res["n_det"].values()) == sum(len(t) for t in truth) == sum(res["n_gt"].values())      # every marker exactly once
    # the negative control: the same labels, every image file holding its neighbour's pixels
    rotated = tmp_path_factory.mktemp("coco_markers_rotated")
    served = [photos[(k + 1) % len(photos)] for k in range(len(photos))]
    for k, a in enumerate(served):
        Image.fromarray(a).save(os.path.join(str(rotated), f"m{k}.png"))
    queue, _ = _tiled_stand_in(m, served, truth, 3, monkeypatch)
    bad = m.evaluate_coco(ann, str(rotated), **kw)
    print("rotated by one image:", bad["AP"])
    assert not queue and bad["AP"] < 0.5
