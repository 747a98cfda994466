"""Labels follow pixels on the device: the seeded cases of tests/test_labels_follow_pixels_cpu.py through
`Engine.augment_u8_batch`, `mosaic_u8_batch`, `preprocess_u8_batch`, `Yolov4.fit`, `Yolov4.evaluate_map` and the pieces of
`Engine.predict_tiled_device`, read with the predicates of tests/marker_photos.py.

Every case first asserts that the device's canvas has the bytes of the host restatement -- without that a later failure cannot
be read -- and then applies the predicates to the device's own bytes.  The detector of items 3 and 4 is a stand-in for the
forward pass: it reads the exact-colour rectangle of every marker off the uint8 canvas the network would see and writes the heads
whose decode is that rectangle (`marker_photos.heads_for_rects`, held to oracle/decode_nms.py on the CPU)."""
import functools

import numpy as np
import pytest

import marker_photos as MP
import test_labels_follow_pixels_cpu as LC
from test_labels_follow_pixels_cpu import EVAL_CANVASES, EVAL_SIZES, FIT_CASES, NAMES

pytestmark = pytest.mark.gpu
MAX_BATCH = 2


@functools.lru_cache(maxsize=None)
def _engine(hw):
    """A bare engine (the canvas kernels, decode and NMS read no weights): 3 classes, max_batch 2."""
    from decode_nms_cases import _engine as bare
    return bare(hw, 3, MAX_BATCH)


@functools.lru_cache(maxsize=None)
def _model(hw):
    """One bf16 facade per canvas for the module (a test that wants letterbox=True sets the flag evaluate_map reads)."""
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    return Yolov4(None, NAMES, make_config(hw, batch_size=3), dtype="bf16", max_batch=MAX_BATCH, synth_seed=3, tune=False)


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    return LC.dataset(tmp_path_factory.mktemp("markers"))


@pytest.fixture(scope="module")
def eval_ds(tmp_path_factory):
    return LC.eval_dataset(tmp_path_factory.mktemp("eval_markers"))


# ------------------------------------------------------------------------------------------------ 1. the canvas kernels
@pytest.mark.parametrize("hw", EVAL_CANVASES)
def test_augment_u8_batch(ds, hw):
    from yolo4hip.augment import augment_host
    _, eng = _engine(hw)
    rows = 0
    for b, batch in enumerate(LC.augment_batches(ds, hw)):
        imgs, params, boxes = batch
        got = eng.augment_u8_batch(imgs, params, pad_value=MP.PAD).cpu().numpy()
        for i, (img, p) in enumerate(zip(imgs, params)):
            assert np.array_equal(got[i], augment_host(img, p, hw, MP.PAD)), (b, i, p)
        rows += LC.check_augment_batch(got, batch, hw, f"device augment {hw} batch {b}")[0]
    assert rows >= 40


@pytest.mark.parametrize("hw", EVAL_CANVASES)
def test_mosaic_u8_batch(ds, hw):
    from yolo4hip.augment import mosaic_host
    _, eng = _engine(hw)
    rows = 0
    for b, batch in enumerate(LC.mosaic_batches(ds, hw)):
        imgs, tile_src, params, cuts, boxes = batch
        got = eng.mosaic_u8_batch(imgs, tile_src, params, cuts, pad_value=MP.PAD).cpu().numpy()
        for i in range(len(cuts)):
            assert np.array_equal(got[i], mosaic_host([imgs[k] for k in tile_src[i]], params[i], cuts[i], hw, MP.PAD)), (b, i)
        rows += LC.check_mosaic_batch(got, batch, hw, f"device mosaic {hw} batch {b}")[0]
    assert rows >= 60


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("hw", EVAL_CANVASES)
def test_preprocess_u8_batch(ds, hw, letterbox):
    """Batches of 4 and 2 photos of six sizes: the canvas of `place_row`, the map of `prepost.box_map`, predicate 3 through the
    map the DEVICE returned (row i's map must belong to image i)."""
    from yolo4hip import prepost
    _, eng = _engine(hw)
    H, W = hw
    count = 0
    for order in ([3, 0, 5, 1], [4, 2]):
        photos = [ds["photos"][k] for k in order]
        out, maps = eng.preprocess_u8_batch(photos, letterbox=letterbox, pad_value=MP.PAD)
        out, maps = out.cpu().numpy(), maps.cpu().numpy()
        for i, k in enumerate(order):
            h, w = photos[i].shape[:2]
            rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
            assert np.array_equal(out[i], MP.place_row(photos[i], (0, 0, h, w), rect, hw)), (order, i)
            assert np.array_equal(maps[i], prepost.box_map(h, w, H, W, rect))
            res = LC.check_inference_row(out[i], ((0, 0, h, w), rect, maps[i]), ds["truth"][k], (h, w), hw,
                                         f"device preprocess {hw} lb={letterbox} photo {k}", k)
            assert len(res) == len(ds["truth"][k])
            count += len(res)
    assert count == sum(len(t) for t in ds["truth"])


# ------------------------------------------------------------------------------------------------ 2. fit pairs chunks with labels
@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_pairs_every_chunk_with_its_labels(eval_ds, name, monkeypatch):
    """One epoch of `Yolov4.fit(trainable='heads')` on a bf16 model: the wrappers of the training engine's `forward_device` and
    `assign_device` record the chunk and the label slice they are handed; every recorded (canvas, label rows) pair then satisfies
    predicates 1 and 2, with the tile geometry the generator handed out for that image."""
    hw = FIT_CASES[name][0]
    m = _model(hw)
    eng = m._train_engine(1)
    gen = LC.fit_generator(eval_ds, name)
    log, chunks, labels = [], [], []
    for k, fn in LC.recorded(gen, eval_ds, log).items():
        monkeypatch.setattr(gen, k, fn)
    forward, assign = eng.forward_device, eng.assign_device

    def w_forward(chunk):
        chunks.append(chunk.cpu().numpy())
        return forward(chunk)

    def w_assign(boxes_dev):
        labels.append(boxes_dev.cpu().numpy())
        return assign(boxes_dev)

    monkeypatch.setattr(eng, "forward_device", w_forward)
    monkeypatch.setattr(eng, "assign_device", w_assign)
    m.fit(gen, 1, trainable="heads", learning_rate=1e-4)
    assert [len(c) for c in chunks] == [len(l) for l in labels] == [2, 1, 2]            # chunks of max_batch, the ragged one too
    canvases = np.concatenate([c if c.dtype == np.uint8 else np.rint(c * 255.0).astype(np.uint8) for c in chunks])
    assert (chunks[0].dtype == np.uint8) == (name != "plain")
    rows_dev = np.concatenate(labels)
    tiles = [t for entry in log for t in entry[0]]
    assert len(canvases) == len(rows_dev) == len(tiles) == len(EVAL_SIZES)
    # the canvas is the host restatement's, image by image
    from yolo4hip.augment import augment_host, mosaic_host
    k = 0
    for per_canvas, boxes, host, extra in log:
        for i in range(len(per_canvas)):
            if host is not None:
                want = host[i]
            elif len(extra) == 2:
                want = augment_host(extra[0][i], extra[1][i], hw, MP.PAD)
            else:
                imgs, src, params, cuts = extra
                want = mosaic_host([imgs[j] for j in src[i]], params[i], cuts[i], hw, MP.PAD)
            assert np.array_equal(canvases[k], want), (name, k)
            k += 1
    rows = 0
    for k in range(len(canvases)):
        rows += MP.check_canvas(canvases[k], rows_dev[k], tiles[k], f"fit {name} image {k}")[0]
    assert rows >= 8


# ------------------------------------------------------------------------------------------------ 3. evaluate_map
def _stand_in(m, eval_ds, seen, rotate_from=None):
    """forward_device of m.engine replaced: the uint8 canvases come back, every marker's exact-colour rectangle becomes a head
    cell, `set_heads` loads them.  rotate_from: the canvases of an earlier run, in image order -- image k is then served the
    canvas of image k + 1 (the negative control)."""
    eng = m.engine
    hw = tuple(m.img_size[:2])

    def forward(imgs_dev):
        canvases = imgs_dev.cpu().numpy()
        assert canvases.dtype == np.uint8
        k0 = len(seen)
        seen.extend(canvases)
        if rotate_from is not None:
            canvases = [rotate_from[(k0 + i + 1) % len(rotate_from)] for i in range(len(canvases))]
        heads, slots, found = MP.detect_markers(canvases, lambda p: eval_ds["truth"][p], hw, 3, m.config["anchors"], m.config["xyscale"])
        assert eng.set_heads(heads) == len(canvases)

    return forward


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("hw", EVAL_CANVASES)
def test_a_detector_that_boxes_every_marker_scores_map_1(eval_ds, hw, letterbox, monkeypatch):
    from yolo4hip import prepost
    m = _model(hw)
    monkeypatch.setattr(m, "_letterbox", letterbox)
    H, W = hw
    gen = LC.generator(eval_ds, hw, 3)
    seen = []
    monkeypatch.setattr(m.engine, "forward_device", _stand_in(m, eval_ds, seen))
    res = m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75))
    # the canvases the detector saw are the host restatement's, in annotation order
    assert len(seen) == len(EVAL_SIZES)
    for p, photo in enumerate(eval_ds["photos"]):
        h, w = photo.shape[:2]
        rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
        assert np.array_equal(seen[p], MP.place_row(photo, (0, 0, h, w), rect, hw)), p
    n_gt = {c: sum(int((t[:, 4] == k).sum()) for t in eval_ds["truth"]) for k, c in enumerate(m.class_names)}
    print(f"evaluate_map {hw} letterbox={letterbox}:", {k: res[k] for k in ("mAP", "tp", "fp", "n_gt")}, res["per_threshold"])
    assert res["n_gt"] == {c: v for c, v in n_gt.items() if v} and sum(res["n_det"].values()) == sum(n_gt.values())
    for thr in (0.5, 0.75):
        r = res["per_threshold"][thr]
        assert r["mAP"] == 1.0
        for c in m.class_names:
            if n_gt[c]:
                assert r["tp"][c] == n_gt[c] and r["fp"][c] == 0, (thr, c, r)
    assert res["mAP"] == 1.0
    # the negative control: every image is served its neighbour's canvas
    again = []
    monkeypatch.setattr(m.engine, "forward_device", _stand_in(m, eval_ds, again, rotate_from=list(seen)))
    bad = m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75))
    print("rotated by one image:", bad["mAP"])
    assert bad["mAP"] < 0.5


# ------------------------------------------------------------------------------------------------ 4. tiled rows
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("hw", EVAL_CANVASES)
def test_tiled_rows_return_every_marker_once(tmp_path_factory, hw, letterbox):
    """The pieces `Engine.predict_tiled_device` calls, in its order, with `set_heads` in place of the forward: one upload of photos,
    window descriptors and maps, per chunk of max_batch rows y4_window_u8_ragged -> (stand-in) -> decode_gather, then nms_gathered."""
    import ctypes as C
    import torch
    from yolo4hip import ext, tiling
    cfg, eng = _engine(hw)
    H, W = hw
    tds = LC.tiled_dataset(tmp_path_factory.mktemp("tiled"))
    photos, truth = tds["photos"], tds["truth"]
    photo, slot, rows = [], [], []
    for p, a in enumerate(photos):
        for t, row in enumerate(tiling.tile_rows(a.shape[0], a.shape[1], hw, None, 0.2, True, letterbox)):
            photo.append(p); slot.append(t); rows.append(row)
    R, P, max_slots = len(rows), len(photos), max(slot) + 1
    assert R > 2 * MAX_BATCH and R % MAX_BATCH == 1                     # several chunks, one of both photos, a ragged last one
    desc = (ext.y4_window_desc * R)()
    for d, (_, rect, _) in zip(desc, rows):
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
    extra = np.concatenate([np.asarray([r[2] for r in rows], np.float32).reshape(-1).view(np.int32), np.asarray(photo, np.int32),
                            np.asarray(slot, np.int32)])
    dev, desc_bytes, head = eng._upload_ragged(photos, desc, extra, rows=photo, windows=[r[0] for r in rows])
    tab = dev[desc_bytes:head].view(torch.int32)
    row_map, row_group, row_slot = tab[:4 * R].view(torch.float32).view(R, 4), tab[4 * R:5 * R], tab[5 * R:6 * R]
    state = eng.gather_begin(P, max_slots, max_slots * eng.num_boxes * eng.num_classes)
    step = C.sizeof(ext.y4_window_desc)
    canvas = torch.empty((MAX_BATCH, H, W, 3), dtype=torch.uint8, device=eng.device)
    src = C.c_void_p(dev.data_ptr() + head)
    shown = [set() for _ in photos]
    for r0 in range(0, R, MAX_BATCH):
        n = min(MAX_BATCH, R - r0)
        eng._canvas_launch(eng.lib.y4_window_u8_ragged, src, (C.c_void_p(dev.data_ptr() + r0 * step),), n, canvas, MP.PAD)
        got = canvas[:n].cpu().numpy()
        for i in range(n):
            win, rect, _ = rows[r0 + i]
            assert np.array_equal(got[i], MP.place_row(photos[photo[r0 + i]], win, rect, hw)), (r0 + i, win, rect)

        def whole(i, p, j, r0=r0):                      # the detector boxes what it sees whole; a marker of another photo is an error
            assert p == photo[r0 + i], (r0 + i, p, photo[r0 + i])
            return j in MP.whole_markers(truth[p], rows[r0 + i][0])

        heads, _, found = MP.detect_markers(got, lambda p: truth[p], hw, 3, cfg["anchors"], cfg["xyscale"], accept=whole)
        for i, mine in enumerate(found):
            shown[photo[r0 + i]] |= {j for _, j, _, _ in mine}
        assert eng.set_heads(heads) == n
        eng.decode_gather(state, n, row_group[r0:r0 + n], row_slot[r0:r0 + n], row_map[r0:r0 + n])
    outs, cnt = eng.nms_gathered(state)
    torch.cuda.synchronize()
    boxes, scores, classes, valid, kept = (o.cpu().numpy() for o in outs)
    for p, a in enumerate(photos):
        h, w = a.shape[:2]
        assert shown[p] == set(range(len(truth[p])))                        # the full image shows every marker whole
        hit = []
        for k in range(int(valid[p])):
            box = boxes[p, k].astype(np.float64) * (w, h, w, h)
            j = int(np.argmax([MP.iou(list(box), [float(v) for v in t[:4]]) for t in truth[p]]))
            row = rows[[i for i in range(R) if photo[i] == p][int(kept[p, k]) // eng.num_boxes]]
            assert int(classes[p, k]) == int(truth[p][j][4]), (p, k, box, truth[p][j])
            MP.detection_sits_on_marker(box, truth[p][j], row[1][1] / row[0][3], row[1][0] / row[0][2], f"tiled {hw} photo {p} box {k}")
            hit.append(j)
        assert sorted(hit) == list(range(len(truth[p]))), (p, hit)         # every marker exactly once
