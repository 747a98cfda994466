"""Labels follow pixels, on the host restatements (no GPU): the three predicates of tests/marker_photos.py on `DataGenerator`'s
plain stretch, `augment_host` + `transform_boxes`, `mosaic_host` + `mosaic_boxes`, and the rows of `tiling.tile_rows` /
`prepost.letterbox` with their maps.  The byte-identity tests pin each strand on its own; these pin that the strands agree:
a flip mirrored in the pixels and not in the boxes, two tiles exchanged, an image of a ragged batch scaled by its neighbour's
size, H and W exchanged on a rectangular canvas all fail here.

The case builders below are shared with tests/test_gpu_labels_follow_pixels.py, which sends the same seeded cases through the
device entry points; every bound is established here first.  Measured figures go to profiles/labels_follow_pixels/measured.json
beside their bounds."""
import json
import os

import numpy as np
import pytest

import marker_photos as MP
from helpers import CLASS_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = os.path.join(CLASS_DIR, "bccd_classes.txt")                       # 3 classes
CANVASES = [(96, 160), (160, 96), (128, 128)]
SIZES = [(60, 90), (200, 150), (96, 160), (300, 400), (130, 75), (48, 220)]     # (h, w): on both sides of every canvas side
EVAL_SIZES = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 80)]           # the five photos of fit and evaluate_map
EVAL_CANVASES = [(96, 160), (160, 160)]
SEED = 20
TILED_PHOTOS = [(200, 260), (96, 120)]                                    # tests/tiled_cases.py's sizes


def note(key, value):
    path = os.path.join(ROOT, "profiles", "labels_follow_pixels", "measured.json")
    try:
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
    except OSError:
        pass                                                               # a read-only checkout: the figures are printed


# ------------------------------------------------------------------------------------------------ the seeded cases
def dataset(folder, sizes=SIZES, seed=SEED, min_side=None):
    """-> {lines, photos, truth, folder}: marker photos of `sizes` written as PNG."""
    lines, photos, truth = MP.write_dataset(folder, sizes, seed, n_boxes=4, min_side=min_side)
    assert all(len(t) >= 1 for t in truth) and sum(len(t) for t in truth) >= 2 * len(sizes)
    return {"lines": lines, "photos": photos, "truth": truth, "folder": str(folder), "sizes": list(sizes)}


def eval_dataset(folder):
    """The five photos of the fit and evaluate_map cases.  Their markers are at least max(20, short side / 4) pixels: the
    exact-colour rectangle stops up to 1 / s raw pixels short of each edge, and that must leave IoU 0.75 (established by
    `test_eval_markers_keep_iou_075`)."""
    return dataset(folder, EVAL_SIZES, SEED + 1, min_side=[max(20, min(h, w) // 4) for h, w in EVAL_SIZES])


def generator(ds, canvas_hw, batch_size, augment=None, seed=None, shuffle=False):
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    return DataGenerator(ds["lines"], NAMES, ds["folder"], shuffle=shuffle, config=make_config(canvas_hw, batch_size=batch_size),
                         augment=augment, seed=seed)


def geometric(**kw):
    """AugmentConfig with the colour factors at hue 0, sat 1, val 1 (the HSV rule is covered elsewhere), the rest default."""
    from yolo4hip.augment import AugmentConfig
    return AugmentConfig(hue=0.0, sat=1.0, val=1.0, **kw)


def forced_augment_rows(H, W):
    """Five rows nobody has to wait for a seed to draw: a flip, a rectangle larger than the canvas (with and without flip), a
    rectangle wholly outside the canvas, and a small one inside."""
    from yolo4hip.augment import PARAM_DTYPE
    rows = [(H // 2 + 7, W - 9, 5, 6, 1), (2 * H + 3, 2 * W - 5, -H // 2 - 1, -W // 3, 0), (H + 40, W + 64, -33, -50, 1),
            (H // 2, W // 2, H + 2, -W, 0), (H // 3 + 1, W // 3 + 2, H // 2, W // 2, 0)]
    out = np.zeros(len(rows), PARAM_DTYPE)
    for p, (oh, ow, top, left, flip) in zip(out, rows):
        p["out_h"], p["out_w"], p["pad_top"], p["pad_left"], p["flip"] = oh, ow, top, left, flip
        p["hue"], p["sat"], p["val"] = 0.0, 1.0, 1.0
    return out


def augment_batches(ds, canvas_hw, passes=3):
    """-> a list of batches (images, params [n], boxes [n, max_boxes, 5]): `passes` epochs of `DataGenerator.raw` over the six
    photos in batches of 3 at the default jitter, scale and flip, then one batch of 5 with `forced_augment_rows`."""
    from yolo4hip.augment import transform_boxes
    np.random.seed(SEED)
    gen = generator(ds, canvas_hw, 3, geometric(), seed=SEED)
    out = [gen.raw(i) for _ in range(passes) for i in range(len(gen))]
    rows = forced_augment_rows(*canvas_hw)
    imgs = [ds["photos"][k] for k in (1, 0, 3, 4, 5)]
    truth = [ds["truth"][k] for k in (1, 0, 3, 4, 5)]
    boxes = np.stack([transform_boxes(t, im.shape[:2], p, canvas_hw, 100) for t, im, p in zip(truth, imgs, rows)])
    assert not boxes[3].any() and boxes[[0, 1, 2, 4]].any(axis=(1, 2)).all()          # the row off the canvas has no label left
    out.append((imgs, rows, boxes))
    return out


def forced_mosaic_batch(ds, canvas_hw):
    """Five canvases drawn by `_draw_row` into forced cuts: (0, W / 3), (H / 2, W) and (H, 0) leave tiles with an empty window, (H, W)
    is a single-image canvas (its four rows are one row), the last is an ordinary mosaic; every tile_src names one of the six photos,
    photo 2 serves three canvases and canvas 1 holds its own photo twice.  The seed is one at which no window edge cuts a label row
    down to a sliver narrower than twice its blend zone (about every second seed leaves one): the centre pixel of such a row is
    a blend, which the instrument cannot read -- an input that does not meet predicate 1's condition on the host."""
    from yolo4hip import augment as A
    H, W = canvas_hw
    cfg = geometric(mosaic=1.0)
    rng = np.random.default_rng(SEED + 9)
    cuts = np.array([(0, W // 3), (H // 2, W), (H, W), (H, 0), (H // 2 + 3, W // 2 - 5)], np.int32)
    tile_src = np.array([[0, 2, 4, 1], [2, 5, 2, 3], [3, 3, 3, 3], [1, 0, 2, 5], [4, 4, 0, 2]])
    params = np.zeros((len(cuts), 4), A.PARAM_DTYPE)
    for i, cut in enumerate(cuts):
        if tuple(cut) == (H, W):
            A._draw_row(rng, params[i, 0], H, W, cfg)
            params[i, 1:] = params[i, 0]
        else:
            for q, window in enumerate(A.tile_windows(cut, canvas_hw)):
                A._draw_row(rng, params[i, q], H, W, cfg, window)
    boxes = np.stack([A.mosaic_boxes([ds["truth"][k] for k in tile_src[i]], [ds["photos"][k].shape[:2] for k in tile_src[i]],
                                     params[i], cuts[i], canvas_hw, 100) for i in range(len(cuts))])
    return ds["photos"], tile_src, params, cuts, boxes


def mosaic_batches(ds, canvas_hw, passes=2):
    """-> a list of batches (images, tile_src [n,4], params [n,4], cuts [n,2], boxes): `passes` epochs of
    `DataGenerator.raw_mosaic` with mosaic = 1.0 over the six photos in batches of 3 (partners repeat, the own image comes
    again), then `forced_mosaic_batch`."""
    np.random.seed(SEED + 1)
    gen = generator(ds, canvas_hw, 3, geometric(mosaic=1.0), seed=SEED + 1)
    out = [gen.raw_mosaic(i) for _ in range(passes) for i in range(len(gen))]
    out.append(forced_mosaic_batch(ds, canvas_hw))
    return out


def check_augment_batch(canvases, batch, canvas_hw, what):
    """Predicates 1 and 2 on the canvases of one `augment_batches` batch -> (rows, interior pixels, overshoot, markers)."""
    imgs, params, boxes = batch
    tot = np.zeros(4)
    for i, canvas in enumerate(canvases):
        r = MP.check_canvas(canvas, boxes[i], MP.augment_tiles(params[i], imgs[i].shape[:2], canvas_hw), f"{what} image {i}")
        tot = [tot[0] + r[0], tot[1] + r[1], max(tot[2], r[2]), tot[3] + r[3]]
    return tot


def check_mosaic_batch(canvases, batch, canvas_hw, what):
    imgs, tile_src, params, cuts, boxes = batch
    tot = np.zeros(4)
    for i, canvas in enumerate(canvases):
        tiles = MP.mosaic_tiles(params[i], [imgs[k].shape[:2] for k in tile_src[i]], cuts[i], canvas_hw)
        r = MP.check_canvas(canvas, boxes[i], tiles, f"{what} canvas {i} cut {tuple(cuts[i])}")
        tot = [tot[0] + r[0], tot[1] + r[1], max(tot[2], r[2]), tot[3] + r[3]]
    return tot


def inference_rows(ds, canvas_hw, letterbox, photos=None, overlap=0.2):
    """-> per photo the rows (window, rect, map) of `tiling.tile_rows(..., full_image=True)`."""
    from yolo4hip import tiling
    return [tiling.tile_rows(h, w, canvas_hw, None, overlap, True, letterbox)
            for h, w in (ds["sizes"] if photos is None else photos)]


def check_inference_row(canvas, row, truth, photo_hw, canvas_hw, what, photo, min_iou=0.5):
    """Predicate 3 on one row's canvas (of photo index `photo`) for every marker wholly inside its window
    -> [(error / bound, IoU, box index)]."""
    window, rect, m = row
    sx, sy = rect[1] / window[3], rect[0] / window[2]
    out = []
    for j in MP.whole_markers(truth, window):
        ex = MP.exact_rect(canvas, MP.colour_of(photo, j, int(truth[j][4])))
        assert ex is not None, f"{what}: marker {j} {list(truth[j])} is wholly inside window {window} and not on the canvas"
        box = MP.mapped_rect(ex, canvas_hw, m, photo_hw)
        e, v = MP.detection_sits_on_marker(box, truth[j], sx, sy, f"{what} window {window} marker {j}", min_iou)
        out.append((e, v, j))
    return out


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    return dataset(tmp_path_factory.mktemp("markers"))


@pytest.fixture(scope="module")
def eval_ds(tmp_path_factory):
    return eval_dataset(tmp_path_factory.mktemp("eval_markers"))


# ------------------------------------------------------------------------------------------------ the instrument itself
def test_no_blend_is_a_marker_colour():
    """t M + (1 - t) BG, rounded either way, is no OTHER marker's colour for any t in (0, 1): an exact marker colour on a canvas
    is that marker.  All pairs of the palette, by the blue channel's t."""
    pal = np.array([(r, g, b) for r in MP.R_LEVELS for g in MP.G_LEVELS for b in MP.B_LEVELS], np.float64)
    bg = np.array(MP.BG, np.float64)
    assert all(abs(v - 128) >= 28 for v in MP.R_LEVELS + MP.G_LEVELS + MP.B_LEVELS)
    for m in pal:
        later = pal[pal[:, 2] > m[2]]                                       # 255 - B' = t (255 - B), t < 1
        t = (255.0 - later[:, 2]) / (255.0 - m[2])
        for dt in (-1.0, 0.0, 1.0):                                         # the blue byte itself may be a rounding off
            blend = (t + dt / (255.0 - m[2]))[:, None] * (m - bg) + bg
            assert (np.abs(blend[:, :2] - later[:, :2]).max(axis=1) > 2.0).all()
    img, boxes = MP.make_photo(90, 140, 2, 5, 4)
    assert len(boxes) == 4 and (boxes[:, 2] - boxes[:, 0] >= 12).all() and (boxes[:, 3] - boxes[:, 1] >= 12).all()
    for j, b in enumerate(boxes):
        x1, y1, x2, y2, c = (int(v) for v in b)
        assert MP.exact_rect(img, MP.colour_of(2, j, c)) == (x1, y1, x2, y2)
        grown = (x1 - 5.5, y1 - 5.5, x2 + 5.5, y2 + 5.5)                    # at least 6 pixels apart
        assert all(MP.iou(grown, [float(v) for v in o[:4]]) == 0 for k, o in enumerate(boxes) if k != j)
    assert MP.identity_of(MP.BG) is None and MP.identity_of((MP.PAD,) * 3) is None


def test_png_round_trip_is_lossless(ds):
    from yolo4hip import prepost
    for p, img in enumerate(ds["photos"]):
        assert np.array_equal(prepost.imread_rgb(os.path.join(ds["folder"], f"m{p}.png")), img)
        assert img.shape[:2] == SIZES[p]


def test_inverse_decode_reproduces_the_rectangles():
    """`heads_for_rects` against oracle/decode_nms.py: the oracle's decode of the crafted heads gives the rectangles to 1e-3 px,
    on the square and the rectangular canvas, cells shared by several boxes included."""
    from yolo4hip.config import make_config
    rng = np.random.default_rng(3)
    for hw in EVAL_CANVASES:
        cfg = make_config(hw)
        H, W = hw
        per_image = []
        for _ in range(3):
            rects = []
            for _ in range(6):
                x0, y0 = int(rng.integers(0, W - 13)), int(rng.integers(0, H - 13))
                rects.append(((x0, y0, int(rng.integers(x0 + 4, W + 1)), int(rng.integers(y0 + 4, H + 1))), int(rng.integers(3))))
            rects += [((0, 0, 5, 4), 1), ((1, 1, 6, 5), 2), ((W - 8, H - 8, W, H), 0), ((2, 0, 7, 6), 0), ((1, 2, 8, 7), 1)]
            per_image.append(rects)
        heads, slots = MP.heads_for_rects(per_image, hw, 3, cfg["anchors"], cfg["xyscale"])
        assert len({s for s in slots[0]}) == len(slots[0]) and len({s[0] for s in slots[0]}) > 1     # a shared cell moved on
        got = MP.oracle_boxes(heads, slots, 3, cfg["anchors"], cfg["xyscale"])
        worst = max(float(np.abs(np.asarray(g, np.float64) - np.asarray(r[0], np.float64)).max())
                    for gi, ri in zip(got, per_image) for g, r in zip(gi, ri))
        print("inverse decode vs the oracle on", hw, ": worst corner error", worst, "px")
        assert worst <= 1e-3


# ------------------------------------------------------------------------------------------------ the training side
@pytest.mark.parametrize("canvas_hw", CANVASES)
def test_plain_stretch(ds, canvas_hw):
    """`DataGenerator.boxes(i)` without augmentation (`get_data`): predicates 1 and 2."""
    H, W = canvas_hw
    np.random.seed(SEED)
    gen = generator(ds, canvas_hw, 4)
    tot, seen = np.zeros(4), 0
    for i in range(len(gen)):
        X, boxes = gen.boxes(i)
        for k in range(len(X)):
            h, w = SIZES[seen]
            canvas = np.rint(X[k] * 255.0).astype(np.uint8)
            r = MP.check_canvas(canvas, boxes[k], MP.whole_canvas(H, W, W / w, H / h), f"stretch {canvas_hw} photo {seen}")
            assert r[0] == r[3] == len(ds["truth"][seen])                   # every box of the photo, once
            tot = [tot[0] + r[0], tot[1] + r[1], max(tot[2], r[2]), tot[3] + r[3]]
            seen += 1
    assert seen == len(SIZES)
    note(f"stretch_{H}x{W}", {"rows": int(tot[0]), "interior_pixels": int(tot[1]), "worst_overshoot_px": tot[2], "overshoot_bound_px": 1.0})


@pytest.mark.parametrize("canvas_hw", CANVASES)
def test_augmentation(ds, canvas_hw):
    """`DataGenerator.raw(i)` with `augment_host`, the forced rows, and `boxes(i)` of a twin generator: predicates 1 and 2."""
    from yolo4hip.augment import augment_host
    H, W = canvas_hw
    batches = augment_batches(ds, canvas_hw)
    tot = np.zeros(4)
    for b, batch in enumerate(batches):
        canvases = [augment_host(img, p, canvas_hw, MP.PAD) for img, p in zip(batch[0], batch[1])]
        r = check_augment_batch(canvases, batch, canvas_hw, f"augment {canvas_hw} batch {b}")
        tot = [tot[0] + r[0], tot[1] + r[1], max(tot[2], r[2]), tot[3] + r[3]]
    params = np.concatenate([b[1] for b in batches[:-1]])
    assert params["flip"].any() and not params["flip"].all()
    assert (params["out_w"] > W).any() and (params["out_w"] < W).any() and (params["pad_left"] < 0).any()
    assert tot[0] >= 40 and tot[1] >= 2000
    print(f"augment {canvas_hw}: rows {tot[0]}, interior pixels {tot[1]}, worst overshoot {tot[2]:.3f} px, visible markers {tot[3]}")
    note(f"augment_{H}x{W}", {"rows": int(tot[0]), "interior_pixels": int(tot[1]), "worst_overshoot_px": tot[2], "overshoot_bound_px": 1.0})
    # boxes(i): the same draws through the generator's own host path
    np.random.seed(SEED)
    twin = generator(ds, canvas_hw, 3, geometric(), seed=SEED)
    for i in range(len(twin)):
        X, boxes = twin.boxes(i)
        assert np.array_equal(boxes, batches[i][2])
        canvases = np.rint(X * 255.0).astype(np.uint8)
        check_augment_batch(canvases, batches[i], canvas_hw, f"augment boxes({i}) {canvas_hw}")


@pytest.mark.parametrize("canvas_hw", CANVASES)
def test_mosaic(ds, canvas_hw):
    """`raw_mosaic(i)` with `mosaic_host` at mosaic = 1.0 over six photos, and the forced cuts: predicates 1 and 2 per tile window."""
    from yolo4hip.augment import mosaic_host
    H, W = canvas_hw
    batches = mosaic_batches(ds, canvas_hw)
    tot = np.zeros(4)
    for b, (imgs, tile_src, params, cuts, boxes) in enumerate(batches):
        assert (boxes[:, -1] == 0).all()                                    # no case reaches max_boxes
        canvases = [mosaic_host([imgs[k] for k in tile_src[i]], params[i], cuts[i], canvas_hw, MP.PAD) for i in range(len(cuts))]
        r = check_mosaic_batch(canvases, (imgs, tile_src, params, cuts, boxes), canvas_hw, f"mosaic {canvas_hw} batch {b}")
        tot = [tot[0] + r[0], tot[1] + r[1], max(tot[2], r[2]), tot[3] + r[3]]
    src = np.concatenate([b[1] for b in batches[:-1]])
    assert any(len(set(row.tolist())) < 4 for row in src)                   # a photo twice on one canvas
    assert any(len(b[0]) < 12 for b in batches[:-1])                        # partners repeat: fewer distinct photos than tiles
    assert tot[0] >= 60 and tot[1] >= 1500
    print(f"mosaic {canvas_hw}: rows {tot[0]}, interior pixels {tot[1]}, worst overshoot {tot[2]:.3f} px, visible markers {tot[3]}")
    note(f"mosaic_{H}x{W}", {"rows": int(tot[0]), "interior_pixels": int(tot[1]), "worst_overshoot_px": tot[2], "overshoot_bound_px": 1.0})


def test_mosaic_boxes_path_of_the_generator(ds):
    """`boxes(i)` of a mosaic generator (its own `mosaic_host` call) gives the canvases and boxes of `raw_mosaic(i)`."""
    canvas_hw = CANVASES[0]
    batches = mosaic_batches(ds, canvas_hw, passes=1)
    np.random.seed(SEED + 1)
    twin = generator(ds, canvas_hw, 3, geometric(mosaic=1.0), seed=SEED + 1)
    for i in range(len(twin)):
        X, boxes = twin.boxes(i)
        assert np.array_equal(boxes, batches[i][4])
        check_mosaic_batch(np.rint(X * 255.0).astype(np.uint8), batches[i], canvas_hw, f"mosaic boxes({i})")


# ------------------------------------------------------------------------------------------------ the inference side
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("canvas_hw", CANVASES)
def test_inference_rows(ds, canvas_hw, letterbox):
    """Every row of `tiling.tile_rows(..., full_image=True)` placed by `resize_bilinear` at its rect: predicate 3 through the
    row's map, for every marker wholly inside the window."""
    H, W = canvas_hw
    worst, low, count, windows = 0.0, 1.0, 0, 0
    for p, rows in enumerate(inference_rows(ds, canvas_hw, letterbox)):
        covered = set()
        for row in rows:
            canvas = MP.place_row(ds["photos"][p], row[0], row[1], canvas_hw)
            res = check_inference_row(canvas, row, ds["truth"][p], SIZES[p], canvas_hw, f"{canvas_hw} lb={letterbox} photo {p}", p)
            covered |= {j for _, _, j in res}
            for e, v, _ in res:
                worst, low, count = max(worst, e), min(low, v), count + 1
            windows += 1
        assert covered == set(range(len(ds["truth"][p])))                   # the full image shows every marker
    assert windows > 2 * len(SIZES) and count >= 40
    print(f"inference rows {canvas_hw} letterbox={letterbox}: {count} markers in {windows} rows, worst error / bound {worst:.3f}, smallest IoU {low:.3f}")
    note(f"inference_{'letterbox' if letterbox else 'stretch'}_{H}x{W}",
         {"markers": count, "worst_error_over_bound": worst, "bound": "max(1, 1/s) + 1 raw px", "smallest_iou": low, "iou_bound": 0.5})


@pytest.mark.parametrize("canvas_hw", CANVASES)
def test_letterbox_with_box_map(ds, canvas_hw):
    """`prepost.letterbox` with `prepost.box_map`: predicate 3."""
    from yolo4hip import prepost
    H, W = canvas_hw
    for p, photo in enumerate(ds["photos"]):
        h, w = photo.shape[:2]
        canvas = prepost.letterbox(photo, canvas_hw, MP.PAD)
        rect = prepost.letterbox_rect(h, w, H, W)
        res = check_inference_row(canvas, ((0, 0, h, w), rect, prepost.box_map(h, w, H, W)), ds["truth"][p], (h, w), canvas_hw,
                                  f"letterbox {canvas_hw} photo {p}", p)
        assert len(res) == len(ds["truth"][p])


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("canvas_hw", EVAL_CANVASES)
def test_eval_markers_keep_iou_075(eval_ds, canvas_hw, letterbox):
    """The case set of the device's evaluate_map test: on the whole photo, stretched or letterboxed, every marker's mapped
    exact-colour rectangle has IoU >= 0.75 with the marker (so a detector that boxes the exact pixels scores mAP 1 at 0.75 too).
    And its negative control's premise: with the canvases rotated by one photo, few boxes meet a marker of their class."""
    from yolo4hip import prepost
    H, W = canvas_hw
    low, boxes = 1.0, []
    for p, photo in enumerate(eval_ds["photos"]):
        h, w = photo.shape[:2]
        rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
        row = ((0, 0, h, w), rect, prepost.box_map(h, w, H, W, rect))
        res = check_inference_row(MP.place_row(photo, *row[:2], canvas_hw), row, eval_ds["truth"][p], (h, w), canvas_hw,
                                  f"eval {canvas_hw} lb={letterbox} photo {p}", p, min_iou=0.75)
        assert len(res) == len(eval_ds["truth"][p])
        low = min([low] + [v for _, v, _ in res])
        # the same rectangles, as the rotated control pairs them: photo p's canvas geometry, photo p + 1's markers
        q = (p + 1) % len(eval_ds["photos"])
        other = eval_ds["photos"][q]
        orect = prepost.letterbox_rect(*other.shape[:2], H, W) if letterbox else (H, W, 0, 0)
        ocanvas = MP.place_row(other, (0, 0, *other.shape[:2]), orect, canvas_hw)
        for colour, ex in MP.marker_colours(ocanvas).items():
            boxes.append((p, MP.identity_of(colour)[2], MP.mapped_rect(ex, canvas_hw, row[2], (h, w))))
    hits = sum(any(int(t[4]) == c and MP.iou(list(b), [float(v) for v in t[:4]]) >= 0.5 for t in eval_ds["truth"][p]) for p, c, b in boxes)
    print(f"eval markers {canvas_hw} letterbox={letterbox}: smallest IoU {low:.3f}; rotated by one photo {hits} of {len(boxes)} boxes meet a marker")
    note(f"eval_{'letterbox' if letterbox else 'stretch'}_{H}x{W}", {"smallest_iou": low, "iou_bound": 0.75,
                                                                     "rotated_boxes_that_meet_a_marker": hits, "boxes": len(boxes)})
    assert hits <= 0.25 * len(boxes)


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("canvas_hw", EVAL_CANVASES)
def test_tiled_duplicates_overlap_above_the_nms_threshold(tmp_path_factory, canvas_hw, letterbox):
    """The tiled case of the device test (200 x 260 and 96 x 120, overlap 0.2, full image): predicate 3 on every row, and every
    two sightings of one marker -- overlapping windows, the full image -- have IoU >= 0.7 in the photo, above the NMS threshold
    0.413, while two different markers do not touch (6 pixels apart, error under 6 / 2)."""
    tds = tiled_dataset(tmp_path_factory.mktemp("tiled"))
    low = 1.0
    for p, rows in enumerate(inference_rows(tds, canvas_hw, letterbox)):
        sightings = {}
        for row in rows:
            canvas = MP.place_row(tds["photos"][p], row[0], row[1], canvas_hw)
            for e, v, j in check_inference_row(canvas, row, tds["truth"][p], TILED_PHOTOS[p], canvas_hw, f"tiled {canvas_hw} photo {p}", p):
                ex = MP.exact_rect(canvas, MP.colour_of(p, j, int(tds["truth"][p][j][4])))
                sightings.setdefault(j, []).append(MP.mapped_rect(ex, canvas_hw, row[2], TILED_PHOTOS[p]))
        assert set(sightings) == set(range(len(tds["truth"][p])))
        for j, boxes in sightings.items():
            low = min([low] + [MP.iou(list(a), list(b)) for a in boxes for b in boxes])
            for k, others in sightings.items():
                assert k == j or all(MP.iou(list(a), list(b)) == 0 for a in boxes for b in others)
    print(f"tiled {canvas_hw} letterbox={letterbox}: smallest IoU between two sightings of a marker {low:.3f}")
    note(f"tiled_{'letterbox' if letterbox else 'stretch'}_{canvas_hw[0]}x{canvas_hw[1]}", {"smallest_duplicate_iou": low, "bound": 0.7})
    assert low >= 0.7


def tiled_dataset(folder):
    """The two photos of the tiled case; markers of at least max(20, short side / 5) pixels, so that two sightings of one marker
    overlap with IoU >= 0.7."""
    return dataset(folder, TILED_PHOTOS, SEED + 2, min_side=[max(20, min(h, w) // 5) for h, w in TILED_PHOTOS])


# ------------------------------------------------------------------------------------------------ the cases of fit
# name -> (canvas, augmentation, shuffle, seed): five photos in batches of 3; on the device max_batch = 2 cuts every batch into
# chunks of 2 + 1 and 2.  The seeds are ones whose draws leave no sliver row (see `forced_mosaic_batch`), which
# `test_fit_cases_meet_the_conditions_on_the_host` establishes.
FIT_CASES = {"plain": ((160, 160), None, False, 3), "augment": ((160, 160), {}, False, 3), "mosaic": ((160, 160), {"mosaic": 0.5}, False, 1),
             "shuffle": ((160, 160), {}, True, 4), "mosaic_rect": ((96, 160), {"mosaic": 0.5}, False, 1)}


def fit_generator(eval_ds, name):
    canvas_hw, aug, shuffle, seed = FIT_CASES[name]
    np.random.seed(SEED + seed)
    return generator(eval_ds, canvas_hw, 3, None if aug is None else geometric(**aug), seed=seed, shuffle=shuffle)


def recorded(gen, eval_ds, log):
    """Wrap `raw`, `raw_mosaic` and `boxes` of a generator: every call appends (tiles per canvas, boxes, host canvases or None)
    to `log` and returns what the generator returned.  -> {name: wrapper} for monkeypatch.setattr(gen, name, wrapper)."""
    hw = tuple(gen.target_img_size[:2])
    raw, raw_mosaic, boxes = gen.raw, gen.raw_mosaic, gen.boxes

    def w_raw(i):
        imgs, params, y = raw(i)
        log.append(([MP.augment_tiles(p, im.shape[:2], hw) for p, im in zip(params, imgs)], y, None, (imgs, params)))
        return imgs, params, y

    def w_mosaic(i):
        imgs, src, params, cuts, y = raw_mosaic(i)
        log.append(([MP.mosaic_tiles(params[k], [imgs[j].shape[:2] for j in src[k]], cuts[k], hw) for k in range(len(cuts))], y, None,
                    (imgs, src, params, cuts)))
        return imgs, src, params, cuts, y

    def w_boxes(i):
        if gen.augment is not None:
            return boxes(i)                                                # (goes through raw / raw_mosaic above)
        idxs = gen.indexes[i * gen.batch_size:(i + 1) * gen.batch_size]
        X, y = boxes(i)
        log.append(([MP.whole_canvas(*hw, hw[1] / eval_ds["sizes"][j][1], hw[0] / eval_ds["sizes"][j][0]) for j in idxs], y,
                    np.rint(X * 255.0).astype(np.uint8), None))
        return X, y

    return {"raw": w_raw, "raw_mosaic": w_mosaic, "boxes": w_boxes}


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_cases_meet_the_conditions_on_the_host(eval_ds, name, monkeypatch):
    """One epoch of each fit case through the generator's own host path (`boxes(i)`): predicates 1 and 2 on every canvas."""
    gen = fit_generator(eval_ds, name)
    log = []
    for k, fn in recorded(gen, eval_ds, log).items():
        monkeypatch.setattr(gen, k, fn)
    canvases = [np.rint(gen.boxes(i)[0] * 255.0).astype(np.uint8) for i in range(len(gen))]
    assert len(log) == len(gen) == 2
    rows = images = 0
    for b, ((tiles, boxes, _, _), cv) in enumerate(zip(log, canvases)):
        for k in range(len(cv)):
            rows += MP.check_canvas(cv[k], boxes[k], tiles[k], f"fit case {name} batch {b} image {k}")[0]
            images += 1
    assert images == len(EVAL_SIZES) and rows >= 8
    if name == "shuffle":
        assert gen.indexes.tolist() != sorted(gen.indexes.tolist())
    if name.startswith("mosaic"):
        kinds = [sum(t["window"][0] < t["window"][1] and t["window"][2] < t["window"][3] for t in tiles)
                 for per_canvas, *_ in log for tiles in per_canvas]
        assert 1 in kinds and 4 in kinds                                    # single canvases and mosaics in one epoch
