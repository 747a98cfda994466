"""Marker photos: the instrument of the labels-follow-pixels tests (tests/test_labels_follow_pixels_cpu.py on the host
restatements, tests/test_gpu_labels_follow_pixels.py on the device).  NumPy / PIL only.

Pixels and boxes travel separately in this project (README.md, Parity); a marker photo makes the boxes readable from the pixels.
It is a uint8 RGB image with background BG = (0, 0, 255) on which every box is a filled axis-aligned rectangle with integer
corners -- the box (x1, y1, x2, y2) fills the pixels [x1, x2) x [y1, y2), sides of at least 12 pixels, rectangles at least 6 pixels
apart -- in ONE flat colour that says who it is: R = R_LEVELS[box index], G = G_LEVELS[class], B = B_LEVELS[photo index].

A bilinear resize of a flat region is flat: wherever both taps of a canvas pixel fall inside a marker the canvas byte is the
marker's colour exactly, so identity is read from the output alone, whatever order `DataGenerator._read` shuffled the boxes into.
A blend is t M + (1 - t) BG with 0 < t < 1 (two markers are never under one 2 x 2 tap footprint, the pad is never blended), and
no such blend is another marker's colour: the blue channel gives t = (255 - B') / (255 - B) >= 155 / 245 = 0.63 for two photos,
while two different green levels differ by a factor of at most 0.45, and the same photo (t = 1) is no blend.
`test_no_blend_is_a_marker_colour` checks that by enumeration.

The three predicates (`row_sits_on_marker`, `visible_markers_are_labelled`, `detection_sits_on_marker`) return figures and raise
AssertionError with the case in the message; the bounds are the blend-zone widths derived in their docstrings."""
import os

import numpy as np

BG = (0, 0, 255)
PAD = 128
R_LEVELS = (24, 48, 72, 96, 160, 184, 208, 232)            # box index   (>= 24 from the background's 0, >= 32 from the pad)
G_LEVELS = (40, 88, 200)                                   # class       (ratios <= 0.45: see the module docstring)
B_LEVELS = (10, 28, 46, 64, 82, 100)                       # photo index (>= 155 from the background's 255)
MIN_SIDE, MIN_GAP = 12, 6
MIN_SPAN = 4                                               # predicate 2: exact-colour pixels on both axes that make a marker visible

_R = {v: i for i, v in enumerate(R_LEVELS)}
_G = {v: i for i, v in enumerate(G_LEVELS)}
_B = {v: i for i, v in enumerate(B_LEVELS)}


def colour_of(photo, box, cls):
    return (R_LEVELS[box], G_LEVELS[cls], B_LEVELS[photo])


def identity_of(colour):
    """(photo index, box index, class) of a marker colour, or None for any other colour."""
    r, g, b = (int(v) for v in colour)
    if r in _R and g in _G and b in _B:
        return _B[b], _R[r], _G[g]
    return None


def make_photo(h, w, photo, seed, n_boxes, min_side=MIN_SIDE, num_classes=3):
    """-> (uint8 [h,w,3], boxes float32 [k,5] (x1, y1, x2, y2, class), k <= n_boxes): seeded rejection sampling; box j has the
    colour colour_of(photo, j, class).  Sides lie in [min_side, max(min_side, side / 2)]."""
    rng = np.random.default_rng([seed, photo, h, w])
    img = np.empty((h, w, 3), np.uint8)
    img[:] = BG
    boxes = []
    for _ in range(400):
        if len(boxes) == min(n_boxes, len(R_LEVELS)):
            break
        bw = int(rng.integers(min_side, max(min_side, w // 2) + 1))
        bh = int(rng.integers(min_side, max(min_side, h // 2) + 1))
        if bw > w or bh > h:
            continue
        x1, y1 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        x2, y2 = x1 + bw, y1 + bh
        if any(x1 < b[2] + MIN_GAP and b[0] < x2 + MIN_GAP and y1 < b[3] + MIN_GAP and b[1] < y2 + MIN_GAP for b in boxes):
            continue
        boxes.append((x1, y1, x2, y2, int(rng.integers(num_classes))))
    for j, (x1, y1, x2, y2, c) in enumerate(boxes):
        img[y1:y2, x1:x2] = colour_of(photo, j, c)
    return img, np.array(boxes, np.float32).reshape(-1, 5)


def write_dataset(folder, sizes, seed, n_boxes=4, min_side=None):
    """PNG marker photos m0.png .. of `sizes` (h, w) in `folder` -> (annotation lines, photos, boxes per photo).  min_side: one
    value or one per photo; None: MIN_SIDE."""
    from PIL import Image
    lines, photos, truth = [], [], []
    for p, (h, w) in enumerate(sizes):
        ms = MIN_SIDE if min_side is None else (min_side[p] if np.ndim(min_side) else min_side)
        img, boxes = make_photo(h, w, p, seed, n_boxes, int(ms))
        Image.fromarray(img).save(os.path.join(str(folder), f"m{p}.png"))
        lines.append(f"m{p}.png " + " ".join(",".join(str(int(v)) for v in b) for b in boxes) + "\n")
        photos.append(img)
        truth.append(boxes)
    return lines, photos, truth


# ------------------------------------------------------------------------------------------------ reading a canvas
def exact_rect(canvas, colour, window=None):
    """The bounding rectangle (x0, y0, x1, y1) in pixel EDGES (x1, y1 exclusive) of the pixels of `canvas` [H,W,3] that have
    exactly `colour`, inside window = (y0, y1, x0, x1) (None: the whole canvas); None when there is none."""
    H, W = canvas.shape[:2]
    wy0, wy1, wx0, wx1 = (0, H, 0, W) if window is None else window
    sub = canvas[wy0:wy1, wx0:wx1]
    hit = (sub == np.asarray(colour, np.uint8)).all(axis=-1)
    if not hit.any():
        return None
    ys, xs = np.nonzero(hit.any(axis=1))[0], np.nonzero(hit.any(axis=0))[0]
    return wx0 + int(xs[0]), wy0 + int(ys[0]), wx0 + int(xs[-1]) + 1, wy0 + int(ys[-1]) + 1


def marker_colours(canvas, window=None):
    """The marker colours that occur in (the window of) a canvas: {colour: exact_rect}."""
    H, W = canvas.shape[:2]
    wy0, wy1, wx0, wx1 = (0, H, 0, W) if window is None else window
    sub = canvas[wy0:wy1, wx0:wx1].reshape(-1, 3)
    if len(sub) == 0:
        return {}
    out = {}
    for c in np.unique(sub, axis=0):
        if identity_of(c) is not None:
            out[tuple(int(v) for v in c)] = exact_rect(canvas, c, window)
    return out


def _centre_pixel(row, H, W):
    return min(int(np.floor((row[1] + row[3]) / 2)), H - 1), min(int(np.floor((row[0] + row[2]) / 2)), W - 1)


def _tile_of(tiles, cy, cx):
    for t in tiles:
        y0, y1, x0, x1 = t["window"]
        if y0 <= cy < y1 and x0 <= cx < x1:
            return t
    return None


def whole_canvas(H, W, sx, sy):
    """The tile list of a canvas that is one image: one window, one scale (out / src per axis)."""
    return [{"window": (0, H, 0, W), "sx": float(sx), "sy": float(sy)}]


# ------------------------------------------------------------------------------------------------ predicate 1
def row_sits_on_marker(canvas, row, tiles, what=""):
    """Predicate 1.  `row` = (x1, y1, x2, y2, cls) on `canvas` uint8 [H,W,3]; `tiles`: dicts {window (y0, y1, x0, x1), sx, sy}
    (`whole_canvas`, or the four of a mosaic); the tile that holds the row's centre governs.
      * the colour at the row's centre pixel is a marker colour, and its class is cls;
      * every pixel whose centre lies at least max(1, s) inside the row on each axis has exactly that colour: canvas pixel x
        reads the source at (x + 0.5) / s - 0.5 and the tap after it, both inside the marker from s / 2 (enlarging) or less than
        one pixel (shrinking) inside the row's edge -- max(1, s) is that blend zone, generously;
      * no pixel of exactly that colour in the tile's window lies more than 1 pixel outside the row (a tap weight that rounds
        to zero gives at most a fraction of a pixel).
    -> (colour, interior pixels checked, overshoot in pixels)."""
    H, W = canvas.shape[:2]
    x1, y1, x2, y2 = (float(v) for v in row[:4])
    cy, cx = _centre_pixel(row, H, W)
    tile = _tile_of(tiles, cy, cx)
    assert tile is not None, f"{what}: the centre ({cx}, {cy}) of row {list(row)} lies in no tile window"
    colour = tuple(int(v) for v in canvas[cy, cx])
    who = identity_of(colour)
    assert who is not None, f"{what}: row {list(row)}: the colour {colour} at its centre ({cx}, {cy}) is no marker's"
    assert who[2] == int(row[4]), f"{what}: row {list(row)} has class {int(row[4])}, the marker under it {who} has class {who[2]}"
    mx, my = max(1.0, tile["sx"]), max(1.0, tile["sy"])
    xs = np.nonzero((np.arange(W) + 0.5 >= x1 + mx) & (np.arange(W) + 0.5 <= x2 - mx))[0]
    ys = np.nonzero((np.arange(H) + 0.5 >= y1 + my) & (np.arange(H) + 0.5 <= y2 - my))[0]
    checked = 0
    if len(xs) and len(ys):
        inner = canvas[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        same = (inner == np.asarray(colour, np.uint8)).all(axis=-1)
        assert same.all(), f"{what}: row {list(row)}: {int((~same).sum())} of {same.size} interior pixels are not {colour}"
        checked = int(same.size)
    ex0, ey0, ex1, ey1 = exact_rect(canvas, colour, tile["window"])
    over = max(x1 - ex0, ex1 - x2, y1 - ey0, ey1 - y2, 0.0)
    assert over <= 1.0, (f"{what}: row {list(row)}: pixels of {colour} reach ({ex0}, {ey0}, {ex1}, {ey1}) in window "
                         f"{tile['window']}, {over:.2f} px outside the row")
    return colour, checked, over


# ------------------------------------------------------------------------------------------------ predicate 2
def visible_markers_are_labelled(canvas, rows, tiles, what=""):
    """Predicate 2.  Every marker colour whose exact-colour pixels span at least MIN_SPAN pixels on both axes inside a tile
    window has exactly one label row (of `rows` [k,5], zero rows ignored) whose centre lies in that window on that colour.
    -> the number of visible markers."""
    H, W = canvas.shape[:2]
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    rows = rows[(rows[:, 2] - rows[:, 0] > 0) & (rows[:, 3] - rows[:, 1] > 0)]
    centres = [_centre_pixel(r, H, W) for r in rows]
    seen = 0
    for t in tiles:
        y0, y1, x0, x1 = t["window"]
        if y0 >= y1 or x0 >= x1:
            continue
        for colour, (ex0, ey0, ex1, ey1) in marker_colours(canvas, t["window"]).items():
            if ex1 - ex0 < MIN_SPAN or ey1 - ey0 < MIN_SPAN:
                continue
            seen += 1
            owners = [k for k, (cy, cx) in enumerate(centres)
                      if y0 <= cy < y1 and x0 <= cx < x1 and tuple(int(v) for v in canvas[cy, cx]) == colour]
            assert len(owners) == 1, (f"{what}: marker {identity_of(colour)} shows at ({ex0}, {ey0}, {ex1}, {ey1}) in window "
                                      f"{t['window']} and {len(owners)} label rows have their centre on it: {rows[owners].tolist()}")
    return seen


def check_canvas(canvas, rows, tiles, what=""):
    """Predicates 1 (every non-zero row) and 2 on one canvas -> (rows, interior pixels, worst overshoot, visible markers)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    used = rows[(rows[:, 2] - rows[:, 0] > 0) & (rows[:, 3] - rows[:, 1] > 0)]
    pixels, worst = 0, 0.0
    for r in used:
        _, n, over = row_sits_on_marker(canvas, r, tiles, what)
        pixels, worst = pixels + n, max(worst, over)
    return len(used), pixels, worst, visible_markers_are_labelled(canvas, used, tiles, what)


# ------------------------------------------------------------------------------------------------ predicate 3
def iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    inter = max(iw, 0.0) * max(ih, 0.0)
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def detection_bound(sx, sy):
    """Predicate 3's bound per axis in raw pixels: the exact-colour rectangle stops up to one canvas pixel (1 / s raw pixels; one
    raw pixel when enlarging) short of the marker's edge, + 1 for the rounding of pixel edges."""
    return max(1.0, 1.0 / sx) + 1.0, max(1.0, 1.0 / sy) + 1.0


def detection_sits_on_marker(box_px, marker, sx, sy, what="", min_iou=0.5):
    """Predicate 3.  box_px: (x1, y1, x2, y2) in raw-photo pixels; marker: the true (x1, y1, x2, y2, ...); sx, sy: out / src of the
    row that showed it.  Each corner within `detection_bound` of the truth, IoU >= min_iou.
    -> (worst error / bound, IoU)."""
    bx, by = detection_bound(sx, sy)
    err = [abs(float(box_px[k]) - float(marker[k])) / (bx, by)[k % 2] for k in range(4)]
    v = iou([float(x) for x in box_px[:4]], [float(x) for x in marker[:4]])
    assert max(err) <= 1.0, f"{what}: box {np.round(box_px[:4], 2).tolist()} vs marker {list(marker[:4])}: {max(err):.2f} of the bound ({bx:.2f}, {by:.2f}) px"
    assert v >= min_iou, f"{what}: box {np.round(box_px[:4], 2).tolist()} vs marker {list(marker[:4])}: IoU {v:.3f} < {min_iou}"
    return max(err), v


def mapped_rect(rect_px, canvas_hw, m, photo_hw):
    """An exact-colour rectangle in canvas pixel edges -> raw-photo pixels through a map (ax, bx, ay, by) of `prepost.box_map` /
    `tiling.window_map`: normalise by (W, H), `prepost.map_boxes`, times (w, h)."""
    from yolo4hip import prepost
    H, W = canvas_hw
    b = np.array([[rect_px[0] / W, rect_px[1] / H, rect_px[2] / W, rect_px[3] / H]], np.float32)
    out = prepost.map_boxes(b, m)[0].astype(np.float64)
    return out * np.array([photo_hw[1], photo_hw[0], photo_hw[1], photo_hw[0]], np.float64)


def whole_markers(truth, window):
    """The indices of the boxes of `truth` [k,5] that lie wholly inside window = (y0, x0, wh, ww) of their photo."""
    y0, x0, wh, ww = window
    return [j for j, b in enumerate(truth) if b[0] >= x0 and b[1] >= y0 and b[2] <= x0 + ww and b[3] <= y0 + wh]


def place_row(photo, window, rect, canvas_hw, pad=PAD):
    """The host restatement of one network row of tiled inference / preprocessing: the window of the photo resized by
    `prepost.resize_bilinear` to its rect (out_h, out_w, pad_top, pad_left) on a `pad` canvas."""
    from yolo4hip import prepost
    H, W = canvas_hw
    y0, x0, wh, ww = window
    out_h, out_w, top, left = rect
    canvas = np.full((H, W, 3), pad, np.uint8)
    canvas[top:top + out_h, left:left + out_w] = prepost.resize_bilinear(np.ascontiguousarray(photo[y0:y0 + wh, x0:x0 + ww]),
                                                                         (out_w, out_h))
    return canvas


# ------------------------------------------------------------------------------------------------ tile lists of the training paths
def augment_tiles(param, size_hw, canvas_hw):
    """The tile list of a single-image augmentation row (augment.PARAM_DTYPE) of an h x w photo."""
    return whole_canvas(canvas_hw[0], canvas_hw[1], int(param["out_w"]) / size_hw[1], int(param["out_h"]) / size_hw[0])


def mosaic_tiles(params4, sizes4, cut, canvas_hw):
    """The tile list of a mosaic canvas: the four windows of `augment.tile_windows`, each with the scale of its own row."""
    from yolo4hip.augment import tile_windows
    return [{"window": win, "sx": int(p["out_w"]) / hw[1], "sy": int(p["out_h"]) / hw[0]}
            for win, p, hw in zip(tile_windows(cut, canvas_hw), params4, sizes4)]


# ------------------------------------------------------------------------------------------------ a detector that boxes every marker
def _logit(p):
    return float(np.log(p / (1.0 - p)))


def heads_for_rects(per_image, canvas_hw, num_classes, anchors, xyscale, strides=(8, 16, 32)):
    """The inverse of the inference decode.  per_image: for each image a list of ((x0, y0, x1, y1) in canvas pixels, class) ->
    (three float32 heads [n, gh, gw, 3 (5 + C)], slots: per image a list of (scale, gy, gx, anchor)).  The cell is the one that
    holds the centre, t_xy the logit of ((c / stride - cell) + (xyscale - 1) / 2) / xyscale, t_wh = log(side / anchor), objectness
    and the class logit 8, every other logit -20 (decode_nms_cases._heads_with).  A box goes to the first (scale, anchor) whose
    cell is still free."""
    H, W = canvas_hw
    n, nf = len(per_image), 5 + num_classes
    anchors = np.asarray(anchors, np.float64).reshape(3, 3, 2)
    heads = [np.full((n, H // s, W // s, 3, nf), -20.0, np.float32) for s in strides]
    for h in heads:
        h[..., :4] = 0.0
    slots = []
    for b, rects in enumerate(per_image):
        taken, mine = set(), []
        for (x0, y0, x1, y1), cls in rects:
            cx, cy, bw, bh = (x0 + x1) / 2.0, (y0 + y1) / 2.0, float(x1 - x0), float(y1 - y0)
            for s in range(3):
                gx, gy = int(cx // strides[s]), int(cy // strides[s])
                free = [a for a in range(3) if (s, gy, gx, a) not in taken]
                if free:
                    a = free[0]
                    break
            else:
                raise AssertionError(f"image {b}: no free cell for the box at ({cx}, {cy})")
            taken.add((s, gy, gx, a))
            mine.append((s, gy, gx, a))
            k = float(xyscale[s])
            cell = heads[s][b, gy, gx, a]
            cell[0] = _logit(((cx / strides[s] - gx) + 0.5 * (k - 1.0)) / k)
            cell[1] = _logit(((cy / strides[s] - gy) + 0.5 * (k - 1.0)) / k)
            cell[2], cell[3] = np.log(bw / anchors[s, a, 0]), np.log(bh / anchors[s, a, 1])
            cell[4] = 8.0
            cell[5 + int(cls)] = 8.0
        slots.append(mine)
    return [h.reshape(n, h.shape[1], h.shape[2], 3 * nf) for h in heads], slots


def oracle_boxes(heads, slots, num_classes, anchors, xyscale, strides=(8, 16, 32)):
    """oracle.decode_nms.get_boxes on `heads` at `slots` -> per image a list of (x1, y1, x2, y2) in canvas pixels.  The oracle's
    grid is square: a rectangular head is laid into the top-left of a square one of its longer side (a cell's box depends on its
    own row, column, logits, anchor and stride alone)."""
    from oracle import decode_nms as OD
    anchors = np.asarray(anchors, np.float32).reshape(3, 3, 2)
    decoded = []
    for s in range(3):
        n, gh, gw, _ = heads[s].shape
        g = max(gh, gw)
        sq = np.full((n, g, g, heads[s].shape[3]), -20.0, np.float32)
        sq[:, :gh, :gw] = heads[s]
        decoded.append(OD.get_boxes(sq, anchors[s], num_classes, g, strides[s], xyscale[s])[0])
    return [[decoded[s][b, gy, gx, a] for s, gy, gx, a in mine] for b, mine in enumerate(slots)]


def detect_markers(canvases, truth_of, canvas_hw, num_classes, anchors, xyscale, accept=None):
    """The stand-in detector: for every canvas uint8 [H,W,3] the exact-colour bounding rectangle of every marker on it, as heads.
    truth_of(photo index) -> that photo's boxes [k,5] (the class is checked against the colour); accept(image, photo, box) -> bool
    filters (None: every marker).  -> (heads, slots, found: per image a list of (photo, box, class, rect))."""
    per_image, found = [], []
    for i, canvas in enumerate(canvases):
        rects, mine = [], []
        for colour, rect in sorted(marker_colours(canvas).items()):
            p, j, c = identity_of(colour)
            if accept is not None and not accept(i, p, j):
                continue
            assert int(truth_of(p)[j][4]) == c, (i, p, j, c)
            rects.append((rect, c))
            mine.append((p, j, c, rect))
        per_image.append(rects)
        found.append(mine)
    heads, slots = heads_for_rects(per_image, canvas_hw, num_classes, anchors, xyscale)
    return heads, slots, found
