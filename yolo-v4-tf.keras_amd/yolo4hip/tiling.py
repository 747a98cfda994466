"""Host geometry of tiled (sliced) inference -- `Engine.predict_tiled`: which windows a photo is cut into, where each window goes
on the network canvas, and the map that takes a window's canvas-normalised boxes to the photo's normalised coordinates.  Pure
NumPy / Python; importable without a GPU.

A photo larger than the network input is cut into overlapping full-size windows at native resolution; each window is one row of
the network batch (`y4_window_u8_ragged`), and all rows of a photo share ONE NMS in the photo's coordinates (`y4_decode_gather`,
`y4_nms_gathered`), so an object two windows see comes back once.

`view_rows` puts any of these rows under (scale, flip) views for test-time augmentation (`Engine.predict_tta`,
`y4_view_u8_ragged`, `y4_decode_gather_views`): the row's rectangle shrunk about its centre, the canvas mirrored, the map mirrored
with it."""
import math

import numpy as np

from . import prepost


def window_starts(L, t, overlap):
    """Start coordinates of the windows of length t along a side of length L: [0] when the side fits one window; otherwise
    0, step, 2 step, ... while below L - t, then L - t, with step = max(1, floor(t * (1 - overlap))).  Every window is full-size
    and inside the side, the last one is flush with the edge, neighbours share at least floor(t * overlap) pixels."""
    L, t = int(L), int(t)
    if L < 1 or t < 1:
        raise ValueError(f"window_starts: side {L} and window {t} must be positive")
    if not 0 <= overlap < 1:                      # (NaN fails too)
        raise ValueError(f"window_starts: overlap must be in [0, 1), got {overlap}")
    if L <= t:
        return [0]
    step = max(1, int(math.floor(t * (1.0 - float(overlap)))))
    starts = list(range(0, L - t, step))
    starts.append(L - t)
    return starts


def tile_windows(h, w, tile_hw, overlap):
    """The windows (y0, x0, wh, ww) of an h x w photo for tiles of tile_hw = (th, tw), row-major; wh = min(th, h), ww = min(tw, w)."""
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    wh, ww = min(th, int(h)), min(tw, int(w))
    return [(y0, x0, wh, ww) for y0 in window_starts(h, th, overlap) for x0 in window_starts(w, tw, overlap)]


def window_map(h, w, H, W, window, rect):
    """float32 (ax, bx, ay, by): canvas-normalised -> photo-normalised for `window` = (y0, x0, wh, ww) of an h x w photo placed at
    rect = (out_h, out_w, pad_top, pad_left) of an H x W canvas.  Computed in float64 and rounded once, like prepost.box_map."""
    y0, x0, wh, ww = (int(v) for v in window)
    out_h, out_w, top, left = (int(v) for v in rect)
    return np.array([(W / out_w) * ww / w, (x0 - left * ww / out_w) / w,
                     (H / out_h) * wh / h, (y0 - top * wh / out_h) / h], dtype=np.float64).astype(np.float32)


def tile_rows(h, w, canvas_hw, tile_hw=None, overlap=0.2, full_image=True, letterbox=False):
    """The network rows of one h x w photo -> a list of (window, rect, map): window = (y0, x0, wh, ww) in photo pixels, rect =
    (out_h, out_w, pad_top, pad_left) where it goes on the H x W canvas -- the whole canvas for stretch, prepost.letterbox_rect of
    the window for letterbox --, map = `window_map`.  tile_hw=None: the canvas size, so that windows inside a photo at least that
    large are 1:1 copies.  full_image=True appends the whole photo as the last row, through the ordinary preprocessing of the
    facade (stretch or letterbox of the photo): its map is prepost.box_map exactly."""
    h, w = int(h), int(w)
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    if h < 1 or w < 1:
        raise ValueError(f"tile_rows: photo {h} x {w}")
    th, tw = (H, W) if tile_hw is None else (int(tile_hw[0]), int(tile_hw[1]))
    if th < 1 or tw < 1:
        raise ValueError(f"tile_rows: tile {th} x {tw}")
    rows = []
    for win in tile_windows(h, w, (th, tw), overlap):
        rect = prepost.fit_rect(win[2], win[3], H, W, letterbox)
        rows.append((win, rect, window_map(h, w, H, W, win, rect)))
    if full_image:
        rect = prepost.fit_rect(h, w, H, W, letterbox)
        rows.append(((0, 0, h, w), rect, prepost.box_map(h, w, H, W, rect)))
    return rows


# ---------------------------------------------------------------------------------------------- views (test-time augmentation)
# A view is (scale, flip): the row's rectangle shrunk about its own centre by `scale` in (0, 1], and the CANVAS mirrored
# left-right ('lr', bit 0), up-down ('ud', bit 1) or both ('lrud').  (1.0, '') is the row as it was.
FLIP_BITS = {"": 0, "lr": 1, "ud": 2, "lrud": 3}
MAX_VIEWS = 16
DEFAULT_VIEWS = ((1.0, ""), (0.83, "lr"), (0.67, ""))          # YOLOv5's augment=True: the image, 0.83 mirrored, 0.67


def check_views(views):
    """A view list -> [(scale as float, flip bits)], or ValueError: no views, more than MAX_VIEWS, a scale that is not finite or
    not in (0, 1], an unknown flip string, a duplicate."""
    try:
        views = [tuple(v) for v in views]
    except TypeError:
        raise ValueError(f"views must be a list of (scale, flip) pairs, got {views!r}") from None
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"views: {len(views)} views (1..{MAX_VIEWS})")
    out = []
    for v in views:
        if len(v) != 2 or not isinstance(v[1], str) or v[1] not in FLIP_BITS:
            raise ValueError(f"views: {v!r} is not (scale, flip) with flip one of {sorted(FLIP_BITS)}")
        try:
            s = float(v[0])
        except (TypeError, ValueError):
            raise ValueError(f"views: the scale of {v!r} is not a number") from None
        if not (math.isfinite(s) and 0.0 < s <= 1.0):
            raise ValueError(f"views: the scale of {v!r} must be finite and in (0, 1]")
        if (s, FLIP_BITS[v[1]]) in out:
            raise ValueError(f"views: {v!r} occurs twice")
        out.append((s, FLIP_BITS[v[1]]))
    return out


def view_rect(rect, scale):
    """rect = (out_h, out_w, pad_top, pad_left) shrunk about its own centre: out' = max(1, floor(scale * out + 0.5)), pad' = pad +
    (out - out') // 2.  At scale == 1 the rectangle itself."""
    out_h, out_w, top, left = (int(v) for v in rect)
    oh = max(1, int(math.floor(float(scale) * out_h + 0.5)))
    ow = max(1, int(math.floor(float(scale) * out_w + 0.5)))
    return oh, ow, top + (out_h - oh) // 2, left + (out_w - ow) // 2


def view_map(h, w, H, W, window, rect, flip_bits):
    """float32 (ax, bx, ay, by) of a view: `window_map` for the view's rectangle in float64, then under bit 0 (ax, bx) -> (-ax, ax +
    bx) -- the canvas column 1 - x carries what column x carried --, under bit 1 the same for (ay, by); rounded to float32 once."""
    y0, x0, wh, ww = (int(v) for v in window)
    out_h, out_w, top, left = (int(v) for v in rect)
    ax, bx = (W / out_w) * ww / w, (x0 - left * ww / out_w) / w
    ay, by = (H / out_h) * wh / h, (y0 - top * wh / out_h) / h
    if flip_bits & 1:
        ax, bx = -ax, ax + bx
    if flip_bits & 2:
        ay, by = -ay, ay + by
    return np.array([ax, bx, ay, by], dtype=np.float64).astype(np.float32)


def view_rows(rows, views, photo_hw, canvas_hw):
    """The rows of `tile_rows` (any of them: windows or the full image) under every view -> a list of (window, rect', flip bits,
    map') in view-major order: all rows under views[0], then all rows under views[1], ...; a row's slot is its index in the
    list.  rect' = `view_rect`, map' = `view_map`; the view (1.0, '') returns window, rect and map of every row as they were."""
    h, w = int(photo_hw[0]), int(photo_hw[1])
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    out = []
    for scale, bits in check_views(views):
        for window, rect, m in rows:
            if scale == 1.0 and bits == 0:
                out.append((tuple(window), tuple(rect), 0, m))
                continue
            r = view_rect(rect, scale)
            out.append((tuple(window), r, bits, view_map(h, w, H, W, window, r, bits)))
    return out
