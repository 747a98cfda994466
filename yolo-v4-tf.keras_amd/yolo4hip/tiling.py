"""Host geometry of tiled (sliced) inference -- `Engine.predict_tiled`: which windows a photo is cut into, where each window goes
on the network canvas, and the map that takes a window's canvas-normalised boxes to the photo's normalised coordinates.  Pure
NumPy / Python; importable without a GPU.

A photo larger than the network input is cut into overlapping full-size windows at native resolution; each window is one row of
the network batch (`y4_window_u8_ragged`), and all rows of a photo share ONE NMS in the photo's coordinates (`y4_decode_gather`,
`y4_nms_gathered`), so an object two windows see comes back once."""
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
        rect = prepost.letterbox_rect(win[2], win[3], H, W) if letterbox else (H, W, 0, 0)
        rows.append((win, rect, window_map(h, w, H, W, win, rect)))
    if full_image:
        rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
        rows.append(((0, 0, h, w), rect, prepost.box_map(h, w, H, W, rect)))
    return rows
