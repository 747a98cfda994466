"""Descriptor tables of the canvas kernels (csrc/canvas_u8.h), built on the host: where a source goes on the network canvas and
where its bytes lie in the one source buffer.  Pure Python / NumPy on the ctypes rows of `ext`: no library, no GPU."""
import math

import numpy as np

from . import prepost


def rect_table(Desc, rects):
    """A zeroed table of `Desc` rows (any descriptor of `ext`), row k placed at rects[k] = (out_h, out_w, pad_top, pad_left)."""
    desc = (Desc * len(rects))()
    for d, rect in zip(desc, rects):
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
    return desc


def fit_table(Desc, sizes, H, W, letterbox):
    """Sources of sizes[k] = (h, w) fitted to an H x W canvas by `prepost.fit_rect` -> (their `rect_table`, float32 [n,4]: the
    `prepost.box_map` of every row)."""
    rects = [prepost.fit_rect(h, w, H, W, letterbox) for h, w in sizes]
    maps = [prepost.box_map(h, w, H, W, rect) for (h, w), rect in zip(sizes, rects)]
    return rect_table(Desc, rects), np.array(maps, np.float32).reshape(-1, 4)


def place_sources(desc, shapes, rows=None, windows=None, place=None):
    """The source fields of the rows of `desc` for uint8 sources of `shapes` packed back to back: row k gets offset, h, w of source k,
    or of source rows[k] (rows may share a source).  With `windows` (one (y0, x0, wh, ww) per row, inside the [h,w,3] image rows[k];
    ValueError otherwise) `desc` holds y4_window_desc rows: offset is the window's first pixel, pitch the image's row, h and w the
    window's.  With `place` the sources are byte buffers of any layout (video frames) and place(row, k, offset) fills the fields.
    -> the offsets [n + 1] of the sources; the last one is the total of source bytes."""
    offs = [0]
    for s in shapes:
        offs.append(offs[-1] + math.prod(s))
    if windows is not None:
        for d, k, (y0, x0, wh, ww) in zip(desc, rows, windows):
            ih, iw = shapes[k][:2]
            if not (0 <= y0 and 0 <= x0 and wh >= 1 and ww >= 1 and y0 + wh <= ih and x0 + ww <= iw):
                raise ValueError(f"window ({y0}, {x0}, {wh}, {ww}) is not inside its {ih} x {iw} image")
            d.offset, d.pitch, d.h, d.w = offs[k] + (y0 * iw + x0) * 3, iw * 3, wh, ww
    else:
        for d, k in zip(desc, range(len(shapes)) if rows is None else rows):
            if place is not None:
                place(d, k, offs[k])
            else:
                d.offset, d.h, d.w = offs[k], shapes[k][0], shapes[k][1]
    return offs
