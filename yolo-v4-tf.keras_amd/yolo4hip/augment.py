"""Training-time augmentation of `Yolov4.fit`: random scale / aspect jitter, shift, left-right flip and an HSV colour
transform (Darknet's YOLOv4 recipe: jitter=.3 hue=.1 saturation=1.5 exposure=1.5 flip=1).  The reference has no augmentation;
the rules below are this project's own.

All randomness is drawn HERE, on the host, from a seeded `numpy.random.Generator` (`draw_params`): one row of parameters per
image.  The image work is then a pure function of that row -- on the device one launch over the batch
(`y4_augment_u8_ragged`, `Engine.augment_u8_batch`), off the device `augment_host`, its NumPy restatement -- and the boxes
follow on the host (`transform_boxes`: 100 rows per image).

Image rule (canvas H x W, parameters out_h, out_w, pad_top, pad_left, flip, hue, sat, val):
  * canvas column x is sourced from column x' = W - 1 - x when flip, else x' = x;
  * with yy = y - pad_top, xx = x' - pad_left: inside [0, out_h) x [0, out_w) the pixel is the uint8 bilinear resize of the image
    to out_w x out_h at (yy, xx) (`prepost.resize_bilinear`, cv2's fixed point), else `pad_value`; the rectangle may stick out of
    the canvas on any side;
  * colour, on resized pixels only, in float32, skipped when (hue, sat, val) == (0, 1, 1): RGB / 255 -> HSV as
    `colorsys.rgb_to_hsv`, H <- H + hue - floor(H + hue), S <- clamp(S sat, 0, 1), V <- clamp(V val, 0, 1), back as
    `colorsys.hsv_to_rgb`, byte = clamp(floor(255 c + 0.5), 0, 255).

Mosaic (AugmentConfig.mosaic > 0) is defined by composition: a canvas has a cut (cut_y, cut_x) and four
tiles q = 0..3 (top-left, top-right, bottom-left, bottom-right), each one parameter row of the rule above; canvas pixel (y, x)
is pixel (y, x) of the single-image augmentation of tile q = 2 (y >= cut_y) + (x >= cut_x) on the whole canvas.
`draw_mosaic_params` draws the rows, `mosaic_host` is np.where over four `augment_host` canvases, `mosaic_boxes` merges the
boxes, and `y4_mosaic_u8_ragged` (`Engine.mosaic_u8_batch`) writes the batch in one launch.
"""
from dataclasses import dataclass

import numpy as np

from . import prepost

# one row per image; the first four fields are the rectangle of y4_image_desc
PARAM_DTYPE = np.dtype([("out_h", np.int32), ("out_w", np.int32), ("pad_top", np.int32), ("pad_left", np.int32),
                        ("flip", np.int32), ("hue", np.float32), ("sat", np.float32), ("val", np.float32)])


@dataclass(frozen=True)
class AugmentConfig:
    """jitter j: the aspect ratio is multiplied by r = U(1-j, 1+j) / U(1-j, 1+j); scale (lo, hi): the rectangle's long side is
    U(lo, hi) of the canvas side; flip: mirror left-right with probability 1/2; hue h: U(-h, h) is added to the hue (a turn is
    1); sat / val s: the factor is U(1, s) or its reciprocal, each with probability 1/2; pad_value: the uint8 level of the
    canvas outside the rectangle.  mosaic: the probability that a canvas is a mosaic of four images (`draw_mosaic_params`), in
    [0, 1]; mosaic_center (lo, hi): the cut of a mosaic is U(lo, hi) of the canvas side, 0 <= lo <= hi <= 1.
    AugmentConfig.identity() changes nothing: the plain stretch of `DataGenerator.get_data`."""
    jitter: float = 0.3
    scale: tuple = (0.25, 2.0)
    flip: bool = True
    hue: float = 0.1
    sat: float = 1.5
    val: float = 1.5
    pad_value: int = 128
    mosaic: float = 0.0
    mosaic_center: tuple = (0.2, 0.8)

    def __post_init__(self):
        lo, hi = (float(v) for v in self.scale)
        if not (0.0 <= self.jitter < 1.0 and 0.0 < lo <= hi and 0.0 <= self.hue <= 1.0 and self.sat >= 1.0 and self.val >= 1.0):
            raise ValueError(f"AugmentConfig: jitter in [0,1), 0 < scale[0] <= scale[1], hue in [0,1], sat >= 1, val >= 1; got {self}")
        if not 0 <= int(self.pad_value) <= 255:
            raise ValueError(f"pad_value must be a uint8 level 0..255, got {self.pad_value}")
        if not 0.0 <= float(self.mosaic) <= 1.0:
            raise ValueError(f"mosaic is a probability in [0,1], got {self.mosaic}")
        if len(self.mosaic_center) != 2 or not 0.0 <= float(self.mosaic_center[0]) <= float(self.mosaic_center[1]) <= 1.0:
            raise ValueError(f"mosaic_center (lo, hi): 0 <= lo <= hi <= 1, got {self.mosaic_center}")

    @classmethod
    def identity(cls, pad_value=128):
        return cls(jitter=0.0, scale=(1.0, 1.0), flip=False, hue=0.0, sat=1.0, val=1.0, pad_value=pad_value)


def draw_params(rng, sizes_hw, canvas_hw, cfg):
    """One row of PARAM_DTYPE per image of `sizes_hw` (only its length matters: the rectangle is relative to the canvas).  Per
    image, in this order, from `rng` (a numpy.random.Generator):
      ja, jb ~ U(1-j, 1+j), r = ja / jb;  s ~ U(scale);
      r < 1: out_h = rint(s H), out_w = rint(s W r);  else: out_w = rint(s W), out_h = rint(s H / r);  both at least 1;
      u, u' ~ U[0,1): pad_left = floor(u (W - out_w)), pad_top = floor(u' (H - out_h))  (negative when the rectangle is larger);
      u'' ~ U[0,1): flip = cfg.flip and u'' < 0.5;  hue ~ U(-cfg.hue, cfg.hue);
      sat: m ~ U(1, cfg.sat), u ~ U[0,1): sat = m if u < 0.5 else 1 / m;  val likewise.
    Every draw is consumed whatever the config, so a seed gives the same stream under every config, and the identity config
    gives exactly (H, W, 0, 0), no flip, (0, 1, 1).  The rounding is `rint`, not keras-yolo3's truncation, for that reason:
    a product that lands a rounding error below an integer loses a whole pixel under truncation and nothing under rint, so
    the identity rectangle does not hang on how s H / r happens to round.
    Ranges: out_h in [max(1, rint(lo H (1-j)/(1+j))), rint(hi H)], out_w likewise with W; pad_left between 0 and W - out_w
    (either sign), pad_top likewise; |hue| <= cfg.hue; sat in [1/cfg.sat, cfg.sat], val in [1/cfg.val, cfg.val]."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    out = np.zeros(len(sizes_hw), dtype=PARAM_DTYPE)
    for p in out:
        _draw_row(rng, p, H, W, cfg)
    return out


def _draw_row(rng, p, H, W, cfg, window=None):
    """One row of `draw_params` into `p`: its draws in its order.  window=None: the position on the whole canvas, as
    `draw_params` states it.  window=(y0, y1, x0, x1) (a mosaic tile): the same u, u' place the VISIBLE rectangle in the window --
    left edge L = x0 + floor(u (x1 - x0 - out_w)), top edge likewise -- and pad_left is L without flip, W - L - out_w with
    flip: the rule mirrors about the whole canvas, which puts a rectangle stored at pad_left on the columns
    [W - pad_left - out_w, W - pad_left)."""
    j, (lo, hi) = float(cfg.jitter), cfg.scale
    ja, jb = rng.uniform(1.0 - j, 1.0 + j), rng.uniform(1.0 - j, 1.0 + j)
    r = ja / jb
    s = rng.uniform(lo, hi)
    if r < 1.0:
        nh, nw = np.rint(s * H), np.rint(s * W * r)
    else:
        nw, nh = np.rint(s * W), np.rint(s * H / r)
    nh, nw = max(1, int(nh)), max(1, int(nw))
    u, v, f = rng.uniform(), rng.uniform(), rng.uniform()
    p["out_h"], p["out_w"] = nh, nw
    p["flip"] = int(bool(cfg.flip) and f < 0.5)
    if window is None:
        p["pad_left"], p["pad_top"] = int(np.floor(u * (W - nw))), int(np.floor(v * (H - nh)))
    else:
        y0, y1, x0, x1 = window
        left = x0 + int(np.floor(u * (x1 - x0 - nw)))
        p["pad_left"], p["pad_top"] = (W - left - nw if p["flip"] else left), y0 + int(np.floor(v * (y1 - y0 - nh)))
    p["hue"] = rng.uniform(-cfg.hue, cfg.hue) + 0.0          # (+ 0.0: U(-0, 0) may be -0.0)
    for name, top in (("sat", cfg.sat), ("val", cfg.val)):
        m, coin = rng.uniform(1.0, top), rng.uniform()
        p[name] = m if coin < 0.5 else 1.0 / m


def tile_windows(cut, canvas_hw):
    """The four windows (y0, y1, x0, x1) of a mosaic canvas, tile order 0..3: top-left, top-right, bottom-left, bottom-right."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    cy, cx = int(cut[0]), int(cut[1])
    return [(0, cy, 0, cx), (0, cy, cx, W), (cy, H, 0, cx), (cy, H, cx, W)]


def draw_mosaic_params(rng, n, dataset_len, canvas_hw, cfg):
    """The draws of n canvases under cfg.mosaic -> (tile_src int64 [n,4]: indices into a dataset of `dataset_len` images, -1
    where the caller puts the canvas's own image -- column 0 always, every column of a single canvas;
    params PARAM_DTYPE [n,4]; cuts int32 [n,2] as (cut_y, cut_x)).  Per canvas, in this order, from `rng`:
      c ~ U[0,1): a mosaic when c < cfg.mosaic, else a single image;
      mosaic: ux, uy ~ U(cfg.mosaic_center): cut_x = rint(ux W), cut_y = rint(uy H);  three partners
              rng.integers(dataset_len) for tiles 1, 2, 3 (with replacement; the own image may come again);  then four rows in
              tile order, each the draws of a `draw_params` row: the size by the jitter and scale rule relative to the CANVAS
              (the object sizes keep the distribution of the single-image path), the position inside the tile's WINDOW by the
              shift rule (`_draw_row`: a rectangle larger than the window covers it and sticks out, a smaller one lies
              inside it on pad), flip, hue, sat, val as there;
      single: the cut is (H, W), row 0 one `draw_params` row on the whole canvas, rows 1..3 copies of it (their windows are
              empty).
    A mosaic canvas consumes 1 + 2 + 3 + 4 x 11 draws, a single one 1 + 11."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    lo, hi = (float(v) for v in cfg.mosaic_center)
    src = np.full((int(n), 4), -1, dtype=np.int64)
    params = np.zeros((int(n), 4), dtype=PARAM_DTYPE)
    cuts = np.zeros((int(n), 2), dtype=np.int32)
    for i in range(int(n)):
        if rng.uniform() < cfg.mosaic:
            ux, uy = rng.uniform(lo, hi), rng.uniform(lo, hi)
            cuts[i] = int(np.rint(uy * H)), int(np.rint(ux * W))
            src[i, 1:] = [int(rng.integers(dataset_len)) for _ in range(3)]
            for q, window in enumerate(tile_windows(cuts[i], (H, W))):
                _draw_row(rng, params[i, q], H, W, cfg, window)
        else:
            cuts[i] = H, W
            _draw_row(rng, params[i, 0], H, W, cfg)
            params[i, 1:] = params[i, 0]
    return src, params, cuts


def transform_boxes(raw_boxes, size_hw, param, canvas_hw, max_boxes):
    """Boxes [k,5] (x1, y1, x2, y2, class) in the pixels of an h x w image -> float32 [max_boxes,5] on the augmented canvas:
    x sx + pad_left, y sy + pad_top in float64, with flip x1, x2 <- W - x2, W - x1, clipped to [0,W] x [0,H]; rows whose width
    or height is then <= 1 are dropped, the survivors compacted to a prefix in their order, the rest zero, one cast to float32.
    sx = out_w / w and sy = out_h / h are rounded to float32 first, as the float32 product of `DataGenerator.get_data` has
    them: an identity row then gives get_data's boxes bit for bit (the product of two float32 values is exact in float64)."""
    h, w = size_hw
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    out = np.zeros((int(max_boxes), 5), dtype=np.float32)
    b = np.asarray(raw_boxes, dtype=np.float64).reshape(-1, 5)[:int(max_boxes)].copy()
    if len(b) == 0:
        return out
    sx, sy = float(np.float32(int(param["out_w"]) / w)), float(np.float32(int(param["out_h"]) / h))
    b[:, [0, 2]] = b[:, [0, 2]] * sx + int(param["pad_left"])
    b[:, [1, 3]] = b[:, [1, 3]] * sy + int(param["pad_top"])
    if param["flip"]:
        b[:, [0, 2]] = W - b[:, [2, 0]]
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0.0, W)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0.0, H)
    keep = b[(b[:, 2] - b[:, 0] > 1.0) & (b[:, 3] - b[:, 1] > 1.0)]
    out[:len(keep)] = keep
    return out


def hsv_shift_u8(rgb, hue, sat, val):
    """The colour rule on uint8 [..., 3], float32 arithmetic in the kernel's order of operations (csrc/canvas_u8.hip: hsv_px_u8)."""
    f32 = np.float32
    hue, sat, val = f32(hue), f32(sat), f32(val)
    if hue == 0 and sat == 1 and val == 1:
        return np.asarray(rgb, dtype=np.uint8).copy()
    c = np.asarray(rgb, dtype=np.uint8).astype(f32) / f32(255.0)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    rng_ = maxc - minc
    grey = rng_ == 0
    safe = np.where(grey, f32(1.0), rng_)
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, f32(2.0) + rc - bc, f32(4.0) + gc - rc)) / f32(6.0)
    h = h - np.floor(h)
    h = np.where(grey, f32(0.0), h)
    s = np.where(grey, f32(0.0), rng_ / np.where(maxc == 0, f32(1.0), maxc))
    h = h + hue
    h = h - np.floor(h)
    s = np.minimum(np.maximum(s * sat, f32(0.0)), f32(1.0))
    v = np.minimum(np.maximum(maxc * val, f32(0.0)), f32(1.0))
    h6 = h * f32(6.0)
    i = h6.astype(np.int32)
    f = h6 - i.astype(f32)
    p, q, t = v * (f32(1.0) - s), v * (f32(1.0) - s * f), v * (f32(1.0) - s * (f32(1.0) - f))
    i = i % 6
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], axis=-1)
    out = np.where((s == 0)[..., None], v[..., None], out)
    return np.clip(np.floor(f32(255.0) * out + f32(0.5)), 0, 255).astype(np.uint8)


def augment_host(img, param, canvas_hw, pad_value=128):
    """uint8 [h,w,3] -> the augmented uint8 canvas [H,W,3]: the NumPy restatement of y4_augment_u8_ragged for one image (the
    geometry is integer arithmetic, byte-identical to the device; the colour agrees to a float32 rounding).  Only the visible
    part of the rectangle is coloured."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    out_h, out_w, top, left = (int(param[k]) for k in ("out_h", "out_w", "pad_top", "pad_left"))
    canvas = np.full((H, W, 3), pad_value, dtype=np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(top + out_h, H), max(left, 0), min(left + out_w, W)
    if y0 < y1 and x0 < x1:
        rect = prepost.resize_bilinear(np.asarray(img, dtype=np.uint8), (out_w, out_h))[y0 - top:y1 - top, x0 - left:x1 - left]
        canvas[y0:y1, x0:x1] = hsv_shift_u8(rect, param["hue"], param["sat"], param["val"])
    return canvas[:, ::-1].copy() if param["flip"] else canvas


def mosaic_boxes(tile_boxes, tile_sizes, params4, cut, canvas_hw, max_boxes):
    """The boxes of one mosaic canvas: per tile q (raw boxes tile_boxes[q] of an image of tile_sizes[q] = (h, w), row
    params4[q]) `transform_boxes` on the whole canvas, clipped to the tile's window, rows whose width or height is then <= 1
    dropped; the tiles concatenated in the order 0..3, the first `max_boxes` kept, zero padded -> float32 [max_boxes,5].  A
    tile whose window is empty contributes nothing."""
    out = np.zeros((int(max_boxes), 5), dtype=np.float32)
    kept = []
    for q, (y0, y1, x0, x1) in enumerate(tile_windows(cut, canvas_hw)):
        if y0 >= y1 or x0 >= x1:
            continue
        b = transform_boxes(tile_boxes[q], tile_sizes[q], params4[q], canvas_hw, max_boxes)
        b = b[b[:, 2] - b[:, 0] > 0]                               # its compacted prefix
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], x0, x1)
        b[:, [1, 3]] = np.clip(b[:, [1, 3]], y0, y1)
        kept.append(b[(b[:, 2] - b[:, 0] > 1.0) & (b[:, 3] - b[:, 1] > 1.0)])
    if kept:
        rows = np.concatenate(kept)[:int(max_boxes)]
        out[:len(rows)] = rows
    return out


def mosaic_host(imgs4, params4, cut, canvas_hw, pad_value=128):
    """Four uint8 images, their four rows and the cut -> the mosaic canvas uint8 [H,W,3]: the NumPy restatement of
    y4_mosaic_u8_ragged for one canvas -- np.where over the four `augment_host` canvases, of which only those with a
    non-empty window are computed (the image of an empty window is not touched)."""
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    canvas = np.empty((H, W, 3), dtype=np.uint8)
    for q, (y0, y1, x0, x1) in enumerate(tile_windows(cut, canvas_hw)):
        if y0 < y1 and x0 < x1:
            canvas[y0:y1, x0:x1] = augment_host(imgs4[q], params4[q], canvas_hw, pad_value)[y0:y1, x0:x1]
    return canvas
