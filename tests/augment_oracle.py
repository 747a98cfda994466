"""Float64 NumPy statement of the augmentation rule of yolo4hip/augment.py and csrc/canvas_u8.hip: the colour transform
(`rgb_to_hsv` / `hsv_to_rgb` follow the standard library's `colorsys`, to which tests/test_augment_cpu.py holds them) and the
geometry, written per canvas pixel (index arithmetic, where `augment.augment_host` works on slices).  The uint8 bilinear resize
itself is `prepost.resize_bilinear` (integer arithmetic, pinned by the letterbox tests)."""
import numpy as np


def rgb_to_hsv(rgb):
    """float64 [..., 3] in [0,1] -> (h, s, v), hue in [0,1); s = 0 and h = 0 at max == 0 or max == min."""
    rgb = np.asarray(rgb, dtype=np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    maxc, minc = rgb.max(axis=-1), rgb.min(axis=-1)
    rangec = maxc - minc
    grey = rangec == 0
    safe = np.where(grey, 1.0, rangec)
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = (h / 6.0) % 1.0
    s = rangec / np.where(maxc == 0, 1.0, maxc)
    return np.where(grey, 0.0, h), np.where(grey, 0.0, s), maxc


def hsv_to_rgb(h, s, v):
    h, s, v = (np.asarray(a, dtype=np.float64) for a in (h, s, v))
    i = (h * 6.0).astype(np.int64)
    f = h * 6.0 - i
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i % 6
    rgb = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], axis=-1)
    return np.where((s == 0)[..., None], v[..., None], rgb)


def colour_levels(rgb_u8, hue, sat, val):
    """uint8 [..., 3] -> float64 255 c of the transformed colour, BEFORE the rounding to a byte."""
    h, s, v = rgb_to_hsv(np.asarray(rgb_u8, dtype=np.float64) / 255.0)
    h = h + float(hue)
    h = h - np.floor(h)
    s = np.clip(s * float(sat), 0.0, 1.0)
    v = np.clip(v * float(val), 0.0, 1.0)
    return 255.0 * hsv_to_rgb(h, s, v)


def colour(rgb_u8, hue, sat, val):
    if float(hue) == 0.0 and float(sat) == 1.0 and float(val) == 1.0:
        return np.asarray(rgb_u8, dtype=np.uint8).copy()
    return np.clip(np.floor(colour_levels(rgb_u8, hue, sat, val) + 0.5), 0, 255).astype(np.uint8)


def augment(img, param, canvas_hw, pad_value=128):
    """-> (uint8 canvas [H,W,3], bool [H,W]: the pixel is a resized one, not pad)."""
    from yolo4hip import prepost
    H, W = int(canvas_hw[0]), int(canvas_hw[1])
    out_h, out_w, top, left = (int(param[k]) for k in ("out_h", "out_w", "pad_top", "pad_left"))
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xs = W - 1 - x if int(param["flip"]) else x
    yy, xx = y - top, xs - left
    inside = (yy >= 0) & (yy < out_h) & (xx >= 0) & (xx < out_w)
    canvas = np.full((H, W, 3), pad_value, dtype=np.uint8)
    if inside.any():
        resized = prepost.resize_bilinear(np.asarray(img, dtype=np.uint8), (out_w, out_h))
        canvas[inside] = colour(resized[yy[inside], xx[inside]], param["hue"], param["sat"], param["val"])
    return canvas, inside
