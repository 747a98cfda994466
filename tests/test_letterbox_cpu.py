"""Letterbox geometry on the host (prepost.letterbox_rect / letterbox / box_map) and the host-side argument checks of the two
C-ABI entries behind it (y4_resize_u8_ragged, y4_decode_nms_mapped).  No GPU: the checks return before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import ROOT

CANVASES = [(608, 608), (352, 608), (608, 352), (96, 160)]
IMAGES = [(1080, 1920), (1920, 1080), (480, 640), (608, 608), (304, 304), (176, 304), (1, 500), (500, 1), (1, 1),
          (3, 4000), (4000, 3), (37, 61)]


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("h,w", IMAGES)
def test_letterbox_rect_fits_touches_and_is_centred(h, w, H, W):
    from yolo4hip import prepost
    out_h, out_w, top, left = prepost.letterbox_rect(h, w, H, W)
    assert 1 <= out_h <= H and 1 <= out_w <= W
    assert 0 <= top and top + out_h <= H and 0 <= left and left + out_w <= W
    # touches two opposite sides: it fills one dimension
    assert out_h == H or out_w == W
    # centred (an odd margin puts the extra row / column at the bottom / right)
    assert top == (H - out_h) // 2 and left == (W - out_w) // 2
    # the aspect is kept to within the integer truncation of the scaled side
    if out_w == W:
        assert out_h == max(1, (h * W) // w)
    else:
        assert out_w == max(1, (w * H) // h)


def test_letterbox_rect_examples():
    from yolo4hip import prepost
    assert prepost.letterbox_rect(1080, 1920, 608, 608) == (342, 608, 133, 0)
    assert prepost.letterbox_rect(1920, 1080, 608, 608) == (608, 342, 0, 133)
    assert prepost.letterbox_rect(1080, 1920, 352, 608) == (342, 608, 5, 0)
    assert prepost.letterbox_rect(1920, 1080, 352, 608) == (352, 198, 0, 205)
    assert prepost.letterbox_rect(304, 304, 608, 608) == (608, 608, 0, 0)     # exact aspect: the whole canvas
    assert prepost.letterbox_rect(1, 5000, 608, 608) == (1, 608, 303, 0)      # never a zero-height rectangle
    with pytest.raises(ValueError):
        prepost.letterbox_rect(0, 5, 608, 608)


@pytest.mark.parametrize("h,w,H,W", [(304, 304, 608, 608), (176, 304, 352, 608), (352, 608, 352, 608), (88, 152, 352, 608)])
def test_letterbox_at_canvas_aspect_is_the_stretch(h, w, H, W):
    from yolo4hip import prepost
    rng = np.random.default_rng(h * w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    assert np.array_equal(prepost.letterbox(img, (H, W)), prepost.resize_bilinear(img, (W, H)))
    f = img.astype(np.float64)
    assert np.array_equal(prepost.letterbox(f, (H, W)), prepost.resize_bilinear(f, (W, H)))


@pytest.mark.parametrize("pad", [0, 128, 255])
def test_letterbox_places_the_resized_image_on_the_pad(pad):
    from yolo4hip import prepost
    rng = np.random.default_rng(pad)
    img = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    out = prepost.letterbox(img, (608, 608), pad)
    out_h, out_w, top, left = prepost.letterbox_rect(1080, 1920, 608, 608)
    assert out.shape == (608, 608, 3) and out.dtype == np.uint8
    assert np.array_equal(out[top:top + out_h, left:left + out_w], prepost.resize_bilinear(img, (out_w, out_h)))
    assert (out[:top] == pad).all() and (out[top + out_h:] == pad).all()


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("h,w", IMAGES)
def test_box_map_sends_the_content_rectangle_to_the_unit_square(h, w, H, W):
    from yolo4hip import prepost
    rect = prepost.letterbox_rect(h, w, H, W)
    out_h, out_w, top, left = rect
    m = prepost.box_map(h, w, H, W, rect)
    assert m.dtype == np.float32 and m.shape == (4,)
    assert np.array_equal(m, prepost.box_map(h, w, H, W))          # rect=None: the letterbox rectangle
    ax, bx, ay, by = (np.float64(v) for v in m)
    # corners of the content rectangle, canvas-normalised -> 0 and 1 (float32 coefficients: a few ulp of 1)
    assert abs((left / W) * ax + bx) < 1e-6 and abs(((left + out_w) / W) * ax + bx - 1) < 1e-6
    assert abs((top / H) * ay + by) < 1e-6 and abs(((top + out_h) / H) * ay + by - 1) < 1e-6
    # float64 then float32
    assert m[0] == np.float32(W / out_w) and m[1] == np.float32(-left / out_w)
    assert m[2] == np.float32(H / out_h) and m[3] == np.float32(-top / out_h)


def test_stretch_map_is_the_identity():
    from yolo4hip import prepost
    for h, w, H, W in [(1080, 1920, 608, 608), (7, 3, 352, 608)]:
        assert prepost.box_map(h, w, H, W, (H, W, 0, 0)).tolist() == [1.0, 0.0, 1.0, 0.0]
    b = np.array([[-0.1, 0.2, 0.5, 1.3]], np.float32)
    assert np.array_equal(prepost.map_boxes(b, [1, 0, 1, 0]), np.clip(b, 0, 1))


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "yolo4hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(y4_[a-z0-9_]+)\s*\(", text))


def test_new_entries_exported_and_bound():
    from yolo4hip import ext
    lib = ext.load()
    for name in ("y4_resize_u8_ragged", "y4_decode_nms_mapped"):
        assert name in _header_symbols()
        assert name in ext.SYMBOLS
        assert hasattr(lib, name)
    assert C.sizeof(ext.y4_image_desc) == 8 + 6 * 4
    assert lib.y4_version().decode().startswith("yolo4hip 0.5")


def test_resize_u8_ragged_host_checks():
    """Every bad argument is refused with Y4_EINVAL before a launch: fake (never dereferenced) pointers are enough."""
    from yolo4hip import ext
    lib = ext.load()
    p = C.c_void_p(0x1000)
    EINVAL = -22
    assert lib.y4_resize_u8_ragged(None, p, 1, p, 608, 608, 128, None) == EINVAL
    assert lib.y4_resize_u8_ragged(p, None, 1, p, 608, 608, 128, None) == EINVAL
    assert lib.y4_resize_u8_ragged(p, p, 1, None, 608, 608, 128, None) == EINVAL
    assert b"null" in lib.y4_last_error()
    for n in (0, -1, 70000):
        assert lib.y4_resize_u8_ragged(p, p, n, p, 608, 608, 128, None) == EINVAL
    for H, W in ((0, 608), (608, 0), (-32, 608)):
        assert lib.y4_resize_u8_ragged(p, p, 1, p, H, W, 128, None) == EINVAL
    for pad in (-1, 256):
        assert lib.y4_resize_u8_ragged(p, p, 1, p, 608, 608, pad, None) == EINVAL
    assert b"pad_value" in lib.y4_last_error()
    # n * H * W * 3 >= 2^31: the output offsets would overflow int32
    assert lib.y4_resize_u8_ragged(p, p, 2000, p, 608, 608, 128, None) == EINVAL
    assert b"2^31" in lib.y4_last_error()


def test_decode_nms_mapped_host_checks():
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    lib = ext.load()
    p = C.c_void_p(0x1000)
    # no handle / an unbound handle: refused before any launch
    assert lib.y4_decode_nms_mapped(None, 1, -1.0, -1.0, p, p, p, p, p, p, None) == -22
    h = C.c_void_p()
    cfg = _cfg_struct(make_config((96, 160)), 3, 2, "f32")
    assert lib.y4_create_hw(C.byref(cfg), 96, 160, C.byref(h)) == 0
    try:
        assert lib.y4_decode_nms_mapped(h, 1, -1.0, -1.0, p, p, p, p, p, p, None) == -1        # Y4_ESTATE: no workspace
        assert lib.y4_decode_nms(h, 1, -1.0, -1.0, p, p, p, p, p, None) == -1
    finally:
        assert lib.y4_destroy(h) == 0
