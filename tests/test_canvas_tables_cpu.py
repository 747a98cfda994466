"""yolo4hip.canvas on the host: the placement rule, the fitted tables and box maps, the tables of max_batch equal sources that
`Engine.predict_stream` uploads (RGB and the four YUV formats), and the placement of sources (shared rows, windows)."""
import ctypes as C

import numpy as np
import pytest

from yolo4hip import canvas, ext, prepost, yuv

H, W = 96, 160
SIZES = [(90, 200), (50, 30), (96, 160), (1, 1)]
FRAMES = [(90, 200), (96, 160), (2, 2)]


def _bytes(table):
    return bytes(np.frombuffer(table, dtype=np.uint8))


def test_importing_canvas_loads_nothing():
    import subprocess
    import sys
    code = "import sys, yolo4hip.canvas, yolo4hip.ext as e; assert 'torch' not in sys.modules and e._lib is None"
    subprocess.run([sys.executable, "-c", code], check=True, env={"PYTHONPATH": ":".join(sys.path)})


@pytest.mark.parametrize("h,w", SIZES)
def test_fit_rect(h, w):
    assert prepost.fit_rect(h, w, H, W, True) == prepost.letterbox_rect(h, w, H, W)
    assert prepost.fit_rect(h, w, H, W, False) == (H, W, 0, 0)


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("Desc", [ext.y4_image_desc, ext.y4_yuv_desc])
def test_fit_table_rects_and_maps(Desc, letterbox):
    desc, maps = canvas.fit_table(Desc, SIZES, H, W, letterbox)
    assert len(desc) == len(SIZES) and maps.dtype == np.float32 and maps.shape == (len(SIZES), 4)
    for d, m, (h, w) in zip(desc, maps, SIZES):
        rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
        assert (d.out_h, d.out_w, d.pad_top, d.pad_left) == rect
        want = prepost.box_map(h, w, H, W, rect)
        assert want.dtype == np.float32 and (m == want).all()
    if not letterbox:
        assert (maps == np.float32([1, 0, 1, 0])).all()


def test_rect_table_takes_rows_that_carry_their_rect():
    from yolo4hip import tiling
    rows = tiling.tile_rows(200, 300, (H, W), None, 0.2, True, True)
    desc = canvas.rect_table(ext.y4_window_desc, [r[1] for r in rows])
    assert [(d.out_h, d.out_w, d.pad_top, d.pad_left) for d in desc] == [tuple(r[1]) for r in rows]
    assert rows[-1][1] == prepost.letterbox_rect(200, 300, H, W)                 # (the full image, through fit_rect)
    assert all(d.offset == 0 and d.h == 0 for d in desc)


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("h,w", FRAMES)
def test_equal_rgb_sources_give_the_stream_table(h, w, letterbox):
    B = 3
    desc, maps = canvas.fit_table(ext.y4_image_desc, [(h, w)] * B, H, W, letterbox)
    offs = canvas.place_sources(desc, [(h, w, 3)] * B)
    rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
    want = (ext.y4_image_desc * B)()
    for j in range(B):
        want[j].offset, want[j].h, want[j].w = j * h * w * 3, h, w
        want[j].out_h, want[j].out_w, want[j].pad_top, want[j].pad_left = rect
    assert _bytes(desc) == _bytes(want)
    assert offs == [j * h * w * 3 for j in range(B + 1)]
    assert (maps == np.tile(prepost.box_map(h, w, H, W, rect), (B, 1))).all()


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_equal_yuv_sources_give_the_stream_table(fmt, h, w, letterbox):
    B = 3
    word = yuv.flags("bt709", True)
    assert word != 0
    layout = yuv.YuvFrame(np.empty((h + h // 2, w), np.uint8), fmt=fmt)
    assert (layout.h, layout.w, layout.nbytes) == (h, w, (h + h // 2) * w)
    desc, maps = canvas.fit_table(ext.y4_yuv_desc, [(h, w)] * B, H, W, letterbox)
    offs = canvas.place_sources(desc, [(layout.nbytes,)] * B, place=lambda d, k, off: layout.fill_desc(d, off, word))
    # the tight frame written out: luma h x w, then w bytes per chroma row pair (interleaved) or two planes of (h/2) x (w/2)
    rect = prepost.letterbox_rect(h, w, H, W) if letterbox else (H, W, 0, 0)
    want = (ext.y4_yuv_desc * B)()
    for j in range(B):
        base, d = j * (h + h // 2) * w, want[j]
        first, second = base + h * w, base + h * w + (h // 2) * (w // 2)
        d.y_offset = base
        d.u_offset, d.v_offset = {"nv12": (first, first + 1), "nv21": (first + 1, first), "i420": (first, second),
                                  "yv12": (second, first)}[fmt]
        d.y_pitch, d.c_pitch, d.c_step = (w, w, 2) if fmt in ("nv12", "nv21") else (w, w // 2, 1)
        d.h, d.w, d.flags = h, w, 3
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
    assert _bytes(desc) == _bytes(want)
    assert offs[-1] == B * (h + h // 2) * w
    assert (maps == np.tile(prepost.box_map(h, w, H, W, rect), (B, 1))).all()


def test_place_sources_offsets_and_shared_rows():
    shapes = [(4, 5, 3), (2, 2, 3), (7, 1, 3)]
    desc = (ext.y4_image_desc * 3)()
    assert canvas.place_sources(desc, shapes) == [0, 60, 72, 93]
    assert [(d.offset, d.h, d.w) for d in desc] == [(0, 4, 5), (60, 2, 2), (72, 7, 1)]
    # mosaic: rows share images, every image is placed once
    desc = (ext.y4_augment_desc * 5)()
    assert canvas.place_sources(desc, shapes, rows=np.array([2, 0, 0, 1, 2]))[-1] == 93
    assert [(d.offset, d.h, d.w) for d in desc] == [(72, 7, 1), (0, 4, 5), (0, 4, 5), (60, 2, 2), (72, 7, 1)]


def test_place_sources_windows():
    shapes = [(10, 20, 3), (6, 8, 3)]
    desc = (ext.y4_window_desc * 3)()
    offs = canvas.place_sources(desc, shapes, rows=[0, 1, 1], windows=[(2, 3, 4, 5), (0, 0, 6, 8), (5, 7, 1, 1)])
    assert offs == [0, 600, 744]
    assert [(d.offset, d.pitch, d.h, d.w) for d in desc] == [((2 * 20 + 3) * 3, 60, 4, 5), (600, 24, 6, 8),
                                                            (600 + (5 * 8 + 7) * 3, 24, 1, 1)]
    for bad in [(0, 0, 7, 8), (0, 1, 6, 8), (-1, 0, 2, 2), (0, 0, 0, 1), (5, 7, 1, 2)]:
        with pytest.raises(ValueError, match="not inside"):
            canvas.place_sources((ext.y4_window_desc * 1)(), shapes, rows=[1], windows=[bad])
    assert C.sizeof(ext.y4_view_desc) > C.sizeof(ext.y4_window_desc)             # (view rows are placed by the same fields)
    vdesc = (ext.y4_view_desc * 1)()
    canvas.place_sources(vdesc, shapes, rows=[1], windows=[(1, 2, 3, 4)])
    assert (vdesc[0].offset, vdesc[0].pitch, vdesc[0].h, vdesc[0].w) == (600 + (1 * 8 + 2) * 3, 24, 3, 4)
