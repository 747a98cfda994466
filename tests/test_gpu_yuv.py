"""YUV 4:2:0 video frames on the GPU: y4_yuv_u8_ragged (csrc/yuv_u8.hip) and the plumbing above it (Engine.preprocess_yuv_batch,
predict_stream(yuv=), Yolov4.predict_yuv).  The reference is always the path that exists -- y4_resize_u8_ragged, or the Engine's
RGB entry -- on `yuv.to_rgb(frame)`, the NumPy restatement of the colour rule, and every comparison is `==` on every byte.

The witnesses restate one wrong kernel each on the host (formats swapped, chroma indexed by x, a wrong chroma pitch, the wrong
range or matrix, no clamp, interpolation before conversion) and check that its result differs from the right one on the very input
the device is then held to: a kernel with that mistake fails here."""
import copy
import os

import numpy as np
import pytest

from helpers import CLASS_DIR, GOLDEN
from test_gpu_letterbox import DEV, _engine, _images, _ragged, _same_bits

pytestmark = pytest.mark.gpu

CASES = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
FORMATS = ("nv12", "nv21", "i420", "yv12")
SIZES = [(1, 1), (2, 2), (1, 7), (7, 1), (5, 3), (45, 37), (64, 48), (333, 501)]
CANVASES = [(32, 32), (7, 9)]               # PX = 4 (three dword stores per thread) and PX = 1 (7 * 9 is no multiple of 4)


def _sample_index(f):
    """Buffer indices of the U and the V samples of frame f, [ch, cw] each."""
    ch, cw = (f.h + 1) // 2, (f.w + 1) // 2
    grid = np.arange(ch)[:, None] * f.c_pitch + np.arange(cw)[None, :] * f.c_step
    return f.u_offset + grid, f.v_offset + grid


def _frame(img, fmt, case, padded, fill, noise_seed=None):
    """from_rgb of `img`; padded: y_pitch = w + 13, c_pitch 13 above its minimum; noise_seed: chroma that changes at every sample
    (random bytes at the sample positions only: the pitch padding keeps `fill`)."""
    from yolo4hip import yuv
    h, w = img.shape[:2]
    step = 2 if fmt in ("nv12", "nv21") else 1
    yp, cp = (w + 13, step * ((w + 1) // 2) + 13) if padded else (None, None)
    f = yuv.from_rgb(img, fmt, case[0], case[1], y_pitch=yp, c_pitch=cp, fill=fill)
    if noise_seed is not None:
        rng = np.random.default_rng(noise_seed)
        for idx in _sample_index(f):
            f.data[idx] = rng.integers(0, 256, idx.shape).astype(np.uint8)
    return f


_cache = {}


def _mixed(H, W, fill):
    """The frames of one launch: every size twice and all 16 (format, matrix, range) combinations, tight and padded pitches,
    block images and per-sample chroma noise alternating; then one 1080 x 1920 frame and one of the canvas's own size (the copy
    path).  -> [(frame, case)], and the rule's RGB image of each (computed once per canvas: `fill` does not enter it)."""
    from yolo4hip import yuv
    key = (H, W, fill)
    if key not in _cache:
        sizes = [SIZES[k % len(SIZES)] for k in range(16)] + [(1080, 1920), (H, W)]
        imgs = _images(sizes, seed=H * 100 + W)
        items = []
        for k, img in enumerate(imgs):
            fmt, case = FORMATS[k % 4], CASES[(k // 4) % 4]
            items.append((_frame(img, fmt, case, padded=k % 3 == 1, fill=fill, noise_seed=k if k % 2 else None), case))
        if ("rgb", H, W) not in _cache:
            _cache[("rgb", H, W)] = [yuv.to_rgb(f, *case) for f, case in items]
        _cache[key] = items
    return _cache[key], _cache[("rgb", H, W)]


def _yuv_ragged(items, H, W, rects, pad):
    """y4_yuv_u8_ragged straight through the C ABI: the frames' buffers back to back + a descriptor table -> uint8 [n,H,W,3]."""
    import torch
    from yolo4hip import ext, yuv
    lib = ext.load()
    n = len(items)
    src = torch.from_numpy(np.concatenate([f.data[:f.nbytes] for f, _ in items])).to(DEV)
    desc = (ext.y4_yuv_desc * n)()
    off = 0
    for i, ((f, case), r) in enumerate(zip(items, rects)):
        f.fill_desc(desc[i], off, yuv.flags(*case))
        desc[i].out_h, desc[i].out_w, desc[i].pad_top, desc[i].pad_left = r
        off += f.nbytes
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
    out = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    ext.check(lib.y4_yuv_u8_ragged(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(out), H, W, pad, ext.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rects(shapes, H, W, mode):
    from yolo4hip import prepost
    return [(H, W, 0, 0) if mode == "stretch" else prepost.letterbox_rect(h, w, H, W) for h, w in shapes]


# ------------------------------------------------------------------ the C entry
@pytest.mark.parametrize("mode", ["stretch", "letterbox"])
@pytest.mark.parametrize("H,W", CANVASES)
def test_yuv_ragged_same_bytes_as_resize_ragged_on_to_rgb(H, W, mode):
    items, rgbs = _mixed(H, W, 0)
    assert {(f.fmt, c) for f, c in items} >= {(fmt, c) for fmt in FORMATS for c in CASES}
    assert items[-1][0].h == H and items[-1][0].w == W                    # h == out_h, w == out_w under both modes: the copy path
    rects = _rects([a.shape[:2] for a in rgbs], H, W, mode)
    want = _ragged(rgbs, H, W, rects, 99)
    got = _yuv_ragged(items, H, W, rects, 99)
    for i, (f, case) in enumerate(items):
        assert np.array_equal(got[i], want[i]), (i, f.h, f.w, f.fmt, case)
    assert np.array_equal(got[-1], rgbs[-1])                              # the copy path is the converted frame itself
    # the pitch padding is never read into the result: the same frames with another fill give the same bytes
    other, _ = _mixed(H, W, 255)
    assert any(not np.array_equal(a.data, b.data) for (a, _), (b, _) in zip(items, other))
    assert np.array_equal(_yuv_ragged(other, H, W, rects, 99), got)
    # a second identical call gives the same bytes
    assert np.array_equal(_yuv_ragged(items, H, W, rects, 99), got)


# ------------------------------------------------------------------ witnesses
def _host_canvas(rgb, H, W, rect, pad):
    """prepost's restatement of y4_resize_u8_ragged for one image."""
    from yolo4hip import prepost
    out_h, out_w, top, left = rect
    canvas = np.full((H, W, 3), pad, np.uint8)
    canvas[top:top + out_h, left:left + out_w] = prepost.resize_bilinear(rgb, (out_w, out_h))
    return canvas


def _noise_frame(h, w, fmt, seed, padded=False):
    """Random luma, chroma that changes at every sample, U != V everywhere."""
    from yolo4hip import yuv
    rng = np.random.default_rng(seed)
    step = 2 if fmt in ("nv12", "nv21") else 1
    ch, cw = (h + 1) // 2, (w + 1) // 2
    yp, cp = (w + 13, step * cw + 13) if padded else (w, step * cw)
    f = yuv.YuvFrame(rng.integers(0, 256, h * yp + 2 * ch * cp // step).astype(np.uint8), h, w, fmt, yp, cp)
    ui, vi = _sample_index(f)
    f.data[vi] = f.data[ui] ^ 0xFF
    return f


@pytest.mark.parametrize("H,W", CANVASES)
def test_witnesses_of_wrong_kernels(H, W):
    from yolo4hip import yuv
    items, wrongs = [], []

    def witness(name, f, case, wrong_rgb):
        items.append((f, case))
        wrongs.append((name, wrong_rgb))

    # NV12 read as NV21 (and I420 as YV12), U != V everywhere
    for fmt, other in (("nv12", "nv21"), ("i420", "yv12")):
        f = _noise_frame(12, 20, fmt, 1)
        g = yuv.YuvFrame(f.data, f.h, f.w, other)
        witness(f"{fmt} read as {other}", f, CASES[0], yuv.to_rgb(g, *CASES[0]))
    # chroma indexed by x instead of x >> 1 (kept inside the plane)
    f = _noise_frame(12, 20, "i420", 2)
    Y, U, V = f.planes()
    ys, xs = np.arange(f.h) >> 1, np.minimum(np.arange(f.w), U.shape[1] - 1)
    witness("chroma indexed by x", f, CASES[0], yuv.convert_px(Y, U[ys][:, xs], V[ys][:, xs], *CASES[0]))
    # c_pitch taken as w on an odd-width interleaved frame (tight pitch: w + 1)
    f = _noise_frame(45, 37, "nv12", 3)
    assert f.c_pitch == 38
    g = copy.copy(f)
    g.c_pitch = f.w
    witness("c_pitch taken as w", f, CASES[0], yuv.to_rgb(g, *CASES[0]))
    # limited range read as full, BT.601 read as BT.709
    f = _noise_frame(10, 14, "nv21", 4, padded=True)
    witness("limited read as full", f, ("bt601", False), yuv.to_rgb(f, "bt601", True))
    witness("bt601 read as bt709", f, ("bt601", False), yuv.to_rgb(f, "bt709", False))
    witness("bt709 full read as bt601 full", f, ("bt709", True), yuv.to_rgb(f, "bt601", True))
    # values that need the clamp at both ends: Y < 16 and Y = 255 under extreme chroma
    f = _noise_frame(8, 8, "yv12", 5)
    f.data[:64] = np.tile(np.array([0, 7, 15, 255], np.uint8), 16)
    ui, vi = _sample_index(f)
    f.data[ui] = np.array([[0, 255, 0, 255]] * 4, np.uint8)
    f.data[vi] = np.array([[0, 0, 255, 255]] * 4, np.uint8)
    Y, U, V = f.planes()
    y0, cy, crv, cgu, cgv, cbu = yuv.COEFFS[CASES[0]]
    C_, D_, E_ = Y.astype(np.int64) - y0, np.repeat(np.repeat(U, 2, 0), 2, 1).astype(np.int64) - 128, \
        np.repeat(np.repeat(V, 2, 0), 2, 1).astype(np.int64) - 128
    raw = np.stack([cy * C_ + crv * E_, cy * C_ + cgu * D_ + cgv * E_, cy * C_ + cbu * D_], -1) + 8192 >> 14
    assert raw.min() < 0 and raw.max() > 255
    witness("no clamp", f, CASES[0], raw.astype(np.uint8))
    # interpolation done in YUV before conversion: a 2 x 2 frame (one chroma sample) whose taps clamp differently in the two orders
    f = yuv.YuvFrame(np.array([255, 0, 0, 255, 128, 255], np.uint8), 2, 2, "i420")
    yuv444 = np.stack([f.planes()[0], np.full((2, 2), 128, np.uint8), np.full((2, 2), 255, np.uint8)], -1)
    items.append((f, ("bt601", True)))
    wrongs.append(("interpolated in YUV", None))

    rgbs = [yuv.to_rgb(f, *case) for f, case in items]
    rects = _rects([a.shape[:2] for a in rgbs], H, W, "stretch")
    want = _ragged(rgbs, H, W, rects, 128)
    got = _yuv_ragged(items, H, W, rects, 128)
    from yolo4hip import prepost
    for i, (name, wrong) in enumerate(wrongs):
        right_host = _host_canvas(rgbs[i], H, W, rects[i], 128)
        if wrong is None:
            # the NumPy restatement written both ways: convert the taps then interpolate / interpolate then convert
            mixed = prepost.resize_bilinear(yuv444, (W, H))
            wrong_host = yuv.convert_px(mixed[..., 0], mixed[..., 1], mixed[..., 2], "bt601", True)
        else:
            wrong_host = _host_canvas(wrong, H, W, rects[i], 128)
        assert np.array_equal(right_host, want[i]), name                  # the host restatement is the reference's bytes
        assert not np.array_equal(wrong_host, right_host), name           # the wrong kernel would be seen on this input ...
        assert np.array_equal(got[i], want[i]), name                      # ... and the device is right


# ------------------------------------------------------------------ Engine.preprocess_yuv_batch
@pytest.mark.parametrize("hw", [(160, 160), (96, 160)])
def test_preprocess_yuv_batch_equals_u8_batch_on_converted_frames(hw):
    from yolo4hip import yuv
    items, rgbs = _mixed(32, 32, 0)
    items, rgbs = items[:12], rgbs[:12]
    _, eng = _engine(hw, n=len(items))
    for case in (CASES[0], CASES[2]):
        frames = [f for f, c in items if c == case] + [yuv.from_rgb(rgbs[6], "nv12", *case).data.reshape(96, 48)]
        conv = [yuv.to_rgb(f, *case) for f in frames]
        assert len(frames) >= 3 and len({f.fmt for f in frames[:-1]}) >= 2
        for letterbox in (False, True):
            u8, bm = eng.preprocess_yuv_batch(frames, letterbox=letterbox, pad_value=90, matrix=case[0], full_range=case[1])
            ref_u8, ref_bm = eng.preprocess_u8_batch(conv, letterbox=letterbox, pad_value=90)
            assert u8.shape == ref_u8.shape and np.array_equal(u8.cpu().numpy(), ref_u8.cpu().numpy()), (case, letterbox)
            assert np.array_equal(bm.cpu().numpy(), ref_bm.cpu().numpy())
    with pytest.raises(ValueError):
        eng.preprocess_yuv_batch(frames, matrix="bt2020")
    with pytest.raises(ValueError):
        eng.preprocess_yuv_batch([np.zeros((6, 4), np.float32)])
    with pytest.raises(ValueError):
        eng.preprocess_yuv_batch([])
    with pytest.raises(ValueError):
        eng.preprocess_yuv_batch(frames, pad_value=256)
    eng.close()


# ------------------------------------------------------------------ predict_stream(yuv=)
def _street(h, w):
    from yolo4hip import prepost
    return prepost.resize_bilinear(prepost.imread_rgb(os.path.join(GOLDEN, "street.jpeg")), (w, h))


@pytest.mark.parametrize("letterbox", [False, True], ids=["stretch", "letterbox"])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_predict_stream_yuv_equals_stream_on_converted_frames(fmt, letterbox):
    import torch
    from yolo4hip import yuv
    _, eng = _engine((160, 160), 3, 2, weights=True)
    case = ("bt709", False)
    for fh, fw in ((120, 160), (160, 160)):
        base = _street(fh, fw)
        rgb6 = [np.roll(base, 7 * k, axis=1) for k in range(6)]
        raw = [yuv.from_rgb(a, fmt, *case).data.reshape(fh + fh // 2, fw) for a in rgb6]
        conv = [yuv.to_rgb(r, *case, fmt=fmt) for r in raw]
        ybatches = [np.stack(raw[i:i + 2]) for i in range(0, 6, 2)]
        ybatches[1] = torch.from_numpy(ybatches[1]).pin_memory()            # a pinned tensor is uploaded from where it lies
        rbatches = [np.stack(conv[i:i + 2]) for i in range(0, 6, 2)]
        kw = dict(with_indices=True, in_flight=2, letterbox=letterbox, pad_value=100)
        got = list(eng.predict_stream(ybatches, yuv=fmt, matrix=case[0], full_range=case[1], **kw))
        want = list(eng.predict_stream(rbatches, **kw))
        assert len(got) == len(want) == 3
        for g, w_ in zip(got, want):
            _same_bits(g, w_)
        # ... and both are the batch path on the converted frames
        u8, bm = eng.preprocess_u8_batch(conv[:2], letterbox=letterbox, pad_value=100)
        _same_bits(got[0], eng.predict(u8, with_indices=True, box_map=bm if letterbox else None))
    with pytest.raises(ValueError):
        list(eng.predict_stream(ybatches, yuv="nv16"))
    with pytest.raises(ValueError):
        list(eng.predict_stream(ybatches, yuv=fmt, matrix="bt2020"))
    with pytest.raises(ValueError):
        list(eng.predict_stream([np.zeros((2, 100, 160), np.uint8)], yuv=fmt))      # 100 rows are no h + h // 2
    with pytest.raises(ValueError):
        list(eng.predict_stream(rbatches, yuv=fmt))                                  # RGB batches under yuv=
    eng.close()


# ------------------------------------------------------------------ facade
@pytest.mark.parametrize("kw", [{}, {"nms_soft": "gaussian"}, {"letterbox": True, "pad_value": 100}],
                         ids=["default", "soft", "letterbox"])
def test_facade_predict_yuv(kw, tmp_path, monkeypatch):
    from yolo4hip import yuv
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    monkeypatch.setenv("YOLO4HIP_CACHE", str(tmp_path / "cache"))
    m = Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(160), dtype="f32", max_batch=2, tune=False, **kw)
    frames = [yuv.from_rgb(_street(200, 300), "nv12"), yuv.from_rgb(_street(121, 97), "yv12", y_pitch=128, c_pitch=64),
              yuv.from_rgb(_street(160, 160), "i420")]
    conv = [yuv.to_rgb(f) for f in frames]
    got = m.predict_yuv(frames)
    lb = bool(kw.get("letterbox"))
    u8, bm = m.engine.preprocess_u8_batch(conv, letterbox=lb, pad_value=kw.get("pad_value", 128))
    iou, score = m._thresholds
    want = m.engine.predict(u8, iou_threshold=iou, score_threshold=score, box_map=bm)
    assert len(got) == 4 and got[0].shape == (3, 100, 4)
    _same_bits(got, want)
    _same_bits(m.predict_yuv(frames), got)                                 # a second identical call gives the same bytes
    # another matrix is another image: the keyword reaches the kernel
    other = m.engine.preprocess_yuv_batch(frames, letterbox=lb, matrix="bt709", full_range=True)[0]
    assert not np.array_equal(other.cpu().numpy(), u8.cpu().numpy())
    # the rawvideo layout with its format keyword
    raw = yuv.from_rgb(_street(120, 160), "nv21").data.reshape(180, 160)
    _same_bits(m.predict_yuv(raw, fmt="nv21"), m.predict_yuv(yuv.YuvFrame(raw, fmt="nv21")))
    for bad in (dict(matrix="bt2020"), dict(fmt="nv16")):
        with pytest.raises(ValueError):
            m.predict_yuv(raw, **bad)
    with pytest.raises(ValueError):
        m.predict_yuv(raw.astype(np.int16))
    m.engine.close()
