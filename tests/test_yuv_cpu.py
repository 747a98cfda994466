"""YUV 4:2:0 frames on the host (yolo4hip/yuv.py): the integer colour rule against the float64 matrices of tests/yuv_oracle.py
over the whole (Y, U, V) cube, the coefficient table, the four layouts with tight and padded pitches, odd sizes, refused inputs,
and the C-ABI entry's host checks.  No GPU: the checks return before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

import yuv_oracle as YO


def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
    img = np.kron(base, np.ones((8, 8, 1)))[:h, :w] + rng.integers(-20, 21, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ the colour rule
def test_coefficient_table_is_rounded_real_coefficients():
    from yolo4hip import yuv
    assert sorted(yuv.COEFFS) == sorted(YO.CASES)
    assert yuv.KR_KB == YO.KR_KB
    for case in YO.CASES:
        real = YO.real_coeffs(*case)
        want = (real[0],) + tuple(math.floor(c * 2 ** 14 + 0.5) for c in real[1:])
        assert yuv.COEFFS[case] == want, (case, yuv.COEFFS[case], want)
    # the table of the issue, literally
    assert yuv.COEFFS[("bt601", False)] == (16, 19077, 26149, -6419, -13320, 33050)
    assert yuv.COEFFS[("bt601", True)] == (0, 16384, 22970, -5638, -11700, 29032)
    assert yuv.COEFFS[("bt709", False)] == (16, 19077, 29372, -3494, -8731, 34610)
    assert yuv.COEFFS[("bt709", True)] == (0, 16384, 25802, -3069, -7670, 30402)
    assert [yuv.flags(m, f) for m, f in YO.CASES] == [0, 2, 1, 3]


def _cube_frames():
    """The 2^24 (Y, U, V) triples as 64 I420 frames of 512 x 512: chroma sample (r, c) is (U, V) = (r, c), and the four luma
    pixels of its block in frame k are Y = 4 k .. 4 k + 3."""
    from yolo4hip import yuv
    u = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    v = u.T
    for k in range(64):
        y = np.empty((512, 512), np.uint8)
        y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = 4 * k, 4 * k + 1, 4 * k + 2, 4 * k + 3
        yield yuv.YuvFrame(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]), 512, 512, "i420")


@pytest.mark.parametrize("matrix,full_range", YO.CASES)
def test_to_rgb_whole_cube_against_float64(matrix, full_range):
    from yolo4hip import yuv
    worst = 0.0
    differ = np.zeros(3, np.int64)
    seen = np.zeros(256, bool)
    for f in _cube_frames():
        got = yuv.to_rgb(f, matrix, full_range)
        Y, U, V = f.planes()
        up = np.repeat(np.repeat(U, 2, axis=0), 2, axis=1)
        vp = np.repeat(np.repeat(V, 2, axis=0), 2, axis=1)
        seen[np.unique(Y)] = True
        exact = YO.exact_rgb(Y, up, vp, matrix, full_range)
        worst = max(worst, float(np.abs(got - np.clip(exact, 0, 255)).max()))
        half_up = np.clip(np.floor(exact + 0.5), 0, 255)
        differ += (got != half_up).reshape(-1, 3).sum(axis=0)
    assert seen.all()
    share = differ / float(2 ** 24)
    print(f"{matrix} full_range={full_range}: max |rule - exact| {worst:.4f}, share != round-half-up per channel {share}")
    assert worst <= 0.51, worst
    assert (share <= 0.0025).all(), share


# ------------------------------------------------------------------ layouts
PITCHES = [(None, None), (13, 13)]          # tight, and y_pitch = w + 13 with c_pitch likewise


def _pitches(h, w, fmt, extra):
    if extra == (None, None):
        return None, None
    step = 2 if fmt in ("nv12", "nv21") else 1
    return w + extra[0], step * ((w + 1) // 2) + extra[1]


@pytest.mark.parametrize("hw", [(48, 64), (45, 37)])
@pytest.mark.parametrize("case", YO.CASES)
def test_four_layouts_and_pitches_give_one_rgb(hw, case):
    from yolo4hip import yuv
    img = _image(*hw, seed=hw[0])
    ref = None
    for fmt in yuv.FORMATS:
        for extra in PITCHES:
            yp, cp = _pitches(hw[0], hw[1], fmt, extra)
            outs = []
            for fill in (0, 255, 77):
                f = yuv.from_rgb(img, fmt, case[0], case[1], y_pitch=yp, c_pitch=cp, fill=fill)
                assert (f.h, f.w, f.fmt) == (hw[0], hw[1], fmt)
                assert f.y_pitch == (hw[1] if yp is None else yp)
                outs.append(yuv.to_rgb(f, *case))
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (fmt, extra)   # independent of fill
            if ref is None:
                ref = outs[0]
            assert np.array_equal(outs[0], ref), (fmt, extra)
    assert ref.shape == img.shape and ref.dtype == np.uint8
    # a round trip is lossy (chroma is subsampled) but close on 8 x 8 blocks of colour: the layouts were not mixed up
    assert np.abs(ref.astype(int) - img.astype(int)).mean() < 12


def test_plane_order_of_the_four_formats():
    from yolo4hip import yuv
    h, w = 4, 6
    img = _image(h, w, seed=1)
    frames = {fmt: yuv.from_rgb(img, fmt) for fmt in yuv.FORMATS}
    Y, U, V = frames["i420"].planes()
    assert not np.array_equal(U, V)
    for fmt, f in frames.items():
        y, u, v = f.planes()
        assert np.array_equal(y, Y) and np.array_equal(u, U) and np.array_equal(v, V), fmt
    assert np.array_equal(frames["nv12"].data[h * w:].reshape(2, 3, 2)[:, :, 0], U)
    assert np.array_equal(frames["nv21"].data[h * w:].reshape(2, 3, 2)[:, :, 0], V)
    assert np.array_equal(frames["i420"].data[h * w:h * w + 6].reshape(2, 3), U)
    assert np.array_equal(frames["yv12"].data[h * w:h * w + 6].reshape(2, 3), V)
    # the rawvideo layout: a 2-D array [h + h // 2, w] is a frame wherever a frame is taken
    raw = frames["nv21"].data.reshape(h + h // 2, w)
    assert np.array_equal(yuv.to_rgb(raw, fmt="nv21"), yuv.to_rgb(frames["nv21"]))
    assert not np.array_equal(yuv.to_rgb(raw, fmt="nv12"), yuv.to_rgb(frames["nv21"]))


def test_from_rgb_rounds_half_up_and_averages_blocks():
    from yolo4hip import yuv
    img = _image(6, 8, seed=2)
    for case in YO.CASES:
        m, off = yuv.forward_matrix(*case)
        x = img.astype(np.float64) @ m.T + off
        f = yuv.from_rgb(img, "i420", *case)
        Y, U, V = f.planes()
        assert np.array_equal(Y, np.clip(np.floor(x[:, :, 0] + 0.5), 0, 255).astype(np.uint8))
        mean = x[:, :, 1:].reshape(3, 2, 4, 2, 2).mean(axis=(1, 3))
        assert np.array_equal(np.stack([U, V], -1), np.clip(np.floor(mean + 0.5), 0, 255).astype(np.uint8))
        # the forward matrix inverts the oracle's: exact YUV -> exact RGB is the identity
        back = YO.exact_rgb(x[:, :, 0], x[:, :, 1], x[:, :, 2], *case)
        assert np.abs(back - img).max() < 1e-9


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (5, 3)])
@pytest.mark.parametrize("fmt", ["nv12", "nv21", "i420", "yv12"])
def test_odd_sizes(hw, fmt):
    from yolo4hip import yuv
    h, w = hw
    ch, cw = (h + 1) // 2, (w + 1) // 2
    assert yuv.chroma_size(h, w) == (ch, cw)
    rng = np.random.default_rng(h * 10 + w)
    step = 2 if fmt in ("nv12", "nv21") else 1
    # chroma that changes at every sample, and every sample distinct from its neighbours
    buf = rng.integers(0, 256, h * w + 2 * ch * cw).astype(np.uint8)
    f = yuv.YuvFrame(buf, h, w, fmt)
    assert f.nbytes == h * w + 2 * ch * cw and (f.y_pitch, f.c_pitch, f.c_step) == (w, step * cw, step)
    Y, U, V = f.planes()
    assert Y.shape == (h, w) and U.shape == (ch, cw) and V.shape == (ch, cw)
    got = yuv.to_rgb(f, "bt709", True)
    for y in range(h):
        for x in range(w):
            want = yuv.convert_px(Y[y, x], U[y >> 1, x >> 1], V[y >> 1, x >> 1], "bt709", True)
            assert np.array_equal(got[y, x], want), (y, x)
    # the last column / row read chroma sample (w - 1) >> 1 / (h - 1) >> 1: changing that sample alone changes them
    g = yuv.YuvFrame(buf.copy(), h, w, fmt)
    g.data[g.u_offset + ((h - 1) >> 1) * g.c_pitch + ((w - 1) >> 1) * g.c_step] ^= 0x80
    assert not np.array_equal(yuv.to_rgb(g, "bt709", True)[h - 1, w - 1], got[h - 1, w - 1])
    # from_rgb: the edge blocks are averaged over what exists
    img = _image(h, w, seed=3)
    fr = yuv.from_rgb(img, fmt)
    m, off = yuv.forward_matrix()
    x = img.astype(np.float64) @ m.T + off
    last = x[2 * (ch - 1):, 2 * (cw - 1):, 1].mean()
    assert fr.planes()[1][-1, -1] == int(np.clip(np.floor(last + 0.5), 0, 255))


# ------------------------------------------------------------------ refused inputs
def test_refused_inputs():
    from yolo4hip import yuv
    ok = np.zeros(8 * 6 * 3 // 2, np.uint8)
    yuv.YuvFrame(ok, 6, 8, "nv12")
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok, 6, 8, "nv16")                               # unknown format
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok[:-1], 6, 8, "nv12")                          # one byte short
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok[:-1], 6, 8, "yv12")
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok, 6, 8, "nv12", y_pitch=9)                    # the buffer is too short for the wider pitch
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros(1000, np.uint8), 6, 8, "nv12", y_pitch=7)      # pitches below the minimum
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros(1000, np.uint8), 6, 8, "nv12", c_pitch=7)
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros(1000, np.uint8), 6, 8, "i420", c_pitch=3)
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros(1000, np.uint8), 5, 7, "nv12", c_pitch=7)      # ceil(7 / 2) samples of 2 bytes
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok.astype(np.int32), 6, 8, "nv12")              # non-uint8 data
    with pytest.raises(ValueError):
        yuv.YuvFrame(ok.astype(np.float32), 6, 8, "nv12")
    with pytest.raises(ValueError):
        yuv.YuvFrame(list(ok), 6, 8, "nv12")
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros((10, 8), np.uint8))                    # 2-D rawvideo: rows are no h + h // 2
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros((9, 7), np.uint8))                     # odd width
    with pytest.raises(ValueError):
        yuv.YuvFrame(np.zeros((18, 16), np.uint8)[:, ::2])           # not contiguous
    f = yuv.YuvFrame(ok, 6, 8, "nv12")
    with pytest.raises(ValueError):
        yuv.to_rgb(f, matrix="bt2020")
    with pytest.raises(ValueError):
        yuv.flags("rec601")
    with pytest.raises(ValueError):
        yuv.from_rgb(np.zeros((4, 4, 3), np.uint8), "rgb24")
    with pytest.raises(ValueError):
        yuv.from_rgb(np.zeros((4, 4, 3), np.uint8), "nv12", matrix="bt2020")
    with pytest.raises(ValueError):
        yuv.from_rgb(np.zeros((4, 4, 3), np.float32), "nv12")
    with pytest.raises(ValueError):
        yuv.from_rgb(np.zeros((4, 4, 3), np.uint8), "nv12", y_pitch=3)
    with pytest.raises(ValueError):
        yuv.as_frames([])


def test_utils_reexports():
    import utils
    from yolo4hip import yuv
    assert utils.YuvFrame is yuv.YuvFrame and utils.yuv_to_rgb is yuv.to_rgb and utils.yuv_from_rgb is yuv.from_rgb


# ------------------------------------------------------------------ the C entry, host side
def test_yuv_desc_layout_and_symbol():
    from yolo4hip import ext
    lib = ext.load()
    assert "y4_yuv_u8_ragged" in ext.SYMBOLS and hasattr(lib, "y4_yuv_u8_ragged")
    assert C.sizeof(ext.y4_yuv_desc) == 64 and C.sizeof(ext.y4_yuv_desc) % 8 == 0
    assert ext.y4_yuv_desc.y_pitch.offset == 24 and ext.y4_yuv_desc.h.offset == 36 and ext.y4_yuv_desc.flags.offset == 60


def test_yuv_u8_ragged_host_checks():
    from yolo4hip import ext
    lib = ext.load()
    EINVAL = -22
    p = C.c_void_p(4096)                                   # never dereferenced: every call below fails a host check
    assert lib.y4_yuv_u8_ragged(None, p, 1, p, 608, 608, 128, None) == EINVAL
    assert lib.y4_yuv_u8_ragged(p, None, 1, p, 608, 608, 128, None) == EINVAL
    assert lib.y4_yuv_u8_ragged(p, p, 1, None, 608, 608, 128, None) == EINVAL
    assert b"yuv_u8_ragged" in lib.y4_last_error()
    for n in (0, -1, 65536):
        assert lib.y4_yuv_u8_ragged(p, p, n, p, 608, 608, 128, None) == EINVAL
    for H, W in ((0, 608), (608, 0), (-1, 608)):
        assert lib.y4_yuv_u8_ragged(p, p, 1, p, H, W, 128, None) == EINVAL
    for pad in (-1, 256):
        assert lib.y4_yuv_u8_ragged(p, p, 1, p, 608, 608, pad, None) == EINVAL
    assert lib.y4_yuv_u8_ragged(p, p, 2000, p, 608, 608, 128, None) == EINVAL      # 2000 * 608 * 608 * 3 >= 2^31
