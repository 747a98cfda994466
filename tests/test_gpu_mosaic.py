"""y4_mosaic_u8_ragged on the GPU (csrc/canvas_u8.hip) against y4_augment_u8_ragged on the same device, `augment.mosaic_host` and
the float64 oracle of tests/augment_oracle.py, and `Yolov4.fit` over a mosaic `DataGenerator` (`Engine.mosaic_u8_batch`).

The rule is a composition (tests/test_mosaic_cpu.py: `compose`): byte identity with np.where over four outputs of the existing
kernel, colour included, since the mosaic kernel calls the same per-pixel functions.  Against the float64 oracle the bound is
that of tests/test_gpu_augment.py (1 level, SHARE_CAP of the bytes) on the same inputs (`colour_table`); the measured share is
written to profiles/fit/mosaic_measured.json."""
import numpy as np
import pytest

import augment_oracle as AO
from test_augment_cpu import CANVASES, SHARE_CAP, colour_table, differing, geometry_rows, make_params, sources
from test_gpu_augment import _augment, _fit
from test_mosaic_cpu import MOSAIC_CANVASES, compose, cuts_of, mixed_table, note, pick_tiles, window_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fill(d, p):
    d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
    d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])


def _mosaic(imgs, tile_src, params4, cuts, H, W, pad, shared=True, misalign=0):
    """y4_mosaic_u8_ragged straight through the C ABI -> uint8 [n,H,W,3] on the host.  shared: every image is packed once and
    the rows of the tiles that use it carry the same offset; otherwise every row gets a copy of its own.  misalign: the output
    starts that many bytes into its buffer."""
    import torch
    from yolo4hip import ext
    lib = ext.load()
    tile_src = np.asarray(tile_src)
    n = len(tile_src)
    flat = tile_src.reshape(-1)
    packed = list(imgs) if shared else [imgs[k] for k in flat]
    offs = np.concatenate([[0], np.cumsum([a.size for a in packed])])
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in packed])).to(DEV)
    desc = (ext.y4_augment_desc * (4 * n))()
    for r, (d, k, p) in enumerate(zip(desc, flat, np.asarray(params4).reshape(-1))):
        d.offset, d.h, d.w = int(offs[k if shared else r]), imgs[k].shape[0], imgs[k].shape[1]
        _fill(d, p)
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
    cuts_dev = torch.from_numpy(np.ascontiguousarray(cuts, dtype=np.int32).reshape(n, 2)).to(DEV)
    buf = torch.full((n * H * W * 3 + misalign,), 7, dtype=torch.uint8, device=DEV)
    out = buf[misalign:]
    ext.check(lib.y4_mosaic_u8_ragged(ext.ptr(src), ext.ptr(desc_dev), ext.ptr(cuts_dev), n, ext.ptr(out), H, W, pad, ext.stream_ptr()))
    torch.cuda.synchronize()
    assert (buf[:misalign] == 7).all()
    return out.cpu().numpy().reshape(n, H, W, 3)


@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)                             # (37, 61): one pixel per thread
def test_same_bytes_as_composed_augment_u8_ragged(H, W):
    imgs, params = mixed_table(H, W)
    singles = _augment(imgs, params, H, W, 99)                              # the existing kernel, on this device
    cuts = cuts_of(H, W)
    src = pick_tiles(len(cuts), len(imgs))
    got = _mosaic(imgs, src, params[src], cuts, H, W, 99)
    for i, cut in enumerate(cuts):
        assert np.array_equal(got[i], compose([singles[k] for k in src[i]], cut)), (cut, src[i])
    if H * W % 4 == 0:                                                      # an output off a dword: the one-pixel variant again
        assert np.array_equal(_mosaic(imgs, src, params[src], cuts, H, W, 99, misalign=1), got)


@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)
def test_cut_at_the_corner_is_augment_u8_ragged_of_tile_0(H, W):
    imgs, params = mixed_table(H, W)
    n = len(imgs)
    # tiles 1..3: offset 0, the size of image 0, and a rectangle, a flip and factors no valid row has -- readable, never used
    garbage = np.repeat(make_params([(-5, 0, 1 << 30, -(1 << 30), 7, float("nan"), float("inf"), -1.0)]), n)
    params4 = np.stack([params, garbage, garbage, garbage], axis=1)
    src = np.stack([np.arange(n), *([np.zeros(n, int)] * 3)], axis=1)
    got = _mosaic(imgs, src, params4, [(H, W)] * n, H, W, 99)
    assert np.array_equal(got, _augment(imgs, params, H, W, 99))


@pytest.mark.parametrize("H,W", CANVASES)
def test_engine_single_canvases_same_bytes_as_augment_u8_batch(H, W):
    from test_gpu_letterbox import _engine
    imgs, params = mixed_table(H, W)
    n = len(imgs)
    _, eng = _engine((H, W), n=n)
    want = eng.augment_u8_batch(imgs, params, pad_value=99).cpu().numpy()
    src = np.repeat(np.arange(n)[:, None], 4, axis=1)
    got = eng.mosaic_u8_batch(imgs, src, np.repeat(params[:, None], 4, axis=1), [(H, W)] * n, pad_value=99)
    assert got.shape == (n, H, W, 3) and np.array_equal(got.cpu().numpy(), want)
    # a real mosaic batch through the engine: 6 distinct images, 8 canvases, the bytes of the C ABI path
    cuts = cuts_of(H, W)
    src = pick_tiles(len(cuts), 12) % 6
    rows = params[pick_tiles(len(cuts), 12)]
    got = eng.mosaic_u8_batch(imgs[:6], src, rows, cuts, pad_value=99).cpu().numpy()
    assert np.array_equal(got, _mosaic(imgs[:6], src, rows, cuts, H, W, 99))
    for bad in (dict(cuts=[(H + 1, W)] + cuts[1:]), dict(cuts=[(0, -1)] + cuts[1:]), dict(tile_src=src + 1), dict(tile_src=src - 1)):
        with pytest.raises(ValueError, match="mosaic_u8_batch"):
            eng.mosaic_u8_batch(imgs[:6], bad.get("tile_src", src), rows, bad.get("cuts", cuts), pad_value=99)
    for name, v in (("out_h", 0), ("out_w", -3), ("hue", float("nan")), ("sat", float("inf"))):
        broken = rows.copy()
        broken[name][3, 2] = v
        with pytest.raises(ValueError, match="mosaic_u8_batch"):
            eng.mosaic_u8_batch(imgs[:6], src, broken, cuts, pad_value=99)
    eng.close()


@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)
def test_geometry_same_bytes_as_mosaic_host(H, W):
    from yolo4hip.augment import mosaic_host
    imgs = sources(H)
    params = make_params(geometry_rows(H, W))
    cuts = cuts_of(H, W)
    src = pick_tiles(len(cuts), len(imgs), stride=1)
    got = _mosaic(imgs, src, params[src], cuts, H, W, 99)
    off_canvas = 0
    for i, cut in enumerate(cuts):
        assert np.array_equal(got[i], mosaic_host([imgs[k] for k in src[i]], params[src[i]], cut, (H, W), 99)), (cut, src[i])
        for q in range(4):
            if src[i, q] == 4:                                             # row 4 lies wholly off the canvas: its window is pad
                y0, y1, x0, x1 = window_of(q, cut, H, W)
                assert (got[i, y0:y1, x0:x1] == 99).all()
                off_canvas += (y1 - y0) * (x1 - x0)
    assert off_canvas > 0


@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)
def test_colour_vs_float64_oracle(H, W):
    imgs, params = colour_table(H, W)
    oracle = [AO.augment(img, p, (H, W), 128) for img, p in zip(imgs, params)]
    cuts = cuts_of(H, W)
    src = pick_tiles(len(cuts), len(imgs))
    got = _mosaic(imgs, src, params[src], cuts, H, W, 128)
    worst = diff = total = 0
    for i, cut in enumerate(cuts):
        want = compose([oracle[k][0] for k in src[i]], cut)
        inside = compose([oracle[k][1] for k in src[i]], cut)
        assert (got[i][~inside] == 128).all()
        m, d, t = differing(got[i], want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    share = diff / total
    print(f"device mosaic vs float64 oracle on {H} x {W}: max level difference", worst, "differing share", share, "of", total)
    note(f"device_vs_oracle_{H}x{W}", {"max_level_difference": worst, "differing_share": share, "bytes": total, "cap": SHARE_CAP})
    assert worst <= 1 and share <= SHARE_CAP


def test_shared_sources_same_bytes_as_copies():
    H, W = CANVASES[0]
    imgs, params = mixed_table(H, W)
    cuts = cuts_of(H, W)
    rows = params[pick_tiles(len(cuts), len(imgs))]
    # canvas 6: its four tiles are one image; images 2 and 3 serve tiles of several canvases
    src = np.array([[2, 3, 2, 3], [3, 2, 0, 1], [0, 1, 2, 3], [5, 2, 2, 3], [1, 1, 3, 3], [3, 4, 5, 2], [2, 2, 2, 2], [4, 3, 3, 2]])
    shared = _mosaic(imgs[:6], src, rows, cuts, H, W, 128)
    assert np.array_equal(shared, _mosaic(imgs[:6], src, rows, cuts, H, W, 128, shared=False))


def test_deterministic_and_independent_of_batch_and_slot():
    H, W = CANVASES[0]
    imgs, params = mixed_table(H, W)
    cuts = np.array(cuts_of(H, W))
    src = pick_tiles(len(cuts), len(imgs))
    rows = params[src]
    full = _mosaic(imgs, src, rows, cuts, H, W, 128)
    assert np.array_equal(full, _mosaic(imgs, src, rows, cuts, H, W, 128))
    for i in range(len(cuts)):
        assert np.array_equal(_mosaic(imgs, src[i:i + 1], rows[i:i + 1], cuts[i:i + 1], H, W, 128)[0], full[i])
    order = [7, 3, 0, 0, 6, 4]
    assert np.array_equal(_mosaic(imgs, src[order], rows[order], cuts[order], H, W, 128), full[order])


def test_argument_refusals_on_device_buffers():
    import torch
    from yolo4hip import ext
    lib = ext.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, s = ext.ptr(buf), ext.stream_ptr()
    f = lib.y4_mosaic_u8_ragged
    for args in ((None, p, p, 1, p, 8, 8, 128), (p, None, p, 1, p, 8, 8, 128), (p, p, None, 1, p, 8, 8, 128),
                 (p, p, p, 1, None, 8, 8, 128), (p, p, p, 0, p, 8, 8, 128), (p, p, p, 65536, p, 8, 8, 128),
                 (p, p, p, 1, p, 0, 8, 128), (p, p, p, 1, p, 8, -8, 128), (p, p, p, 1, p, 8, 8, -1), (p, p, p, 1, p, 8, 8, 256),
                 (p, p, p, 2000, p, 608, 608, 128)):
        assert f(*args, s) == -22
    torch.cuda.synchronize()
    assert not buf.any()                                                    # nothing ran


# ---- fit through the device path
@pytest.mark.parametrize("dtype,trainable", [("bf16", "heads"), ("bf16", "head_blocks")])
def test_fit_mosaic_is_reproducible(tmp_path, dtype, trainable):
    from yolo4hip.augment import AugmentConfig
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    h1, f1, _ = _fit(tmp_path / "a", dtype, trainable, AugmentConfig(mosaic=1.0), seed=5)
    h2, f2, _ = _fit(tmp_path / "b", dtype, trainable, AugmentConfig(mosaic=1.0), seed=5)
    print(dtype, trainable, "mosaic=1.0, seed 5:", h1)
    assert h1 == h2 and np.array_equal(f1.view(np.int32), f2.view(np.int32))
    assert np.isfinite(h1["loss"]).all() and len(h1["loss"]) == 2


def test_fit_mixed_batches_stay_finite(tmp_path):
    from yolo4hip.augment import AugmentConfig, draw_mosaic_params
    hist, _, _ = _fit(tmp_path, "bf16", "heads", AugmentConfig(mosaic=0.5), seed=1)
    print("mosaic=0.5, seed 1:", hist)
    assert np.isfinite(hist["loss"]).all() and len(hist["loss"]) == 2
    # the same stream again: the first batch (3 canvases) holds both kinds
    cuts = draw_mosaic_params(np.random.default_rng(1), 3, 5, (160, 160), AugmentConfig(mosaic=0.5))[2]
    single = (cuts == (160, 160)).all(axis=1)
    assert single.any() and not single.all()


def test_fit_mosaic_batch_with_every_box_dropped(tmp_path):
    """The pattern of tests/test_gpu_augment.py: test_fit_batch_with_every_box_dropped, with a scale range that drops every box
    of every tile whatever the shifts: scale 0.01..0.012 of a 160 x 160 canvas draws each 64 x 64 image at 2 x 2 px, and a box
    of less than half an image is then under 1 px wide.  Batches without a single box must train like any other."""
    from yolo4hip.augment import AugmentConfig
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    cfg = AugmentConfig(jitter=0.0, scale=(0.01, 0.012), flip=False, hue=0.0, sat=1.0, val=1.0, mosaic=1.0)
    hist, _, gen = _fit(tmp_path, "f32", "heads", cfg, seed=2, sizes=[(64, 64)] * 3, per_image=[1, 1, 1], epochs=4)
    assert np.isfinite(hist["loss"]).all() and len(hist["loss"]) == 4
    # the same stream again on a twin generator: none of the four batches had a box left
    twin = DataGenerator(gen.annotation_lines, gen.class_name_path, gen.folder_path, shuffle=False,
                         config=make_config(160, batch_size=3), augment=cfg, seed=2)
    for _ in range(4):
        _, _, params, _, boxes = twin.raw_mosaic(0)
        assert (params["out_h"] == 2).all() and (params["out_w"] == 2).all() and not boxes.any()
