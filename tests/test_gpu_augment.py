"""y4_augment_u8_ragged on the GPU (csrc/canvas_u8.hip) against y4_resize_u8_ragged, `augment.augment_host` and the float64
oracle of tests/augment_oracle.py, and `Yolov4.fit` over an augmenting `DataGenerator` (`Engine.augment_u8_batch`).

Geometry is integer arithmetic: byte identity.  Colour: every byte within 1 level of the float64 oracle and at most 1e-3 of
the bytes different at all, on the inputs of tests/test_augment_cpu.py (its docstring has the reasoning); the measured share is
written to profiles/fit/augment_measured.json."""
import os

import numpy as np
import pytest

import augment_oracle as AO
from helpers import CLASS_DIR
from test_augment_cpu import (CANVASES, SHARE_CAP, colour_table, differing, geometry_rows, make_params, natural_photo, note,
                              sources)
from test_gpu_letterbox import _ragged
from test_loss_cpu import _write_dataset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _augment(imgs, params, H, W, pad):
    """y4_augment_u8_ragged straight through the C ABI: packed sources + a descriptor table -> uint8 [n,H,W,3] on the host."""
    import torch
    from yolo4hip import ext
    lib = ext.load()
    n = len(imgs)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(DEV)
    desc = (ext.y4_augment_desc * n)()
    off = 0
    for d, a, p in zip(desc, imgs, params):
        d.offset, d.h, d.w = off, a.shape[0], a.shape[1]
        d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
        d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])
        off += a.size
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
    out = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    ext.check(lib.y4_augment_u8_ragged(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(out), H, W, pad, ext.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", CANVASES + [(37, 61)])                      # (37, 61): H * W % 4 != 0, one pixel per thread
def test_identity_rows_same_bytes_as_resize_u8_ragged(H, W):
    from yolo4hip import prepost
    imgs = sources(H + W)
    for rects in ([(H, W, 0, 0)] * len(imgs), [prepost.letterbox_rect(a.shape[0], a.shape[1], H, W) for a in imgs],
                  [(H - 9, W - 6, 3, 5)] * len(imgs)):
        got = _augment(imgs, make_params([r + (0, 0, 1, 1) for r in rects]), H, W, 128)
        assert np.array_equal(got, _ragged(imgs, H, W, rects, 128))


@pytest.mark.parametrize("H,W", CANVASES + [(37, 61)])
def test_flip_and_rectangles_off_the_canvas_same_bytes_as_host(H, W):
    from yolo4hip.augment import augment_host
    imgs = sources(H)
    params = make_params(geometry_rows(H, W))
    got = _augment(imgs, params, H, W, 99)
    for i, (img, p) in enumerate(zip(imgs, params)):
        assert np.array_equal(got[i], augment_host(img, p, (H, W), 99)), i
    assert (got[4] == 99).all()                                            # wholly off the canvas


@pytest.mark.parametrize("H,W", CANVASES)
def test_colour_vs_float64_oracle(H, W):
    imgs, params = colour_table(H, W)
    got = _augment(imgs, params, H, W, 128)
    worst = diff = total = 0
    for i, (img, p) in enumerate(zip(imgs, params)):
        want, inside = AO.augment(img, p, (H, W), 128)
        assert (got[i][~inside] == 128).all()
        m, d, t = differing(got[i], want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    share = diff / total
    print(f"device vs float64 oracle on {H} x {W}: max level difference", worst, "differing share", share, "of", total, "bytes")
    note(f"device_vs_oracle_{H}x{W}", {"max_level_difference": worst, "differing_share": share, "bytes": total, "cap": SHARE_CAP})
    assert worst <= 1 and share <= SHARE_CAP
    # drawn factors on the photograph as it is, resampled
    from yolo4hip.augment import AugmentConfig, draw_params
    photo = natural_photo()
    drawn = draw_params(np.random.default_rng(7), [photo.shape[:2]] * 8, (H, W), AugmentConfig())
    got = _augment([photo] * 8, drawn, H, W, 128)
    worst = diff = total = 0
    for i, p in enumerate(drawn):
        want, inside = AO.augment(photo, p, (H, W), 128)
        m, d, t = differing(got[i], want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    print(f"drawn factors on {H} x {W}: max level difference", worst, "differing bytes", diff, "of", total)
    note(f"device_vs_oracle_drawn_{H}x{W}", {"max_level_difference": worst, "differing_share": diff / max(total, 1), "bytes": total})
    assert worst <= 1 and diff <= SHARE_CAP * total


def test_deterministic_and_independent_of_batch_and_slot():
    H, W = CANVASES[0]
    imgs = sources(1)
    rows = geometry_rows(H, W)
    for k, r in enumerate(rows):                                            # colour on top of the geometry
        rows[k] = r[:5] + ((0.07, 1.3, 0.8) if k % 2 else (-0.04, 0.75, 1.2))
    params = make_params(rows)
    full = _augment(imgs, params, H, W, 128)
    assert np.array_equal(full, _augment(imgs, params, H, W, 128))
    for i in range(len(imgs)):
        assert np.array_equal(_augment(imgs[i:i + 1], params[i:i + 1], H, W, 128)[0], full[i])
    order = [5, 3, 0, 0, 2]
    again = _augment([imgs[i] for i in order], params[order], H, W, 128)
    assert np.array_equal(again, full[order])


@pytest.mark.parametrize("entry", ["y4_resize_u8_ragged", "y4_augment_u8_ragged"])
def test_output_off_a_dword_same_bytes_and_guards_untouched(entry):
    """An output one byte into a larger buffer takes the one-pixel-per-thread store (H * W % 4 == 0 here, so the aligned call
    stores dwords): the same bytes, and the bytes before and behind the batch stay as they were.  Mixed sizes with 1 x N, N x 1
    and one image of the canvas's size; the augment rows carry flip, colour and rectangles off the canvas."""
    import torch
    from yolo4hip import ext, prepost
    from test_gpu_letterbox import _images
    H, W = 96, 160
    imgs = _images([(1, 77), (77, 1), (H, W), (333, 501), (45, 37), (200, 90)], seed=96160)
    n, size = len(imgs), len(imgs) * H * W * 3
    if entry == "y4_resize_u8_ragged":
        desc = (ext.y4_image_desc * n)()
        rects = [prepost.letterbox_rect(a.shape[0], a.shape[1], H, W) for a in imgs[:3]] + [(H, W, 0, 0), (H - 9, W - 6, 3, 5), (H, W, 0, 0)]
        for d, r in zip(desc, rects):
            d.out_h, d.out_w, d.pad_top, d.pad_left = r
    else:
        desc = (ext.y4_augment_desc * n)()
        rows = [(H, W, 0, 0, 1, 0, 1, 1), (H + 9, W + 13, -4, -7, 0, 0.07, 1.3, 0.8), (H, W, 0, 0, 0, 0, 1, 1),
                (H - 11, W + 30, 5, -17, 1, -0.04, 0.75, 1.2), (7, 5, H - 3, W - 2, 1, 0, 1, 1), (H + 21, W - 5, -13, 3, 0, 0, 1, 1.1)]
        for d, p in zip(desc, make_params(rows)):
            d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
            d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])
    off = 0
    for d, a in zip(desc, imgs):
        d.offset, d.h, d.w = off, a.shape[0], a.shape[1]
        off += a.size
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(DEV)
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
    fn = getattr(ext.load(), entry)
    aligned = torch.full((size,), 7, dtype=torch.uint8, device=DEV)
    assert aligned.data_ptr() % 4 == 0
    ext.check(fn(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(aligned), H, W, 128, ext.stream_ptr()))
    flat = torch.full((size + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    assert flat[1:].data_ptr() % 4 == 1
    ext.check(fn(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(flat[1:]), H, W, 128, ext.stream_ptr()))
    torch.cuda.synchronize()
    aligned, flat = aligned.cpu().numpy(), flat.cpu().numpy()
    assert np.array_equal(flat[1:1 + size], aligned)
    assert flat[0] == 0xA5 and (flat[1 + size:] == 0xA5).all()
    got = aligned.reshape(n, H, W, 3)
    assert np.array_equal(got[2], imgs[2])                                  # the image of the canvas's size, unflipped, uncoloured
    assert (got != 7).any(axis=-1).mean() > 0.99                            # the aligned call wrote the batch


def test_argument_refusals_on_device_buffers():
    import torch
    from yolo4hip import ext
    lib = ext.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, s = ext.ptr(buf), ext.stream_ptr()
    f = lib.y4_augment_u8_ragged
    for args in ((None, p, 1, p, 8, 8, 128), (p, None, 1, p, 8, 8, 128), (p, p, 1, None, 8, 8, 128), (p, p, 0, p, 8, 8, 128),
                 (p, p, 65536, p, 8, 8, 128), (p, p, 1, p, 0, 8, 128), (p, p, 1, p, 8, -8, 128), (p, p, 1, p, 8, 8, -1),
                 (p, p, 1, p, 8, 8, 256), (p, p, 2000, p, 608, 608, 128)):
        assert f(*args, s) == -22
    torch.cuda.synchronize()
    assert not buf.any()                                                    # nothing ran


# ---- fit through the device path
def _fit(tmp_path, dtype, trainable, augment, seed=None, sizes=None, per_image=None, epochs=2):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    m = Yolov4(None, names, make_config(160, batch_size=3), dtype=dtype, max_batch=2, synth_seed=3, tune=False)
    sizes = sizes or [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64)]
    lines = _write_dataset(tmp_path, sizes, per_image or [3, 0, 5, 8, 1])
    gen = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=m.config, augment=augment, seed=seed)
    np.random.seed(11)
    hist = m.fit(gen, epochs, trainable=trainable, learning_rate=1e-3)
    flat = m._flat.copy()
    m.engine.close()
    return hist.history, flat, gen


@pytest.mark.parametrize("dtype,trainable", [("f32", "heads"), ("bf16", "heads"), ("bf16", "head_blocks")])
def test_fit_identity_config_is_the_host_path(tmp_path, dtype, trainable):
    from yolo4hip.augment import AugmentConfig
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    plain_hist, plain_flat, _ = _fit(tmp_path / "a", dtype, trainable, None)
    hist, flat, _ = _fit(tmp_path / "b", dtype, trainable, AugmentConfig.identity(), seed=1)
    print(dtype, trainable, "augment=None:", plain_hist, "identity config:", hist)
    assert hist == plain_hist
    assert np.array_equal(flat.view(np.int32), plain_flat.view(np.int32))


def test_fit_default_config_is_reproducible(tmp_path):
    from yolo4hip.augment import AugmentConfig
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
    h1, f1, _ = _fit(tmp_path / "a", "bf16", "heads", AugmentConfig(), seed=5, epochs=3)
    h2, f2, _ = _fit(tmp_path / "b", "bf16", "heads", AugmentConfig(), seed=5, epochs=3)
    print("default config, seed 5:", h1)
    assert h1 == h2 and np.array_equal(f1.view(np.int32), f2.view(np.int32))
    assert np.isfinite(h1["loss"]).all() and len(h1["loss"]) == 3


def test_fit_batch_with_every_box_dropped(tmp_path):
    """scale 4..4.5 of a 160 x 160 canvas: boxes of at most half an image in its top-left quarter, drawn at >= 640 px with a pad
    that may reach -480 -- so some batches lose every box; one whose boxes are all gone must train like any other."""
    from yolo4hip.augment import AugmentConfig, draw_params, transform_boxes
    cfg = AugmentConfig(jitter=0.0, scale=(4.0, 4.5), flip=False, hue=0.0, sat=1.0, val=1.0)
    hist, _, gen = _fit(tmp_path, "f32", "heads", cfg, seed=2, sizes=[(64, 64)] * 3, per_image=[1, 1, 1], epochs=4)
    assert np.isfinite(hist["loss"]).all() and len(hist["loss"]) == 4
    # the same stream again: at least one of the four batches had no box left
    rng, lines, empty = np.random.default_rng(2), gen.annotation_lines, 0
    for _ in range(4):
        params = draw_params(rng, [(64, 64)] * 3, (160, 160), cfg)
        left = 0
        for line, p in zip(lines, params):
            raw = np.array([[float(v) for v in f.split(',')] for f in line.split()[1:]], np.float32)
            left += int((transform_boxes(raw, (64, 64), p, (160, 160), 100)[:, 2] > 0).sum())
        empty += left == 0
    assert empty >= 1
