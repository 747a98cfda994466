"""Mosaic off the device (yolo4hip/augment.py: draw_mosaic_params, mosaic_boxes, mosaic_host; DataGenerator.raw_mosaic) and the
host-side refusals of y4_mosaic_u8_ragged.  No GPU.

The rule is a composition: canvas pixel (y, x) is pixel (y, x) of the single-image augmentation of tile
q = 2 (y >= cut_y) + (x >= cut_x).  `compose` states it as np.where over four whole canvases, and every image check here holds
`mosaic_host` to that, byte for byte, with `augment_host` as the yardstick.  Against the float64 oracle the bound is the one of
tests/test_augment_cpu.py (1 level, SHARE_CAP of the bytes) on the same inputs (`colour_table`): the composition picks bytes, it
computes none, so the share of a mosaic is a mean of shares that each lie under the cap.  The measured shares are written to
profiles/fit/mosaic_measured.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import augment_oracle as AO
from helpers import CLASS_DIR, ROOT
from test_augment_cpu import CANVASES, SHARE_CAP, colour_table, differing, geometry_rows, make_params, sources
from test_loss_cpu import _write_dataset

MOSAIC_CANVASES = CANVASES + [(37, 61)]                  # (37, 61): H * W % 4 != 0


def note(key, value):
    path = os.path.join(ROOT, "profiles", "fit", "mosaic_measured.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc[key] = value
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


def cuts_of(H, W):
    """(cut_y, cut_x): the four corners (one tile alone), one-pixel windows on either side, and two cuts whose cut_x is no
    multiple of 4 (a thread's four pixels lie on both sides of it)."""
    return [(0, 0), (H, W), (0, W), (H, 0), (1, 1), (H - 1, W - 1), (23, 41), (H // 2, 50)]


def tile_of(cut, H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return 2 * (y >= cut[0]) + (x >= cut[1])


def compose(canvases4, cut):
    """np.where over four [H,W,...] arrays by the tile of every pixel."""
    H, W = canvases4[0].shape[:2]
    q = tile_of(cut, H, W).reshape((H, W) + (1,) * (canvases4[0].ndim - 2))
    out = canvases4[0]
    for k in (1, 2, 3):
        out = np.where(q == k, canvases4[k], out)
    return out


def window_of(q, cut, H, W):
    return [(0, cut[0], 0, cut[1]), (0, cut[0], cut[1], W), (cut[0], H, 0, cut[1]), (cut[0], H, cut[1], W)][q]


def mixed_table(H, W):
    """(images, rows) to pick tiles from: the six geometry rows of `geometry_rows` on `sources`, then the same six with a colour
    transform on top."""
    imgs = sources(H)
    rows = geometry_rows(H, W)
    coloured = [r[:5] + ((0.07, 1.3, 0.8) if k % 2 else (-0.04, 0.75, 1.2)) for k, r in enumerate(rows)]
    return imgs + imgs, make_params(rows + coloured)


def pick_tiles(count, pool, stride=5):
    """tile_src [count,4] into a pool of `pool` rows: canvas c takes rows c, c + stride, c + 2 stride, c + 3 stride (mod pool)."""
    return np.array([[(c + q * stride) % pool for q in range(4)] for c in range(count)])


# ---- mosaic_host
@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)
def test_mosaic_host_is_the_composition(H, W):
    from yolo4hip.augment import augment_host, mosaic_host
    imgs, params = mixed_table(H, W)
    singles = [augment_host(img, p, (H, W), 99) for img, p in zip(imgs, params)]
    cuts = cuts_of(H, W)
    for cut, src in zip(cuts, pick_tiles(len(cuts), len(imgs))):
        got = mosaic_host([imgs[k] for k in src], params[src], cut, (H, W), 99)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3)
        assert np.array_equal(got, compose([singles[k] for k in src], cut)), (cut, src)
    # the cut (H, W) is tile 0 alone; an image behind an empty window is not touched
    assert np.array_equal(mosaic_host([imgs[7], None, None, None], params[[7, 0, 0, 0]], (H, W), (H, W), 99), singles[7])
    assert np.array_equal(mosaic_host([None, None, None, imgs[8]], params[[0, 0, 0, 8]], (0, 0), (H, W), 99), singles[8])


@pytest.mark.parametrize("H,W", MOSAIC_CANVASES)
def test_mosaic_host_colour_vs_float64_oracle(H, W):
    from yolo4hip.augment import mosaic_host
    imgs, params = colour_table(H, W)
    oracle = [AO.augment(img, p, (H, W), 128) for img, p in zip(imgs, params)]
    worst = diff = total = 0
    cuts = cuts_of(H, W)
    for cut, src in zip(cuts, pick_tiles(len(cuts), len(imgs))):
        want = compose([oracle[k][0] for k in src], cut)
        inside = compose([oracle[k][1] for k in src], cut)
        got = mosaic_host([imgs[k] for k in src], params[src], cut, (H, W), 128)
        assert (got[~inside] == 128).all()
        m, d, t = differing(got, want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    share = diff / total
    print(f"mosaic_host vs float64 oracle on {H} x {W}: max level difference", worst, "differing share", share, "of", total)
    note(f"host_vs_oracle_{H}x{W}", {"max_level_difference": worst, "differing_share": share, "bytes": total, "cap": SHARE_CAP})
    assert worst <= 1 and share <= SHARE_CAP


# ---- draw_mosaic_params
def _visible(lo_pad, size, side, flip):
    """The canvas coordinates the single-image rule maps into [0, size), by its own index arithmetic, evaluated on a range wide
    enough to hold any rectangle: (first, one past the last)."""
    x = np.arange(-2 * (side + size), 2 * (side + size))
    xx = (side - 1 - x if flip else x) - lo_pad
    hit = x[(xx >= 0) & (xx < size)]
    assert len(hit) == size and hit[-1] - hit[0] == size - 1
    return int(hit[0]), int(hit[-1]) + 1


def test_draw_mosaic_params_seed_cuts_and_positions():
    from yolo4hip.augment import AugmentConfig, draw_mosaic_params, draw_params
    cfg = AugmentConfig(mosaic=1.0)
    a = draw_mosaic_params(np.random.default_rng(5), 6, 11, (64, 96), cfg)
    b = draw_mosaic_params(np.random.default_rng(5), 6, 11, (64, 96), cfg)
    c = draw_mosaic_params(np.random.default_rng(6), 6, 11, (64, 96), cfg)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[1].tobytes() != c[1].tobytes()
    assert a[0].shape == (6, 4) and a[1].shape == (6, 4) and a[2].shape == (6, 2) and a[2].dtype == np.int32
    for (H, W), center in [((64, 96), (0.2, 0.8)), ((416, 608), (0.2, 0.8)), ((37, 61), (0.0, 1.0)), ((96, 64), (0.45, 0.55))]:
        cfg = AugmentConfig(mosaic=1.0, mosaic_center=center)
        src, params, cuts = draw_mosaic_params(np.random.default_rng(H), 200, 7, (H, W), cfg)
        lo, hi = center
        assert (cuts[:, 0] >= np.rint(lo * H)).all() and (cuts[:, 0] <= np.rint(hi * H)).all()
        assert (cuts[:, 1] >= np.rint(lo * W)).all() and (cuts[:, 1] <= np.rint(hi * W)).all()
        assert len(np.unique(cuts[:, 0])) > 3 and len(np.unique(cuts[:, 1])) > 3
        assert (src[:, 0] == -1).all() and (src[:, 1:] >= 0).all() and (src[:, 1:] < 7).all()
        assert set(np.unique(src[:, 1:])) == set(range(7))
        assert set(np.unique(params["flip"])) == {0, 1}
        inside = covers = 0
        for i in range(len(cuts)):
            for q in range(4):
                p = params[i, q]
                y0, y1, x0, x1 = window_of(q, cuts[i], H, W)
                for first, size, a0, a1, flip, side in ((p["pad_left"], p["out_w"], x0, x1, p["flip"], W),
                                                        (p["pad_top"], p["out_h"], y0, y1, 0, H)):
                    L, R = _visible(int(first), int(size), side, int(flip))
                    if size <= a1 - a0:
                        assert a0 <= L and R <= a1, (i, q, p, cuts[i])
                        inside += 1
                    else:
                        assert L <= a0 and R >= a1, (i, q, p, cuts[i])
                        covers += 1
        assert inside > 0 and covers > 0
    # the identity config in every tile: each rectangle has the canvas's size (it covers its window, wherever the shift puts it)
    ident = AugmentConfig(jitter=0, scale=(1, 1), flip=False, hue=0, sat=1, val=1, mosaic=1.0)
    _, params, _ = draw_mosaic_params(np.random.default_rng(1), 50, 7, (64, 96), ident)
    for name, v in (("out_h", 64), ("out_w", 96), ("flip", 0), ("hue", 0), ("sat", 1), ("val", 1)):
        assert (params[name] == v).all(), name
    # centre (1, 1): every canvas is cut at (H, W)
    cfg = AugmentConfig(mosaic=1.0, mosaic_center=(1, 1))
    assert (draw_mosaic_params(np.random.default_rng(2), 40, 7, (64, 96), cfg)[2] == (64, 96)).all()
    # a single canvas: the coin, then one draw_params row; rows 1..3 copy it; nothing else is drawn
    cfg = AugmentConfig(mosaic=0.0)
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    src, params, cuts = draw_mosaic_params(r1, 3, 7, (64, 96), cfg)
    for i in range(3):
        r2.uniform()
        want = draw_params(r2, [None], (64, 96), cfg)[0]
        assert all(params[i, q].tobytes() == want.tobytes() for q in range(4))
    assert (cuts == (64, 96)).all() and (src == -1).all() and r1.uniform() == r2.uniform()
    # a mix: both kinds in one call, singles at (H, W) only
    cfg = AugmentConfig(mosaic=0.5)
    src, params, cuts = draw_mosaic_params(np.random.default_rng(3), 200, 7, (64, 96), cfg)
    single = (src[:, 1] < 0)
    assert 60 < single.sum() < 140 and (cuts[single] == (64, 96)).all() and (cuts[~single] < (64, 96)).all()


def test_generator_without_mosaic_draws_as_before(tmp_path):
    from yolo4hip.augment import AugmentConfig, draw_params
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    sizes = [(120, 200), (160, 160), (90, 64), (64, 64)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 1])
    cfg = make_config((96, 160), batch_size=2)
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    gen = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=AugmentConfig(), seed=5)
    assert gen.augment.mosaic == 0 and AugmentConfig.identity().mosaic == 0
    rng = np.random.default_rng(5)
    for i in range(2):
        want = draw_params(rng, sizes[2 * i:2 * i + 2], (96, 160), AugmentConfig())
        assert gen.raw(i)[1].tobytes() == want.tobytes()
    assert gen.rng.uniform() == rng.uniform()
    with pytest.raises(ValueError, match="raw_mosaic"):
        gen.raw_mosaic(0)


# ---- mosaic_boxes
def test_mosaic_boxes_hand_cases():
    from yolo4hip.augment import mosaic_boxes
    H, W = 64, 96
    plain, flipped = (H, W, 0, 0, 0, 0, 1, 1), (H, W, 0, 0, 1, 0, 1, 1)   # images of the canvas's size: boxes stay where they are
    params4 = make_params([plain, flipped, plain, plain])
    sizes = [(H, W)] * 4
    boxes = [np.array([[10, 5, 60, 40, 0],          # tile 0, straddles the cut both ways: clipped to x2 48, y2 32
                       [47.5, 5, 70, 20, 1]]),      # half a pixel left in the window: dropped
             np.array([[10, 10, 30, 20, 2]]),       # tile 1, flipped: x1, x2 <- 96 - 30, 96 - 10
             np.array([[0, 0, 20, 20, 1],           # tile 2: wholly above the cut, dropped
                       [5, 40, 25, 60, 1]]),
             np.array([[50, 40, 90, 60, 0],
                       [40, 30, 60, 50, 2]])]       # tile 3, straddles: clipped to x1 48, y1 32
    got = mosaic_boxes(boxes, sizes, params4, (32, 48), (H, W), 8)
    assert got.dtype == np.float32 and got.shape == (8, 5)
    want = [[10, 5, 48, 32, 0], [66, 10, 86, 20, 2], [5, 40, 25, 60, 1], [50, 40, 90, 60, 0], [48, 32, 60, 50, 2]]
    assert got[:5].tolist() == want and not got[5:].any()                  # tile order 0, 1, 2, 3
    got = mosaic_boxes(boxes, sizes, params4, (32, 48), (H, W), 3)
    assert got.shape == (3, 5) and got.tolist() == want[:3]                # cut at max_boxes
    # cut_y = 0: tiles 0 and 1 have no window and contribute nothing; tiles 2 and 3 reach the top of the canvas
    got = mosaic_boxes(boxes, sizes, params4, (0, 48), (H, W), 8)
    assert got[:4].tolist() == [[0, 0, 20, 20, 1], [5, 40, 25, 60, 1], [50, 40, 90, 60, 0], [48, 30, 60, 50, 2]]
    assert not got[4:].any()
    # the cut (H, W) is transform_boxes of tile 0
    from yolo4hip.augment import transform_boxes
    p = make_params([(80, 120, -10, -20, 1, 0, 1, 1)] * 4)
    raw = np.array([[5, 10, 20, 20, 0], [40, 10, 58, 20, 1], [0, 0, 9, 4, 1]], np.float32)
    assert np.array_equal(mosaic_boxes([raw, raw[:1], raw[:1], raw[:1]], [(32, 48)] * 4, p, (H, W), (H, W), 8),
                          transform_boxes(raw, (32, 48), p[0], (H, W), 8))
    assert not mosaic_boxes([np.zeros((0, 5))] * 4, sizes, params4, (32, 48), (H, W), 8).any()


def test_mosaic_boxes_lie_in_their_windows():
    from yolo4hip.augment import AugmentConfig, draw_mosaic_params, mosaic_boxes
    H, W, mb = 96, 160, 12
    rng = np.random.default_rng(4)
    _, params, cuts = draw_mosaic_params(np.random.default_rng(2), 150, 9, (H, W), AugmentConfig(mosaic=1.0))
    kept = 0
    none = np.zeros((0, 5), np.float32)
    for p4, cut in zip(params, cuts):
        sizes = [(int(rng.integers(8, 400)), int(rng.integers(8, 400))) for _ in range(4)]
        raws = []
        for h, w in sizes:
            x1, y1 = rng.uniform(0, w - 2, mb), rng.uniform(0, h - 2, mb)
            raws.append(np.stack([x1, y1, rng.uniform(x1, w), rng.uniform(y1, h), rng.integers(0, 3, mb)], -1).astype(np.float32))
        parts = []
        for q in range(4):                                                    # one tile's boxes at a time
            only = [raws[k] if k == q else none for k in range(4)]
            b = mosaic_boxes(only, sizes, p4, cut, (H, W), 4 * mb)
            b = b[b[:, 2] > b[:, 0]]
            y0, y1, x0, x1 = window_of(q, cut, H, W)
            assert (b[:, 0] >= x0).all() and (b[:, 2] <= x1).all() and (b[:, 1] >= y0).all() and (b[:, 3] <= y1).all()
            assert (b[:, 2] - b[:, 0] > 1).all() and (b[:, 3] - b[:, 1] > 1).all()
            parts.append(b)
        both = mosaic_boxes(raws, sizes, p4, cut, (H, W), 4 * mb)
        rows = np.concatenate(parts)
        assert np.array_equal(both[:len(rows)], rows) and not both[len(rows):].any()
        kept += len(rows)
    assert 0 < kept < 150 * 4 * mb


# ---- the generator
def test_generator_raw_mosaic_and_host_path(tmp_path):
    from yolo4hip import prepost
    from yolo4hip.augment import AugmentConfig, mosaic_host
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 8, 1])
    cfg = make_config((96, 160), batch_size=3)
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    H, W = 96, 160
    for mosaic in (1.0, 0.5):
        aug = AugmentConfig(mosaic=mosaic)
        a = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=aug, seed=5)
        b = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=aug, seed=5)
        with pytest.raises(ValueError, match="raw_mosaic"):
            a.raw(0)
        for batch, own in ((0, [0, 1, 2]), (1, [3, 4])):
            np.random.seed(3)
            imgs, tile_src, params, cuts, boxes = a.raw_mosaic(batch)
            n = len(own)
            assert tile_src.shape == (n, 4) and params.shape == (n, 4) and cuts.shape == (n, 2)
            assert boxes.shape == (n, 100, 5) and boxes.dtype == np.float32
            assert tile_src.min() == 0 and tile_src.max() == len(imgs) - 1 and set(tile_src.reshape(-1)) == set(range(len(imgs)))
            assert tile_src[:, 0].tolist() == list(range(n))                 # the own images first, in batch order
            files = [prepost.imread_rgb(os.path.join(str(tmp_path), line.split()[0])) for line in lines]
            for i, j in enumerate(own):
                assert np.array_equal(imgs[i], files[j])
            which = [[k for k, f in enumerate(files) if f.shape == img.shape and np.array_equal(f, img)] for img in imgs]
            assert all(len(w) == 1 for w in which) and len({w[0] for w in which}) == len(imgs)       # distinct photos
            single = (cuts == (H, W)).all(axis=1)
            assert (tile_src[single] == tile_src[single][:, :1]).all()
            if mosaic == 1.0:
                assert not single.any()
            np.random.seed(3)
            X, bb = b.boxes(batch)
            assert np.array_equal(bb.view(np.int32), boxes.view(np.int32))
            for i in range(n):
                want = (mosaic_host([imgs[k] for k in tile_src[i]], params[i], cuts[i], (H, W), 128) / 255.).astype(np.float32)
                assert np.array_equal(X[i].view(np.int32), want.view(np.int32))
        np.random.seed(3)
        (Xb, y_s, y_m, y_l, xywh), zeros = b[0]
        assert Xb.shape == (3, H, W, 3) and xywh.shape == (3, 100, 4) and y_s.shape == (3, 12, 20, 3, 8)


# ---- the C ABI without a device
def test_mosaic_abi_and_host_checks():
    from yolo4hip import ext
    lib = ext.load()
    assert C.sizeof(ext.y4_mosaic_cut) == 8 and ext.y4_mosaic_cut.cut_y.offset == 0 and ext.y4_mosaic_cut.cut_x.offset == 4
    EINVAL = -22
    p = C.c_void_p(4096)                                  # never dereferenced: every case returns before a launch
    f = lib.y4_mosaic_u8_ragged
    assert f(None, p, p, 1, p, 608, 608, 128, None) == EINVAL and f(p, None, p, 1, p, 608, 608, 128, None) == EINVAL
    assert f(p, p, None, 1, p, 608, 608, 128, None) == EINVAL and b"mosaic_u8_ragged" in lib.y4_last_error()
    assert f(p, p, p, 1, None, 608, 608, 128, None) == EINVAL and b"mosaic_u8_ragged" in lib.y4_last_error()
    for n in (0, -1, 65536):
        assert f(p, p, p, n, p, 608, 608, 128, None) == EINVAL
    for H, W in ((0, 608), (608, 0), (-32, 608)):
        assert f(p, p, p, 1, p, H, W, 128, None) == EINVAL
    for pad in (-1, 256):
        assert f(p, p, p, 1, p, 608, 608, pad, None) == EINVAL
    assert f(p, p, p, 2000, p, 608, 608, 128, None) == EINVAL                # 2000 x 608 x 608 x 3 >= 2^31 bytes


def test_augment_config_refuses_mosaic_fields_out_of_range():
    from yolo4hip.augment import AugmentConfig
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mosaic"):
            AugmentConfig(mosaic=bad)
    for bad in ((0.5, 0.2), (-0.1, 0.5), (0.2, 1.1), (0.5,), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="mosaic_center"):
            AugmentConfig(mosaic_center=bad)
    cfg = AugmentConfig(mosaic=1, mosaic_center=(0, 1))
    assert cfg.mosaic == 1 and AugmentConfig().mosaic == 0 and AugmentConfig().mosaic_center == (0.2, 0.8)
    assert AugmentConfig.identity().mosaic == 0
