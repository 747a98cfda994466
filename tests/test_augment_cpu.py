"""Augmentation off the device (yolo4hip/augment.py, DataGenerator(augment=, seed=)): the float64 oracle against `colorsys`,
`augment_host` against the oracle, `draw_params`, `transform_boxes`, the generator, and the host-side refusals of
y4_augment_u8_ragged.  No GPU.

Colour tolerance: the float32 chain of the colour rule carries about 1e-4 of a level, so a byte may differ from the float64
oracle only where 255 c + 0.5 lies that close to an integer: at most 1 level anywhere, and on at most 1e-3 of the bytes.  The
prescribed factors (hue +-0.1, sat and val 1.5 and 1 / 1.5) are small rationals, and 255 x 6 x 0.1 = 153 is an integer: on
arbitrary integer levels a few per cent of the outputs are EXACT ties, 255 c = k + 1/2, where float64 itself is decided by
its rounding noise (measured with these factors on the unquantised photograph: 4-11 % of the bytes one level apart).  The
cap is a condition on the inputs: the colour sources hold the levels 60, 80 .. 160 only, at their own size (no resampling).
Then max <= 160 and max - min <= 0.625 max, so neither clamp is reached (1.5 x 160 < 255, 1.5 x 0.625 < 1), and every output
is a sum of multiples of 20 times 1.5, 2.25, 1.35, 0.9, 0.6 or 1 -- integers -- and of thirds: never within 1/6 of a tie.
A second comparison uses drawn (non-dyadic) factors on the photograph as it is, resampled.  The measured shares are written
to profiles/fit/augment_measured.json."""
import colorsys
import ctypes as C
import itertools
import json
import os
import types

import numpy as np
import pytest

import augment_oracle as AO
from helpers import CLASS_DIR, GOLDEN, ROOT
from test_loss_cpu import _write_dataset

CANVASES = [(64, 96), (96, 64)]
SIZES = [(37, 53), (120, 200), (64, 96), (1, 1), (200, 31), (96, 64)]
COLOUR_CASES = list(itertools.product((0.1, -0.1), (1.5, 1 / 1.5), (1.5, 1 / 1.5)))      # (hue, sat, val)
SHARE_CAP = 1e-3


def note(key, value):
    path = os.path.join(ROOT, "profiles", "fit", "augment_measured.json")
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


def sources(seed=0):
    """The six sources of SIZES: blocks of random colour with noise, so that bilinear taps hit real gradients."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SIZES:
        base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
        img = np.kron(base, np.ones((8, 8, 1)))[:h, :w] + rng.integers(-20, 21, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def colour_sources():
    """Seeded noise and the street photograph on the levels 60, 80 .. 160 (module docstring)."""
    from yolo4hip import prepost
    street = prepost.imread_rgb(os.path.join(GOLDEN, "street.jpeg"))[:120, :200].astype(np.int64)
    street = np.clip((street + 10) // 20 * 20, 60, 160).astype(np.uint8)
    noise = (np.random.default_rng(0).integers(3, 9, (37, 53, 3)) * 20).astype(np.uint8)
    return [street, noise]


def natural_photo():
    from yolo4hip import prepost
    return prepost.imread_rgb(os.path.join(GOLDEN, "street.jpeg"))


def make_params(rows):
    """rows of (out_h, out_w, pad_top, pad_left, flip, hue, sat, val) -> PARAM_DTYPE array"""
    from yolo4hip.augment import PARAM_DTYPE
    return np.array([tuple(r) for r in rows], dtype=PARAM_DTYPE)


def colour_table(H, W):
    """(images, params): every colour case on both colour sources at their own size, the photograph cut by the canvas at a
    negative pad, the noise inside it; flip alternates."""
    street, noise = colour_sources()
    imgs, rows = [], []
    for k, (hue, sat, val) in enumerate(COLOUR_CASES):
        imgs += [street, noise]
        rows += [(120, 200, -5, -3, k & 1, hue, sat, val), (37, 53, 7, 9, 1 - (k & 1), hue, sat, val)]
    return imgs, make_params(rows)


def geometry_rows(H, W):
    """One row per source of SIZES: flip, negative pads, out_w > W, out_h > H, one wholly off the canvas, the 1 x 1 source, edges
    that are no multiples of 4."""
    return [(H + 9, W + 13, -4, -7, 1, 0, 1, 1), (H - 11, W + 30, 5, -17, 0, 0, 1, 1), (H + 21, W - 5, -13, 3, 1, 0, 1, 1),
            (7, 5, H - 3, W - 2, 1, 0, 1, 1), (33, 41, -40, 10, 0, 0, 1, 1), (H, W, 0, 0, 1, 0, 1, 1)]


def differing(got, want, inside):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    return int(d.max()), int((d[inside] != 0).sum()), int(inside.sum()) * 3


# ---- the oracle
def test_oracle_hsv_is_colorsys():
    rng = np.random.default_rng(1)
    px = rng.integers(0, 256, (3000, 3)).astype(np.float64)
    special = [(0, 0, 0), (255, 255, 255), (77, 77, 77), (255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 200, 10), (10, 200, 200),
               (200, 10, 200), (9, 9, 8), (1, 0, 0), (255, 255, 0)]
    px = np.concatenate([px, np.array(special, dtype=np.float64)]) / 255.0
    h, s, v = AO.rgb_to_hsv(px)
    want = np.array([colorsys.rgb_to_hsv(*p) for p in px])
    assert np.abs(np.stack([h, s, v], -1) - want).max() <= 1e-12
    hsv = np.concatenate([rng.uniform(0, 1, (3000, 3)), [[0, 0, 0.5], [0.999999, 1, 1], [0.5, 0, 1], [1 / 6, 1, 0.3], [0, 1, 1]]])
    got = AO.hsv_to_rgb(hsv[:, 0], hsv[:, 1], hsv[:, 2])
    want = np.array([colorsys.hsv_to_rgb(*p) for p in hsv])
    assert np.abs(got - want).max() <= 1e-12


# ---- augment_host
@pytest.mark.parametrize("H,W", CANVASES)
def test_augment_host_geometry_same_bytes_as_oracle(H, W):
    from yolo4hip import prepost
    from yolo4hip.augment import augment_host
    imgs = sources(H)
    for img, p in zip(imgs, make_params(geometry_rows(H, W))):
        want, inside = AO.augment(img, p, (H, W), 99)
        got = augment_host(img, p, (H, W), 99)
        assert got.dtype == np.uint8 and got.shape == (H, W, 3) and np.array_equal(got, want)
        assert (got[~inside] == 99).all()
    assert not AO.augment(imgs[4], make_params(geometry_rows(H, W))[4], (H, W), 99)[1].any()       # wholly off the canvas
    # a stretch row is the plain resize, a letterbox row the host letterbox
    for img in imgs:
        h, w = img.shape[:2]
        stretch = make_params([(H, W, 0, 0, 0, 0, 1, 1)])[0]
        assert np.array_equal(augment_host(img, stretch, (H, W), 128), prepost.resize_bilinear(img, (W, H)))
        box = make_params([prepost.letterbox_rect(h, w, H, W) + (0, 0, 1, 1)])[0]
        assert np.array_equal(augment_host(img, box, (H, W), 128), prepost.letterbox(img, (H, W), 128))


def test_augment_host_colour_vs_oracle():
    from yolo4hip.augment import AugmentConfig, augment_host, draw_params
    H, W = CANVASES[0]
    worst = diff = total = 0
    imgs, params = colour_table(H, W)
    for img, p in zip(imgs, params):
        want, inside = AO.augment(img, p, (H, W), 128)
        got = augment_host(img, p, (H, W), 128)
        assert (got[~inside] == 128).all()
        m, d, t = differing(got, want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    share = diff / total
    print("augment_host vs float64 oracle: max level difference", worst, "differing share", share, "of", total, "bytes")
    note("host_vs_oracle", {"max_level_difference": worst, "differing_share": share, "bytes": total, "cap": SHARE_CAP})
    assert worst <= 1 and share <= SHARE_CAP
    # drawn factors with a real resample (no exact ties: the factors are not dyadic)
    photo = natural_photo()
    drawn = draw_params(np.random.default_rng(7), [photo.shape[:2]] * 8, (H, W), AugmentConfig())
    worst = diff = total = 0
    for p in drawn:
        want, inside = AO.augment(photo, p, (H, W), 128)
        m, d, t = differing(augment_host(photo, p, (H, W), 128), want, inside)
        worst, diff, total = max(worst, m), diff + d, total + t
    note("host_vs_oracle_drawn", {"max_level_difference": worst, "differing_share": diff / max(total, 1), "bytes": total})
    assert worst <= 1 and diff <= SHARE_CAP * total


# ---- draw_params
def test_draw_params_identity_seed_and_ranges():
    from yolo4hip.augment import AugmentConfig, draw_params
    ident = AugmentConfig.identity()
    assert ident == AugmentConfig(jitter=0, scale=(1, 1), flip=False, hue=0, sat=1, val=1)
    for seed, (H, W), sizes in [(0, (64, 96), SIZES), (5, (608, 608), [(480, 640)] * 3), (123456, (96, 64), [(1, 1), (3000, 7)])]:
        p = draw_params(np.random.default_rng(seed), sizes, (H, W), ident)
        assert len(p) == len(sizes)
        for r in p:
            assert (r["out_h"], r["out_w"], r["pad_top"], r["pad_left"], r["flip"]) == (H, W, 0, 0, 0)
            assert r["hue"] == 0 and not np.signbit(r["hue"]) and r["sat"] == 1 and r["val"] == 1
    cfg = AugmentConfig()
    a = draw_params(np.random.default_rng(5), SIZES, (64, 96), cfg)
    b = draw_params(np.random.default_rng(5), SIZES, (64, 96), cfg)
    assert a.tobytes() == b.tobytes() and a.tobytes() != draw_params(np.random.default_rng(6), SIZES, (64, 96), cfg).tobytes()
    # every config consumes the same draws: the stream after the call does not depend on it
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    draw_params(r1, SIZES, (64, 96), cfg)
    draw_params(r2, SIZES, (64, 96), ident)
    assert r1.uniform() == r2.uniform()
    H, W = 416, 608
    p = draw_params(np.random.default_rng(1), [(1, 1)] * 10000, (H, W), cfg)
    j, (lo, hi) = cfg.jitter, cfg.scale
    rmin = (1 - j) / (1 + j)
    assert p["out_h"].min() >= max(1, np.rint(lo * H * rmin)) and p["out_h"].max() <= np.rint(hi * H)
    assert p["out_w"].min() >= max(1, np.rint(lo * W * rmin)) and p["out_w"].max() <= np.rint(hi * W)
    for pad, room in ((p["pad_left"], W - p["out_w"]), (p["pad_top"], H - p["out_h"])):
        assert (np.minimum(room, 0) <= pad).all() and (pad <= np.maximum(room, 0)).all()
    assert set(np.unique(p["flip"])) == {0, 1} and 0.45 < p["flip"].mean() < 0.55
    assert np.abs(p["hue"]).max() <= np.float32(cfg.hue)
    for name, top in (("sat", cfg.sat), ("val", cfg.val)):
        assert p[name].min() >= np.float32(1 / top) and p[name].max() <= np.float32(top)
        assert 0.45 < (p[name] > 1).mean() < 0.55
    assert (p["pad_left"] < 0).any() and (p["pad_top"] < 0).any() and (p["out_w"] < W).any()


# ---- transform_boxes
def _centre_rule(boxes, H, W, ncls):
    """Engine._check_boxes itself, on a stand-in for the engine: it reads img_hw, num_classes and the box capacity only."""
    from yolo4hip.engine import Engine
    stub = types.SimpleNamespace(img_hw=(H, W), num_classes=ncls, _loss_max_boxes=lambda: boxes.shape[1])
    return Engine._check_boxes(stub, boxes)


def test_transform_boxes_hand_cases():
    from yolo4hip.augment import transform_boxes
    H, W = 64, 96
    raw = np.array([[10, 20, 30, 40, 1]], np.float32)
    ident = make_params([(H, W, 0, 0, 0, 0, 1, 1)])[0]
    assert np.array_equal(transform_boxes(raw, (H, W), ident, (H, W), 4)[0], raw[0])
    flip = make_params([(H, W, 0, 0, 1, 0, 1, 1)])[0]
    assert transform_boxes(raw, (H, W), flip, (H, W), 4)[0].tolist() == [66, 20, 86, 40, 1]
    # a 32 x 48 image drawn at 2x with pads (-10, -20): x -> 2 x - 20, y -> 2 y - 10
    p = make_params([(64, 96, -10, -20, 0, 0, 1, 1)])[0]
    raw = np.array([[5, 10, 20, 20, 0],        # cut by the left edge: x1 -10 -> 0
                    [40, 10, 58, 20, 1],       # cut by the right edge: x2 96
                    [20, 2, 30, 12, 2],        # cut by the top edge: y1 -6 -> 0
                    [20, 30, 30, 37, 0],       # cut by the bottom edge: y2 64
                    [0, 0, 9, 4, 1],           # wholly outside (left and above): dropped
                    [30, 10, 30.5, 20, 2],     # 1 px wide after the transform: dropped
                    [25, 15, 35, 25, 1]], np.float32)
    got = transform_boxes(raw, (32, 48), p, (H, W), 8)
    assert got.dtype == np.float32 and got.shape == (8, 5)
    assert got[:5].tolist() == [[0, 10, 20, 30, 0], [60, 10, 96, 30, 1], [20, 0, 40, 14, 2], [20, 50, 40, 64, 0], [30, 20, 50, 40, 1]]
    assert not got[5:].any()
    # flipped: x1, x2 <- W - x2, W - x1, then the same clip
    pf = make_params([(64, 96, -10, -20, 1, 0, 1, 1)])[0]
    gotf = transform_boxes(raw, (32, 48), pf, (H, W), 8)
    assert gotf[:5].tolist() == [[76, 10, 96, 30, 0], [0, 10, 36, 30, 1], [56, 0, 76, 14, 2], [56, 50, 76, 64, 0], [46, 20, 66, 40, 1]]
    assert not transform_boxes(np.zeros((0, 5), np.float32), (32, 48), p, (H, W), 8).any()
    assert transform_boxes(np.tile(raw[6], (9, 1)), (32, 48), p, (H, W), 3).shape == (3, 5)


def test_transform_boxes_survivors_pass_the_centre_rule():
    from yolo4hip.augment import AugmentConfig, draw_params, transform_boxes
    H, W, mb = 96, 160, 20
    rng = np.random.default_rng(4)
    params = draw_params(np.random.default_rng(2), [None] * 300, (H, W), AugmentConfig())
    out = np.zeros((len(params), mb, 5), np.float32)
    for i, p in enumerate(params):
        h, w = int(rng.integers(8, 400)), int(rng.integers(8, 400))
        x1, y1 = rng.uniform(0, w - 2, mb), rng.uniform(0, h - 2, mb)
        raw = np.stack([x1, y1, rng.uniform(x1, w), rng.uniform(y1, h), rng.integers(0, 3, mb)], -1).astype(np.float32)
        out[i] = transform_boxes(raw, (h, w), p, (H, W), mb)
        valid = out[i, :, 2] - out[i, :, 0] > 0
        k = int(valid.sum())
        assert valid[:k].all() and not out[i, k:].any()                       # a compacted prefix
        assert (out[i, :k, 2] - out[i, :k, 0] > 1).all() and (out[i, :k, 3] - out[i, :k, 1] > 1).all()
        assert (out[i, :k, :4] >= 0).all() and (out[i, :k, [0, 2]] <= W).all() and (out[i, :k, [1, 3]] <= H).all()
    kept = (out[..., 2] > out[..., 0]).sum()
    assert 0 < kept < out.shape[0] * mb                                        # some dropped, some kept
    assert _centre_rule(out, H, W, 3) is not None                             # raises ValueError on a centre off the grid


# ---- the generator
def test_generator_without_augment_is_unchanged_and_with_identity_equal(tmp_path):
    from yolo4hip import prepost
    from yolo4hip.augment import AugmentConfig
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    sizes = [(120, 200), (160, 160), (90, 64)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5])
    cfg = make_config((96, 160), batch_size=3)
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    gen = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg)
    assert gen.augment is None
    np.random.seed(3)
    X, boxes = gen.boxes(0)
    # the same values from prepost directly, with the global generator in the same state
    np.random.seed(3)
    H, W = 96, 160
    for i, line in enumerate(lines):
        fields = line.split()
        img = prepost.imread_rgb(os.path.join(str(tmp_path), fields[0]))
        want_x = (prepost.resize_bilinear(img, (W, H)) / 255.).astype(np.float32)
        raw = np.array([[float(v) for v in f.split(',')] for f in fields[1:]], dtype=np.float32)
        want_b = np.zeros((100, 5), np.float32)
        if len(raw):
            np.random.shuffle(raw)
            raw[:, [0, 2]] = raw[:, [0, 2]] * (W / img.shape[1])
            raw[:, [1, 3]] = raw[:, [1, 3]] * (H / img.shape[0])
            want_b[:len(raw)] = raw
        assert np.array_equal(X[i].view(np.int32), want_x.view(np.int32))
        assert np.array_equal(boxes[i].view(np.int32), want_b.view(np.int32))
    with pytest.raises(ValueError, match="does not augment"):
        gen.raw(0)
    # the identity config: the same batch, bit for bit, on both of the augmenting generator's paths
    ident = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=AugmentConfig.identity(), seed=1)
    np.random.seed(3)
    Xi, bi = ident.boxes(0)
    assert np.array_equal(Xi.view(np.int32), X.view(np.int32)) and np.array_equal(bi.view(np.int32), boxes.view(np.int32))
    np.random.seed(3)
    raws, params, br = ident.raw(0)
    assert [r.shape[:2] for r in raws] == sizes and all(r.dtype == np.uint8 for r in raws)
    assert np.array_equal(br.view(np.int32), boxes.view(np.int32)) and br.dtype == np.float32
    # the default config: the same seed gives the same parameters through raw() and through boxes() / gen[i]
    a = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=AugmentConfig(), seed=5)
    b = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=cfg, augment=AugmentConfig(), seed=5)
    np.random.seed(3)
    raws, params, ba = a.raw(0)
    np.random.seed(3)
    (Xb, y_s, y_m, y_l, xywh), zeros = b[0]
    from yolo4hip.augment import augment_host
    for i in range(3):
        want = (augment_host(raws[i], params[i], (H, W), 128) / 255.).astype(np.float32)
        assert np.array_equal(Xb[i].view(np.int32), want.view(np.int32))
    assert xywh.shape == (3, 100, 4) and y_s.shape == (3, 12, 20, 3, 8)
    assert params.tobytes() != a.raw(0)[1].tobytes()                          # the next batch draws on


# ---- the C ABI without a device
def test_augment_abi_and_host_checks():
    from yolo4hip import ext
    lib = ext.load()
    assert C.sizeof(ext.y4_augment_desc) == 48 and ext.y4_augment_desc.flip.offset == 32 and ext.y4_augment_desc.val.offset == 44
    EINVAL = -22
    p = C.c_void_p(4096)                                  # never dereferenced: every case returns before a launch
    f = lib.y4_augment_u8_ragged
    assert f(None, p, 1, p, 608, 608, 128, None) == EINVAL and f(p, None, 1, p, 608, 608, 128, None) == EINVAL
    assert f(p, p, 1, None, 608, 608, 128, None) == EINVAL and b"augment_u8_ragged" in lib.y4_last_error()
    for n in (0, -1, 65536):
        assert f(p, p, n, p, 608, 608, 128, None) == EINVAL
    for H, W in ((0, 608), (608, 0), (-32, 608)):
        assert f(p, p, 1, p, H, W, 128, None) == EINVAL
    for pad in (-1, 256):
        assert f(p, p, 1, p, 608, 608, pad, None) == EINVAL
    assert f(p, p, 2000, p, 608, 608, 128, None) == EINVAL                   # 2000 x 608 x 608 x 3 >= 2^31 bytes
