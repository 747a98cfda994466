"""Views (test-time augmentation) on the host, no GPU: `tiling.view_rows` -- the rectangle rule, the map composition with the
corner swap, validation --, the geometry of a view through the marker predicates of tests/marker_photos.py on the host
restatement `views_oracle.view_host`, the witnesses of the oriented gather on the oracle, and the recorded figures of
tests/views_cases.py."""
import math

import numpy as np
import pytest

import marker_photos as MP
import views_cases as VC
import views_oracle as VO

CANVAS = (96, 128)
PHOTOS = [(131, 97), (97, 131), (64, 80), (200, 150), (96, 128)]
EPS = 2.0 ** -24


def _rows(h, w, letterbox, canvas=CANVAS, tile=None, full=True):
    from yolo4hip import tiling
    return tiling.tile_rows(h, w, canvas, tile, 0.2, full, letterbox)


def test_default_views_are_yolov5s():
    from yolo4hip import tiling
    assert tiling.DEFAULT_VIEWS == ((1.0, ""), (0.83, "lr"), (0.67, ""))
    assert tiling.FLIP_BITS == {"": 0, "lr": 1, "ud": 2, "lrud": 3}


@pytest.mark.parametrize("letterbox", [False, True])
def test_the_identity_view_returns_every_row_unchanged(letterbox):
    from yolo4hip import tiling
    for h, w in PHOTOS:
        rows = _rows(h, w, letterbox, tile=(64, 64))
        assert len(rows) > 1 or (h <= 64 and w <= 64)
        got = tiling.view_rows(rows, ((1.0, ""),), (h, w), CANVAS)
        assert len(got) == len(rows)
        for (win, rect, bits, m), (win0, rect0, m0) in zip(got, rows):
            assert win == tuple(win0) and rect == tuple(rect0) and bits == 0
            assert m.dtype == np.float32 and np.array_equal(m.view(np.int32), m0.view(np.int32))
        # ... and as view 0 of a longer list: view-major order, a row's slot is its index
        got = tiling.view_rows(rows, tiling.DEFAULT_VIEWS, (h, w), CANVAS)
        assert len(got) == 3 * len(rows)
        assert [g[0] for g in got] == [tuple(r[0]) for r in rows] * 3
        assert [g[2] for g in got] == [0] * len(rows) + [1] * len(rows) + [0] * len(rows)
        for g, r in zip(got[:len(rows)], rows):
            assert g[1] == tuple(r[1]) and np.array_equal(g[3], r[2])


@pytest.mark.parametrize("letterbox", [False, True])
def test_the_scaled_rectangle_shrinks_about_the_rows_own_centre(letterbox):
    from yolo4hip import tiling
    H, W = CANVAS
    for h, w in PHOTOS:
        base = _rows(h, w, letterbox)[-1:]
        (_, (oh, ow, top, left), _), = base
        for scale in (1.0, 0.83, 0.67, 0.5, 0.333, 0.01, 1e-9):
            (win, (oh2, ow2, top2, left2), bits, m), = tiling.view_rows(base, ((scale, "lr"),), (h, w), CANVAS)
            assert oh2 == max(1, math.floor(scale * oh + 0.5)) and ow2 == max(1, math.floor(scale * ow + 0.5))
            assert top2 == top + (oh - oh2) // 2 and left2 == left + (ow - ow2) // 2
            assert 0 <= top2 and top2 + oh2 <= H and 0 <= left2 and left2 + ow2 <= W           # inside the canvas
            assert abs((top2 + oh2 / 2) - (top + oh / 2)) <= 0.5 and abs((left2 + ow2 / 2) - (left + ow / 2)) <= 0.5
            assert win == (0, 0, h, w) and bits == 1
    # odd differences leave the extra row / column at the bottom / right, as letterbox_rect does
    assert tiling.view_rect((96, 128, 0, 0), 0.83) == (80, 106, 8, 11)
    assert tiling.view_rect((71, 128, 12, 0), 0.67) == (48, 86, 23, 21)
    assert tiling.view_rect((5, 7, 1, 2), 1.0) == (5, 7, 1, 2)


@pytest.mark.parametrize("letterbox", [False, True])
def test_map_composition_returns_the_photo_box(letterbox):
    """Random boxes in photo pixels -> the canvas box under the view in float64 (views_oracle.canvas_box), rounded to float32 as
    the decode stage stores it -> back through map' with the corner swap.  The bound: the canvas box, the two map entries and the
    result each round once (relative 2^-24), so the normalised error is at most 2^-24 (2 |a c| + |b| + |u|) <= 4 * 2^-24 (|a| +
    |b| + 1) for c, u in [0, 1]; times the photo's side in pixels."""
    from yolo4hip import tiling
    H, W = CANVAS
    rng = np.random.default_rng(7)
    views = ((1.0, ""), (0.83, "lr"), (0.67, ""), (1.0, "ud"), (0.5, "lrud"), (0.9, "lr"), (0.77, "ud"))
    worst = 0.0
    for h, w in PHOTOS:
        rows = _rows(h, w, letterbox, tile=(64, 64))
        for (win, rect, bits, m) in tiling.view_rows(rows, views, (h, w), CANVAS):
            y0, x0, wh, ww = win
            for _ in range(8):
                xs = np.sort(rng.uniform(x0, x0 + ww, 2))
                ys = np.sort(rng.uniform(y0, y0 + wh, 2))
                box = np.array([xs[0], ys[0], xs[1], ys[1]])
                cb = VO.canvas_box(box, win, rect, bits, CANVAS)
                assert cb[0] <= cb[2] and cb[1] <= cb[3]
                norm = (cb / (W, H, W, H)).astype(np.float32)
                back = VO.map_boxes_oriented(norm, m).astype(np.float64)
                assert back[0] <= back[2] and back[1] <= back[3]                        # the swap keeps the corners ordered
                m64 = m.astype(np.float64)
                bound = 4 * EPS * np.array([abs(m64[0]) + abs(m64[1]) + 1, abs(m64[2]) + abs(m64[3]) + 1] * 2) * (w, h, w, h)
                err = np.abs(back * (w, h, w, h) - box)
                assert (err <= bound).all(), (h, w, win, rect, bits, box, err, bound)
                worst = max(worst, float((err / bound).max()))
                if bits:                                                                 # without the swap the corners cross
                    plain = VO.unoriented(norm, m)
                    assert (bits & 1 == 0 or plain[0] >= plain[2]) and (bits & 2 == 0 or plain[1] >= plain[3])
    print(f"map composition: worst error {worst:.3f} of the float32 bound")


def test_the_map_is_rounded_once_from_float64():
    from yolo4hip import tiling
    h, w, (H, W) = 131, 97, CANVAS
    win, rect = (3, 5, 60, 70), (48, 86, 23, 21)
    base = tiling.window_map(h, w, H, W, win, rect)
    assert np.array_equal(tiling.view_map(h, w, H, W, win, rect, 0), base)
    ax, bx = (W / 86) * 70 / w, (5 - 21 * 70 / 86) / w
    ay, by = (H / 48) * 60 / h, (3 - 23 * 60 / 48) / h
    want = np.array([-ax, ax + bx, -ay, ay + by], np.float64).astype(np.float32)
    assert np.array_equal(tiling.view_map(h, w, H, W, win, rect, 3), want)
    assert np.array_equal(tiling.view_map(h, w, H, W, win, rect, 1), [want[0], want[1], base[2], base[3]])
    assert np.array_equal(tiling.view_map(h, w, H, W, win, rect, 2), [base[0], base[1], want[2], want[3]])


def test_validation():
    from yolo4hip import tiling
    rows = _rows(131, 97, False)
    ok = lambda v: tiling.view_rows(rows, v, (131, 97), CANVAS)                   # noqa: E731
    assert len(ok([(1.0, ""), (1.0, "lr"), (0.5, "")])) == 3 * len(rows)
    assert len(ok([(1 - 0.05 * k, "ud") for k in range(16)])) == 16 * len(rows)
    for bad in ([], (), [(1 - 0.05 * k, "") for k in range(17)],
                [(0.0, "")], [(-0.5, "")], [(1.0001, "")], [(float("nan"), "")], [(float("inf"), "")], [(-float("inf"), "")],
                [(1.0, "rl")], [(1.0, "LR")], [(1.0, 1)], [(1.0, None)], [(1.0,)], [("x", "")], 5,
                [(1.0, ""), (0.5, "lr"), (1.0, "")], [(0.5, "lr"), (0.5, "lr")]):
        with pytest.raises(ValueError):
            ok(bad)


# ------------------------------------------------------------------------------------------------ geometry, by the marker predicates
def _marker_photo(p, h, w):
    return MP.make_photo(h, w, p, 31, 4, min_side=max(24, min(h, w) // 4))


@pytest.mark.parametrize("letterbox", [False, True])
def test_view_host_canvases_carry_the_markers_where_the_maps_say(letterbox):
    """`view_host` (prepost's resize, np.flip) under every default view and under ((1.0, 'ud'), (0.5, 'lrud')): the label rows --
    the photo's boxes through `canvas_box` -- satisfy predicates 1 and 2 on the canvas, and every marker's exact-colour rectangle,
    mapped back through map' with the corner swap, satisfies predicate 3 with the bound of the row's own scale.  With the flip bit
    dropped from the map alone, predicate 3 fails."""
    from yolo4hip import tiling
    H, W = CANVAS
    checked = refused = 0
    for p, (h, w) in enumerate(PHOTOS):
        photo, truth = _marker_photo(p, h, w)
        assert len(truth) >= 2
        base = _rows(h, w, letterbox)[-1:]
        for views in (tiling.DEFAULT_VIEWS, ((1.0, "ud"), (0.5, "lrud"))):
            for (win, rect, bits, m), (scale, _) in zip(tiling.view_rows(base, views, (h, w), CANVAS), views):
                canvas = VO.view_host(photo, win, rect, bits, CANVAS)
                plain = MP.place_row(photo, win, rect, CANVAS)
                assert np.array_equal(canvas, np.flip(plain, axis=[a for a, b in ((1, 1), (0, 2)) if bits & b]) if bits else plain)
                sx, sy = rect[1] / w, rect[0] / h
                rows = np.array([list(VO.canvas_box(t[:4], win, rect, bits, CANVAS)) + [t[4]] for t in truth])
                r = MP.check_canvas(canvas, rows, MP.whole_canvas(H, W, sx, sy), f"view ({scale}, {bits}) of photo {p}")
                assert r[0] == r[3] == len(truth)
                for j, t in enumerate(truth):
                    ex = MP.exact_rect(canvas, MP.colour_of(p, j, int(t[4])))
                    MP.detection_sits_on_marker(VO.photo_box(ex, CANVAS, m, (h, w)), t, sx, sy, f"photo {p} view {bits} marker {j}")
                    checked += 1
                    if bits:
                        wrong = tiling.view_map(h, w, H, W, win, rect, 0)
                        try:
                            MP.detection_sits_on_marker(VO.photo_box(ex, CANVAS, wrong, (h, w)), t, sx, sy)
                        except AssertionError:
                            refused += 1
    assert checked >= 40 and refused >= 10


# ------------------------------------------------------------------------------------------------ the oriented gather, on the oracle
def test_recorded_cases_meet_the_conditions():
    """Every case of views_cases: an 'lr', a 'ud', an 'lrud' and a scaled map, 2 to 6 slots per group, and the recorded figures."""
    for geo, views in VC.VIEW_SETS.items():
        rows, group, slot, maps, per_group = VC.geometry(geo)
        assert per_group == [len(views), 2] and all(2 <= n <= 6 for n in per_group) and len(rows) > VC.CHUNK
        bits = {r[2] for r in rows}
        assert {1, 2, 3} <= bits
        assert any(s < 1.0 for s, _ in views)
        for (win, rect, b, m) in rows:
            assert (m[0] < 0) == bool(b & 1) and (m[2] < 0) == bool(b & 2)
    assert sorted(VC.CASES) == sorted((c, g, r) for c in (3, 80) for g in VC.VIEW_SETS for r in VC.RULES)
    for key, (seed, nms_margin, member_margin, flipped, cross) in VC.CASES.items():
        assert nms_margin >= VC.MIN_MARGIN >= 1e-5 and member_margin >= VC.MIN_MARGIN and flipped >= 1 and cross >= 1, key


@pytest.mark.parametrize("key", [(3, 0, "iou"), (3, 2, "agn_iou"), (80, 1, "diou06")])
def test_recorded_figures_are_the_oracles(key):
    seed, nms_margin, member_margin, flipped, cross = VC.CASES[key]
    got = VC.figures(*key, seed)
    assert abs(got[0] - nms_margin) <= 0.01 * nms_margin and abs(got[1] - member_margin) <= 0.01 * member_margin
    assert got[2:] == (flipped, cross)
    for b, _ in VC.tables(key[0], key[1], seed):                             # every stored box has its corners in order
        assert (b[..., 0] <= b[..., 2]).all() and (b[..., 1] <= b[..., 3]).all()
