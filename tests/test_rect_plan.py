"""Rectangular network input (img_size = (H, W, 3)), host side: the Python plan against the C++ plan through
y4_create_hw / y4_layer_dims, square handles made either way are the same, errors, and host preprocessing orientation.
No GPU needed: nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

RECTS = [(352, 608), (608, 352), (96, 160), (256, 1024)]


def _lib():
    from yolo4hip import ext
    return ext, ext.load()


def _create(H, W, ncls=80, dtype="f32", max_batch=1):
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    ext, lib = _lib()
    cfg = _cfg_struct(make_config((H, W)), ncls, max_batch, dtype)
    h = C.c_void_p()
    ext.check(lib.y4_create_hw(C.byref(cfg), H, W, C.byref(h)))
    return lib, h


@pytest.mark.parametrize("hw", RECTS, ids=lambda t: f"{t[0]}x{t[1]}")
def test_rect_plan_matches_library(hw):
    from yolo4hip.plan import build_plan
    H, W = hw
    plan = build_plan((H, W), 80)
    lib, h = _create(H, W)
    try:
        ih, iw = C.c_int32(), C.c_int32()
        assert lib.y4_input_dims(h, C.byref(ih), C.byref(iw)) == 0 and (ih.value, iw.value) == (H, W)
        assert lib.y4_num_layers(h) == len(plan.convs) == 110
        from yolo4hip import ext
        dims = (C.c_int32 * 4)()
        for cs in plan.convs:
            d = ext.y4_layer_desc()
            assert lib.y4_layer_info(h, cs.idx, C.byref(d)) == 0
            assert (d.ksize, d.stride, d.cin, d.cout) == (cs.k, cs.s, cs.cin, cs.cout), cs.idx
            assert (d.in_side, d.out_side) == (-1, -1), cs.idx          # no one side on a rectangle
            assert lib.y4_layer_dims(h, cs.idx, dims) == 0
            assert tuple(dims) == (cs.in_h, cs.in_w, cs.out_h, cs.out_w), cs.idx
        assert plan.convs[0].in_h == H and plan.convs[0].in_w == W
        flops, nbox, hcs, wfl = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        assert lib.y4_model_info(h, C.byref(flops), C.byref(nbox), C.byref(hcs), C.byref(wfl)) == 0
        assert flops.value == plan.flops_per_image
        assert nbox.value == plan.num_boxes == 3 * sum((H // s) * (W // s) for s in (8, 16, 32))
        assert wfl.value == plan.n_params
        assert plan.grids == tuple((H // s, W // s) for s in (8, 16, 32))
        # the head convs write [gh, gw] grids: rows over H, columns over W
        for idx, s in zip((93, 101, 109), (8, 16, 32)):
            assert lib.y4_layer_dims(h, idx, dims) == 0 and (dims[2], dims[3]) == (H // s, W // s)
    finally:
        lib.y4_destroy(h)


def test_rect_flops_scale_with_area():
    from yolo4hip.plan import build_plan
    sq, rect = build_plan(608, 80), build_plan((352, 608), 80)
    assert rect.flops_per_image * 608 == sq.flops_per_image * 352


@pytest.mark.parametrize("side", [416, 608])
def test_square_create_hw_equals_create(side):
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    from yolo4hip.plan import build_plan
    ext, lib = _lib()
    cfg = _cfg_struct(make_config(side), 80, 2, "bf16")
    a, b = C.c_void_p(), C.c_void_p()
    ext.check(lib.y4_create(C.byref(cfg), C.byref(a)))
    ext.check(lib.y4_create_hw(C.byref(cfg), side, side, C.byref(b)))
    try:
        for i in range(110):
            da, db = ext.y4_layer_desc(), ext.y4_layer_desc()
            assert lib.y4_layer_info(a, i, C.byref(da)) == 0 and lib.y4_layer_info(b, i, C.byref(db)) == 0
            assert bytes(da) == bytes(db), i
            assert da.in_side > 0
        infos = []
        for h in (a, b):
            f, nb, hc, wf = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
            ext.check(lib.y4_model_info(h, C.byref(f), C.byref(nb), C.byref(hc), C.byref(wf)))
            ab, wb = C.c_size_t(), C.c_size_t()
            ext.check(lib.y4_workspace_bytes(h, C.byref(ab), C.byref(wb)))
            infos.append((f.value, nb.value, hc.value, wf.value, ab.value, wb.value))
        assert infos[0] == infos[1]
        # and the Python plan's square statement is unchanged by the tuple form
        p1, p2 = build_plan(side, 80), build_plan((side, side), 80)
        assert p1.img_size == p2.img_size == side and p1.grids == p2.grids == tuple(side // s for s in (8, 16, 32))
        assert [c.__dict__ for c in p1.convs] == [c.__dict__ for c in p2.convs] and p1.sides == p2.sides
    finally:
        lib.y4_destroy(a)
        lib.y4_destroy(b)


def test_rect_errors():
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    ext, lib = _lib()
    cfg = _cfg_struct(make_config(416), 80, 1, "f32")
    h = C.c_void_p()
    for H, W in ((352, 600), (340, 608), (0, 608), (352, -32)):
        assert lib.y4_create_hw(C.byref(cfg), H, W, C.byref(h)) == -22, (H, W)
        assert b"multiple" in lib.y4_last_error()
    lib2, h = _create(352, 608, dtype="bf16")
    try:
        # stem fusion is square-only: refused on a rectangle, with a message that says so
        assert lib.y4_set_stem_fusion(h, 1) == -22 and b"square" in lib.y4_last_error()
        assert lib.y4_layer_dims(h, 110, (C.c_int32 * 4)()) == -22
        assert lib.y4_layer_dims(h, 0, None) == -22
    finally:
        lib.y4_destroy(h)


def test_rect_workspace_aliasing_and_tiles_without_gpu():
    ext, lib = _lib()
    _, h = _create(352, 608, ncls=80, dtype="bf16", max_batch=4)
    try:
        a0, w0 = C.c_size_t(), C.c_size_t()
        ext.check(lib.y4_workspace_bytes(h, C.byref(a0), C.byref(w0)))
        ext.check(lib.y4_set_workspace_aliasing(h, 1))
        a1, w1 = C.c_size_t(), C.c_size_t()
        ext.check(lib.y4_workspace_bytes(h, C.byref(a1), C.byref(w1)))
        assert 0 < a1.value < a0.value and w1.value == w0.value
        # the activations alone scale with the area: a 608^2 handle needs more
        _, hs = _create(608, 608, ncls=80, dtype="bf16", max_batch=4)
        try:
            ext.check(lib.y4_set_workspace_aliasing(hs, 1))
            a2 = C.c_size_t()
            ext.check(lib.y4_workspace_bytes(hs, C.byref(a2), None))
            assert a2.value > a1.value
        finally:
            lib.y4_destroy(hs)
        ok = (C.c_int32 * 110)(*([0] * 110))
        assert lib.y4_set_tiles(h, ok, 110) == 0
        bad = (C.c_int32 * 110)(*([0] * 110))
        bad[5] = 10 ** 6                                   # not a tile id
        assert lib.y4_set_tiles(h, bad, 110) == -22
        assert lib.y4_set_tiles(h, ok, 109) == -22
        got = (C.c_int32 * 110)()
        assert lib.y4_get_tiles(h, got, 110) == 0 and list(got) == [0] * 110
    finally:
        lib.y4_destroy(h)


def test_make_config_and_synth_images_take_hw():
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    assert make_config((352, 608))['img_size'] == (352, 608, 3)
    assert make_config(416)['img_size'] == (416, 416, 3)
    assert W.synth_images(2, (64, 96)).shape == (2, 64, 96, 3)
    assert np.array_equal(W.synth_images(1, 64), W.synth_images(1, (64, 64)))


@pytest.mark.parametrize("src", [(200, 90), (90, 200)], ids=["tall", "wide"])
def test_preprocess_img_is_h_by_w(src):
    """The stretch resize targets height H and width W (cv2's dsize is (width, height)): output [H, W, 3] from a tall and a
    wide source, and a source already at (H, W) passes through unchanged up to the / 255."""
    from yolo4hip import prepost
    H, W = 96, 160
    rng = np.random.default_rng(sum(src))
    img = rng.integers(0, 256, (src[0], src[1], 3), dtype=np.uint8)
    out = prepost.preprocess_img(img, (H, W, 3))
    assert out.shape == (H, W, 3)
    out2 = prepost.preprocess_img(img, (W, H, 3))
    assert out2.shape == (W, H, 3)
    # a horizontal ramp stays horizontal: columns vary, rows do not
    ramp = np.tile(np.linspace(0, 255, src[1]).astype(np.uint8)[None, :, None], (src[0], 1, 3))
    r = prepost.preprocess_img(ramp, (H, W, 3))
    assert np.all(r[0] == r[-1]) and r[0, 0, 0] < r[0, -1, 0]
    same = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(prepost.preprocess_img(same, (H, W, 3)), same / 255.)
