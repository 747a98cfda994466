"""Rectangular network input (img_size = (H, W, 3)) on the GPU: the kernels on H != W planes against the oracle, decode + NMS
against a NumPy restatement of the rectangular decode, whole forwards against oracle/forward.py, bit identity of every fusion
and schedule on a rectangle, the square path unchanged, and the Yolov4 facade at 352 x 608.

Tolerances are those of the square tests: tests/test_gpu_conv.py (TOL), tests/test_gpu_decode_nms.py (boxes 1e-5, scores
1e-6, decisions identical), tests/test_gpu_forward.py (fp32 heads, 16-bit bounds)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import CLASS_DIR, detection_agreement, make_conv_weights, quantize, run_conv_gpu

pytestmark = pytest.mark.gpu

TOL = {"f32": (2e-5, 2e-5), "bf16": (1e-2, 2.0 ** -7), "f16": (2e-3, 2.0 ** -9)}


# ------------------------------------------------------------------ NumPy restatement of the rectangular decode
def rect_inference_from_heads(heads, ncls, anchors, xyscale, H, W, strides=(8, 16, 32), iou_threshold=0.413,
                              score_threshold=0.3, max_boxes=100):
    """oracle.decode_nms.inference_from_heads for [n, gh, gw, 3(5+C)] heads: the reference's get_boxes (custom_layers.py:221-258)
    with a (gh, gw) grid -- x = column, y = row -- boxes flattened in (row, col, anchor) order per scale, x1 / x2 divided by W and
    y1 / y2 by H; then the oracle's own combined_nms (flat boxes and scores: shape-agnostic)."""
    from oracle import decode_nms as OD
    F32 = np.float32
    anchors = np.asarray(anchors, F32).reshape(3, 3, 2)
    n = heads[0].shape[0]
    all_boxes, all_scores = [], []
    for s in range(3):
        gh, gw = heads[s].shape[1:3]
        pred = np.asarray(heads[s], F32).reshape(n, gh, gw, 3, 5 + ncls)
        xy = OD.sigmoid(pred[..., 0:2])
        obj = OD.sigmoid(pred[..., 4:5])
        cls = OD.sigmoid(pred[..., 5:])
        gx, gy = np.meshgrid(np.arange(gw), np.arange(gh))
        grid = np.stack([gx, gy], axis=-1)[:, :, None, :].astype(F32)
        xy = ((xy * F32(xyscale[s])) - F32(0.5 * (xyscale[s] - 1)) + grid) * F32(strides[s])
        wh = np.exp(pred[..., 2:4]).astype(F32) * anchors[s]
        box = np.concatenate([xy - wh / F32(2), xy + wh / F32(2)], axis=-1).astype(F32)
        all_boxes.append(box.reshape(n, -1, 4))
        all_scores.append((obj * cls).astype(F32).reshape(n, -1, ncls))
    boxes = np.concatenate(all_boxes, axis=1)
    boxes = (boxes / np.array([W, H, W, H], F32)).astype(F32)
    scores = np.concatenate(all_scores, axis=1)
    return OD.combined_nms(boxes, scores, 100, max_boxes, iou_threshold, score_threshold)


def _random_heads(rng, n, H, W, ncls, obj_bias, cls_bias, gain=1.5):
    heads = []
    nf = 5 + ncls
    for s in (8, 16, 32):
        h = (rng.standard_normal((n, H // s, W // s, 3, nf)) * gain).astype(np.float32)
        h[..., 2:4] *= 0.3
        h[..., 4] += obj_bias
        h[..., 5:] += cls_bias
        heads.append(h.reshape(n, H // s, W // s, 3 * nf))
    return heads


def test_restatement_matches_oracle_on_square():
    """The rectangular restatement is the oracle's decode on a square input (same float32 arithmetic, bit for bit)."""
    from oracle import decode_nms as OD
    from yolo4hip.config import make_config
    cfg = make_config(160)
    heads = _random_heads(np.random.default_rng(3), 2, 160, 160, 5, -2.0, -1.0)
    a = rect_inference_from_heads(heads, 5, cfg["anchors"], cfg["xyscale"], 160, 160)
    b = OD.inference_from_heads(heads, 5, cfg["anchors"], cfg["xyscale"], 160)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert int(a[3].sum()) > 0


# ------------------------------------------------------------------ standalone kernels
def _conv_ref(x, cw, k, stride, act, res, ups):
    from oracle.forward import conv_block
    y = conv_block(x, cw, k, stride, act, res)
    if ups:
        y = y.repeat(2, axis=1).repeat(2, axis=2)
    return y


def _tile_descs():
    from yolo4hip import ext
    lib = ext.load()
    out = {}
    for t in range(1, lib.y4_conv_tile_count() + 1):
        cfg = (C.c_int32 * 6)()
        ext.check(lib.y4_conv_tile_desc(t, cfg))
        out[t] = tuple(cfg)
    return out


# k, stride, cin, cout, (h, w), act, residual, upsample, out_f32, n
RECT_CONV = [
    (1, 1, 64, 64, (44, 76), "mish", False, False, False, 2),
    (1, 1, 64, 64, (76, 44), "mish", False, False, False, 2),
    (3, 1, 64, 128, (44, 76), "leaky", True, False, False, 2),
    (3, 1, 64, 128, (76, 44), "mish", True, False, False, 1),
    (3, 1, 128, 64, (11, 19), "mish", False, False, False, 3),
    (3, 2, 64, 128, (44, 76), "mish", False, False, False, 1),
    (3, 2, 32, 64, (76, 44), "leaky", False, False, False, 2),
    (3, 2, 128, 256, (22, 38), "leaky", False, False, False, 2),
    (1, 1, 256, 128, (11, 19), "leaky", False, True, False, 2),
    (1, 1, 256, 255, (19, 11), None, False, False, True, 2),
]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", RECT_CONV, ids=lambda c: f"k{c[0]}s{c[1]}_{c[2]}to{c[3]}_{c[4][0]}x{c[4][1]}")
def test_rect_conv_every_tile_vs_oracle(case, dtype):
    """Every tile id (implicit GEMM 16x16 and 32x32, p8, halo, halo2 KC 64 / KC 32, split-K) on an H != W plane: each that
    accepts the conv matches the oracle; one that does not fit is refused (-22), never run.  Tiles of one summation order
    agree bit for bit among themselves."""
    from yolo4hip import ext
    from yolo4hip.weights import ConvWeights
    k, stride, cin, cout, (h, w), act, use_res, ups, out_f32, n = case
    rng = np.random.default_rng(7 * h + w + cin)
    x = quantize(rng.standard_normal((n, h, w, cin)).astype(np.float32), dtype)
    cw = make_conv_weights(rng, cout, cin, k, bn=act is not None)
    cwq = ConvWeights(w=quantize(cw.w, dtype), bn=cw.bn, bias=cw.bias)
    ho, wo = h // stride, w // stride
    res = quantize(rng.standard_normal((n, ho, wo, cout)).astype(np.float32), dtype) if use_res else None
    want = _conv_ref(x, cwq, k, stride, act, res, ups)
    atol, rtol = TOL[dtype]
    if out_f32 and dtype != "f32":
        atol, rtol = 1e-4, 1e-4
    descs = _tile_descs()
    base, _ = run_conv_gpu(x, cwq, k, stride, act, dtype, residual=res, upsample=ups, out_f32=out_f32)
    assert base.shape == want.shape
    err = np.abs(base - want)
    assert np.all(err <= atol + rtol * np.abs(want)), f"heuristic tile: max err {err.max():.3e}"
    ran, kinds = 0, set()
    tiles = list(descs) + [t + 100 * e for t in descs if 2 <= descs[t][5] <= 7 for e in (1, 2)]
    for tile in tiles:
        try:
            got, _ = run_conv_gpu(x, cwq, k, stride, act, dtype, residual=res, upsample=ups, out_f32=out_f32, tile=tile)
        except ext.Y4Error as e:
            assert e.code == -22, (tile, e)
            continue
        ran += 1
        nst = descs[tile % 100][5]
        kinds.add(nst if tile < 100 else "splitk")
        other_order = tile >= 100 or nst in (21, 32)
        f = 2 if other_order else 1
        err = np.abs(got - want)
        assert np.all(err <= f * (atol + rtol * np.abs(want))), f"tile {tile}: max err {err.max():.3e}"
        if not other_order and nst != 10 and not out_f32:
            assert np.array_equal(got, base) or dtype == "f32", f"tile {tile} differs from the heuristic tile"
    assert ran >= 4
    if k == 3 and stride == 1 and dtype != "f32" and cout >= 128:
        assert 20 in kinds or 21 in kinds, kinds          # a halo / halo2 tile ran on the 44 x 76 / 76 x 44 planes


def test_rect_halo_tile_that_does_not_fit_is_refused():
    """A plane wider than a halo tile's pixel block (W + 2 halo columns in LDS) is refused by every halo / halo2 id."""
    from yolo4hip import ext
    from yolo4hip.weights import ConvWeights
    rng = np.random.default_rng(1)
    x = quantize(rng.standard_normal((1, 4, 416, 64)).astype(np.float32), "bf16")
    cw = make_conv_weights(rng, 64, 64, 3)
    cwq = ConvWeights(w=quantize(cw.w, "bf16"), bn=cw.bn)
    for tile, d in _tile_descs().items():
        if d[5] in (20, 21) and d[0] < 416:
            with pytest.raises(ext.Y4Error) as ei:
                run_conv_gpu(x, cwq, 3, 1, "mish", "bf16", tile=tile)
            assert ei.value.code == -22


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("hw", [(19, 11), (11, 19), (12, 24)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("variant", ["lds", "global"])
def test_spp_hw_vs_oracle(hw, dtype, variant):
    import torch
    from oracle.forward import spp_concat
    from yolo4hip import ext
    from helpers import torch_dtype
    lib = ext.load()
    h, w = hw
    epc = 4 if dtype == "f32" else 8
    c = 4 * epc if variant == "lds" else epc      # the LDS variant needs c % (2 * epc) == 0; c = epc takes the global one
    rng = np.random.default_rng(h * 100 + w + c)
    x = quantize(rng.standard_normal((2, h, w, c)).astype(np.float32), dtype)
    buf = torch.full((2, h, w, 4 * c), 3.0, dtype=torch_dtype(dtype), device="cuda:0")
    buf[..., 3 * c:] = torch.from_numpy(x).to("cuda:0").to(buf.dtype)
    ext.check(lib.y4_spp_hw(ext.DTYPE_IDS[dtype], ext.ptr(buf), 2, h, w, c, ext.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(buf.float().cpu().numpy(), spp_concat(x))


# ------------------------------------------------------------------ decode + NMS
def _bare_engine(H, W, ncls, n, dtype="bf16"):
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    cfg = make_config((H, W))
    eng = Engine(ncls, cfg, max_batch=n, dtype=dtype)
    eng.adopt_packed()
    return cfg, eng


def _compare_decode(eng, cfg, heads, H, W, ncls, iou=-1.0, score=-1.0):
    n = eng.set_heads(heads)
    got = [o.cpu().numpy() for o in eng.decode_nms_device(n, None, iou, score)]
    ref = rect_inference_from_heads(heads, ncls, cfg["anchors"], cfg["xyscale"], H, W,
                                    iou_threshold=cfg["iou_threshold"] if iou < 0 else iou,
                                    score_threshold=cfg["score_threshold"] if score < 0 else score)
    assert np.array_equal(got[3], ref[3]), (got[3], ref[3])
    assert np.array_equal(got[4], ref[4])
    assert np.array_equal(got[2], ref[2])
    assert np.abs(got[0] - ref[0]).max() < 1e-5
    assert np.abs(got[1] - ref[1]).max() < 1e-6
    return got


@pytest.mark.parametrize("hw,ncls,n,obj_bias,cls_bias", [
    ((352, 608), 80, 2, -3.0, -3.0),
    ((608, 352), 3, 2, -1.0, 0.0),
    ((352, 608), 200, 1, -2.0, -3.0),       # 3 (5 + C) > 256: the box-per-lane decode kernel
])
def test_rect_decode_nms_random_logits(hw, ncls, n, obj_bias, cls_bias):
    H, W = hw
    cfg, eng = _bare_engine(H, W, ncls, n)
    heads = _random_heads(np.random.default_rng(H + W + ncls), n, H, W, ncls, obj_bias, cls_bias)
    got = _compare_decode(eng, cfg, heads, H, W, ncls)
    assert got[3].min() > 0
    eng.close()


def test_rect_decode_closed_form_cell():
    """One box at known pixels: cell (row 5, col 30) of the stride-16 scale of a 352 x 608 input, anchor 1, zero offsets ->
    centre ((30 + 0.5) * 16, (5 + 0.5) * 16) = (488, 88), size = that scale's anchor 1 (76, 55).  x is divided by W = 608, y by
    H = 352, and the box index is scale-0 boxes + (5 * 38 + 30) * 3 + 1."""
    H, W, ncls = 352, 608, 2
    cfg, eng = _bare_engine(H, W, ncls, 1)
    heads = [np.full((1, H // s, W // s, 3 * (5 + ncls)), -20.0, np.float32) for s in (8, 16, 32)]
    for h in heads:
        h[..., 0::7] = 0.0
        h[..., 1::7] = 0.0
        h[..., 2::7] = 0.0
        h[..., 3::7] = 0.0
    row, col, a, nf = 5, 30, 1, 5 + ncls
    heads[1][0, row, col, a * nf + 4] = 20.0          # objectness ~1
    heads[1][0, row, col, a * nf + 5 + 1] = 20.0      # class 1 ~1
    got = _compare_decode(eng, cfg, heads, H, W, ncls)
    assert got[3][0] == 1 and got[2][0, 0] == 1.0
    assert got[4][0, 0] == 3 * (H // 8) * (W // 8) + (row * (W // 16) + col) * 3 + a
    aw, ah = cfg["anchors"][(3 + a) * 2], cfg["anchors"][(3 + a) * 2 + 1]
    cx, cy = (col + 0.5) * 16, (row + 0.5) * 16
    want = np.array([(cx - aw / 2) / W, (cy - ah / 2) / H, (cx + aw / 2) / W, (cy + ah / 2) / H])
    assert np.abs(got[0][0, 0] - np.clip(want, 0, 1)).max() < 1e-6, (got[0][0, 0], want)
    eng.close()


# ------------------------------------------------------------------ whole forwards
def _setup(hw, ncls, n, dtype, seed=0, **kw):
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(hw)
    plan = build_plan(hw, ncls)
    ws = W.synth_weights(plan, seed)
    imgs = W.synth_images(n, hw, seed)
    eng = Engine(ncls, cfg, max_batch=n, dtype=dtype, **kw)
    eng.load_weight_blob(W.flatten(ws))
    return cfg, plan, ws, imgs, eng


_ORACLE = {}


def _oracle_heads(hw, ncls, n, seed=0):
    key = (hw, ncls, n, seed)
    if key not in _ORACLE:
        from oracle import forward as OF
        from yolo4hip import weights as W
        from yolo4hip.plan import build_plan
        ws = W.synth_weights(build_plan(hw, ncls), seed)
        _ORACLE[key] = OF.yolo_model_forward(W.synth_images(n, hw, seed), ws, ncls)
    return _ORACLE[key]


@pytest.mark.parametrize("hw,n", [((352, 608), 2), ((608, 352), 2), ((96, 160), 3)], ids=["352x608", "608x352", "96x160"])
def test_rect_fp32_forward_vs_oracle(hw, n):
    H, W = hw
    ncls = 3
    cfg, plan, ws, imgs, eng = _setup(hw, ncls, n, "f32")
    ref = _oracle_heads(hw, ncls, n)
    heads = eng.forward_heads(imgs)
    for a, b, s in zip(heads, ref, (8, 16, 32)):
        assert a.shape == b.shape == (n, H // s, W // s, 3 * (5 + ncls))
        assert np.abs(a - b).max() < 1e-3, np.abs(a - b).max()
    boxes, scores, classes, valid, kept = eng.predict(imgs, with_indices=True)
    rb, rs, rc, rv, ri = rect_inference_from_heads(ref, ncls, cfg["anchors"], cfg["xyscale"], H, W)
    for b in range(n):
        frac, ds, db = detection_agreement(kept[b], classes[b], scores[b], boxes[b], valid[b], ri[b], rc[b], rs[b], rb[b], rv[b])
        assert frac >= 0.95 and ds < 1e-3 and db < 1e-3, (b, frac, ds, db)
    eng.close()


@pytest.mark.parametrize("dtype,tol,min_common", [("bf16", 0.40, 0.86), ("f16", 0.049, 0.96)])
def test_rect_16bit_forward_close_to_fp32_oracle(dtype, tol, min_common):
    hw, ncls, n = (352, 608), 3, 2
    cfg, plan, ws, imgs, eng = _setup(hw, ncls, n, dtype)
    ref = _oracle_heads(hw, ncls, n)
    for a, b in zip(eng.forward_heads(imgs), ref):
        err = np.abs(a - b)
        assert np.isfinite(a).all()
        assert err.mean() < tol / 5 and np.quantile(err, 0.999) < tol, (err.mean(), err.max())
    boxes, scores, classes, valid, kept = eng.predict(imgs, with_indices=True)
    rb, rs, rc, rv, ri = rect_inference_from_heads(ref, ncls, cfg["anchors"], cfg["xyscale"], *hw)
    for b in range(n):
        common = len(set(zip(kept[b, :valid[b]].tolist(), classes[b, :valid[b]].tolist())) &
                     set(zip(ri[b, :rv[b]].tolist(), rc[b, :rv[b]].tolist())))
        assert common >= min_common * rv[b], (common, rv[b])
    eng.close()


def _snapshot(eng, n):
    """Every materialised conv output (shapes from y4_layer_dims), the heads and the detections, as host arrays."""
    import torch
    from yolo4hip import ext
    snap = {}
    dims = (C.c_int32 * 4)()
    for i in range(110):
        ext.check(eng.lib.y4_layer_dims(eng.handle, i, dims))
        up = 2 if i in (78, 85) else 1
        cout = eng.layer_table()[i]["cout"] if not hasattr(eng, "_couts") else eng._couts[i]
        out = torch.empty((n, dims[2] * up, dims[3] * up, cout), dtype=torch.float32, device=eng.device)
        if eng.lib.y4_get_conv_output(eng.handle, i, n, ext.ptr(out), out.numel(), ext.stream_ptr()) == 0:
            snap[f"conv{i}"] = out.cpu().numpy()
    for k, h in enumerate(eng.heads_device(n)):
        snap[f"head{k}"] = h.cpu().numpy()
    for name, t in zip(("boxes", "scores", "classes", "valid", "kept"), eng.decode_nms_device(n)):
        snap[name] = t.cpu().numpy()
    return snap


def _same(a, b):
    for k in a:
        if k in b:
            assert np.array_equal(a[k], b[k]), k
    for k in ("head0", "head1", "head2", "boxes", "scores", "classes", "valid", "kept"):
        assert k in a and k in b


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rect_fusions_and_schedules_bit_identical(dtype):
    """On a 352 x 608 batch: chain, stage and residual-block fusion on == all off, for every tensor they leave behind; the
    heuristic == a tuned schedule without split-K or halo2 ids; sub-batching; y4_forward_u8 == the float path; two runs of a
    tuned schedule with halo2 ids agree.  Stem fusion is square-only and refused here."""
    import torch
    from yolo4hip import ext, schedule
    hw, n = (352, 608), 2
    cfg, plan, ws, imgs, eng = _setup(hw, 3, n, dtype, seed=6)
    eng._couts = [lt["cout"] for lt in eng.layer_table()]
    dev = torch.from_numpy(imgs).to(eng.device)
    eng.forward_device(dev)
    base = _snapshot(eng, n)
    with pytest.raises(ext.Y4Error):
        eng.set_stem_fusion(True)
    assert eng.set_chain_fusion(True) > 0
    assert eng.set_stage_fusion(True) == 1                 # 176 x 304 at the first CSP stage: both multiples of 16
    assert eng.set_res_fusion(True) > 0
    eng.forward_device(dev)
    _same(base, _snapshot(eng, n))
    tiles = eng.autotune(n, reps=1)                        # tuned without split-K / halo2 ids: the same bits
    assert not schedule.uses_halo2(eng.lib, tiles) and not schedule.uses_splitk(tiles)
    eng.forward_device(dev)
    _same(base, _snapshot(eng, n))
    eng.set_subbatch(1, 16)
    eng.forward_device(dev)
    _same(base, _snapshot(eng, n))
    eng.set_subbatch(0)
    # uint8 frames: the stem's /255 == the float32 path on float32(v / 255.)
    u8 = (np.random.default_rng(4).integers(0, 256, (n, *hw, 3))).astype(np.uint8)
    f = torch.from_numpy((u8 / 255.).astype(np.float32)).to(eng.device)
    eng.forward_device(f)
    a = _snapshot(eng, n)
    eng.forward_device(torch.from_numpy(u8).to(eng.device))
    _same(a, _snapshot(eng, n))
    # halo2 ids may be tuned in: another fixed summation order, deterministic run to run
    eng.set_halo2(True)
    eng.autotune(n, reps=1)
    eng.forward_device(dev)
    h1 = _snapshot(eng, n)
    eng.forward_device(dev)
    _same(h1, _snapshot(eng, n))
    eng.close()


def test_square_create_hw_same_bits_as_create():
    """A square engine (created through y4_create_hw) gives the bits of a handle made by y4_create on the same workspaces."""
    from yolo4hip import ext
    for dtype in ("bf16", "f32"):
        cfg, plan, ws, imgs, eng = _setup(416, 3, 2, dtype, seed=2)
        a = eng.predict(imgs, with_indices=True)
        ha = eng.forward_heads(imgs)
        h2 = C.c_void_p()
        ext.check(eng.lib.y4_create(C.byref(eng.cfg), C.byref(h2)))
        ab, wb = C.c_size_t(), C.c_size_t()
        ext.check(eng.lib.y4_workspace_bytes(h2, C.byref(ab), C.byref(wb)))
        assert (ab.value, wb.value) == (eng.act_bytes, eng.wts_bytes)
        ext.check(eng.lib.y4_bind_workspace(h2, ext.ptr(eng.act), eng.act_bytes, ext.ptr(eng.wts), eng.wts_bytes))
        ext.check(eng.lib.y4_adopt_packed_weights(h2))
        own, eng.handle = eng.handle, h2
        b = eng.predict(imgs, with_indices=True)
        hb = eng.forward_heads(imgs)
        eng.handle = own
        eng.lib.y4_destroy(h2)
        for x, y in zip(a + ha, b + hb):
            assert np.array_equal(x, y)
        eng.close()


# ------------------------------------------------------------------ the facade
def test_rect_facade(tmp_path, monkeypatch):
    from PIL import Image
    from yolo4hip import prepost
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    monkeypatch.setenv("YOLO4HIP_CACHE", str(tmp_path / "cache"))
    cls = os.path.join(CLASS_DIR, "coco_classes.txt")
    m = Yolov4(config=make_config((352, 608)), class_name_path=cls, dtype="f16", max_batch=2, tune=True)
    assert m.img_size == (352, 608, 3) and m.output_sizes == [(44, 76), (22, 38), (11, 19)]
    assert m.schedule_source[0] == "tuned"
    path = m.schedule_source[1]
    assert os.path.basename(path).startswith("352x608_80_2_f16_") and os.path.exists(path)
    m2 = Yolov4(config=make_config((352, 608)), class_name_path=cls, dtype="f16", max_batch=2, tune=True)
    assert m2.schedule_source == ("cached", path)
    del m2
    # a 1080 x 1920 frame: device and host preprocessing give the same detections, in raw-frame pixels
    rng = np.random.default_rng(0)
    frame = np.kron(rng.integers(0, 256, (27, 48, 3)), np.ones((40, 40, 1))).astype(np.uint8)
    host = m.preprocess_img(frame)
    assert host.shape == (352, 608, 3)
    dev = m.engine.preprocess_u8(frame, as_float=True).cpu().numpy()[0]
    assert np.array_equal(dev, host.astype(np.float32))
    out_host = m.inference_model.predict(host[None])
    df = m.predict_img(frame, plot_img=False)
    out_dev = m.inference_model.predict(m.engine.preprocess_u8(frame))
    for x, y in zip(out_host, out_dev):
        assert np.array_equal(x, y)
    nv = int(out_dev[3][0])
    assert len(df) == nv
    if nv:
        bx = out_dev[0][0, :nv]
        assert np.array_equal(df["x1"].values, (bx[:, 0] * 1920).astype(np.int64))
        assert np.array_equal(df["y2"].values, (bx[:, 3] * 1080).astype(np.int64))
    # export_prediction writes pixel boxes of each raw image
    img_dir, pred_dir = tmp_path / "img", tmp_path / "pred"
    img_dir.mkdir(); pred_dir.mkdir()
    Image.fromarray(frame).save(img_dir / "a.png")
    Image.fromarray(frame[:540, :1200].copy()).save(img_dir / "b.png")
    (tmp_path / "ann.txt").write_text("a.png 1,2,3,4,0\nb.png 1,2,3,4,0\n")
    m.export_prediction(str(tmp_path / "ann.txt"), str(pred_dir), str(img_dir), bs=2)
    for name, (h, w) in (("a", (1080, 1920)), ("b", (540, 1200))):
        raw = prepost.imread_rgb(str(img_dir / f"{name}.png"))[:, :, ::-1]
        ref = m.engine.predict(np.stack([m.preprocess_img(raw)]))
        lines = (pred_dir / f"{name}.txt").read_text().splitlines()
        assert len(lines) == int(ref[3][0])
        for j, line in enumerate(lines):
            v = [float(t) for t in line.split()[-4:]]
            want = ref[0][0, j] * np.array([w, h, w, h], np.float32)
            assert np.allclose(v, want, atol=1e-3), (name, j, v, want)
    # a checkpoint refuses another img_size
    ck = str(tmp_path / "m.y4ckpt")
    m.save_model(ck)
    m.load_model(ck)
    sq = Yolov4(config=make_config(352), class_name_path=cls, dtype="f16", max_batch=1, tune=False)
    with pytest.raises(ValueError):
        sq.load_model(ck)
