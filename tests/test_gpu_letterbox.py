"""Letterbox input and mixed-size batches on the GPU: y4_resize_u8_ragged against y4_resize_u8 (stretch) and
prepost.letterbox (letterbox), y4_decode_nms_mapped against y4_decode_nms and the decode restated in NumPy, and the
Engine / Yolov4 plumbing (preprocess_u8_batch, predict(box_map=), predict_stream(letterbox=), Yolov4(letterbox=))."""
import os

import numpy as np
import pytest

from helpers import CLASS_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# up- and down-scale, odd sides, 1 x N, N x 1, one at network size (608 x 608 / 352 x 608 both appear)
SIZES = [(1080, 1920), (1920, 1080), (608, 608), (352, 608), (1, 77), (77, 1), (1, 1), (333, 501), (45, 37), (700, 300),
         (4, 1000), (601, 999)]


def _images(sizes, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        # blocks of random colour with noise: bilinear taps hit real gradients, not only flat areas
        base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
        img = np.kron(base, np.ones((8, 8, 1)))[:h, :w] + rng.integers(-20, 21, (h, w, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _ragged(imgs, H, W, rects, pad):
    """y4_resize_u8_ragged straight through the C ABI: packed sources + a descriptor table -> uint8 [n,H,W,3] on the host."""
    import torch
    from yolo4hip import ext
    lib = ext.load()
    n = len(imgs)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(DEV)
    desc = (ext.y4_image_desc * n)()
    off = 0
    for i, (a, r) in enumerate(zip(imgs, rects)):
        desc[i].offset, desc[i].h, desc[i].w = off, a.shape[0], a.shape[1]
        desc[i].out_h, desc[i].out_w, desc[i].pad_top, desc[i].pad_left = r
        off += a.size
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
    out = torch.full((n, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    ext.check(lib.y4_resize_u8_ragged(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(out), H, W, pad, ext.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _resize_one(img, H, W):
    import torch
    from yolo4hip import ext
    lib = ext.load()
    d = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
    out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=DEV)
    ext.check(lib.y4_resize_u8(ext.ptr(d), 1, img.shape[0], img.shape[1], ext.ptr(out), H, W, ext.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


# (37, 61): H * W is no multiple of 4 -> the one-pixel-per-thread variant
CANVASES = [(608, 608), (352, 608), (37, 61)]


@pytest.mark.parametrize("H,W", CANVASES)
def test_ragged_stretch_same_bytes_as_resize_u8(H, W):
    imgs = _images(SIZES, seed=H + W)
    got = _ragged(imgs, H, W, [(H, W, 0, 0)] * len(imgs), 128)
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], _resize_one(a, H, W)), (i, a.shape)


@pytest.mark.parametrize("H,W", CANVASES)
@pytest.mark.parametrize("pad", [128, 0])
def test_ragged_letterbox_same_bytes_as_host_letterbox(H, W, pad):
    from yolo4hip import prepost
    imgs = _images(SIZES, seed=3 * H + W)
    rects = [prepost.letterbox_rect(a.shape[0], a.shape[1], H, W) for a in imgs]
    got = _ragged(imgs, H, W, rects, pad)
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], prepost.letterbox(a, (H, W), pad)), (i, a.shape)


# ------------------------------------------------------------------ engine-level preprocessing
def _engine(hw, ncls=3, n=4, dtype="f32", weights=False, seed=0):
    from yolo4hip import weights as Wt
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(hw)
    eng = Engine(ncls, cfg, max_batch=n, dtype=dtype, device=DEV)
    if weights:
        eng.load_weight_blob(Wt.flatten(Wt.synth_weights(build_plan(hw, ncls), seed)))
    else:
        eng.adopt_packed()                      # decode / NMS tests drive the heads through y4_set_heads
    return cfg, eng


@pytest.mark.parametrize("hw", [(160, 160), (96, 160)])
def test_preprocess_u8_batch(hw):
    from yolo4hip import prepost
    H, W = hw
    _, eng = _engine(hw, n=len(SIZES))
    imgs = _images(SIZES, seed=5)
    imgs[1] = imgs[1][:, ::-1]                  # a non-contiguous view (BGR-style) is packed as well
    u8, bm = eng.preprocess_u8_batch(imgs)
    assert np.array_equal(u8.cpu().numpy(), eng.preprocess_u8([np.ascontiguousarray(a) for a in imgs]).cpu().numpy())
    assert np.array_equal(bm.cpu().numpy(), np.tile(np.float32([1, 0, 1, 0]), (len(imgs), 1)))
    u8, bm = eng.preprocess_u8_batch(imgs, letterbox=True, pad_value=90)
    got, maps = u8.cpu().numpy(), bm.cpu().numpy()
    for i, a in enumerate(imgs):
        assert np.array_equal(got[i], prepost.letterbox(a, hw, 90))
        assert np.array_equal(maps[i], prepost.box_map(a.shape[0], a.shape[1], H, W))
    # the pinned staging buffer is reused: a second, smaller call gives its own results
    u8b, _ = eng.preprocess_u8_batch(imgs[:2], letterbox=True, pad_value=90)
    assert np.array_equal(u8b.cpu().numpy(), got[:2])
    with pytest.raises(ValueError):
        eng.preprocess_u8_batch([imgs[0].astype(np.float32)])
    eng.close()


# ------------------------------------------------------------------ mapped decode / NMS
def _random_heads(rng, n, H, W, ncls, obj_bias=-2.0, cls_bias=-1.0, gain=1.5):
    heads = []
    nf = 5 + ncls
    for s in (8, 16, 32):
        h = (rng.standard_normal((n, H // s, W // s, 3, nf)) * gain).astype(np.float32)
        h[..., 2:4] *= 0.6                      # boxes big enough to cross the canvas border now and then
        h[..., 4] += obj_bias
        h[..., 5:] += cls_bias
        heads.append(h.reshape(n, H // s, W // s, 3 * nf))
    return heads


def _decoded_boxes(heads, ncls, cfg, H, W):
    """Unclipped normalised boxes [n, nbox, 4] (x1, y1, x2, y2) in the decode's box order.  Square: the oracle's
    get_boxes + flatten_for_nms.  Rectangle: the reference's get_boxes (custom_layers.py:221-258) restated for a (gh, gw)
    grid -- x = column, y = row -- with x divided by W and y by H (custom_layers.py:284 divides by input_shape[0])."""
    from oracle import decode_nms as OD
    if H == W:
        head = OD.yolov4_head(heads, ncls, cfg["anchors"], cfg["xyscale"])
        return OD.flatten_for_nms(head, H, ncls)[0]
    F32 = np.float32
    anchors = np.asarray(cfg["anchors"], F32).reshape(3, 3, 2)
    n = heads[0].shape[0]
    out = []
    for s, stride in enumerate((8, 16, 32)):
        gh, gw = heads[s].shape[1:3]
        pred = np.asarray(heads[s], F32).reshape(n, gh, gw, 3, 5 + ncls)
        xy = OD.sigmoid(pred[..., 0:2])
        gx, gy = np.meshgrid(np.arange(gw), np.arange(gh))
        grid = np.stack([gx, gy], axis=-1)[:, :, None, :].astype(F32)
        xys = cfg["xyscale"][s]
        xy = ((xy * F32(xys)) - F32(0.5 * (xys - 1)) + grid) * F32(stride)
        wh = np.exp(pred[..., 2:4]).astype(F32) * anchors[s]
        out.append(np.concatenate([xy - wh / F32(2), xy + wh / F32(2)], axis=-1).astype(F32).reshape(n, -1, 4))
    return (np.concatenate(out, axis=1) / np.array([W, H, W, H], F32)).astype(F32)


def _mapped(eng, n, box_map):
    import torch
    outs = eng.decode_nms_device(n, None, box_map=box_map)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _plain(eng, n):
    import torch
    outs = eng.decode_nms_device(n, None)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _null_map_call(eng, n):
    """y4_decode_nms_mapped with box_map_dev == NULL, through the C ABI."""
    import torch
    from yolo4hip import ext
    b, s, c, v, k = eng.alloc_outputs(n)
    ext.check(eng.lib.y4_decode_nms_mapped(eng.handle, n, -1.0, -1.0, None, ext.ptr(b), ext.ptr(s), ext.ptr(c), ext.ptr(v),
                                           ext.ptr(k), ext.stream_ptr()))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in (b, s, c, v, k)]


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("hw", [(160, 160), (96, 160)])
def test_mapped_identity_and_null_equal_plain_on_set_heads(hw):
    import torch
    H, W = hw
    ncls, n = 4, 3
    cfg, eng = _engine(hw, ncls, n)
    heads = _random_heads(np.random.default_rng(H * 7 + W), n, H, W, ncls)
    eng.set_heads(heads)
    plain = _plain(eng, n)
    assert plain[3].min() > 0
    eng.set_heads(heads)
    ident = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * n, dtype=torch.float32, device=DEV)
    _same_bits(_mapped(eng, n, ident), plain)
    eng.set_heads(heads)
    _same_bits(_null_map_call(eng, n), plain)
    eng.close()


@pytest.mark.parametrize("hw", [(160, 160), (96, 160)])
def test_mapped_identity_equals_plain_after_forward(hw):
    import torch
    from yolo4hip import weights as Wt
    _, eng = _engine(hw, 3, 2, weights=True)
    imgs = torch.from_numpy(Wt.synth_images(2, hw, seed=4)).to(DEV)
    eng.forward_device(imgs)
    plain = _plain(eng, 2)
    eng.forward_device(imgs)
    ident = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 2, dtype=torch.float32, device=DEV)
    _same_bits(_mapped(eng, 2, ident), plain)
    eng.forward_device(imgs)
    _same_bits(_null_map_call(eng, 2), plain)
    # and y4_predict's own decode is the same as forward + y4_decode_nms
    pred = [o.cpu().numpy() for o in eng.predict_device(imgs)]
    _same_bits(pred, plain)
    eng.close()


@pytest.mark.parametrize("hw", [(160, 160), (96, 160), (352, 608)])
def test_mapped_letterbox_maps(hw):
    import torch
    from yolo4hip import prepost
    H, W = hw
    ncls, n = 3, 4
    cfg, eng = _engine(hw, ncls, n)
    heads = _random_heads(np.random.default_rng(H + 3 * W), n, H, W, ncls)
    srcs = [(1080, 1920), (1920, 1080), (7, 3), (H, W)]
    maps = np.stack([prepost.box_map(h, w, H, W) for h, w in srcs])
    eng.set_heads(heads)
    plain = _plain(eng, n)
    eng.set_heads(heads)
    got = _mapped(eng, n, torch.from_numpy(maps).to(DEV))
    for i in (1, 2, 3, 4):                                   # scores, classes, valid, kept_idx: bit for bit
        assert np.array_equal(got[i], plain[i])
    assert plain[3].min() > 0
    dboxes = _decoded_boxes(heads, ncls, cfg, H, W)
    for b in range(n):
        k = int(plain[3][b])
        idx = plain[4][b, :k]
        m = maps[b]
        # against the unclipped decoded boxes (oracle / restatement): the decode agrees with them to 1e-5 (the tolerance of
        # the decode tests), which the map scales by up to max(ax, ay)
        ref = prepost.map_boxes(dboxes[b, idx], m)
        tol = 1e-5 * max(1.0, float(m[0]), float(m[2]))
        assert np.abs(got[0][b, :k] - ref).max() < tol, (b, np.abs(got[0][b, :k] - ref).max())
        # against the device's own canvas boxes: a canvas coordinate outside [0, 1] maps outside [0, 1] (the content rectangle
        # lies inside the canvas), so clipping before the map changes nothing after it -- the map alone, to 1e-6
        x = plain[0][b, :k].astype(np.float64)
        exact = np.empty_like(x)
        exact[:, [0, 2]] = x[:, [0, 2]] * m[0] + m[1]
        exact[:, [1, 3]] = x[:, [1, 3]] * m[2] + m[3]
        exact = np.clip(exact, 0, 1)
        assert np.abs(got[0][b, :k] - exact).max() < 1e-6
        assert got[0][b, :k].min() >= 0 and got[0][b, :k].max() <= 1
        assert (got[0][b, k:] == 0).all()
    eng.close()


# ------------------------------------------------------------------ streaming
@pytest.mark.parametrize("hw", [(160, 160), (96, 160)])
def test_predict_stream_letterbox(hw):
    _, eng = _engine(hw, 3, 2, weights=True)
    frames = _images([(90, 200)] * 6, seed=11)
    batches = [np.stack(frames[i:i + 2]) for i in range(0, 6, 2)]
    got = list(eng.predict_stream(batches, with_indices=True, letterbox=True, pad_value=100))
    assert len(got) == 3
    for b, res in zip(batches, got):
        u8, bm = eng.preprocess_u8_batch(list(b), letterbox=True, pad_value=100)
        want = eng.predict(u8, with_indices=True, box_map=bm)
        _same_bits(res, want)
    # stretch through the same generator is unchanged
    got = list(eng.predict_stream(batches[:1], with_indices=True))
    u8, _ = eng.preprocess_u8_batch(list(batches[0]))
    _same_bits(got[0], eng.predict(u8, with_indices=True))
    eng.close()


# ------------------------------------------------------------------ facade
def _facade(hw, dtype, tmp_path, monkeypatch, **kw):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    monkeypatch.setenv("YOLO4HIP_CACHE", str(tmp_path / "cache"))
    return Yolov4(config=make_config(hw), class_name_path=os.path.join(CLASS_DIR, "coco_classes.txt"), dtype=dtype,
                  max_batch=2, tune=False, **kw)


def _host_letterbox_outputs(m, raw):
    """prepost.letterbox -> float -> inference_model.predict -> NumPy map + clip."""
    from yolo4hip import prepost
    H, W = m.img_size[0], m.img_size[1]
    img = prepost.letterbox(raw, (H, W), m._pad_value) / 255.
    b, s, c, v = m.inference_model.predict(img[None])
    nv = int(v[0])
    mapped = np.zeros_like(b)
    mapped[0, :nv] = prepost.map_boxes(b[0, :nv], prepost.box_map(raw.shape[0], raw.shape[1], H, W))
    return [mapped, s, c, v]


def _write_images(tmp_path, raws):
    from PIL import Image
    img_dir, pred_dir = tmp_path / "img", tmp_path / "pred"
    img_dir.mkdir(exist_ok=True); pred_dir.mkdir(exist_ok=True)
    lines = []
    for i, r in enumerate(raws):
        Image.fromarray(r).save(img_dir / f"im{i}.png")
        lines.append(f"im{i}.png 1,2,3,4,0\n")
    (tmp_path / "ann.txt").write_text("".join(lines))
    return img_dir, pred_dir


@pytest.mark.parametrize("hw", [(320, 320), (352, 608)], ids=["320", "352x608"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_facade_letterbox(hw, dtype, tmp_path, monkeypatch):
    from yolo4hip import prepost
    m = _facade(hw, dtype, tmp_path, monkeypatch, letterbox=True, pad_value=128)
    H, W = hw
    raws = _images([(720, 1280), (1280, 720), (301, 199)], seed=H + W)
    for raw in raws:
        h, w = raw.shape[:2]
        out_dev = m._predict_mapped(*m.engine.preprocess_u8_batch([raw], letterbox=True, pad_value=128))
        out_host = _host_letterbox_outputs(m, raw)
        nv = int(out_dev[3][0])
        assert nv == int(out_host[3][0])
        assert np.array_equal(out_dev[2], out_host[2]) and np.array_equal(out_dev[1], out_host[1])
        # boxes within 1e-5 x the image size, in pixels
        err = np.abs(out_dev[0] - out_host[0]).max()
        assert err < 1e-5, err
        df = m.predict_img(raw, plot_img=False)
        assert len(df) == nv
        ref_df = prepost.get_detection_data(raw, out_dev[:4], m.class_names)
        for col in ("x1", "y1", "x2", "y2", "score"):
            assert np.array_equal(df[col].values, ref_df[col].values), col
        if nv:
            assert df["x1"].min() >= 0 and df["x2"].max() <= w and df["y1"].min() >= 0 and df["y2"].max() <= h
    # device_preprocess=False: the host letterbox and the same device map give the same detections
    m._device_preprocess = False
    df_host = m.predict_img(raws[0], plot_img=False)
    m._device_preprocess = True
    df_dev = m.predict_img(raws[0], plot_img=False)
    assert len(df_host) == len(df_dev)
    assert np.array_equal(df_host["score"].values, df_dev["score"].values)
    if len(df_dev):
        assert np.abs(df_host[["x1", "y1", "x2", "y2"]].values - df_dev[["x1", "y1", "x2", "y2"]].values).max() <= 1
    # export_prediction agrees with predict_img on each image (BGR order, as the reference feeds it)
    img_dir, pred_dir = _write_images(tmp_path, raws)
    m.export_prediction(str(tmp_path / "ann.txt"), str(pred_dir), str(img_dir), bs=2)
    for i in range(len(raws)):
        bgr = prepost.imread_rgb(str(img_dir / f"im{i}.png"))[:, :, ::-1]
        h, w = bgr.shape[:2]
        ref = m._predict_mapped(*m.engine.preprocess_u8_batch([bgr], letterbox=True, pad_value=128))
        lines = (pred_dir / f"im{i}.txt").read_text().splitlines()
        assert len(lines) == int(ref[3][0])
        for j, line in enumerate(lines):
            v = [float(t) for t in line.split()[-4:]]
            want = ref[0][0, j] * np.array([w, h, w, h], np.float32)
            assert np.allclose(v, want, atol=1e-3), (i, j, v, want)
            assert 0 <= v[0] <= w and 0 <= v[2] <= w and 0 <= v[1] <= h and 0 <= v[3] <= h


def _export_old_way(m, annotation_path, pred_folder_path, img_folder_path, bs):
    """export_prediction's stretch path as it was before preprocess_u8_batch: one preprocess_u8 per image."""
    from yolo4hip import prepost
    with open(annotation_path) as fh:
        img_paths = [os.path.join(img_folder_path, line.split(' ')[0].split(os.sep)[-1].strip()) for line in fh]
    for start in range(0, len(img_paths), bs):
        paths = img_paths[start:start + bs]
        raws = [prepost.imread_rgb(pth)[:, :, ::-1] for pth in paths]
        imgs = m.engine.preprocess_u8([np.ascontiguousarray(r) for r in raws])
        b_boxes, b_scores, b_classes, b_valid = m.inference_model.predict(imgs)
        for k, pth in enumerate(paths):
            nb = int(b_valid[k])
            h, w = raws[k].shape[:2]
            boxes = b_boxes[k, :nb]
            boxes[:, [0, 2]] *= w
            boxes[:, [1, 3]] *= h
            names = [m.class_names[int(c)] for c in b_classes[k, :nb]]
            stem = pth.split(os.sep)[-1].split('.')[0]
            with open(os.path.join(pred_folder_path, stem + '.txt'), 'w') as out:
                for j in range(nb):
                    b = boxes[j]
                    out.write(f'{names[j]} {b_scores[k, j]} {b[0]} {b[1]} {b[2]} {b[3]}\n')


@pytest.mark.parametrize("hw", [(320, 320), (352, 608)], ids=["320", "352x608"])
def test_facade_stretch_export_unchanged(hw, tmp_path, monkeypatch):
    m = _facade(hw, "f16", tmp_path, monkeypatch)
    raws = _images([(720, 1280), (1280, 720), (301, 199), (hw[0], hw[1]), (33, 47)], seed=7)
    img_dir, pred_dir = _write_images(tmp_path, raws)
    old_dir = tmp_path / "old"
    old_dir.mkdir()
    m.export_prediction(str(tmp_path / "ann.txt"), str(pred_dir), str(img_dir), bs=2)
    _export_old_way(m, str(tmp_path / "ann.txt"), str(old_dir), str(img_dir), 2)
    for i in range(len(raws)):
        assert (pred_dir / f"im{i}.txt").read_bytes() == (old_dir / f"im{i}.txt").read_bytes(), i
