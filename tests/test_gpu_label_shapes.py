"""The label and training kernels (y4_loss_assign, y4_loss, y4_loss_grad, y4_head_grad, y4_block_grad; csrc/loss.hip, loss_common.h,
grad_common.h, head_train.hip, block_train.hip) at every max_boxes and class count the library accepts and no other GPU test runs
at: 1, 64, 65, 129 and 256 rows with 1, 32, 33, 64 and 65 classes (loss_cases.LABEL_CASES).  tests/test_label_shapes_cpu.py holds
the cases to their conditions and says which path of the kernels each one reaches.

What "right" is: the assignment exactly (yolo4hip.data.records_from_boxes, tied to the reference's own preprocess_true_boxes by the
fixtures); the loss by the rule of tests/test_gpu_loss.py, relative distance to the float64 restatement <= max(4 x d_ref, 1e-6) per
(scale, term), d_ref the reference's own float32 error from the fixture; the gradients by the rule of tests/test_gpu_fit.py,
rel_to_max <= max(4 x d_ref, 1e-6), d_ref from the oracles alone (their float32 evaluation for a float32 handle, dZ rounded to the
operand type for a 16-bit one).  Every distance goes beside its budget to profiles/loss/parity_measured.json and
profiles/fit/parity_measured.json.

One engine per case serves tests 1 .. 4 (heads set from the case), one pair of engines per (case, dtype) tests 5 and 6 (a real
forward; the second, non-aliased and unfused, is the tap the oracle's inputs are read from)."""
import ctypes as C
import os

import numpy as np
import pytest

import blockgrad_oracle as BO
import loss_cases as LC
import loss_oracle as LO
import lossgrad_oracle as GO
from test_gpu_fit import _bits, _within
from test_gpu_fit_blocks import BLOCK_IN, HEAD_IN, _layer_params
from test_gpu_fit_blocks_f16 import _hold_dk as _hold_dk_f16
from test_gpu_fit_blocks_f16 import round_f16, scale_for
from test_gpu_fit_geometry import CHANNELS, WEIGHTS, _block_oracle, _hold_dk, _hold_dw
from test_gpu_loss import _within_budget
from test_label_shapes_cpu import NAMES, label_fixture

pytestmark = pytest.mark.gpu
EINVAL = -22
_FLATS = {}


def _make_engine(case, dtype="f32", n=None, **kw):
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(case["hw"][0], max_boxes=case["max_boxes"])
    eng = Engine(case["ncls"], cfg, max_batch=n or case["n"], dtype=dtype, device="cuda:0", **kw)
    key = (tuple(case["hw"]), case["ncls"])
    if key not in _FLATS:                                                    # the synthetic weight stream of a class count, made once
        _FLATS[key] =W.flatten(W.synth_weights(build_plan(case["hw"], case["ncls"]), seed=2))
    flat = _FLATS[key]
    eng.load_weight_blob(flat)
    assert eng._loss_max_boxes() == case["max_boxes"] and eng.nout == 3 * (5 + case["ncls"])
    return eng, flat


@pytest.fixture(scope="module")
def engines():
    """name -> dict(case, fx, labels, eng): built on first use, closed when the module is done"""
    made = {}

    def get(name):
        if name not in made:
            case, fx, labels = label_fixture(name)
            made[name] = dict(case=case, fx=fx, labels=labels, eng=_make_engine(case)[0])
        return made[name]
    yield get
    for c in made.values():
        c["eng"].close()


@pytest.fixture(scope="module")
def forwards():
    """(name, dtype) -> the two engines after a forward of four images with the case's boxes, and the float64 side"""
    made = {}

    def get(name, dtype):
        import torch
        from yolo4hip.data import dense_from_records
        if (name, dtype) in made:
            return made[(name, dtype)]
        case = LC.make_label_case(name)
        hw, ncls, n = case["hw"], case["ncls"], case["n"]
        eng, flat = _make_engine(case, dtype, alias_workspace=True, retain_head_inputs=2)
        ref, _ = _make_engine(case, dtype)
        if dtype != "f32":
            assert eng.set_chain_fusion(True) > 0
        imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)).to(eng.device)
        eng.forward_device(imgs)
        ref.forward_device(imgs)
        heads = [h.cpu().numpy() for h in eng.heads_device(n)]
        for a, b in zip(heads, ref.heads_device(n)):
            assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
        labels = dense_from_records(case["records"], hw, ncls)

        def g64(w):
            return GO.loss_grad(heads, labels, case["true_xywh"], LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, hw, img_weight=w)
        made[(name, dtype)] = dict(eng=eng, ref=ref, flat=flat, imgs=imgs, boxes_dev=torch.from_numpy(case["boxes"]).to(eng.device),
                                   ncls=ncls, n=n, w=WEIGHTS[:n].copy(), g64=g64, torch=torch, case=case, heads=heads)
        return made[(name, dtype)]
    yield get
    for c in made.values():
        c["eng"].close()
        c["ref"].close()


def _device_records(eng, boxes):
    import torch
    rec, cnt, xywh = eng.assign_device(torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(eng.device))
    return rec.cpu().numpy(), cnt.cpu().numpy(), xywh.cpu().numpy()


# ---- 1. the assignment
@pytest.mark.parametrize("name", NAMES)
def test_assign_gives_the_host_records_exactly(name, engines):
    from yolo4hip.data import pad_records
    c = engines(name)
    case, eng = c["case"], c["eng"]
    mb, ncls = case["max_boxes"], case["ncls"]
    rec, cnt, xywh = _device_records(eng, case["boxes"])
    want, want_cnt = pad_records(case["records"], mb, ncls)
    assert rec.shape == want.shape == (case["n"], mb, 8 + (ncls + 31) // 32)
    assert np.array_equal(cnt, want_cnt)
    assert np.array_equal(rec, want)                                         # integers and float bits, zero padding included
    assert np.array_equal(xywh.view(np.int32), c["fx"]["true_xywh"].view(np.int32))
    # every image alone and the batch reversed: the same records (a workgroup is one image)
    rev, rev_cnt, _ = _device_records(eng, case["boxes"][::-1])
    assert np.array_equal(rev, want[::-1]) and np.array_equal(rev_cnt, want_cnt[::-1])
    # an off-grid centre and a class id equal to the class count in the LAST row of the full image (wave 3 of 256 rows; for 32 and
    # 64 classes the id one past a mask word that is exactly full): count -1
    last = mb - 1
    bad = case["boxes"][[1, 1, 2]].copy()
    bad[0, last] = [150, 10, 180, 50, 0]                                     # centre x = 165 >= 160
    bad[1, last, 4] = ncls
    _, cnt_bad, _ = _device_records(eng, bad)
    assert cnt_bad.tolist() == [-1, -1, int(want_cnt[2])]
    if mb > 3 * LC.WAVE:
        assert last // LC.WAVE == 3
        inner = case["boxes"][[1, 1]].copy()
        inner[0, 3 * LC.WAVE + 8] = [150, 10, 180, 50, 0]
        inner[1, 3 * LC.WAVE + 8, 4] = -1.0
        assert _device_records(eng, inner)[1].tolist() == [-1, -1]
    with pytest.raises(ValueError, match="outside"):
        eng.loss(np.zeros((1,) + tuple(case["hw"]) + (3,), np.float32), boxes=bad[0:1])
    with pytest.raises(ValueError, match="class id"):
        eng.loss(np.zeros((1,) + tuple(case["hw"]) + (3,), np.float32), boxes=bad[1:2])


# ---- 2. the loss
@pytest.mark.parametrize("name", NAMES)
def test_loss_of_case_heads_vs_float64(name, engines):
    import torch
    from yolo4hip.engine import combine_loss
    c = engines(name)
    case, fx, labels, eng = c["case"], c["fx"], c["labels"], c["eng"]
    n = eng.set_heads(case["heads"])
    triple = eng.upload_records(case["records"], fx["true_xywh"])
    got = eng.loss_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert got.shape == (n, 3, 3) and got.dtype == np.float32
    oracle = LO.loss_terms(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH, case["hw"])
    _within_budget(f"label_shapes_{name}", got, oracle, fx["d_ref"])
    assert np.all(LO.rel_dist(got, fx["ref_img"]) <= 5.0 * np.maximum(fx["d_ref"], 1e-6))
    total = combine_loss(got)[0].mean()
    assert abs(total - float(fx["ref_total"])) <= 5e-6 * float(fx["ref_total"])
    # the host-records front and the device-assign front: the same bits
    got_b = eng.loss_device(n, boxes_dev=torch.from_numpy(case["boxes"]).to(eng.device), iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert np.array_equal(got.view(np.int32), got_b.view(np.int32))


# ---- 3. the dense gradient
@pytest.mark.parametrize("name", NAMES)
def test_loss_grad_of_case_heads_vs_float64(name, engines):
    import torch
    c = engines(name)
    case, fx, labels, eng = c["case"], c["fx"], c["labels"], c["eng"]
    n = eng.set_heads(case["heads"])
    w = WEIGHTS[:n].copy()
    args = (case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH, case["hw"])
    g64, g32 = GO.loss_grad(*args, img_weight=w), GO.loss_grad(*args, img_weight=w, dtype=np.float32)
    triple = eng.upload_records(case["records"], fx["true_xywh"])
    got = eng.loss_grad_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH, img_weight=w)
    for s in range(3):
        g = got[s].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == case["heads"][s].shape
        _within(f"label_shapes_{name}_loss_grad_scale{s}", g, g64[s], GO.rel_to_max(g32[s], g64[s]))
        # the class columns alone: a wrong mask bit moves a class logit's gradient by its image weight, which the box columns' larger
        # magnitude must not hide
        cls = np.arange(g.shape[-1]) % (5 + case["ncls"]) >= 5
        _within(f"label_shapes_{name}_loss_grad_scale{s}_class", g[..., cls], g64[s][..., cls], GO.rel_to_max(g32[s][..., cls], g64[s][..., cls]))
    got_b = eng.loss_grad_device(n, boxes_dev=torch.from_numpy(case["boxes"]).to(eng.device), iou_loss_thresh=LC.IOU_LOSS_THRESH, img_weight=w)
    for a, b in zip(_bits(got), _bits(got_b)):
        assert np.array_equal(a, b)


# ---- 4. batch and position
@pytest.mark.parametrize("name", ["mb256_c65", "mb1_c1"])
def test_loss_and_gradient_are_independent_of_batch_and_position(name, engines):
    import torch
    c = engines(name)
    case, eng = c["case"], c["eng"]
    boxes = torch.from_numpy(case["boxes"]).to(eng.device)
    ones = np.ones(4, np.float32)

    def run(order):
        eng.set_heads([h[order] for h in case["heads"]])
        b = boxes[order].contiguous()
        return [eng.loss_device(len(order), boxes_dev=b).cpu().numpy().view(np.int32)] + _bits(eng.loss_grad_device(len(order), boxes_dev=b, img_weight=ones[:len(order)]))
    full = run([0, 1, 2, 3])
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [0], [1], [2], [3], [1, 1, 3]):
        for a, b in zip(full, run(order)):
            assert np.array_equal(a[order], b), order


# ---- 5. the head weight gradient after a real forward
def _wgrad_two_orders(g64, X):
    """float32 evaluation of the oracle's weight gradient over the four images at once and as two halves added: the distance of
    the two is what the order of a float32 sum costs -> (db, dW) margins"""
    g32 = g64.astype(np.float32)
    db4, dW4 = GO.head_wgrad(g32, X, np.float32)
    halves = [GO.head_wgrad(g32[i:i + 2], X[i:i + 2], np.float32) for i in (0, 2)]
    db22, dW22 = halves[0][0] + halves[1][0], halves[0][1] + halves[1][1]
    assert db22.dtype == np.float32 and dW22.dtype == np.float32
    return GO.rel_to_max(db22, db4), GO.rel_to_max(dW22, dW4)


@pytest.mark.parametrize("name,dtype", [("mb1_c1", "f32"), ("mb1_c1", "bf16"), ("mb65_c33", "f32"), ("mb65_c33", "bf16"),
                                        ("mb256_c65", "f32"), ("mb256_c65", "bf16"), ("mb256_c65", "f16")])
def test_head_grad_after_a_forward(name, dtype, forwards):
    from test_gpu_fit import _unpack
    c = forwards(name, dtype)
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    eng.forward_device(c["imgs"])
    X = [c["ref"].conv_output(i, n) for i in HEAD_IN]
    g64 = c["g64"](w)
    tag = f"label_shapes_{name}_head_grad_{dtype}"
    dw = eng.head_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert dw.numel() == sum(3 * (5 + c["ncls"]) * (1 + cout) for _, cout in CHANNELS)
    one = dw.cpu().numpy()
    _hold_dw(tag, eng, one, g64, X)
    again = eng.head_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert np.array_equal(_bits([dw])[0], _bits([again])[0])

    # the same batch as 2 + 2 images with accumulate: other rounds of the sparse pass, the same sum
    def chunked():
        acc = torch.empty_like(dw)
        w_dev = torch.from_numpy(w).to(eng.device)
        for i0 in (0, 2):
            eng.forward_device(c["imgs"][i0:i0 + 2])
            eng.head_grad_device(2, boxes_dev=c["boxes_dev"][i0:i0 + 2], img_weight=w_dev[i0:i0 + 2], dw=acc, accumulate=i0 > 0)
        return acc.cpu().numpy()
    two = chunked()
    assert np.array_equal(two.view(np.int32), chunked().view(np.int32))
    _hold_dw(tag + "_two_chunks", eng, two, g64, X)
    for s, ((db1, dW1), (db2, dW2)) in enumerate(zip(_unpack(eng, one), _unpack(eng, two))):
        m_db, m_dW = _wgrad_two_orders(g64[s], X[s])
        _within(f"{tag}_scale{s}_4_vs_2plus2_dW", dW2, dW1, m_dW)
        _within(f"{tag}_scale{s}_4_vs_2plus2_db", db2, db1, m_db)
    eng.forward_device(c["imgs"])


# ---- 6. the block gradient after a real forward
@pytest.mark.parametrize("name,dtype", [("mb1_c1", "f32"), ("mb1_c1", "bf16"), ("mb256_c65", "f32"), ("mb256_c65", "bf16")])
def test_block_grad_after_a_forward(name, dtype, forwards):
    c = forwards(name, dtype)
    eng, n, w = c["eng"], c["n"], c["w"]
    eng.forward_device(c["imgs"])
    oracle = _block_oracle(c, dtype, c["g64"](w))
    tag = f"label_shapes_{name}_block_grad_{dtype}"
    dk = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    _hold_dk(tag, eng, dk.cpu().numpy(), oracle)
    again = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert np.array_equal(_bits([dk])[0], _bits([again])[0])


def test_block_grad_scaled_f16_after_a_forward(forwards):
    name = "mb256_c65"
    c = forwards(name, "f16")
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    eng.forward_device(c["imgs"])
    U = [c["ref"].conv_output(i, n) for i in BLOCK_IN]
    A = [c["ref"].conv_output(i, n) for i in HEAD_IN]
    g64 = c["g64"](w)
    params = [(wh.astype(np.float16).astype(np.float64), BO.bn_scale(bn[1], bn[3])) for wh, _, _, bn in _layer_params(eng, c["flat"], "f16")]
    dz = [BO.block_dz(g64[s], wh, A[s], sc) for s, (wh, sc) in enumerate(params)]
    max_dz = [float(np.abs(z).max()) for z in dz]
    s_good = min(scale_for(m, 12) for m in max_dz)
    assert 2.0 ** 12 <= max(max_dz) * s_good < 2.0 ** 13
    # d_ref: dZ rounded as (dZ * S -> fp16 -> / S), subnormals kept and flushed, the larger distance (test_gpu_fit_blocks_f16)
    oracle = [(BO.block_wgrad(dz[s], U[s]), [BO.block_grad(g64[s], wh, A[s], U[s], sc, round_dz=round_f16(s_good, keep)) for keep in (True, False)])
              for s, (wh, sc) in enumerate(params)]
    dk, word = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=s_good)
    assert word.dtype == torch.int32 and int(word.cpu().numpy()[0]) == 0
    _hold_dk_f16(f"label_shapes_{name}_block_grad_scaled_f16", eng, dk.cpu().numpy(), oracle)


# ---- 7. refusals come before any launch
def test_max_boxes_outside_1_256_is_refused_at_every_entry(forwards):
    from yolo4hip import ext
    c = forwards("mb1_c1", "f32")
    eng, torch = c["eng"], c["torch"]
    eng.forward_device(c["imgs"])
    n, rows = 1, 257                                                         # buffers of 257 rows: nothing could leave them anyway
    rw = 8 + (c["ncls"] + 31) // 32
    dev = eng.device
    boxes = torch.zeros((n, rows, 5), dtype=torch.float32, device=dev)
    xywh = torch.zeros((n, rows, 4), dtype=torch.float32, device=dev)
    rec = torch.zeros((n, rows, rw), dtype=torch.int32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int32, device=dev)
    w = torch.ones((n,), dtype=torch.float32, device=dev)
    out = torch.full((n, 3, 3), 7.0, dtype=torch.float32, device=dev)
    fl = C.c_size_t()
    ext.check(eng.lib.y4_loss_scratch_floats(eng.handle, n, C.byref(fl)))
    scratch = torch.empty((fl.value,), dtype=torch.float32, device=dev)
    dense = [torch.full((n, gh, gw, eng.nout), 7.0, dtype=torch.float32, device=dev) for gh, gw in eng.grids_hw]
    dw = torch.full((eng.head_floats(),), 7.0, dtype=torch.float32, device=dev)
    dk = torch.full((eng.block_floats(),), 7.0, dtype=torch.float32, device=dev)
    hs, bs = eng._group_scratch("heads", n), eng._group_scratch("blocks", n)
    lib, h, p, st = eng.lib, eng.handle, ext.ptr, ext.stream_ptr
    for mb in (0, 257, -1):
        with torch.cuda.device(dev):
            calls = {
                "y4_loss_assign": lambda: lib.y4_loss_assign(h, n, p(boxes), mb, p(xywh), p(rec), p(cnt), st()),
                "y4_loss": lambda: lib.y4_loss(h, n, p(rec), p(cnt), p(xywh), mb, 0.5, p(scratch), fl.value, p(out), st()),
                "y4_loss_grad": lambda: lib.y4_loss_grad(h, n, p(rec), p(cnt), p(xywh), mb, 0.5, p(w), p(dense[0]), p(dense[1]), p(dense[2]), st()),
                "y4_head_grad": lambda: lib.y4_head_grad(h, n, p(rec), p(cnt), p(xywh), mb, 0.5, p(w), p(hs), hs.numel(), p(dw), dw.numel(), 0, st()),
                "y4_block_grad": lambda: lib.y4_block_grad(h, n, p(rec), p(cnt), p(xywh), mb, 0.5, p(w), p(bs), bs.numel(), p(dk), dk.numel(), 0, st()),
            }
            for who, call in calls.items():
                assert call() == EINVAL, (who, mb)
                assert b"max_boxes" in lib.y4_last_error(), (who, mb, lib.y4_last_error())
    # nothing ran: every output still holds what it held
    for t in [out, dw, dk] + dense:
        assert bool((t == 7.0).all())
    assert not rec.any() and not cnt.any()
    # the accepted ends, 1 and 256 rows of the same buffers, answer
    for mb in (1, 256):
        with torch.cuda.device(dev):
            assert lib.y4_loss_assign(h, n, p(boxes), mb, p(xywh), p(rec), p(cnt), st()) == 0
            assert lib.y4_loss(h, n, p(rec), p(cnt), p(xywh), mb, 0.5, p(scratch), fl.value, p(out), st()) == 0
        assert cnt.cpu().numpy().tolist() == [0] and np.isfinite(out.cpu().numpy()).all()
    # a boxes tensor whose second dimension is not the handle's max_boxes
    two_rows = torch.zeros((1, 2, 5), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="max_boxes=1"):
        eng.assign_device(two_rows)
    with pytest.raises(ValueError, match="max_boxes=1"):
        eng.loss_device(1, boxes_dev=two_rows)
    with pytest.raises(ValueError, match="max_boxes=1"):
        eng.head_grad_device(1, boxes_dev=two_rows)
    with pytest.raises(ValueError, match="max_boxes"):
        eng.loss(np.zeros((1, 160, 160, 3), np.float32), boxes=np.zeros((1, 100, 5), np.float32))
    with pytest.raises(ValueError, match="max_boxes"):
        eng.upload_records([np.zeros((0, rw), np.int32)], np.zeros((1, 100, 4), np.float32))


# ---- 8. the facade at 256 rows and 65 classes
def _write_crowd(tmp_path, sizes, counts, ncls):
    from PIL import Image
    rng = np.random.default_rng(3)
    lines = []
    for i, ((h, w), m) in enumerate(zip(sizes, counts)):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(tmp_path / f"im{i}.png")
        objs = []
        for k in range(m):
            x1, y1 = rng.integers(0, w - 12), rng.integers(0, h - 12)
            cls = (ncls - 1, ncls - 2, 31, 32)[k] if k < 4 else rng.integers(0, ncls)
            objs.append(f"{x1},{y1},{x1 + rng.integers(8, min(w - x1, w // 2))},{y1 + rng.integers(8, min(h - y1, h // 2))},{cls}")
        lines.append(f"im{i}.png " + " ".join(objs) + "\n")
    return lines


def test_facade_evaluate_and_fit_at_256_rows_and_65_classes(tmp_path):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    from yolo4hip.engine import Engine, combine_loss
    ncls, mb = 65, 256
    names = tmp_path / "names65.txt"
    names.write_text("".join(f"class{i}\n" for i in range(ncls)))
    cfg = make_config(160, batch_size=3, max_boxes=mb)
    m = Yolov4(None, str(names), cfg, dtype="f32", max_batch=4, synth_seed=3, tune=False)
    assert m.num_classes == ncls and m.max_boxes == mb and m.engine._loss_max_boxes() == mb
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64)]
    lines = _write_crowd(tmp_path, sizes, [150, 0, 5, 8, 1], ncls)
    gen = DataGenerator(lines, str(names), str(tmp_path), max_boxes=mb, shuffle=False, config=m.config)
    assert len(gen) == 2 and gen.max_boxes == mb and gen.num_classes == ncls
    with pytest.raises(ValueError, match="max_boxes"):
        m.evaluate(DataGenerator(lines, str(names), str(tmp_path), shuffle=False, config=m.config))      # a generator of 100 rows
    np.random.seed(11)
    res = m.evaluate(gen)
    assert res["images"] == 5
    np.random.seed(11)                                                       # (get_data shuffles each image's boxes)
    singles, crowd = [], 0
    for i in range(len(gen)):
        X, boxes = gen.boxes(i)
        assert boxes.shape[1:] == (mb, 5)
        crowd = max(crowd, int((boxes[..., 2] > boxes[..., 0]).sum(axis=1).max()))
        for k in range(len(X)):
            singles.append(m.engine.loss(X[k:k + 1], boxes=boxes[k:k + 1])[0])
    assert crowd == 150                                                      # more rows than the default 100 could carry
    total, box, conf, cls = combine_loss(np.stack(singles))
    assert res["loss"] == pytest.approx(total.mean(), rel=1e-12) and res["box"] == pytest.approx(box.mean(), rel=1e-12)
    assert res["conf"] == pytest.approx(conf.mean(), rel=1e-12) and res["class"] == pytest.approx(cls.mean(), rel=1e-12)
    # one fit step on the first batch against head_grad + head_adam at engine level: the same bits
    one = DataGenerator(lines[:3], str(names), str(tmp_path), max_boxes=mb, shuffle=False, config=m.config)
    assert len(one) == 1
    before = m._flat.copy()
    eng = Engine(ncls, m.config, max_batch=4, dtype="f32", device="cuda:0", alias_workspace=True, retain_head_inputs=1)
    eng.load_weight_blob(before)
    m.engine.copy_schedule_to(eng)
    np.random.seed(5)
    X, boxes = one.boxes(0)
    torch = eng.torch
    boxes_dev = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(eng.device)
    state = eng.head_state(before)
    chunks = list(eng._chunks(X))
    assert len(chunks) == 1
    eng.forward_device(chunks[0])
    weight = torch.full((3,), 1.0 / 3, dtype=torch.float32, device=eng.device)
    eng.head_adam_step(state, eng.head_grad_device(3, boxes_dev=boxes_dev, img_weight=weight), lr=1e-3)
    want = eng.head_weights_to_flat(state, before.copy())
    np.random.seed(5)
    hist = m.fit(one, 1, trainable="heads", learning_rate=1e-3)
    assert len(hist.history["loss"]) == 1 and np.isfinite(hist.history["loss"][0])
    changed = m._flat.view(np.int32) != before.view(np.int32)
    assert changed.any() and np.array_equal(m._flat.view(np.int32), want.view(np.int32))
    inside = np.zeros(m._flat.size, bool)
    for o, k in m.engine.head_records():
        inside[o:o + k] = True
    assert not changed[~inside].any()
    eng.close()
    m.engine.close()
