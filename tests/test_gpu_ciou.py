"""The CIoU box term on the device (y4_set_box_loss(h, 1): csrc/loss.hip, csrc/grad_common.h box_grad_ciou; Engine(box_loss='ciou'),
Yolov4(box_loss='ciou')) against the reference-generated fixtures (tests/golden/make_ciou_fixtures.py), the float64 restatement of
tests/ciou_oracle.py, and itself; and the default (GIoU) against a handle whose setter was never called.

Budget of every comparison with a float64 value: the project's rule, max(4 x d_ref, 1e-6), where d_ref is how far the same
quantity in float32 lies from float64 -- the reference's own float32 run where a fixture holds one (per-image sums: elementwise,
per (scale, term), as tests/test_gpu_loss.py; gradients: relative to the tensor's largest magnitude, as tests/test_gpu_fit.py),
else the float32 CPU evaluation of the oracle with the roundings tests/test_gpu_fit*.py use for each dtype.  The four box columns
of the gradient are also held on their own (the confidence column is twenty times larger and would hide them), d_ref then being
the fixture's float32 box columns against its float64 ones.  Every measured distance is written beside its budget to
profiles/fit/ciou_measured.json."""
import json
import os

import numpy as np
import pytest

import blockgrad_oracle as BO
import ciou_oracle as CO
import loss_cases as LC
import loss_oracle as LO
import lossgrad_oracle as GO
from helpers import CLASS_DIR, ROOT
from test_ciou_cpu import CASE_NAMES, load_ciou_fixture
from test_loss_cpu import _write_dataset

pytestmark = pytest.mark.gpu
FLOOR = 1e-6
BLOCK_IN, HEAD_IN = (91, 99, 107), (92, 100, 108)
ORDERS = ([0, 1, 2, 3], [3, 2, 1, 0], [0], [1], [2], [3], [1, 1, 3])       # of test_loss_grad_is_independent_of_batch_and_position


def _note(key, value):
    path = os.path.join(ROOT, "profiles", "fit", "ciou_measured.json")
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


def _within(key, got, want64, d_ref):
    dist, budget = GO.rel_to_max(got, want64), max(4.0 * float(d_ref), FLOOR)
    _note(key, {"rel_to_max": dist, "budget": budget, "d_ref": float(d_ref)})
    print(key, "distance:", dist, "budget:", budget)
    assert np.isfinite(np.asarray(got)).all(), key
    assert dist <= budget, (key, dist, budget)


def _engine(hw, ncls, n, dtype="f32", seed=2, **kw):
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    from yolo4hip import weights as W
    cfg = make_config(hw if hw[0] != hw[1] else hw[0])
    eng = Engine(ncls, cfg, max_batch=n, dtype=dtype, device="cuda:0", **kw)
    flat = W.flatten(W.synth_weights(build_plan(hw, ncls), seed=seed))
    eng.load_weight_blob(flat)
    return eng, flat


def _bits(ts):
    return [t.cpu().numpy().view(np.int32) for t in ts]


def _kind(eng):
    return eng.lib.y4_get_box_loss(eng.handle)


# ---- 1, 2. y4_loss and y4_loss_grad with kind 1 on the fixture heads
@pytest.mark.parametrize("name", CASE_NAMES)
def test_ciou_loss_and_gradient_of_fixture_heads_vs_reference(name):
    import torch
    from yolo4hip.data import records_from_dense
    from yolo4hip.engine import combine_loss
    case, labels, xywh, fx = load_ciou_fixture(name)
    eng, _ = _engine(case["hw"], case["ncls"], case["n"], box_loss="ciou")
    assert _kind(eng) == 1 and eng.box_loss == "ciou"
    n = eng.set_heads(case["heads"])
    triple = eng.upload_records(records_from_dense(labels, case["ncls"]), xywh)
    boxes_dev = torch.from_numpy(case["boxes"]).to(eng.device)
    # the nine sums of every image
    got = eng.loss_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert got.shape == (n, 3, 3) and got.dtype == np.float32 and np.isfinite(got).all()
    dist = LO.rel_dist(got, fx["terms64"])
    budget = np.maximum(4.0 * fx["terms_d_ref"], FLOOR)
    _note(f"loss_{name}", {"max_rel_dist": dist.max(axis=0).tolist(), "budget": budget.tolist()})
    print(name, "max rel dist per (scale, term):", dist.max(axis=0).tolist(), "budget:", budget.tolist())
    assert np.all(dist <= budget), (dist.max(axis=0), budget)
    total = combine_loss(got)[0].mean()
    assert abs(total - float(fx["total64"])) <= 5e-6 * float(fx["total64"])
    got_b = eng.loss_device(n, boxes_dev=boxes_dev, iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert np.array_equal(got.view(np.int32), got_b.view(np.int32))           # labels assigned on the device: the same bits
    # the dense gradient
    grad = eng.loss_grad_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH)
    for s in range(3):
        g = grad[s].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == case["heads"][s].shape
        g = g.reshape(fx["g64"][s].shape)
        _within(f"loss_grad_{name}_scale{s}", g, fx["g64"][s], fx["d_ref"][s])
        box64 = fx["g64"][s][..., 0:4]
        _within(f"loss_grad_{name}_scale{s}_box_columns", g[..., 0:4], box64, GO.rel_to_max(fx["g32"][s][..., 0:4], box64))
    grad_b = eng.loss_grad_device(n, boxes_dev=boxes_dev, iou_loss_thresh=LC.IOU_LOSS_THRESH)
    for a, b in zip(_bits(grad), _bits(grad_b)):
        assert np.array_equal(a, b)
    # the switch is live on a bound handle: back to GIoU gives other box sums and the same confidence and class sums
    eng.set_box_loss("giou")
    assert _kind(eng) == 0
    giou = eng.loss_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH).cpu().numpy()
    assert np.array_equal(giou[:, :, 1:].view(np.int32), got[:, :, 1:].view(np.int32))
    assert np.all(giou[:, :, 0][got[:, :, 0] != 0] != got[:, :, 0][got[:, :, 0] != 0])
    eng.close()


def test_ciou_loss_and_gradient_are_independent_of_batch_and_position():
    import torch
    case, _, _, _ = load_ciou_fixture("160_coco_g")
    eng, _ = _engine(case["hw"], case["ncls"], 4, box_loss="ciou")
    boxes = torch.from_numpy(case["boxes"]).to(eng.device)
    ones = np.ones(4, np.float32)

    def run(order):
        eng.set_heads([h[order] for h in case["heads"]])
        b = boxes[order].contiguous()
        return [eng.loss_device(len(order), boxes_dev=b).cpu().numpy().view(np.int32)] + \
            _bits(eng.loss_grad_device(len(order), boxes_dev=b, img_weight=ones[:len(order)]))
    full = run(ORDERS[0])
    for order in ORDERS:
        for a, b in zip(full, run(order)):
            assert np.array_equal(a[order], b), order
    eng.close()


# ---- 3. y4_head_grad after a real forward
def _unpack(eng, dw):
    lt = eng.layer_table()
    out, pos = [], 0
    for i in eng.HEAD_CONVS:
        cout, cin = lt[i]["cout"], lt[i]["cin"]
        out.append((dw[pos:pos + cout], dw[pos + cout:pos + cout * (1 + cin)].reshape(cout, cin)))
        pos += cout * (1 + cin)
    assert pos == dw.size
    return out


def _unpack_k(eng, dk):
    lt = eng.layer_table()
    out, pos = [], 0
    for i in eng.BLOCK_CONVS:
        cout, cin = lt[i]["cout"], lt[i]["cin"]
        out.append(dk[pos:pos + cout * cin * 9].reshape(cout, cin, 3, 3))
        pos += cout * cin * 9
    assert pos == dk.size
    return out


class _Grads(list):
    """the oracle's three float64 gradients, with `box32`: the same with the box columns evaluated in float32"""


def _after_a_forward(hw, dtype, seed, level, taps):
    """An engine with box_loss='ciou' after a forward of four images, the taps of a non-aliased unfused engine, and the oracle's
    CIoU gradient for the device's own heads."""
    import torch
    from yolo4hip.data import preprocess_true_boxes
    ncls, n = 3, 4
    eng, flat = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=level, box_loss="ciou")
    ref, _ = _engine(hw, ncls, n, dtype)
    if dtype != "f32":
        assert eng.set_chain_fusion(True) > 0
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)).to(eng.device)
    boxes = LC.make_boxes(hw, ncls, n, seed=seed)
    eng.forward_device(imgs)
    ref.forward_device(imgs)
    heads = [h.cpu().numpy() for h in eng.heads_device(n)]
    for a, b in zip(heads, ref.heads_device(n)):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    tapped = [[ref.conv_output(c, n) for c in convs] for convs in taps]
    ref.close()
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    w = np.array([0.4, 0.1, 0.3, 0.2], np.float32)
    args = (heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw)
    d_min, c2_min = CO.lane_conditions(heads, labels, LC.ANCHORS, LC.STRIDES, ncls, hw)
    assert d_min >= 0.01 and c2_min >= 1.0, (d_min, c2_min)                   # away from where the reference itself divides by 0
    g64 = _Grads(CO.loss_grad(*args, img_weight=w))
    giou64 = GO.loss_grad(*args, img_weight=w)
    assert all(GO.rel_to_max(a, b) > 1e-3 for a, b in zip(g64, giou64))   # another gradient than GIoU's
    g64.box32 = CO.loss_grad(*args, img_weight=w, dtype=np.float32)          # the box columns evaluated in float32
    return eng, flat, torch.from_numpy(boxes).to(eng.device), w, g64, tapped


@pytest.mark.parametrize("hw,dtype,seed", [((160, 160), "f32", 9), ((160, 160), "bf16", 9), ((160, 160), "f16", 9),
                                           ((96, 160), "f32", 14), ((96, 160), "bf16", 14), ((96, 160), "f16", 14)])
def test_ciou_head_grad_after_a_forward(hw, dtype, seed):
    eng, _, boxes_dev, w, g64, (X,) = _after_a_forward(hw, dtype, seed, 1, [HEAD_IN])
    dw = eng.head_grad_device(4, boxes_dev=boxes_dev, img_weight=w)
    got = _unpack(eng, dw.cpu().numpy())
    for s in range(3):
        db64, dW64 = GO.head_wgrad(g64[s], X[s])
        db32, dW32 = GO.head_wgrad(g64[s].astype(np.float32), X[s], np.float32)
        tag = f"head_grad_{hw[0]}x{hw[1]}_{dtype}_scale{s}"
        _within(tag + "_dW", got[s][1], dW64, GO.rel_to_max(dW32, dW64))
        _within(tag + "_db", got[s][0], db64, GO.rel_to_max(db32, db64))
        # the rows of the four box values of each anchor on their own (only responsible lanes feed them; the confidence rows are
        # far larger): d_ref from the oracle's box columns evaluated in float32, summed in float32
        nout = g64[s].shape[-1] // 3
        rows = np.array([a * nout + j for a in range(3) for j in range(4)])
        _, dWb = GO.head_wgrad(g64.box32[s].astype(np.float32), X[s], np.float32)
        _within(tag + "_dW_box_rows", got[s][1][rows], dW64[rows], GO.rel_to_max(dWb[rows], dW64[rows]))
    again = eng.head_grad_device(4, boxes_dev=boxes_dev, img_weight=w)
    assert np.array_equal(dw.cpu().numpy().view(np.int32), again.cpu().numpy().view(np.int32))
    eng.close()


# ---- 4. y4_block_grad (f32, bf16) and y4_block_grad_scaled (f16, S = 2^7)
def _round_f16(scale, keep_subnormals):
    def rnd(dz):
        with np.errstate(over="ignore"):
            y = (np.asarray(dz, np.float64) * scale).astype(np.float16)
        if not keep_subnormals:
            y = np.where(np.abs(y) < np.float16(2.0 ** -14), np.float16(0), y)
        return y.astype(np.float64) / scale
    return rnd


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_ciou_block_grad_after_a_forward(dtype):
    hw, S = (160, 160), 2.0 ** 7
    eng, flat, boxes_dev, w, g64, (U, A) = _after_a_forward(hw, dtype, 9, 2, [BLOCK_IN, HEAD_IN])
    lt = eng.layer_table()
    want, d_ref = [], []
    for s, (hc, bc) in enumerate(zip(eng.HEAD_CONVS, eng.BLOCK_CONVS)):
        o, cout, cin = lt[hc]["weight_offset"], lt[hc]["cout"], lt[hc]["cin"]
        wh = flat[o + cout:o + cout * (1 + cin)].reshape(cout, cin).astype(np.float64)
        if dtype == "bf16":
            wh = BO.round_bf16(wh)                                               # Wh as the handle packs it
        elif dtype == "f16":
            wh = wh.astype(np.float16).astype(np.float64)
        bo, bcout = lt[bc]["weight_offset"], lt[bc]["cout"]
        bn = flat[bo:bo + 4 * bcout].reshape(4, bcout)
        sc = BO.bn_scale(bn[1], bn[3])
        dk64 = BO.block_grad(g64[s], wh, A[s], U[s], sc)
        if dtype == "f32":
            others = [BO.block_grad(g64[s].astype(np.float32), wh, A[s], U[s], BO.bn_scale(bn[1], bn[3], np.float32), np.float32)]
        elif dtype == "bf16":
            others = [BO.block_grad(g64[s], wh, A[s], U[s], sc, round_dz=BO.round_bf16)]
        else:
            assert np.abs(BO.block_dz(g64[s], wh, A[s], sc)).max() * S < 65504.0     # S leaves fp16's range alone
            others = [BO.block_grad(g64[s], wh, A[s], U[s], sc, round_dz=_round_f16(S, keep)) for keep in (True, False)]
        want.append(dk64)
        d_ref.append(max(GO.rel_to_max(o, dk64) for o in others))

    def call():
        if dtype != "f16":
            return eng.block_grad_device(4, boxes_dev=boxes_dev, img_weight=w)
        dk, word = eng.block_grad_device(4, boxes_dev=boxes_dev, img_weight=w, loss_scale=S)
        assert int(word.cpu().numpy()[0]) == 0
        return dk
    dk = call()
    for s, got in enumerate(_unpack_k(eng, dk.cpu().numpy())):
        assert got.shape == want[s].shape and np.abs(want[s]).max() > 0
        _within(f"block_grad_160x160_{dtype}_scale{s}_dK", got, want[s], d_ref[s])
    assert np.array_equal(dk.cpu().numpy().view(np.int32), call().cpu().numpy().view(np.int32))      # two calls: the same bits
    eng.close()


# ---- 5. the facade
def _facade(dtype="f32", **kw):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    return Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(160, batch_size=3), dtype=dtype, max_batch=2,
                  synth_seed=3, tune=False, **kw)


def _dataset(tmp_path, m):
    from yolo4hip.data import DataGenerator
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 8, 1, 4, 2])
    return DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False, config=m.config)


def test_facade_evaluates_the_ciou_term(tmp_path):
    from yolo4hip.data import preprocess_true_boxes
    with pytest.raises(ValueError, match="box_loss"):
        _facade(box_loss="xiou")
    m, plain = _facade(box_loss="ciou"), _facade()
    assert m.box_loss == m.engine.box_loss == "ciou" and _kind(m.engine) == 1 and _kind(plain.engine) == 0
    gen = _dataset(tmp_path, m)
    np.random.seed(11)
    res = m.evaluate(gen)
    np.random.seed(11)
    res_giou = plain.evaluate(gen)
    assert res["conf"] == res_giou["conf"] and res["class"] == res_giou["class"] and res["box"] != res_giou["box"]
    assert res["loss"] == pytest.approx(res["box"] + res["conf"] + res["class"], rel=1e-12)
    np.random.seed(11)                                                       # (get_data shuffles each image's boxes)
    box64, box32, dense_total = [], [], []
    for i in range(len(gen)):
        X, boxes = gen.boxes(i)
        heads = m.engine.forward_heads(X)
        labels, xywh = preprocess_true_boxes(boxes, (160, 160), LC.ANCHORS, 3)
        args = (heads, labels, xywh, LC.ANCHORS, LC.STRIDES, 3, m.iou_loss_thresh, (160, 160))
        box64.append(CO.loss_terms(*args)[:, :, 0].sum(axis=1) * LO.WEIGHTS[0])
        box32.append(CO.loss_terms(*args, dtype=np.float32)[:, :, 0].sum(axis=1) * LO.WEIGHTS[0])
        dense_total.append((float(m.training_model.predict([X, *labels, xywh])), len(X),
                            LO.total(CO.loss_terms(*args))))
    want, f32 = float(np.concatenate(box64).mean()), float(np.concatenate(box32).mean())
    d_ref = abs(f32 - want) / want
    dist, budget = abs(res["box"] - want) / want, max(4.0 * d_ref, FLOOR)
    _note("facade_evaluate_box", {"rel_dist": dist, "budget": budget, "d_ref": d_ref, "box_ciou": res["box"], "box_giou": res_giou["box"]})
    print("evaluate()['box'] ciou:", res["box"], "oracle:", want, "distance:", dist, "budget:", budget, "giou:", res_giou["box"])
    assert dist <= budget
    # training_model.predict runs the same term: the batch's scalar against the oracle's total
    for got, _, total in dense_total:
        assert abs(got - total) <= 5e-6 * total
    m.engine.close()
    plain.engine.close()


@pytest.mark.parametrize("trainable,rate", [("heads", 1e-3), ("head_blocks", 1e-4)])
def test_facade_fit_with_ciou(tmp_path, trainable, rate):
    runs = []
    for d in "ab":
        (tmp_path / d).mkdir()
        m = _facade(box_loss="ciou")
        gen = _dataset(tmp_path / d, m)
        np.random.seed(11)
        hist = m.fit(gen, 2, val_data_gen=gen, trainable=trainable, learning_rate=rate)
        eng = m._fit_engine if trainable == "heads" else m._fit_engine_blocks
        assert eng.box_loss == "ciou" and _kind(eng) == 1                     # the training engine inherits the kind
        runs.append((hist.history, m._flat.copy()))
        m.engine.close()
    history = runs[0][0]
    print(f"fit {trainable} ciou:", history)
    _note(f"facade_fit_{trainable}", {"history": history})
    assert set(history) == {"loss", "val_loss"} and np.isfinite(history["loss"]).all() and np.isfinite(history["val_loss"]).all()
    assert history["loss"][1] < history["loss"][0]
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1].view(np.int32), runs[1][1].view(np.int32))


def test_facade_fit_with_ciou_f16_loss_scale(tmp_path):
    m = _facade("f16", box_loss="ciou")
    gen = _dataset(tmp_path, m)
    np.random.seed(11)
    hist = m.fit(gen, 2, trainable="head_blocks", learning_rate=1e-4, loss_scale=2.0 ** 7)
    print("fit head_blocks f16 ciou:", hist.history)
    _note("facade_fit_head_blocks_f16", {"history": hist.history})
    assert m._fit_engine_blocks.box_loss == "ciou" and np.isfinite(hist.history["loss"]).all()
    assert hist.history["loss"][1] < hist.history["loss"][0]
    m.engine.close()


# ---- 6. the default is what it was
def test_kind_0_set_explicitly_gives_the_bits_of_an_untouched_handle():
    import torch
    hw, ncls, n = (160, 160), 3, 2
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to("cuda:0")
    boxes = torch.from_numpy(LC.make_boxes(hw, ncls, 4, seed=9)[2:]).to("cuda:0")
    for dtype in ("f32", "bf16"):
        fresh, _ = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=2)      # its setter is never called
        back, _ = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=2)
        back.set_box_loss("ciou")
        back.set_box_loss("giou")
        assert _kind(fresh) == 0 and _kind(back) == 0
        outs = []
        for e in (fresh, back):
            e.forward_device(imgs)
            outs.append([e.loss_device(n, boxes_dev=boxes), *e.loss_grad_device(n, boxes_dev=boxes),
                         e.head_grad_device(n, boxes_dev=boxes).clone(), e.block_grad_device(n, boxes_dev=boxes).clone()])
        for a, b in zip(_bits(outs[0]), _bits(outs[1])):
            assert np.array_equal(a, b)
        # ... and the other kind moves every one of them
        back.set_box_loss("ciou")
        sib = back.sibling()                                                 # a sibling inherits the kind
        assert sib.box_loss == "ciou" and _kind(sib) == 1 and _kind(fresh.sibling()) == 0
        sib.close()
        other = [back.loss_device(n, boxes_dev=boxes), *back.loss_grad_device(n, boxes_dev=boxes),
                 back.head_grad_device(n, boxes_dev=boxes).clone(), back.block_grad_device(n, boxes_dev=boxes).clone()]
        for a, b in zip(_bits(outs[0]), _bits(other)):
            assert not np.array_equal(a, b)
        fresh.close()
        back.close()
