"""Head fine-tuning on the device (csrc/head_train.hip: y4_loss_grad, y4_head_grad, y4_head_adam; Yolov4.fit(trainable='heads'))
against the reference-generated gradient fixtures, the float64 restatements of tests/lossgrad_oracle.py, and itself.

Budget of every comparison with a float64 value: 4 x d_ref with a floor of 1e-6, relative to the largest magnitude of the tensor
compared, where d_ref is how far the same quantity computed in float32 by the reference (the gradient: stored in the fixture) or
by NumPy / torch on the CPU (weight gradient, Adam, the training simulation) lies from float64.  Every measured distance is
written to profiles/fit/parity_measured.json beside its budget."""
import json
import os

import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
import lossgrad_oracle as GO
from helpers import CLASS_DIR, ROOT
from test_loss_cpu import _write_dataset
from test_lossgrad_cpu import CASE_NAMES, FLOOR, load_grad_fixture

pytestmark = pytest.mark.gpu
HEAD_IN = (92, 100, 108)


def _note(key, value):
    path = os.path.join(ROOT, "profiles", "fit", "parity_measured.json")
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


# ---- 3. the dense gradient
@pytest.mark.parametrize("name", CASE_NAMES)
def test_loss_grad_of_fixture_heads_vs_reference(name):
    import torch
    from yolo4hip.data import records_from_dense
    case, labels, xywh, fx = load_grad_fixture(name)
    eng, _ = _engine(case["hw"], case["ncls"], case["n"])
    n = eng.set_heads(case["heads"])
    triple = eng.upload_records(records_from_dense(labels, case["ncls"]), xywh)
    got = eng.loss_grad_device(n, records=triple, iou_loss_thresh=LC.IOU_LOSS_THRESH)
    for s in range(3):
        g = got[s].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == case["heads"][s].shape
        _within(f"loss_grad_{name}_scale{s}", g.reshape(fx["g64"][s].shape), fx["g64"][s], fx["d_ref"][s])
    # labels assigned on the device give the same bits
    got_b = eng.loss_grad_device(n, boxes_dev=torch.from_numpy(case["boxes"]).to(eng.device), iou_loss_thresh=LC.IOU_LOSS_THRESH)
    for a, b in zip(_bits(got), _bits(got_b)):
        assert np.array_equal(a, b)
    eng.close()


def test_loss_grad_is_independent_of_batch_and_position():
    import torch
    case, labels, xywh, fx = load_grad_fixture("160_coco_g")
    eng, _ = _engine(case["hw"], case["ncls"], 4)
    boxes = torch.from_numpy(case["boxes"]).to(eng.device)
    ones = np.ones(4, np.float32)

    def run(order):
        eng.set_heads([h[order] for h in case["heads"]])
        return _bits(eng.loss_grad_device(len(order), boxes_dev=boxes[order].contiguous(), img_weight=ones[:len(order)]))
    full = run([0, 1, 2, 3])
    for a, b in zip(full, run([0, 1, 2, 3])):
        assert np.array_equal(a, b)
    for a, b in zip(full, run([3, 2, 1, 0])):
        assert np.array_equal(a[[3, 2, 1, 0]], b)
    for i in range(4):
        for a, b in zip(full, run([i])):
            assert np.array_equal(a[i:i + 1], b)
    for a, b in zip(full, run([1, 1, 3])):
        assert np.array_equal(a[[1, 1, 3]], b)
    eng.close()


# ---- 4. the head weight gradient after a real forward
def _unpack(eng, dw):
    """the flat gradient -> [(db [cout], dW [cout, cin])] for convs 93 / 101 / 109"""
    lt = eng.layer_table()
    out, pos = [], 0
    for i in eng.HEAD_CONVS:
        cout, cin = lt[i]["cout"], lt[i]["cin"]
        out.append((dw[pos:pos + cout], dw[pos + cout:pos + cout * (1 + cin)].reshape(cout, cin)))
        pos += cout * (1 + cin)
    assert pos == dw.size
    return out


@pytest.mark.parametrize("hw,dtype,seed", [((160, 160), "f32", 9), ((160, 160), "bf16", 9), ((160, 160), "f16", 9),
                                           ((96, 160), "f32", 14), ((96, 160), "bf16", 14), ((96, 160), "f16", 14)])
def test_head_grad_after_a_forward(hw, dtype, seed):
    import torch
    from yolo4hip.data import preprocess_true_boxes
    ncls, n = 3, 4
    eng, _ = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=True)
    ref, _ = _engine(hw, ncls, n, dtype)                                     # non-aliased, unfused: the tap for X
    if dtype != "f32":
        assert eng.set_chain_fusion(True) > 0
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)).to(eng.device)
    boxes = LC.make_boxes(hw, ncls, n, seed=seed)
    boxes_dev = torch.from_numpy(boxes).to(eng.device)
    eng.forward_device(imgs)
    ref.forward_device(imgs)
    heads = [h.cpu().numpy() for h in eng.heads_device(n)]
    for a, b in zip(heads, ref.heads_device(n)):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    X = [ref.conv_output(c, n) for c in HEAD_IN]
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    w = np.array([0.4, 0.1, 0.3, 0.2], np.float32)
    g64 = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw, img_weight=w)
    dw = eng.head_grad_device(n, boxes_dev=boxes_dev, img_weight=w)
    got = _unpack(eng, dw.cpu().numpy())
    for s in range(3):
        db64, dW64 = GO.head_wgrad(g64[s], X[s])
        db32, dW32 = GO.head_wgrad(g64[s].astype(np.float32), X[s], np.float32)
        tag = f"head_grad_{hw[0]}x{hw[1]}_{dtype}_scale{s}"
        _within(tag + "_dW", got[s][1], dW64, GO.rel_to_max(dW32, dW64))
        _within(tag + "_db", got[s][0], db64, GO.rel_to_max(db32, db64))
    # bit-reproducible, and two accumulated chunks against the one call
    again = eng.head_grad_device(n, boxes_dev=boxes_dev, img_weight=w)
    assert np.array_equal(dw.cpu().numpy().view(np.int32), again.cpu().numpy().view(np.int32))

    def chunked():
        acc = torch.empty_like(dw)
        w_dev = torch.from_numpy(w).to(eng.device)
        for i0 in (0, 2):
            eng.forward_device(imgs[i0:i0 + 2])
            eng.head_grad_device(2, boxes_dev=boxes_dev[i0:i0 + 2], img_weight=w_dev[i0:i0 + 2], dw=acc, accumulate=i0 > 0)
        return acc.cpu().numpy()
    two = chunked()
    assert np.array_equal(two.view(np.int32), chunked().view(np.int32))
    for s, (db2, dW2) in enumerate(_unpack(eng, two)):
        db64, dW64 = GO.head_wgrad(g64[s], X[s])
        db32, dW32 = GO.head_wgrad(g64[s].astype(np.float32), X[s], np.float32)
        _within(f"head_grad_{hw[0]}x{hw[1]}_{dtype}_scale{s}_two_chunks_dW", dW2, dW64, GO.rel_to_max(dW32, dW64))
        _within(f"head_grad_{hw[0]}x{hw[1]}_{dtype}_scale{s}_two_chunks_db", db2, db64, GO.rel_to_max(db32, db64))
    eng.close()
    ref.close()


def test_head_grad_needs_retained_inputs_and_retention_changes_nothing():
    import torch
    from yolo4hip import ext
    hw, ncls, n = (160, 160), 3, 2
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to("cuda:0")
    boxes = torch.from_numpy(LC.make_boxes(hw, ncls, 4, seed=9)[2:]).to("cuda:0")
    plain, _ = _engine(hw, ncls, n, "bf16", alias_workspace=True)
    keep, _ = _engine(hw, ncls, n, "bf16", alias_workspace=True, retain_head_inputs=True)
    for e in (plain, keep):
        assert e.set_chain_fusion(True) > 0
        e.forward_device(imgs)
    assert keep.act_bytes >= plain.act_bytes
    for a, b in zip(_bits(plain.heads_device(n)), _bits(keep.heads_device(n))):
        assert np.array_equal(a, b)
    with pytest.raises(ext.Y4Error) as err:
        plain.head_grad_device(n, boxes_dev=boxes)
    assert err.value.code == -1 and "retain" in str(err.value)
    keep.head_grad_device(n, boxes_dev=boxes)
    plain.close()
    keep.close()


# ---- 5. Adam and the re-pack
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_head_adam_steps_and_repack(dtype):
    import torch
    hw, ncls, n = (160, 160), 3, 2
    eng, flat = _engine(hw, ncls, n, dtype)
    state = eng.head_state(flat)
    count = eng.head_floats()
    rng = np.random.default_rng(8)
    grads = [(rng.normal(size=count) * 10.0 ** rng.integers(-3, 1, size=count)).astype(np.float32) for _ in range(5)]
    w0 = state["w"].cpu().numpy()
    w64, m64, v64 = w0.astype(np.float64), np.zeros(count), np.zeros(count)
    w32, m32, v32 = w0.copy(), np.zeros(count, np.float32), np.zeros(count, np.float32)
    p = torch.tensor(w0.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-7)
    for t, g in enumerate(grads, 1):
        eng.head_adam_step(state, torch.from_numpy(g).to(eng.device), lr=1e-3)
        w64, m64, v64 = GO.adam_step(w64, m64, v64, g, t, lr=1e-3)
        w32, m32, v32 = GO.adam_step(w32, m32, v32, g, t, lr=1e-3, dtype=np.float32)
        opt.param_groups[0]["eps"] = 1e-7 / np.sqrt(1.0 - 0.999 ** t)
        p.grad = torch.tensor(g.astype(np.float64))
        opt.step()
    assert state["t"] == 5
    got = state["w"].cpu().numpy()
    # the step is what is compared (w itself hides it behind w0): w - w0 against the float64 rule
    _within(f"adam_{dtype}_update", got.astype(np.float64) - w0, w64 - w0, GO.rel_to_max(w32.astype(np.float64) - w0, w64 - w0))
    _within(f"adam_{dtype}_m", state["m"].cpu().numpy(), m64, GO.rel_to_max(m32, m64))
    _within(f"adam_{dtype}_v", state["v"].cpu().numpy(), v64, GO.rel_to_max(v32, v64))
    # float32 weights of magnitude <= 4 carry 2.4e-7 of rounding: 1e-6 absolute of torch's own Adam
    assert np.abs(got - p.detach().numpy()).max() <= 1e-6
    # the re-packed handle against a fresh engine that loads the updated stream
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to(eng.device)
    new_flat = eng.head_weights_to_flat(state, flat.copy())
    changed = np.flatnonzero(new_flat != flat)
    spans = eng.head_records()
    assert changed.size and all(any(o <= i < o + k for o, k in spans) for i in changed[[0, changed.size // 2, -1]])
    fresh, _ = _engine(hw, ncls, n, dtype)
    fresh.load_weight_blob(new_flat)
    eng.forward_device(imgs)
    fresh.forward_device(imgs)
    for a, b in zip(_bits(eng.heads_device(n)), _bits(fresh.heads_device(n))):
        assert np.array_equal(a, b)
    assert np.array_equal(eng.wts.cpu().numpy(), fresh.wts.cpu().numpy())
    eng.close()
    fresh.close()


# ---- 6. fit end to end
def _facade(hw, dtype, max_batch=4):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = make_config(hw[0], batch_size=3)
    return Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), cfg, dtype=dtype, max_batch=max_batch, synth_seed=3, tune=False)


def _fit_once(tmp_path, dtype, epochs=4):
    from yolo4hip.data import DataGenerator
    m = _facade((160, 160), dtype, max_batch=2)                             # batches of 3 through max_batch 2: two chunks
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 8, 1, 4, 2])
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False, config=m.config)
    before_flat = m._flat.copy()
    np.random.seed(11)
    before = m.evaluate(gen)["loss"]
    seen = []

    class Callback:
        def on_epoch_end(self, epoch, logs):
            seen.append((epoch, dict(logs)))
    np.random.seed(11)
    hist = m.fit(gen, epochs, val_data_gen=gen, callbacks=[Callback()], trainable="heads", learning_rate=1e-3)
    np.random.seed(11)
    after = m.evaluate(gen)["loss"]
    return m, gen, before_flat, before, after, hist, seen


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fit_heads_end_to_end(tmp_path, dtype):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    m, gen, before_flat, before, after, hist, seen = _fit_once(tmp_path / "a", dtype)
    m2, _, _, _, after2, hist2, _ = _fit_once(tmp_path / "b", dtype)
    assert set(hist.history) == {"loss", "val_loss"} and len(hist.history["loss"]) == 4 and len(seen) == 4
    assert [e for e, _ in seen] == [0, 1, 2, 3] and seen[-1][1]["loss"] == hist.history["loss"][-1]
    assert np.isfinite(hist.history["loss"]).all() and np.isfinite(hist.history["val_loss"]).all()
    # two runs from the same seed: the same bits
    assert np.array_equal(m._flat.view(np.int32), m2._flat.view(np.int32))
    assert hist.history == hist2.history and after == after2
    # only the three head records moved
    changed = np.flatnonzero(m._flat != before_flat)
    inside = np.zeros(m._flat.size, bool)
    for o, k in m.engine.head_records():
        inside[o:o + k] = True
    assert changed.size > 0 and inside[changed].all()
    print(f"fit {dtype}: evaluate(train) before {before} after {after}; history {hist.history}")
    _note(f"fit_{dtype}", {"evaluate_before": before, "evaluate_after": after, "history": hist.history})
    assert after < before
    # every front sees the trained weights; a checkpoint reproduces predict bit for bit, in both formats
    imgs = np.random.default_rng(6).uniform(0, 1, size=(2, 160, 160, 3)).astype(np.float32)
    want = m.inference_model.predict(imgs)
    heads = m.yolo_model.predict(imgs)
    for name in ("trained.ckpt", "trained.weights"):
        path = str(tmp_path / name)
        m.save_model(path)
        fresh = _facade((160, 160), dtype, max_batch=2)
        fresh.load_model(path)
        assert np.array_equal(fresh._flat.view(np.int32), m._flat.view(np.int32))
        for a, b in zip(heads, fresh.yolo_model.predict(imgs)):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
        got = fresh.inference_model.predict(imgs)
        ref = m.engine.predict(imgs, iou_threshold=0.413, score_threshold=0.3)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)
        fresh.engine.close()
    assert len(want) == 4
    # a later fit starts from the trained weights; the reference's fit (every layer) still raises
    again = m.fit(gen, 1, trainable="heads", learning_rate=1e-3)
    assert set(again.history) == {"loss"} and again.history["loss"][0] < hist.history["loss"][0]
    with pytest.raises(NotImplementedError, match="trainable='heads'"):
        m.fit(None, 1)
    bad = gen.boxes(0)[1].copy()
    bad[0, 0] = [400, 10, 460, 50, 0]

    class BadGen:
        max_boxes = gen.max_boxes

        def __len__(self):
            return 1

        def boxes(self, i):
            return gen.boxes(0)[0], bad
    keep = m._flat.copy()
    with pytest.raises(ValueError, match="outside"):
        m.fit(BadGen(), 1, trainable="heads")
    assert np.array_equal(keep, m._flat)
    m.engine.close()
    m2.engine.close()


# ---- 7. ten training steps against a float64 simulation (the backbone is frozen: heads = X W^T + b)
def test_training_steps_vs_float64_simulation():
    import torch
    from yolo4hip.data import preprocess_true_boxes
    from yolo4hip.engine import combine_loss
    hw, ncls, n, steps, lr = (160, 160), 3, 4, 10, 1e-3
    eng, flat = _engine(hw, ncls, n, "f32", retain_head_inputs=True)
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to(eng.device)
    boxes = LC.make_boxes(hw, ncls, n, seed=9)
    boxes_dev = torch.from_numpy(boxes).to(eng.device)
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    state = eng.head_state(flat)
    device_loss = []
    for _ in range(steps):
        eng.forward_device(imgs)
        triple = eng.assign_device(boxes_dev)
        device_loss.append(float(combine_loss(eng.loss_device(n, records=triple).cpu().numpy())[0].mean()))
        eng.head_adam_step(state, eng.head_grad_device(n, records=triple), lr=lr)
    X = [eng.conv_output(c, n) for c in HEAD_IN]                             # constant: the backbone and neck are frozen
    lt = eng.layer_table()

    def simulate(dtype):
        ws = []
        for i in eng.HEAD_CONVS:
            o, cout, cin = lt[i]["weight_offset"], lt[i]["cout"], lt[i]["cin"]
            ws.append([flat[o:o + cout].astype(dtype), flat[o + cout:o + cout * (1 + cin)].reshape(cout, cin).astype(dtype)])
        moments = [[np.zeros_like(b), np.zeros_like(b), np.zeros_like(W), np.zeros_like(W)] for b, W in ws]
        out = []
        for t in range(1, steps + 1):
            heads = [(X[s].astype(dtype) @ ws[s][1].T + ws[s][0]).astype(dtype) for s in range(3)]
            out.append(LO.total(LO.loss_terms(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw)))
            g = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw)
            for s in range(3):
                db, dW = GO.head_wgrad(g[s].astype(dtype), X[s], dtype)
                mo = moments[s]
                ws[s][0], mo[0], mo[1] = GO.adam_step(ws[s][0], mo[0], mo[1], db, t, lr=lr, dtype=dtype)
                ws[s][1], mo[2], mo[3] = GO.adam_step(ws[s][1], mo[2], mo[3], dW, t, lr=lr, dtype=dtype)
        return np.array(out)
    sim64, sim32 = simulate(np.float64), simulate(np.float32)
    d_ref = GO.rel_to_max(sim32, sim64)
    print("device loss:", device_loss, "float64 simulation:", sim64.tolist())
    assert sim64[-1] < sim64[0]
    _within("training_10_steps_f32", np.array(device_loss), sim64, d_ref)
    eng.close()
