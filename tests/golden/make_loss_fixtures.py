#!/usr/bin/env python3
"""Loss fixtures written by the REFERENCE'S OWN PYTHON (runs only where /root/reference exists; nothing of it is copied).

  python tests/golden/make_loss_fixtures.py          writes tests/golden/loss_<case>.npz for every case of tests/loss_cases.py
                                                     (CASES, and LABEL_CASES: other max_boxes and class counts)
  python tests/golden/make_loss_fixtures.py --seeds  prints, per case, the first seed that passes check_case
  (case names after the options restrict either to those cases)

The reference's `loss.py` and `utils.py` are imported UNMODIFIED.  `tensorflow` is a module of eager torch-CPU float32
functions made here (the ~20 names loss.py touches; tests/golden/tf_standin.py is not involved), `cv2` an empty placeholder.
What runs is the reference's `utils.preprocess_true_boxes`, `loss.decode` + `loss.loss_layer` per scale (for the whole batch
and for every image alone, which gives the per-image sums) and `loss.yolo_loss`.

Inputs come from seeds through tests/loss_cases.py, so only results are stored: the dense labels in sparse form (flat indices
and values of the non-zeros), y_true_boxes_xywh, the per-image and the batch components, the total, `d_ref` -- per (scale,
term) the largest relative distance over the images between the reference's float32 result and the float64 restatement of
tests/loss_oracle.py, from which the GPU test takes its budget -- and the size of the ignore region per scale.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))


def _t(v):
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


def _same(a, b):
    a = _t(a)
    b = _t(b)
    return a, (b.to(a.dtype) if b.dtype != a.dtype else b)


def install_tf():
    tf = types.ModuleType("tensorflow")
    keras = types.ModuleType("tensorflow.keras")
    backend = types.ModuleType("tensorflow.keras.backend")
    kutils = types.ModuleType("tensorflow.keras.utils")
    kutils.Sequence = object
    tf.float32, tf.int32, tf.newaxis = torch.float32, torch.int32, None
    tf.concat = lambda xs, axis: torch.cat([_t(x) for x in xs], dim=axis)
    tf.maximum = lambda a, b: torch.maximum(*_same(a, b))
    tf.minimum = lambda a, b: torch.minimum(*_same(a, b))
    tf.shape = lambda x: torch.tensor(list(x.shape), dtype=torch.int32)
    tf.reshape = lambda x, shape: _t(x).reshape([int(v) for v in shape])
    tf.range = lambda n, dtype=None: torch.arange(int(n), dtype=dtype)
    tf.tile = lambda x, reps: x.repeat([int(r) for r in reps])
    tf.cast = lambda x, dtype: _t(x).to(dtype)
    tf.sigmoid, tf.exp, tf.atan, tf.pow = torch.sigmoid, torch.exp, torch.atan, torch.pow
    tf.expand_dims = lambda x, axis: x.unsqueeze(axis)
    tf.reduce_max = lambda x, axis: x.max(dim=axis).values
    tf.reduce_sum = lambda x, axis: x.sum(dim=axis)
    tf.reduce_mean = lambda x: x.mean()
    tf.math = types.SimpleNamespace(divide_no_nan=lambda a, b: torch.where(b == 0, torch.zeros_like(a), a / b))
    tf.nn = types.SimpleNamespace(sigmoid_cross_entropy_with_logits=lambda labels, logits: (
        torch.clamp(logits, min=0) - logits * labels + torch.log1p(torch.exp(-logits.abs()))))
    backend.epsilon = lambda: 1e-7
    backend.pow = torch.pow
    keras.backend, keras.utils, tf.keras = backend, kutils, keras
    for name, mod in (("tensorflow", tf), ("tensorflow.keras", keras), ("tensorflow.keras.backend", backend),
                      ("tensorflow.keras.utils", kutils), ("cv2", types.ModuleType("cv2"))):
        sys.modules[name] = mod
    import matplotlib
    matplotlib.use("Agg")


def import_reference():
    install_tf()
    mods = {}
    sys.path.insert(0, REF)
    try:
        for name in ("config", "utils", "loss"):
            mods[name] = __import__(name)
            assert os.path.dirname(os.path.abspath(mods[name].__file__)) == REF, mods[name].__file__
    finally:
        sys.path.remove(REF)
    return mods


def run_case(name, mods, seed=None):
    """-> (arrays to store, problems: a list of failed conditions)."""
    import loss_cases as LC
    if name in LC.LABEL_CASES:
        return run_label_case(name, mods, seed)
    if seed is not None:
        LC.CASES[name] = dict(LC.CASES[name], seed=seed)
    case = LC.make_case(name)
    return run_reference(case, mods)


def run_label_case(name, mods, seed=None):
    """A case of loss_cases.LABEL_CASES (max_boxes and class counts beside 100 and {3, 80}): its conditions are check_case's."""
    import loss_cases as LC
    case = LC.make_label_case(name, seed)
    try:
        LC.check_case(name, case)
    except AssertionError as err:
        return None, [str(err) or repr(err)]
    out, problems = run_reference(case, mods, structure=False)
    # the host assignment the heads were made from is the reference's
    from yolo4hip.data import dense_from_records
    for s, y in enumerate(dense_from_records(case["records"], case["hw"], case["ncls"])):
        ref = np.zeros(y.size, dtype=np.float32)
        ref[out[f"label{s}_idx"]] = out[f"label{s}_val"]
        if not np.array_equal(ref, y.reshape(-1)):
            problems.append(f"scale {s}: the host records are not the reference's labels")
    return out, problems


def run_reference(case, mods, structure=True):
    """The reference on a case's inputs -> (arrays to store, problems); structure: the conditions of the cases of 100 rows."""
    import loss_cases as LC
    import loss_oracle as LO
    hw, ncls, n = case["hw"], case["ncls"], case["n"]
    boxes, heads = case["boxes"], case["heads"]
    y_true, xywh = mods["utils"].preprocess_true_boxes(boxes.copy(), hw, LC.ANCHORS, ncls)
    anchors_t = torch.tensor(LC.ANCHORS.reshape(3, 3, 2).astype(np.float32))
    heads_t = [torch.from_numpy(h) for h in heads]
    labels_t = [torch.from_numpy(y) for y in y_true]
    xywh_t = torch.from_numpy(xywh)
    L = mods["loss"]

    def layer(s, sl):
        conv = heads_t[s][sl]
        pred = L.decode(conv, anchors_t[s], LC.STRIDES[s], ncls)
        return [float(v) for v in L.loss_layer(conv, pred, labels_t[s][sl], xywh_t[sl], LC.STRIDES[s], ncls,
                                               LC.IOU_LOSS_THRESH)]
    ref_batch = np.array([layer(s, slice(None)) for s in range(3)], dtype=np.float32)                    # [3 scales, 3 terms]
    ref_img = np.array([[layer(s, slice(i, i + 1)) for s in range(3)] for i in range(n)], dtype=np.float32)
    ref_total = np.float32(float(L.yolo_loss([*heads_t, *labels_t, xywh_t], ncls, LC.IOU_LOSS_THRESH, anchors_t)))

    oracle = LO.loss_terms(heads, y_true, xywh, LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, hw)
    d_ref = LO.rel_dist(ref_img, oracle).max(axis=0)                                                       # [3, 3]
    problems, ignore = [], []
    anchors3 = LC.ANCHORS.reshape(3, 3, 2)
    for s in range(3):
        _, max_iou, respond = LO.scale_terms(heads[s], y_true[s], xywh, anchors3[s], LC.STRIDES[s], ncls,
                                             LC.IOU_LOSS_THRESH, float(hw[0] * hw[1]))
        if respond.sum() == 0:
            problems.append(f"scale {s} has no responsible cell")
        ignore.append(int(((respond == 0) & (max_iou >= LC.IOU_LOSS_THRESH)).sum()))
        if ignore[-1] == 0:
            problems.append(f"scale {s}: empty ignore region")
        near = int((np.abs(max_iou - LC.IOU_LOSS_THRESH) < 1e-4).sum())
        if near:
            problems.append(f"scale {s}: {near} lanes within 1e-4 of the ignore threshold")
    valid = boxes[..., 2] - boxes[..., 0] > 0
    if not (~valid).all(axis=1).any():
        problems.append("no image without boxes")
    if not valid.all(axis=1).any():
        problems.append("no image with exactly max_boxes boxes")
    if structure and not any(np.any(~v[:-1] & (np.cumsum(v[::-1])[::-1][1:] > 0)) and v[0] for v in valid):
        problems.append("no degenerate row between valid rows")
    if structure and not any(((y[..., 4] == 1) & (y[..., 5:].sum(axis=-1) > 1)).any() for y in y_true):
        problems.append("no collision of two classes on one cell and anchor")
    out = dict(sha=np.array(case["sha"]), true_xywh=xywh, ref_img=ref_img, ref_batch=ref_batch, ref_total=ref_total,
               d_ref=d_ref, ignore_count=np.array(ignore, dtype=np.int64))
    for s, y in enumerate(y_true):
        nz = np.flatnonzero(y)
        out[f"label{s}_idx"], out[f"label{s}_val"] = nz.astype(np.int64), y.reshape(-1)[nz]
    return out, problems


def main():
    mods = import_reference()
    import loss_cases as LC
    names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(LC.CASES) + list(LC.LABEL_CASES)
    if "--seeds" in sys.argv:
        for name in names:
            for seed in range(1, 400):
                _, problems = run_case(name, mods, seed)
                if not problems:
                    print(name, "seed", seed)
                    break
        return
    for name in names:
        out, problems = run_case(name, mods)
        assert not problems, (name, problems)
        path = os.path.join(HERE, f"loss_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes, total {out['ref_total']}, ignore {out['ignore_count'].tolist()}, "
              f"max d_ref {out['d_ref'].max():.2e}")


if __name__ == "__main__":
    main()
