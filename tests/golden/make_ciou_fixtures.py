#!/usr/bin/env python3
"""CIoU fixtures: the REFERENCE'S OWN `loss.py` with its box term switched to `bbox_ciou` (runs only where the reference exists;
it is imported unmodified through make_loss_fixtures.import_reference under the eager torch-CPU stand-in for `tensorflow`, and
nothing of it is copied or written).  The reference's `loss_layer` calls `bbox_giou` with `# ... bbox_ciou(...)` as the line under
it; here the imported module object gets `loss.bbox_giou = loss.bbox_ciou` at run time, which is that one-line switch.

  python tests/golden/make_ciou_fixtures.py     writes tests/golden/ciou_<case>.npz for every case of tests/lossgrad_cases.py

Stored, in the layout of lossgrad_<case>.npz: the autograd gradient of `yolo_loss` w.r.t. the three heads in float32 and float64
(`conf32_s`, `conf64_s` dense; `idx_s`, `val32_s`, `val64_s` for every other non-zero), `d_ref` [3] = max |g32 - g64| / max |g64|
per scale, the inputs' checksum `sha`; and the forward: `terms32`, `terms64` [n, 3 scales, 3 terms] = the box / confidence / class
sums of every image alone from `decode` + `loss_layer` (as make_loss_fixtures.run_case takes them), `terms_d_ref` [3, 3] = the
largest relative distance over the images between the two, `total32`, `total64` = `yolo_loss` of the batch.

Asserted here, because the comparison means nothing without it: everything make_lossgrad_fixtures.check_ties asserts (the maxima
and minima of the intersection and of the enclosing box are those of GIoU), every value finite, and on every responsible lane
1 - iou + v >= 0.01 and c2 >= 1 (the reference divides by both).
"""
import glob
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_loss_fixtures as MLF  # noqa: E402  (puts tests/ and the package on sys.path)
import make_lossgrad_fixtures as MGF  # noqa: E402


def forward_terms(L, case, y_true, xywh, dtype):
    """-> ([n, 3, 3] per-image sums, the batch's yolo_loss) as the reference computes them in `dtype`."""
    import loss_cases as LC
    ncls, n = case["ncls"], case["n"]
    anchors_t = torch.tensor(LC.ANCHORS.reshape(3, 3, 2), dtype=dtype)
    heads_t = [torch.tensor(h, dtype=dtype) for h in case["heads"]]
    labels_t = [torch.tensor(y, dtype=dtype) for y in y_true]
    xywh_t = torch.tensor(xywh, dtype=dtype)

    def layer(s, i):
        conv = heads_t[s][i:i + 1]
        pred = L.decode(conv, anchors_t[s], LC.STRIDES[s], ncls)
        return [float(v) for v in L.loss_layer(conv, pred, labels_t[s][i:i + 1], xywh_t[i:i + 1], LC.STRIDES[s], ncls,
                                               LC.IOU_LOSS_THRESH)]
    terms = np.array([[layer(s, i) for s in range(3)] for i in range(n)], dtype=np.float64)
    return terms, float(L.yolo_loss([*heads_t, *labels_t, xywh_t], ncls, LC.IOU_LOSS_THRESH, anchors_t))


def run_case(name, mods):
    import ciou_oracle as CO
    import loss_cases as LC
    import loss_oracle as LO
    import lossgrad_cases as GC
    L = mods["loss"]
    assert L.bbox_giou is L.bbox_ciou, "the switch did not take"
    out, problems = MGF.run_case(name, mods)                # gradient, d_ref, sha and the tie / threshold conditions
    case = GC.make_case(name)
    y_true, xywh = mods["utils"].preprocess_true_boxes(case["boxes"].copy(), case["hw"], LC.ANCHORS, case["ncls"])
    t32, total32 = forward_terms(L, case, y_true, xywh, torch.float32)
    t64, total64 = forward_terms(L, case, y_true, xywh, torch.float64)
    if not (np.isfinite(t32).all() and np.isfinite(t64).all() and np.isfinite([total32, total64]).all()):
        problems.append("non-finite loss term")
    d_min, c2_min = CO.lane_conditions(case["heads"], y_true, LC.ANCHORS, LC.STRIDES, case["ncls"], case["hw"])
    if d_min < 0.01:
        problems.append(f"a responsible lane with 1 - iou + v = {d_min:.3e}")
    if c2_min < 1.0:
        problems.append(f"a responsible lane with c2 = {c2_min:.3e}")
    out.update(terms32=t32.astype(np.float32), terms64=t64, terms_d_ref=LO.rel_dist(t32, t64).max(axis=0),
               total32=np.float32(total32), total64=np.float64(total64))
    return out, problems, (d_min, c2_min)


def save_npz(path, arrays):
    """np.savez_compressed with LZMA in place of deflate (np.load reads either): the dense float64 confidence columns, which are
    most of a file, pack a quarter smaller, which keeps every file under the largest lossgrad_*.npz."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(key + ".npy", buf.getvalue())


def main():
    mods = MLF.import_reference()
    mods["loss"].bbox_giou = mods["loss"].bbox_ciou          # loss.py:156 -> :157 on the imported module object
    import lossgrad_cases as GC
    largest = max(os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "lossgrad_*.npz")))
    for name in GC.CASES:
        out, problems, (d_min, c2_min) = run_case(name, mods)
        assert not problems, (name, problems)
        path = os.path.join(HERE, f"ciou_{name}.npz")
        save_npz(path, out)
        assert os.path.getsize(path) <= largest, (path, os.path.getsize(path), largest)
        print(f"{path}: {os.path.getsize(path)} bytes, gradient d_ref {out['d_ref'].tolist()}, terms d_ref max "
              f"{out['terms_d_ref'].max():.2e}, total {out['total64']}, min 1 - iou + v {d_min:.3f}, min c2 {c2_min:.1f}")


if __name__ == "__main__":
    main()
