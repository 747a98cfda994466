#!/usr/bin/env python3
"""Loss-gradient fixtures: autograd through the REFERENCE'S OWN `loss.yolo_loss` (runs only where the reference exists; it is
imported unmodified through make_loss_fixtures.import_reference, under the same eager torch-CPU stand-in for `tensorflow`;
nothing of it is copied).

  python tests/golden/make_lossgrad_fixtures.py          writes tests/golden/lossgrad_<case>.npz for every case of tests/lossgrad_cases.py
  python tests/golden/make_lossgrad_fixtures.py --seeds  prints, per case, the first seed that passes every assertion

For the cases of tests/lossgrad_cases.py (those of loss_cases.py hold exact ties, see there): `yolo_loss([heads..., labels..., true_xywh])` with the three heads as leaves, then
`.backward()`, once in float32 and once in float64.  Stored per scale s: the confidence columns dense (`conf32_s`, `conf64_s`:
[n, gh, gw, 3]), every other non-zero as flat index + value (`idx_s`, `val32_s`, `val64_s` over the union of both runs'
non-zeros), `d_ref` [3] = max |g32 - g64| / max |g64| per scale -- how far the reference's own float32 gradient lies from
float64, from which the tests take their budget -- and the inputs' checksum `sha`.

Asserted here, because the comparison means nothing without it: every gradient is finite; on every responsible lane the operands
of each maximum / minimum inside GIoU differ by more than 1e-3 px (autodiff's choice at a tie is unspecified) and the enclosing
area is non-zero; no lane lies within 1e-4 of the ignore threshold; no confidence logit, and no class logit of a responsible
lane, is exactly 0 (the stand-in writes the BCE with clamp and abs, whose subgradients at 0 torch picks differently from
TensorFlow's where-based formula, which gives the analytic sigmoid(0) - z there).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_loss_fixtures as MLF  # noqa: E402  (puts tests/ and the package on sys.path)


def autograd(L, heads, y_true, xywh, ncls, dtype):
    import loss_cases as LC
    leaves = [torch.tensor(h, dtype=dtype, requires_grad=True) for h in heads]
    labels = [torch.tensor(y, dtype=dtype) for y in y_true]
    anchors = torch.tensor(LC.ANCHORS.reshape(3, 3, 2), dtype=dtype)
    loss = L.yolo_loss([*leaves, *labels, torch.tensor(xywh, dtype=dtype)], ncls, LC.IOU_LOSS_THRESH, anchors)
    loss.backward()
    return [t.grad.numpy() for t in leaves]


def check_ties(case, y_true, xywh):
    """-> problems (a list) of the tie / threshold conditions, from the float64 restatement's decode."""
    import loss_cases as LC
    import loss_oracle as LO
    problems = []
    anchors3 = LC.ANCHORS.reshape(3, 3, 2)
    for s in range(3):
        _, pred = LO.decode(case["heads"][s], anchors3[s], LC.STRIDES[s], case["ncls"])
        label = np.asarray(y_true[s], dtype=np.float64)
        resp = label[..., 4] == 1
        plo, phi = LO._corners(pred[resp])
        llo, lhi = LO._corners(label[resp][:, 0:4])
        raw = np.minimum(phi, lhi) - np.maximum(plo, llo)
        gaps = np.concatenate([np.abs(plo - llo), np.abs(phi - lhi), np.abs(raw)], axis=-1)
        if gaps.size and gaps.min() <= 1e-3:
            problems.append(f"scale {s}: a maximum / minimum of GIoU within {gaps.min():.2e} px of a tie")
        enc = np.prod(np.maximum(phi, lhi) - np.minimum(plo, llo), axis=-1)
        if (enc == 0).any():
            problems.append(f"scale {s}: zero enclosing area")
        t5 = np.asarray(case["heads"][s]).reshape(label.shape)
        if (t5[..., 4] == 0).any() or (t5[resp][:, 5:] == 0).any():
            problems.append(f"scale {s}: a logit with a BCE gradient is exactly 0")
        _, max_iou, _ = LO.scale_terms(case["heads"][s], y_true[s], xywh, anchors3[s], LC.STRIDES[s], case["ncls"],
                                       LC.IOU_LOSS_THRESH, float(case["hw"][0] * case["hw"][1]))
        if (np.abs(max_iou - LC.IOU_LOSS_THRESH) < 1e-4).any():
            problems.append(f"scale {s}: a lane within 1e-4 of the ignore threshold")
    return problems


def run_case(name, mods, seed=None, ties_only=False):
    import loss_cases as LC
    import lossgrad_cases as GC
    if seed is not None:
        GC.CASES[name] = dict(GC.CASES[name], seed=seed)
    case = GC.make_case(name)
    ncls = case["ncls"]
    y_true, xywh = mods["utils"].preprocess_true_boxes(case["boxes"].copy(), case["hw"], LC.ANCHORS, ncls)
    problems = check_ties(case, y_true, xywh)
    if ties_only:
        return None, problems
    g32 = autograd(mods["loss"], case["heads"], y_true, xywh, ncls, torch.float32)
    g64 = autograd(mods["loss"], case["heads"], y_true, xywh, ncls, torch.float64)
    out = dict(sha=np.array(case["sha"]))
    d_ref = []
    for s in range(3):
        a, b = g32[s], g64[s]
        assert a.dtype == np.float32 and b.dtype == np.float64
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            problems.append(f"scale {s}: non-finite gradient")
        d_ref.append(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
        sh = a.shape[:3] + (3, 5 + ncls)
        a5, b5 = a.reshape(sh).copy(), b.reshape(sh).copy()
        out[f"conf32_{s}"], out[f"conf64_{s}"] = a5[..., 4].copy(), b5[..., 4].copy()
        a5[..., 4] = 0
        b5[..., 4] = 0
        idx = np.flatnonzero((a5 != 0) | (b5 != 0))
        out[f"idx_{s}"] = idx.astype(np.int64)
        out[f"val32_{s}"], out[f"val64_{s}"] = a5.reshape(-1)[idx], b5.reshape(-1)[idx]
    out["d_ref"] = np.array(d_ref, dtype=np.float64)
    return out, problems


def main():
    mods = MLF.import_reference()
    import lossgrad_cases as GC
    if "--seeds" in sys.argv:
        for name in GC.CASES:
            for seed in range(1, 400):
                if not run_case(name, mods, seed, ties_only=True)[1]:
                    print(name, "seed", seed)
                    break
        return
    for name in GC.CASES:
        out, problems = run_case(name, mods)
        assert not problems, (name, problems)
        path = os.path.join(HERE, f"lossgrad_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes, d_ref {out['d_ref'].tolist()}, "
              f"sparse non-zeros {[int(out[f'idx_{s}'].size) for s in range(3)]}")


if __name__ == "__main__":
    main()
