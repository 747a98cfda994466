#!/usr/bin/env python3
"""What the validation loss costs on the device: y4_loss_assign + y4_loss on the heads of a real forward, against the same
formula in torch ops on the GPU over y4_get_heads' dense heads (what a user without the kernel would write), and against
one forward step.  Default: 608^2, 80 classes, batch 32, bf16 compute.  Writes profiles/loss/bench_loss.json.

  python scripts/bench_loss.py [--size 608] [--classes 80] [--batch 32] [--dtype bf16] [--reps 30] [--box-loss giou|ciou] [--out PATH]

Timing: hip events around one call, 5 warm-up calls, the median of --reps; the shader clock read afterwards is noted."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def torch_loss(heads, labels, xywh, anchors, strides, ncls, thresh, area):
    """loss.py's arithmetic in torch ops on dense labels -> [n, 3, 3]; materialises the [n, gh, gw, 3, max_boxes] IoU tensor."""
    import torch
    import torch.nn.functional as F

    def parts(b1, b2):
        a1, a2 = b1[..., 2] * b1[..., 3], b2[..., 2] * b2[..., 3]
        lo1, hi1 = b1[..., :2] - b1[..., 2:] * 0.5, b1[..., :2] + b1[..., 2:] * 0.5
        lo2, hi2 = b2[..., :2] - b2[..., 2:] * 0.5, b2[..., :2] + b2[..., 2:] * 0.5
        inter = (torch.minimum(hi1, hi2) - torch.maximum(lo1, lo2)).clamp(min=0).prod(-1)
        union = a1 + a2 - inter
        return inter / (union + 1e-7), union, (torch.maximum(hi1, hi2) - torch.minimum(lo1, lo2)).prod(-1)
    out = []
    for s in range(3):
        n, gh, gw, _ = heads[s].shape
        t = heads[s].reshape(n, gh, gw, 3, 5 + ncls)
        gy, gx = torch.meshgrid(torch.arange(gh, device=t.device), torch.arange(gw, device=t.device), indexing="ij")
        grid = torch.stack([gx, gy], -1)[None, :, :, None, :].float()
        pred = torch.cat([(torch.sigmoid(t[..., :2]) + grid) * strides[s], torch.exp(t[..., 2:4]) * anchors[s]], -1)
        lab = labels[s]
        respond = lab[..., 4]
        iou, union, enc = parts(pred, lab[..., :4])
        giou = iou - torch.where(enc == 0, torch.zeros_like(enc), (enc - union) / enc)
        box = respond * (2.0 - lab[..., 2] * lab[..., 3] / area) * (1 - giou)
        cls = respond * F.binary_cross_entropy_with_logits(t[..., 5:], lab[..., 5:], reduction="none").sum(-1)
        max_iou = parts(pred[..., None, :], xywh[:, None, None, None, :, :])[0].max(-1).values
        bgd = (1 - respond) * (max_iou < thresh).float()
        bce = F.binary_cross_entropy_with_logits(t[..., 4], respond, reduction="none")
        conf = (respond - torch.sigmoid(t[..., 4])) ** 2 * (respond * bce + bgd * bce)
        out.append(torch.stack([x.sum((1, 2, 3)) for x in (box, conf, cls)], -1))
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box-loss", default="giou", choices=("giou", "ciou"), help="the box term the engine evaluates and differentiates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "bench_loss.json"))
    a = ap.parse_args()
    import torch
    import loss_cases as LC
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.data import preprocess_true_boxes
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    hw, n, ncls = (a.size, a.size), a.batch, a.classes
    cfg = make_config(a.size)
    eng = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0", alias_workspace=True, box_loss=a.box_loss)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(hw, ncls), seed=1)))
    schedule = eng.ensure_schedule(tune=False, verbose=False)
    imgs = torch.from_numpy(W.synth_images(n, a.size, seed=1)).to(eng.device)
    rng = np.random.default_rng(0)
    boxes = np.zeros((n, LC.MAX_BOXES, 5), dtype=np.float32)
    for i in range(n):                                           # 1 .. 100 boxes per image, some images full
        m = LC.MAX_BOXES if i % 8 == 0 else int(rng.integers(1, 60))
        boxes[i, :m] = LC._random_boxes(rng, m, hw, ncls)
    boxes_dev = torch.from_numpy(boxes).to(eng.device)
    y_true, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    labels_dev = [torch.from_numpy(y).to(eng.device) for y in y_true]
    xywh_dev = torch.from_numpy(xywh).to(eng.device)
    anchors = torch.tensor(LC.ANCHORS.reshape(3, 3, 2).astype(np.float32), device=eng.device)
    thr = float(cfg["iou_loss_thresh"])

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    forward = timed(lambda: eng.forward_device(imgs), a.reps)
    eng.forward_device(imgs)
    kernel_out = eng.loss_device(n, boxes_dev=boxes_dev)
    triple = eng.assign_device(boxes_dev)
    kernel = timed(lambda: eng.loss_device(n, boxes_dev=boxes_dev), a.reps)
    loss_only = timed(lambda: eng.loss_device(n, records=triple), a.reps)

    def baseline():
        return torch_loss(eng.heads_device(n), labels_dev, xywh_dev, anchors, LC.STRIDES, ncls, thr, float(hw[0] * hw[1]))
    base_out = baseline()
    base = timed(baseline, max(5, a.reps // 3))
    rel = float(((kernel_out - base_out).abs() / base_out.abs().clamp(min=1e-30)).max())
    # bytes of head data the loss kernel touches: 5 logits per (cell, anchor) lane, and the C class logits of the responsible lanes
    lanes = n * sum(3 * (a.size // s) ** 2 for s in LC.STRIDES)
    responsible = int(sum((y[..., 4] == 1).sum() for y in y_true))
    touched = 4 * (5 * lanes + ncls * responsible)
    head_bytes = 4 * eng.head_cstride * lanes // 3
    clock = None
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        clock = [l.strip() for l in smi.splitlines() if "sclk" in l][:1]
    except Exception:
        pass
    doc = {"shape": {"size": a.size, "classes": ncls, "batch": n, "dtype": a.dtype, "max_boxes": LC.MAX_BOXES, "box_loss": a.box_loss,
                     "responsible_cells": responsible, "schedule": list(schedule)[:1]},
           "ms_median_min_max": {"forward": forward, "loss_assign_plus_loss": kernel, "loss_alone": loss_only,
                                 "torch_baseline_get_heads_plus_formula": base},
           "speedup_over_torch_baseline": base[0] / kernel[0],
           "loss_share_of_forward_step": kernel[0] / forward[0],
           "head_bytes_stored": head_bytes, "head_bytes_touched": touched,
           "achieved_GBps_on_touched_bytes": touched / (loss_only[0] * 1e-3) / 1e9,
           "max_rel_diff_kernel_vs_torch_baseline": rel if a.box_loss == "giou" else None,      # (the torch baseline is the GIoU formula)
           "reps": a.reps, "sclk_after": clock}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
