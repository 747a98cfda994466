#!/usr/bin/env python3
"""What the COCO protocol costs beside the VOC one, on one GPU: 608^2, 80 classes, batch 32, bf16, the shipped schedule, the
images of bench.py (`weights.synth_images(seed=0)`, written as PNG files for the end-to-end part), synthetic weights.

  (a) y4_coco_match at 10 thresholds x 4 ranges against y4_map_match at 10 thresholds: the same build, the same device inputs --
      the kept boxes of one batch and --gt-rows ground-truth rows per image (the image's own detections rounded to integers,
      filled up with seeded random boxes) --, by events, --reps alternating measurements each, medians;
  (b) `Yolov4.evaluate_coco` against `Yolov4.evaluate_map(iou_thresholds=np.arange(0.5, 1.0, 0.05))` end to end on the same
      --images images, wall time, --reps alternating measurements each after one warm-up pass, medians.
The COCO kernel does four times the walks and rescans the free rows per detection; there is no target, the ratio is written down.
Writes profiles/coco/bench_coco.json (--out).

  python scripts/bench_coco.py [--images 64] [--size 608] [--batch 32] [--dtype bf16] [--reps 20] [--gt-rows 20] [--out PATH]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gt-rows", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco", "bench_coco.json"))
    a = ap.parse_args()
    import torch
    from PIL import Image
    from yolo4hip import cocoeval, weights as W
    from yolo4hip.api import Yolov4, default_class_path
    from yolo4hip.config import make_config
    from yolo4hip.data import MAP_MAX_GT
    m = Yolov4(None, default_class_path("coco_classes.txt"), make_config(a.size), dtype=a.dtype, max_batch=a.batch)
    m._ensure_tuned()
    eng = m.engine
    work = tempfile.mkdtemp(prefix="bench_coco_")
    imgdir = os.path.join(work, "img")
    os.makedirs(imgdir)
    names = [f"synth{k:03d}.png" for k in range(a.images)]
    raws = []
    for k0 in range(0, a.images, a.batch):
        part = W.synth_images(min(a.batch, a.images - k0), a.size, seed=0, first_index=k0)
        for k, img in enumerate(part):
            raws.append(np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8))
            Image.fromarray(raws[-1]).save(os.path.join(imgdir, names[k0 + k]))

    # ground truth per image: its own detections in pixels, rounded to integers, filled up to --gt-rows with seeded random boxes
    rng = np.random.default_rng(0)
    gts, n_det = [], []
    for k0 in range(0, a.images, a.batch):
        part = raws[k0:k0 + a.batch]
        boxes, _scores, classes, valid = m.inference_model.predict(eng.preprocess_u8_batch(part)[0])
        for k in range(len(part)):
            nb = int(valid[k])
            n_det.append(nb)
            rows = [[int(round(float(v) * a.size)) for v in boxes[k, j]] + [int(classes[k, j])] for j in range(min(nb, a.gt_rows))]
            rows = [r for r in rows if r[2] > r[0] and r[3] > r[1]]
            while len(rows) < a.gt_rows:
                x1, y1 = (int(v) for v in rng.integers(0, a.size - 8, 2))
                w, h = (int(v) for v in rng.integers(8, a.size // 2, 2))
                rows.append([x1, y1, min(x1 + w, a.size), min(y1 + h, a.size), int(rng.integers(0, m.num_classes))])
            gts.append(rows)
    ann = os.path.join(work, "ann.txt")
    with open(ann, "w") as fh:
        for name, rows in zip(names, gts):
            fh.write(" ".join([f"/data/{name}"] + [",".join(str(v) for v in r) for r in rows]) + "\n")

    # ---- (a) the two kernels on the same device inputs, alternating
    n = min(a.batch, a.images)
    imgs, _ = eng.preprocess_u8_batch(raws[:n])
    gt = np.zeros((n, MAP_MAX_GT, 5), np.float32)
    for k in range(n):
        gt[k, :len(gts[k])] = np.array(gts[k], np.float32)
    gt_dev = torch.from_numpy(gt).to(eng.device)
    cnt_dev = torch.tensor([len(g) for g in gts[:n]], dtype=torch.int32, device=eng.device)
    scale_dev = torch.full((n, 2), float(a.size), dtype=torch.float32, device=eng.device)
    flat, outs, _cand, match_out = eng.alloc_coco_outputs_flat(n, 4, MAP_MAX_GT)
    tp_mask = torch.empty((n, eng.T), dtype=torch.int32, device=eng.device)
    iou, score = m._thresholds
    eng.forward_device(imgs)
    eng.decode_nms_device(n, outs, iou, score)
    thr_voc = [float(t) for t in np.arange(0.5, 1.0, 0.05)]
    thr_coco, ranges = cocoeval.IOU_THRESHOLDS, cocoeval.AREA_RANGES

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        return e0.elapsed_time(e1)

    fns = {"map_match_10": lambda: eng.map_match_device(outs, scale_dev, gt_dev, cnt_dev, thr_voc, tp_mask=tp_mask),
           "coco_match_10x4": lambda: eng.coco_match_device(outs, scale_dev, gt_dev, cnt_dev, thr_coco, ranges, out=match_out),
           "forward": lambda: eng.forward_device(imgs)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    eng.forward_device(imgs)                                   # (the heads of this batch again, for whoever reads on)

    # ---- (b) end to end, alternating
    def coco():
        return m.evaluate_coco(ann, imgdir, bs=a.batch)

    def voc():
        return m.evaluate_map(ann, imgdir, bs=a.batch, iou_thresholds=np.arange(0.5, 1.0, 0.05))

    res_coco, res_voc = coco(), voc()
    wall = {"evaluate_coco": [], "evaluate_map_10": []}
    for _ in range(a.reps):
        t0 = time.perf_counter(); coco(); t1 = time.perf_counter(); voc(); t2 = time.perf_counter()
        wall["evaluate_coco"].append(t1 - t0)
        wall["evaluate_map_10"].append(t2 - t1)

    med = {k: float(np.median(v)) for k, v in ms.items()}
    doc = {"shape": {"images": a.images, "size": a.size, "classes": m.num_classes, "batch": a.batch, "dtype": a.dtype,
                     "gt_rows_per_image": a.gt_rows, "detections_per_image_mean": float(np.mean(n_det)),
                     "detections_per_image_max": int(np.max(n_det)), "schedule": list(m.schedule_source)[:1]},
           "device_ms_median": med, "device_ms_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "coco_match_over_map_match": med["coco_match_10x4"] / med["map_match_10"],
           "coco_match_share_of_forward": med["coco_match_10x4"] / med["forward"],
           "wall_s_median": {k: float(np.median(v)) for k, v in wall.items()}, "wall_s_all": wall,
           "evaluate_coco_over_evaluate_map": float(np.median(wall["evaluate_coco"]) / np.median(wall["evaluate_map_10"])),
           "numbers": {"AP": res_coco["AP"], "AP50": res_coco["AP50"], "APs": res_coco["APs"], "APm": res_coco["APm"],
                       "APl": res_coco["APl"], "voc_mAP_mean": res_voc["mAP_mean"], "voc_mAP_50": res_voc["mAP"]},
           "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
