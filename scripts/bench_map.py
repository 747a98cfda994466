#!/usr/bin/env python3
"""What VOC mAP costs: `Yolov4.evaluate_map` (matching on the device, one copy per batch) against the file pipeline of the same
build -- `export_gt` + `export_prediction(bs=32)` + `eval_map` -- on 64 copies of tests/golden/street.jpeg, 416^2, 80 classes,
bf16, synthetic weights, batch 32.  The two are run alternately, --reps times each after one warm-up pass, and the medians of
the wall times are reported; the ground truth is the model's own predictions rounded to integers.  Beside them the device
time of y4_map_match alone, by events, next to one forward of the same batch.  Writes profiles/map/bench_map.json.

  python scripts/bench_map.py [--images 64] [--size 416] [--batch 32] [--dtype bf16] [--reps 5] [--out PATH]"""
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
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map", "bench_map.json"))
    a = ap.parse_args()
    import torch
    from yolo4hip import evalmap, prepost
    from yolo4hip.api import Yolov4, default_class_path
    from yolo4hip.config import make_config
    from yolo4hip.data import MAP_MAX_GT
    work = tempfile.mkdtemp(prefix="bench_map_")
    imgdir = os.path.join(work, "img")
    os.makedirs(imgdir)
    names = [f"street{k:03d}.jpeg" for k in range(a.images)]
    for name in names:
        shutil.copy(os.path.join(ROOT, "tests", "golden", "street.jpeg"), os.path.join(imgdir, name))
    # the 80 COCO names with "_" for " ": the text files separate their fields by blanks, so `eval_map` cannot read "wine glass"
    class_path = os.path.join(work, "classes.txt")
    with open(class_path, "w") as fh:
        fh.write("".join(line.strip().replace(" ", "_") + "\n" for line in open(default_class_path("coco_classes.txt"))))
    m = Yolov4(None, class_path, make_config(a.size), dtype=a.dtype, max_batch=a.batch)

    def folders(tag):
        out = [os.path.join(work, f"{d}_{tag}") for d in ("gt", "pred", "tmp", "out")]
        for d in out:
            os.makedirs(d)
        return out

    # ground truth := the predictions, rounded to integers
    ann0 = os.path.join(work, "ann0.txt")
    with open(ann0, "w") as fh:
        fh.write("".join(f"/data/{name}\n" for name in names))
    _, pred0, _, _ = folders("seed")
    m.export_prediction(ann0, pred0, imgdir, bs=a.batch)
    ann, n_boxes = os.path.join(work, "ann.txt"), 0
    with open(ann, "w") as fh:
        for name in names:
            objs = []
            for line in open(os.path.join(pred0, name.split(".")[0] + ".txt")).read().splitlines()[:MAP_MAX_GT]:
                cls, _conf, *bb = line.split(" ")
                objs.append(",".join(str(int(round(float(v)))) for v in bb) + f",{m.class_names.index(cls)}")
            n_boxes += len(objs)
            fh.write(" ".join([f"/data/{name}"] + objs) + "\n")

    def device_path():
        return m.evaluate_map(ann, imgdir, bs=a.batch, channel_order="bgr")

    def file_path(tag):
        gt, pred, tmp, out = folders(tag)
        m.export_gt(ann, gt)
        m.export_prediction(ann, pred, imgdir, bs=a.batch)
        return evalmap.eval_map(gt, pred, tmp, out, verbose=False)

    res_dev, res_file = device_path(), file_path("warm")
    t_dev, t_file = [], []
    for r in range(a.reps):
        t0 = time.perf_counter(); device_path(); t1 = time.perf_counter(); file_path(f"r{r}"); t2 = time.perf_counter()
        t_dev.append(t1 - t0)
        t_file.append(t2 - t1)

    # y4_map_match alone, by events, beside the forward of the same batch
    eng = m.engine
    raws = [prepost.imread_rgb(os.path.join(imgdir, name))[:, :, ::-1] for name in names[:a.batch]]
    n = len(raws)
    imgs, _ = eng.preprocess_u8_batch(raws)
    gt = np.zeros((n, MAP_MAX_GT, 5), np.float32)
    cnt = np.zeros(n, np.int32)
    for k, line in enumerate(open(ann).read().splitlines()[:n]):
        rows = [[float(v) for v in obj.split(",")] for obj in line.split(" ")[1:]]
        gt[k, :len(rows)], cnt[k] = np.array(rows, np.float32).reshape(-1, 5), len(rows)
    gt_dev, cnt_dev = torch.from_numpy(gt).to(eng.device), torch.from_numpy(cnt).to(eng.device)
    scale_dev = torch.tensor([[r.shape[1], r.shape[0]] for r in raws], dtype=torch.float32, device=eng.device)
    flat, outs, tp_mask = eng.alloc_map_outputs_flat(n)
    thr10 = [float(t) for t in np.arange(0.5, 1.0, 0.05)]

    def timed(fn, reps=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    forward = timed(lambda: eng.forward_device(imgs))
    eng.forward_device(imgs)
    decode = timed(lambda: eng.decode_nms_device(n, outs))
    match1 = timed(lambda: eng.map_match_device(outs, scale_dev, gt_dev, cnt_dev, (0.5,), tp_mask=tp_mask))
    match10 = timed(lambda: eng.map_match_device(outs, scale_dev, gt_dev, cnt_dev, thr10, tp_mask=tp_mask))
    valid = outs[3].cpu().numpy()
    doc = {"shape": {"images": a.images, "size": a.size, "classes": m.num_classes, "batch": a.batch, "dtype": a.dtype,
                     "gt_boxes": n_boxes, "detections_per_image_mean": float(valid.mean()), "schedule": list(m.schedule_source)[:1]},
           "wall_s_median": {"evaluate_map": float(np.median(t_dev)), "export_gt_export_prediction_eval_map": float(np.median(t_file))},
           "wall_s_all": {"evaluate_map": t_dev, "export_gt_export_prediction_eval_map": t_file},
           "file_pipeline_over_evaluate_map": float(np.median(t_file) / np.median(t_dev)),
           "device_ms_median_min_max": {"forward": forward, "decode_nms": decode, "map_match_1_threshold": match1,
                                        "map_match_10_thresholds": match10},
           "map_match_share_of_forward": match1[0] / forward[0],
           "mAP": {"evaluate_map": res_dev["mAP"], "file_pipeline": res_file["mAP"]}, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
