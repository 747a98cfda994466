#!/usr/bin/env python3
"""Throughput of a square and a rectangular input side by side, in one process on one GPU: 608 x 608 and 352 x 608 (H x W,
close to 16:9) at bf16, batch 32, tuned schedules (the shipped one for 608^2; 352 x 608 is tuned on first use and cached under
$YOLO4HIP_CACHE), one stream, predict (forward + decode + NMS) on device-resident float32 images timed with HIP events.
Prints one JSON line per shape and the ratio.

  python scripts/bench_rect.py [--batch 32] [--steps 30] [--warmup 5] [--dtype bf16] [--shapes 608x608,352x608]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))


def run(shape, batch, steps, warmup, dtype, ncls=80):
    import torch
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    plan = build_plan(shape, ncls)
    eng = Engine(ncls, make_config(shape), max_batch=batch, dtype=dtype, alias_workspace=True)
    eng.load_weight_blob(W.flatten(W.synth_weights(plan, 0)))
    src, path = eng.ensure_schedule(tune=True, verbose=False)
    imgs = torch.from_numpy(W.synth_images(batch, shape, seed=1)).to(eng.device)
    outs = eng.alloc_outputs(batch)
    for _ in range(warmup):
        eng.predict_device(imgs, outs)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.predict_device(imgs, outs)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1) / steps
    res = {"shape": f"{shape[0]}x{shape[1]}", "dtype": dtype, "batch": batch, "steps": steps, "schedule": src,
           "ms_per_step": round(ms, 3), "img_per_s": round(batch * 1000.0 / ms, 1),
           "gflop_per_img": round(eng.flops_per_image / 1e9, 2), "valid_img0": int(outs[3][0])}
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--shapes", default="608x608,352x608")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    rows = [run(s, a.batch, a.steps, a.warmup, a.dtype) for s in shapes]
    for r in rows:
        print(json.dumps(r))
    if len(rows) == 2:
        print(json.dumps({"ratio_img_per_s": round(rows[1]["img_per_s"] / rows[0]["img_per_s"], 3),
                          "ratio_flops": round(rows[0]["gflop_per_img"] / rows[1]["gflop_per_img"], 3)}))


if __name__ == "__main__":
    main()
