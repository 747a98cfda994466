#!/usr/bin/env python3
"""Preprocessing of a batch of mixed-size uint8 photos, old against new, in one process on one GPU: 32 images of assorted
sizes (VGA to 1080p, portrait and landscape) through

  loop    Engine.preprocess_u8: one pageable H2D copy and one y4_resize_u8 launch per image, then a synchronize
  batch   Engine.preprocess_u8_batch: one pinned staging buffer, one H2D copy, one y4_resize_u8_ragged launch (stretch)
  batch+lb  the same with letterbox=True

Each step is timed on the host from the call to the finished result (torch.cuda.synchronize), which is what a caller waits
for; the median and the minimum over --steps are reported.  The device time of the resize kernels alone is best read with
`rocprofv3 --kernel-trace --stats -- python scripts/bench_letterbox.py` (resize_u8_kernel against canvas_u8_kernel).
The stretch results of both paths are compared byte for byte first.  Prints one JSON line.

  python scripts/bench_letterbox.py [--images 32] [--steps 50] [--warmup 5] [--size 608x608]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))

PHOTO_SIZES = [(480, 640), (640, 480), (720, 1280), (1280, 720), (1080, 1920), (1920, 1080), (768, 1024), (1024, 768),
               (600, 800), (375, 500), (500, 375), (960, 1280)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", default="608x608", help="network input H x W")
    a = ap.parse_args()
    import numpy as np
    import torch
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    H, W = (int(v) for v in a.size.split("x"))
    rng = np.random.default_rng(0)
    sizes = [PHOTO_SIZES[i % len(PHOTO_SIZES)] for i in range(a.images)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    eng = Engine(3, make_config((H, W)), max_batch=a.images, dtype="bf16")
    eng.adopt_packed()                       # no forward runs here: preprocessing only

    old = eng.preprocess_u8(imgs)
    new, _ = eng.preprocess_u8_batch(imgs)
    torch.cuda.synchronize()
    if not torch.equal(old, new):
        raise SystemExit("stretch results differ between preprocess_u8 and preprocess_u8_batch")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
            torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3)}

    res = {"size": f"{H}x{W}", "images": a.images, "source_mb": round(sum(i.nbytes for i in imgs) / 2 ** 20, 1),
           "steps": a.steps, "device": torch.cuda.get_device_name(0),
           "loop": timed(lambda: eng.preprocess_u8(imgs)),
           "batch": timed(lambda: eng.preprocess_u8_batch(imgs)),
           "batch_letterbox": timed(lambda: eng.preprocess_u8_batch(imgs, letterbox=True))}
    res["speedup_median"] = round(res["loop"]["median_ms"] / res["batch"]["median_ms"], 2)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
