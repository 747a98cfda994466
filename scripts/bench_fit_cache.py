#!/usr/bin/env python3
"""What `Yolov4.fit(cache_features=True)` saves.  Default: 608^2, 80 classes, batch 32, bf16 compute, shipped schedule.  Writes
profiles/fit/bench_fit_cache.json.

  (a) y4_feature_store and y4_feature_load of one batch at retention level 1 and 2, beside `torch.Tensor.copy_` between two
      device tensors of the same bytes (all three read and write every byte once)
  (b) the cached step -- load, y4_forward_tail, labels + loss + gradients, Adam -- beside the full step (forward instead of load
      and tail) of the same build, for 'heads' (level 1) and 'head_blocks' (level 2); the tail and the load on their own
  (c) `fit` from call to return on 64 JPEG files (the set of scripts/bench_fit_input.py), three epochs, per epoch, uncached and
      cached in turn; the first epoch of a cached call reads the photos and fills the cache

  python scripts/bench_fit_cache.py [--size 608] [--classes 80] [--batch 32] [--dtype bf16] [--reps 20] [--out PATH]

One process; (a) and (b) are hip events around one call, 5 warm-up calls, the median of --reps, the variants measured in turn;
(c) is wall clock.  Every timed step runs under its own time limit (--limit seconds), as in scripts/bench_fit_blocks.py."""
import argparse
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

BACK_TO_BACK = 10                     # calls of a copy between two events: (a)

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--fit-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit", "bench_fit_cache.json"))
    a = ap.parse_args()
    import torch
    import loss_cases as LC
    from bench_fit_input import PHOTO_SIZES
    from yolo4hip import weights as W
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    hw, n, ncls = (a.size, a.size), a.batch, a.classes
    cfg = make_config(a.size, batch_size=n)
    flat = W.flatten(W.synth_weights(build_plan(hw, ncls), seed=1))
    engines = {}
    for level in (1, 2):
        e = engines[level] = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0", alias_workspace=True, retain_head_inputs=level)
        e.load_weight_blob(flat)
        schedule = e.ensure_schedule(tune=False, verbose=False)
    dev = engines[1].device
    imgs = torch.from_numpy(W.synth_images(n, a.size, seed=1)).to(dev)
    rng = np.random.default_rng(0)
    boxes = np.zeros((n, LC.MAX_BOXES, 5), dtype=np.float32)
    for i in range(n):
        m = LC.MAX_BOXES if i % 8 == 0 else int(rng.integers(1, 60))
        boxes[i, :m] = LC._random_boxes(rng, m, hw, ncls)
    boxes_dev = torch.from_numpy(boxes).to(dev)

    def overrun():
        sys.stderr.write(f"a timed step ran longer than {a.limit} s\n")
        sys.stderr.flush()
        os._exit(124)

    def guarded(fn):
        watchdog = threading.Timer(a.limit, overrun)
        watchdog.daemon = True
        watchdog.start()
        try:
            return fn()
        finally:
            watchdog.cancel()

    def once(fn):
        def timed():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1)
        return guarded(timed)

    def stats(ms):
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def alternating(fns, reps):
        """{name: fn} measured in turn, reps rounds -> {name: (median, min, max)}"""
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                ms[k].append(once(fn))
        return {k: stats(v) for k, v in ms.items()}

    # ---- (a) the two copy kernels beside a device-to-device copy of the same bytes
    slots = np.random.default_rng(2).permutation(n)
    copies, caches = {}, {}
    for level, e in engines.items():
        e.forward_device(imgs)
        row = e.feature_row_bytes()[0]
        cache = caches[level] = e.alloc_feature_cache(n)
        src, dst = torch.empty((n * row,), dtype=torch.uint8, device=dev), torch.empty((n * row,), dtype=torch.uint8, device=dev)
        src.random_(0, 256)
        # a copy of this size takes tens of microseconds, about what the host needs to issue one: BACK_TO_BACK calls between
        # the two events keep the queue filled, and a sample is their mean
        def burst(fn):
            def run():
                for _ in range(BACK_TO_BACK):
                    fn()
            return run
        ms = alternating({"y4_feature_store": burst(lambda e=e, cache=cache: e.store_features(cache, slots)),
                          "y4_feature_load": burst(lambda e=e, cache=cache: e.load_features(cache, slots)),
                          "torch_copy_": burst(lambda src=src, dst=dst: dst.copy_(src))}, a.reps)
        ms = {k: tuple(x / BACK_TO_BACK for x in v) for k, v in ms.items()}
        copies[f"level{level}"] = {
            "bytes": n * row, "row_bytes": row, "calls_per_sample": BACK_TO_BACK, "ms_median_min_max": ms,
            "GBps_read_plus_write": {k: 2 * n * row / (v[0] * 1e-3) / 1e9 for k, v in ms.items()},
            "store_over_copy": ms["y4_feature_store"][0] / ms["torch_copy_"][0],
            "load_over_copy": ms["y4_feature_load"][0] / ms["torch_copy_"][0],
            "copy_spread_max_over_min": ms["torch_copy_"][2] / ms["torch_copy_"][1]}
        del src, dst
        e.store_features(cache, np.arange(n))                    # what (b) loads: image i in row i

    # ---- (b) the cached step beside the full step
    steps = {}
    for trainable, level in (("heads", 1), ("head_blocks", 2)):
        e, cache = engines[level], caches[level]
        groups = ("heads", "blocks") if level == 2 else ("heads",)
        state = {g: e._group_state(g, flat) for g in groups}
        grad = {g: torch.empty((e._group_floats(g),), dtype=torch.float32, device=dev) for g in groups}
        weight = torch.full((n,), 1.0 / n, dtype=torch.float32, device=dev)
        rows = np.arange(n)

        def behind(e=e, groups=groups, state=state, grad=grad, weight=weight):
            labels = e.assign_device(boxes_dev)
            for g in groups:
                e._group_grad_device(g, n, None, labels, None, weight, grad[g], False)
            e.loss_device(n, records=labels)
            for g in groups:
                e._group_adam_step(g, state[g], grad[g], lr=1e-6)

        def full(e=e, behind=behind):
            e.forward_device(imgs)
            behind()

        def cached(e=e, cache=cache, rows=rows, behind=behind):
            e.load_features(cache, rows)
            e.forward_tail_device(n)
            behind()
        ms = alternating({"full_step": full, "cached_step": cached, "behind_the_forward": behind,
                          "forward": lambda e=e: e.forward_device(imgs),
                          "load": lambda e=e, cache=cache, rows=rows: e.load_features(cache, rows),
                          "tail": lambda e=e: e.forward_tail_device(n)}, a.reps)
        steps[trainable] = {"ms_median_min_max": ms, "cached_over_full": ms["cached_step"][0] / ms["full_step"][0],
                            "tail_share_of_cached_step": ms["tail"][0] / ms["cached_step"][0],
                            "load_share_of_cached_step": ms["load"][0] / ms["cached_step"][0]}
    for e in engines.values():
        e.close()
    del caches, engines

    # ---- (c) fit from call to return, per epoch
    from PIL import Image
    epochs = {"uncached": [], "cached": []}
    with tempfile.TemporaryDirectory() as folder:
        lines = []
        for i in range(64):
            h, w = PHOTO_SIZES[i % len(PHOTO_SIZES)]
            base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
            photo = np.clip(np.kron(base, np.ones((8, 8, 1)))[:h, :w] + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(photo).save(os.path.join(folder, f"im{i}.jpg"), quality=90)
            objs = [f"{x},{y},{x + w // 4},{y + h // 4},{c % ncls}" for c, (x, y) in
                    enumerate(zip(rng.integers(0, w // 2, 8), rng.integers(0, h // 2, 8)))]
            lines.append(f"im{i}.jpg " + " ".join(objs) + "\n")
        names = os.path.join(folder, "classes.txt")
        with open(names, "w") as fh:
            fh.write("".join(f"c{c}\n" for c in range(ncls)))
        model = Yolov4(None, names, cfg, dtype=a.dtype, max_batch=n, synth_seed=1, tune=False)
        for r in range(a.fit_rounds + 1):                        # (round 0 warms up: engines, workspaces, file cache)
            for variant in ("uncached", "cached"):
                marks = [0.0]

                class Clock:
                    def on_epoch_end(self, epoch, logs):
                        marks.append(time.perf_counter())
                np.random.seed(3)
                gen = DataGenerator(lines, names, folder, shuffle=True, config=cfg)

                def run():
                    marks[0] = time.perf_counter()
                    return model.fit(gen, 3, callbacks=[Clock()], trainable="heads", learning_rate=1e-6,
                                     cache_features=variant == "cached")
                guarded(run)
                if r > 0:
                    epochs[variant].append([(t1 - t0) * 1e3 for t0, t1 in zip(marks, marks[1:])])
    fit_doc = {"images": 64, "epochs_ms_per_round": epochs,
               "epoch_ms_median": {k: [float(np.median([r[i] for r in v])) for i in range(3)] for k, v in epochs.items()}}
    fit_doc["cached_epoch_over_uncached_epoch"] = float(np.mean(fit_doc["epoch_ms_median"]["cached"][1:]) /
                                                        np.mean(fit_doc["epoch_ms_median"]["uncached"][1:]))
    doc = {"shape": {"size": a.size, "classes": ncls, "batch": n, "dtype": a.dtype, "schedule": list(schedule)[:1]},
           "copy_kernels": copies, "steps": steps, "fit_heads_3_epochs": fit_doc, "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
