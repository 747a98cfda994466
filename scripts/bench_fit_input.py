#!/usr/bin/env python3
"""What the input side of a `Yolov4.fit` batch costs: the host path (`DataGenerator.get_data`'s resize of every image on the host,
a float32 batch, one upload) against the device path (`Engine.augment_u8_batch`: raw uint8 upload, one y4_augment_u8_ragged
launch) with the identity config and with the default AugmentConfig, and the augment kernel alone against y4_resize_u8_ragged
on the same descriptor table.  Default: 608^2, batch 32, bf16 engine, 32 in-memory photos of mixed sizes.  Writes
profiles/fit/bench_fit_input.json.

The mosaic row: y4_mosaic_u8_ragged beside y4_augment_u8_ragged on the SAME canvases (the default config's rows, every cut at
(H, W): one tile per canvas) and on drawn mosaic canvases (AugmentConfig(mosaic=1): four tiles each), `Engine.mosaic_u8_batch`
beside `Engine.augment_u8_batch` from the host images, and the host time of `DataGenerator.raw_mosaic` beside `raw` on 64
JPEG files of those sizes in a temporary folder (decoding included: a mosaic batch reads its partners too).

  python scripts/bench_fit_input.py [--size 608] [--batch 32] [--dtype bf16] [--reps 20] [--out PATH]

Timing: the three paths are wall clock from the host images to a synchronised device batch, measured in turn (host, identity,
default, host, ...) so that they share the machine's state, 2 warm-up rounds, the median of --reps; the kernels are hip events
around one launch on device-resident buffers, alternating likewise."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

PHOTO_SIZES = [(480, 640), (375, 500), (600, 800), (720, 1280), (640, 480), (333, 500), (1080, 1920), (427, 640)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit", "bench_fit_input.json"))
    a = ap.parse_args()
    import torch
    from yolo4hip import ext, prepost
    from yolo4hip.augment import AugmentConfig, draw_mosaic_params, draw_params
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    H = W = a.size
    n = a.batch
    eng = Engine(80, make_config(a.size), max_batch=n, dtype=a.dtype, device="cuda:0", alias_workspace=True)
    schedule = eng.ensure_schedule(tune=False, verbose=False)
    rng = np.random.default_rng(0)
    photos = []
    for i in range(n):
        h, w = PHOTO_SIZES[i % len(PHOTO_SIZES)]
        base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3))
        img = np.kron(base, np.ones((8, 8, 1)))[:h, :w] + rng.integers(-20, 21, (h, w, 3))
        photos.append(np.clip(img, 0, 255).astype(np.uint8))
    sizes = [p.shape[:2] for p in photos]
    ident, full = AugmentConfig.identity(), AugmentConfig()
    draws = np.random.default_rng(5)

    def host_path():
        X = np.empty((n, H, W, 3), dtype=np.float32)
        for i, img in enumerate(photos):
            X[i] = prepost.resize_bilinear(img, (W, H)) / 255.
        return eng._to_device_images(X)

    def device_path(cfg):
        return eng.augment_u8_batch(photos, draw_params(draws, sizes, (H, W), cfg), pad_value=cfg.pad_value)

    mosaic_cfg = AugmentConfig(mosaic=1.0)

    def mosaic_path():
        tile_src, params4, cuts = draw_mosaic_params(draws, n, n, (H, W), mosaic_cfg)
        tile_src[:, 0] = np.arange(n)
        return eng.mosaic_u8_batch(photos, tile_src, params4, cuts, pad_value=mosaic_cfg.pad_value)

    paths = {"host_resize_float32_upload": host_path, "device_identity_config": lambda: device_path(ident),
             "device_default_config": lambda: device_path(full), "device_mosaic": mosaic_path}
    wall = {k: [] for k in paths}
    for r in range(a.reps + 2):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                wall[k].append((time.perf_counter() - t0) * 1e3)

    # ---- the kernels alone, on device-resident sources and tables
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(eng.device)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=eng.device)

    def table(cls, params):
        desc, off = (cls * n)(), 0
        for d, p, img in zip(desc, params, photos):
            d.offset, d.h, d.w = off, img.shape[0], img.shape[1]
            d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
            if cls is ext.y4_augment_desc:
                d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])
            off += img.size
        return torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(eng.device)
    p_ident = draw_params(np.random.default_rng(1), sizes, (H, W), ident)
    p_full = draw_params(np.random.default_rng(1), sizes, (H, W), full)
    p_flip = p_ident.copy()
    p_flip["flip"] = 1
    lib = eng.lib
    offsets = np.concatenate([[0], np.cumsum([p.size for p in photos])])

    def mosaic_table(tile_src, params4, cuts):
        desc = (ext.y4_augment_desc * (4 * n))()
        for d, k, p in zip(desc, tile_src.reshape(-1), params4.reshape(-1)):
            d.offset, d.h, d.w = int(offsets[k]), photos[k].shape[0], photos[k].shape[1]
            d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
            d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])
        return (torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(eng.device),
                torch.from_numpy(np.ascontiguousarray(cuts, dtype=np.int32)).to(eng.device))

    def mosaic_fn(cuts_dev):
        return lambda s, d, n_, o, H_, W_, pad, st: lib.y4_mosaic_u8_ragged(s, d, ext.ptr(cuts_dev), n_, o, H_, W_, pad, st)
    own = np.repeat(np.arange(n)[:, None], 4, axis=1)
    single_desc, single_cuts = mosaic_table(own, np.repeat(p_full[:, None], 4, axis=1), np.tile([H, W], (n, 1)))
    m_src, m_params, m_cuts = draw_mosaic_params(np.random.default_rng(1), n, n, (H, W), mosaic_cfg)
    m_src[:, 0] = np.arange(n)
    four_desc, four_cuts = mosaic_table(m_src, m_params, m_cuts)
    launches = {
        "resize_u8_ragged_stretch": (lib.y4_resize_u8_ragged, table(ext.y4_image_desc, p_ident)),
        "augment_identity": (lib.y4_augment_u8_ragged, table(ext.y4_augment_desc, p_ident)),
        "augment_flip_only": (lib.y4_augment_u8_ragged, table(ext.y4_augment_desc, p_flip)),
        "augment_default_config": (lib.y4_augment_u8_ragged, table(ext.y4_augment_desc, p_full)),
        "mosaic_same_canvases_as_augment_default_config": (mosaic_fn(single_cuts), single_desc),
        "mosaic_four_tiles_default_config": (mosaic_fn(four_cuts), four_desc),
    }
    # the single-tile mosaic table must give the canvases of the augment launch it is timed beside
    ext.check(lib.y4_augment_u8_ragged(ext.ptr(src), ext.ptr(launches["augment_default_config"][1]), n, ext.ptr(out), H, W, 128,
                                       ext.stream_ptr()))
    want = out.clone()
    ext.check(launches["mosaic_same_canvases_as_augment_default_config"][0](ext.ptr(src), ext.ptr(single_desc), n, ext.ptr(out), H, W,
                                                                           128, ext.stream_ptr()))
    torch.cuda.synchronize()
    if not torch.equal(out, want):
        raise SystemExit("y4_mosaic_u8_ragged with cuts (H, W) differs from y4_augment_u8_ragged on the same rows")
    kern = {k: [] for k in launches}
    for r in range(a.reps + 5):
        for k, (fn, desc_dev) in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ext.check(fn(ext.ptr(src), ext.ptr(desc_dev), n, ext.ptr(out), H, W, 128, ext.stream_ptr()))
            e1.record()
            e1.synchronize()
            if r >= 5:
                kern[k].append(e0.elapsed_time(e1))

    # ---- the generator's host side: raw(i) against raw_mosaic(i), files decoded from a temporary folder
    from PIL import Image
    from yolo4hip.data import DataGenerator
    gen_ms = {"raw": [], "raw_mosaic": []}
    with tempfile.TemporaryDirectory() as folder:
        lines = []
        for i in range(2 * n):
            photo = photos[i % n]
            h, w = photo.shape[:2]
            Image.fromarray(photo).save(os.path.join(folder, f"im{i}.jpg"), quality=90)
            objs = [f"{x},{y},{x + w // 4},{y + h // 4},{c % 80}" for c, (x, y) in
                    enumerate(zip(rng.integers(0, w // 2, 8), rng.integers(0, h // 2, 8)))]
            lines.append(f"im{i}.jpg " + " ".join(objs) + "\n")
        names = os.path.join(folder, "classes.txt")
        with open(names, "w") as fh:
            fh.write("".join(f"c{c}\n" for c in range(80)))
        cfg = make_config(a.size, batch_size=n)
        gens = {"raw": DataGenerator(lines, names, folder, shuffle=False, config=cfg, augment=full, seed=5),
                "raw_mosaic": DataGenerator(lines, names, folder, shuffle=False, config=cfg, augment=mosaic_cfg, seed=5)}
        distinct = []
        for r in range(min(a.reps, 5) + 1):
            for k, g in gens.items():
                t0 = time.perf_counter()
                got = getattr(g, k)(r % 2)
                if r >= 1:
                    gen_ms[k].append((time.perf_counter() - t0) * 1e3)
                    if k == "raw_mosaic":
                        distinct.append(len(got[0]))

    def stats(ms):
        return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]
    moved = int(src.numel()) + n * H * W * 3                       # every source byte once + every canvas byte once
    kern_stats = {k: stats(v) for k, v in kern.items()}
    doc = {"shape": {"size": a.size, "batch": n, "dtype": a.dtype, "schedule": list(schedule)[:1], "photo_sizes": PHOTO_SIZES},
           "raw_upload_bytes": int(src.numel()), "float32_upload_bytes": n * H * W * 3 * 4,
           "input_ms_median_min_max": {k: stats(v) for k, v in wall.items()},
           "kernel_ms_median_min_max": kern_stats,
           "kernel_GBps_source_plus_canvas_bytes": {k: moved / (v[0] * 1e-3) / 1e9 for k, v in kern_stats.items()},
           "augment_identity_over_resize_ragged": kern_stats["augment_identity"][0] / kern_stats["resize_u8_ragged_stretch"][0],
           "mosaic_over_augment_same_canvases": kern_stats["mosaic_same_canvases_as_augment_default_config"][0]
           / kern_stats["augment_default_config"][0],
           "generator_host_ms_median_min_max": {k: stats(v) for k, v in gen_ms.items()},
           "generator_dataset_files": 2 * n, "raw_mosaic_distinct_images_per_batch": distinct,
           "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    eng.close()


if __name__ == "__main__":
    main()
