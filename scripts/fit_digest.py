#!/usr/bin/env python3
"""The bits of a matrix of small `Yolov4.fit` calls, for comparing the Python of two trees on one build of the library.

  python scripts/fit_digest.py --tree PATH --out FILE [--limit 300]

PATH is the root of a checkout (this one, or `git archive` of another commit unpacked somewhere).  A fresh child process puts
PATH's `yolo-v4-tf.keras_amd` on its path, loads THIS tree's libyolo4hip.so through YOLO4HIP_LIB (a change that leaves csrc/ alone
needs one build for both) and runs every case below at (160, 160) and (96, 160): the test suite's seven synthetic images of mixed
sizes, 3 classes, shuffled batches of 3 through max_batch 2, 3 epochs, rate 1e-3, `np.random` and the generator seeded.  FILE gets,
per case, every `.history` value as a float hex string and the sha256 of the trained host weight stream; it names no path, so
the files of two trees are equal byte for byte when the trees compute the same.  The child runs under --limit seconds."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(160, 160), (96, 160)]
SIZES = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)]
BOXES = [3, 0, 5, 8, 1, 4, 2]
# name, dtype, trainable, fit keywords, generator: None (plain), 'augment' (default AugmentConfig) or 'mosaic'; validate
OVERFLOWING_SCALE = 2.0 ** 12            # skips one step per epoch on this data (tests/test_gpu_fit_blocks_f16.py, STATIC_SCALE)
CASES = [
    ("heads_f32_host_val_map", "f32", "heads", {"val_map": True}, None, True),
    ("heads_bf16_augment", "bf16", "heads", {}, "augment", False),
    ("head_blocks_bf16_mosaic", "bf16", "head_blocks", {}, "mosaic", False),
    ("head_blocks_f16_dynamic", "f16", "head_blocks", {"loss_scale": "dynamic"}, None, False),
    ("head_blocks_f16_static_overflowing", "f16", "head_blocks", {"loss_scale": OVERFLOWING_SCALE}, None, False),
    ("heads_bf16_cached", "bf16", "heads", {"cache_features": True}, None, False),
    ("head_blocks_f16_cached", "f16", "head_blocks", {"loss_scale": 2.0 ** 7, "cache_features": True}, None, False),
]


def child(tree, out):
    sys.path[:0] = [os.path.join(tree, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    import yolo4hip
    from helpers import CLASS_DIR
    from test_loss_cpu import _write_dataset
    from yolo4hip.api import Yolov4
    from yolo4hip.augment import AugmentConfig
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    if not os.path.realpath(yolo4hip.__file__).startswith(os.path.realpath(tree) + os.sep):
        raise SystemExit(f"yolo4hip was imported from {yolo4hip.__file__}, not from {tree}")
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    doc = {}
    with tempfile.TemporaryDirectory() as folder:
        import pathlib
        lines = _write_dataset(pathlib.Path(folder), SIZES, BOXES)
        for hw in SHAPES:
            cfg = make_config(hw if hw[0] != hw[1] else hw[0], batch_size=3)
            for name, dtype, trainable, kw, route, validate in CASES:
                m = Yolov4(None, names, cfg, dtype=dtype, max_batch=2, synth_seed=3, tune=False)
                augment = {None: None, "augment": AugmentConfig(), "mosaic": AugmentConfig(mosaic=0.5)}[route]
                np.random.seed(11)
                gen = DataGenerator(lines, names, folder, shuffle=True, config=cfg, augment=augment, seed=5)
                val = DataGenerator(lines, names, folder, shuffle=False, config=cfg) if validate else None
                hist = m.fit(gen, 3, val_data_gen=val, trainable=trainable, learning_rate=1e-3, **kw)
                doc[f"{name}@{hw[0]}x{hw[1]}"] = {
                    "history": {k: [float(v).hex() for v in vals] for k, vals in hist.history.items()},
                    "flat_sha256": hashlib.sha256(np.ascontiguousarray(m._flat).tobytes()).hexdigest()}
                for eng in (m.engine, getattr(m, "_fit_engine", None), getattr(m, "_fit_engine_blocks", None)):
                    if eng is not None:
                        eng.close()
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.tree), a.out)
    env = dict(os.environ, YOLO4HIP_LIB=os.path.join(ROOT, "yolo-v4-tf.keras_amd", "yolo4hip", "libyolo4hip.so"), YOLO4HIP_TUNE="0")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", a.tree, "--out", a.out], env=env,
                          timeout=a.limit)
    sys.exit(done.returncode)


if __name__ == "__main__":
    main()
