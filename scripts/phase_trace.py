"""In-kernel phase trace of one of the three spatially tiled fused kernels (csrc/phase_trace.h), read from a trace variant build:

    bash scripts/build_variant.sh rbtr resblock "-DRB_TRACE=128"        (or -DRB_TRACE=64: the channel count that is traced)
    YOLO4HIP_LIB=scratch/libyolo4hip_rbtr.so python scripts/phase_trace.py resblock [--json out.json]

and likewise `csp_stage` with "-DCS_TRACE=1" and `stem_down` with "-DSD_TRACE=1".  Runs the 608/80/bf16 batch-32 model and prints, for
workgroup 8 and a few of its tiles / output rows, per wave the shader-clock offset of the first trace point and the cycles between the
points.  Every point is a sched_barrier, so the traced kernel is slower than the shipped one."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd")); sys.path.insert(0, ROOT)

# flag: the variant build; reader / shape: the exported reader and the buffer's [item][wave][point slot] shape (csrc/<kernel>.hip);
# points: names of the recorded points; item / first: what is traced and the number of its first one; simd: the waves that share a
# SIMD; fusions: True sets the three fusions by hand, False takes the shipped schedule (the full-tile resblock launch is part of it)
KERNELS = {
    "resblock": dict(flag="-DRB_TRACE=128|64", reader="y4_rb_trace_read", shape=(3, 8, 16), item="tile", first=1, simd="w, w+4", fusions=False,
                     points=["arrive", "bar0", "1x1", "midbar", "issue", "taps0-2", "taps3-5", "taps6-8", "endbar", "prefetch", "epilogue"]),
    "csp_stage": dict(flag="-DCS_TRACE=1", reader="y4_cs_trace_read", shape=(4, 8, 16), item="tile", first=3, simd="w, w+4", fusions=True,
                      points=["arrive", "landed", "m32", "v32", "extra", "c4", "midbar", "dma", "m5", "v5", "c6", "m7", "v7+st"]),
    "stem_down": dict(flag="-DSD_TRACE=1", reader="y4_sd_trace_read", shape=(4, 16, 8), item="output row", first=5, simd="w, w+4, w+8, w+12",
                      fusions=True, points=["start", "stem", "bar1", "conv", "epi", "bar2"]),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0], epilog="; ".join(
        f"{k}: {v['flag']}, waves {v['simd']} share a SIMD" for k, v in KERNELS.items()))
    ap.add_argument("kernel", choices=sorted(KERNELS))
    ap.add_argument("--json", help="also write cycles[item][wave][point] to this file")
    args = ap.parse_args()
    k = KERNELS[args.kernel]

    import numpy as np
    import torch
    from yolo4hip import weights as W, ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan

    size, n = 608, 32
    eng = Engine(80, make_config(size), max_batch=n, dtype="bf16")
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(size, 80), 0)))
    imgs = torch.from_numpy(W.synth_images(n, size, 0)).to(eng.device)
    if k["fusions"]:
        eng.set_stem_fusion(True); eng.set_chain_fusion(True); eng.set_stage_fusion(True)
    else:
        eng.ensure_schedule(tune=False, verbose=True)
    outs = eng.alloc_outputs(n)
    for _ in range(3): eng.predict_device(imgs, outs)
    torch.cuda.synchronize()

    items, waves, slots = k["shape"]
    names, item = k["points"], k["item"]
    buf = (C.c_ulonglong * (items * waves * slots))()
    reader = getattr(ext.load(), k["reader"], None)
    assert reader is not None, f"not a {k['flag']} build of {args.kernel} (YOLO4HIP_LIB=...)"
    reader.restype = C.c_int
    assert reader(buf) == 0, f"{k['reader']} failed"
    raw = np.array(buf[:], dtype=np.int64).reshape(items, waves, slots)[:, :, :len(names)]
    t0 = raw[0, :, 0].min()
    print(f"cycles per {item} (wave 0, {names[0]} -> {names[0]}):", [int(raw[i + 1, 0, 0] - raw[i, 0, 0]) for i in range(items - 1)])
    for i in range(items):
        print(item.split()[-1], k["first"] + i)
        for w in range(waves):
            r = raw[i, w] - t0
            print("  wave %*d: %s %7d | dt: " % (len(str(waves - 1)), w, names[0], r[0]) +
                  " ".join("%s %5d" % (names[p], r[p] - r[p - 1]) for p in range(1, len(names))))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"kernel": args.kernel, "workgroup": 8, item.split()[-1] + "s": [k["first"] + i for i in range(items)], "points": names,
                       "cycles": (raw - t0).tolist(),
                       "note": "cycles[%s][wave][point], shader-clock cycles from the first arrival; every point is a sched_barrier, so "
                               "the traced kernel is slower than the shipped one" % item.split()[-1]}, f, indent=1)


if __name__ == "__main__":
    main()
