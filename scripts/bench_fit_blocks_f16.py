#!/usr/bin/env python3
"""What the fit(trainable='head_blocks') step costs on an f16 model (y4_block_grad_scaled) beside the bf16 step (y4_block_grad) of
the same build.  Default: 608^2, 80 classes, batch 32, shipped schedules.  Writes profiles/fit/bench_fit_blocks_f16.json.

Three engines at retention level 2 -- one f16, two bf16 -- measured alternately: the two bf16 engines run the same work, so their
difference is the spread that the f16 / bf16 difference has to be read against.  Per engine
  forward     the forward alone (the two dtypes run different shipped schedules)
  step        forward / labels + loss + y4_head_grad / the block gradient / both Adam steps with their re-packs, one timed call
  block_grad  y4_block_grad_scaled (f16: --loss-scale, one overflow word, zeroed inside the timed call as fit does per batch)
              or y4_block_grad (bf16) alone, on the tensors the forward left; and its kernels' durations from torch.profiler

  python scripts/bench_fit_blocks_f16.py [--size 608] [--classes 80] [--batch 32] [--loss-scale 256] [--reps 20] [--out PATH]

One process; hip events around one call, 5 warm-up calls, the median of --reps.  Every timed call runs under its own time limit
(--limit seconds), as in scripts/bench_fit_blocks.py."""
import argparse
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--loss-scale", type=float, default=256.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit", "bench_fit_blocks_f16.json"))
    a = ap.parse_args()
    import torch
    import loss_cases as LC
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    hw, n, ncls = (a.size, a.size), a.batch, a.classes
    cfg = make_config(a.size)
    flat = W.flatten(W.synth_weights(build_plan(hw, ncls), seed=1))
    engines, schedules = {}, {}
    for name, dtype in (("f16", "f16"), ("bf16_a", "bf16"), ("bf16_b", "bf16")):
        e = engines[name] = Engine(ncls, cfg, max_batch=n, dtype=dtype, device="cuda:0", alias_workspace=True, retain_head_inputs=2)
        e.load_weight_blob(flat)
        schedules[name] = list(e.ensure_schedule(tune=False, verbose=False))[:1]
    dev = engines["f16"].device
    imgs = torch.from_numpy(W.synth_images(n, a.size, seed=1)).to(dev)
    rng = np.random.default_rng(0)
    boxes = np.zeros((n, LC.MAX_BOXES, 5), dtype=np.float32)
    for i in range(n):
        m = LC.MAX_BOXES if i % 8 == 0 else int(rng.integers(1, 60))
        boxes[i, :m] = LC._random_boxes(rng, m, hw, ncls)
    boxes_dev = torch.from_numpy(boxes).to(dev)

    def overrun():
        sys.stderr.write(f"a timed call ran longer than {a.limit} s\n")
        sys.stderr.flush()
        os._exit(124)

    def once(fn):
        watchdog = threading.Timer(a.limit, overrun)
        watchdog.daemon = True
        watchdog.start()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        watchdog.cancel()
        return t0.elapsed_time(t1)

    def alternating(fns, reps):
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                ms[k].append(once(fn))
        return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}

    work = {}
    for name, e in engines.items():
        work[name] = dict(hs=e.head_state(flat), bs=e.block_state(flat),
                          dw=torch.empty((e.head_floats(),), dtype=torch.float32, device=dev),
                          dk=torch.empty((e.block_floats(),), dtype=torch.float32, device=dev),
                          word=torch.zeros((1,), dtype=torch.int32, device=dev))
        e.forward_device(imgs)
        work[name]["labels"] = e.assign_device(boxes_dev)

    def block_grad(name, labels):
        e, w = engines[name], work[name]
        if name == "f16":
            w["word"].zero_()
            e.block_grad_device(n, records=labels, dk=w["dk"], loss_scale=a.loss_scale, overflow=w["word"])
        else:
            e.block_grad_device(n, records=labels, dk=w["dk"])

    def step(name):
        e, w = engines[name], work[name]
        e.forward_device(imgs)
        t = e.assign_device(boxes_dev)
        e.loss_device(n, records=t)
        e.head_grad_device(n, records=t, dw=w["dw"])
        block_grad(name, t)
        e.head_adam_step(w["hs"], w["dw"])
        e.block_adam_step(w["bs"], w["dk"])
    grads = alternating({k: (lambda k=k: block_grad(k, work[k]["labels"])) for k in engines}, a.reps)
    word_after_grad = int(work["f16"]["word"].cpu()[0])

    # the gradient call by kernel, from the profiler's kernel records (left out when the profiler sees no kernels of ours)
    split = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for name in ("f16", "bf16_a"):
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                for _ in range(5):
                    block_grad(name, work[name]["labels"])
                torch.cuda.synchronize()
            found = {"block_dgrad": [], "block_wgrad_kernel": [], "block_wgrad_finish": []}
            for ev in prof.events():
                for key in found:
                    if key in ev.name:
                        found[key].append(float(getattr(ev, "device_time", getattr(ev, "cuda_time", 0.0))) / 1e3)
            if len(found["block_wgrad_kernel"]) == 15 and len(found["block_dgrad"]) == 5:
                split[name] = {"head_dgrad_ms": float(np.median(found["block_dgrad"])),
                               "wgrad_ms_conv92_100_108": [float(x) for x in np.median(np.array(found["block_wgrad_kernel"]).reshape(5, 3), axis=0)],
                               "finish_ms_total": float(np.median(np.array(found["block_wgrad_finish"]).reshape(5, 3).sum(axis=1)))}
    except Exception as ex:                                                  # the split is an extra; the totals stand
        split = {"unavailable": repr(ex)}
    steps = alternating({k: (lambda k=k: step(k)) for k in engines}, a.reps)
    fwd = alternating({k: (lambda e=e: e.forward_device(imgs)) for k, e in engines.items()}, a.reps)

    def rel(x, y):
        return (x - y) / y
    doc = {"shape": {"size": a.size, "classes": ncls, "batch": n, "max_boxes": LC.MAX_BOXES, "loss_scale": a.loss_scale, "schedules": schedules},
           "ms_median_min_max": {"head_blocks_step": steps, "block_grad": grads, "forward": fwd},
           "f16_vs_bf16_a": {"head_blocks_step": rel(steps["f16"][0], steps["bf16_a"][0]), "block_grad": rel(grads["f16"][0], grads["bf16_a"][0])},
           "bf16_b_vs_bf16_a_spread": {"head_blocks_step": rel(steps["bf16_b"][0], steps["bf16_a"][0]),
                                       "block_grad": rel(grads["bf16_b"][0], grads["bf16_a"][0])},
           "block_grad_split": split,
           "overflow_word_after_block_grad": word_after_grad,
           "overflow_word_note": "the timed steps apply Adam at the default rate to synthetic weights; only the word of the gradient "
                                 "calls on the loaded weights is reported",
           "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
