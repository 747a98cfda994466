#!/usr/bin/env python3
"""What a fit(trainable='head_blocks') step costs on the device, beside the 'heads' step of the same build and the same backward
written in torch ops.  Default: 608^2, 80 classes, batch 32, bf16 compute, shipped schedule.  Writes
profiles/fit/bench_fit_blocks.json.

  (a) the 'head_blocks' step: forward (retention level 2) / labels + loss + y4_head_grad / y4_block_grad / both Adam steps with
      their re-packs; y4_block_grad split into head dgrad, the wgrad of conv 92 / 100 / 108 and the finish kernels from the
      kernel durations torch.profiler records (left out when the profiler sees no kernels of ours)
  (b) the 'heads' step (retention level 1) of the same build, beside the 5.97 ms recorded in profiles/fit/bench_fit.json
  (c) the same backward in torch ops on the device: autograd through conv2d (MIOpen's weight gradient), the frozen-BN affine,
      leaky_relu and the 1x1 head conv from the dense head gradient y4_loss_grad gives, then torch.optim.Adam on the three kernels
  (d) the forward at retention level 0 / 1 / 2, alternating

  python scripts/bench_fit_blocks.py [--size 608] [--classes 80] [--batch 32] [--dtype bf16] [--reps 20] [--out PATH]

One process; hip events around one call, 5 warm-up calls, the median of --reps, variants that are compared measured alternately.
Every timed step runs under its own time limit (--limit seconds): a watchdog thread ends the process with os._exit(124) when a
step has not returned by then, also while the main thread waits inside the driver, where no Python signal handler would run."""
import argparse
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

HEADS_STEP_RECORDED_MS = 5.97          # profiles/fit/bench_fit.json of the commit that introduced fit(trainable='heads')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit", "bench_fit_blocks.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import loss_cases as LC
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    hw, n, ncls = (a.size, a.size), a.batch, a.classes
    cfg = make_config(a.size)
    flat = W.flatten(W.synth_weights(build_plan(hw, ncls), seed=1))
    engines = {}
    for level in (0, 1, 2):
        e = engines[level] = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0", alias_workspace=True, retain_head_inputs=level)
        e.load_weight_blob(flat)
        schedule = e.ensure_schedule(tune=False, verbose=False)
    e1, e2 = engines[1], engines[2]
    dev = e2.device
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

    # (d) the forward per retention level
    fwd = alternating({f"level{lv}": (lambda e=e: e.forward_device(imgs)) for lv, e in engines.items()}, a.reps)

    # (a) / (b): the pieces of both steps, on the heads each engine's forward left
    st1, st2, bst = e1.head_state(flat), e2.head_state(flat), e2.block_state(flat)
    dw1 = torch.empty((e1.head_floats(),), dtype=torch.float32, device=dev)
    dw2 = torch.empty_like(dw1)
    dk = torch.empty((e2.block_floats(),), dtype=torch.float32, device=dev)
    tr1, tr2 = e1.assign_device(boxes_dev), e2.assign_device(boxes_dev)

    def head_part(e, dw):
        t = e.assign_device(boxes_dev)
        e.loss_device(n, records=t)
        e.head_grad_device(n, records=t, dw=dw)
    e2.block_grad_device(n, records=tr2, dk=dk)                              # allocates the scratch once
    parts = alternating({"heads_assign_loss_head_grad_level1": lambda: head_part(e1, dw1),
                         "heads_assign_loss_head_grad_level2": lambda: head_part(e2, dw2),
                         "block_grad": lambda: e2.block_grad_device(n, records=tr2, dk=dk)}, a.reps)
    adam = alternating({"head_adam_level1": lambda: e1.head_adam_step(st1, dw1),
                        "head_adam_level2": lambda: e2.head_adam_step(st2, dw2),
                        "block_adam_plus_repack": lambda: e2.block_adam_step(bst, dk)}, a.reps)
    for e in (e1, e2):
        e.load_weight_blob(flat)                                             # (the timed Adam steps moved the packed weights)
        e.forward_device(imgs)
    kernel_dk = e2.block_grad_device(n, records=tr2).clone()

    # the split of y4_block_grad by kernel, from the profiler's kernel records
    split = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(5):
                e2.block_grad_device(n, records=tr2, dk=dk)
            torch.cuda.synchronize()
        names = {"block_dgrad": [], "block_wgrad_kernel": [], "block_wgrad_finish": []}
        for ev in prof.events():
            for key in names:
                if key in ev.name:
                    names[key].append(float(getattr(ev, "device_time", getattr(ev, "cuda_time", 0.0))) / 1e3)
        if len(names["block_wgrad_kernel"]) == 15 and len(names["block_dgrad"]) == 5:
            wg = np.array(names["block_wgrad_kernel"]).reshape(5, 3)
            split = {"head_dgrad_ms": float(np.median(names["block_dgrad"])),
                     "wgrad_ms_conv92_100_108": [float(x) for x in np.median(wg, axis=0)],
                     "finish_ms_total": float(np.median(np.array(names["block_wgrad_finish"]).reshape(5, 3).sum(axis=1)))}
    except Exception as ex:                                                  # the split is an extra; the totals above stand
        split = {"unavailable": repr(ex)}

    # (c) the same backward in torch ops
    lt = e2.layer_table()
    tap = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0")
    tap.load_weight_blob(flat)
    tap.forward_device(imgs)
    tdt = torch.float32 if a.dtype == "f32" else torch.bfloat16
    U = [torch.from_numpy(tap.conv_output(c, n)).to(dev).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).to(tdt)
         for c in (91, 99, 107)]
    tap.close()
    g_dense = [g.permute(0, 3, 1, 2).contiguous().to(tdt) for g in e2.loss_grad_device(n, records=tr2)]
    ks, consts = [], []
    for hc, bc in zip(e2.HEAD_CONVS, e2.BLOCK_CONVS):
        o, cout, cin = lt[bc]["weight_offset"], lt[bc]["cout"], lt[bc]["cin"]
        bn = flat[o:o + 4 * cout].reshape(4, cout)
        sc = bn[1] / np.sqrt(bn[3] + np.float32(1e-3))
        k = torch.from_numpy(flat[o + 4 * cout:o + 4 * cout + cout * cin * 9].reshape(cout, cin, 3, 3).copy()).to(dev)
        ks.append(k.requires_grad_())
        ho, hcout, hcin = lt[hc]["weight_offset"], lt[hc]["cout"], lt[hc]["cin"]
        wh = torch.from_numpy(flat[ho + hcout:ho + hcout * (1 + hcin)].reshape(hcout, hcin, 1, 1).copy()).to(dev).to(tdt)
        consts.append((torch.from_numpy(sc).to(dev).view(1, -1, 1, 1).to(tdt),
                       torch.from_numpy((bn[0] - bn[2] * sc).astype(np.float32)).to(dev).view(1, -1, 1, 1).to(tdt), wh))
    opt = torch.optim.Adam(ks, lr=1e-4, eps=1e-7)

    def torch_backward():
        for s in range(3):
            sc, sh, wh = consts[s]
            z = F.conv2d(U[s], ks[s].to(tdt), padding=1)
            head = F.conv2d(F.leaky_relu(z * sc + sh, 0.1), wh)
            head.backward(gradient=g_dense[s])

    def torch_step():
        opt.zero_grad(set_to_none=True)
        torch_backward()
        opt.step()
    # ... and its backward alone, on a graph built once: what compares with y4_block_grad, which also starts from retained tensors
    graph_heads = []
    for s in range(3):
        sc, sh, wh = consts[s]
        graph_heads.append(F.conv2d(F.leaky_relu(F.conv2d(U[s], ks[s].to(tdt), padding=1) * sc + sh, 0.1), wh))

    def torch_backward_only():
        for k in ks:
            k.grad = None
        torch.autograd.backward(graph_heads, g_dense, retain_graph=True)
    opt.zero_grad(set_to_none=True)
    torch_backward()
    base_dk = torch.cat([k.grad.reshape(-1) for k in ks])
    rel = float((kernel_dk - base_dk).abs().max() / base_dk.abs().max())
    base = alternating({"torch_forward_backward_of_the_block": torch_backward, "torch_the_same_plus_adam": torch_step,
                        "torch_backward_only": torch_backward_only,
                        "block_grad": lambda: e2.block_grad_device(n, records=tr2, dk=dk)}, max(5, a.reps // 2))

    step_blocks = (fwd["level2"][0] + parts["heads_assign_loss_head_grad_level2"][0] + parts["block_grad"][0] +
                   adam["head_adam_level2"][0] + adam["block_adam_plus_repack"][0])
    step_heads = fwd["level1"][0] + parts["heads_assign_loss_head_grad_level1"][0] + adam["head_adam_level1"][0]
    doc = {"shape": {"size": a.size, "classes": ncls, "batch": n, "dtype": a.dtype, "max_boxes": LC.MAX_BOXES, "schedule": list(schedule)[:1]},
           "ms_median_min_max": {"forward": fwd, **parts, **adam, "against_torch": base},
           "block_grad_split": split,
           "head_blocks_step_ms": step_blocks, "heads_step_ms": step_heads, "heads_step_recorded_ms": HEADS_STEP_RECORDED_MS,
           "block_backward_ms": parts["block_grad"][0],
           "torch_backward_only_ms": base["torch_backward_only"][0],
           "torch_backward_ms_note": "torch_forward_backward_of_the_block includes the forward of the three convs; torch_backward_only runs on a graph built once",
           "retention_cost_ms": {"level1": fwd["level1"][0] - fwd["level0"][0], "level2": fwd["level2"][0] - fwd["level0"][0]},
           "act_bytes": {f"level{lv}": e.act_bytes for lv, e in engines.items()},
           "block_scratch_bytes": int(e2._block_scratch.numel()),
           "wgrad_partial_bytes": int(sum(-(-512 // ((lt[c]["cin"] // 64) * (lt[c]["cout"] // 64))) * 9 * lt[c]["cin"] * lt[c]["cout"] * 4
                                          for c in e2.BLOCK_CONVS)),
           "max_diff_kernel_vs_torch_dk_rel_to_max": rel, "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
