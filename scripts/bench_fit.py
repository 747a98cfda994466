#!/usr/bin/env python3
"""What a head fine-tuning step costs on the device: forward / y4_loss_assign + y4_loss + y4_head_grad / y4_head_adam (with the
re-pack), the forward with the head convs' inputs retained against the plain one (two engines, alternating), and the same
gradient + update written in torch ops on the device (autograd through scripts/bench_loss.py's torch restatement of the loss
over heads = X W^T + b, `matmul` for dW, torch.optim.Adam): the thing the kernels replace.  Default: 608^2, 80 classes, batch 32,
bf16 compute, shipped schedule.  Writes profiles/fit/bench_fit.json.

  python scripts/bench_fit.py [--size 608] [--classes 80] [--batch 32] [--dtype bf16] [--reps 30] [--box-loss giou|ciou] [--out PATH]

Timing: hip events around one call, 5 warm-up calls, the median of --reps; the shader clock read afterwards is noted."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--box-loss", default="giou", choices=("giou", "ciou"), help="the box term the engine evaluates and differentiates")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit", "bench_fit.json"))
    a = ap.parse_args()
    import torch
    import loss_cases as LC
    from bench_loss import torch_loss
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.data import preprocess_true_boxes
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    hw, n, ncls = (a.size, a.size), a.batch, a.classes
    cfg = make_config(a.size)
    flat = W.flatten(W.synth_weights(build_plan(hw, ncls), seed=1))
    engines = {}
    for key, retain in (("plain", False), ("retain", True)):
        e = engines[key] = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0", alias_workspace=True,
                                  retain_head_inputs=retain, box_loss=a.box_loss)
        e.load_weight_blob(flat)
        schedule = e.ensure_schedule(tune=False, verbose=False)
    eng = engines["retain"]
    imgs = torch.from_numpy(W.synth_images(n, a.size, seed=1)).to(eng.device)
    rng = np.random.default_rng(0)
    boxes = np.zeros((n, LC.MAX_BOXES, 5), dtype=np.float32)
    for i in range(n):                                           # 1 .. 100 boxes per image, some images full
        m = LC.MAX_BOXES if i % 8 == 0 else int(rng.integers(1, 60))
        boxes[i, :m] = LC._random_boxes(rng, m, hw, ncls)
    boxes_dev = torch.from_numpy(boxes).to(eng.device)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        return stats([once(fn) for _ in range(reps)])

    # the forward, retention off against on: alternating on the same box
    for e in engines.values():
        for _ in range(5):
            e.forward_device(imgs)
    torch.cuda.synchronize()
    fwd = {"plain": [], "retain": []}
    for _ in range(a.reps):
        for key, e in engines.items():
            fwd[key].append(once(lambda: e.forward_device(imgs)))
    fwd = {k: stats(v) for k, v in fwd.items()}

    eng.forward_device(imgs)
    state = eng.head_state(flat)
    dw = torch.empty((eng.head_floats(),), dtype=torch.float32, device=eng.device)
    triple = eng.assign_device(boxes_dev)

    def loss_and_grad():
        t = eng.assign_device(boxes_dev)
        eng.loss_device(n, records=t)
        eng.head_grad_device(n, records=t, dw=dw)
    loss_grad = timed(loss_and_grad, a.reps)
    grad_only = timed(lambda: eng.head_grad_device(n, records=triple, dw=dw), a.reps)
    adam = timed(lambda: eng.head_adam_step(state, dw), a.reps)
    eng.load_weight_blob(flat)                                   # (the timed Adam steps moved the packed heads)
    eng.forward_device(imgs)
    kernel_dw = eng.head_grad_device(n, records=triple).clone()

    # ---- the same in torch ops: autograd gives the dense gradient w.r.t. the heads, matmul with X (read back once, as float32,
    # from a non-aliased engine) makes dW, torch.optim.Adam steps float32 parameters
    y_true, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    labels_dev = [torch.from_numpy(y).to(eng.device) for y in y_true]
    xywh_dev = torch.from_numpy(xywh).to(eng.device)
    anchors = torch.tensor(LC.ANCHORS.reshape(3, 3, 2).astype(np.float32), device=eng.device)
    thr, area = float(cfg["iou_loss_thresh"]), float(hw[0] * hw[1])
    lt = eng.layer_table()
    tap = Engine(ncls, cfg, max_batch=n, dtype=a.dtype, device="cuda:0")
    tap.load_weight_blob(flat)
    tap.forward_device(imgs)
    X = [torch.from_numpy(tap.conv_output(c, n)).to(eng.device).reshape(-1, lt[c]["cout"]) for c in (92, 100, 108)]
    tap.close()
    params = []
    for i in eng.HEAD_CONVS:
        o, cout, cin = lt[i]["weight_offset"], lt[i]["cout"], lt[i]["cin"]
        params.append(torch.from_numpy(flat[o:o + cout].copy()).to(eng.device).requires_grad_())
        params.append(torch.from_numpy(flat[o + cout:o + cout * (1 + cin)].reshape(cout, cin).copy()).to(eng.device).requires_grad_())
    opt = torch.optim.Adam(params, lr=1e-4, eps=1e-7)
    wsum = torch.tensor([3.54, 64.3, 1.0], device=eng.device)

    def torch_grad():
        heads = [h.requires_grad_() for h in eng.heads_device(n)]
        terms = torch_loss(heads, labels_dev, xywh_dev, anchors, LC.STRIDES, ncls, thr, area)
        ((terms.sum(1) * wsum).sum(1).mean()).backward()
        for s in range(3):
            g = heads[s].grad.reshape(-1, heads[s].shape[-1])
            params[2 * s].grad = g.sum(0)
            params[2 * s + 1].grad = g.t() @ X[s]

    def torch_step():
        torch_grad()
        opt.step()
    torch_grad()
    base_dw = torch.cat([p.grad.reshape(-1) for p in params])
    rel = float((kernel_dw - base_dw).abs().max() / base_dw.abs().max())
    base = timed(torch_step, max(5, a.reps // 3))

    x_bytes = sum(int(x.numel()) for x in X) * (4 if a.dtype == "f32" else 2)
    clock = None
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        clock = [l.strip() for l in smi.splitlines() if "sclk" in l][:1]
    except Exception:
        pass
    step = fwd["retain"][0] + loss_grad[0] + adam[0]
    doc = {"shape": {"size": a.size, "classes": ncls, "batch": n, "dtype": a.dtype, "max_boxes": LC.MAX_BOXES, "box_loss": a.box_loss,
                     "schedule": list(schedule)[:1]},
           "ms_median_min_max": {"forward_retain_off": fwd["plain"], "forward_retain_on": fwd["retain"],
                                 "assign_plus_loss_plus_head_grad": loss_grad, "head_grad_alone": grad_only,
                                 "adam_plus_repack": adam, "torch_baseline_grad_plus_adam": base},
           "training_step_ms": step,
           "grad_plus_update_share_of_forward": (loss_grad[0] + adam[0]) / fwd["retain"][0],
           "retention_cost_ms": fwd["retain"][0] - fwd["plain"][0],
           "speedup_over_torch_baseline": base[0] / (loss_grad[0] + adam[0]),
           "head_input_bytes": x_bytes, "achieved_GBps_head_grad_on_head_inputs": x_bytes / (grad_only[0] * 1e-3) / 1e9,
           "act_bytes": {k: e.act_bytes for k, e in engines.items()},
           "max_diff_kernel_vs_torch_dw_rel_to_max": rel if a.box_loss == "giou" else None,      # (the torch baseline is the GIoU formula)
           "reps": a.reps, "sclk_after": clock}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
