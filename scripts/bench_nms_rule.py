#!/usr/bin/env python3
"""What the NMS pair rule (y4_set_nms_rule) costs: the `nms` op time of y4_profile on the bench input -- 608^2, 80 classes, batch 32,
bf16, synthetic weights and images of seed 0, the schedule that ships for the shape -- for the parent commit's build, for this
build with the default rule, and for 'diou' at beta 1 and 0.6 and the agnostic rule.  Writes profiles/decode_paths/bench_nms_rule.json.

  python scripts/bench_nms_rule.py --parent-tree DIR [--reps 20] [--runs 2] [--out PATH]

DIR is a built checkout of the parent commit (its own yolo4hip package and library; it has no y4_set_nms_rule).  Every measurement
is a process of its own, one after the other: parent and this build's default rule alternate `--runs` times, then `--runs` runs of
each other rule.  A run is 5 warm-up y4_profile calls and the median / min / max of `--reps` more.  The default rule passes when its
medians lie inside [min, max] of the parent's own medians of the same session; the other rules are recorded, not judged.  The
comparison is made on nanoseconds: y4_profile hands out float32 milliseconds of an event timer that ticks at 40 ns, and the same
tick count comes back with different last float32 bits (some 4e-9 ms at these values).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {"iou": ("iou", 1.0, False), "diou_beta1": ("diou", 1.0, False), "diou_beta06": ("diou", 0.6, False),
         "agnostic_iou": ("iou", 1.0, True), "agnostic_diou_beta06": ("diou", 0.6, True)}


def child(a):
    sys.path.insert(0, os.path.join(a.tree, "yolo-v4-tf.keras_amd"))
    import numpy as np
    import torch
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(a.size)
    eng = Engine(a.classes, cfg, max_batch=a.batch, dtype=a.dtype, device="cuda:0", alias_workspace=True)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(a.size, a.classes), seed=0)))
    schedule = eng.ensure_schedule(tune=False, verbose=False)
    if a.rule != "parent":
        eng.set_nms_rule(*RULES[a.rule])
    imgs = torch.from_numpy(W.synth_images(a.batch, a.size, seed=0)).to(eng.device)
    outs = eng.predict(imgs)
    for _ in range(5):
        eng.profile(imgs)
    ms = [dict(eng.profile(imgs))["nms"] for _ in range(a.reps)]
    print(json.dumps({"rule": a.rule, "nms_ms_median_min_max": [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))],
                      "valid_total": int(outs[3].sum()), "schedule": list(schedule)[:1]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_paths", "bench_nms_rule.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--rule", default="iou", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR: a built checkout of the parent commit")

    def run(tree, rule):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--rule", rule, "--size", str(a.size),
               "--classes", str(a.classes), "--batch", str(a.batch), "--dtype", a.dtype, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                      # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{rule} on {tree}: exit {r.returncode}")
        doc = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(doc), flush=True)
        return doc
    runs = {}
    for k in range(a.runs):
        runs[f"parent_run{k + 1}"] = run(os.path.abspath(a.parent_tree), "parent")
        runs[f"new_iou_run{k + 1}"] = run(ROOT, "iou")
    for rule in list(RULES)[1:]:
        for k in range(a.runs):
            runs[f"new_{rule}_run{k + 1}"] = run(ROOT, rule)
    med = lambda prefix: [v["nms_ms_median_min_max"][0] for k, v in runs.items() if k.startswith(prefix)]      # noqa: E731
    parent, iou = med("parent_run"), med("new_iou_run")
    ns = lambda ms: round(ms * 1e6)                # noqa: E731
    verdict = {"parent_medians": parent, "parent_vs_parent_spread": max(parent) - min(parent), "iou_medians": iou,
               "iou_within_parent_spread": all(ns(min(parent)) <= ns(m) <= ns(max(parent)) for m in iou),
               "iou_minus_largest_parent_median": [m - max(parent) for m in iou],
               "iou_minus_parent_mid": [m - 0.5 * (min(parent) + max(parent)) for m in iou]}
    for rule in list(RULES)[1:]:
        verdict[f"{rule}_medians"] = med(f"new_{rule}_run")
    doc = {"what": f"the nms op of y4_profile in ms, {a.size}^2, {a.classes} classes, batch {a.batch}, {a.dtype}, bench input; one process "
                   f"per run, 5 warm-up calls, median / min / max of {a.reps}; parent and this build alternating, one MI355X, one session",
           "runs": runs, "verdict": verdict}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(verdict))


if __name__ == "__main__":
    main()
