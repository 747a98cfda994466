#!/usr/bin/env python3
"""What decode and NMS cost under every NMS pair rule (y4_set_nms_rule), in this tree and in a built checkout of the parent commit:
the `decode` and `nms` op times of y4_profile on the bench input -- 608^2, 80 classes, batch 32, bf16, synthetic weights and images
of seed 0, the schedule that ships for the shape -- for 'iou', 'diou' at beta 1 and 0.6, and the agnostic forms of the first and
the last.  Writes profiles/decode_paths/bench_nms_rule.json.

  python scripts/bench_nms_rule.py --parent-tree DIR [--classes 80] [--reps 20] [--runs 2] [--out PATH]

DIR is a built checkout of the parent commit (its own yolo4hip package and library).  A run is one process that measures every
rule in turn: per rule 5 warm-up y4_profile calls and the median / min / max of `--reps` more.  Parent and this tree alternate
`--runs` times.  A figure passes when every median of this tree lies within the span of the parent's medians of the same session,
widened on each side by that span; a figure outside is reported with its distance, not run again.  The comparison is made on
nanoseconds: y4_profile hands out float32 milliseconds of an event timer that ticks at 40 ns, and the same tick count comes back
with different last float32 bits (some 4e-9 ms at these values).  --classes 81 is the smallest count that takes the generic
decode_kernel instead of the cell kernels.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {"iou": ("iou", 1.0, False), "diou_beta1": ("diou", 1.0, False), "diou_beta06": ("diou", 0.6, False),
         "agnostic_iou": ("iou", 1.0, True), "agnostic_diou_beta06": ("diou", 0.6, True)}
OPS = ("decode", "nms")


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
    imgs = torch.from_numpy(W.synth_images(a.batch, a.size, seed=0)).to(eng.device)
    doc = {"tree": a.tree, "schedule": list(schedule)[:1], "rules": {}}
    for rule in a.rules.split(","):
        eng.set_nms_rule(*RULES[rule])
        outs = eng.predict(imgs)
        for _ in range(5):
            eng.profile(imgs)
        ms = [dict(eng.profile(imgs)) for _ in range(a.reps)]
        doc["rules"][rule] = {"valid_total": int(outs[3].sum())}
        for op in OPS:
            t = [m[op] for m in ms]
            doc["rules"][rule][f"{op}_ms_median_min_max"] = [float(np.median(t)), float(np.min(t)), float(np.max(t))]
    print(json.dumps(doc))


def judge(parent, new):
    """The span rule on medians in ms -> dict."""
    ns = lambda ms: round(ms * 1e6)                # noqa: E731
    lo, hi = ns(min(parent)), ns(max(parent))
    span = hi - lo
    dist = [ns(m) - (hi + span) if ns(m) > hi + span else min(ns(m) - (lo - span), 0) for m in new]      # > 0 slower, < 0 faster
    return {"parent_medians_ms": parent, "new_medians_ms": new, "allowed_ms": [(lo - span) / 1e6, (hi + span) / 1e6],
            "passes": all(d == 0 for d in dist), "outside_by_ns": dist}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--classes", type=int, default=80)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--rules", default=",".join(RULES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_paths", "bench_nms_rule.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR: a built checkout of the parent commit")

    def run(tree):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--rules", a.rules, "--size", str(a.size),
               "--classes", str(a.classes), "--batch", str(a.batch), "--dtype", a.dtype, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                      # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{tree}: exit {r.returncode}")
        doc = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(doc), flush=True)
        return doc
    runs = {}
    for k in range(a.runs):
        runs[f"parent_run{k + 1}"] = run(os.path.abspath(a.parent_tree))
        runs[f"new_run{k + 1}"] = run(ROOT)
    verdict = {}
    for rule in a.rules.split(","):
        for op in OPS:
            med = lambda prefix: [v["rules"][rule][f"{op}_ms_median_min_max"][0] for k, v in runs.items() if k.startswith(prefix)]  # noqa: E731
            verdict[f"{rule}/{op}"] = judge(med("parent_run"), med("new_run"))
        valid = {v["rules"][rule]["valid_total"] for v in runs.values()}
        verdict[f"{rule}/same_valid_total"] = len(valid) == 1
    doc = {"what": f"the decode and nms ops of y4_profile in ms, {a.size}^2, {a.classes} classes, batch {a.batch}, {a.dtype}, bench input; "
                   f"one process per run measuring every rule, 5 warm-up calls, median / min / max of {a.reps}; parent and this tree "
                   f"alternating, one MI355X, one session",
           "runs": runs, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(verdict))


if __name__ == "__main__":
    main()
