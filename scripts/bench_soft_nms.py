#!/usr/bin/env python3
"""What Soft-NMS (y4_set_nms_soft) costs, and that switching it off costs nothing: the `nms` op of y4_profile on the bench input --
608^2, 80 classes, batch 32, bf16, synthetic weights and images of seed 0, the schedule that ships for the shape.

  python scripts/bench_soft_nms.py --parent-tree DIR [--reps 20] [--runs 2] [--out PATH]

DIR is a built checkout of the parent commit (its own yolo4hip package and library).

  off     parent and this tree alternate `--runs` times, one process per run, 5 warm-up y4_profile calls and the median / min / max
          of `--reps` more, mode off.  This tree passes when each of its medians lies within the span of the parent's medians of
          the same session, widened on each side by that span (the rule of scripts/bench_nms_rule.py, on nanoseconds).
  soft    in this tree's runs, the same measurement under gaussian / linear / hard, class-aware and agnostic, each beside the
          hard kernel under the same pair rule: the multiple is the soft median over that.  Nothing to compare these with.
  tiled   in this tree's first run, y4_nms_gathered by HIP events on the 2432 x 1824 photo of scripts/bench_tiled.py (21 rows, one
          group, 608^2, 80 classes, bf16, weights of seed 1) under the same modes.

One session on one machine; nothing beyond that is claimed.  Writes profiles/soft_nms/bench_soft_nms.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(m, agn) for agn in (False, True) for m in (None, "gaussian", "linear", "hard")]
PHOTO_HW, OVERLAP = (1824, 2432), 0.2


def name_of(method, agn):
    return f"{method or 'off'}{'_agnostic' if agn else ''}"


def med3(t):
    import numpy as np
    return [float(np.median(t)), float(np.min(t)), float(np.max(t))]


def child(a):
    sys.path.insert(0, os.path.join(a.tree, "yolo-v4-tf.keras_amd"))
    import numpy as np
    import torch
    from yolo4hip import tiling, weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(a.size)
    eng = Engine(a.classes, cfg, max_batch=a.batch, dtype=a.dtype, device="cuda:0", alias_workspace=True)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(a.size, a.classes), seed=0)))
    schedule = eng.ensure_schedule(tune=False, verbose=False)
    imgs = torch.from_numpy(W.synth_images(a.batch, a.size, seed=0)).to(eng.device)
    doc = {"tree": "this tree" if os.path.abspath(a.tree) == ROOT else "parent", "schedule": list(schedule)[:1], "modes": {}}
    soft = hasattr(eng, "set_nms_soft")
    for method, agn in MODES:
        if method is not None and not (soft and a.soft):
            continue
        if agn and not a.soft:
            continue
        eng.set_nms_rule("iou", agnostic=agn)
        if soft:
            eng.set_nms_soft(method)
        outs = eng.predict(imgs)
        for _ in range(5):
            eng.profile(imgs)
        t = [dict(eng.profile(imgs))["nms"] for _ in range(a.reps)]
        doc["modes"][name_of(method, agn)] = {"valid_total": int(outs[3].sum()), "nms_ms_median_min_max": med3(t)}
    if soft and a.tiled:
        eng.close()
        eng = Engine(a.classes, cfg, max_batch=a.batch, dtype=a.dtype, device="cuda:0")
        eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(a.size, a.classes), seed=1)))
        eng.ensure_schedule(tune=False, verbose=False)
        photo = np.random.default_rng(0).integers(0, 256, PHOTO_HW + (3,), dtype=np.uint8)
        rows = tiling.tile_rows(PHOTO_HW[0], PHOTO_HW[1], (a.size, a.size), None, OVERLAP, True, False)
        R = len(rows)
        tiles = [np.ascontiguousarray(photo[y0:y0 + wh, x0:x0 + ww]) for (y0, x0, wh, ww), _, _ in rows]
        batch = eng.preprocess_u8_batch(tiles)[0]
        dev = eng.device
        eng.predict(batch)                             # (leaves the rows' heads in the workspace: decode_gather reads them)
        group = torch.zeros(R, dtype=torch.int32, device=dev)
        slot = torch.arange(R, dtype=torch.int32, device=dev)
        maps = torch.from_numpy(np.stack([m for _, _, m in rows]).astype(np.float32)).to(dev)
        cap = 1 << 18
        outs = eng.alloc_outputs(1)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        doc["tiled"] = {"rows": R}
        for method, agn in MODES:
            eng.set_nms_rule("iou", agnostic=agn)
            eng.set_nms_soft(method)
            t = []
            for i in range(3 + a.reps):
                state = eng.gather_begin(1, R, cap)
                eng.decode_gather(state, R, group, slot, maps)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); eng.nms_gathered(state, outs, cnt); e1.record()
                e1.synchronize()
                if i >= 3:
                    t.append(e0.elapsed_time(e1))
            doc["tiled"][name_of(method, agn)] = {"candidates": int(cnt.cpu()[0]), "valid": int(outs[3].cpu()[0]),
                                                  "nms_gathered_ms_median_min_max": med3(t)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_nms", "bench_soft_nms.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--soft", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--tiled", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR: a built checkout of the parent commit")

    def run(tree, soft, tiled):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--size", str(a.size), "--classes", str(a.classes),
               "--batch", str(a.batch), "--dtype", a.dtype, "--reps", str(a.reps), "--soft", str(int(soft)), "--tiled", str(int(tiled))]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                      # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{tree}: exit {r.returncode}")
        doc = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(doc), flush=True)
        return doc
    runs = {}
    for k in range(a.runs):
        runs[f"parent_run{k + 1}"] = run(os.path.abspath(a.parent_tree), False, False)
        runs[f"new_run{k + 1}"] = run(ROOT, True, k == 0)
    med = lambda prefix, mode: [v["modes"][mode]["nms_ms_median_min_max"][0] for k, v in runs.items() if k.startswith(prefix)]  # noqa: E731
    verdict = {"off/nms": judge(med("parent_run", "off"), med("new_run", "off")),
               "off/same_valid_total": len({v["modes"]["off"]["valid_total"] for v in runs.values()}) == 1}
    multiples = {}
    for method, agn in MODES:
        if method is None:
            continue
        base = med("new_run", name_of(None, agn))
        multiples[name_of(method, agn)] = [round(s / b, 2) for s, b in zip(med("new_run", name_of(method, agn)), base)]
    tiled = runs["new_run1"].get("tiled", {})
    tiled_multiples = {}
    for method, agn in MODES:
        if method is not None and name_of(method, agn) in tiled:
            tiled_multiples[name_of(method, agn)] = round(tiled[name_of(method, agn)]["nms_gathered_ms_median_min_max"][0] /
                                                          tiled[name_of(None, agn)]["nms_gathered_ms_median_min_max"][0], 2)
    doc = {"what": f"the nms op of y4_profile in ms, {a.size}^2, {a.classes} classes, batch {a.batch}, {a.dtype}, bench input; one process "
                   f"per run, 5 warm-up calls, median / min / max of {a.reps}; parent and this tree alternating, one MI355X, one session",
           "runs": runs, "verdict": verdict, "soft_over_hard_kernel": multiples, "tiled_soft_over_hard_kernel": tiled_multiples}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"verdict": verdict, "soft_over_hard_kernel": multiples, "tiled_soft_over_hard_kernel": tiled_multiples}))


if __name__ == "__main__":
    main()
