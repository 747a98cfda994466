#!/usr/bin/env python3
"""What Matrix-NMS (y4_set_nms_matrix) costs, and that switching it off costs nothing: the `nms` op of y4_profile on the bench input
-- 608^2, 80 classes, batch 32, bf16, synthetic weights and images of seed 0, the schedule that ships for the shape.

  python scripts/bench_matrix_nms.py --parent-tree DIR [--reps 20] [--runs 2] [--out PATH]

DIR is a built checkout of the parent commit (its own yolo4hip package and library).

  off     parent and this tree alternate `--runs` times, one process per run, 5 warm-up y4_profile calls and the median / min / max
          of `--reps` more, both decay modes off.  This tree passes when each of its medians lies within the span of the parent's
          medians of the same session, widened on each side by that span (the rule of scripts/bench_soft_nms.py, on nanoseconds).
  on      in this tree's runs, the same measurement under Matrix-NMS gaussian / linear, class-aware and agnostic, beside the hard
          kernel under the same pair rule and beside this build's Soft-NMS gaussian on the same lists.
  tiled   in this tree's first run, y4_nms_gathered by HIP events on the 2432 x 1824 photo of scripts/bench_tiled.py (21 rows, one
          group, 608^2, 80 classes, bf16, weights of seed 1) under the same modes.
  worst   in this tree's first run, one list of 4096 participants that all interact (soft_nms_cases.edge_case(4096) under an
          agnostic rule at 160^2, 80 classes): decode + NMS by HIP events, against the hard kernel on the same list.  A price, not a gate.

One session on one machine; nothing beyond that is claimed.  Writes profiles/matrix_nms/bench_matrix_nms.json."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (decay family, method): the hard kernel, Matrix-NMS, and Soft-NMS gaussian to set it beside
MODES = [(agn, fam, m) for agn in (False, True) for fam, m in ((None, None), ("matrix", "gaussian"), ("matrix", "linear"), ("soft", "gaussian"))]
PHOTO_HW, OVERLAP = (1824, 2432), 0.2


def name_of(agn, fam, method):
    return f"{'off' if fam is None else fam + '_' + method}{'_agnostic' if agn else ''}"


def med3(t):
    import numpy as np
    return [float(np.median(t)), float(np.min(t)), float(np.max(t))]


def set_mode(eng, agn, fam, method):
    eng.set_nms_rule("iou", agnostic=agn)
    if hasattr(eng, "set_nms_matrix"):
        eng.set_nms_matrix(None)
    eng.set_nms_soft(None)
    if fam == "matrix":
        eng.set_nms_matrix(method)
    elif fam == "soft":
        eng.set_nms_soft(method)


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
    for agn, fam, method in MODES:
        if not a.on and (fam is not None or agn):
            continue
        set_mode(eng, agn, fam, method)
        outs = eng.predict(imgs)
        for _ in range(5):
            eng.profile(imgs)
        t = [dict(eng.profile(imgs))["nms"] for _ in range(a.reps)]
        doc["modes"][name_of(agn, fam, method)] = {"valid_total": int(outs[3].sum()), "nms_ms_median_min_max": med3(t)}
    if a.on and a.extra:
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
        for agn, fam, method in MODES:
            set_mode(eng, agn, fam, method)
            t = []
            for i in range(3 + a.reps):
                state = eng.gather_begin(1, R, cap)
                eng.decode_gather(state, R, group, slot, maps)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); eng.nms_gathered(state, outs, cnt); e1.record()
                e1.synchronize()
                if i >= 3:
                    t.append(e0.elapsed_time(e1))
            doc["tiled"][name_of(agn, fam, method)] = {"candidates": int(cnt.cpu()[0]), "valid": int(outs[3].cpu()[0]),
                                                       "nms_gathered_ms_median_min_max": med3(t)}
        eng.close()
        # ---- the worst case: 4096 participants of one segment
        sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
        import soft_nms_cases as SC
        heads = SC.edge_case(4096)[0]
        eng = Engine(SC.NCLS_LEN, make_config(SC.SIZE_LEN), max_batch=1, dtype="bf16", device="cuda:0")
        eng.adopt_packed()                             # (decode and NMS read no weights)
        n = eng.set_heads(heads)
        doc["worst"] = {"participants": 4096}
        for fam, method in ((None, None), ("matrix", "gaussian"), ("matrix", "linear"), ("soft", "gaussian")):
            set_mode(eng, True, fam, method)
            t = []
            for i in range(3 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); outs = eng.decode_nms_device(n, None); e1.record()
                e1.synchronize()
                if i >= 3:
                    t.append(e0.elapsed_time(e1))
            doc["worst"][name_of(True, fam, method)] = {"valid": int(outs[3].cpu()[0]), "decode_nms_ms_median_min_max": med3(t)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_nms", "bench_matrix_nms.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--on", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--extra", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR: a built checkout of the parent commit")

    def run(tree, on, extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--size", str(a.size), "--classes", str(a.classes),
               "--batch", str(a.batch), "--dtype", a.dtype, "--reps", str(a.reps), "--on", str(int(on)), "--extra", str(int(extra))]
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
    over_hard, over_soft = {}, {}
    for agn, fam, method in MODES:
        if fam is None:
            continue
        mine = med("new_run", name_of(agn, fam, method))
        over_hard[name_of(agn, fam, method)] = [round(s / b, 2) for s, b in zip(mine, med("new_run", name_of(agn, None, None)))]
        if fam == "matrix":
            over_soft[name_of(agn, fam, method)] = [round(s / b, 2) for s, b in zip(mine, med("new_run", name_of(agn, "soft", "gaussian")))]
    extra = runs["new_run1"]
    tiled = {k: v["nms_gathered_ms_median_min_max"][0] for k, v in extra.get("tiled", {}).items() if isinstance(v, dict)}
    worst = {k: v["decode_nms_ms_median_min_max"][0] for k, v in extra.get("worst", {}).items() if isinstance(v, dict)}
    doc = {"what": f"the nms op of y4_profile in ms, {a.size}^2, {a.classes} classes, batch {a.batch}, {a.dtype}, bench input; one process "
                   f"per run, 5 warm-up calls, median / min / max of {a.reps}; parent and this tree alternating, one MI355X, one session",
           "runs": runs, "verdict": verdict, "over_hard_kernel": over_hard, "matrix_over_soft_gaussian": over_soft,
           "tiled_nms_gathered_ms": tiled, "worst_case_decode_nms_ms": worst}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: doc[k] for k in ("verdict", "over_hard_kernel", "matrix_over_soft_gaussian", "tiled_nms_gathered_ms",
                                           "worst_case_decode_nms_ms")}))


if __name__ == "__main__":
    main()
