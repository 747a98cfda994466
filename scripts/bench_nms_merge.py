#!/usr/bin/env python3
"""What merge-NMS costs (y4_decode_nms_merged, y4_nms_gathered_merged) and that nothing else moved, on one MI355X in one session.
Writes profiles/nms_merge/bench_nms_merge.json.

  python scripts/bench_nms_merge.py --parent-tree DIR [--reps 20] [--runs 2] [--out PATH]

DIR is a built checkout of the parent commit (its own yolo4hip package, library and bench.py).  Parent and this tree alternate
`--runs` times; a run is one process.

  merge     (this tree) the bench input -- 608^2, 80 classes, batch 32, bf16, synthetic weights and images of seed 0, the schedule that
            ships for the shape: y4_decode_nms_mapped against y4_decode_nms_merged on the same heads, alternating, HIP events around
            each call, medians of --reps; their difference is the merge's cost (the count copy and box_merge_kernel), reported beside
            the `decode` and `nms` ops of y4_profile on the same input, with the images' candidate-list lengths.
  tiled     (this tree) the 2432 x 1824 photo of scripts/bench_tiled.py (21 rows of 608^2, one group): y4_nms_gathered against
            y4_nms_gathered_merged on the same gathered list, alternating, with the list's length.
  merge_off (both trees) the `nms` op of y4_profile with merge off, and `bench.py --gpus 1 --steps 20 --warmup 3` images/s: this
            tree's medians must lie inside the span of the parent's own runs of the same session, widened by that span on each
            side (the rule of scripts/bench_nms_rule.py); outputs_sha256 of bench.py must equal the parent's at 160^2 / 3 classes /
            batch 4 and at the headline shape.

There is no target for the merge's cost and nothing else to compare it with: the ratio to the `nms` op is stated as measured.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, NCLS, BATCH, DTYPE = 608, 80, 32, "bf16"
PHOTO_HW, OVERLAP = (1824, 2432), 0.2


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 5), "min_ms": round(ts[0], 5), "max_ms": round(ts[-1], 5)}


def child(a):
    sys.path.insert(0, os.path.join(a.tree, "yolo-v4-tf.keras_amd"))
    import numpy as np
    import torch
    from yolo4hip import ext, tiling, weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    cfg = make_config(SIZE)
    eng = Engine(NCLS, cfg, max_batch=BATCH, dtype=DTYPE, device="cuda:0", alias_workspace=True)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(SIZE, NCLS), seed=0)))
    schedule = eng.ensure_schedule(tune=False, verbose=False)
    imgs = torch.from_numpy(W.synth_images(BATCH, SIZE, seed=0)).to(eng.device)
    doc = {"schedule": list(schedule)[:1], "device": torch.cuda.get_device_name(0)}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(fa, fb):
        for _ in range(5):
            ev_time(fa); ev_time(fb)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(ev_time(fa)); tb.append(ev_time(fb))
        return ta, tb

    # ---- merge off: the ops of y4_profile
    outs = eng.predict(imgs)
    for _ in range(5):
        eng.profile(imgs)
    ms = [dict(eng.profile(imgs)) for _ in range(a.reps)]
    doc["profile"] = {op: stats([m[op] for m in ms]) for op in ("decode", "nms")}
    doc["valid_total"] = int(outs[3].sum())
    if not hasattr(eng, "set_nms_merge"):              # the parent: nothing more to measure
        print(json.dumps(doc))
        return

    # ---- the merge on the bench input (the heads of the last profile are in the workspace)
    n = BATCH
    o_plain, o_merged = eng.alloc_outputs(n), eng.alloc_outputs(n)
    ident = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * n, dtype=torch.float32, device=eng.device)

    def plain():
        eng.set_nms_merge(False)
        eng.decode_nms_device(n, o_plain, box_map=ident)

    def merged():
        eng.set_nms_merge(True)
        eng.decode_nms_device(n, o_merged, box_map=ident)
    tp, tm = alternate(plain, merged)
    eng.set_nms_merge(False)
    torch.cuda.synchronize()
    counts = eng._merge_counts(n).cpu().numpy()
    same = all(torch.equal(x, y) for x, y in zip(o_plain[1:], o_merged[1:]))
    moved = int((o_plain[0] != o_merged[0]).any(dim=2).sum())
    d = [m - p for p, m in zip(tp, tm)]
    doc["merge"] = {"y4_decode_nms_mapped": stats(tp), "y4_decode_nms_merged": stats(tm), "merged_minus_plain": stats(d),
                    "list_lengths": {"min": int(counts.min()), "median": int(np.median(counts)), "max": int(counts.max())},
                    "kept_boxes": int(o_plain[3].sum()), "boxes_moved": moved, "everything_but_boxes_identical": bool(same),
                    "ratio_to_profile_nms_median": round(stats(d)["median_ms"] / doc["profile"]["nms"]["median_ms"], 4)}

    # ---- the tiled photo: one group of 21 rows
    photo = np.random.default_rng(0).integers(0, 256, PHOTO_HW + (3,), dtype=np.uint8)
    rows = tiling.tile_rows(PHOTO_HW[0], PHOTO_HW[1], (SIZE, SIZE), None, OVERLAP, True, False)
    R = len(rows)
    wdesc = (ext.y4_window_desc * R)()
    for dsc, ((y0, x0, wh, ww), rect, _) in zip(wdesc, rows):
        dsc.offset, dsc.pitch, dsc.h, dsc.w = (y0 * PHOTO_HW[1] + x0) * 3, PHOTO_HW[1] * 3, wh, ww
        dsc.out_h, dsc.out_w, dsc.pad_top, dsc.pad_left = rect
    dev = eng.device
    src = torch.from_numpy(photo.reshape(-1)).to(dev)
    wd = torch.from_numpy(np.frombuffer(wdesc, dtype=np.uint8).copy()).to(dev)
    canvas = torch.empty((R, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    eng.window_u8_ragged(src, wd, R, canvas)
    eng.forward_device(canvas)
    group = torch.zeros(R, dtype=torch.int32, device=dev)
    slot = torch.arange(R, dtype=torch.int32, device=dev)
    maps = torch.from_numpy(np.stack([m for _, _, m in rows])).to(dev)
    cap = 1 << 18
    state = eng.gather_begin(1, R, cap)
    eng.decode_gather(state, R, group, slot, maps)
    g_plain, g_merged = eng.alloc_outputs(1), eng.alloc_outputs(1)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    counter = state[1][:4].view(torch.int32)
    saved = counter.clone()

    def gathered(merge, outs_):
        counter.copy_(saved)                           # the NMS kernel zeroes the group's counter: restore the list's length
        eng.set_nms_merge(merge)
        return ev_time(lambda: eng.nms_gathered(state, outs_, cnt))
    for _ in range(5):
        gathered(False, g_plain); gathered(True, g_merged)
    tp, tm = [], []
    for _ in range(a.reps):
        tp.append(gathered(False, g_plain)); tm.append(gathered(True, g_merged))
    eng.set_nms_merge(False)
    torch.cuda.synchronize()
    d = [m - p for p, m in zip(tp, tm)]
    doc["tiled"] = {"rows": R, "list_length": int(cnt.cpu()[0]), "group_cap": cap, "y4_nms_gathered": stats(tp),
                    "y4_nms_gathered_merged": stats(tm), "merged_minus_plain": stats(d), "kept_boxes": int(g_plain[3].sum()),
                    "boxes_moved": int((g_plain[0] != g_merged[0]).any(dim=2).sum()),
                    "everything_but_boxes_identical": bool(all(torch.equal(x, y) for x, y in zip(g_plain[1:], g_merged[1:]))),
                    "ratio_to_y4_nms_gathered_median": round(stats(d)["median_ms"] / stats(tp)["median_ms"], 4)}
    print(json.dumps(doc))
    eng.close()


def judge(parent, new):
    """The span rule of scripts/bench_nms_rule.py on medians."""
    lo, hi = min(parent), max(parent)
    span = hi - lo
    return {"parent": parent, "new": new, "allowed": [lo - span, hi + span], "passes": all(lo - span <= v <= hi + span for v in new)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_merge", "bench_nms_merge.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR: a built checkout of the parent commit")
    parent = os.path.abspath(a.parent_tree)

    def last_json(cmd, cwd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=cwd)
        if r.returncode != 0:                          # (nothing more is started on the GPU after a failed run)
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"{cwd}: {' '.join(cmd)}: exit {r.returncode}")
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        doc = json.loads(lines[-1])
        print(json.dumps(doc)[:600], flush=True)
        return doc

    def measure(tree):
        return last_json([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--reps", str(a.reps)], tree)

    def bench(tree, *shape):
        keep = ("value", "unit", "outputs_sha256")
        doc = last_json([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", *shape], tree)
        return {k: doc.get(k) for k in keep}
    small = ("--size", "160", "--classes", "3", "--batch", "4")
    runs = {}
    for k in range(a.runs):
        for name, tree in (("parent", parent), ("new", ROOT)):
            runs[f"{name}_run{k + 1}"] = {"measure": measure(tree), "bench": bench(tree)}
    runs["parent_small"], runs["new_small"] = bench(parent, *small), bench(ROOT, *small)

    def col(prefix, get):
        return [get(v) for k, v in runs.items() if k.startswith(prefix + "_run")]
    verdict = {
        "nms_op_ms": judge(col("parent", lambda v: v["measure"]["profile"]["nms"]["median_ms"]),
                           col("new", lambda v: v["measure"]["profile"]["nms"]["median_ms"])),
        "decode_op_ms": judge(col("parent", lambda v: v["measure"]["profile"]["decode"]["median_ms"]),
                              col("new", lambda v: v["measure"]["profile"]["decode"]["median_ms"])),
        "bench_images_per_s": judge(col("parent", lambda v: v["bench"]["value"]), col("new", lambda v: v["bench"]["value"])),
        "outputs_sha256_headline_equal": len({v["bench"]["outputs_sha256"] for k, v in runs.items() if "_run" in k}) == 1,
        "outputs_sha256_160_3_4_equal": runs["parent_small"]["outputs_sha256"] == runs["new_small"]["outputs_sha256"],
    }
    doc = {"what": f"{SIZE}^2, {NCLS} classes, batch {BATCH}, {DTYPE}, bench input; medians of {a.reps}; parent and this tree alternating, "
                   f"{a.runs} runs each, one MI355X, one session",
           "runs": runs, "verdict": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(verdict))


if __name__ == "__main__":
    main()
