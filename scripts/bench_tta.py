#!/usr/bin/env python3
"""Test-time augmentation, measured in one process on one GPU: 608^2, 80 classes, bf16, batch capacity 32, the shipped schedule,
synthetic weights; one 1824 x 2432 random uint8 photo.

  view      (a) y4_view_u8_ragged at flip 0, 'lr' (1) and 'ud' (2) against y4_window_u8_ragged on the same table (the 21 rows of
            scripts/bench_tiled.py: 5 x 4 windows + the full image), device time by HIP events.  The window kernel is measured
            against itself too (window, window alternating): its own spread in this session is the yardstick for flip 0;
  gather    (b) y4_decode_gather_views against y4_decode_gather on the same 21 rows under identity maps (decode stage + gather
            kernel, by events);
  end2end   (c) Engine.predict_tta under the default views against the loop a user writes today: host resize + flip of the photo
            per view, three `predict` calls, host un-flip and one greedy NumPy NMS over the survivors.  Host time from the call
            to the result on the host.  The two do NOT compute the same thing: the loop shrinks the whole canvas rather than a
            centred rectangle, caps at max_total per view and suppresses inside each view before the views meet.

The two sides of every comparison ALTERNATE (a, b, a, b, ...) after a warm-up; medians, minima and maxima of --reps are reported.
(d) -- bench.py of the parent checkout against this build -- is two trees and therefore not in this script: run bench.py in each,
alternating, and compare outputs_sha256 and images/s (profiles/tta/README.md).
One run on one machine; nothing beyond that is claimed.

  python scripts/bench_tta.py [--reps 20] [--warmup 3] [--out profiles/tta/bench_tta_run1.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tiled import BATCH, DTYPE, NCLS, OVERLAP, PHOTO_HW, SIZE, host_nms, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta", "bench_tta_run1.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from yolo4hip import ext, prepost, tiling, weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan

    cfg = make_config(SIZE)
    eng = Engine(NCLS, cfg, max_batch=BATCH, dtype=DTYPE)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(SIZE, NCLS), seed=1)))
    source = eng.ensure_schedule(tune=False, verbose=False)
    H = Wd = SIZE
    photo = np.random.default_rng(0).integers(0, 256, PHOTO_HW + (3,), dtype=np.uint8)
    rows = tiling.tile_rows(PHOTO_HW[0], PHOTO_HW[1], (H, Wd), None, OVERLAP, True, False)
    R = len(rows)
    assert R <= BATCH
    dev = eng.device

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(fa, fb, timer):
        for _ in range(a.warmup):
            timer(fa); timer(fb)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timer(fa)); tb.append(timer(fb))
        return stats(ta), stats(tb)

    def table(Desc, flip=None):
        desc = (Desc * R)()
        for d, ((y0, x0, wh, ww), rect, _) in zip(desc, rows):
            d.offset, d.pitch, d.h, d.w = (y0 * PHOTO_HW[1] + x0) * 3, PHOTO_HW[1] * 3, wh, ww
            d.out_h, d.out_w, d.pad_top, d.pad_left = rect
            if flip is not None:
                d.flip = flip
        return torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(dev)

    # ---- (a) the view kernel against the window kernel on the same table
    src = torch.from_numpy(photo.reshape(-1)).to(dev)
    wd = table(ext.y4_window_desc)
    out_w = torch.empty((R, H, Wd, 3), dtype=torch.uint8, device=dev)
    out_v = torch.empty((R, H, Wd, 3), dtype=torch.uint8, device=dev)
    window = lambda: eng.window_u8_ragged(src, wd, R, out_w)                   # noqa: E731
    w1, w2 = alternate(window, window, ev_time)
    spread = round(max(w1["max_ms"], w2["max_ms"]) - min(w1["min_ms"], w2["min_ms"]), 4)
    res = {"device": torch.cuda.get_device_name(0), "size": SIZE, "classes": NCLS, "dtype": DTYPE, "max_batch": BATCH,
           "schedule": source[0], "photo_hw": list(PHOTO_HW), "rows": R, "reps": a.reps,
           "view_kernel": {"window_vs_window": {"a": w1, "b": w2, "spread_ms": spread,
                                                "median_difference_ms": round(abs(w1["median_ms"] - w2["median_ms"]), 4)}}}
    for name, flip, axes in (("flip0", 0, None), ("lr", 1, (2,)), ("ud", 2, (1,))):
        vd = table(ext.y4_view_desc, flip)
        eng.window_u8_ragged(src, wd, R, out_w)
        eng.view_u8_ragged(src, vd, R, out_v)
        torch.cuda.synchronize()
        if not torch.equal(out_v, out_w if axes is None else torch.flip(out_w, axes)):
            raise SystemExit(f"view kernel at flip {flip} is not the flipped window kernel")
        v, w = alternate(lambda: eng.view_u8_ragged(src, vd, R, out_v), window, ev_time)
        diff = round(v["median_ms"] - w["median_ms"], 4)
        res["view_kernel"][name] = {"y4_view_u8_ragged": v, "y4_window_u8_ragged": w, "view_minus_window_median_ms": diff,
                                    "inside_window_spread": bool(abs(diff) <= spread)}

    # ---- (b) the oriented gather against the plain gather, identity maps
    eng.window_u8_ragged(src, wd, R, out_w)
    eng.forward_device(out_w)
    group = torch.zeros(R, dtype=torch.int32, device=dev)
    slot = torch.arange(R, dtype=torch.int32, device=dev)
    ident = torch.tensor([[1.0, 0.0, 1.0, 0.0]] * R, dtype=torch.float32, device=dev)
    cap = 1 << 18
    state = eng.gather_begin(1, R, cap)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = eng.alloc_outputs(1)

    def gather(oriented):
        def run():
            ext.check(eng.lib.y4_gather_begin(eng.handle, 1, R, cap, ext.ptr(state[1]), ext.stream_ptr()))
            eng.decode_gather(state, R, group, slot, ident, oriented=oriented)
        return run

    kept = []
    for oriented in (False, True):
        gather(oriented)()
        eng.nms_gathered(state, outs, cnt)
        torch.cuda.synchronize()
        kept.append([o.cpu().numpy().copy() for o in outs])
    if not all(np.array_equal(x, y) for x, y in zip(*kept)):
        raise SystemExit("oriented and plain gather differ under identity maps")
    g_views, g_plain = alternate(gather(True), gather(False), ev_time)
    res["gather"] = {"candidates": int(cnt.cpu()[0]), "group_cap": cap, "begin+y4_decode_gather_views": g_views,
                     "begin+y4_decode_gather": g_plain,
                     "views_minus_plain_median_ms": round(g_views["median_ms"] - g_plain["median_ms"], 4)}

    # ---- (c) end to end against today's loop
    views = tiling.DEFAULT_VIEWS

    def tta():
        return eng.predict_tta([photo])

    def loop():
        bs, ss, cs = [], [], []
        for scale, flip in views:
            side = (max(1, int(round(Wd * scale))), max(1, int(round(H * scale))))
            small = prepost.resize_bilinear(photo, side)                         # host resize of the whole photo
            canvas = np.full((H, Wd, 3), 128, np.uint8)
            top, left = (H - side[1]) // 2, (Wd - side[0]) // 2
            canvas[top:top + side[1], left:left + side[0]] = small
            if "lr" in flip:
                canvas = canvas[:, ::-1]
            if "ud" in flip:
                canvas = canvas[::-1]
            b, s, c, v = eng.predict(np.ascontiguousarray(canvas)[None].astype(np.float32) / 255.0)
            bb = b[0, :v[0]].copy()
            if "lr" in flip:
                bb[:, [0, 2]] = 1.0 - bb[:, [2, 0]]
            if "ud" in flip:
                bb[:, [1, 3]] = 1.0 - bb[:, [3, 1]]
            bb[:, 0::2] = (bb[:, 0::2] * Wd - left) / side[0]
            bb[:, 1::2] = (bb[:, 1::2] * H - top) / side[1]
            bs.append(bb); ss.append(s[0, :v[0]]); cs.append(c[0, :v[0]])
        bs, ss, cs = np.concatenate(bs), np.concatenate(ss), np.concatenate(cs)
        keep = host_nms(bs, ss, cs, cfg["iou_threshold"], eng.T)
        return np.clip(bs[keep], 0, 1), ss[keep], cs[keep]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_tta, t_loop = alternate(tta, loop, wall)
    res["end_to_end"] = {"predict_tta": t_tta, "host_loop": t_loop, "valid_tta": int(tta()[3][0]), "kept_loop": int(len(loop()[1])),
                         "views": [list(v) for v in views],
                         "note": "not the same computation: the loop resizes on the host, runs NMS per view (max_total per view) "
                                 "and merges the survivors on the host"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
