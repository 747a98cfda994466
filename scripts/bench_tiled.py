#!/usr/bin/env python3
"""Tiled inference, measured in one process on one GPU: 608^2, 80 classes, bf16, batch capacity 32, the shipped schedule, synthetic
weights; one 2432 x 1824 random uint8 photo at overlap 0.2 plus the full image (5 x 4 windows + 1 = 21 rows, one forward chunk).

  window    y4_window_u8_ragged on the photo against y4_resize_u8_ragged on contiguous copies of the same windows (device time,
            HIP events around the launch);
  gather    y4_decode_gather (decode stage + gather_kernel) and y4_nms_gathered (count copy + the grouped NMS) by events, beside
            the `decode` and `nms` ops y4_profile reports for the same rows: gather_kernel alone is about decode_gather - decode;
  end2end   Engine.predict_tiled against the loop a user writes from the existing pieces: host crops -> preprocess_u8_batch ->
            predict per chunk -> host merge of the per-tile survivors (boxes mapped to the photo, one greedy NumPy NMS over
            them).  Host time from the call to the result on the host.  The two do NOT compute the same thing: the loop caps at
            max_total per tile and suppresses inside each tile before cross-tile duplicates are visible.

The two sides of every comparison ALTERNATE (a, b, a, b, ...) after a warm-up; medians, minima and maxima of --reps are reported.
One run on one machine; nothing beyond that is claimed.

  python scripts/bench_tiled.py [--reps 20] [--warmup 3] [--out profiles/tiled/bench_tiled.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))

SIZE, NCLS, BATCH, DTYPE = 608, 80, 32, "bf16"
PHOTO_HW, OVERLAP = (1824, 2432), 0.2


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def host_nms(boxes, scores, classes, iou_thr, total):
    """Greedy class-aware IoU NMS over the merged survivors (the user's host merge)."""
    import numpy as np
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))
    keep = []
    for i in order:
        if len(keep) >= total:
            break
        same = [k for k in keep if classes[k] == classes[i]]
        if same:
            b, o = boxes[i], boxes[same]
            iw = np.maximum(np.minimum(b[2], o[:, 2]) - np.maximum(b[0], o[:, 0]), 0)
            ih = np.maximum(np.minimum(b[3], o[:, 3]) - np.maximum(b[1], o[:, 1]), 0)
            inter = iw * ih
            union = (b[2] - b[0]) * (b[3] - b[1]) + (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1]) - inter
            if np.any(inter > iou_thr * union):
                continue
        keep.append(i)
    return keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled", "bench_tiled.json"))
    a = ap.parse_args()
    import ctypes as C
    import numpy as np
    import torch
    from yolo4hip import ext, tiling, weights as W
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

    # ---- window kernel against the ragged resize on contiguous copies
    wdesc = (ext.y4_window_desc * R)()
    rdesc = (ext.y4_image_desc * R)()
    crops, off = [], 0
    for d, r, ((y0, x0, wh, ww), rect, _) in zip(wdesc, rdesc, rows):
        d.offset, d.pitch, d.h, d.w = (y0 * PHOTO_HW[1] + x0) * 3, PHOTO_HW[1] * 3, wh, ww
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
        c = np.ascontiguousarray(photo[y0:y0 + wh, x0:x0 + ww])
        r.offset, r.h, r.w = off, wh, ww
        r.out_h, r.out_w, r.pad_top, r.pad_left = rect
        off += c.size
        crops.append(c)
    dev = eng.device
    src = torch.from_numpy(photo.reshape(-1)).to(dev)
    csrc = torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).to(dev)
    wd = torch.from_numpy(np.frombuffer(wdesc, dtype=np.uint8).copy()).to(dev)
    rd = torch.from_numpy(np.frombuffer(rdesc, dtype=np.uint8).copy()).to(dev)
    out_w = torch.empty((R, H, Wd, 3), dtype=torch.uint8, device=dev)
    out_r = torch.empty((R, H, Wd, 3), dtype=torch.uint8, device=dev)
    eng.window_u8_ragged(src, wd, R, out_w)
    eng.resize_u8_ragged(csrc, rd, R, out_r)
    torch.cuda.synchronize()
    if not torch.equal(out_w, out_r):
        raise SystemExit("window kernel and ragged resize of the copies differ")
    window, resize = alternate(lambda: eng.window_u8_ragged(src, wd, R, out_w), lambda: eng.resize_u8_ragged(csrc, rd, R, out_r), ev_time)
    res = {"device": torch.cuda.get_device_name(0), "size": SIZE, "classes": NCLS, "dtype": DTYPE, "max_batch": BATCH,
           "schedule": source[0], "photo_hw": list(PHOTO_HW), "overlap": OVERLAP, "rows": R, "reps": a.reps,
           "window_kernel": {"y4_window_u8_ragged": window, "y4_resize_u8_ragged_on_copies": resize,
                             "resize_spread_ms": round(resize["max_ms"] - resize["min_ms"], 4),
                             "window_minus_resize_median_ms": round(window["median_ms"] - resize["median_ms"], 4)}}
    res["window_kernel"]["no_slower_beyond_resize_spread"] = bool(
        res["window_kernel"]["window_minus_resize_median_ms"] <= res["window_kernel"]["resize_spread_ms"])

    # ---- gather and the grouped NMS, beside y4_profile's decode and nms for the same rows
    eng.forward_device(out_w)
    group = torch.zeros(R, dtype=torch.int32, device=dev)
    slot = torch.arange(R, dtype=torch.int32, device=dev)
    maps = torch.from_numpy(np.stack([m for _, _, m in rows])).to(dev)
    cap = 1 << 18
    state = eng.gather_begin(1, R, cap)
    outs = eng.alloc_outputs(1)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    t_dg, t_nms = [], []
    for i in range(a.warmup + a.reps):
        ext.check(eng.lib.y4_gather_begin(eng.handle, 1, R, cap, ext.ptr(state[1]), ext.stream_ptr()))
        x = ev_time(lambda: eng.decode_gather(state, R, group, slot, maps))
        y = ev_time(lambda: eng.nms_gathered(state, outs, cnt))
        if i >= a.warmup:
            t_dg.append(x); t_nms.append(y)
    prof = {}
    imgs_f = out_w.float() / 255.0
    for i in range(a.warmup + a.reps):
        ops = eng.profile(imgs_f)
        if i >= a.warmup:
            for name, ms in ops:
                if name in ("decode", "nms"):
                    prof.setdefault(name, []).append(ms)
    res["gather"] = {"candidates": int(cnt.cpu()[0]), "group_cap": cap,
                     "y4_decode_gather(decode+gather)": stats(t_dg), "y4_nms_gathered(counts+nms)": stats(t_nms),
                     "y4_profile": {k: stats(v) for k, v in prof.items()}}

    # ---- end to end against today's loop
    def tiled():
        return eng.predict_tiled([photo], overlap=OVERLAP)

    def loop():
        tiles = [np.ascontiguousarray(photo[y0:y0 + wh, x0:x0 + ww]) for (y0, x0, wh, ww), _, _ in rows]
        bs, ss, cs = [], [], []
        for r0 in range(0, R, BATCH):
            imgs, _ = eng.preprocess_u8_batch(tiles[r0:r0 + BATCH])
            b, s, c, v = eng.predict(imgs)
            for k in range(len(v)):
                m = rows[r0 + k][2].astype(np.float32)
                bb = b[k, :v[k]].copy()
                bb[:, 0::2] = bb[:, 0::2] * m[0] + m[1]
                bb[:, 1::2] = bb[:, 1::2] * m[2] + m[3]
                bs.append(bb); ss.append(s[k, :v[k]]); cs.append(c[k, :v[k]])
        bs, ss, cs = np.concatenate(bs), np.concatenate(ss), np.concatenate(cs)
        keep = host_nms(bs, ss, cs, cfg["iou_threshold"], eng.T)
        return np.clip(bs[keep], 0, 1), ss[keep], cs[keep]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_tiled, t_loop = alternate(tiled, loop, wall)
    res["end_to_end"] = {"predict_tiled": t_tiled, "host_loop": t_loop, "valid_tiled": int(tiled()[3][0]), "kept_loop": int(len(loop()[1])),
                         "note": "not the same computation: the loop runs NMS per tile (max_total per tile) before the merge"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
