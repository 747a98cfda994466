#!/usr/bin/env python3
"""Video frames (NV12) against packed RGB frames of the same size, in one process on one GPU, at 608 x 608 / 80 classes /
batch 32 / bf16 under the shipped schedule:

  kernel   y4_yuv_u8_ragged on 32 NV12 frames of 1080 x 1920 against y4_resize_u8_ragged on their RGB conversions (device time
           between two events, alternating), and each kernel against itself for the spread.  The results are compared byte for
           byte first.
  stream   Engine.predict_stream(yuv='nv12') against Engine.predict_stream on the RGB frames, from pinned host batches to host
           results, in images/s, alternating passes of --batches batches; per frame size.
  to_rgb   the host-side conversion a user pays today before the RGB path can start, here `yuv.to_rgb` (NumPy, one thread) per
           1080 x 1920 frame.  It is NOT part of the stream comparison, which compares equal work on frames that already exist.

Medians, minima and maxima over --reps alternating measurements.  Writes one JSON document to --out and prints it.

  python scripts/bench_yuv.py [--reps 20] [--warmup 3] [--batches 8] [--out profiles/yuv/bench_yuv.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-v4-tf.keras_amd"))

SIZE, NCLS, BATCH, DTYPE = 608, 80, 32, "bf16"
STREAM_FRAMES = [(1080, 1920), (720, 1280), (608, 608)]


def stats(ts):
    s = sorted(ts)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8, help="batches per timed stream pass")
    ap.add_argument("--in-flight", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv", "bench_yuv.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from yolo4hip import ext, yuv, weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan

    eng = Engine(NCLS, make_config(SIZE), max_batch=BATCH, dtype=DTYPE, alias_workspace=True)
    eng.load_weight_blob(W.flatten(W.synth_weights(build_plan(SIZE, NCLS), 0)))
    eng.set_stem_fusion(True)
    eng.set_chain_fusion(True)
    eng.set_stage_fusion(True)
    eng.set_res_fusion(True)
    source = eng.ensure_schedule(tune=False, verbose=False)
    dev = eng.device
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "size": SIZE, "classes": NCLS, "dtype": DTYPE, "batch": BATCH,
           "schedule": source[0], "reps": a.reps, "in_flight": a.in_flight}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(fa, fb, timer, warmup):
        for _ in range(warmup):
            timer(fa); timer(fb)
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timer(fa)); tb.append(timer(fb))
        return ta, tb

    def frames(fh, fw):
        """BATCH distinct NV12 frames [BATCH, fh + fh // 2, fw]: four images of 8 x 8 blocks of random colour plus noise (the content
        of the tests) through from_rgb, each shifted sideways by an even number of columns eight times."""
        out = []
        for _ in range(4):
            base = rng.integers(0, 256, ((fh + 7) // 8, (fw + 7) // 8, 3))
            img = np.kron(base, np.ones((8, 8, 1)))[:fh, :fw] + rng.integers(-20, 21, (fh, fw, 3))
            f = yuv.from_rgb(np.clip(img, 0, 255).astype(np.uint8), "nv12").data.reshape(fh + fh // 2, fw)
            out += [np.roll(f, 2 * 37 * k, axis=1) for k in range(BATCH // 4)]
        return np.stack(out)

    # ---- (a) the kernels: 32 NV12 frames of 1080 x 1920
    h, w = 1080, 1920
    raw = frames(h, w)
    t0 = time.perf_counter()
    rgb = np.stack([yuv.to_rgb(f) for f in raw])
    res["to_rgb_host"] = {"what": "yuv.to_rgb (NumPy restatement, one thread), 1080 x 1920 NV12 -> RGB",
                          "ms_per_frame": round((time.perf_counter() - t0) * 1e3 / BATCH, 2)}
    ydesc, rdesc = (ext.y4_yuv_desc * BATCH)(), (ext.y4_image_desc * BATCH)()
    layout = yuv.YuvFrame(raw[0])
    for j in range(BATCH):
        layout.fill_desc(ydesc[j], j * raw[0].size, yuv.flags())
        rdesc[j].offset, rdesc[j].h, rdesc[j].w = j * h * w * 3, h, w
        for d in (ydesc[j], rdesc[j]):
            d.out_h, d.out_w, d.pad_top, d.pad_left = SIZE, SIZE, 0, 0
    ysrc, rsrc = torch.from_numpy(raw.reshape(-1)).to(dev), torch.from_numpy(rgb.reshape(-1)).to(dev)   # (flat: the bytes as they lie)
    yd = torch.from_numpy(np.frombuffer(ydesc, dtype=np.uint8).copy()).to(dev)
    rd = torch.from_numpy(np.frombuffer(rdesc, dtype=np.uint8).copy()).to(dev)
    out_y = torch.empty((BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    out_r = torch.empty((BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device=dev)
    run_y = lambda: eng.yuv_u8_ragged(ysrc, yd, BATCH, out_y)
    run_r = lambda: eng.resize_u8_ragged(rsrc, rd, BATCH, out_r)
    run_y(); run_r()
    torch.cuda.synchronize()
    if not torch.equal(out_y, out_r):
        from yolo4hip import prepost
        host = prepost.resize_bilinear(rgb[0], (SIZE, SIZE))
        raise SystemExit("y4_yuv_u8_ragged and y4_resize_u8_ragged on the converted frames differ; against the host restatement "
                         f"on frame 0: yuv {int((out_y[0].cpu().numpy() != host).sum())} bytes, rgb "
                         f"{int((out_r[0].cpu().numpy() != host).sum())} bytes")
    ty, tr = alternate(run_y, run_r, ev_time, a.warmup)
    ty_a, ty_b = alternate(run_y, run_y, ev_time, 1)
    tr_a, tr_b = alternate(run_r, run_r, ev_time, 1)
    ky, kr = stats(ty), stats(tr)
    res["kernel"] = {"frames": f"{BATCH} x {h} x {w}", "unit": "ms", "source_mb": {"nv12": round(raw.nbytes / 1e6, 1), "rgb": round(rgb.nbytes / 1e6, 1)},
                     "y4_yuv_u8_ragged": ky, "y4_resize_u8_ragged_on_rgb": kr,
                     "yuv_over_rgb_median": round(ky["median"] / kr["median"], 3),
                     "yuv_against_itself": [stats(ty_a), stats(ty_b)], "rgb_against_itself": [stats(tr_a), stats(tr_b)]}
    del ysrc, rsrc

    # ---- (b) the stream: pinned host batches -> host results
    res["stream"] = []
    for fh, fw in STREAM_FRAMES:
        # two distinct batches per side: the frames of the kernel part where the size is theirs, and the same frames in reverse order
        y0 = raw if (fh, fw) == (h, w) else frames(fh, fw)
        r0 = rgb if (fh, fw) == (h, w) else np.stack([yuv.to_rgb(f) for f in y0])
        yb = [torch.from_numpy(np.ascontiguousarray(b)).pin_memory() for b in (y0, y0[::-1])]
        rb = [torch.from_numpy(np.ascontiguousarray(b)).pin_memory() for b in (r0, r0[::-1])]

        def pass_yuv():
            return sum(r[3].shape[0] for r in eng.predict_stream((yb[i % 2] for i in range(a.batches)), in_flight=a.in_flight, yuv="nv12"))

        def pass_rgb():
            return sum(r[3].shape[0] for r in eng.predict_stream((rb[i % 2] for i in range(a.batches)), in_flight=a.in_flight))

        def rate(fn):
            t0 = time.perf_counter()
            got = fn()
            return got / (time.perf_counter() - t0)

        got_y = list(eng.predict_stream(yb, yuv="nv12", with_indices=True, in_flight=a.in_flight))
        got_r = list(eng.predict_stream(rb, with_indices=True, in_flight=a.in_flight))
        same = all(np.array_equal(x, y) for gy, gr in zip(got_y, got_r) for x, y in zip(gy, gr))
        ry, rr = alternate(pass_yuv, pass_rgb, rate, a.warmup)
        sy, sr = stats(ry), stats(rr)
        res["stream"].append({"frames": f"{fh} x {fw}", "unit": "images/s", "batches_per_pass": a.batches, "same_results": bool(same),
                              "mb_per_batch": {"nv12": round(yb[0].numel() / 1e6, 1), "rgb": round(rb[0].numel() / 1e6, 1)},
                              "predict_stream_nv12": sy, "predict_stream_rgb": sr,
                              "nv12_over_rgb_median": round(sy["median"] / sr["median"], 3)})
        del yb, rb
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh_:
        json.dump(res, fh_, indent=1)
        fh_.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
