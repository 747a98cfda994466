#!/usr/bin/env python3
"""What the data-set anchor search costs on one MI355X, beside the NumPy restatement of the same rule on the host's CPUs.

  python scripts/bench_anchors.py [--boxes 1048576] [--reps 20] [--runs 2] [--cpu-procs 16] [--out PATH]

Input: `--boxes` seeded log-normal box sizes (tests/anchors_oracle.mixture, seed 0), k = 9.  Per run, one process:
  step        y4_anchor_step (the memset, the accumulate kernel, the next-anchor kernel) by HIP events
  fitness     y4_anchor_fitness of P = 64 sets by HIP events; the pair-measure rate n * P * k / time is reported as a RATE of
              centred-IoU evaluations (a float64 division each), not as FLOP/s
  generation  y4_anchor_evolve with G = 1, P = 64 (the memset, the fitness launch, the select launch) by HIP events
  fit         the default fit_anchors(wh) end to end, wall clock, upload and every read-back included (once per run)
each after 3 warm-up calls, median / min / max of `--reps`.  Beside that, once: the oracle's step and its P = 64 generation on the
CPUs -- in one process (NumPy's elementwise kernels use one thread) and with the 64 candidates spread over `--cpu-procs` processes,
what a user without the device path would run.  Nothing is gated.  Writes profiles/anchors/bench_anchors.json."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "yolo-v4-tf.keras_amd"), os.path.join(ROOT, "tests")]
K, P = 9, 64


def med3(t):
    import numpy as np
    return [float(np.median(t)), float(np.min(t)), float(np.max(t))]


def inputs(n):
    import anchors_oracle as AO
    from yolo4hip.anchors import draw_mult
    wh = AO.mixture(n, 0)
    anchors = AO.start(wh, K)
    return wh, anchors, draw_mult(0, 1, P, K)


def gpu_child(a):
    import numpy as np
    import torch
    from yolo4hip import ext
    from yolo4hip.anchors import _Device, fit_anchors
    wh, anchors, mult = inputs(a.boxes)
    dev = _Device(wh, "cuda:0")
    lib, p, s = dev.lib, ext.ptr, ext.stream_ptr()
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev.device)      # noqa: E731
    anc, nxt = up(anchors, np.float32), torch.empty((K, 2), dtype=torch.float32, device=dev.device)
    stats = torch.empty(1 + 3 * K, dtype=torch.int64, device=dev.device)
    sets = up(np.maximum(anchors[None] * mult[0], np.float32(1.0)), np.float32)
    f = torch.empty(P, dtype=torch.int64, device=dev.device)
    m, hist = up(mult, np.float32), torch.empty((1, P), dtype=torch.int64, device=dev.device)
    acc, fb = torch.empty(1, dtype=torch.int32, device=dev.device), torch.zeros(1, dtype=torch.int64, device=dev.device)
    best = anc.clone()
    fb.fill_(1 << 62)                                             # nothing is accepted: every repetition does the same work

    def timed(call):
        t = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ext.check(call()); e1.record()
            e1.synchronize()
            if i >= 3:
                t.append(e0.elapsed_time(e1))
        return med3(t)

    def generation():
        return lib.y4_anchor_evolve(p(dev.wh), dev.n, p(best), p(fb), p(m), 1, P, K, p(hist), p(acc), s)

    doc = {"boxes": a.boxes, "k": K, "P": P}
    doc["step_ms"] = timed(lambda: lib.y4_anchor_step(p(dev.wh), dev.n, p(anc), K, p(nxt), p(stats), None, s))
    doc["fitness_ms"] = timed(lambda: lib.y4_anchor_fitness(p(dev.wh), dev.n, p(sets), P, K, p(f), s))
    doc["generation_ms"] = timed(generation)
    doc["pair_measures_per_second"] = a.boxes * P * K / (doc["fitness_ms"][0] * 1e-3)
    doc["step_F"], doc["fitness_sum"] = int(stats.cpu()[0]), int(f.cpu().sum())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = fit_anchors(wh)
    doc["fit_anchors_default_s"] = time.perf_counter() - t0
    doc["fit"] = {"iterations": fit.iterations, "converged": bool(fit.converged), "generations": len(fit.accepted),
                  "accepted": int((fit.accepted >= 0).sum()), "avg_iou_kmeans": fit.avg_iou_kmeans, "avg_iou": fit.avg_iou,
                  "anchors": [round(float(v), 3) for v in fit.anchors.reshape(-1)]}
    print(json.dumps(doc))


_WH = None


def _one_fitness(cand):
    import anchors_oracle as AO
    return AO.fitness(_WH, cand)


def cpu_child(a):
    global _WH
    import multiprocessing as mp
    import numpy as np
    import anchors_oracle as AO
    wh, anchors, mult = inputs(a.boxes)
    _WH = wh
    cands = [np.maximum(anchors * mult[0, q], np.float32(1.0)) for q in range(P)]
    t0 = time.perf_counter(); _nxt, stats, _as = AO.step(wh, anchors); t_step = time.perf_counter() - t0
    t0 = time.perf_counter(); f1 = [AO.fitness(wh, c) for c in cands]; t_gen1 = time.perf_counter() - t0
    with mp.get_context("fork").Pool(a.cpu_procs) as pool:
        pool.map(_one_fitness, cands[:a.cpu_procs])              # (the workers are up before the clock starts)
        t0 = time.perf_counter(); fN = pool.map(_one_fitness, cands); t_genN = time.perf_counter() - t0
    assert f1 == fN
    print(json.dumps({"boxes": a.boxes, "k": K, "P": P, "numpy_step_s": t_step, "numpy_generation_1_process_s": t_gen1,
                      "numpy_generation_pool_s": t_genN, "pool_processes": a.cpu_procs, "step_F": int(stats[0]),
                      "fitness_sum": int(sum(f1))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchors", "bench_anchors.json"))
    ap.add_argument("--child", choices=("gpu", "cpu"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return gpu_child(a) if a.child == "gpu" else cpu_child(a)

    def run(kind):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--boxes", str(a.boxes), "--reps", str(a.reps),
               "--cpu-procs", str(a.cpu_procs)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
        if r.returncode != 0:                                      # (nothing more is started after a failed run)
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{kind} run: exit {r.returncode}")
        doc = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(doc), flush=True)
        return doc
    runs = {f"run{i + 1}": run("gpu") for i in range(a.runs)}
    cpu = run("cpu")
    same = all(r["step_F"] == cpu["step_F"] and r["fitness_sum"] == cpu["fitness_sum"] for r in runs.values())
    r1 = runs["run1"]
    doc = {"what": f"{a.boxes} seeded boxes, k = {K}, P = {P}; HIP events, 3 warm-up calls, median / min / max of {a.reps}, one process "
                   f"per run; the NumPy oracle on the same machine's CPUs beside it; one MI355X, one session, nothing gated",
           "device_runs": runs, "numpy": cpu, "device_and_numpy_sums_equal": same,
           "numpy_over_device": {"step": cpu["numpy_step_s"] * 1e3 / r1["step_ms"][0],
                                 "generation_1_process": cpu["numpy_generation_1_process_s"] * 1e3 / r1["generation_ms"][0],
                                 "generation_pool": cpu["numpy_generation_pool_s"] * 1e3 / r1["generation_ms"][0]}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    if not same:
        raise SystemExit("the device sums differ from the oracle's")


if __name__ == "__main__":
    main()
