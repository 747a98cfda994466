"""The data-set anchor search restated in NumPy, rule by rule (include/yolo4hip.h "Data-set anchors"): what
y4_anchor_step / y4_anchor_fitness / y4_anchor_evolve and yolo4hip.anchors.fit_anchors must give, bit for bit.  Loops run over
anchors, sets and generations; one statement handles all boxes.  Nothing here imports the package."""
import numpy as np

Q30 = 1073741824.0
Q16 = 65536.0


def iou64(wh, anchor):
    """The centred IoU of every box [n,2] float32 with ONE anchor (w, h): half sides and box area in float32, the rest float64."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    w, h = wh[:, 0], wh[:, 1]
    hbw = (w * np.float32(0.5)).astype(np.float64)
    hbh = (h * np.float32(0.5)).astype(np.float64)
    area_b = (w * h).astype(np.float64)                                   # a float32 product
    aw, ah = np.float64(np.float32(anchor[0])), np.float64(np.float32(anchor[1]))
    lo_x, hi_x = np.maximum(-hbw, -(aw / 2.0)), np.minimum(hbw, aw / 2.0)
    lo_y, hi_y = np.maximum(-hbh, -(ah / 2.0)), np.minimum(hbh, ah / 2.0)
    inter = np.maximum(hi_x - lo_x, 0.0) * np.maximum(hi_y - lo_y, 0.0)
    return inter / (area_b + aw * ah - inter)


def best_anchor(wh, anchors):
    """-> (index int64 [n], iou float64 [n]): the first arg-max over the anchors, strict `>` to replace."""
    anchors = np.asarray(anchors, dtype=np.float32).reshape(-1, 2)
    best = iou64(wh, anchors[0])
    idx = np.zeros(len(best), dtype=np.int64)
    for j in range(1, len(anchors)):
        iou = iou64(wh, anchors[j])
        m = iou > best
        best = np.where(m, iou, best)
        idx[m] = j
    return idx, best


def fitness(wh, anchors):
    """F = sum llrint(iou64(best) * 2^30) as a Python int."""
    _idx, best = best_anchor(wh, anchors)
    return int(np.rint(best * Q30).astype(np.int64).sum())


def step(wh, anchors):
    """One Lloyd step -> (next float32 [k,2], stats int64 [1 + 3k] = F, cnt, SW, SH, assign uint8 [n])."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    anchors = np.asarray(anchors, dtype=np.float32).reshape(-1, 2)
    k = len(anchors)
    idx, best = best_anchor(wh, anchors)
    stats = np.zeros(1 + 3 * k, dtype=np.int64)
    stats[0] = np.rint(best * Q30).astype(np.int64).sum()
    qw = np.rint(wh[:, 0].astype(np.float64) * Q16).astype(np.int64)
    qh = np.rint(wh[:, 1].astype(np.float64) * Q16).astype(np.int64)
    nxt = anchors.copy()
    for j in range(k):
        m = idx == j
        cnt = int(m.sum())
        stats[1 + j], stats[1 + k + j], stats[1 + 2 * k + j] = cnt, qw[m].sum(), qh[m].sum()
        if cnt:
            nxt[j, 0] = np.float32(np.float64(stats[1 + k + j]) / np.float64(cnt) / Q16)
            nxt[j, 1] = np.float32(np.float64(stats[1 + 2 * k + j]) / np.float64(cnt) / Q16)
    return nxt, stats, idx.astype(np.uint8)


def by_size(wh):
    """The order (float32 area w * h, w, h) ascending."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    return np.lexsort((wh[:, 1], wh[:, 0], wh[:, 0] * wh[:, 1]))


def start(wh, k):
    """Anchor j = the box at rank ((2j + 1) n) // (2k) of that order."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    order = by_size(wh)
    n = len(wh)
    return np.stack([wh[order[((2 * j + 1) * n) // (2 * k)]] for j in range(k)]).astype(np.float32)


def lloyd(wh, anchors, iters):
    """-> (anchors, steps run, converged): until a step returns its input bit for bit, or `iters` steps have run."""
    cur = np.asarray(anchors, dtype=np.float32).reshape(-1, 2).copy()
    steps, converged = 0, False
    while steps < iters and not converged:
        nxt, _stats, _assign = step(wh, cur)
        steps += 1
        converged = nxt.tobytes() == cur.tobytes()
        cur = nxt
    return cur, steps, converged


def evolve(wh, best, f_best, mult):
    """mult float32 [G,P,k,2] -> (best, F_best, F_hist int64 [G,P], accepted int32 [G])."""
    best = np.asarray(best, dtype=np.float32).reshape(-1, 2).copy()
    mult = np.asarray(mult, dtype=np.float32)
    G, P = mult.shape[:2]
    f_best = int(f_best)
    f_hist = np.zeros((G, P), dtype=np.int64)
    accepted = np.full(G, -1, dtype=np.int32)
    for g in range(G):
        cand = [np.maximum(best * mult[g, p], np.float32(1.0)).astype(np.float32) for p in range(P)]
        for p in range(P):
            f_hist[g, p] = fitness(wh, cand[p])
        win = 0
        for p in range(1, P):
            if f_hist[g, p] > f_hist[g, win]:
                win = p
        if int(f_hist[g, win]) > f_best:
            best, f_best, accepted[g] = cand[win], int(f_hist[g, win]), win
    return best, f_best, f_hist, accepted


def fit(wh, mult, iters=300, init=None, k=9):
    """The whole of fit_anchors on given multipliers (mult None or empty: no evolution) -> dict."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    a0 = start(wh, k) if init is None else np.asarray(init, dtype=np.float32).reshape(k, 2)
    km, steps, converged = lloyd(wh, a0, iters)
    f_km = fitness(wh, km)
    best, f_best = km, f_km
    f_hist, accepted = np.zeros((0, 0), dtype=np.int64), np.zeros(0, dtype=np.int32)
    if mult is not None and len(mult):
        best, f_best, f_hist, accepted = evolve(wh, km, f_km, mult)
    final = best[by_size(best)]
    _nxt, stats, assign = step(wh, final)
    n = len(wh)
    return {"anchors": final, "fitness": int(stats[0]), "avg_iou": int(stats[0]) / n / Q30, "counts": stats[1:1 + k].copy(),
            "assign": assign, "iterations": steps, "converged": converged, "anchors_kmeans": km, "fitness_kmeans": f_km,
            "avg_iou_kmeans": f_km / n / Q30, "f_hist": f_hist, "accepted": accepted}


def mixture(n, seed, size=416.0):
    """Seeded log-normal mixture of box sizes, float32 [n,2] inside [1, size]: three populations of small, wide and tall boxes."""
    rng = np.random.default_rng(seed)
    comp = rng.integers(0, 3, size=n)
    mu = np.array([[2.8, 3.0], [4.6, 3.8], [4.0, 5.2]])[comp]
    sd = np.array([0.45, 0.35, 0.30])[comp][:, None]
    wh = np.exp(mu + sd * rng.standard_normal((n, 2)))
    return np.clip(wh, 1.0, size).astype(np.float32)
