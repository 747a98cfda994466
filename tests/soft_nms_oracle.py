"""Test oracle for Soft-NMS (y4_set_nms_soft): the rule of include/yolo4hip.h restated as a loop, NumPy only.

Per image: the candidates are every (box, class) with score > score_threshold (strict); the participants P are the `top_k` best in
the order this build defines (score descending, box index ascending, class ascending).  Working scores w = s.  Until `total`
boxes are kept: among the participants that are neither kept nor turned away and have w > min_score (strict) take the one with
the largest (w, then box index ascending, then class ascending); none: stop.  If its class holds `per_class` kept boxes it is
turned away -- not kept, decays nothing.  Otherwise it is kept with output score w, and every other live participant j of its class
(of any class with `agnostic`) gets w_j *= f(m), m = the measure of the pair rule (tests/nms_rule_oracle.measure: the float32
function, the penalty on every pair):
    gaussian  f = m > 0 ? exp(-(m * m) / sigma) : 1          linear  f = m > iou_thr ? 1 - m : 1          hard  f = m > iou_thr ? 0 : 1

Two faces, one loop (`face`):
  'f32'  every operation in float32 in the kernel's order: m * m, / sigma, exp, w * f, one rounding each.
  'f64'  the measure is still the float32 function (the rule defines it so) but everything behind it -- the factor, the products,
         every comparison -- is float64.  This face also returns
           margin  the smallest relative distance at any decision it took: picked score against every other live score
                   (|w_k - w_j| / w_k; pairs of two never-decayed scores are left out: they are float32 inputs, compared exactly on
                   both sides, ties by index), a decayed w against min_score (|w - min| / min), m against iou_thr for linear / hard
                   (|m - thr| / thr, m in float32 and again in float64, the smaller), and for gaussian m against 0 (|m|: zero has no
                   scale; an m that is exactly 0 in float32 and float64 alike -- disjoint boxes under 'iou', whose intersection is
                   max(difference of two inputs, 0) on both sides -- is exact and left out);
           bound   per output score, the first-order bound of the float32 face's relative error against this face (see
                   `decay_ulps`), 0 for a score that was never decayed.
"""
import numpy as np

import nms_rule_oracle as NR

F32 = np.float32
METHODS = ("gaussian", "linear", "hard")
EXPF_ULPS = 1.0          # float32 expf of the device library and of NumPy: within 1 ulp of the exact value
POWF_ULPS = 2.0          # float32 powf of either side (the 'diou' penalty with beta != 1): within 2 ulp


def measure_ulps(kind, beta):
    """Units of 2^-24 (absolute; the measure is at most 1) by which the float32 measure of the device may differ from this
    oracle's.  'iou', and 'diou' with beta == 1, are additions, products and divisions in one order: the same bits on both sides.
    beta != 1: the penalty powf(q, beta) <= 1 is within POWF_ULPS ulp (an ulp being at most 2 * 2^-24 of the value) on either
    side, and the subtraction iou - penalty rounds once on either side: 4 POWF_ULPS + 2."""
    return 0.0 if kind == "iou" or float(beta) == 1.0 else 4.0 * POWF_ULPS + 2.0


def decay_ulps(method, arg, m=0.0, f=1.0, sigma=0.5, m_ulps=0.0):
    """Units of 2^-24 of relative error one float32 decay adds to a working score, first order.  gaussian: t = fl(m * m) and
    u = fl(t / sigma) carry 2^-24 relative each, i.e. the argument of exp is off by at most 2 * u * 2^-24 absolute, which is the
    relative error it gives exp(-u); expf itself is within EXPF_ULPS ulp, an ulp being at most 2^-23 = 2 * 2^-24 relative; the
    product w * f rounds once: 2 u + 2 EXPF_ULPS + 1.  linear: fl(1 - m) and the product: 2.  hard: the factor is 0 or 1: 0.
    A measure that is off by m_ulps (`measure_ulps`) moves ln f by (2 m / sigma) * m_ulps (gaussian) and f by m_ulps, i.e. by
    m_ulps / f relative (linear)."""
    if method == "gaussian":
        return 2.0 * arg + 2.0 * EXPF_ULPS + 1.0 + (2.0 * abs(m) / sigma) * m_ulps
    if method == "linear":
        return 2.0 + m_ulps / max(f, 1e-30)
    return 0.0


def global_bound(total, sigma=0.5, method="gaussian"):
    """The bound for any score after at most `total` decays (a box is decayed once per kept box at most), with m <= 1 and a
    measure that is the same bits on both sides: total * (2 / sigma + 2 * EXPF_ULPS + 1) * 2^-24 -- 4.2e-5 at total = 100,
    sigma = 0.5; with the typical argument m * m / sigma well under 1/2 it is total * (EXPF_ULPS + 1) * 2^-23 = 2.4e-5."""
    return total * decay_ulps(method, 1.0 / sigma) * 2.0 ** -24


def soft_nms(boxes, scores, per_class=100, total=100, iou_thr=0.413, score_thr=0.3, kind="iou", beta=1.0, agnostic=False,
             method="gaussian", sigma=0.5, min_score=None, top_k=4096, face="f32"):
    """boxes [N, nbox, 4] normalised, scores [N, nbox, C] -> (nmsed_boxes [N, T, 4] clipped, nmsed_scores [N, T] (float32 for face
    'f32', float64 for 'f64'), nmsed_classes [N, T], valid [N] int32, kept_idx [N, T] int32 (-1 padded), margin, bound [N, T])."""
    assert method in METHODS and kind in NR.KINDS and face in ("f32", "f64") and 1 <= top_k
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    n, nbox, ncls = scores.shape
    T = total
    W = F32 if face == "f32" else np.float64
    thr32, sthr = F32(iou_thr), F32(score_thr)
    thr, sig = W(thr32), W(F32(sigma))
    floor = W(sthr if min_score is None else F32(min_score))
    out_b = np.zeros((n, T, 4), F32); out_s = np.zeros((n, T), W)
    out_c = np.zeros((n, T), F32); out_v = np.zeros((n,), np.int32)
    out_i = np.full((n, T), -1, np.int32)
    out_bound = np.zeros((n, T), np.float64)
    margin = np.inf
    for b in range(n):
        sc = scores[b]
        bi, ci = np.nonzero(sc > sthr)
        order = np.lexsort((ci, bi, -sc[bi, ci].astype(np.float64)))[:top_k]
        bi, ci = bi[order], ci[order]                      # the participants, best first
        w = sc[bi, ci].astype(W)
        pb = boxes[b, bi]
        free = np.ones(len(w), bool)                       # neither kept nor turned away
        touched = np.zeros(len(w), bool)
        ulps = np.zeros(len(w), np.float64)
        count = np.zeros(ncls, np.int64)
        k = 0
        while k < T:
            live = free & (w > floor)
            if not live.any():
                break
            idx = np.nonzero(live)[0]
            # the largest (w, then box ascending, then class ascending): idx is in (box, class)-compatible candidate order only
            # for equal ORIGINAL scores, so order explicitly
            best = idx[np.lexsort((ci[idx], bi[idx], -w[idx].astype(np.float64)))[0]]
            if face == "f64":
                others = idx[idx != best]
                others = others[touched[others] | touched[best]]
                if others.size:
                    margin = min(margin, float(np.min(np.abs(w[best] - w[others])) / w[best]))
            free[best] = False
            c = ci[best]
            if count[c] >= per_class:
                continue                                   # turned away: not kept, decays nothing
            count[c] += 1
            out_b[b, k] = np.clip(pb[best], F32(0), F32(1))
            out_s[b, k] = w[best]; out_c[b, k] = c; out_i[b, k] = bi[best]
            out_bound[b, k] = ulps[best] * 2.0 ** -24 * 1.001
            k += 1
            nb = np.nonzero(free & (w > floor) & (True if agnostic else ci == c))[0]
            if not nb.size:
                continue
            m32 = NR.measure(pb[best], pb[nb], kind, beta, F32)         # measure(a, others) is symmetric in its two boxes
            m = m32.astype(W)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                if method == "gaussian":
                    hit = m > 0
                    arg = (m * m) / sig
                    f = np.where(hit, np.exp(-arg), W(1)).astype(W)
                else:
                    hit = m > thr
                    arg = np.zeros_like(m)
                    f = np.where(hit, (W(1) - m) if method == "linear" else W(0), W(1)).astype(W)
                if face == "f64":
                    m64 = NR.measure(pb[best], pb[nb], kind, beta, np.float64)
                    if method == "gaussian":
                        exact_zero = (m32 == 0) & (m64 == 0)
                        d = np.concatenate([np.abs(m32.astype(np.float64))[~exact_zero], np.abs(m64)[~exact_zero]])
                    else:
                        d = np.concatenate([np.abs(m32.astype(np.float64) - thr), np.abs(m64 - thr)]) / thr
                    d = d[np.isfinite(d)]
                    if d.size:
                        margin = min(margin, float(d.min()))
                changed = np.nonzero(hit)[0]
                w[nb] = (w[nb] * f).astype(W)
            touched[nb[changed]] = True
            mu = measure_ulps(kind, beta)
            ulps[nb[changed]] += [decay_ulps(method, float(arg[j]), float(m[j]), float(f[j]), float(sig), mu) for j in changed]
            if face == "f64" and changed.size and floor > 0:
                margin = min(margin, float(np.min(np.abs(w[nb[changed]] - floor)) / floor))
        out_v[b] = k
    return out_b, out_s, out_c, out_v, out_i, margin, out_bound
