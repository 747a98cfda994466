"""Test oracle for Matrix-NMS (y4_set_nms_matrix): the rule of include/yolo4hip.h restated in NumPy, vectorised per class.

Per image: the candidates are every (box, class) with score > score_threshold (strict); the participants P are the `top_k` best in
the order this build defines (score descending, box index ascending, class ascending); i < j means i comes earlier.  i and j
interact iff they have one class (always with `agnostic`).  m_ij is the measure of the pair rule (tests/nms_rule_oracle.measure: the
float32 function, the penalty on every pair), m+ its positive part (NaN -> 0).
    c_i = max over interacting k < i of m+_ki  (0 without one)        d_j = min over interacting i < j of t_ij  (1 without one)
    gaussian  t = exp((c_i * c_i - m+ * m+) / sigma)                  linear  t = (1 - m+) / (1 - c_i) where c_i < 1, else no term
    w_j = s_j * d_j
The candidates with w_j > min_score (strict) are walked by (w, then box index ascending, then class ascending), largest first; one whose
class holds `per_class` boxes is skipped; the walk stops at `total` boxes.

Two faces (`face`):
  'f32'  every operation in float32 in the kernel's order: c * c, m * m, the difference, / sigma, exp, s * d -- one rounding each
         (linear: 1 - m, 1 - c, the quotient, s * d).
  'f64'  the measure is still the float32 function (the rule defines it so; c, a maximum of measures, is then the same number) but
         everything behind it is float64.  This face also returns
           margin  the smallest relative distance at any decision: a decayed score against its neighbours in the walk's order, over
                   the walk up to the first candidate not taken (|w_a - w_b| / max; two undecayed scores are float32 inputs,
                   compared exactly on both sides, and left out); a decayed score against min_score (|w - min| / min; of the
                   candidates of that stretch, and of every participant when the walk reaches the end of the list); for linear,
                   1 - c_i of every term used (zero has no scale);
           bound   per output score, the first-order bound of the float32 face's relative error against this face (`term_ulps`),
                   0 for a score that was not decayed.  The minimum needs no margin of its own: min is 1-Lipschitz, so the two
                   faces' minima differ by no more than the terms do -- the bound of a score is the largest bound among the terms
                   that lie within that distance of the minimum.
"""
import numpy as np

import nms_rule_oracle as NR
from soft_nms_oracle import EXPF_ULPS, measure_ulps

F32 = np.float32
METHODS = ("gaussian", "linear")
U = 2.0 ** -24
BLOCK = 512                 # columns per step of the pair passes (a [n, BLOCK] float64 table at a time)


def term_ulps(method, c, m, sigma, m_ulps=0.0):
    """Units of 2^-24 of relative error of one float32 term t_ij against the float64 one, first order; arrays broadcast.
    gaussian: a = fl(c * c), b = fl(m * m) carry 2^-24 relative each, the difference and the quotient x = (a - b) / sigma one more
    each: x is off by at most (a + b) / sigma + 2 |x| units absolute, which is the relative error it gives exp(x); expf is within
    EXPF_ULPS ulp, an ulp being at most 2 units.  linear: fl(1 - m), fl(1 - c) and the quotient: 3.  A measure that is off by m_ulps
    units (`measure_ulps`; c is a measure) moves x by (2 c + 2 m) / sigma * m_ulps, and 1 - m, 1 - c by m_ulps / (1 - m), m_ulps /
    (1 - c) relative."""
    c = np.asarray(c, np.float64); m = np.asarray(m, np.float64)
    if method == "gaussian":
        a, b = c * c, m * m
        return (a + b) / sigma + 2.0 * np.abs(a - b) / sigma + 2.0 * EXPF_ULPS + (2.0 * c + 2.0 * m) / sigma * m_ulps
    with np.errstate(divide="ignore"):
        return 3.0 + m_ulps / np.maximum(1.0 - m, 1e-30) + m_ulps / np.maximum(1.0 - c, 1e-30)


def global_bound(sigma=0.5, method="gaussian"):
    """The bound of any score under a measure that is the same bits on both sides (c, m in [0, 1]): one term and the product."""
    return (float(term_ulps(method, 1.0, 1.0, sigma)) + 2.0 / sigma + 1.0) * U


def _group(pb, s, method, sig, kind, beta, W, want_bound):
    """One interacting group in order: boxes pb [n, 4], scores s [n] (float32) -> (w [n] in W, decayed [n], c [n], bound units [n])."""
    n = len(s)
    mp = np.zeros((n, n), F32)                                  # m+_ij for i < j
    for i in range(n - 1):
        m = NR.measure(pb[i], pb[i + 1:], kind, beta, F32)
        mp[i, i + 1:] = np.where(m > 0, m, F32(0))              # (NaN > 0 is False)
    c = mp.max(axis=0) if n else np.zeros(0, F32)               # column j: over i < j (the rest is 0, as is "no such k")
    d = np.ones(n, W)
    ulps = np.zeros(n, np.float64)
    mu = measure_ulps(kind, beta)
    cw = c.astype(W)
    rows = np.arange(n)[:, None]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for j0 in range(0, n, BLOCK):
            j1 = min(n, j0 + BLOCK)
            m = mp[:, j0:j1].astype(W)
            cc = cw[:, None]
            if method == "gaussian":
                t = np.exp(((cc * cc - m * m) / sig).astype(W)).astype(W)
                used = rows < np.arange(j0, j1)[None, :]
            else:
                t = ((W(1) - m) / (W(1) - cc)).astype(W)
                used = (rows < np.arange(j0, j1)[None, :]) & (cc < W(1))
            t = np.where(used, t, W(np.inf))
            dj = t.min(axis=0)
            dj = np.where(used.any(axis=0), dj, W(1)).astype(W)
            d[j0:j1] = dj
            if want_bound:
                e = np.where(used, term_ulps(method, cc, m, float(sig), mu), 0.0)
                near = used & (t <= dj[None, :].astype(np.float64) * (1.0 + 2.0 * e.max(axis=0)[None, :] * U))
                ulps[j0:j1] = np.where(near, e, 0.0).max(axis=0)
    w = (s.astype(W) * d).astype(W)
    decayed = d != W(1)
    return w, decayed, c, np.where(decayed, ulps + 1.0, 0.0)    # (+ the product)


def matrix_nms(boxes, scores, per_class=100, total=100, score_thr=0.3, kind="iou", beta=1.0, agnostic=False, method="gaussian",
               sigma=0.5, min_score=None, top_k=4096, face="f32"):
    """boxes [N, nbox, 4] normalised, scores [N, nbox, C] -> (nmsed_boxes [N, T, 4] clipped, nmsed_scores [N, T] (float32 for face
    'f32', float64 for 'f64'), nmsed_classes [N, T], valid [N] int32, kept_idx [N, T] int32 (-1 padded), margin, bound [N, T])."""
    assert method in METHODS and kind in NR.KINDS and face in ("f32", "f64") and 1 <= top_k
    boxes = np.asarray(boxes, F32)
    scores = np.asarray(scores, F32)
    n, nbox, ncls = scores.shape
    T = total
    W = F32 if face == "f32" else np.float64
    sthr = F32(score_thr)
    sig = W(F32(sigma))
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
        s = sc[bi, ci]
        pb = boxes[b, bi]
        w = np.zeros(len(s), W); decayed = np.zeros(len(s), bool); ulps = np.zeros(len(s), np.float64)
        groups = [np.arange(len(s))] if agnostic else [np.nonzero(ci == c)[0] for c in np.unique(ci)]
        for g in groups:
            w[g], decayed[g], c, ulps[g] = _group(pb[g], s[g], method, sig, kind, beta, W, face == "f64")
            if face == "f64" and method == "linear" and len(g) > 1:
                cu = c[:-1].astype(np.float64)             # (the last one of a group has nobody behind it)
                cu = cu[cu < 1.0]
                if cu.size:
                    margin = min(margin, float(np.min(1.0 - cu)))
        live = np.nonzero(w > floor)[0]
        walk = live[np.lexsort((ci[live], bi[live], -w[live].astype(np.float64)))]
        count = np.zeros(ncls, np.int64)
        k = 0
        seen = 0                                           # walk[:seen]: up to the first one not taken
        for seen, j in enumerate(walk, 1):
            if k == T:
                break
            if count[ci[j]] >= per_class:
                continue                                   # skipped: it has decayed the others all the same
            count[ci[j]] += 1
            out_b[b, k] = np.clip(pb[j], F32(0), F32(1))
            out_s[b, k] = w[j]; out_c[b, k] = ci[j]; out_i[b, k] = bi[j]
            out_bound[b, k] = ulps[j] * U * 1.001
            k += 1
        out_v[b] = k
        if face == "f64":
            part = walk[:seen]
            ws = w[part].astype(np.float64)
            if len(part) > 1:
                either = decayed[part][1:] | decayed[part][:-1]
                gap = (np.abs(np.diff(ws)) / np.maximum(ws[:-1], ws[1:]))[either]
                if gap.size:
                    margin = min(margin, float(gap.min()))
            at_floor = np.nonzero(decayed)[0] if k < T else part[decayed[part]]
            if at_floor.size and floor > 0:
                margin = min(margin, float(np.min(np.abs(w[at_floor].astype(np.float64) - float(floor))) / float(floor)))
    return out_b, out_s, out_c, out_v, out_i, margin, out_bound
