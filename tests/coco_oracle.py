"""COCOeval's bbox protocol without crowd regions, restated in its own loop form -- `evaluate_img` / `accumulate` / `summarize` --
independently of yolo4hip/cocoeval.py and of the two-candidate form csrc/coco_match.hip walks: ground-truth rows stably sorted
by the ignore flag, `iou >= best` updates, a break at the first ignored row once a non-ignored one is held; per-image lists cut
to the largest maxDet before the matching and to each maxDet when accumulating.  Python floats on float32 inputs widened exactly.

Boxes are (x1, y1, x2, y2): area = (x2 - x1) * (y2 - y1); iw = min(dx2, gx2) - max(dx1, gx1), ih likewise, IoU 0 when either is
<= 0, else i = iw * ih, i / (da + ga - i).  One project rule on top of COCO: a detection with a NaN score takes no part."""
import numpy as np

from map_oracle import pixel_boxes  # noqa: F401  (float32 product box * scale, shared with the VOC oracle)

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def area(b):
    return (b[2] - b[0]) * (b[3] - b[1])


def iou(d, g):
    iw = min(d[2], g[2]) - max(d[0], g[0])
    if iw <= 0:
        return 0.0
    ih = min(d[3], g[3]) - max(d[1], g[1])
    if ih <= 0:
        return 0.0
    i = iw * ih
    u = area(d) + area(g) - i
    return i / u


def _image(boxes_px, scores, classes, gt):
    """-> (dets: dicts id (slot + 1), box, score, cls; gts: dicts id (row + 1), box, cls), Python floats."""
    k, m = len(scores), len(gt)
    bb = np.asarray(boxes_px, dtype=np.float32).reshape(k, 4)
    gg = np.asarray(gt, dtype=np.float32).reshape(m, 5)
    dets = [{"id": d + 1, "box": [float(v) for v in bb[d]], "score": float(np.float32(scores[d])), "cls": int(classes[d])}
            for d in range(k)]
    dets = [d for d in dets if d["score"] == d["score"]]
    gts = [{"id": g + 1, "box": [float(v) for v in gg[g, :4]], "cls": int(gg[g, 4])} for g in range(m)]
    return dets, gts


def evaluate_img(dets, gts, cat, a_rng, max_det, iou_thrs):
    """COCOeval.evaluateImg for one image and category -> None, or dict dtIds, dtMatches [T,D], dtIgnore [T,D], dtScores, gtIds,
    gtIgnore (rows in the sorted order)."""
    gt = [dict(g) for g in gts if g["cls"] == cat]
    dt = [d for d in dets if d["cls"] == cat]
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g["_ignore"] = 1 if (area(g["box"]) < a_rng[0] or area(g["box"]) > a_rng[1]) else 0
    gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    ious = [[iou(d["box"], g["box"]) for g in gt] for d in dt]
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm, dtm = np.zeros((T, G), dtype=np.int64), np.zeros((T, D), dtype=np.int64)
    gt_ig = np.array([g["_ignore"] for g in gt], dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for tind, t in enumerate(iou_thrs):
        for dind, d in enumerate(dt):
            best = min([float(t), 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind, gind] > 0:                         # already matched (no crowd rows here)
                    continue
                if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                    break                                       # a regular row is held: stop at the first ignored one
                if ious[dind][gind] < best:
                    continue
                best = ious[dind][gind]
                m = gind
            if m == -1:
                continue
            dt_ig[tind, dind] = gt_ig[m]
            dtm[tind, dind] = gt[m]["id"]
            gtm[tind, m] = d["id"]
    out_of_range = np.array([area(d["box"]) < a_rng[0] or area(d["box"]) > a_rng[1] for d in dt], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out_of_range, T, 0)))
    return {"dtIds": [d["id"] for d in dt], "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "dtIgnore": dt_ig,
            "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig}


def match_image(boxes_px, scores, classes, gt, area_ranges, thresholds):
    """What one workgroup of y4_coco_match writes for one image (the valid slots / counted rows only) -> (dt_match uint32 [A,k],
    dt_ignore uint32 [A,k], cls_rank int32 [k], gt_ignore uint32 [m], match_row int32 [A,T,k]): `evaluate_img` per class and
    range with no maxDet cut, scattered back to slots and rows."""
    k, m = len(scores), len(gt)
    A, T = len(area_ranges), len(thresholds)
    dets, gts = _image(boxes_px, scores, classes, gt)
    dt_match, dt_ignore = np.zeros((A, k), dtype=np.uint32), np.zeros((A, k), dtype=np.uint32)
    cls_rank, gt_ignore = np.full(k, -1, dtype=np.int32), np.zeros(m, dtype=np.uint32)
    match_row = np.full((A, T, k), -1, dtype=np.int32)
    for cat in sorted({d["cls"] for d in dets} | {g["cls"] for g in gts}):
        for a, a_rng in enumerate(area_ranges):
            e = evaluate_img(dets, gts, cat, a_rng, 10 ** 9, thresholds)
            for pos, did in enumerate(e["dtIds"]):
                cls_rank[did - 1] = pos
                for t in range(T):
                    if e["dtMatches"][t, pos]:
                        dt_match[a, did - 1] |= np.uint32(1 << t)
                        match_row[a, t, did - 1] = e["dtMatches"][t, pos] - 1
                    if e["dtIgnore"][t, pos]:
                        dt_ignore[a, did - 1] |= np.uint32(1 << t)
            for gid, ig in zip(e["gtIds"], e["gtIgnore"]):
                if ig:
                    gt_ignore[gid - 1] |= np.uint32(1 << a)
    return dt_match, dt_ignore, cls_rank, gt_ignore, match_row


def accumulate(eval_imgs, n_images, K, iou_thrs, rec_thrs, area_ranges, max_dets):
    """COCOeval.accumulate: eval_imgs[k][a][i] from `evaluate_img` at max_dets[-1] -> (precision [T,R,K,A,M], recall [T,K,A,M])."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_ranges), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [eval_imgs[k][a][i] for i in range(n_images)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp, fp = np.array(tp), np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def summarize(precision, recall, iou_thrs, max_dets):
    """COCOeval.summarize's twelve numbers, in its order (ranges all / small / medium / large = 0..3)."""
    def one(ap, iou_thr=None, a=0, m=len(max_dets) - 1):
        if ap:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == np.asarray(iou_thrs))[0]]
            s = s[:, :, :, a, m]
        else:
            s = recall[:, :, a, m]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    return [one(1), one(1, iou_thr=.5), one(1, iou_thr=.75), one(1, a=1), one(1, a=2), one(1, a=3),
            one(0, m=0), one(0, m=1), one(0, m=2), one(0, a=1), one(0, a=2), one(0, a=3)]


def tables(images, K, iou_thrs=IOU_THRS, area_ranges=AREA_RNG, max_dets=MAX_DETS, rec_thrs=REC_THRS):
    """images: per image (boxes_px float32 [k,4], scores [k], classes [k], gt float32 [m,5]) in annotation order ->
    (precision, recall): evaluate_img per (class, range, image) at max_dets[-1], then accumulate."""
    parsed = [_image(*im) for im in images]
    eval_imgs = [[[evaluate_img(d, g, k, a_rng, max_dets[-1], iou_thrs) for d, g in parsed] for a_rng in area_ranges]
                 for k in range(K)]
    return accumulate(eval_imgs, len(images), K, iou_thrs, rec_thrs, area_ranges, max_dets)


def evaluate(images, K):
    """`tables` under COCO's own parameters and `summarize` -> (precision, recall, stats)."""
    precision, recall = tables(images, K)
    return precision, recall, summarize(precision, recall, IOU_THRS, MAX_DETS)
