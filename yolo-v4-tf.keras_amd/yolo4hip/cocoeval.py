"""COCO-protocol AP / AR from per-detection flags: the host half of `Yolov4.evaluate_coco`.

`y4_coco_match` decides on the device, per image, area range and IoU threshold, which kept detections are matched and which are
ignored (COCOeval's `evaluateImg` for boxes, without crowd regions; the rule is stated in csrc/coco_match.hip and DESIGN.md 7i).
What is left of COCOeval is `accumulate` and `summarize`, and that is `CocoAccumulator`: NumPy only, it takes each batch's scores,
classes, valid, `cls_rank`, the two masks and `gt_ignore` (one device-to-host copy, no boxes) and follows COCOeval's arithmetic
-- float64 running sums, `np.spacing(1)` in the precision's denominator, the monotone envelope from the right, `searchsorted`
on the recall thresholds -- so that the numbers are COCOeval's, not approximately.

Per class k, range a, maxDet m and threshold t, over the images in the order they were added:
  * keep the detections of class k with 0 <= cls_rank < m (COCO cuts each (image, class) list to maxDet before matching; the
    walk is greedy in score order, so cutting afterwards changes no earlier decision);
  * sort by score descending with a stable sort;
  * tp = matched & ~ignored, fp = ~matched & ~ignored, cumulative sums as float64;
  * npig = the class's rows not ignored under a; npig == 0 leaves precision and recall at -1;
  * rc = tp / npig, pr = tp / (fp + tp + np.spacing(1)); recall[t,k,a,m] = rc[-1] (0 without detections);
  * pr made monotone from the right; precision[t,:,k,a,m] = pr[searchsorted(rc, recThrs, 'left')], 0 past the end.
"""
import numpy as np

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
REC_THRESHOLDS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))     # all, small, medium, large
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def check_params(iou_thresholds, area_ranges, max_dets):
    """-> (float64 thresholds [T], float64 ranges [A,2], tuple of ints) or ValueError: 1..16 thresholds, 1..4 ranges (lo <= hi, in
    the order all / small / medium / large), max_dets positive and ascending."""
    thr = np.array(IOU_THRESHOLDS if iou_thresholds is None else iou_thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= 16 or not np.all(np.isfinite(thr)):
        raise ValueError(f"1..16 finite IoU thresholds, got {thr.tolist()}")
    rng = np.array(AREA_RANGES if area_ranges is None else area_ranges, dtype=np.float64)
    if rng.ndim != 2 or rng.shape[1] != 2 or not 1 <= len(rng) <= 4 or np.isnan(rng).any() or (rng[:, 0] > rng[:, 1]).any():
        raise ValueError(f"area_ranges: 1..4 rows [lo, hi] with lo <= hi, got {np.asarray(area_ranges).tolist()}")
    try:
        md = tuple(int(m) for m in max_dets)
        exact = all(m == v for m, v in zip(md, max_dets))
    except (TypeError, ValueError):
        md, exact = (), False
    if not md or not exact or md[0] < 1 or any(b <= a for a, b in zip(md, md[1:])):
        raise ValueError(f"max_dets: positive integers in ascending order, got {max_dets!r}")
    return thr, rng, md


class CocoAccumulator:
    def __init__(self, class_names, iou_thresholds=None, area_ranges=None, max_dets=MAX_DETS):
        self.class_names = list(class_names)
        self.iou_thresholds, self.area_ranges, self.max_dets = check_params(iou_thresholds, area_ranges, max_dets)
        self.rec_thresholds = REC_THRESHOLDS
        self._dets, self._gts = [], []          # per image (scores, classes, cls_rank, dt_match [A,k], dt_ignore [A,k]); (classes, gt_ignore)

    def add(self, scores, classes, valid, cls_rank, dt_match, dt_ignore, gt_classes_per_image, gt_ignore):
        """One batch: scores, classes, cls_rank [n, max_total]; valid [n]; dt_match, dt_ignore uint32 [n, A, max_total] (bit t:
        matched / ignored at iou_thresholds[t] under range a); gt_classes_per_image: per image the class ids of its rows, in
        annotation order; gt_ignore uint32 [n, max_gt] (bit a: the row is ignored under range a)."""
        n = len(valid)
        if not (len(scores) == len(classes) == len(cls_rank) == len(dt_match) == len(dt_ignore) == len(gt_classes_per_image)
                == len(gt_ignore) == n):
            raise ValueError("CocoAccumulator.add: the batch's arrays differ in length")
        A = len(self.area_ranges)
        for i in range(n):
            nb = int(valid[i])
            rank = np.asarray(cls_rank[i][:nb], dtype=np.int64)
            keep = rank >= 0                                        # a slot that was not walked (NaN score) takes no part
            self._dets.append((np.asarray(scores[i][:nb], dtype=np.float64)[keep], np.asarray(classes[i][:nb]).astype(np.int64)[keep],
                               rank[keep], np.asarray(dt_match[i], dtype=np.uint32)[:A, :nb][:, keep],
                               np.asarray(dt_ignore[i], dtype=np.uint32)[:A, :nb][:, keep]))
            gcls = np.asarray(gt_classes_per_image[i]).astype(np.int64).reshape(-1)
            self._gts.append((gcls, np.asarray(gt_ignore[i][:len(gcls)], dtype=np.uint32)))

    def result(self):
        """-> the twelve summary numbers by name (STAT_NAMES), `stats` (the twelve in COCO's order), `per_class` {name: AP},
        `precision` [T,R,K,A,M], `recall` [T,K,A,M], `n_gt` and `n_det` {name: count}.  AP / AR use the last max_dets entry and
        the first range; APs / APm / APl and ARs / ARm / ARl ranges 1 / 2 / 3; AR1 / AR10 / AR100 max_dets[0] / [1] / [2]; AP50 /
        AP75 the thresholds equal to 0.5 / 0.75.  Each is the mean over the entries > -1, or -1.0 when there are none (or when
        that range, maxDet or threshold was not asked for)."""
        thr, rec, md = self.iou_thresholds, self.rec_thresholds, self.max_dets
        T, R, K, A, M = len(thr), len(rec), len(self.class_names), len(self.area_ranges), len(md)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        A0 = max(A, 1)
        scores = np.concatenate([d[0] for d in self._dets]) if self._dets else np.zeros(0)
        cls = np.concatenate([d[1] for d in self._dets]) if self._dets else np.zeros(0, np.int64)
        rank = np.concatenate([d[2] for d in self._dets]) if self._dets else np.zeros(0, np.int64)
        dtm = np.concatenate([d[3] for d in self._dets], axis=1) if self._dets else np.zeros((A0, 0), np.uint32)
        dti = np.concatenate([d[4] for d in self._dets], axis=1) if self._dets else np.zeros((A0, 0), np.uint32)
        gcls = np.concatenate([g[0] for g in self._gts]) if self._gts else np.zeros(0, np.int64)
        gign = np.concatenate([g[1] for g in self._gts]) if self._gts else np.zeros(0, np.uint32)
        bits = np.arange(T, dtype=np.uint32)[:, None]
        for k in range(K):
            mine, rows = np.nonzero(cls == k)[0], gign[gcls == k]
            if len(mine) == 0 and len(rows) == 0:
                continue
            for a in range(A):
                npig = int(np.count_nonzero(((rows >> np.uint32(a)) & np.uint32(1)) == 0))
                if npig == 0:
                    continue
                for m, max_det in enumerate(md):
                    idx = mine[rank[mine] < max_det]
                    idx = idx[np.argsort(-scores[idx], kind="mergesort")]
                    nd = len(idx)
                    if nd == 0:
                        recall[:, k, a, m], precision[:, :, k, a, m] = 0, 0
                        continue
                    matched = ((dtm[a, idx][None, :] >> bits) & np.uint32(1)).astype(bool)          # [T, nd]
                    ignored = ((dti[a, idx][None, :] >> bits) & np.uint32(1)).astype(bool)
                    tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                    fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[:, k, a, m] = rc[:, -1]
                    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                    for t in range(T):
                        at = np.searchsorted(rc[t], rec, side="left")
                        q = np.zeros(R)
                        q[at < nd] = pr[t, at[at < nd]]
                        precision[t, :, k, a, m] = q

        def mean(s):
            s = s[s > -1]
            return float(np.mean(s)) if len(s) else -1.0

        def ap(a, thr_value=None):
            if a >= A:
                return -1.0
            s = precision[:, :, :, a, M - 1]
            return mean(s if thr_value is None else s[thr == thr_value])

        def ar(a, m):
            return mean(recall[:, :, a, m]) if a < A and m < M else -1.0

        stats = [ap(0), ap(0, 0.5), ap(0, 0.75), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, M - 1), ar(2, M - 1),
                 ar(3, M - 1)]
        out = dict(zip(STAT_NAMES, stats))
        out["stats"] = stats
        out["per_class"] = {name: mean(precision[:, :, k, 0, M - 1]) for k, name in enumerate(self.class_names)}
        out["precision"], out["recall"] = precision, recall
        out["n_gt"] = {self.class_names[int(c)]: int(v) for c, v in zip(*np.unique(gcls, return_counts=True))}
        out["n_det"] = {self.class_names[int(c)]: int(v) for c, v in zip(*np.unique(cls, return_counts=True))}
        return out
