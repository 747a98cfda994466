"""VOC mAP from per-detection flags: the host half of `Yolov4.evaluate_map`.

`y4_map_match` decides on the device, per image and per IoU threshold, which kept detections are true positives (the matching
loop of `evalmap.eval_map`, reference models.py:282-330).  What is left of `eval_map` is bookkeeping over the whole dataset --
the per-class confidence sort, the running tp / fp, recall, precision and `voc_ap` -- and that is `MapAccumulator`: it takes
each batch's `scores`, `classes`, `valid` and `tp_mask` (one device-to-host copy, no boxes) and repeats `eval_map`'s list
arithmetic, so that the numbers are `eval_map`'s with `==`, not approximately.

Order rules taken over from `eval_map`:
  * classes are those present in the ground truth, sorted by name; mAP is the mean over them;
  * a class's detections are sorted by confidence descending with a STABLE sort over the order `eval_map` reads them in:
    prediction files in `sorted(glob(...))` order -- the string order of `stem + ".txt"`, so that "a-b" comes before "a" --
    then line order, which is slot order.
"""
from .evalmap import voc_ap


class MapAccumulator:
    def __init__(self, class_names, iou_thresholds=(0.5,)):
        self.class_names = list(class_names)
        self.iou_thresholds = [float(t) for t in iou_thresholds]
        if not 1 <= len(self.iou_thresholds) <= 16:
            raise ValueError(f"1..16 IoU thresholds, got {len(self.iou_thresholds)}")
        self._images = {}          # stem -> (confidences, class names, tp masks of the valid slots, ground-truth class names)

    def add(self, stems, scores, classes, valid, tp_mask, gt_classes_per_image):
        """One batch: stems [n]; scores, classes [n, max_total]; valid [n]; tp_mask [n, max_total] (bit t: true positive at
        iou_thresholds[t]); gt_classes_per_image: per image the class ids of its ground-truth boxes."""
        if not (len(stems) == len(scores) == len(classes) == len(valid) == len(tp_mask) == len(gt_classes_per_image)):
            raise ValueError("MapAccumulator.add: the batch's arrays differ in length")
        for i, stem in enumerate(stems):
            if stem in self._images:
                raise ValueError(f"two images with the stem {stem!r}")
            nb = int(valid[i])
            self._images[stem] = ([float(s) for s in scores[i][:nb]],
                                  [self.class_names[int(c)] for c in classes[i][:nb]],
                                  [int(m) for m in tp_mask[i][:nb]],
                                  [self.class_names[int(c)] for c in gt_classes_per_image[i]])

    def result(self):
        """-> the keys `eval_map` returns (mAP, ap, tp, fp, n_gt, n_images, n_det) at iou_thresholds[0], plus
        per_threshold {thr: {mAP, ap, tp, fp}} and mAP_mean, the mean of mAP over the thresholds."""
        order = sorted(self._images, key=lambda stem: stem + ".txt")
        n_gt, n_img, det_count = {}, {}, {}
        for stem in order:
            seen = set()
            for cls in self._images[stem][3]:
                n_gt[cls] = n_gt.get(cls, 0) + 1
                if cls not in seen:
                    seen.add(cls)
                    n_img[cls] = n_img.get(cls, 0) + 1
        if not n_gt:
            raise ValueError("MapAccumulator.result: no ground-truth box")
        gt_classes = sorted(n_gt)
        per_class = {cls: [] for cls in gt_classes}
        for stem in order:
            confs, names, masks, _ = self._images[stem]
            for conf, cls, mask in zip(confs, names, masks):
                det_count[cls] = det_count.get(cls, 0) + 1
                if cls in per_class:
                    per_class[cls].append((conf, mask))
        for cls in gt_classes:
            per_class[cls].sort(key=lambda d: d[0], reverse=True)          # stable, like eval_map
        per_threshold = {}
        for t, thr in enumerate(self.iou_thresholds):
            aps, tps, fps = {}, {}, {}
            for cls in gt_classes:
                dets = per_class[cls]
                tp = [(mask >> t) & 1 for _, mask in dets]
                fp = [1 - v for v in tp]
                n_fp = n_tp = 0
                for k in range(len(dets)):                                  # running totals
                    n_fp += fp[k]; fp[k] = n_fp
                    n_tp += tp[k]; tp[k] = n_tp
                rec = [tp[k] / n_gt[cls] for k in range(len(dets))]
                prec = [tp[k] / (fp[k] + tp[k]) for k in range(len(dets))]
                ap, _mrec, _mpre = voc_ap(rec, prec)
                aps[cls], tps[cls], fps[cls] = ap, n_tp, n_fp
            for cls in det_count:                                           # predicted, but absent from the ground truth
                tps.setdefault(cls, 0)
            per_threshold[thr] = {"mAP": sum(aps.values()) / len(gt_classes), "ap": aps, "tp": tps, "fp": fps}
        first = per_threshold[self.iou_thresholds[0]]
        return {"mAP": first["mAP"], "ap": first["ap"], "tp": first["tp"], "fp": first["fp"], "n_gt": n_gt, "n_images": n_img,
                "n_det": det_count, "per_threshold": per_threshold,
                "mAP_mean": sum(per_threshold[thr]["mAP"] for thr in self.iou_thresholds) / len(self.iou_thresholds)}
