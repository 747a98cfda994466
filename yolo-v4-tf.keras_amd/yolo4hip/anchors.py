"""Anchors from the data set: IoU k-means and a mutate-and-select evolution on the device (csrc/anchors.hip; the rule is stated in
include/yolo4hip.h "Data-set anchors" and DESIGN.md).  Darknet has `calc_anchors` for this, YOLOv5 its autoanchor step.

    wh = dataset_wh(lines, folder, cfg['img_size'])          # the (w, h) of every label box at the network input
    fit = fit_anchors(wh)                                    # k-means, then evolution; nine anchors sorted by size
    cfg = fit.config(cfg)                                    # hand THIS dict to both Yolov4(config=) and DataGenerator(config=)
    print(fit.avg_iou, fit.avg_iou_of(yolo_config['anchors']))

The pair measure is the centred IoU of `y4_loss_assign` / `data._assign` (one shared device function), so the anchor index the
search gives a box is the one the label assignment will give it.  Pretrained heads were calibrated to the anchors they were trained
with: `Yolov4.rebase_anchors(trained_with)` moves that calibration into the tw / th biases -- explicitly, never by itself.

What runs where: the start (boxes ordered by size, nine evenly spaced ranks), the draw of the multipliers and the final sort are
host work; every pass over the boxes is a device launch.  There is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import ext, prepost
from .config import yolo_config

K = 9                             # anchors of a model: three per detection scale
MAX_BOXES = 1 << 22               # y4_anchor_*: n
MAX_SIDE = 16384.0                # ... and a side, so that every integer sum converts to float64 exactly
Q30 = 1073741824.0


def dataset_wh(annotation_lines, folder_path, img_size, letterbox=False):
    """The (w, h) every label box of a data set has at the network input -> float32 [N, 2], in annotation order.

    annotation_lines: "path x1,y1,x2,y2,cls ..." as `DataGenerator` reads them; img_size: a side, (H, W) or (H, W, 3).  Only the
    image headers are read.  Stretch (default): the float32 expressions of `DataGenerator.get_data` and `data._assign` --
    x * float32(W / w_img), then x2 - x1 -- so the values are the `wh` the label assignment sees, bit for bit.  letterbox=True: the
    scale of `prepost.letterbox_rect` on both axes, applied as `augment.transform_boxes` applies it (float32-rounded scale, product
    and pad offset in float64, one cast to float32), then x2 - x1 in float32.  Every box is kept -- no shuffle, no cut to
    max_boxes, no clipping -- except rows with w <= 0 or h <= 0; a side that is not finite or exceeds 16384 raises ValueError."""
    if isinstance(img_size, (tuple, list, np.ndarray)):
        H, W = int(img_size[0]), int(img_size[1])
    else:
        H = W = int(img_size)
    out = []
    for line in annotation_lines:
        fields = line.split()
        if not fields:
            continue
        boxes = np.array([[float(v) for v in f.split(',')] for f in fields[1:]], dtype=np.float32).reshape(-1, 5)
        if len(boxes) == 0:
            continue
        ih, iw = prepost.image_hw(os.path.join(folder_path, fields[0]))   # the header: no pixel is decoded
        if letterbox:
            out_h, out_w, top, left = prepost.letterbox_rect(ih, iw, H, W)
            sx, sy = float(np.float32(out_w / iw)), float(np.float32(out_h / ih))
            b = boxes.astype(np.float64)
            xs = (b[:, [0, 2]] * sx + left).astype(np.float32)
            ys = (b[:, [1, 3]] * sy + top).astype(np.float32)
        else:
            xs = boxes[:, [0, 2]] * (W / iw)                              # float32 products, as get_data's
            ys = boxes[:, [1, 3]] * (H / ih)
        wh = np.stack((xs[:, 1] - xs[:, 0], ys[:, 1] - ys[:, 0]), axis=1).astype(np.float32)
        if not np.all(np.isfinite(wh)) or np.any(wh > MAX_SIDE):
            raise ValueError(f"{fields[0]}: a box side is not finite or exceeds {int(MAX_SIDE)} px at the network input")
        out.append(wh[(wh[:, 0] > 0) & (wh[:, 1] > 0)])
    return np.concatenate(out, axis=0) if out else np.zeros((0, 2), dtype=np.float32)


def by_size(wh):
    """The order (float32 area w * h, w, h) ascending: of the boxes for the start, of the anchors at the end."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    return np.lexsort((wh[:, 1], wh[:, 0], wh[:, 0] * wh[:, 1]))


def start_anchors(wh, k=K):
    """The deterministic start: anchor j is the box at rank ((2j + 1) n) // (2k) of the boxes ordered by size."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    order, n = by_size(wh), len(wh)
    return np.ascontiguousarray(wh[order[[((2 * j + 1) * n) // (2 * k) for j in range(k)]]], dtype=np.float32)


def draw_mult(seed, generations, population, k=K, sigma=0.1):
    """The multipliers of the evolution, float32 [G, P, k, 2], from numpy.random.default_rng(seed): a mask with probability 0.9,
    then 1 + mask * normal * sigma clipped to [0.3, 3.0] (YOLOv5's mutation) -- all drawn up front, so a seed fixes the search."""
    rng = np.random.default_rng(seed)
    shape = (int(generations), int(population), int(k), 2)
    mask = rng.random(shape) < 0.9
    return np.clip(1 + mask * rng.standard_normal(shape) * sigma, 0.3, 3.0).astype(np.float32)


def _check_wh(wh):
    wh = np.ascontiguousarray(wh, dtype=np.float32)
    if wh.ndim != 2 or wh.shape[1] != 2 or not 1 <= len(wh) <= MAX_BOXES:
        raise ValueError(f"wh must be [n, 2] with 1 <= n <= 2^22, got {wh.shape}")
    if not np.all(np.isfinite(wh)) or np.any(wh <= 0) or np.any(wh > MAX_SIDE):
        raise ValueError(f"every box side must be finite and in (0, {int(MAX_SIDE)}]")
    return wh


def _check_anchors(anchors, what):
    a = np.ascontiguousarray(np.asarray(anchors, dtype=np.float32).reshape(-1))
    if a.size != 2 * K or not np.all(np.isfinite(a)) or np.any(a <= 0) or np.any(a > MAX_SIDE):
        raise ValueError(f"{what}: nine (w, h) pairs, finite and in (0, {int(MAX_SIDE)}], expected")
    return a.reshape(K, 2)


class _Device:
    """The boxes on the device and the three entry points over them (any k; the facade below is fixed at nine)."""

    def __init__(self, wh, device=None):
        import torch
        self.torch, self.lib = torch, ext.load()
        if not torch.cuda.is_available():
            raise RuntimeError("yolo4hip needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.n = len(wh)
        self.wh = torch.tensor(wh, dtype=torch.float32, device=self.device)      # (a copy: the caller's array may be read-only)

    def _up(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def step(self, anchors, with_assign=False):
        """-> (next float32 [k,2], stats int64 [1 + 3k], assign uint8 [n] or None) of one Lloyd step from `anchors`."""
        torch = self.torch
        a = self._up(anchors, np.float32).reshape(-1, 2)
        k = a.shape[0]
        nxt = torch.empty_like(a)
        stats = torch.empty(1 + 3 * k, dtype=torch.int64, device=self.device)
        assign = torch.empty(self.n, dtype=torch.uint8, device=self.device) if with_assign else None
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_anchor_step(ext.ptr(self.wh), self.n, ext.ptr(a), k, ext.ptr(nxt), ext.ptr(stats), ext.ptr(assign),
                                              ext.stream_ptr()))
        return nxt.cpu().numpy(), stats.cpu().numpy(), None if assign is None else assign.cpu().numpy()

    def fitness(self, sets):
        """sets [P, k, 2] -> int64 [P]."""
        torch = self.torch
        s = self._up(sets, np.float32)
        P, k = s.shape[0], s.shape[1]
        f = torch.empty(P, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_anchor_fitness(ext.ptr(self.wh), self.n, ext.ptr(s), P, k, ext.ptr(f), ext.stream_ptr()))
        return f.cpu().numpy()

    def evolve(self, best, f_best, mult):
        """mult float32 [G, P, k, 2] -> (best float32 [k,2], F_best int, F_hist int64 [G,P], accepted int32 [G])."""
        torch = self.torch
        m = self._up(mult, np.float32)
        G, P, k = m.shape[0], m.shape[1], m.shape[2]
        b = self._up(best, np.float32).reshape(k, 2)
        fb = self._up(np.array([f_best]), np.int64)
        hist = torch.empty((G, P), dtype=torch.int64, device=self.device)
        acc = torch.empty(G, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_anchor_evolve(ext.ptr(self.wh), self.n, ext.ptr(b), ext.ptr(fb), ext.ptr(m), G, P, k, ext.ptr(hist),
                                                ext.ptr(acc), ext.stream_ptr()))
        return b.cpu().numpy(), int(fb.cpu().numpy()[0]), hist.cpu().numpy(), acc.cpu().numpy()


class AnchorFit:
    """What `fit_anchors` found.  anchors float32 [9,2] sorted by (area, w, h) -- position decides the detection scale; avg_iou
    the mean best IoU of the boxes under them, avg_iou_kmeans the same before the evolution; counts int64 [9] boxes per anchor and
    assign uint8 [n] the anchor of every box (what `y4_loss_assign` will give it: scale = index // 3, anchor = index % 3);
    iterations / converged: the Lloyd steps run, and whether a step returned its input bit for bit; accepted int32 [G]: per
    generation the winning candidate, or -1; fitness / fitness_kmeans / f_hist: the int64 sums behind the averages."""

    def __init__(self, dev, **fields):
        self._dev = dev
        self.__dict__.update(fields)

    def avg_iou_of(self, anchors):
        """The same measure for any nine anchors (e.g. config['anchors']) on these boxes, computed on the device."""
        a = _check_anchors(anchors, "avg_iou_of")
        return int(self._dev.fitness(a[None])[0]) / self._dev.n / Q30

    def config(self, base=None):
        """A copy of `base` (default: the package's yolo_config) with these anchors as 18 Python floats."""
        cfg = dict(yolo_config if base is None else base)
        cfg['anchors'] = [float(v) for v in self.anchors.reshape(-1)]
        return cfg


def fit_anchors(wh, *, iters=300, generations=100, population=64, sigma=0.1, seed=0, init=None, device=None):
    """Nine anchors for the boxes `wh` (float32 [n, 2], `dataset_wh`): Lloyd steps from the size-ordered start (or `init`) until a
    step changes nothing or `iters` have run, then `generations` generations of `population` mutated candidates, of which the best
    replaces the current set only if it is strictly fitter (generations=0: k-means only).  -> AnchorFit."""
    wh = _check_wh(wh)
    if not 1 <= int(population) <= 256 or not 0 <= int(generations) <= 4096 or int(iters) < 0:
        raise ValueError("fit_anchors: population in 1..256, generations in 0..4096, iters >= 0")
    dev = _Device(wh, device)
    cur = start_anchors(wh) if init is None else _check_anchors(init, "init").copy()
    steps, converged = 0, False
    while steps < int(iters) and not converged:
        nxt, _stats, _assign = dev.step(cur)
        steps += 1
        converged = nxt.tobytes() == cur.tobytes()
        cur = nxt
    kmeans = cur
    f_km = int(dev.fitness(kmeans[None])[0])
    best, f_best = kmeans, f_km
    f_hist, accepted = np.zeros((0, int(population)), dtype=np.int64), np.zeros(0, dtype=np.int32)
    if int(generations) > 0:
        best, f_best, f_hist, accepted = dev.evolve(kmeans, f_km, draw_mult(seed, generations, population, K, sigma))
    final = np.ascontiguousarray(best[by_size(best)])
    _nxt, stats, assign = dev.step(final, with_assign=True)
    return AnchorFit(dev, anchors=final, fitness=int(stats[0]), avg_iou=int(stats[0]) / len(wh) / Q30, counts=stats[1:1 + K].copy(),
                     assign=assign, iterations=steps, converged=converged, anchors_kmeans=kmeans, fitness_kmeans=f_km,
                     avg_iou_kmeans=f_km / len(wh) / Q30, f_hist=f_hist, accepted=accepted)


def anchor_log_shift(trained_with, anchors):
    """float32 [9, 2]: log(old / new) per anchor side, computed in float64 -- what `Yolov4.rebase_anchors` adds to tw / th."""
    old = _check_anchors(trained_with, "trained_with").astype(np.float64)
    new = _check_anchors(anchors, "anchors").astype(np.float64)
    return np.log(old / new).astype(np.float32)


def head_bias_offsets(plan):
    """Where the bias rows of the three detection convs (93 / 101 / 109: the convs without batch norm) start in the Darknet-order
    weight stream (weights.flatten), in scale order."""
    offs, off = [], 0
    for c in plan.convs:
        if not c.bn:
            offs.append(off)
        off += (4 * c.cout if c.bn else c.cout) + c.n_weights
    if len(offs) != 3:
        raise ValueError(f"expected three detection convs, the plan has {len(offs)}")
    return offs


def rebase_flat(flat, plan, num_classes, trained_with, anchors):
    """The host part of `Yolov4.rebase_anchors`: a copy of the Darknet-order weight stream `flat` with log(old / new) added in
    float32 to the tw / th biases (channels a * (5 + C) + 2 and + 3) of the three detection convs; nothing else moves."""
    shift = anchor_log_shift(trained_with, anchors)
    out = np.array(flat, dtype=np.float32, copy=True)
    nf = 5 + int(num_classes)
    for s, off in enumerate(head_bias_offsets(plan)):
        for a in range(3):
            for c in (0, 1):
                i = off + a * nf + 2 + c
                out[i] = np.float32(out[i] + shift[3 * s + a, c])
    return out
