"""Labels for the validation loss (reference utils.py:80-86, 121-303): `preprocess_true_boxes`, `DataGenerator`,
`read_annotation_lines`, and the sparse *responsible-cell records* the device loss works on.

`preprocess_true_boxes` gives the reference's four arrays bit for bit, its quirks included (tests/test_loss_cpu.py holds it
to fixtures the reference's own function wrote):
  * the centre is `(x1 + x2) // 2` on float32 (a floor), width / height the plain difference;
  * the cell is floor(float32(centre / side) * grid) with the product in float64 (NumPy's promotion of a float32 by an int32);
  * the anchor is the first arg-max over the 9 anchors of the IoU of the two boxes centred on each other;
  * rows with w <= 0 are dropped by compaction: the k-th VALID row's (w, h) picks the anchor, row k of the UNCOMPACTED array
    gives the cell, the label xywh and the class -- the same thing whenever the valid rows are a prefix (`DataGenerator`);
  * two boxes on one (scale, row, col, anchor): the later one's xywh stays, the class bits of both stay set.
What the reference lets through by accident is refused here with ValueError: a centre outside the grid (its IndexError, or a
silent wrap for a negative index) and a class id outside [0, num_classes).

Record format (one image, `records_from_boxes` / `records_from_dense`, and `y4_loss_assign` on the device): int32 words
  [scale, row, col, anchor, bits(x), bits(y), bits(w), bits(h), class mask word 0 .. ceil(C / 32) - 1]
sorted by (scale, row, col, anchor), at most max_boxes of them; class c is bit (c % 32) of mask word c // 32.
"""
import os

import numpy as np

from . import prepost
from .config import yolo_config

STRIDES = (8, 16, 32)
REC_HEAD = 8                      # words before the class mask


def mask_words(num_classes):
    return (int(num_classes) + 31) // 32


def record_words(num_classes):
    return REC_HEAD + mask_words(num_classes)


def read_annotation_lines(annotation_path, test_size=None, random_seed=5566):
    with open(annotation_path) as fh:
        lines = fh.readlines()
    if not test_size:
        return lines
    from sklearn.model_selection import train_test_split
    return train_test_split(lines, test_size=test_size, random_state=random_seed)


MAP_MAX_GT = 256                  # ground-truth rows per image y4_map_match takes


def read_map_annotations(annotation_lines, num_classes):
    """Annotation lines "path x1,y1,x2,y2,cls ..." as `Yolov4.export_gt` reads them, for `Yolov4.evaluate_map`: per line
    (path field, stem, boxes float32 [k, 5]) with `float(v)` values in raw-image pixels, in annotation order -- not shuffled
    and not cut to max_boxes (`DataGenerator._read` does both).  The stem is the file name up to its first dot, the name of
    the text files `export_gt` / `export_prediction` write.  ValueError: more than 256 boxes on an image, a class id outside
    [0, num_classes), two lines with the same stem."""
    out, seen = [], set()
    for line in annotation_lines:
        if not line.strip():
            continue
        fields = line.split(' ')
        name = fields[0].strip()
        stem = name.split(os.sep)[-1].split('.')[0]
        if stem in seen:
            raise ValueError(f"two annotation lines with the stem {stem!r}")
        seen.add(stem)
        rows = [[float(v) for v in obj.strip().split(',')] for obj in fields[1:] if obj.strip()]
        if len(rows) > MAP_MAX_GT:
            raise ValueError(f"{name}: {len(rows)} boxes, more than {MAP_MAX_GT}")
        for row in rows:
            if len(row) != 5 or not 0 <= int(row[4]) < num_classes:
                raise ValueError(f"{name}: box {row}: x1,y1,x2,y2,class with class in [0, {num_classes})")
        out.append((name, stem, np.array(rows, dtype=np.float32).reshape(-1, 5)))
    return out


def _assign(true_boxes, input_shape, anchors, num_classes):
    """The assignment of every used row -> (xy [bs,mb,2], wh [bs,mb,2] float32, per image a list of
    (scale, row, col, anchor, row index k, class id) in row order)."""
    boxes = np.array(true_boxes, dtype=np.float32)
    if boxes.ndim != 3 or boxes.shape[-1] != 5:
        raise ValueError(f"true_boxes must be [batch, max_boxes, 5], got {boxes.shape}")
    hw = np.array(input_shape, dtype=np.int32)
    if hw.shape != (2,) or np.any(hw <= 0) or np.any(hw % STRIDES[-1]):
        raise ValueError(f"input_shape {tuple(input_shape)}: (H, W), positive multiples of {STRIDES[-1]}")
    anchors = np.asarray(anchors)
    if anchors.shape != (9, 2):
        raise ValueError(f"anchors must be (9, 2), got {anchors.shape}")
    xy = (boxes[..., 0:2] + boxes[..., 2:4]) // 2
    wh = boxes[..., 2:4] - boxes[..., 0:2]
    norm = np.empty_like(xy)
    norm[...] = xy / hw[::-1]                                   # float64 quotient, stored as float32
    grids = [hw // s for s in STRIDES]                          # int32 (rows, columns)
    half_a = anchors / 2.
    area_a = anchors[:, 0] * anchors[:, 1]
    out = []
    for b in range(boxes.shape[0]):
        sel = wh[b, wh[b, :, 0] > 0]
        hits = []
        if len(sel):
            half_b = sel[:, None, :] / 2.
            lo = np.maximum(-half_b, -half_a[None])
            hi = np.minimum(half_b, half_a[None])
            inter = np.prod(np.maximum(hi - lo, 0.), axis=-1)
            area_b = sel[:, 0] * sel[:, 1]
            iou = inter / (area_b[:, None] + area_a[None] - inter)
            best = np.argmax(iou, axis=-1)
            for k in range(len(sel)):
                s, a = divmod(int(best[k]), 3)
                col = int(np.floor(norm[b, k, 0] * grids[s][1]))
                row = int(np.floor(norm[b, k, 1] * grids[s][0]))
                cls = int(boxes[b, k, 4].astype(np.int32))
                if not (0 <= row < grids[s][0] and 0 <= col < grids[s][1]):
                    raise ValueError(f"image {b} box {k}: centre ({xy[b, k, 0]}, {xy[b, k, 1]}) is outside the "
                                     f"{int(hw[0])} x {int(hw[1])} input")
                if not 0 <= cls < num_classes:
                    raise ValueError(f"image {b} box {k}: class id {cls} outside [0, {num_classes})")
                hits.append((s, row, col, a, k, cls))
        out.append(hits)
    return xy, wh, grids, out


def preprocess_true_boxes(true_boxes, input_shape, anchors, num_classes):
    """true_boxes [bs, max_boxes, 5] (x1, y1, x2, y2, class in network-input pixels), input_shape (H, W) ->
    ([y_s, y_m, y_l] dense labels [bs, gh, gw, 3, 5 + C] float32, y_true_boxes_xywh [bs, max_boxes, 4] float32)."""
    xy, wh, grids, hits = _assign(true_boxes, input_shape, anchors, num_classes)
    bs = xy.shape[0]
    y_true = [np.zeros((bs, int(g[0]), int(g[1]), 3, 5 + num_classes), dtype=np.float32) for g in grids]
    for b, rows in enumerate(hits):
        for s, row, col, a, k, cls in rows:
            cell = y_true[s][b, row, col, a]
            cell[0:2] = xy[b, k]
            cell[2:4] = wh[b, k]
            cell[4] = 1
            cell[5 + cls] = 1
    return y_true, np.concatenate((xy, wh), axis=-1)


def _pack(entries, num_classes):
    """{(scale, row, col, anchor): (xywh float32[4], mask uint32[mw])} -> sorted int32 records [m, 8 + mw]."""
    mw = mask_words(num_classes)
    rec = np.zeros((len(entries), REC_HEAD + mw), dtype=np.int32)
    for i, key in enumerate(sorted(entries)):
        xywh, mask = entries[key]
        rec[i, 0:4] = key
        rec[i, 4:8] = np.asarray(xywh, dtype=np.float32).view(np.int32)
        rec[i, 8:] = mask.view(np.int32)
    return rec


def records_from_boxes(true_boxes, input_shape, anchors, num_classes):
    """-> (per image an int32 array [m_i, 8 + mw] of records, y_true_boxes_xywh): what `y4_loss_assign` computes."""
    xy, wh, _grids, hits = _assign(true_boxes, input_shape, anchors, num_classes)
    mw = mask_words(num_classes)
    recs = []
    for b, rows in enumerate(hits):
        entries = {}
        for s, row, col, a, k, cls in rows:
            mask = entries[(s, row, col, a)][1] if (s, row, col, a) in entries else np.zeros(mw, dtype=np.uint32)
            mask[cls // 32] |= np.uint32(1 << (cls % 32))
            entries[(s, row, col, a)] = (np.concatenate((xy[b, k], wh[b, k])), mask)
        recs.append(_pack(entries, num_classes))
    return recs, np.concatenate((xy, wh), axis=-1)


def records_from_dense(y_true, num_classes):
    """Dense labels (3 arrays [bs, gh, gw, 3, 5 + C]) -> per image the records of the cells with label[..., 4] == 1.
    Label values other than 0 and 1 (smoothed labels) cannot be carried by the class bit mask: ValueError."""
    if len(y_true) != 3:
        raise ValueError("three label arrays expected (small, medium, large boxes)")
    y_true = [np.asarray(y, dtype=np.float32) for y in y_true]
    bs = y_true[0].shape[0]
    mw = mask_words(num_classes)
    entries = [dict() for _ in range(bs)]
    for s, y in enumerate(y_true):
        if y.ndim != 5 or y.shape[0] != bs or y.shape[3] != 3 or y.shape[4] != 5 + num_classes:
            raise ValueError(f"label {s}: shape {y.shape}, expected [{bs}, gh, gw, 3, {5 + num_classes}]")
        flags = y[..., 4:]
        if not np.all((flags == 0) | (flags == 1)):
            raise ValueError(f"label {s}: objectness and class values must be 0 or 1 (smoothed labels are not supported)")
        for b, row, col, a in zip(*np.nonzero(y[..., 4] == 1)):
            cell = y[b, row, col, a]
            mask = np.zeros(mw, dtype=np.uint32)
            for cls in np.nonzero(cell[5:])[0]:
                mask[cls // 32] |= np.uint32(1 << (int(cls) % 32))
            entries[b][(s, int(row), int(col), int(a))] = (cell[0:4].copy(), mask)
    return [_pack(e, num_classes) for e in entries]


def dense_from_records(records, input_shape, num_classes):
    """The inverse of `records_from_dense`: per-image records -> the three dense label arrays."""
    hw = np.array(input_shape, dtype=np.int32)
    y_true = [np.zeros((len(records), int(hw[0]) // s, int(hw[1]) // s, 3, 5 + num_classes), dtype=np.float32) for s in STRIDES]
    for b, rec in enumerate(records):
        for r in np.asarray(rec, dtype=np.int32):
            cell = y_true[r[0]][b, r[1], r[2], r[3]]
            cell[0:4] = r[4:8].view(np.float32)
            cell[4] = 1
            mask = r[8:].view(np.uint32)
            for cls in range(num_classes):
                if (int(mask[cls // 32]) >> (cls % 32)) & 1:
                    cell[5 + cls] = 1
    return y_true


def pad_records(records, max_boxes, num_classes):
    """Per-image records -> (int32 [n, max_boxes, 8 + mw] zero padded, int32 counts [n]): the device layout."""
    rw = record_words(num_classes)
    out = np.zeros((len(records), int(max_boxes), rw), dtype=np.int32)
    cnt = np.zeros(len(records), dtype=np.int32)
    for b, rec in enumerate(records):
        if len(rec) > max_boxes:
            raise ValueError(f"image {b}: {len(rec)} responsible cells, more than max_boxes = {max_boxes}")
        out[b, :len(rec)] = rec
        cnt[b] = len(rec)
    return out, cnt


class DataGenerator:
    """The reference's Keras `Sequence` (utils.py:121-212) without Keras: `len(gen)` batches, `gen[i]` ->
    ([X, y_s, y_m, y_l, y_true_boxes_xywh], zeros(batch)).  img_size, batch_size (x num_gpu) and anchors come from `config`
    (default: the package's `yolo_config`); images are read and stretched through `prepost`.  `boxes(i)` gives batch i as
    (X, [n, max_boxes, 5] boxes) -- what `Yolov4.evaluate` uploads instead of the dense labels.

    augment=None (default): the reference's plain stretch, every epoch the same pixels.  augment=AugmentConfig(...)
    (yolo4hip.augment) with seed=: every batch draws one parameter row per image from the generator's own
    `numpy.random.default_rng(seed)`; `raw(i)` gives (uint8 images, parameters, transformed boxes) for the device path of
    `Yolov4.fit` (`Engine.augment_u8_batch`), `boxes(i)` and `gen[i]` the same batch through `augment.augment_host` -- either
    way one draw per image in batch order, so a seed gives the same parameters on both paths.  The box shuffle and the epoch
    shuffle stay on the global `np.random`, as without augmentation.

    Mosaic: with `augment.mosaic > 0` every canvas is, with that probability, four images around a random cut
    (`augment.draw_mosaic_params`): its own image top-left and three partners drawn from the whole dataset.  `raw_mosaic(i)`
    gives (distinct uint8 images, tile_src [n,4] into them, parameters [n,4], cuts [n,2], merged boxes) for
    `Engine.mosaic_u8_batch`; `boxes(i)` and `gen[i]` build the same batch through `augment.mosaic_host`, with the same draws.
    `raw(i)` refuses such a generator: one parameter row per image cannot describe its batch."""

    def __init__(self, annotation_lines, class_name_path, folder_path, max_boxes=100, shuffle=True, config=None, augment=None,
                 seed=None):
        config = yolo_config if config is None else config
        self.annotation_lines = annotation_lines
        self.class_name_path = class_name_path
        self.num_classes = len([line.strip() for line in open(class_name_path).readlines()])
        self.num_gpu = config.get('num_gpu', 1)
        self.batch_size = config['batch_size'] * self.num_gpu
        self.target_img_size = tuple(config['img_size'])
        self.anchors = np.array(config['anchors']).reshape((9, 2))
        self.shuffle = shuffle
        self.indexes = np.arange(len(self.annotation_lines))
        self.folder_path = folder_path
        self.max_boxes = max_boxes
        self.augment = augment
        self.rng = np.random.default_rng(seed)              # augmentation parameters only
        self._sizes = {}                                    # path field -> (h, w) of the image as first read (`labels`)
        self.on_epoch_end()

    def __len__(self):
        return int(np.ceil(len(self.annotation_lines) / self.batch_size))

    def on_epoch_end(self):
        if self.shuffle:
            np.random.shuffle(self.indexes)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def raw(self, index):
        """Batch `index` of an augmenting generator -> (list of uint8 RGB images as read, parameter rows
        (augment.PARAM_DTYPE) [n], boxes float32 [n, max_boxes, 5] already on the augmented canvas)."""
        from . import augment as A
        if self.augment is None:
            raise ValueError("DataGenerator.raw: this generator does not augment (augment=None)")
        if self.augment.mosaic > 0:
            raise ValueError("DataGenerator.raw: this generator draws mosaic canvases (augment.mosaic > 0), use raw_mosaic")
        idxs = self.indexes[index * self.batch_size:(index + 1) * self.batch_size]
        read = [self._read(self.annotation_lines[j]) for j in idxs]
        imgs = [img for img, _ in read]
        hw = self.target_img_size[:2]
        params = A.draw_params(self.rng, [img.shape[:2] for img in imgs], hw, self.augment)
        y_bbox = np.zeros((len(idxs), self.max_boxes, 5), dtype=np.float32)
        for i, (img, boxes) in enumerate(read):
            y_bbox[i] = A.transform_boxes(boxes, img.shape[:2], params[i], hw, self.max_boxes)
        return imgs, params, y_bbox

    def raw_mosaic(self, index):
        """Batch `index` of a mosaic generator (augment.mosaic > 0) -> (images: the DISTINCT uint8 RGB photos of the batch,
        each read once -- the batch's own images in batch order, then the partners in the order tiles first name them;
        tile_src int64 [n,4]: per canvas and tile the index into `images`; parameter rows (augment.PARAM_DTYPE) [n,4];
        cuts int32 [n,2] as (cut_y, cut_x); boxes float32 [n, max_boxes, 5] on the mosaic canvas, `augment.mosaic_boxes`).
        A single canvas (cut (H, W)) carries its own image and row 0 in all four tiles."""
        from . import augment as A
        if self.augment is None or not self.augment.mosaic > 0:
            raise ValueError("DataGenerator.raw_mosaic: this generator draws no mosaic canvases (augment.mosaic > 0)")
        idxs = self.indexes[index * self.batch_size:(index + 1) * self.batch_size]
        hw = self.target_img_size[:2]
        slot, read = {}, []                                 # annotation line -> slot in `read`
        for j in idxs:
            slot[int(j)] = len(read)
            read.append(self._read(self.annotation_lines[j]))
        data_src, params, cuts = A.draw_mosaic_params(self.rng, len(idxs), len(self.annotation_lines), hw, self.augment)
        tile_src = np.empty((len(idxs), 4), dtype=np.int64)
        for i, j in enumerate(idxs):
            for q in range(4):
                k = int(j) if data_src[i, q] < 0 else int(data_src[i, q])
                if k not in slot:
                    slot[k] = len(read)
                    read.append(self._read(self.annotation_lines[k]))
                tile_src[i, q] = slot[k]
        y_bbox = np.zeros((len(idxs), self.max_boxes, 5), dtype=np.float32)
        for i in range(len(idxs)):
            tiles = [read[k] for k in tile_src[i]]
            y_bbox[i] = A.mosaic_boxes([b for _, b in tiles], [img.shape[:2] for img, _ in tiles], params[i], cuts[i], hw,
                                       self.max_boxes)
        return [img for img, _ in read], tile_src, params, cuts, y_bbox

    def boxes(self, index):
        if self.augment is not None and self.augment.mosaic > 0:
            from .augment import mosaic_host
            imgs, tile_src, params, cuts, y_bbox = self.raw_mosaic(index)
            X = np.empty((len(tile_src), *self.target_img_size), dtype=np.float32)
            for i in range(len(tile_src)):
                X[i] = mosaic_host([imgs[k] for k in tile_src[i]], params[i], cuts[i], self.target_img_size[:2],
                                   self.augment.pad_value) / 255.
            return X, y_bbox
        if self.augment is not None:
            from .augment import augment_host
            imgs, params, y_bbox = self.raw(index)
            X = np.empty((len(imgs), *self.target_img_size), dtype=np.float32)
            for i, img in enumerate(imgs):
                X[i] = augment_host(img, params[i], self.target_img_size[:2], self.augment.pad_value) / 255.
            return X, y_bbox
        idxs = self.indexes[index * self.batch_size:(index + 1) * self.batch_size]
        X = np.empty((len(idxs), *self.target_img_size), dtype=np.float32)
        y_bbox = np.empty((len(idxs), self.max_boxes, 5), dtype=np.float32)
        for i, j in enumerate(idxs):
            X[i], y_bbox[i] = self.get_data(self.annotation_lines[j])
        return X, y_bbox

    def __getitem__(self, index):
        X, y_bbox = self.boxes(index)
        y_tensor, y_xywh = preprocess_true_boxes(y_bbox, self.target_img_size[:2], self.anchors, self.num_classes)
        return [X, *y_tensor, y_xywh], np.zeros(len(X))

    def _read(self, annotation_line):
        """One annotation line "path x1,y1,x2,y2,cls ..." -> (uint8 RGB image as read, its boxes float32 [k, 5] in the image's
        own pixels, shuffled (global np.random) and cut to max_boxes)."""
        fields = annotation_line.split()
        img = prepost.imread_rgb(os.path.join(self.folder_path, fields[0]))
        self._sizes[fields[0]] = img.shape[:2]
        return img, self._read_boxes(fields)

    def _read_boxes(self, fields):
        """The boxes of one split annotation line, shuffled (global np.random: one draw per line with a box) and cut to max_boxes."""
        boxes = np.array([[float(v) for v in f.split(',')] for f in fields[1:]], dtype=np.float32)
        if len(boxes) > 0:
            np.random.shuffle(boxes)
            boxes = boxes[:self.max_boxes]
        return boxes

    def _stretch_boxes(self, boxes, ih, iw):
        """Boxes in the pixels of an ih x iw image -> [max_boxes, 5] at the network input (float32 products, zero padded)."""
        h, w = self.target_img_size[:2]
        box_data = np.zeros((self.max_boxes, 5))
        if len(boxes) > 0:
            boxes[:, [0, 2]] = boxes[:, [0, 2]] * (w / iw)
            boxes[:, [1, 3]] = boxes[:, [1, 3]] * (h / ih)
            box_data[:len(boxes)] = boxes
        return box_data

    def get_data(self, annotation_line):
        """One annotation line "path x1,y1,x2,y2,cls ..." -> (image [H, W, 3] in [0, 1], boxes [max_boxes, 5] scaled to it)."""
        img, boxes = self._read(annotation_line)
        ih, iw = img.shape[:2]
        h, w = self.target_img_size[:2]
        image_data = prepost.resize_bilinear(img, (w, h)) / 255.
        return image_data, self._stretch_boxes(boxes, ih, iw)

    def labels(self, index):
        """Batch `index` -> boxes float32 [n, max_boxes, 5]: `boxes(index)[1]` bit for bit, without decoding a photo, and with the
        same draws from the global np.random in the same order (the per-image box shuffle), so that a run that calls `labels`
        where another calls `boxes` stays aligned with it -- what `Yolov4.fit(cache_features=True)` does from its second epoch
        on.  The image size the stretch needs is the one this generator saw when it first read the line; for a line it has not
        read, the image header (`prepost.image_hw`: no pixel is decoded).  An augmenting generator raises ValueError: its boxes
        follow parameters drawn per batch, and its pixels differ every epoch."""
        if self.augment is not None:
            raise ValueError("DataGenerator.labels: this generator augments; its boxes come with its pixels (raw / boxes)")
        idxs = self.indexes[index * self.batch_size:(index + 1) * self.batch_size]
        y_bbox = np.empty((len(idxs), self.max_boxes, 5), dtype=np.float32)
        for i, j in enumerate(idxs):
            fields = self.annotation_lines[j].split()
            if fields[0] not in self._sizes:
                self._sizes[fields[0]] = prepost.image_hw(os.path.join(self.folder_path, fields[0]))
            y_bbox[i] = self._stretch_boxes(self._read_boxes(fields), *self._sizes[fields[0]])
        return y_bbox
