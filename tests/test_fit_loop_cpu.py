"""The loop under `Yolov4.fit` (yolo4hip/fitloop.py) on a recording engine: no GPU, no library.

Every expected record below is written out by hand from the order fit documents: per batch the generator read, the box check,
the route's pixel launch, then per chunk forward (or cache load + tail) -> assign -> one gradient call per group -> loss, one
host read, and Adam for every group or for none.  Batches are 3 images through max_batch 2 -- a chunk of 2 and a chunk of 1, the
smallest shape at which the slices, `accumulate` and the count check can go wrong -- and one batch of 1."""
import types

import numpy as np
import pytest
import torch

from yolo4hip import fitloop
from yolo4hip.engine import Engine

THR = 0.25
# what the fake's loss_device returns per image: [3 scales, 3 terms] = box, conf, class sums
TERMS = np.array([[1.0, 0.5, 0.25], [2.0, 0.125, 4.0], [0.5, 8.0, 1.0]], dtype=np.float32)
# combine_loss by hand: the terms summed over the scales, weighed 3.54 / 64.3 / 1 (reference loss.py:136-138), summed
PER_IMAGE = (1.0 + 2.0 + 0.5) * 3.54 + (0.5 + 0.125 + 8.0) * 64.3 + (0.25 + 4.0 + 1.0) * 1.0


class FakeEngine:
    """The engine methods the loop calls, each appending (name, salient arguments) to `rec`."""
    device = torch.device("cpu")
    max_batch = 2
    torch = torch
    _paired_chunks = Engine._paired_chunks                 # the real pairing over this object's `_chunks`

    def __init__(self, rec, refuse_boxes=False):
        self.rec, self.refuse_boxes = rec, refuse_boxes

    def _chunks(self, X):
        for i in range(0, len(X), self.max_batch):
            yield X[i:i + self.max_batch]

    def _check_boxes(self, boxes):
        self.rec.append(("check_boxes", len(boxes)))
        if self.refuse_boxes:
            raise ValueError("image 0 box 0: centre is outside the 160 x 160 input")
        return np.ascontiguousarray(boxes, dtype=np.float32)

    def augment_u8_batch(self, raws, params, pad_value):
        self.rec.append(("augment_u8_batch", len(raws), params, pad_value))
        return np.stack(raws)

    def mosaic_u8_batch(self, raws, tile_src, params, cuts, pad_value):
        self.rec.append(("mosaic_u8_batch", len(raws), tile_src, params, cuts, pad_value))
        return np.stack(raws)

    def forward_device(self, chunk):
        self.rec.append(("forward_device", [int(v) for v in chunk[:, 0]]))

    def store_features(self, cache, slots):
        self.rec.append(("store_features", cache, [int(v) for v in slots]))

    def load_features(self, cache, slots):
        self.rec.append(("load_features", cache, [int(v) for v in slots]))

    def forward_tail_device(self, n):
        self.rec.append(("forward_tail_device", n))

    def assign_device(self, boxes_dev):
        ids = [int(v) for v in boxes_dev[:, 0, 0]]
        self.rec.append(("assign_device", ids))
        return ("labels", ids)

    def _group_grad_device(self, g, n, boxes_dev, records, thr, img_weight, dw, accumulate, loss_scale=None, overflow=None):
        assert boxes_dev is None and thr == THR and dw is self.grads[g]
        if overflow is not None:
            assert overflow is self.overflow_seen or self.overflow_seen is None
            self.overflow_seen = overflow
        self.rec.append(("grad", g, n, records, [float(v) for v in img_weight], accumulate, loss_scale,
                         None if overflow is None else int(overflow)))

    overflow_seen = None

    def loss_device(self, n, records=None, iou_loss_thresh=None):
        assert iou_loss_thresh == THR
        self.rec.append(("loss_device", n, records))
        return torch.from_numpy(TERMS).expand(n, 3, 3).clone()

    def _group_floats(self, g):
        return {"heads": 4, "blocks": 6}[g]

    def _group_state(self, g, flat):
        return {"w": g, "t": 0}

    def _group_adam_step(self, g, state, dw, lr):
        assert dw is self.grads[g]
        state["t"] += 1
        self.rec.append(("adam", g, state["t"], lr))

    def _group_weights_to_flat(self, g, state, flat):
        self.rec.append(("weights_to_flat", g, state["w"]))


class FakeGen:
    """Batches of image ids: an image is a [1] array holding its id, its boxes a [max_boxes=1, 5] block whose first number is
    the id.  `order` is what DataGenerator calls `indexes`."""
    batch_size = 3

    def __init__(self, rec, order, augment=None, image_shift=0):
        self.rec, self.indexes, self.image_shift = rec, list(order), image_shift
        if augment is not None:
            self.augment = augment

    def __len__(self):
        return -(-len(self.indexes) // self.batch_size)

    def _ids(self, i):
        return self.indexes[i * self.batch_size:(i + 1) * self.batch_size]

    def _boxes(self, i):
        return np.array([[[k, 0, 1, 1, 0]] for k in self._ids(i)], dtype=np.float32)

    def _images(self, i):
        ids = self._ids(i)
        ids = ids + [99] * self.image_shift if self.image_shift > 0 else ids[:len(ids) + self.image_shift]
        return np.array([[k] for k in ids], dtype=np.float32)

    def boxes(self, i):
        self.rec.append(("boxes", i))
        return self._images(i), self._boxes(i)

    def labels(self, i):
        self.rec.append(("labels", i))
        return self._boxes(i)

    def raw(self, i):
        self.rec.append(("raw", i))
        return list(self._images(i)), f"params{i}", self._boxes(i)

    def raw_mosaic(self, i):
        self.rec.append(("raw_mosaic", i))
        return list(self._images(i)), f"tiles{i}", f"params{i}", f"cuts{i}", self._boxes(i)

    def on_epoch_end(self):
        self.rec.append(("gen.on_epoch_end",))


class FakePolicy:
    """`update` answers from a list, one entry per batch, and halves the scale on a False like a dynamic scale."""

    def __init__(self, rec, answers, scale=8.0):
        self.rec, self.answers, self.scale = rec, list(answers), scale

    def update(self, overflow):
        self.rec.append(("policy.update", overflow))
        ok = self.answers.pop(0)
        if not ok:
            self.scale /= 2
        return ok


def _run(rec, gen, groups, epochs=1, initial_epoch=0, policy=None, cache=None, callbacks=None, validate=None, val_names=(),
         eng=None, learning_rate=0.5):
    eng = eng or FakeEngine(rec)
    state = {g: eng._group_state(g, None) for g in groups}
    eng.grads = {g: torch.zeros(eng._group_floats(g)) for g in groups}

    def publish(flat):
        rec.append(("publish", flat))

    def no_validation():
        rec.append(("validate",))
        return {}
    out = fitloop.run(eng, gen, groups, state, eng.grads, "flat", THR, publish, validate or no_validation, val_names, epochs,
                      initial_epoch, callbacks, learning_rate, policy, cache)
    return out, state


GROUPS = [("heads",), ("heads", "blocks")]
ORDER = [3, 0, 5, 6]                     # a batch of images 3, 0, 5 and a batch of image 6


def _grads(groups, n, ids, w, accumulate, scale=None, word=None):
    """one gradient record per group, heads first; only `blocks` is handed the scale and the overflow word"""
    return [("grad", g, n, ("labels", ids), w, accumulate, scale if g == "blocks" else None, word if g == "blocks" else None)
            for g in groups]


def _batch_tail(groups, t, lr=0.5):
    return [("adam", g, t, lr) for g in groups]


def _epoch_tail(groups):
    return [("weights_to_flat", g, g) for g in groups] + [("publish", "flat"), ("validate",), ("gen.on_epoch_end",)]


def _chunk(groups, n, ids, w, accumulate):
    return [("assign_device", ids)] + _grads(groups, n, ids, w, accumulate) + [("loss_device", n, ("labels", ids))]


def _forward_epoch(groups, read, launch, t0=0, store=None):
    """the records of one epoch over ORDER on a route that forwards: `read` names the generator method, `launch(i)` the route's
    pixel launch (a list), store: the cache whose rows follow every forward"""
    def fwd(ids):
        return [("forward_device", ids)] + ([("store_features", store, ids)] if store else [])
    return ([(read, 0), ("check_boxes", 3)] + launch(0)
            + fwd([3, 0]) + _chunk(groups, 2, [3, 0], W3 * 2, False)
            + fwd([5]) + _chunk(groups, 1, [5], W3, True)
            + _batch_tail(groups, t0 + 1)
            + [(read, 1), ("check_boxes", 1)] + launch(1)
            + fwd([6]) + _chunk(groups, 1, [6], [1.0], False)
            + _batch_tail(groups, t0 + 2)
            + _epoch_tail(groups))


W3 = [float(np.float32(1 / 3))]          # one image's weight in a batch of three; the weight tensor is float32
# an epoch over ORDER: the batch of three summed, the batch of one added, the mean over the four images
EPOCH_LOSS = ((PER_IMAGE + PER_IMAGE + PER_IMAGE) + PER_IMAGE) / 4


# ---- the four routes
@pytest.mark.parametrize("groups", GROUPS)
def test_host_route(groups):
    rec = []
    out, state = _run(rec, FakeGen(rec, ORDER), groups)
    assert rec == _forward_epoch(groups, "boxes", lambda i: [])
    assert [s["t"] for s in state.values()] == [2] * len(groups)
    assert out.history == {"loss": [EPOCH_LOSS]} and out.epoch == [0]


@pytest.mark.parametrize("groups", GROUPS)
def test_augment_route(groups):
    rec = []
    aug = types.SimpleNamespace(pad_value=77, mosaic=0.0)
    _run(rec, FakeGen(rec, ORDER, augment=aug), groups)
    assert rec == _forward_epoch(groups, "raw", lambda i: [("augment_u8_batch", (3, 1)[i], f"params{i}", 77)])


@pytest.mark.parametrize("groups", GROUPS)
def test_mosaic_route(groups):
    rec = []
    aug = types.SimpleNamespace(pad_value=5, mosaic=0.5)
    _run(rec, FakeGen(rec, ORDER, augment=aug), groups)
    assert rec == _forward_epoch(groups, "raw_mosaic",
                                 lambda i: [("mosaic_u8_batch", (3, 1)[i], f"tiles{i}", f"params{i}", f"cuts{i}", 5)])


@pytest.mark.parametrize("groups", GROUPS)
def test_cached_route(groups):
    rec = []
    _run(rec, FakeGen(rec, ORDER), groups, epochs=5, initial_epoch=3, cache="cache")
    first = _forward_epoch(groups, "boxes", lambda i: [], store="cache")
    assert rec[:len(first)] == first                   # the call's first epoch: the host route, every forward stored at `indexes`
    second = ([("labels", 0), ("check_boxes", 3),
               ("load_features", "cache", [3, 0]), ("forward_tail_device", 2)] + _chunk(groups, 2, [3, 0], W3 * 2, False)
              + [("load_features", "cache", [5]), ("forward_tail_device", 1)] + _chunk(groups, 1, [5], W3, True)
              + _batch_tail(groups, 3)
              + [("labels", 1), ("check_boxes", 1),
                 ("load_features", "cache", [6]), ("forward_tail_device", 1)] + _chunk(groups, 1, [6], [1.0], False)
              + _batch_tail(groups, 4)
              + _epoch_tail(groups))
    assert rec[len(first):] == second
    assert not {"boxes", "forward_device", "store_features"} & {r[0] for r in rec[len(first):]}


def test_cache_rows_must_match_the_labels():
    rec = []
    gen = FakeGen(rec, ORDER)
    gen.batch_size = 2                                  # `indexes` is cut in twos, the batches stay threes
    gen._ids = lambda i: ORDER[i * 3:(i + 1) * 3]
    with pytest.raises(ValueError, match=r"^labels for 3 images, but the generator names 2 of them in `indexes`$"):
        _run(rec, gen, ("heads",), cache="cache")
    assert rec == [("boxes", 0), ("check_boxes", 3)]


# ---- the loss scale
def test_scaling_skips_both_groups_and_counts():
    rec = []
    groups = ("heads", "blocks")
    policy = FakePolicy(rec, [True, False, True, True])
    eng = FakeEngine(rec)
    real_grad = eng._group_grad_device

    def grad_that_overflows(g, n, *a):
        real_grad(g, n, *a)
        if g == "blocks" and n == 2:
            a[-1].fill_(1)                              # what y4_block_grad_scaled does to the word on an overflow
    eng._group_grad_device = grad_that_overflows
    out, state = _run(rec, FakeGen(rec, ORDER), groups, epochs=2, policy=policy, eng=eng)

    def chunk(n, ids, w, accumulate, scale, word):
        return [("assign_device", ids)] + _grads(groups, n, ids, w, accumulate, scale, word) + [("loss_device", n, ("labels", ids))]

    def epoch(scale1, scale2, tail1, tail2):
        # the word reads 0 at the batch's first gradient call in every batch (zeroed per batch), 1 once the chunk of 2 has set it
        return ([("boxes", 0), ("check_boxes", 3), ("forward_device", [3, 0])] + chunk(2, [3, 0], W3 * 2, False, scale1, 0)
                + [("forward_device", [5])] + chunk(1, [5], W3, True, scale1, 1) + [("policy.update", True)] + tail1
                + [("boxes", 1), ("check_boxes", 1), ("forward_device", [6])] + chunk(1, [6], [1.0], False, scale2, 0)
                + [("policy.update", False)] + tail2 + _epoch_tail(groups))
    # answers True, False, True, True: batch 2 of epoch 1 does not step and halves the scale
    assert rec == (epoch(8.0, 8.0, _batch_tail(groups, 1), []) + epoch(4.0, 4.0, _batch_tail(groups, 2), _batch_tail(groups, 3)))
    assert state["heads"]["t"] == state["blocks"]["t"] == 3
    assert out.history == {"loss": [EPOCH_LOSS, EPOCH_LOSS], "loss_scale": [4.0, 4.0], "skipped_steps": [1, 0]}


def test_scaling_history_of_one_epoch():
    rec = []
    out, _ = _run(rec, FakeGen(rec, ORDER), ("heads", "blocks"), policy=FakePolicy(rec, [True, False]))
    assert out.history["skipped_steps"] == [1] and out.history["loss_scale"] == [4.0]
    assert [r for r in rec if r[0] == "adam"] == [("adam", "heads", 1, 0.5), ("adam", "blocks", 1, 0.5)]


# ---- the epoch's order
def test_epoch_order_schedule_history():
    rec = []

    class Schedule:
        def schedule(self, epoch, lr):
            rec.append(("schedule", epoch, lr))
            return lr / 2

    class Logger:
        def on_epoch_end(self, epoch, logs):
            rec.append(("cb.on_epoch_end", epoch, dict(logs)))

    def validate():
        rec.append(("validate",))
        return {"val_loss": 2.5, "val_mAP": 0.75}
    out, _ = _run(rec, FakeGen(rec, [4]), ("heads", "blocks"), epochs=4, initial_epoch=2, callbacks=[Schedule(), Logger()],
                  validate=validate, val_names=("val_loss", "val_mAP"), learning_rate=1.0)
    logs = {"loss": PER_IMAGE, "val_loss": 2.5, "val_mAP": 0.75}

    def epoch(e, asked, lr, t):
        return ([("schedule", e, asked), ("boxes", 0), ("check_boxes", 1), ("forward_device", [4])]
                + _chunk(("heads", "blocks"), 1, [4], [1.0], False) + _batch_tail(("heads", "blocks"), t, lr)
                + [("weights_to_flat", "heads", "heads"), ("weights_to_flat", "blocks", "blocks"), ("publish", "flat"),
                   ("validate",), ("gen.on_epoch_end",), ("cb.on_epoch_end", e, logs)])
    assert rec == epoch(2, 1.0, 0.5, 1) + epoch(3, 0.5, 0.25, 2)
    assert out.history == {"loss": [PER_IMAGE] * 2, "val_loss": [2.5] * 2, "val_mAP": [0.75] * 2}
    assert list(out.history) == ["loss", "val_loss", "val_mAP"] and out.epoch == [2, 3]


def test_history_keys_and_printed_line(capsys):
    rec = []
    out, _ = _run(rec, FakeGen(rec, ORDER), ("heads",), epochs=2)
    assert list(out.history) == ["loss"] and out.epoch == [0, 1]
    assert capsys.readouterr().out == f"Epoch 1/2 - loss: {PER_IMAGE:.4f}\nEpoch 2/2 - loss: {PER_IMAGE:.4f}\n"
    out, _ = _run(rec, FakeGen(rec, ORDER), ("heads", "blocks"), policy=FakePolicy(rec, [True, True]),
                  validate=lambda: {"val_loss": 1.0}, val_names=("val_loss",))
    assert list(out.history) == ["loss", "val_loss", "loss_scale", "skipped_steps"]
    assert capsys.readouterr().out == f"Epoch 1/1 - loss: {PER_IMAGE:.4f} - val_loss: 1.0000\n"


# ---- refusals
@pytest.mark.parametrize("shift,text,seen", [
    (1, "labels for 3 images, the images are more", [[3, 0]]),            # 4 images: the chunk of images 5, 99 is refused
    (-1, "labels for 3 images, but 2 images", [[3, 0]]),                  # 2 images: refused when the chunks run out
])
def test_image_and_label_counts_must_agree(shift, text, seen):
    rec = []
    with pytest.raises(ValueError) as e:
        _run(rec, FakeGen(rec, ORDER, image_shift=shift), ("heads", "blocks"))
    assert str(e.value) == text
    assert [r[1] for r in rec if r[0] == "forward_device"] == seen
    assert not [r for r in rec if r[0] in ("adam", "publish", "weights_to_flat")]


def test_paired_chunks_of_predict():
    eng, X = FakeEngine([]), np.arange(3, dtype=np.float32)[:, None]
    assert [(i0, c[:, 0].tolist()) for i0, c in eng._paired_chunks(X, 3, "box_map")] == [(0, [0.0, 1.0]), (2, [2.0])]
    assert [i0 for i0, _ in eng._paired_chunks(X, None, "box_map")] == [0, 2]           # no box_map: nothing to pair
    with pytest.raises(ValueError, match="^box_map has 2 rows, the images are more$"):
        list(eng._paired_chunks(X, 2, "box_map"))
    with pytest.raises(ValueError, match="^box_map has 4 rows for 3 images$"):
        list(eng._paired_chunks(X, 4, "box_map"))


@pytest.mark.parametrize("augment", [None, types.SimpleNamespace(pad_value=0, mosaic=0.0), types.SimpleNamespace(pad_value=0, mosaic=1.0)])
def test_a_refused_box_raises_before_any_launch(augment):
    rec = []
    with pytest.raises(ValueError, match="centre is outside"):
        _run(rec, FakeGen(rec, ORDER, augment=augment), ("heads",), eng=FakeEngine(rec, refuse_boxes=True))
    assert rec == [({None: "boxes", 0.0: "raw", 1.0: "raw_mosaic"}[augment and augment.mosaic], 0), ("check_boxes", 3)]


def test_empty_generator():
    rec = []
    with pytest.raises(ValueError, match="^fit: the generator is empty$"):
        _run(rec, FakeGen(rec, []), ("heads",))
    assert rec == []


class _Gen:
    max_boxes = 100


class _Augmenting(_Gen):
    augment = object()


class _Full(_Gen):
    indexes, batch_size = [0], 1

    def labels(self, i):
        pass


def _check(gen=_Full(), val=None, trainable="heads", loss_scale=None, val_map=False, cache_features=False, dtype="bf16",
           max_boxes=100):
    return fitloop.check_arguments(gen, val, trainable, loss_scale, val_map, cache_features, dtype, max_boxes)


def test_argument_check_accepts():
    assert _check() == (("heads",), None)
    assert _check(trainable="head_blocks", cache_features=True, val=_Gen(), val_map=True) == (("heads", "blocks"), None)
    groups, policy = _check(trainable="head_blocks", dtype="f16", loss_scale=128.0)
    assert groups == ("heads", "blocks") and policy.scale == 128.0 and not policy.dynamic
    assert _check(trainable="head_blocks", dtype="f16", loss_scale="dynamic")[1].dynamic
    assert _check(gen=None) == (("heads",), None)         # an object without max_boxes is taken at the config's


# each case breaks two neighbouring rules of fit's order at once; the earlier one speaks
@pytest.mark.parametrize("kw,exc,text", [
    (dict(val_map=True, cache_features="yes"), ValueError, "fit: val_map=True needs val_data_gen"),
    (dict(cache_features=0, gen=_Augmenting()), ValueError, "fit: cache_features is False, True or a positive byte budget, got 0"),
    (dict(cache_features=True, gen=_Augmenting()), ValueError, "fit: cache_features needs a generator that does not augment"),
    (dict(cache_features=4096, gen=_Gen(), trainable=None), ValueError,
     "this one lacks indexes, batch_size, labels"),
    (dict(trainable="all", dtype="f16", loss_scale=3), NotImplementedError, "training every layer is out of scope"),
    (dict(trainable="head_blocks", dtype="f16", max_boxes=7), NotImplementedError, "needs loss scaling"),
    (dict(trainable="heads", dtype="f16", loss_scale=3, max_boxes=7), ValueError,
     "nothing to scale on a f16 model with trainable='heads'"),
    (dict(trainable="head_blocks", dtype="f16", loss_scale=3, max_boxes=7), ValueError,
     "loss_scale 3: 'dynamic', a LossScale or a power of two"),
    (dict(max_boxes=7), ValueError, "the generator's max_boxes 100 != config['max_boxes'] 7"),
])
def test_argument_check_refuses_in_fits_order(kw, exc, text):
    with pytest.raises(exc) as e:
        _check(**kw)
    assert text in str(e.value)
