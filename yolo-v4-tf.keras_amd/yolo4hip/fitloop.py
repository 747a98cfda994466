"""The loop under `Yolov4.fit`: the argument check, one batch source per input route, the step of one batch, the epoch loop.

Nothing here imports the facade or loads the library: the training engine, the host weight stream and the two callables
`publish(flat)` and `validate()` arrive as arguments, so the loop runs on any object with the engine's methods
(tests/test_fit_loop_cpu.py runs it on a recording one).  `Yolov4.fit`'s docstring is the user documentation; DESIGN.md
section 7e.3 names the parts."""
import numpy as np

from .engine import combine_loss
from .loss_scale import make_loss_scale


def check_arguments(gen, val_data_gen, trainable, loss_scale, val_map, cache_features, dtype, max_boxes):
    """Every refusal `fit` makes before it touches a device, in this order -> (groups in step order, LossScale or None)."""
    if val_map and val_data_gen is None:
        raise ValueError('fit: val_map=True needs val_data_gen')
    if cache_features is not False:
        if not isinstance(cache_features, (bool, int, np.integer)) or int(cache_features) < 1:
            raise ValueError(f'fit: cache_features is False, True or a positive byte budget, got {cache_features!r}')
        if getattr(gen, 'augment', None) is not None:
            raise ValueError('fit: cache_features needs a generator that does not augment: an augmented image has other '
                             'pixels in every epoch, so there is nothing to cache')
        missing = [a for a in ('indexes', 'batch_size', 'labels') if not hasattr(gen, a)]
        if missing:
            raise ValueError(f"fit: cache_features needs a generator with `indexes`, `batch_size` and `labels(i)` "
                             f"(yolo4hip.data.DataGenerator); this one lacks {', '.join(missing)}")
    if trainable not in ('heads', 'head_blocks'):
        raise NotImplementedError("training every layer is out of scope of the MI355X path; fit(..., trainable='heads') "
                                  "fine-tunes the three detection convs on a frozen backbone and neck, "
                                  "trainable='head_blocks' also the 3x3 convs in front of them")
    groups = ('heads', 'blocks') if trainable == 'head_blocks' else ('heads',)
    scaling = 'blocks' in groups and dtype == 'f16'
    if scaling and loss_scale is None:
        raise NotImplementedError("fit(trainable='head_blocks') on an f16 model: a 16-bit gradient in fp16 needs loss scaling; "
                                  "pass loss_scale='dynamic' or a power of two (or use dtype 'bf16' or 'f32')")
    if loss_scale is not None and not scaling:
        raise ValueError("fit: loss_scale is for trainable='head_blocks' on an f16 model; there is nothing to scale on "
                         f"a {dtype} model with trainable={trainable!r}")
    policy = make_loss_scale(loss_scale) if scaling else None
    if getattr(gen, 'max_boxes', max_boxes) != max_boxes:
        raise ValueError(f"the generator's max_boxes {gen.max_boxes} != config['max_boxes'] {max_boxes}")
    return groups, policy


def alloc_feature_cache(eng, gen, cache_features, describe):
    """The device cache of `fit(cache_features=...)`, one row per annotation line; MemoryError when it is larger than the budget
    (True: what the driver has free and what torch holds without using it).  describe: the model, for the message."""
    torch = eng.torch
    rows, row_bytes = int(np.max(gen.indexes)) + 1, eng.feature_row_bytes()[0]
    if cache_features is True:
        with torch.cuda.device(eng.device):
            budget = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        what = 'bytes of device memory are free'
    else:
        budget, what = int(cache_features), 'bytes is the budget (cache_features)'
    if rows * row_bytes > budget:
        raise MemoryError(f'fit: the feature cache needs {rows * row_bytes} bytes ({rows} images, {row_bytes} bytes per '
                          f'image {describe}); {budget} {what}')
    return eng.alloc_feature_cache(rows)


# ---- batch sources, one per input route.  source(i) reads batch i from the generator -> (boxes, chunks); chunks(count), called
# once the boxes are checked and uploaded, makes the batch's pixels where the route has a launch for that and returns an
# iterable of (i0, n): the workspace then holds the heads of images i0 .. i0 + n - 1.
def _forwarded(eng, X, count):
    for i0, chunk in eng._paired_chunks(X, count):
        eng.forward_device(chunk)
        yield i0, chunk.shape[0]


def host_source(eng, gen):
    def read(i):
        X, boxes = gen.boxes(i)
        return boxes, lambda count: _forwarded(eng, X, count)
    return read


def augment_source(eng, gen, augment):
    def read(i):
        raws, params, boxes = gen.raw(i)
        return boxes, lambda count: _forwarded(eng, eng.augment_u8_batch(raws, params, pad_value=augment.pad_value), count)
    return read


def mosaic_source(eng, gen, augment):
    def read(i):
        raws, tile_src, params, cuts, boxes = gen.raw_mosaic(i)
        return boxes, lambda count: _forwarded(
            eng, eng.mosaic_u8_batch(raws, tile_src, params, cuts, pad_value=augment.pad_value), count)
    return read


def _cache_rows(gen, i):
    """the batch's rows in the cache: the annotation-line indices of its images"""
    bs = int(gen.batch_size)
    return np.asarray(gen.indexes[i * bs:(i + 1) * bs], dtype=np.int64)


def _rows_of(idxs, count):
    if len(idxs) != count:
        raise ValueError(f'labels for {count} images, but the generator names {len(idxs)} of them in `indexes`')
    return idxs


def _stored(eng, X, cache, idxs):
    for i0, n in _forwarded(eng, X, len(idxs)):
        eng.store_features(cache, idxs[i0:i0 + n])
        yield i0, n


def _loaded(eng, cache, idxs):
    """a chunk is a range of cache rows, loaded where the forward would have left them"""
    for i0 in range(0, len(idxs), eng.max_batch):
        n = min(eng.max_batch, len(idxs) - i0)
        eng.load_features(cache, idxs[i0:i0 + n])
        eng.forward_tail_device(n)
        yield i0, n


def filling_source(eng, gen, cache):
    """the host route of the epoch that fills the cache"""
    def read(i):
        idxs = _cache_rows(gen, i)
        X, boxes = gen.boxes(i)
        return boxes, lambda count: _stored(eng, X, cache, _rows_of(idxs, count))
    return read


def cached_source(eng, gen, cache):
    def read(i):
        idxs = _cache_rows(gen, i)
        return gen.labels(i), lambda count: _loaded(eng, cache, _rows_of(idxs, count))
    return read


def choose_source(eng, gen, cache, filled):
    """The route of one epoch.  filled: an earlier epoch of this call has been through every batch with `filling_source`."""
    if cache is not None:
        return (cached_source if filled else filling_source)(eng, gen, cache)
    augment = getattr(gen, 'augment', None)
    if augment is None:
        return host_source(eng, gen)
    return (mosaic_source if getattr(augment, 'mosaic', 0) > 0 else augment_source)(eng, gen, augment)


def step(eng, groups, state, grad, boxes_dev, chunks, lr, iou_loss_thresh, policy=None, overflow=None):
    """One batch: the gradients of every group accumulated over `chunks` (each image weighs 1 / batch images), one host read,
    one Adam step per group -> (the batch's loss sum, whether it stepped).  policy / overflow: the loss scale and its device
    word, or None."""
    torch = eng.torch
    count = boxes_dev.shape[0]
    weight = torch.full((count,), 1.0 / count, dtype=torch.float32, device=eng.device)
    if policy is not None:
        overflow.zero_()
    scaled = {'blocks': (policy.scale, overflow)} if policy is not None else {}
    parts = []
    for i0, n in chunks:
        labels = eng.assign_device(boxes_dev[i0:i0 + n])
        for g in groups:
            eng._group_grad_device(g, n, None, labels, iou_loss_thresh, weight[i0:i0 + n], grad[g], i0 > 0, *scaled.get(g, ()))
        parts.append(eng.loss_device(n, records=labels, iou_loss_thresh=iou_loss_thresh))
    # heads first, and every gradient of the batch before the first step: y4_block_grad must see the head weights
    # the forward used.  The steps share their t.  An overflow of the scaled block gradient skips the step of both.
    if policy is not None:
        parts.append(overflow.to(torch.float32).expand(1, *parts[0].shape[1:]))
    losses = torch.cat(parts).cpu().numpy()                     # one copy: the loss and the overflow word
    stepped = policy is None or policy.update(bool(losses[-1].flat[0] != 0))
    if stepped:
        for g in groups:
            eng._group_adam_step(g, state[g], grad[g], lr=lr)
    return float(combine_loss(losses[:-1] if policy is not None else losses)[0].sum()), stepped


def batches(eng, indices, source, groups, state, grad, lr, iou_loss_thresh, policy=None, overflow=None):
    """The batches `indices` of one epoch -> (loss sum, images, skipped steps).  A frame of its own: the last batch's pixels are
    released when the epoch's batches are done, not by the next epoch's first read."""
    torch = eng.torch
    total, images, skipped = 0.0, 0, 0
    for i in indices:
        boxes, chunks = source(i)
        boxes_dev = torch.from_numpy(eng._check_boxes(boxes)).to(eng.device)     # ValueError before any update
        loss, stepped = step(eng, groups, state, grad, boxes_dev, chunks(boxes_dev.shape[0]), lr, iou_loss_thresh, policy, overflow)
        total, images, skipped = total + loss, images + boxes_dev.shape[0], skipped + (not stepped)
    return total, images, skipped


class History:
    """What `fit` returns, as Keras does: `.history` {name: one value per epoch} and `.epoch`, the epochs run."""

    def __init__(self, names, epochs):
        self.history, self.epoch = {k: [] for k in names}, list(epochs)


def run(eng, gen, groups, state, grad, flat, iou_loss_thresh, publish, validate, val_names, epochs, initial_epoch=0,
        callbacks=None, learning_rate=1e-4, policy=None, cache=None):
    """The epochs initial_epoch .. epochs - 1 of `fit` -> History.  publish(flat) hands the host stream, with the epoch's trained
    weights in it, to whoever infers with it; validate() -> the epoch's further log entries, under the names `val_names`."""
    torch = eng.torch
    epochs, initial_epoch, callbacks = int(epochs), int(initial_epoch), callbacks or []
    out = History(('loss',) + tuple(val_names) + (('loss_scale', 'skipped_steps') if policy is not None else ()),
                  range(initial_epoch, epochs))
    overflow = torch.zeros((1,), dtype=torch.int32, device=eng.device) if policy is not None else None
    for epoch in out.epoch:
        for cb in callbacks:
            if hasattr(cb, 'schedule'):
                learning_rate = float(cb.schedule(epoch, learning_rate))
        total, images, skipped = batches(eng, range(len(gen)), choose_source(eng, gen, cache, filled=epoch > initial_epoch),
                                         groups, state, grad, learning_rate, iou_loss_thresh, policy, overflow)
        if images == 0:
            raise ValueError('fit: the generator is empty')
        # the trained weights reach the host stream and the inference engine at the end of every epoch
        for g in groups:
            eng._group_weights_to_flat(g, state[g], flat)
        publish(flat)
        logs = {'loss': total / images, **validate()}
        for k, v in logs.items():
            out.history[k].append(v)
        if policy is not None:
            out.history['loss_scale'].append(policy.scale)
            out.history['skipped_steps'].append(skipped)
        print(f'Epoch {epoch + 1}/{epochs} - ' + ' - '.join(f'{k}: {v:.4f}' for k, v in logs.items()))
        if hasattr(gen, 'on_epoch_end'):
            gen.on_epoch_end()
        for cb in callbacks:
            if hasattr(cb, 'on_epoch_end'):
                cb.on_epoch_end(epoch, logs)
    return out
