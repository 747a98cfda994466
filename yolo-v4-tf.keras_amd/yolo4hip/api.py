"""`Yolov4` facade: the reference's user API (models.py:17-127, 509-529) over the HIP engine.

Drop-in surface kept: constructor signature and asserts, the attributes users read
(`class_names, img_size, num_classes, anchors, xyscale, strides, output_sizes, class_color, config,
weight_path, max_boxes`), `.yolo_model.predict(imgs)` -> 3 raw heads, `.inference_model.predict(imgs)` ->
`[boxes, scores, classes, valid_detections]`, `.predict / .predict_img / .predict_raw / .predict_nonms`
with their prints (`img shape:`, `# of bboxes:`) and DataFrame layout.
Differences, all supersets: the passed `config` is honoured (the reference reads the module global,
models.py:26-37); grid sizes follow img_size (the reference hard-codes 52/26/13) and img_size may be a rectangle (H, W, 3) --
the reference's 'not support yet' assert is lifted, boxes are normalised x / W, y / H; extra keyword-only
arguments pick the compute dtype / batch capacity, and `letterbox=True` (keyword-only, off by default) letterboxes the input
instead of the reference's stretch (Darknet's letter_box=1 geometry) with boxes returned in each raw image's pixels.  `save_model` / `load_model` (models.py:86-93) are stand-ins on a
self-describing checkpoint of this framework (Keras' SavedModel / H5 needs TensorFlow); `eval_map` (models.py:182-507)
is the VOC mAP tool over the exported text files (yolo4hip/evalmap.py).  `training_model.predict([X, y_s, y_m, y_l, true_xywh])`
is the reference's yolo_loss FORWARD (models.py:54-65, loss.py) on the device and `evaluate(data_gen)` the validation loss over
a `DataGenerator`, `evaluate_map(data)` VOC mAP with the matching on the device (y4_map_match; the numbers of `eval_map` without
its text files) and `evaluate_coco(data, views=..., tiled=...)` COCO's AP / AR (y4_coco_match; over the plain, the view or the tiled
path); `fit(..., trainable='heads')` fine-tunes the three detection convs on a frozen backbone and neck (with a
`DataGenerator(..., augment=AugmentConfig())` under scale, shift, flip and HSV augmentation applied on the device), while
training every layer (the reference's `fit`) is out of scope and raises.  `predict_tiled` / `predict_img_tiled` (not in the reference)
cut a photo much larger than the network input into overlapping windows and run one NMS per photo over all of them on the device;
`predict_tta` / `predict_img_tta` (not in the reference either) run a photo under flipped and scaled views, again under one NMS.
`rebase_anchors(trained_with)` (not in the reference) keeps the boxes of loaded weights when `config['anchors']` are not the ones
they were trained with (yolo4hip/anchors.py fits anchors to a data set).
"""
import json
import os

import numpy as np

from . import prepost, tiling, weights as W
from .config import yolo_config
from .engine import NMS_OPTIONS, Engine
from .plan import build_plan


class _KerasLikeModel:
    """The slice of `tf.keras.Model` the reference touches: `.predict(x)`."""

    def __init__(self, fn, name):
        self._fn, self.name = fn, name

    def predict(self, x, batch_size=None, verbose=0, **_):
        return self._fn(x)

    __call__ = predict


class Yolov4(object):
    def __init__(self, weight_path=None, class_name_path='coco_classes.txt', config=yolo_config, *,
                 dtype='f32', max_batch=32, synth_seed=0, device=None, device_preprocess=True, tune=None, share_schedule=None,
                 letterbox=False, pad_value=128, box_loss='giou', nms_kind='iou', nms_beta=0.6, nms_agnostic=False,
                 nms_merge=False, nms_soft=None, nms_sigma=0.5, nms_soft_min_score=None, nms_top_k=4096, nms_matrix=None):
        # (reference models.py:23 also asserts img_size[0] == img_size[1], 'not support yet': rectangles are supported here)
        assert config['img_size'][0] % config['strides'][-1] == 0, 'must be a multiple of last stride'
        assert config['img_size'][1] % config['strides'][-1] == 0, 'must be a multiple of last stride'
        self.class_names = [line.strip() for line in open(class_name_path).readlines()]
        self.img_size = tuple(config['img_size'])
        self.num_classes = len(self.class_names)
        self.weight_path = weight_path
        self.anchors = np.array(config['anchors']).reshape((3, 3, 2))
        self.xyscale = config['xyscale']
        self.strides = config['strides']
        H, W = self.img_size[0], self.img_size[1]
        # square: one grid side per scale (as the reference); rectangle: (rows, columns) per scale
        self.output_sizes = [H // s for s in self.strides] if H == W else [(H // s, W // s) for s in self.strides]
        self.class_color = {name: list(np.random.random(size=3) * 255) for name in self.class_names}
        self.max_boxes = config['max_boxes']
        self.iou_loss_thresh = config.get('iou_loss_thresh', 0.5)
        self.config = config
        assert self.num_classes > 0, 'no classes detected!'
        self._dtype, self._max_batch, self._synth_seed, self._device = dtype, max_batch, synth_seed, device
        self._device_preprocess = device_preprocess
        # box_loss: the box term of training_model -- 'giou', what the reference's loss.py has switched on, or 'ciou', its bbox_ciou
        # (the commented line under it).  training_model.predict, evaluate, fit and its val_loss all run with it; it is no part
        # of a checkpoint.
        Engine._box_kind(box_loss)                 # (raises ValueError for an unknown name)
        self.box_loss = box_loss
        # nms_kind / nms_beta / nms_agnostic: the pair rule of the NMS stage (Engine.set_nms_rule): 'iou', what the reference's
        # tf.image.combined_non_max_suppression does, or 'diou' (DIoU-NMS, Darknet's nms_kind=diounms with beta_nms = nms_beta);
        # nms_agnostic=True lets a kept box suppress later candidates of every class.  It is state of the engines' handles, so
        # inference_model, predict, predict_img, predict_nonms, export_prediction, evaluate_map and fit(val_map=True) all run with
        # it, with and without letterbox, before and after load_model and fit; it is no part of a checkpoint.
        Engine._nms_rule(nms_kind, nms_beta, nms_agnostic)      # (raises ValueError)
        self.nms_kind, self.nms_beta, self.nms_agnostic = nms_kind, float(nms_beta), bool(nms_agnostic)
        # nms_merge=True: merge-NMS (box voting, YOLOv5's merge=True) -- each kept box is replaced by the score-weighted mean of the
        # candidates it absorbed under that pair rule (Engine.set_nms_merge); the kept set, scores and classes do not change.  Like
        # the rule it is state of both engines and in force for inference_model, predict, predict_img, predict_nonms,
        # export_prediction, evaluate_map, fit(val_map=True), predict_tiled and predict_img_tiled, with and without letterbox, before
        # and after load_model and fit; it is no part of a checkpoint or a schedule.
        self.nms_merge = Engine._merge_flag(nms_merge)          # (raises ValueError)
        # nms_soft='gaussian' | 'linear' | 'hard' (None: off): Soft-NMS (Engine.set_nms_soft) -- a kept box decays the scores of its
        # neighbours under that pair rule instead of deleting them, with nms_sigma, the floor nms_soft_min_score (None: the config's
        # score_threshold, whatever a call's run-time thresholds are) and the nms_top_k best candidates of a list taking part.  Like
        # the rule it is state of both engines and in force for everything nms_kind is in force for, over tiles and views too; it
        # is no part of a checkpoint or a schedule.
        Engine._decay_mode("soft", nms_soft, nms_sigma, nms_soft_min_score, nms_top_k)      # (raises ValueError)
        self.nms_soft, self.nms_sigma, self.nms_top_k = nms_soft, float(nms_sigma), int(nms_top_k)
        self.nms_soft_min_score = None if nms_soft_min_score is None else float(nms_soft_min_score)
        # nms_matrix='gaussian' | 'linear' (None: off): Matrix-NMS (Engine.set_nms_matrix) -- one-shot score decay by the earlier
        # candidates of a class, no pick sequence; nms_sigma, nms_soft_min_score and nms_top_k parameterise whichever of nms_soft /
        # nms_matrix is set, and the two exclude each other.  In force wherever nms_soft would be.
        if Engine._decay_mode("matrix", nms_matrix, nms_sigma, nms_soft_min_score, nms_top_k)[0] and nms_soft is not None:      # (raises ValueError)
            raise ValueError(f"nms_soft={nms_soft!r} and nms_matrix={nms_matrix!r} exclude each other")
        self.nms_matrix = nms_matrix
        # letterbox=True: predict_img / predict / export_prediction resize each image with its aspect ratio kept, centred on a
        # canvas of uint8 level `pad_value` (Darknet's letterbox_image geometry; the resize is still cv2's uint8 arithmetic and the
        # pad a uint8 level, 128 = 0.502, where Darknet pads 0.5), and the boxes are mapped back to each raw image on the device.
        # inference_model.predict(imgs) keeps the reference's meaning (preprocessed images in, canvas-normalised boxes out), and
        # predict_raw / predict_nonms stay stretch-only.
        self._letterbox = bool(letterbox)
        self._pad_value = int(pad_value)
        if not 0 <= self._pad_value <= 255:
            raise ValueError(f'pad_value must be a uint8 level 0..255, got {pad_value}')
        # A shape without a shipped / cached schedule is tuned ONCE (a full-size predict + y4_autotune on `max_batch` synthetic
        # images: seconds at 160^2, ~20 s at 608^2 x 32; written to $YOLO4HIP_CACHE, default ~/.cache/yolo4hip):
        #   tune=None (default)  on the first predict of this object, not in the constructor; YOLO4HIP_TUNE=0: never
        #   tune=True            now, in the constructor          tune=False   never (built-in tile heuristic)
        # share_schedule=True (or YOLO4HIP_SHARE_SCHEDULE=1) under an initialised torch.distributed group of more than one rank makes
        # the constructor a COLLECTIVE -- rank 0 resolves (and, if allowed, tunes) the schedule now and broadcasts it, so every rank
        # runs the same tile set after ONE tuning run; every rank must then construct the same model.  Off by default (a
        # model built on some ranks only -- a rank-0 evaluation inside a DDP job -- must not block in a broadcast): each rank then
        # resolves its own schedule, which for shipped and cached schedules is the same file everywhere.
        self._share_schedule = (os.environ.get('YOLO4HIP_SHARE_SCHEDULE', '0') == '1') if share_schedule is None else bool(share_schedule)
        self._tune = (os.environ.get('YOLO4HIP_TUNE', '1') != '0') if tune is None else bool(tune)
        self._tune_eager = tune is True
        self.build_model(load_pretrained=True if self.weight_path else False)

    def nms_options(self):
        """The `nms_*` keywords both engines are built with: this object's attributes of those names."""
        return {k: getattr(self, k) for k in NMS_OPTIONS}

    def build_model(self, load_pretrained=True):
        self.plan = build_plan(self.img_size[:2], self.num_classes)
        # alias_workspace: like the reference's Keras model, the facade keeps no intermediate activations (2.7x less HBM)
        self.engine = Engine(self.num_classes, self.config, max_batch=self._max_batch, dtype=self._dtype,
                             device=self._device, alias_workspace=True, box_loss=self.box_loss, **self.nms_options())
        self.yolo_model = _KerasLikeModel(self._tuned_first(self.engine.forward_heads), 'yolo_model')
        print(f"nms iou: {self.config['iou_threshold']} score: {self.config['score_threshold']}")
        self._thresholds = (-1.0, -1.0)  # what inference_model runs with (-1: the config's); load_model changes them
        self.inference_model = _KerasLikeModel(self._tuned_first(self.engine.predict), 'inference_model')
        # the reference's other model (models.py:54-65): yolo_loss over the raw heads and the labels, forward only
        self.training_model = _KerasLikeModel(self._tuned_first(self._loss_of_dense), 'training_model')
        if load_pretrained and self.weight_path and self.weight_path.endswith('.weights'):
            load_weights(self, self.weight_path)
            print(f'load from {self.weight_path}')
        else:
            # the reference leaves Keras' random initialisation in place; ours is the seeded synthetic set
            self._set_weights(W.flatten(W.synth_weights(self.plan, self._synth_seed)))
        # No silent un-tuned shapes: the tuned schedule that ships for this (size, classes, batch, dtype), else the one
        # tuned on this machine before, else tune -- once, cached on disk -- and say which is active.  Schedules without split-K
        # ids are bit-identical scheduling choices (tests/test_gpu_forward.py), so WHEN the tuning happens changes no result.
        from . import dist as D
        self._tune_pending = False
        if self._share_schedule and D.group_rank_world()[1] > 1:
            self.schedule_source = self.engine.ensure_schedule(tune=self._tune, share=True)
        elif self._tune_eager or not self._tune:
            self.schedule_source = self.engine.ensure_schedule(tune=self._tune)
        else:
            self.schedule_source = self.engine.ensure_schedule(tune=False, verbose=False)
            self._tune_pending = self.schedule_source[0] == 'heuristic'
            if self._tune_pending:
                print('schedule: none ships or is cached for this shape -- tuned on the first predict (tune=True: in the constructor)')
            else:
                self.engine.say_schedule()

    def _ensure_tuned(self):
        if self._tune_pending:
            self._tune_pending = False
            self.schedule_source = self.engine.ensure_schedule(tune=True)

    def _tuned_first(self, fn):
        def call(x, **kw):
            self._ensure_tuned()
            return fn(x, **kw)
        return call

    def _set_weights(self, flat):
        """flat: the Darknet-order float32 stream (weights.flatten).  Kept on the host like Keras keeps its variables,
        so that `save_model` can write it back."""
        self._flat = np.ascontiguousarray(flat, dtype=np.float32)
        self.engine.load_weight_blob(self._flat)

    # ---- reference models.py:86-93.  Keras writes architecture + variables of `yolo_model` (SavedModel / H5); without
    # TensorFlow the stand-in is a self-describing checkpoint of THIS framework: magic, a JSON header (what fixes the
    # architecture here: img_size, num_classes, anchors, strides, xyscale), then the float32 weight stream in Darknet
    # order -- dtype independent, so a model saved from a bf16 engine loads into an fp32 one.  A path ending in
    # `.weights` is written / read as a plain Darknet file instead.
    _CKPT_MAGIC = b'Y4CKPT1\n'

    def save_model(self, path):
        if path.endswith('.weights'):
            W.write_darknet(path, W.unflatten(self.plan, self._flat))
            return
        head = json.dumps({'format': 'yolo4hip-checkpoint', 'version': 1, 'img_size': list(self.img_size),
                           'num_classes': self.num_classes, 'class_names': self.class_names,
                           'anchors': np.asarray(self.anchors).reshape(-1).tolist(), 'strides': list(self.strides),
                           'xyscale': list(self.xyscale), 'n_floats': int(self._flat.size)}).encode()
        with open(path, 'wb') as fh:
            fh.write(self._CKPT_MAGIC)
            fh.write(len(head).to_bytes(8, 'little'))
            fh.write(head)
            self._flat.tofile(fh)

    def load_model(self, path):
        """Like the reference, rebuilds `yolo_model` and `inference_model` from the file; like it (models.py:90-91: `nms`
        called without thresholds) the inference model then uses the DEFAULT thresholds iou 0.413 / score 0.3."""
        if path.endswith('.weights'):
            ws, _header, _unread = W.read_darknet(path, self.plan)
            flat = W.flatten(ws)
        else:
            with open(path, 'rb') as fh:
                if fh.read(len(self._CKPT_MAGIC)) != self._CKPT_MAGIC:
                    raise ValueError(f'{path}: not a yolo4hip checkpoint (Keras SavedModel / H5 files need TensorFlow)')
                head = json.loads(fh.read(int.from_bytes(fh.read(8), 'little')).decode())
                flat = np.fromfile(fh, dtype=np.float32)
            same = (head['num_classes'] == self.num_classes and list(head['img_size']) == list(self.img_size)
                    and head['n_floats'] == self.plan.n_params)
            if not same or flat.size != self.plan.n_params:
                raise ValueError(f"{path}: checkpoint is for img_size {head['img_size']}, {head['num_classes']} classes, "
                                 f"{flat.size} floats; this model has {list(self.img_size)}, {self.num_classes}, "
                                 f"{self.plan.n_params}")
        self._set_weights(flat)
        self.yolo_model = _KerasLikeModel(self._tuned_first(self.engine.forward_heads), 'yolo_model')
        self.inference_model = _KerasLikeModel(
            self._tuned_first(lambda x: self.engine.predict(x, iou_threshold=0.413, score_threshold=0.3)), 'inference_model')
        self._thresholds = (0.413, 0.3)

    def rebase_anchors(self, trained_with):
        """For weights that were trained under the anchors `trained_with` (18 numbers) while this model decodes with
        `self.anchors` (e.g. pretrained heads under anchors from `yolo4hip.anchors.fit_anchors`): adds log(old_w / new_w) and
        log(old_h / new_h), computed in float64 and added in float32, to the tw / th biases of convs 93 / 101 / 109 in the host
        weight stream and re-loads it.  Afterwards exp(t') * new == exp(t) * old up to rounding: the model predicts the boxes it
        predicted under the old anchors.  Explicit, never automatic -- `load_model` and the constructor leave weights as they
        are -- and not idempotent: call it once per loaded weight set."""
        from .anchors import rebase_flat
        self._set_weights(rebase_flat(self._flat, self.plan, self.num_classes, trained_with, self.anchors))

    # ---- reference models.py:100-107.  Training all 110 convs is out of scope; what is here is the
    # fine-tuning of the three detection convs on a frozen backbone and neck: in Keras terms every layer trainable = False
    # except conv 93 / 101 / 109.
    def fit(self, train_data_gen, epochs, val_data_gen=None, initial_epoch=0, callbacks=None, *, trainable=None,
            learning_rate=1e-4, loss_scale=None, val_map=False, cache_features=False):
        """trainable='heads': Adam (the reference's compile, models.py:83; `learning_rate` replaces its 1e-4) on the weights and
        biases of the three detection convs.  Per batch: `train_data_gen.boxes(i)` -> one upload -> forward in chunks of
        max_batch -> labels assigned on the device -> y4_head_grad accumulated over the chunks (each image weighs 1 / batch
        images) -> y4_head_adam; the batch's training loss is y4_loss on the same heads.  Per epoch a Keras-like line,
        `train_data_gen.on_epoch_end()` and every callback's `on_epoch_end(epoch, logs)`.  -> an object whose `.history` is
        {'loss': [...], 'val_loss': [...]} (val_loss only with `val_data_gen`).  A batch with a box off the grid or an unknown
        class raises ValueError before any update.  trainable=None (the reference's meaning: every layer) is not implemented.

        trainable='head_blocks' additionally trains the KERNELS of the 3x3 convs in front of the heads (92 / 100 / 108); their
        BatchNormalization stays frozen and runs in inference mode, as Keras runs a frozen BN.  Per chunk y4_block_grad follows
        y4_head_grad (both use the head weights the forward used), per batch both Adam steps run with the same t.

        loss_scale (an f16 model with trainable='head_blocks' needs it, nothing else takes it): 'dynamic' -- the rule of Keras'
        LossScaleOptimizer, yolo4hip.loss_scale.LossScale() -- a LossScale of your own, or a power of two as a static scale.  The
        block gradient of every chunk runs through y4_block_grad_scaled with the batch's scale: dZ is multiplied by it before
        its rounding to fp16, the float32 sum divided by it.  One overflow word per batch is read next to the loss; when it is
        set NEITHER group steps (no Adam step, no step count) and a dynamic scale is halved.  `.history` then also holds
        'loss_scale' (the scale at the end of each epoch) and 'skipped_steps' (per epoch).

        Augmentation: a `train_data_gen` whose `augment` is an `AugmentConfig` (DataGenerator(..., augment=, seed=)) is read
        through `raw(i)`: the raw uint8 images cross PCIe once, `Engine.augment_u8_batch` resizes, shifts, flips and colour-shifts
        them in one launch into the uint8 batch the forward takes, and the boxes arrive already transformed.  With
        AugmentConfig.identity() that path gives the bits of the host path.  `val_data_gen` and `evaluate` never take the device
        path: handed an augmenting generator they call `boxes(i)`, which augments on the host and draws from the generator's own
        random stream -- validate on a generator without `augment`.

        Mosaic: with `augment.mosaic > 0` the batch is read through `raw_mosaic(i)` instead: every canvas is, with that
        probability, four images around a random cut.  The distinct photos of the batch cross PCIe once, and
        `Engine.mosaic_u8_batch` writes all canvases in one launch; the merged boxes arrive from the host.  Everything after
        the uint8 batch -- chunks, labels, gradients, Adam -- is the same.

        A callback with a `schedule(epoch, lr)` method (yolo4hip.callbacks.CosineAnnealingScheduler; Keras'
        LearningRateScheduler pattern) is asked at the start of every epoch; its result is that epoch's learning rate.

        val_map=True (needs `val_data_gen`): every epoch's logs and `.history` also hold 'val_mAP', `evaluate_map(val_data_gen)`'s
        mAP at IoU 0.5 with the epoch's weights.

        cache_features=True, or an int byte budget (Keras' "bottleneck features"): everything in front of the trainable convs is
        frozen, so with a generator that does not augment it computes the same tensors for an image in every epoch.  The first
        epoch of the call runs as above and, after each chunk's forward, `Engine.store_features` copies what the engine retains
        -- the head convs' inputs, with trainable='head_blocks' the inputs of convs 92 / 100 / 108 -- into a device cache, one row
        per image at its annotation-line index (`train_data_gen.indexes`).  Every later epoch asks `train_data_gen.labels(i)`
        instead of `boxes(i)` -- no photo is read, no image uploaded -- and per chunk runs `Engine.load_features` ->
        `Engine.forward_tail_device` -> the same assignment, loss, gradient and Adam calls: `.history` and the trained weights
        have the bits of the uncached call.  The cache lives for this call only (`load_model` may change the frozen weights
        between calls).  Refused before any update: an augmenting generator and one without `indexes`, `batch_size` and
        `labels` (ValueError); a cache larger than the budget, or with True than the free device memory (MemoryError naming the
        bytes needed and the bytes per image).  `val_data_gen` is not cached.  False (default): the path above, call for call."""
        from . import fitloop
        groups, policy = fitloop.check_arguments(train_data_gen, val_data_gen, trainable, loss_scale, val_map, cache_features,
                                                 self._dtype, self.max_boxes)
        self._ensure_tuned()
        eng = self._train_engine(2 if 'blocks' in groups else 1)
        state = {g: eng._group_state(g, self._flat) for g in groups}
        grad = {g: eng.torch.empty((eng._group_floats(g),), dtype=eng.torch.float32, device=eng.device) for g in groups}
        cache = None
        if cache_features is not False:
            cache = fitloop.alloc_feature_cache(eng, train_data_gen, cache_features,
                                                f'at {self.img_size} in {self._dtype} with trainable={trainable!r}')
        val_names = () if val_data_gen is None else ('val_loss', 'val_mAP') if val_map else ('val_loss',)

        def validate():
            logs = {}
            if val_data_gen is not None:
                logs['val_loss'] = self.evaluate(val_data_gen)['loss']
                if val_map:
                    logs['val_mAP'] = self.evaluate_map(val_data_gen)['mAP']
            return logs
        return fitloop.run(eng, train_data_gen, groups, state, grad, self._flat, self.iou_loss_thresh,
                           self.engine.load_weight_blob, validate, val_names, epochs, initial_epoch, callbacks, learning_rate,
                           policy, cache)

    def _train_engine(self, level=1):
        """The engine `fit` runs on: created on the first `fit`, with the head convs' inputs retained (the inference engine keeps
        its size for users who never train), the inference engine's schedule, and the current weights.  level 2
        (trainable='head_blocks') is an engine of its own that also retains the inputs of convs 92 / 100 / 108, so that
        trainable='heads' keeps the engine, the workspace and the speed it has."""
        name = '_fit_engine' if level == 1 else '_fit_engine_blocks'
        eng = getattr(self, name, None)
        if eng is None:
            eng = Engine(self.num_classes, self.config, max_batch=self._max_batch, dtype=self._dtype,
                         device=self._device, alias_workspace=True, retain_head_inputs=level, box_loss=self.box_loss,
                         **self.nms_options())
            setattr(self, name, eng)
        eng.load_weight_blob(self._flat)
        self.engine.copy_schedule_to(eng)
        return eng

    # ---- reference models.py:57-65: training_model's inputs [X, y_s, y_m, y_l, true_xywh] -> the yolo_loss Lambda's scalar
    def _loss_of_dense(self, inputs):
        """The dense labels never reach the device: their responsible cells (label[..., 4] == 1) are extracted on the host into
        the sparse records `y4_loss` reads.  Label values other than 0 / 1 (smoothed labels) raise ValueError."""
        from .data import records_from_dense
        from .engine import combine_loss
        if len(inputs) != 5:
            raise ValueError('training_model.predict takes [X, y_small, y_medium, y_large, true_boxes_xywh]')
        X, y_s, y_m, y_l, xywh = inputs
        for y, g in zip((y_s, y_m, y_l), self.engine.grids_hw):
            if tuple(np.shape(y)[1:3]) != tuple(g):
                raise ValueError(f'label grid {tuple(np.shape(y)[1:3])} != {tuple(g)}')
        records = records_from_dense([y_s, y_m, y_l], self.num_classes)
        parts = self.engine.loss(X, records=records, true_xywh=xywh, iou_loss_thresh=self.iou_loss_thresh)
        return np.float32(combine_loss(parts)[0].mean())

    def evaluate(self, data_gen):
        """The validation loss over a `DataGenerator` (yolo4hip.data / the drop-in utils): per batch the images and the
        [n, max_boxes, 5] boxes are uploaded, labels are assigned on the device (y4_loss_assign) and the loss is one read of the
        heads (y4_loss).  -> {'loss', 'box', 'conf', 'class', 'images'}: means over all images of the weighted terms
        (loss = box + conf + class, weights 3.54 / 64.3 / 1 as loss.py:136-140), and the image count."""
        from .engine import combine_loss
        self._ensure_tuned()
        if getattr(data_gen, 'max_boxes', self.max_boxes) != self.max_boxes:
            raise ValueError(f"the generator's max_boxes {data_gen.max_boxes} != config['max_boxes'] {self.max_boxes}")
        sums, images = np.zeros(4), 0
        for i in range(len(data_gen)):
            X, boxes = data_gen.boxes(i)
            parts = self.engine.loss(X, boxes=boxes, iou_loss_thresh=self.iou_loss_thresh)
            sums += np.array([t.sum() for t in combine_loss(parts)])
            images += len(parts)
        if images == 0:
            raise ValueError('evaluate: the generator is empty')
        mean = sums / images
        return {'loss': float(mean[0]), 'box': float(mean[1]), 'conf': float(mean[2]), 'class': float(mean[3]), 'images': images}

    def evaluate_map(self, data, img_folder_path=None, bs=None, *, iou_thresholds=(0.5,), channel_order='rgb', views=None,
                     tile_candidates=1 << 18):
        """VOC mAP with the matching on the device: the numbers of `export_gt` + `export_prediction` + `eval_map`, without the
        text files.  `data` is an annotation file path (then `img_folder_path` is required, images are looked up by file name as
        `export_prediction` does, and `bs` defaults to max_batch) or a `DataGenerator`: its `annotation_lines`, `folder_path` and
        `batch_size` are used, in annotation order -- its shuffle and augmentation are not.  Images are read, batched (`bs`
        images per batch, in file order) and preprocessed as `export_prediction` does (`preprocess_u8_batch`; the letterbox
        path with its box map on a letterbox=True model; this model's thresholds).  Per batch the kept boxes stay on the device:
        `y4_map_match` matches them against the ground truth -- the annotation line's boxes as `export_gt` reads them: raw-image
        pixels, annotation order, every box (no shuffle, no max_boxes cut; at most 256 per image), as float32 -- and one copy
        brings scores, classes, valid and the true-positive flags back; `mapeval.MapAccumulator` turns them into AP.
        iou_thresholds: 1..16 values; -> `eval_map`'s keys (mAP, ap, tp, fp, n_gt, n_images, n_det) at iou_thresholds[0], plus
        per_threshold {thr: {mAP, ap, tp, fp}} and mAP_mean (with numpy.arange(0.5, 1.0, 0.05) the COCO-style summary under VOC
        interpolation).  (A class name with a blank in it, COCO's "wine glass", is no obstacle here; the text files cannot carry it.)
        channel_order: 'rgb' (default) feeds the images as `DataGenerator` and `fit` feed them -- the order the model is trained
        on; 'bgr' feeds what `export_prediction` feeds, the reference's unflipped cv2.imread, and reproduces that pipeline.
        views: None, or a list of (scale, flip) views: each batch then goes through `Engine.predict_tta_device` (test-time
        augmentation: one NMS per image over all its views, merged under nms_merge) instead of the forward and decode + NMS; its
        boxes arrive normalised to each raw image and stay on the device for the matching.  RuntimeError when an image has more
        than tile_candidates candidates, as `predict_tiled`."""
        from .mapeval import MapAccumulator
        items, paths, bs, views = self._eval_items('evaluate_map', data, img_folder_path, bs, channel_order, views)
        self._ensure_tuned()
        eng = self.engine
        acc = MapAccumulator(self.class_names, iou_thresholds)
        for i0, part, raws, gt_dev, scale_dev, count_dev in self._eval_batches(items, paths, bs, channel_order):
            n = len(part)
            flat, outs, tp_mask = eng.alloc_map_outputs_flat(n)
            # with views the map block still comes back in its one copy, the candidate counts (no field of it) in a second small one
            cand = None if views is None else eng.torch.empty((n,), dtype=eng.torch.int32, device=eng.device)
            group_cap = self._eval_infer(raws, (flat, outs, cand), views, tile_candidates=tile_candidates)
            eng.map_match_device(outs, scale_dev, gt_dev, count_dev, acc.iou_thresholds, tp_mask=tp_mask)
            scores, classes, valid, tp = eng.map_outputs_to_host(flat, n)
            if group_cap is not None:
                self._check_candidates('evaluate_map', i0, cand.cpu().numpy(), group_cap)
            acc.add([stem for _, stem, _ in part], scores, classes, valid, tp, [boxes[:, 4] for _, _, boxes in part])
        return acc.result()

    def _eval_infer(self, raws, outputs, views=None, tiled=False, tile=None, overlap=0.2, full_image=True, tile_candidates=1 << 18):
        """The inference of one batch of `evaluate_map` / `evaluate_coco`, under this object's thresholds, letterbox and pad value,
        into outputs = (flat, outs, cand_count): tiled -> `predict_tiled_device`, views -> `predict_tta_device` (both write cand_count),
        else preprocess_u8_batch -> forward -> decode + NMS.  -> group_cap for `_check_candidates`, or None on the plain path."""
        eng = self.engine
        iou, score = self._thresholds
        if tiled:
            return eng.predict_tiled_device(raws, tile, overlap, full_image, self._letterbox, self._pad_value, iou, score,
                                            tile_candidates, views, outputs=outputs)[3]
        if views is not None:
            return eng.predict_tta_device(raws, views, self._letterbox, self._pad_value, iou, score, tile_candidates,
                                          outputs=outputs)[3]
        imgs, box_map = eng.preprocess_u8_batch(raws, letterbox=self._letterbox, pad_value=self._pad_value)
        eng.forward_device(imgs)
        eng.decode_nms_device(len(raws), outputs[1], iou, score, box_map=box_map if self._letterbox else None)
        return None

    def _eval_items(self, who, data, img_folder_path, bs, channel_order, views):
        """The arguments `evaluate_map` and `evaluate_coco` share -> (items of `read_map_annotations`, image paths, bs, views as a
        list or None); ValueError before anything is read or uploaded."""
        from .data import read_map_annotations
        if channel_order not in ('rgb', 'bgr'):
            raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
        if views is not None:
            tiling.check_views(views)
            views = list(views)
        if isinstance(data, (str, os.PathLike)):
            if img_folder_path is None:
                raise ValueError(f'{who}: an annotation file needs img_folder_path')
            with open(data) as fh:
                items = read_map_annotations(fh.readlines(), self.num_classes)
            paths = [os.path.join(img_folder_path, name.split(os.sep)[-1]) for name, _, _ in items]
            bs = self._max_batch if bs is None else int(bs)
        else:
            items = read_map_annotations(data.annotation_lines, self.num_classes)
            paths = [os.path.join(data.folder_path, name) for name, _, _ in items]
            bs = int(data.batch_size) if bs is None else int(bs)
        if bs < 1:
            raise ValueError(f'{who}: bs {bs}')
        if not items:
            raise ValueError(f'{who}: no annotation lines')
        return items, paths, bs, views

    def _eval_batches(self, items, paths, bs, channel_order):
        """The batch loop `evaluate_map` and `evaluate_coco` share: `bs` images per batch in file order, a batch larger than the
        engine's in chunks, as predict does.  Per chunk the images are read, put into the channel order, and the side block --
        per image: boxes | w, h | count (as int32 bits) -- is uploaded in one copy.
        -> (index of the first image, items, raw images, gt_dev [n,256,5], scale_dev [n,2], count_dev int32 [n])."""
        from .data import MAP_MAX_GT
        eng = self.engine
        torch = eng.torch
        step = min(bs, eng.max_batch)
        for start in range(0, len(items), bs):
            for i0 in range(start, min(start + bs, len(items)), step):
                part = items[i0:min(i0 + step, start + bs)]
                n = len(part)
                raws = [prepost.imread_rgb(pth) for pth in paths[i0:i0 + n]]
                if channel_order == 'bgr':
                    raws = [r[:, :, ::-1] for r in raws]
                side = np.zeros((n, MAP_MAX_GT * 5 + 3), dtype=np.float32)
                for k, (raw, (_, _, boxes)) in enumerate(zip(raws, part)):
                    side[k, :boxes.size] = boxes.reshape(-1)
                    side[k, MAP_MAX_GT * 5:MAP_MAX_GT * 5 + 2] = raw.shape[1], raw.shape[0]
                    side[k, MAP_MAX_GT * 5 + 2:].view(np.int32)[0] = len(boxes)
                side_dev = torch.from_numpy(side).to(eng.device)
                gt_dev = side_dev[:, :MAP_MAX_GT * 5].contiguous().view(n, MAP_MAX_GT, 5)
                scale_dev = side_dev[:, MAP_MAX_GT * 5:MAP_MAX_GT * 5 + 2].contiguous()
                count_dev = side_dev[:, MAP_MAX_GT * 5 + 2].contiguous().view(torch.int32)
                yield i0, part, raws, gt_dev, scale_dev, count_dev

    @staticmethod
    def _check_candidates(who, i0, cand, group_cap):
        if (cand > group_cap).any():
            g = int(np.argmax(cand))
            raise RuntimeError(f'{who}: image {i0 + g} has {int(cand[g])} candidates, more than '
                               f'tile_candidates = {group_cap} holds; raise tile_candidates')

    def evaluate_coco(self, data, img_folder_path=None, bs=None, *, channel_order='rgb', views=None, tiled=False, tile=None,
                      overlap=0.2, full_image=True, tile_candidates=1 << 18, max_dets=(1, 10, 100), area_ranges=None):
        """COCO-protocol AP / AR (COCOeval's bbox protocol without crowd regions) with the matching on the device, over the plain,
        the test-time-view or the tiled inference path -- one call answers "what does tiling do to APs on my data".
        `data`, `img_folder_path`, `bs`, `channel_order`, the annotation reading (raw-image pixels, annotation order, every box,
        at most 256 per image, as float32) and the batching are `evaluate_map`'s.  The inference path:
          plain (default)   forward + `decode_nms_device`, as `evaluate_map`;
          views=[...]       `Engine.predict_tta_device`: (scale, flip) views under one NMS per image;
          tiled=True        `Engine.predict_tiled_device(raws, tile, overlap, full_image, ..., views=views)`: windows of `tile`
                            (default the network input) with `overlap`, plus the whole photo when full_image, under one NMS per
                            photo; RuntimeError when a photo has more than tile_candidates candidates (also with views=).
        Every path runs under this object's thresholds, letterbox, pad value, NMS rule and nms_merge.  Per batch the kept boxes
        stay on the device: `y4_coco_match` matches them (the rule: csrc/coco_match.hip) at IoU .50:.05:.95 under `area_ranges`
        (default COCO's all / small / medium / large = [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10] in raw-image pixels; 1..4
        rows in that order), and ONE copy brings scores, classes, valid, the class ranks and the flags back;
        `cocoeval.CocoAccumulator` turns them into precision and recall under `max_dets`.
        -> AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl by name, `stats` (the twelve in COCO's order),
        `per_class` {class name: AP}, `precision` [T,R,K,A,M], `recall` [T,K,A,M], `n_gt` and `n_det` {class name: count}.  A number
        without ground truth in its range is -1.0.
        COCO numbers are normally taken at a very low score_threshold (0.001) with up to 100 boxes per image, so that the
        precision-recall curve reaches far to the right; this method uses the model's own score_threshold as it is -- lower it on
        the model to compare with published tables."""
        from .cocoeval import CocoAccumulator
        from .data import MAP_MAX_GT
        items, paths, bs, views = self._eval_items('evaluate_coco', data, img_folder_path, bs, channel_order, views)
        acc = CocoAccumulator(self.class_names, None, area_ranges, max_dets)          # ValueError on bad ranges / max_dets
        if int(tile_candidates) < 1:
            raise ValueError(f'evaluate_coco: tile_candidates must be >= 1, got {tile_candidates}')
        if tiled:
            if not 0.0 <= float(overlap) < 1.0:
                raise ValueError(f'evaluate_coco: overlap must lie in [0, 1), got {overlap}')
            if tile is not None and (np.ndim(tile) > 1 or np.size(tile) not in (1, 2) or np.min(tile) < 1):
                raise ValueError(f'evaluate_coco: tile must be a positive int or (th, tw), got {tile!r}')
        elif tile is not None:
            raise ValueError('evaluate_coco: tile= needs tiled=True')
        self._ensure_tuned()
        eng = self.engine
        A = len(acc.area_ranges)
        for i0, part, raws, gt_dev, scale_dev, count_dev in self._eval_batches(items, paths, bs, channel_order):
            n = len(part)
            flat, outs, cand_count, match_out = eng.alloc_coco_outputs_flat(n, A, MAP_MAX_GT)
            group_cap = self._eval_infer(raws, (flat, outs, cand_count), views, tiled, tile, overlap, full_image, tile_candidates)
            eng.coco_match_device(outs, scale_dev, gt_dev, count_dev, acc.iou_thresholds, acc.area_ranges, out=match_out)
            scores, classes, valid, cand, rank, dm, di, gi = eng.coco_outputs_to_host(flat, n, A, MAP_MAX_GT)
            if group_cap is not None:
                self._check_candidates('evaluate_coco', i0, cand, group_cap)
            acc.add(scores, classes, valid, rank, dm, di, [boxes[:, 4] for _, _, boxes in part], gi)
        return acc.result()

    # ---- reference models.py:95-98
    def preprocess_img(self, img):
        return prepost.preprocess_img(img, self.img_size)

    def _letterboxed(self, raws):
        """Letterboxed network input for a list of raw images -> (images for engine.predict, box map [n,4]): on the device
        (one upload, one ragged resize) for uint8 images when device_preprocess is on, else prepost.letterbox on the host."""
        if self._device_preprocess and all(getattr(r, 'dtype', None) == np.uint8 for r in raws):
            return self.engine.preprocess_u8_batch(raws, letterbox=True, pad_value=self._pad_value)
        H, W = self.img_size[0], self.img_size[1]
        imgs = np.stack([prepost.letterbox(r, (H, W), self._pad_value) / 255. for r in raws])
        maps = np.stack([prepost.box_map(r.shape[0], r.shape[1], H, W) for r in raws])
        return imgs, maps

    def _predict_mapped(self, imgs, box_map):
        """inference_model.predict with boxes normalised to each raw image (box_map from `_letterboxed`)."""
        self._ensure_tuned()
        iou, score = self._thresholds
        return self.engine.predict(imgs, iou_threshold=iou, score_threshold=score, box_map=box_map)

    # ---- video frames: not in the reference.  8-bit YUV 4:2:0 frames as a decoder delivers them (yolo4hip/yuv.py: YuvFrame) are
    # uploaded as they are, 1.5 bytes per pixel, and converted and resized in one launch (Engine.preprocess_yuv_batch).  Honours this
    # object's letterbox / pad_value, thresholds and every NMS setting.
    def predict_yuv(self, frames, *, matrix='bt601', full_range=False, fmt='nv12'):
        """frames: one `YuvFrame` or a list of them, any mix of sizes, formats and pitches (a 2-D uint8 array [h + h // 2, w] with
        even h, w is a frame of format `fmt`) -> (boxes [n,100,4] normalised to each frame, scores, classes, valid), the form of
        inference_model.predict.  matrix: 'bt601' or 'bt709'; full_range: Y 0..255 instead of 16..235.  The detections are
        those of the RGB frames `yuv.to_rgb` gives, bit for bit."""
        imgs, box_map = self.engine.preprocess_yuv_batch(frames, letterbox=self._letterbox, pad_value=self._pad_value,
                                                         matrix=matrix, full_range=full_range, fmt=fmt)
        return self._predict_mapped(imgs, box_map)

    # ---- reference models.py:109-123 (raw_img: RGB)
    def predict_img(self, raw_img, random_color=True, plot_img=True, figsize=(10, 10), show_text=True,
                    return_output=False):
        print('img shape: ', raw_img.shape)
        if self._letterbox:
            pred_output = self._predict_mapped(*self._letterboxed([raw_img]))
        elif self._device_preprocess and getattr(raw_img, 'dtype', None) == np.uint8:
            # same arithmetic as preprocess_img (tests: bit-identical), on the GPU: the uint8 image crosses PCIe
            pred_output = self.inference_model.predict(self.engine.preprocess_u8(np.ascontiguousarray(raw_img)))
        else:
            pred_output = self.inference_model.predict(np.expand_dims(self.preprocess_img(raw_img), axis=0))
        return self._show(raw_img, pred_output, random_color, plot_img, figsize, show_text, return_output)

    # ---- tiled (sliced) inference: not in the reference.  A photo much larger than the network input is cut into overlapping
    # windows at native resolution (yolo4hip/tiling.py), the windows run as batch rows, and one NMS per photo runs over all rows
    # in the photo's coordinates (Engine.predict_tiled).  Honours this object's letterbox / pad_value (how a window that is not of
    # the network's size, and the full image, go on the canvas), thresholds and NMS rule.  uint8 images only.
    def predict_tiled(self, raw_imgs, *, tile=None, overlap=0.2, full_image=True, tile_candidates=1 << 18, views=None):
        """raw_imgs: one uint8 RGB photo [h,w,3] or a list of them, any sizes -> (boxes [P,100,4] normalised to each photo,
        scores, classes, valid), the form of inference_model.predict.  tile: window size, an int or (th, tw), default the network
        input; overlap: fraction of a tile neighbouring windows share at least; full_image: the whole photo, resized as
        predict_img resizes it, takes part as one more row (large objects); tile_candidates: candidate capacity per photo;
        views: None, or (scale, flip) views every row also runs under (see `predict_tta`)."""
        self._ensure_tuned()
        iou, score = self._thresholds
        return tuple(self.engine.predict_tiled(raw_imgs, tile=tile, overlap=overlap, full_image=full_image,
                                               letterbox=self._letterbox, pad_value=self._pad_value, iou_threshold=iou,
                                               score_threshold=score, tile_candidates=tile_candidates, views=views))

    def _show(self, raw_img, pred_output, random_color, plot_img, figsize, show_text, return_output):
        """The DataFrame and drawing of `predict_img` for outputs normalised to the photo."""
        detections = prepost.get_detection_data(img=raw_img, model_outputs=pred_output, class_names=self.class_names)
        output_img = prepost.draw_bbox(raw_img, detections, cmap=self.class_color, random_color=random_color,
                                       figsize=figsize, show_text=show_text, show_img=plot_img)
        return (output_img, detections) if return_output else detections

    def predict_img_tiled(self, raw_img, random_color=True, plot_img=True, figsize=(10, 10), show_text=True,
                          return_output=False, *, tile=None, overlap=0.2, full_image=True, views=None):
        """`predict_img` through `predict_tiled`: the same prints, drawing and DataFrame, boxes in the photo's pixels."""
        print('img shape: ', raw_img.shape)
        pred_output = self.predict_tiled([raw_img], tile=tile, overlap=overlap, full_image=full_image, views=views)
        return self._show(raw_img, pred_output, random_color, plot_img, figsize, show_text, return_output)

    # ---- test-time augmentation: not in the reference (YOLOv5's augment=True).  The photo runs under several views -- the
    # rectangle it occupies shrunk about its centre, the canvas mirrored (yolo4hip/tiling.py: view_rows) -- as batch rows, and one
    # NMS per photo runs over the candidates of all views in the photo's coordinates (Engine.predict_tta); with nms_merge the
    # copies of an object become one score-weighted box.  Views are call arguments, not state.  uint8 images only.
    def predict_tta(self, raw_imgs, *, views=tiling.DEFAULT_VIEWS, tile_candidates=1 << 18):
        """raw_imgs: one uint8 RGB photo [h,w,3] or a list of them, any sizes -> (boxes [P,100,4] normalised to each photo,
        scores, classes, valid), the form of inference_model.predict.  views: a list of (scale in (0, 1], flip in '', 'lr', 'ud',
        'lrud'), at most 16, no duplicates; ((1.0, ''),) is `predict_img`'s own path."""
        self._ensure_tuned()
        iou, score = self._thresholds
        return tuple(self.engine.predict_tta(raw_imgs, views=views, letterbox=self._letterbox, pad_value=self._pad_value,
                                             iou_threshold=iou, score_threshold=score, tile_candidates=tile_candidates))

    def predict_img_tta(self, raw_img, random_color=True, plot_img=True, figsize=(10, 10), show_text=True,
                        return_output=False, *, views=tiling.DEFAULT_VIEWS):
        """`predict_img` through `predict_tta`: the same prints, drawing and DataFrame, boxes in the photo's pixels."""
        print('img shape: ', raw_img.shape)
        pred_output = self.predict_tta([raw_img], views=views)
        return self._show(raw_img, pred_output, random_color, plot_img, figsize, show_text, return_output)

    # ---- reference models.py:125-127
    def predict(self, img_path, random_color=True, plot_img=True, figsize=(10, 10), show_text=True):
        raw_img = prepost.imread_rgb(img_path)
        return self.predict_img(raw_img, random_color, plot_img, figsize, show_text)

    # ---- reference models.py:129-139: annotation lines "path x1,y1,x2,y2,cls ..." -> one "<name> x1 y1 x2 y2" file each
    def export_gt(self, annotation_path, gt_folder_path):
        with open(annotation_path) as fh:
            for line in fh:
                fields = line.split(' ')
                stem = fields[0].split(os.sep)[-1].split('.')[0]
                with open(os.path.join(gt_folder_path, stem + '.txt'), 'w') as out:
                    for obj in fields[1:]:
                        x_min, y_min, x_max, y_max, class_id = [float(v) for v in obj.strip().split(',')]
                        out.write(f'{self.class_names[int(class_id)]} {x_min} {y_min} {x_max} {y_max}\n')

    # ---- reference models.py:141-179: the reference's only BATCHED caller of inference_model.predict.
    # One "<class> <score> <x1> <y1> <x2> <y2>" line per detection, coordinates in raw-image pixels.  Like the
    # reference it feeds cv2.imread's BGR channel order (no flip, unlike predict()).
    def export_prediction(self, annotation_path, pred_folder_path, img_folder_path, bs=2):
        with open(annotation_path) as fh:
            img_paths = [os.path.join(img_folder_path, line.split(' ')[0].split(os.sep)[-1].strip()) for line in fh]
        try:
            from tqdm import tqdm
        except ImportError:                      # progress bar only
            def tqdm(it):
                return it
        for start in tqdm(range(0, len(img_paths), bs)):
            paths = img_paths[start:start + bs]
            raws = [prepost.imread_rgb(pth)[:, :, ::-1] for pth in paths]
            if self._letterbox:                   # boxes come back normalised to each raw image: the * w, * h below hold
                imgs, box_map = self._letterboxed(raws)
                b_boxes, b_scores, b_classes, b_valid = self._predict_mapped(imgs, box_map)
            else:
                if self._device_preprocess:       # one upload + one ragged stretch launch: the bytes of preprocess_u8
                    imgs, _ = self.engine.preprocess_u8_batch(raws)
                else:
                    imgs = np.stack([self.preprocess_img(r) for r in raws])
                b_boxes, b_scores, b_classes, b_valid = self.inference_model.predict(imgs)
            for k, pth in enumerate(paths):
                nb = int(b_valid[k])
                h, w = raws[k].shape[:2]
                boxes = b_boxes[k, :nb]
                boxes[:, [0, 2]] *= w                 # the returned arrays are writable host copies
                boxes[:, [1, 3]] *= h
                names = [self.class_names[int(c)] for c in b_classes[k, :nb]]
                stem = pth.split(os.sep)[-1].split('.')[0]
                with open(os.path.join(pred_folder_path, stem + '.txt'), 'w') as out:
                    for j in range(nb):
                        b = boxes[j]
                        out.write(f'{names[j]} {b_scores[k, j]} {b[0]} {b[1]} {b[2]} {b[3]}\n')

    # ---- reference models.py:182-507: VOC mAP over the folders export_gt / export_prediction wrote (text outputs and
    # prints kept, matplotlib windows not; also returns the numbers) -- see yolo4hip/evalmap.py
    def eval_map(self, gt_folder_path, pred_folder_path, temp_json_folder_path, output_files_path):
        from .evalmap import eval_map
        return eval_map(gt_folder_path, pred_folder_path, temp_json_folder_path, output_files_path)

    # ---- reference models.py:509-514 (note: no BGR->RGB flip there; cv2.imread order is BGR)
    def predict_raw(self, img_path):
        raw_img = prepost.imread_rgb(img_path)[:, :, ::-1]
        print('img shape: ', raw_img.shape)
        img = self.preprocess_img(raw_img)
        imgs = np.expand_dims(img, axis=0)
        return self.yolo_model.predict(imgs)

    # ---- reference models.py:516-529 (thresholds as run-time arguments)
    def predict_nonms(self, img_path, iou_threshold=0.413, score_threshold=0.1):
        raw_img = prepost.imread_rgb(img_path)[:, :, ::-1]
        print('img shape: ', raw_img.shape)
        img = self.preprocess_img(raw_img)
        imgs = np.expand_dims(img, axis=0)
        print(f'nms iou: {iou_threshold} score: {score_threshold}')
        self._ensure_tuned()
        pred_output = self.engine.predict(imgs, iou_threshold=iou_threshold, score_threshold=score_threshold)
        detections = prepost.get_detection_data(img=raw_img, model_outputs=pred_output, class_names=self.class_names)
        prepost.draw_bbox(raw_img, detections, cmap=self.class_color, random_color=True)
        return detections


def load_weights(model, weights_file_path):
    """reference utils.py:12-53: read a Darknet `.weights` file into the model.  `model` is a `Yolov4`
    (the reference passes the Keras `yolo_model`; the facade object owns the engine here)."""
    ws, _header, unread = W.read_darknet(weights_file_path, model.plan)
    model._set_weights(W.flatten(ws))
    if unread == 0:
        print('all weights read')
    else:
        print(f'failed to read  all weights, # of unread weights: {unread}')


def default_class_path(name='coco_classes.txt'):
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'class_names', name)
