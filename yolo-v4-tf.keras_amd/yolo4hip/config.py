"""Inference constants of the path (mirror of the reference's module-global dict, `config.py:1-17`).

The inference path reads the Basic and Inference keys.  Of the training keys, `iou_loss_thresh` is the ignore
threshold of the validation loss (`Yolov4.training_model`, `Yolov4.evaluate`), and `batch_size` x `num_gpu` is the
batch of `DataGenerator`; nothing here trains.  Unlike the reference (`models.py:26-37` ignores the ctor's `config=` argument),
`Yolov4(config=...)` honours a passed dict.
"""

yolo_config = {
    # Basic
    'img_size': (416, 416, 3),
    'anchors': [12, 16, 19, 36, 40, 28, 36, 75, 76, 55, 72, 146, 142, 110, 192, 243, 459, 401],
    'strides': [8, 16, 32],
    'xyscale': [1.2, 1.1, 1.05],

    # Training (the validation loss and DataGenerator read them; there is no fit)
    'iou_loss_thresh': 0.5,
    'batch_size': 8,
    'num_gpu': 1,

    # Inference
    'max_boxes': 100,
    'iou_threshold': 0.413,
    'score_threshold': 0.3,
}


def make_config(img_size=416, **overrides):
    """Copy of `yolo_config` at another resolution: a square side (e.g. 608 for the headline configs) or (H, W), height
    first like the Keras Input shape (e.g. (352, 608) for 16:9 frames) -> img_size (H, W, 3)."""
    cfg = dict(yolo_config)
    if isinstance(img_size, (tuple, list)):
        cfg['img_size'] = (int(img_size[0]), int(img_size[1]), 3)
    else:
        cfg['img_size'] = (int(img_size), int(img_size), 3)
    cfg.update(overrides)
    return cfg
