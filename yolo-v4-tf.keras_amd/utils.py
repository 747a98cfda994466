"""Drop-in for the inference-path names of the reference's `utils.py`
(`load_weights` :12-53, `get_detection_data` :56-78, `draw_bbox` :88-118, `voc_ap` :311-356, `read_txt_to_list` :469-475) and of its label side (`read_annotation_lines` :80-86, `DataGenerator` :121-212,
`preprocess_true_boxes` :215-303); `AugmentConfig` (yolo4hip.augment) is what `DataGenerator(..., augment=)` takes, and
`dataset_wh` / `fit_anchors` (yolo4hip.anchors, not in the reference) fit the nine anchors to a data set on the device;
`YuvFrame` / `yuv_to_rgb` / `yuv_from_rgb` (yolo4hip.yuv, not in the reference) describe 4:2:0 video frames for `Yolov4.predict_yuv`."""
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
from yolo4hip.api import load_weights  # noqa: E402,F401
from yolo4hip.prepost import get_detection_data, draw_bbox  # noqa: E402,F401
from yolo4hip.evalmap import voc_ap, read_txt_to_list  # noqa: E402,F401
from yolo4hip.data import read_annotation_lines, DataGenerator, preprocess_true_boxes  # noqa: E402,F401
from yolo4hip.augment import AugmentConfig  # noqa: E402,F401
from yolo4hip.anchors import dataset_wh, fit_anchors  # noqa: E402,F401
from yolo4hip.yuv import YuvFrame, to_rgb as yuv_to_rgb, from_rgb as yuv_from_rgb  # noqa: E402,F401
