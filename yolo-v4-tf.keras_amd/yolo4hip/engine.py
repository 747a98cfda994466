"""Engine: one libyolo4hip handle on one GPU, with its workspaces held as torch-ROCm tensors.

Stands where TensorFlow's runtime stands in the reference: `Yolov4.yolo_model.predict`
and `Yolov4.inference_model.predict` (reference models.py:113,159,514) end up in `Engine.forward_heads`
/ `Engine.predict`.  No compute happens in Python and nothing here falls back to a CPU path.
"""
import ctypes as C
import os

import numpy as np

from . import canvas, ext, schedule, tiling
from .config import yolo_config


def _img_hw(config):
    """(H, W) of config['img_size'] = (H, W, 3), the Keras Input shape (height first)."""
    size = config["img_size"]
    return int(size[0]), int(size[1])


def _cfg_struct(config, num_classes, max_batch, dtype, max_per_class=100, max_total=100):
    c = ext.y4_config()
    H, W = _img_hw(config)
    # reference models.py:24, for each side (its models.py:23 'not support yet' for H != W is lifted: y4_create_hw)
    assert H % config["strides"][-1] == 0 and W % config["strides"][-1] == 0, "must be a multiple of last stride"
    assert num_classes > 0, "no classes detected!"                   # models.py:38
    c.img_size = H; c.num_classes = int(num_classes); c.max_batch = int(max_batch)     # (img_size: y4_create only)
    c.dtype = ext.DTYPE_IDS[dtype] if isinstance(dtype, str) else int(dtype)
    anchors = np.asarray(config["anchors"], dtype=np.float32).reshape(-1)
    assert anchors.size == 18, "9 anchors (w,h) expected"
    for i in range(18):
        c.anchors[i] = float(anchors[i])
    for i in range(3):
        c.xyscale[i] = float(config["xyscale"][i])
        c.strides[i] = int(config["strides"][i])
    c.iou_threshold = float(config["iou_threshold"])
    c.score_threshold = float(config["score_threshold"])
    c.max_per_class = int(max_per_class)        # custom_layers.py:293 (hard-coded to 100 in the reference)
    c.max_total = int(max_total)                # custom_layers.py:294 (likewise)
    return c


# Several results as views of ONE int32 block, so that they cross PCIe in a single copy.  A block is described by its fields,
# [(dtype name, shape)] in element order, every dtype four bytes wide.
def _detection_fields(n, T):
    """boxes, scores, classes, valid, kept of n images (`Engine.alloc_outputs`)."""
    return [("float32", (n, T, 4)), ("float32", (n, T)), ("float32", (n, T)), ("int32", (n,)), ("int32", (n, T))]


def _block_len(fields):
    return sum(int(np.prod(shape)) for _, shape in fields)


def _block_views(flat, fields):
    """The fields of a block as views of `flat`, a 1-D int32 torch tensor (device or pinned host) or numpy array."""
    lib = np
    if not isinstance(flat, np.ndarray):
        import torch as lib
    views, at = [], 0
    for dtype, shape in fields:
        part = flat[at:at + int(np.prod(shape))]
        at += int(np.prod(shape))
        views.append((part if dtype == "int32" else part.view(getattr(lib, dtype))).reshape(shape))
    return views


# the keywords of the NMS stage, of Engine and of Yolov4 alike
NMS_OPTIONS = ("nms_kind", "nms_beta", "nms_agnostic", "nms_merge", "nms_soft", "nms_sigma", "nms_soft_min_score", "nms_top_k", "nms_matrix")


class Engine:
    def __init__(self, num_classes, config=None, max_batch=32, dtype="f32", device=None, alias_workspace=False,
                 retain_head_inputs=False, **kw):
        """**kw: the keyword-only arguments of `_build`, where their defaults are written."""
        self._build(num_classes, config, max_batch, dtype, device, alias_workspace, retain_head_inputs, None, **kw)

    def _build(self, num_classes, config, max_batch, dtype, device, alias_workspace, retain_head_inputs, parent, *,
               max_per_class=100, max_total=100, box_loss="giou", nms_kind="iou", nms_beta=0.6, nms_agnostic=False,
               nms_merge=False, nms_soft=None, nms_sigma=0.5, nms_soft_min_score=None, nms_top_k=4096, nms_matrix=None):
        """What `__init__` and `sibling` share: the handle, its workspaces and every attribute.  `parent` is None for an engine
        with weights of its own, or the engine whose packed weights and schedule this one takes over."""
        box_kind = self._box_kind(box_loss)           # (an unknown name is refused before anything is loaded or created)
        nms_rule = self._nms_rule(nms_kind, nms_beta, nms_agnostic)      # (likewise)
        self.nms_merge = self._merge_flag(nms_merge)                     # (likewise); a sibling takes its parent's
        # nms_sigma / nms_soft_min_score / nms_top_k parameterise whichever of nms_soft / nms_matrix is set
        soft_mode = self._decay_mode("soft", nms_soft, nms_sigma, nms_soft_min_score, nms_top_k)      # (likewise)
        matrix_mode = self._decay_mode("matrix", nms_matrix, nms_sigma, nms_soft_min_score, nms_top_k)
        if soft_mode[0] and matrix_mode[0]:
            raise ValueError(f"nms_soft={nms_soft!r} and nms_matrix={nms_matrix!r} exclude each other")
        import torch
        self.torch = torch
        self.lib = ext.load()
        if not torch.cuda.is_available():
            raise RuntimeError("yolo4hip needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.config = dict(config or yolo_config)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.num_classes = int(num_classes)
        self.max_batch = int(max_batch)
        self.cfg = _cfg_struct(self.config, num_classes, max_batch, dtype, max_per_class, max_total)
        self.dtype = ext.DTYPE_NAMES[self.cfg.dtype]
        # img_size: the side of a square engine (as before), (H, W) of a rectangular one; img_hw is (H, W) either way
        self.img_hw = _img_hw(self.config)
        self.img_size = self.img_hw[0] if self.img_hw[0] == self.img_hw[1] else self.img_hw
        self.handle = C.c_void_p()
        ext.check(self.lib.y4_create_hw(C.byref(self.cfg), self.img_hw[0], self.img_hw[1], C.byref(self.handle)))
        # box_loss: the box term of `loss` and of every gradient, 'giou' (what the reference's loss.py has switched on) or 'ciou'
        # (its bbox_ciou, the line under it); a sibling takes its parent's
        if box_kind:                              # (the default is the handle's own: nothing to set)
            ext.check(self.lib.y4_set_box_loss(self.handle, box_kind))
        self.box_loss = self.BOX_LOSSES[box_kind]
        # nms_kind / nms_beta / nms_agnostic: the pair rule of the NMS stage (`set_nms_rule`); a sibling takes its parent's
        self._apply_nms_rule(nms_rule)
        # nms_soft / nms_sigma / nms_soft_min_score / nms_top_k: Soft-NMS instead of hard suppression (`set_nms_soft`); likewise
        self._apply_decay_mode("soft", soft_mode)
        # nms_matrix: Matrix-NMS (`set_nms_matrix`); likewise -- and its own sigma, floor and top_k, which no keyword carries
        self._apply_decay_mode("matrix", matrix_mode if parent is None else parent._decay_state("matrix"))
        flops, nbox, hcs, wfl = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        ext.check(self.lib.y4_model_info(self.handle, C.byref(flops), C.byref(nbox), C.byref(hcs), C.byref(wfl)))
        self.flops_per_image, self.num_boxes = flops.value, nbox.value
        self.head_cstride, self.weight_floats = hcs.value, wfl.value
        # alias_workspace: activation buffers with disjoint lifetimes share memory (y4_set_workspace_aliasing): ~4x less
        # activation memory; conv_output() taps are then unavailable
        self.alias_workspace = bool(alias_workspace)
        if self.alias_workspace:
            ext.check(self.lib.y4_set_workspace_aliasing(self.handle, 1))
        # retain_head_inputs: the head convs' inputs stay in the workspace after a forward (y4_set_retain_head_inputs), which
        # `head_grad_device` needs; level 2 also keeps the inputs of convs 92 / 100 / 108, which `block_grad_device` needs.
        # A sibling computes batches for inference: it records its parent's level, its own handle retains nothing.
        self.retain_level = int(retain_head_inputs)
        if self.retain_level not in (0, 1, 2):
            raise ValueError(f"retain_head_inputs must be False / True (0 / 1) or 2, got {retain_head_inputs!r}")
        self.retain_head_inputs = self.retain_level > 0
        if self.retain_head_inputs and parent is None:
            ext.check(self.lib.y4_set_retain_head_inputs(self.handle, self.retain_level))
        if parent is None:
            a, w = C.c_size_t(), C.c_size_t()
            ext.check(self.lib.y4_workspace_bytes(self.handle, C.byref(a), C.byref(w)))
            self.act_bytes, self.wts_bytes = a.value, w.value
        else:
            self.act_bytes, self.wts_bytes = parent.act_bytes, parent.wts_bytes
        with torch.cuda.device(self.device):
            self.act = torch.empty(self.act_bytes, dtype=torch.uint8, device=self.device)
            # a sibling's is the SAME tensor: packed weights are never written after packing
            self.wts = torch.zeros(self.wts_bytes, dtype=torch.uint8, device=self.device) if parent is None else parent.wts
            ext.check(self.lib.y4_bind_workspace(self.handle, ext.ptr(self.act), self.act_bytes, ext.ptr(self.wts),
                                                 self.wts_bytes))
        self.grids_hw = [(self.img_hw[0] // s, self.img_hw[1] // s) for s in self.config["strides"]]
        self.grids = [g[0] for g in self.grids_hw] if self.img_hw[0] == self.img_hw[1] else list(self.grids_hw)
        self.nout = 3 * (self.num_classes + 5)
        self.T = self.cfg.max_total
        self.stem_fusion = self.halo2 = False
        if parent is not None:
            self.adopt_packed()
            parent.copy_schedule_to(self)
        elif self.dtype != "f32" and os.environ.get("YOLO4HIP_HALO2", "0") == "1":
            self.set_halo2(True)          # (experiments: `autotune` may pick the halo2 tiles; shipped schedules that hold them need no switch)

    def sibling(self):
        """A second handle on the same GPU that SHARES this engine's packed weights (read-only) and owns a second activation
        workspace, with the same scheduling choices (fusions, tuned tiles).  Two independent batches can then be in flight
        on two HIP streams (`InFlight`): one batch's partial last rounds, its 32-workgroup NMS and its small 19^2 layers
        overlap the other batch's kernels.  Results are those of this engine, bit for bit."""
        e = Engine.__new__(Engine)
        e._build(self.num_classes, self.config, self.max_batch, self.dtype, self.device, self.alias_workspace, self.retain_level, self,
                 max_per_class=self.cfg.max_per_class, max_total=self.cfg.max_total, box_loss=self.box_loss, **self.nms_options())
        return e

    BOX_LOSSES = ("giou", "ciou")          # the kinds of y4_set_box_loss, by number

    @classmethod
    def _box_kind(cls, name):
        if name not in cls.BOX_LOSSES:
            raise ValueError(f"box_loss must be one of {cls.BOX_LOSSES}, got {name!r}")
        return cls.BOX_LOSSES.index(name)

    def set_box_loss(self, name):
        """The box term `loss_device` / `loss` and every gradient evaluate from now on: 'giou' or 'ciou' (y4_set_box_loss; host
        state of the handle, settable at any time).  Siblings made later inherit it."""
        ext.check(self.lib.y4_set_box_loss(self.handle, self._box_kind(name)))
        self.box_loss = name

    NMS_KINDS = ("iou", "diou")            # the kinds of y4_set_nms_rule, by number

    @classmethod
    def _nms_rule(cls, kind, beta, agnostic):
        """-> (kind number, beta, agnostic 0 / 1), or ValueError.  beta is validated also for 'iou', which ignores it."""
        if kind not in cls.NMS_KINDS:
            raise ValueError(f"nms_kind must be one of {cls.NMS_KINDS}, got {kind!r}")
        try:
            b = float(beta)
        except (TypeError, ValueError):
            raise ValueError(f"nms_beta must be a finite number > 0, got {beta!r}") from None
        if not (np.isfinite(b) and b > 0.0):
            raise ValueError(f"nms_beta must be a finite number > 0, got {beta!r}")
        if agnostic not in (False, True, 0, 1):
            raise ValueError(f"nms_agnostic must be False or True, got {agnostic!r}")
        return cls.NMS_KINDS.index(kind), b, int(bool(agnostic))

    def _apply_nms_rule(self, rule, force=False):
        kind, beta, agnostic = rule
        if force or rule != (0, 1.0, 0):          # (that is the handle's own rule: 'iou' ignores beta, nothing to set)
            ext.check(self.lib.y4_set_nms_rule(self.handle, kind, 1.0 if kind == 0 else beta, agnostic))
        self.nms_kind, self.nms_beta, self.nms_agnostic = self.NMS_KINDS[kind], beta, bool(agnostic)

    def set_nms_rule(self, kind, beta=0.6, agnostic=False):
        """The pair rule every later predict / decode_nms call of this engine runs (y4_set_nms_rule; host state of the handle,
        settable at any time): kind 'iou' -- suppress iff IoU > iou_threshold, what tf.image.combined_non_max_suppression does --
        or 'diou' -- iff IoU - (d^2 / c^2)^beta > iou_threshold (DIoU-NMS; Darknet's nms_kind=diounms, beta_nms=0.6); agnostic:
        a kept box suppresses later candidates of every class, not only its own.  `beta` is ignored by 'iou' but validated.
        The stream siblings this engine already has follow; siblings made later inherit it."""
        self._apply_nms_rule(self._nms_rule(kind, beta, agnostic), force=True)
        self._tell_siblings("set_nms_rule", kind, beta, agnostic)

    SOFT_METHODS = (None, "gaussian", "linear", "hard")      # the methods of y4_set_nms_soft, by number
    MATRIX_METHODS = (None, "gaussian", "linear")            # the methods of y4_set_nms_matrix, by number
    SOFT_TOP_K_MAX = 4096
    # the two score-decay modes: (method names, setter, the attributes of method / sigma / min_score / top_k -- the first is also the
    # keyword of the method).  The keywords nms_sigma / nms_soft_min_score / nms_top_k serve both, so messages name those.
    _DECAY = {"soft": (SOFT_METHODS, "y4_set_nms_soft", ("nms_soft", "nms_sigma", "nms_soft_min_score", "nms_top_k")),
              "matrix": (MATRIX_METHODS, "y4_set_nms_matrix", ("nms_matrix", "nms_matrix_sigma", "nms_matrix_min_score", "nms_matrix_top_k"))}

    @classmethod
    def _decay_mode(cls, family, method, sigma, min_score, top_k):
        """-> (method number, sigma, min_score or None, top_k), or ValueError.  Every value is validated for every method."""
        methods, _, attrs = cls._DECAY[family]
        if method is not None and not isinstance(method, str) or method not in methods:
            raise ValueError(f"{attrs[0]} must be one of {methods}, got {method!r}")
        try:
            sg = float(sigma)
        except (TypeError, ValueError):
            raise ValueError(f"nms_sigma must be a finite number > 0, got {sigma!r}") from None
        if not (np.isfinite(sg) and sg > 0.0):
            raise ValueError(f"nms_sigma must be a finite number > 0, got {sigma!r}")
        ms = None
        if min_score is not None:
            try:
                ms = float(min_score)
            except (TypeError, ValueError):
                raise ValueError(f"nms_soft_min_score must be None or a number in [0, 1), got {min_score!r}") from None
            if not (np.isfinite(ms) and 0.0 <= ms < 1.0):
                raise ValueError(f"nms_soft_min_score must be None or a number in [0, 1), got {min_score!r}")
        if isinstance(top_k, (bool, np.bool_)) or not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= cls.SOFT_TOP_K_MAX:
            raise ValueError(f"nms_top_k must be an integer in 1 .. {cls.SOFT_TOP_K_MAX}, got {top_k!r}")
        return methods.index(method), sg, ms, int(top_k)

    def _decay_state(self, family):
        """The mode of `family` this engine is in, as `_decay_mode` returns it."""
        methods, _, attrs = self._DECAY[family]
        method, sigma, min_score, top_k = (getattr(self, a) for a in attrs)
        return methods.index(method), sigma, min_score, top_k

    def _apply_decay_mode(self, family, mode, force=False):
        methods, setter, attrs = self._DECAY[family]
        method, sigma, min_score, top_k = mode
        if force or mode != (0, 0.5, None, self.SOFT_TOP_K_MAX):     # (that is the handle's own mode: nothing to set)
            ext.check(getattr(self.lib, setter)(self.handle, method, sigma, -1.0 if min_score is None else min_score, top_k))
        for a, v in zip(attrs, (methods[method], sigma, min_score, top_k)):
            setattr(self, a, v)

    def _set_decay(self, family, method, sigma, min_score, top_k):
        """`set_nms_soft` / `set_nms_matrix`: validate, refuse while the other mode is on, set, tell the stream siblings."""
        mode = self._decay_mode(family, method, sigma, min_score, top_k)
        own, other = self._DECAY[family][2][0], self._DECAY["matrix" if family == "soft" else "soft"][2][0]
        if mode[0] and getattr(self, other, None) is not None:
            raise ValueError(f"{own}={method!r} while {other}={getattr(self, other)!r}: the two decay modes exclude each other")
        self._apply_decay_mode(family, mode, force=True)
        self._tell_siblings("set_" + own, method, sigma, min_score, top_k)

    def _tell_siblings(self, setter, *args):
        """The stream siblings this engine already has follow a setter of NMS state."""
        for e in getattr(self, "_stream_siblings", []):
            getattr(e, setter)(*args)

    def set_nms_soft(self, method, sigma=0.5, min_score=None, top_k=4096):
        """Soft-NMS for every later predict / decode_nms / nms_gathered / predict_tiled / predict_tta call of this engine
        (y4_set_nms_soft; host state of the handle, settable at any time).  method None: off, the hard kernel as before.
        'gaussian': a kept box multiplies the score of every live neighbour of its class (of any class under an agnostic rule) by
        exp(-m^2 / sigma), m the measure of `set_nms_rule`; 'linear': by 1 - m where m > iou_threshold; 'hard': by 0 there -- the
        hard rule in this kernel, equal to method None bit for bit while no list is longer than top_k.  The next box kept is the one
        with the best CURRENT score, output scores are the decayed ones, a box whose score falls to `min_score` or below is gone
        (None: the config's score_threshold; a run-time score threshold of a call does not change it), and only the `top_k` best
        candidates of a list take part (at most 4096).  Every value is validated for every method.  With `nms_merge` on, the
        merge runs behind it unchanged: only the boxes move.  The stream siblings this engine already has follow; siblings made
        later inherit it."""
        self._set_decay("soft", method, sigma, min_score, top_k)

    def set_nms_matrix(self, method, sigma=0.5, min_score=None, top_k=4096):
        """Matrix-NMS (Wang et al. 2020) for every later predict / decode_nms / nms_gathered / predict_tiled / predict_tta call of
        this engine (y4_set_nms_matrix; host state of the handle, settable at any time).  method None: off.  'gaussian' / 'linear':
        the `top_k` best candidates of a list (at most 4096), ordered by score, decay each other in one shot -- candidate j's score
        is multiplied by the minimum over the earlier candidates i of its class (of any class under an agnostic rule) of
        exp((c_i^2 - m_ij^2) / sigma), or of (1 - m_ij) / (1 - c_i), m the positive part of the measure of `set_nms_rule` and c_i
        the largest m of i against anything earlier -- and the results are the decayed scores above `min_score` (None: the
        config's score_threshold) in their new order, under max_per_class and max_total.  iou_threshold plays no part in the
        decay.  It excludes Soft-NMS: ValueError when `nms_soft` is on (and `set_nms_soft` refuses while this is on).  The
        stream siblings this engine already has follow; siblings made later inherit it."""
        self._set_decay("matrix", method, sigma, min_score, top_k)

    def nms_options(self):
        """The `nms_*` keywords an Engine in this one's NMS state is built with (`sibling`; `Yolov4.nms_options` is its twin)."""
        return {k: getattr(self, k) for k in NMS_OPTIONS}

    @staticmethod
    def _merge_flag(on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"nms_merge must be False or True, got {on!r}")
        return bool(on)

    def set_nms_merge(self, on):
        """Merge-NMS (box voting) on or off for every later predict / decode_nms / nms_gathered / predict_tiled call of this
        engine: each kept box is then replaced by the score-weighted mean of the candidates it absorbed -- same class (any class
        under an agnostic rule) and a pair measure above the iou threshold of the call, under the rule of `set_nms_rule`
        (y4_decode_nms_merged, y4_nms_gathered_merged).  The kept set, scores, classes, valid and kept indices are unchanged,
        bit for bit; only the boxes move.  Host state of this object: with the flag off every call is the plain entry point.
        The stream siblings this engine already has follow; siblings made later inherit it."""
        self.nms_merge = self._merge_flag(on)
        self._tell_siblings("set_nms_merge", on)

    def _merge_counts(self, n):
        """The [n] int32 device words the merged entry points save the candidate counts in (kept for the engine's lifetime)."""
        buf = getattr(self, "_merge_count_buf", None)
        if buf is None or buf.numel() < n:
            buf = self._merge_count_buf = self.torch.empty((max(int(n), self.max_batch),), dtype=self.torch.int32, device=self.device)
        return buf[:n]

    # what the Python side remembers of the handle's schedule (`stem_fusion`: tests/test_gpu_api.py; `halo2`: the YOLO4HIP_HALO2 switch)
    _SCHEDULE_SHADOWS = ("stem_fusion", "halo2")

    def copy_schedule_to(self, e):
        """Give engine `e` (a sibling) this engine's scheduling choices: sub-batching, fusions, every run's state, tuned tiles
        (y4_copy_schedule copies the handle's Schedule; a get_tiles -> set_tiles hop would not carry the switches)."""
        ext.check(self.lib.y4_copy_schedule(self.handle, e.handle))
        for name in self._SCHEDULE_SHADOWS:
            setattr(e, name, getattr(self, name))

    def close(self):
        for e in getattr(self, "_stream_siblings", []):
            e.close()
        self._stream_siblings = []
        self._stream_slots = None                          # predict_stream's pinned staging buffers
        self._batch_pin = None                             # preprocess_u8_batch's staging buffer and packing threads
        if getattr(self, "_pack_pool", None) is not None:
            self._pack_pool.shutdown(wait=True)
            self._pack_pool = None
        if getattr(self, "handle", None) is not None and self.handle:
            self.lib.y4_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- weights
    def load_weight_blob(self, flat):
        """flat: float32 Darknet stream (numpy or torch; see weights.flatten / read_darknet)."""
        torch = self.torch
        if isinstance(flat, np.ndarray):
            flat = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32))
        flat = flat.to(self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_pack_weights(self.handle, ext.ptr(flat), flat.numel(), ext.stream_ptr()))
            torch.cuda.current_stream().synchronize()      # `flat` may be freed after this returns

    # packed-weight cache: the packed workspace is a pure function of (weights, classes, dtype,
    # library layout version), so it can be written once and re-loaded without re-reading / re-packing the
    # 258 MB Darknet file.
    def save_packed(self, path):
        import json
        meta = {"version": self.lib.y4_version().decode(), "num_classes": self.num_classes, "dtype": self.dtype,
                "wts_bytes": self.wts_bytes}
        blob = self.wts.cpu().numpy()
        with open(path, "wb") as f:
            head = json.dumps(meta).encode()
            f.write(len(head).to_bytes(8, "little")); f.write(head); blob.tofile(f)

    def load_packed(self, path):
        import json
        with open(path, "rb") as f:
            n = int.from_bytes(f.read(8), "little")
            meta = json.loads(f.read(n).decode())
            want = {"version": self.lib.y4_version().decode(), "num_classes": self.num_classes, "dtype": self.dtype,
                    "wts_bytes": self.wts_bytes}
            if meta != want:
                raise ValueError(f"packed-weight cache {path} was written for {meta}, this engine needs {want}")
            blob = np.fromfile(f, dtype=np.uint8)
        if blob.size != self.wts_bytes:
            raise ValueError(f"packed-weight cache {path} is truncated: {blob.size} of {self.wts_bytes} bytes")
        self.wts.copy_(self.torch.from_numpy(blob).to(self.device))
        self.torch.cuda.synchronize(self.device)
        self.adopt_packed()

    def adopt_packed(self):
        ext.check(self.lib.y4_adopt_packed_weights(self.handle))

    def workspace_map(self):
        """The regions of `self.act` (y4_workspace_map): a list of dicts sorted by offset, see `ext.workspace_map`."""
        return ext.workspace_map(self.lib, self.handle)

    def conv_output_view(self, conv_idx):
        """(row index in `workspace_map`, channel offset, channel stride, materialised) of the view conv `conv_idx` stores its
        output in; materialised is False while a fused kernel keeps that tensor on chip (`conv_output` then shows stale bytes)"""
        return ext.conv_output_view(self.lib, self.handle, conv_idx)

    def layer_table(self):
        n = self.lib.y4_num_layers(self.handle)
        out = []
        for i in range(n):
            d = ext.y4_layer_desc()
            ext.check(self.lib.y4_layer_info(self.handle, i, C.byref(d)))
            out.append({k: getattr(d, k) for k, _ in ext.y4_layer_desc._fields_})
        return out

    # ---------------------------------------------------------------- compute
    def _to_device_images(self, imgs):
        """array-like [N,H,W,3] any float dtype (Keras casts to float32) -> contiguous cuda float32.  uint8 input -- a
        torch tensor OR a numpy array, the container must not change the meaning -- is "frames at network size before the
        /255" (what `preprocess_u8` returns, also after a `.cpu().numpy()` round trip): it stays uint8 and the stem
        divides inside its operand load.  Other integer dtypes are refused: their scale would be a guess."""
        torch = self.torch
        if isinstance(imgs, torch.Tensor) and imgs.dtype == torch.uint8:
            t = imgs.to(self.device)                        # network-size uint8 frames: the stem divides by 255
        elif isinstance(imgs, torch.Tensor):
            if not imgs.dtype.is_floating_point:
                raise ValueError(f"images must be floating point in [0,1] or uint8 frames, got {imgs.dtype}")
            t = imgs.to(self.device, dtype=torch.float32)
        else:
            a = np.asarray(imgs)
            if a.dtype == np.uint8:
                t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            elif a.dtype.kind != "f":
                raise ValueError(f"images must be floating point in [0,1] or uint8 frames, got {a.dtype}")
            else:
                if a.dtype != np.float32:
                    a = a.astype(np.float32)
                t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        H, W = self.img_hw
        if t.dim() != 4 or t.shape[1] != H or t.shape[2] != W or t.shape[3] != 3:
            raise ValueError(f"expected images of shape [N,{H},{W},3], got {tuple(t.shape)}")
        return t.contiguous()

    def preprocess_u8(self, raw_imgs, as_float=False):
        """Device-side `Yolov4.preprocess_img` (reference models.py:95-98) for one uint8 RGB image [h,w,3] or a list of
        them (any sizes).  Returns the tensor `forward_device` / `predict` take: by default a uint8 cuda tensor [n,H,W,3]
        (the resize done with cv2's uint8 arithmetic; the `/ 255.` then happens inside the stem's operand load), with
        as_float=True the float32 tensor in [0,1] (`y4_preprocess_u8`).  Both give bit-identical network outputs."""
        torch = self.torch
        if isinstance(raw_imgs, np.ndarray) and raw_imgs.ndim == 3:
            raw_imgs = [raw_imgs]
        H, W = self.img_hw
        out = torch.empty((len(raw_imgs), H, W, 3), dtype=torch.float32 if as_float else torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            for i, im in enumerate(raw_imgs):
                a = np.ascontiguousarray(im)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError(f"expected uint8 [h,w,3] images, got {a.dtype} {a.shape}")
                d = torch.from_numpy(a.copy() if not a.flags.writeable else a).to(self.device)
                if as_float:
                    ext.check(self.lib.y4_preprocess_u8(ext.ptr(d), a.shape[0], a.shape[1], ext.ptr(out[i]), H, W, ext.stream_ptr()))
                else:
                    ext.check(self.lib.y4_resize_u8(ext.ptr(d), 1, a.shape[0], a.shape[1], ext.ptr(out[i]), H, W, ext.stream_ptr()))
            torch.cuda.current_stream().synchronize()       # the uint8 staging tensors may be freed now
        return out

    def preprocess_u8_batch(self, raw_imgs, letterbox=False, pad_value=128):
        """Device-side preprocessing of uint8 RGB images [h,w,3] of ANY mix of sizes in one upload and one launch: the images
        and their descriptor table are packed into one pinned staging buffer (kept across calls), cross PCIe in one copy, and
        `y4_resize_u8_ragged` writes the uint8 network batch.  letterbox=False: the stretch of `Yolov4.preprocess_img`
        (reference models.py:95-98), the same bytes as `preprocess_u8`; letterbox=True: each image resized with its aspect
        kept and centred on a `pad_value` canvas (prepost.letterbox_rect / prepost.letterbox, bit for bit).
        -> (uint8 cuda tensor [n,H,W,3], float32 cuda tensor [n,4] box map for `predict(..., box_map=)`: the identity rows
        for stretch, prepost.box_map for letterbox).  Asynchronous on the current stream."""
        raw_imgs, pad_value = self._check_ragged(raw_imgs, pad_value, "preprocess_u8_batch")
        return self._fit_batch(self.lib.y4_resize_u8_ragged, ext.y4_image_desc, raw_imgs, [a.shape[:2] for a in raw_imgs],
                               letterbox, pad_value)

    def preprocess_yuv_batch(self, frames, letterbox=False, pad_value=128, matrix='bt601', full_range=False, fmt='nv12'):
        """`preprocess_u8_batch` for 8-bit 4:2:0 video frames: `frames` is one `yuv.YuvFrame` or a list of them, of ANY mix of
        sizes, formats (nv12, nv21, i420, yv12) and pitches; a 2-D uint8 array [h + h // 2, w] with even h, w (the rawvideo
        layout) is a frame of format `fmt`.  The frames and their y4_yuv_desc table are packed into the one pinned staging buffer,
        cross PCIe in one copy at 1.5 bytes per pixel, and one launch (`y4_yuv_u8_ragged`) converts and resizes: the batch is,
        byte for byte, `preprocess_u8_batch` of `yuv.to_rgb(frame, matrix, full_range)`.
        -> (uint8 cuda tensor [n,H,W,3], float32 cuda tensor [n,4] box map: prepost.box_map of each frame's h, w).
        Asynchronous on the current stream."""
        from . import yuv
        frames = yuv.as_frames(frames, fmt)
        word = yuv.flags(matrix, full_range)
        return self._fit_batch(self.lib.y4_yuv_u8_ragged, ext.y4_yuv_desc, [f.data[:f.nbytes] for f in frames],
                               [(f.h, f.w) for f in frames], letterbox, self._check_pad(pad_value),
                               place=lambda d, k, off: frames[k].fill_desc(d, off, word))

    def _fit_batch(self, fn, Desc, sources, sizes, letterbox, pad_value, place=None):
        """What `preprocess_u8_batch` and `preprocess_yuv_batch` share: the `Desc` table and box maps of sources of `sizes` (h, w)
        fitted to the canvas, the one upload, the one launch of `fn` -> (uint8 cuda batch [n,H,W,3], float32 cuda box map [n,4])."""
        n = len(sources)
        desc, maps = canvas.fit_table(Desc, sizes, *self.img_hw, letterbox)
        dev, desc_bytes, head = self._upload_ragged(sources, desc, maps, place=place)
        out = self._canvas_launch(fn, C.c_void_p(dev.data_ptr() + head), (ext.ptr(dev),), n, None, pad_value)
        return out, dev[desc_bytes:head].view(self.torch.float32).view(n, 4)

    def augment_u8_batch(self, raw_imgs, params, pad_value=128):
        """The training input of `Yolov4.fit` on the device: uint8 RGB images [h,w,3] of any mix of sizes and one parameter row
        per image (yolo4hip.augment.PARAM_DTYPE: `draw_params`) -> the augmented uint8 cuda batch [n,H,W,3] for
        `forward_device`, through one pinned staging buffer, one copy and one launch (`y4_augment_u8_ragged`): resize into a
        rectangle that may stick out of the canvas, left-right flip and the HSV transform; `augment.augment_host` is the same
        function on the host.  Asynchronous on the current stream."""
        raw_imgs, pad_value = self._check_ragged(raw_imgs, pad_value, "augment_u8_batch")
        n = len(raw_imgs)
        if len(params) != n:
            raise ValueError(f"augment_u8_batch: {n} images, {len(params)} parameter rows")
        dev, _, head = self._upload_ragged(raw_imgs, self._augment_desc(params, "augment_u8_batch"))
        return self._canvas_launch(self.lib.y4_augment_u8_ragged, C.c_void_p(dev.data_ptr() + head), (ext.ptr(dev),), n, None,
                                   pad_value)

    def mosaic_u8_batch(self, images, tile_src, params, cuts, pad_value=128):
        """Mosaic canvases on the device (`DataGenerator.raw_mosaic`): `images` the DISTINCT uint8 RGB photos [h,w,3] of the
        batch, tile_src int [n,4] the image of every tile, params (yolo4hip.augment.PARAM_DTYPE) [n,4] its row, cuts int
        [n,2] the (cut_y, cut_x) of every canvas -> the uint8 cuda batch [n,H,W,3].  Every image is packed and uploaded once,
        however many tiles use it: the 4 n descriptors carry shared offsets, and they, the cuts and the images cross in the
        one staging buffer and the one copy of `augment_u8_batch`; one launch (`y4_mosaic_u8_ragged`) follows.
        `augment.mosaic_host` is the same function on the host.  What the kernel does not check is checked here (ValueError):
        0 <= cut <= (H, W), tile_src inside `images`, out_h, out_w >= 1, finite factors.  Asynchronous on the current stream."""
        images, pad_value = self._check_ragged(images, pad_value, "mosaic_u8_batch")
        H, W = self.img_hw
        tile_src, cuts = np.asarray(tile_src), np.ascontiguousarray(cuts, dtype=np.int32)
        n = len(cuts)
        if n < 1 or tile_src.shape != (n, 4) or np.shape(params) != (n, 4) or cuts.shape != (n, 2):
            raise ValueError(f"mosaic_u8_batch: tile_src {tile_src.shape}, params {np.shape(params)}, cuts {cuts.shape}: "
                             f"[n,4], [n,4], [n,2]")
        if tile_src.dtype.kind not in "iu" or tile_src.min() < 0 or tile_src.max() >= len(images):
            raise ValueError(f"mosaic_u8_batch: tile_src must index the {len(images)} images")
        if (cuts < 0).any() or (cuts[:, 0] > H).any() or (cuts[:, 1] > W).any():
            raise ValueError(f"mosaic_u8_batch: cuts (cut_y, cut_x) must lie in [0, {H}] x [0, {W}]")
        desc = self._augment_desc(np.asarray(params).reshape(-1), "mosaic_u8_batch")
        dev, desc_bytes, head = self._upload_ragged(images, desc, cuts, rows=tile_src.reshape(-1))
        return self._canvas_launch(self.lib.y4_mosaic_u8_ragged, C.c_void_p(dev.data_ptr() + head),
                                   (ext.ptr(dev), C.c_void_p(dev.data_ptr() + desc_bytes)), n, None, pad_value)

    @staticmethod
    def _augment_desc(params, who):
        """yolo4hip.augment.PARAM_DTYPE rows -> a ctypes array of y4_augment_desc with the rectangle, flip and HSV factors filled
        in (offset, h, w are `_upload_ragged`'s), or ValueError for what the kernel does not check."""
        desc = (ext.y4_augment_desc * len(params))()
        for d, p in zip(desc, params):
            d.out_h, d.out_w, d.pad_top, d.pad_left = int(p["out_h"]), int(p["out_w"]), int(p["pad_top"]), int(p["pad_left"])
            d.flip, d.hue, d.sat, d.val = int(p["flip"]), float(p["hue"]), float(p["sat"]), float(p["val"])
            if d.out_h < 1 or d.out_w < 1 or not np.isfinite([d.hue, d.sat, d.val]).all():
                raise ValueError(f"{who}: rectangle {d.out_h} x {d.out_w}, factors {d.hue}, {d.sat}, {d.val}")
        return desc

    def _canvas_launch(self, fn, src, tables, n, out, pad_value):
        """One launch of a canvas entry point (y4_resize / window / augment / mosaic _u8_ragged) on the current stream: `src` the
        first image byte, `tables` the descriptor table(s) as pointers, `out` a uint8 cuda tensor of at least [n,H,W,3] (None: a
        fresh one) -> out[:n]."""
        H, W = self.img_hw
        with self.torch.cuda.device(self.device):
            if out is None:
                out = self.torch.empty((n, H, W, 3), dtype=self.torch.uint8, device=self.device)
            ext.check(fn(src, *tables, int(n), ext.ptr(out), H, W, int(pad_value), ext.stream_ptr()))
        return out[:n]

    @staticmethod
    def _check_pad(pad_value):
        if not 0 <= int(pad_value) <= 255:
            raise ValueError(f"pad_value must be a uint8 level 0..255, got {int(pad_value)}")
        return int(pad_value)

    @staticmethod
    def _check_ragged(raw_imgs, pad_value, who):
        """One image or a list of them -> (list of uint8 [h,w,3] arrays, pad_value as an int), or ValueError."""
        if isinstance(raw_imgs, np.ndarray) and raw_imgs.ndim == 3:
            raw_imgs = [raw_imgs]
        raw_imgs = list(raw_imgs)
        if len(raw_imgs) == 0:
            raise ValueError(f"{who}: no images")
        pad_value = Engine._check_pad(pad_value)
        for a in raw_imgs:
            if getattr(a, "dtype", None) != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"expected uint8 [h,w,3] images, got {getattr(a, 'dtype', type(a))} {getattr(a, 'shape', '')}")
        return raw_imgs, pad_value

    def _upload_ragged(self, raw_imgs, desc, extra=None, rows=None, windows=None, place=None):
        """The one upload of a ragged batch (`preprocess_u8_batch`, `augment_u8_batch`, `mosaic_u8_batch`, `predict_tiled`): the
        source fields of every row of `desc` are filled by `canvas.place_sources` (which explains `rows`, `windows` and `place`), then
        descriptors | `extra` (a numpy array, or None) | the images are packed into the pinned staging buffer (kept across calls)
        and copied to a fresh device block in one copy.
        -> (device block, descriptor bytes, bytes before the first image); descriptor offsets count from the first image byte."""
        torch = self.torch
        n = len(raw_imgs)
        desc_bytes = C.sizeof(desc)
        head = desc_bytes + (extra.nbytes if extra is not None else 0)
        offs = canvas.place_sources(desc, [a.shape for a in raw_imgs], rows, windows, place)
        off, total = offs[-1], head + offs[-1]
        pin = getattr(self, "_batch_pin", None)
        if pin is not None:
            self._batch_pin_free.synchronize()              # the previous call's upload has left the buffer
        if pin is None or pin.numel() < total:
            pin = self._batch_pin = torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
            self._batch_pin_np = pin.numpy()
            self._batch_pin_free = torch.cuda.Event()
        buf = self._batch_pin_np
        buf[:desc_bytes] = np.frombuffer(desc, dtype=np.uint8)
        if extra is not None:
            buf[desc_bytes:head] = extra.view(np.uint8).reshape(-1)

        def pack(i):
            a, o = raw_imgs[i], head + offs[i]
            np.copyto(buf[o:o + a.size].reshape(a.shape), a)   # (any strides: BGR views included; releases the GIL)

        if off >= (8 << 20) and n > 1:
            # tens of MB of photos: one thread's memcpy into the staging buffer would cost more than the upload itself
            # (measured), so the images are packed by a few worker threads (they block when idle, they do not spin)
            if getattr(self, "_pack_pool", None) is None:
                from concurrent.futures import ThreadPoolExecutor
                self._pack_pool = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
            list(self._pack_pool.map(pack, range(n)))
        else:
            for i in range(n):
                pack(i)
        with torch.cuda.device(self.device):
            # a fresh device block per call (torch's caching allocator): views of it (the box map) stay valid
            dev = torch.empty(total, dtype=torch.uint8, device=self.device)
            dev.copy_(pin[:total], non_blocking=True)
            self._batch_pin_free.record()
        return dev, desc_bytes, head

    def resize_u8_ragged(self, src_dev, desc_dev, n, out, pad_value=128):
        """y4_resize_u8_ragged on device buffers: `desc_dev` holds n y4_image_desc rows (offsets into `src_dev`), `out` is a
        uint8 cuda tensor of at least [n,H,W,3].  Asynchronous on the current stream; returns out[:n]."""
        return self._canvas_launch(self.lib.y4_resize_u8_ragged, ext.ptr(src_dev), (ext.ptr(desc_dev),), n, out, pad_value)

    def yuv_u8_ragged(self, src_dev, desc_dev, n, out, pad_value=128):
        """y4_yuv_u8_ragged on device buffers: `desc_dev` holds n y4_yuv_desc rows (planes of 4:2:0 frames in `src_dev`, a
        decoder's surfaces for instance), `out` is a uint8 cuda tensor of at least [n,H,W,3].  Asynchronous on the current
        stream; returns out[:n]."""
        return self._canvas_launch(self.lib.y4_yuv_u8_ragged, ext.ptr(src_dev), (ext.ptr(desc_dev),), n, out, pad_value)

    def window_u8_ragged(self, src_dev, desc_dev, n, out, pad_value=128):
        """y4_window_u8_ragged on device buffers: `desc_dev` holds n y4_window_desc rows (windows of images in `src_dev`), `out`
        is a uint8 cuda tensor of at least [n,H,W,3].  Asynchronous on the current stream; returns out[:n]."""
        return self._canvas_launch(self.lib.y4_window_u8_ragged, ext.ptr(src_dev), (ext.ptr(desc_dev),), n, out, pad_value)

    def view_u8_ragged(self, src_dev, desc_dev, n, out, pad_value=128):
        """y4_view_u8_ragged on device buffers: `desc_dev` holds n y4_view_desc rows (windows of images in `src_dev`, each with
        its flip bits: the canvas mirrored left-right / up-down), `out` is a uint8 cuda tensor of at least [n,H,W,3].
        Asynchronous on the current stream; returns out[:n]."""
        return self._canvas_launch(self.lib.y4_view_u8_ragged, ext.ptr(src_dev), (ext.ptr(desc_dev),), n, out, pad_value)

    # ---------------------------------------------------------------- tiled inference: one NMS over the rows of a group
    def gather_begin(self, n_groups, max_slots, group_cap):
        """Scratch for a gathered decode + NMS sequence (y4_gather_scratch_bytes, y4_gather_begin): -> the state `decode_gather`
        and `nms_gathered` take.  n_groups photos of at most max_slots rows each, group_cap candidate keys per photo."""
        torch = self.torch
        geo = (int(n_groups), int(max_slots), int(group_cap))
        if geo[2] < 1 or geo[2] >= 1 << 32:
            raise ValueError(f"group_cap must be in [1, 2^32), got {group_cap}")
        nbytes = C.c_size_t()
        ext.check(self.lib.y4_gather_scratch_bytes(self.handle, *geo, C.byref(nbytes)))
        with torch.cuda.device(self.device):
            scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            ext.check(self.lib.y4_gather_begin(self.handle, *geo, ext.ptr(scratch), ext.stream_ptr()))
        return geo, scratch

    def decode_gather(self, state, n, row_group, row_slot, row_map, score_threshold=-1.0, oriented=False):
        """y4_decode_gather: the decode stage on rows 0 .. n-1 of the workspace, their candidates merged into the groups of
        `state`.  row_group / row_slot: int32 cuda tensors [n], row_map float32 cuda [n,4] (contiguous).  oriented=True is
        y4_decode_gather_views: a map with a negative scale (a mirrored view) swaps the corners it reads, so that stored boxes
        keep x1 <= x2 and y1 <= y2.  Asynchronous."""
        torch = self.torch
        geo, scratch = state
        for t, dt, shape in ((row_group, torch.int32, (n,)), (row_slot, torch.int32, (n,)), (row_map, torch.float32, (n, 4))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"decode_gather: expected a contiguous {dt} cuda tensor {shape}, got {t.dtype} {tuple(t.shape)}")
        fn = self.lib.y4_decode_gather_views if oriented else self.lib.y4_decode_gather
        with torch.cuda.device(self.device):
            ext.check(fn(self.handle, int(n), float(score_threshold), ext.ptr(row_group), ext.ptr(row_slot),
                         ext.ptr(row_map), *geo, ext.ptr(scratch), ext.stream_ptr()))

    def alloc_tiled_outputs_flat(self, n_groups):
        """`alloc_outputs_flat(n_groups)` with the groups' candidate counts behind it, ONE int32 device block for one copy back:
        -> (flat, (boxes, scores, classes, valid, kept) views, cand_count int32 view [n_groups]); the first part of `flat` has
        the layout of `alloc_outputs_flat`."""
        flat, v = self._alloc_block(self._tiled_fields(n_groups))
        return flat, tuple(v[:5]), v[5]

    def _tiled_fields(self, n_groups):
        n = int(n_groups)
        return _detection_fields(n, self.T) + [("int32", (n,))]

    def tiled_outputs_to_host(self, flat, n_groups):
        """The one copy of `alloc_tiled_outputs_flat`'s block -> ([boxes, scores, classes, valid, kept], cand_count) as fresh
        writable numpy arrays."""
        p = [a.copy() for a in _block_views(flat.cpu().numpy(), self._tiled_fields(n_groups))]
        return p[:5], p[5]

    def nms_gathered(self, state, outs=None, cand_count=None, iou_threshold=-1.0):
        """y4_nms_gathered over the groups of `state`: -> (outs as `decode_nms_device` for n_groups images, boxes normalised to
        each group; cand_count int32 cuda [n_groups]: the candidates each group received -- above group_cap: that group's
        result is not defined).  Asynchronous."""
        torch = self.torch
        geo, scratch = state
        outs = outs or self.alloc_outputs(geo[0])
        if cand_count is None:
            cand_count = torch.empty((geo[0],), dtype=torch.int32, device=self.device)
        b, s, c, v, k = outs
        if self.nms_merge and k is None:                   # (the merge reads the kept indices)
            k = torch.empty((geo[0], self.T), dtype=torch.int32, device=self.device)
        fn = self.lib.y4_nms_gathered_merged if self.nms_merge else self.lib.y4_nms_gathered
        with torch.cuda.device(self.device):
            ext.check(fn(self.handle, *geo, float(iou_threshold), ext.ptr(scratch), ext.ptr(cand_count),
                         ext.ptr(b), ext.ptr(s), ext.ptr(c), ext.ptr(v), ext.ptr(k), ext.stream_ptr()))
        return outs, cand_count

    def _rows_device(self, who, raw_imgs, rows_of, views, pad_value, iou_threshold, score_threshold, tile_candidates,
                     outputs=None):
        """The loop of `predict_tiled_device` and `predict_tta_device`: rows_of(h, w) -> the base rows (window, rect, map) of a
        photo.  views=None: the rows as they are, through y4_window_u8_ragged and y4_decode_gather; a view list: every row under
        every view (tiling.view_rows, slot = its index there), through y4_view_u8_ragged and y4_decode_gather_views.
        outputs: None, or the (flat, outs, cand_count) of a block the caller allocated for len(raw_imgs) photos
        (`alloc_coco_outputs_flat`) in place of `alloc_tiled_outputs_flat`'s."""
        torch = self.torch
        raw_imgs, pad_value = self._check_ragged(raw_imgs, pad_value, who)
        if int(tile_candidates) < 1:
            raise ValueError(f"tile_candidates must be >= 1, got {tile_candidates}")
        if views is not None:
            tiling.check_views(views)                      # ValueError before anything is uploaded
            views = list(views)
        H, W = self.img_hw
        photo, slot, windows, rects, maps, flips = [], [], [], [], [], []
        for p, a in enumerate(raw_imgs):
            rows = rows_of(a.shape[0], a.shape[1])
            if views is None:
                rows = [(win, rect, 0, m) for win, rect, m in rows]
            else:
                rows = tiling.view_rows(rows, views, a.shape[:2], (H, W))
            for t, (win, rect, bits, m) in enumerate(rows):
                photo.append(p); slot.append(t); windows.append(win); rects.append(rect); maps.append(m); flips.append(bits)
        R, P, max_slots = len(photo), len(raw_imgs), max(slot) + 1
        Desc, launch = ((ext.y4_window_desc, self.lib.y4_window_u8_ragged) if views is None
                        else (ext.y4_view_desc, self.lib.y4_view_u8_ragged))
        desc = canvas.rect_table(Desc, rects)
        if views is not None:
            for d, bits in zip(desc, flips):
                d.flip = bits
        # maps | groups | slots travel behind the descriptors in the one upload
        extra = np.concatenate([np.asarray(maps, np.float32).reshape(-1).view(np.int32), np.asarray(photo, np.int32),
                                np.asarray(slot, np.int32)])
        dev, desc_bytes, head = self._upload_ragged(raw_imgs, desc, extra, rows=photo, windows=windows)
        tab = dev[desc_bytes:head].view(torch.int32)
        row_map, row_group, row_slot = tab[:4 * R].view(torch.float32).view(R, 4), tab[4 * R:5 * R], tab[5 * R:6 * R]
        # a photo cannot yield more candidates than its rows have (box, class) pairs: no larger list is ever needed
        group_cap = int(min(int(tile_candidates), max_slots * self.num_boxes * self.num_classes))
        state = self.gather_begin(P, max_slots, group_cap)
        flat, outs, cand_count = self.alloc_tiled_outputs_flat(P) if outputs is None else outputs
        step = C.sizeof(Desc)
        with torch.cuda.device(self.device):
            batch = torch.empty((min(R, self.max_batch), H, W, 3), dtype=torch.uint8, device=self.device)
            src = C.c_void_p(dev.data_ptr() + head)
            for r0 in range(0, R, self.max_batch):
                n = min(self.max_batch, R - r0)
                self.forward_device(self._canvas_launch(launch, src, (C.c_void_p(dev.data_ptr() + r0 * step),), n, batch, pad_value))
                self.decode_gather(state, n, row_group[r0:r0 + n], row_slot[r0:r0 + n], row_map[r0:r0 + n], score_threshold,
                                   oriented=views is not None)
            self.nms_gathered(state, outs, cand_count, iou_threshold)
        return flat, outs, cand_count, group_cap

    def _rows_to_host(self, who, device_result, n, with_indices):
        """The one copy back of `_rows_device`'s result and the capacity check."""
        flat, _, _, group_cap = device_result
        res, cand = self.tiled_outputs_to_host(flat, n)
        if (cand > group_cap).any():
            g = int(np.argmax(cand))
            raise RuntimeError(f"{who}: photo {g} has {int(cand[g])} candidates, more than tile_candidates = {group_cap} "
                               f"holds; raise tile_candidates")
        return res if with_indices else res[:4]

    def predict_tiled_device(self, raw_imgs, tile=None, overlap=0.2, full_image=True, letterbox=False, pad_value=128,
                             iou_threshold=-1.0, score_threshold=-1.0, tile_candidates=1 << 18, views=None, outputs=None):
        """`predict_tiled` with the results left on the device: -> (flat, outs, cand_count, group_cap) in the form of
        `alloc_tiled_outputs_flat(len(raw_imgs))` -- outs are what `decode_nms_device` returns for that many images, boxes
        normalised to each photo, ready for `map_match_device`.  The caller checks cand_count <= group_cap.  Asynchronous."""
        H, W = self.img_hw
        tile_hw = None if tile is None else ((int(tile), int(tile)) if np.ndim(tile) == 0 else (int(tile[0]), int(tile[1])))
        return self._rows_device("predict_tiled", raw_imgs,
                                 lambda h, w: tiling.tile_rows(h, w, (H, W), tile_hw, overlap, full_image, letterbox),
                                 views, pad_value, iou_threshold, score_threshold, tile_candidates, outputs)

    def predict_tiled(self, raw_imgs, tile=None, overlap=0.2, full_image=True, letterbox=False, pad_value=128,
                      iou_threshold=-1.0, score_threshold=-1.0, tile_candidates=1 << 18, with_indices=False, views=None):
        """Tiled (sliced) inference of uint8 RGB photos [h,w,3] of any sizes: each photo is cut into overlapping windows of `tile`
        (an int or (th, tw); None: the network input, so interior windows are 1:1 copies) at native resolution
        (yolo4hip.tiling.tile_rows; full_image=True adds the whole photo as one more row), the windows run through the network
        as batch rows, and ONE NMS per photo runs over all of its rows' candidates in the photo's coordinates -- an object two
        windows see comes back once.  One upload (photos, descriptors, maps), per chunk of max_batch rows y4_window_u8_ragged ->
        y4_forward_u8 -> y4_decode_gather, then y4_nms_gathered and one copy back.  letterbox / pad_value: how a window (and the
        full image) that is not of the network's size is placed on the canvas.  tile_candidates: the candidate keys a photo may
        have (8 bytes each); RuntimeError when a photo has more.
        views: None, or a list of (scale, flip) views (yolo4hip.tiling.view_rows): every row then runs under every view -- rows x
        views slots per photo, through y4_view_u8_ragged and y4_decode_gather_views -- still under the one NMS.
        -> [boxes [P,max_total,4] normalised to each photo, scores, classes, valid], with_indices also kept = slot * num_boxes +
        box, as fresh host arrays, like `predict`."""
        raws = [raw_imgs] if isinstance(raw_imgs, np.ndarray) and raw_imgs.ndim == 3 else list(raw_imgs)
        res = self.predict_tiled_device(raws, tile, overlap, full_image, letterbox, pad_value, iou_threshold, score_threshold,
                                        tile_candidates, views)
        return self._rows_to_host("predict_tiled", res, len(raws), with_indices)

    def predict_tta_device(self, raw_imgs, views=tiling.DEFAULT_VIEWS, letterbox=False, pad_value=128, iou_threshold=-1.0, score_threshold=-1.0,
                           tile_candidates=1 << 18, outputs=None):
        """`predict_tta` with the results left on the device, in the form of `predict_tiled_device`: -> (flat, outs, cand_count,
        group_cap), boxes normalised to each photo, ready for `map_match_device`."""
        H, W = self.img_hw
        return self._rows_device("predict_tta", raw_imgs,
                                 lambda h, w: tiling.tile_rows(h, w, (H, W), None, 0.0, True, letterbox)[-1:],
                                 views, pad_value, iou_threshold, score_threshold, tile_candidates, outputs)

    def predict_tta(self, raw_imgs, views=tiling.DEFAULT_VIEWS, letterbox=False, pad_value=128, iou_threshold=-1.0, score_threshold=-1.0,
                    tile_candidates=1 << 18, with_indices=False):
        """Test-time augmentation of uint8 RGB photos [h,w,3] of any sizes: each photo's full-image row (stretch, or letterbox)
        runs under every view (scale, flip) of `views` (default: YOLOv5's three) as one batch row each --
        the rectangle shrunk about its centre, the canvas mirrored --, and ONE NMS per photo runs over the candidates of all its
        views in the photo's coordinates (merged into score-weighted boxes when `nms_merge` is on).  The loop of
        `predict_tiled`: one upload, per chunk of max_batch rows y4_view_u8_ragged -> y4_forward_u8 -> y4_decode_gather_views,
        then y4_nms_gathered, one copy back.  RuntimeError when a photo has more than tile_candidates candidates.
        -> what `predict_tiled` returns; kept = slot * num_boxes + box with slot the view's index."""
        raws = [raw_imgs] if isinstance(raw_imgs, np.ndarray) and raw_imgs.ndim == 3 else list(raw_imgs)
        res = self.predict_tta_device(raws, views, letterbox, pad_value, iou_threshold, score_threshold, tile_candidates)
        return self._rows_to_host("predict_tta", res, len(raws), with_indices)

    def resize_u8(self, frames_dev, out=None):
        """Device-side stretch resize (cv2.resize to width W, height H) on a uint8 cuda batch [n,h,w,3] -> uint8 [n,H,W,3]
        (cv2's uint8 INTER_LINEAR arithmetic); frames already at network size are returned as they are."""
        torch = self.torch
        n, h, w, _ = frames_dev.shape
        H, W = self.img_hw
        if h == H and w == W:
            return frames_dev
        if out is None:
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_resize_u8(ext.ptr(frames_dev), n, h, w, ext.ptr(out), H, W, ext.stream_ptr()))
        return out[:n]

    def _check_device_images(self, imgs_dev):
        torch = self.torch
        H, W = self.img_hw
        if imgs_dev.dtype not in (torch.float32, torch.uint8) or imgs_dev.dim() != 4 or tuple(imgs_dev.shape[1:]) != (H, W, 3) \
                or not imgs_dev.is_contiguous():
            raise ValueError(f"expected a contiguous float32 or uint8 cuda tensor [n,{H},{W},3], got {imgs_dev.dtype} {tuple(imgs_dev.shape)}")
        return imgs_dev.dtype == torch.uint8

    def forward_device(self, imgs_dev):
        """imgs_dev: float32 [n,S,S,3] in [0,1] (what preprocess_img gives), or uint8 [n,S,S,3] frames at network size
        BEFORE the /255 -- the stem then divides inside its operand load (bit-identical, no float image tensor)."""
        n = imgs_dev.shape[0]
        u8 = self._check_device_images(imgs_dev)
        with self.torch.cuda.device(self.device):
            fn = self.lib.y4_forward_u8 if u8 else self.lib.y4_forward
            ext.check(fn(self.handle, ext.ptr(imgs_dev), n, ext.stream_ptr()))

    def forward_until_device(self, imgs_dev, last_conv=71):
        """The forward pass cut behind conv `last_conv` (default 71: CSPDarknet53 proper, reference custom_layers.py:100-124) on a
        float32 device batch -- what `bench.py` times as `backbone`.  Asynchronous on the current stream."""
        n = imgs_dev.shape[0]
        if self._check_device_images(imgs_dev):
            raise ValueError("forward_until_device takes float32 images")
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_forward_until(self.handle, ext.ptr(imgs_dev), n, int(last_conv), ext.stream_ptr()))

    # ---------------------------------------------------------------- cached frozen features
    def feature_row_bytes(self):
        """y4_feature_row_bytes -> (bytes of one cache row, the three scales' byte offsets in it): what one image contributes at
        this engine's retention level -- level 1 the head convs' inputs, level 2 the inputs of convs 92 / 100 / 108 -- dense, in
        the engine's dtype.  An engine that retains nothing raises Y4Error (Y4_ESTATE)."""
        row, offs = C.c_size_t(), (C.c_size_t * 3)()
        ext.check(self.lib.y4_feature_row_bytes(self.handle, C.byref(row), offs))
        return row.value, tuple(int(o) for o in offs)

    def alloc_feature_cache(self, rows):
        """A cache of `rows` rows: a uint8 cuda tensor [rows, row_bytes] that owns the memory (not initialised)."""
        rows = int(rows)
        if rows < 1:
            raise ValueError(f"alloc_feature_cache: {rows} rows")
        return self.torch.empty((rows, self.feature_row_bytes()[0]), dtype=self.torch.uint8, device=self.device)

    def _feature_copy(self, fn, who, cache, slots):
        torch = self.torch
        row = self.feature_row_bytes()[0]
        if not isinstance(cache, torch.Tensor) or cache.dtype != torch.uint8 or cache.dim() != 2 or cache.shape[1] != row \
                or not cache.is_contiguous() or cache.device != self.device:
            raise ValueError(f"{who}: the cache must be a contiguous uint8 tensor [rows, {row}] on {self.device} (alloc_feature_cache)")
        slots = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)      # host memory: read before the call returns
        with torch.cuda.device(self.device):
            ext.check(fn(self.handle, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int64)), ext.ptr(cache), cache.shape[0],
                         ext.stream_ptr()))

    def store_features(self, cache, slots):
        """After `forward_device` of len(slots) images: image i's retained tensors -> row slots[i] of `cache` (y4_feature_store, one
        launch, asynchronous on the current stream).  A slot outside the cache or named twice raises Y4Error before any launch."""
        self._feature_copy(self.lib.y4_feature_store, "store_features", cache, slots)

    def load_features(self, cache, slots):
        """Row slots[i] of `cache` -> batch position i of the retained tensors in the workspace (y4_feature_load); follow it with
        `forward_tail_device(len(slots))`."""
        self._feature_copy(self.lib.y4_feature_load, "load_features", cache, slots)

    def forward_tail_device(self, n):
        """y4_forward_tail: only the convs behind the cached tensors, on what the workspace holds for n images.  Afterwards the
        raw heads are those `forward_device` of the same images leaves, bit for bit, and `loss_device`, the gradient calls,
        `heads_device` and `decode_nms_device` work as after it."""
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_forward_tail(self.handle, int(n), ext.stream_ptr()))

    def heads_device(self, n):
        torch = self.torch
        outs = [torch.empty((n, gh, gw, self.nout), dtype=torch.float32, device=self.device) for gh, gw in self.grids_hw]
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_get_heads(self.handle, n, ext.ptr(outs[0]), ext.ptr(outs[1]), ext.ptr(outs[2]),
                                            ext.stream_ptr()))
        return outs

    def set_heads(self, heads):
        """Load dense float32 raw heads (3 arrays [n,gh,gw,3(C+5)]) into the workspace (decode/NMS tests)."""
        torch = self.torch
        ts = [torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(self.device) for h in heads]
        n = ts[0].shape[0]
        for t, (gh, gw) in zip(ts, self.grids_hw):
            if tuple(t.shape) != (n, gh, gw, self.nout):
                raise ValueError(f"head shape {tuple(t.shape)} != {(n, gh, gw, self.nout)}")
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_set_heads(self.handle, n, ext.ptr(ts[0]), ext.ptr(ts[1]), ext.ptr(ts[2]),
                                            ext.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        return n

    def alloc_outputs(self, n):
        torch = self.torch
        T = self.T
        return (torch.empty((n, T, 4), dtype=torch.float32, device=self.device),
                torch.empty((n, T), dtype=torch.float32, device=self.device),
                torch.empty((n, T), dtype=torch.float32, device=self.device),
                torch.empty((n,), dtype=torch.int32, device=self.device),
                torch.empty((n, T), dtype=torch.int32, device=self.device))

    def alloc_outputs_flat(self, n):
        """The five outputs of `alloc_outputs` as views of ONE int32 device block, so that a step's results return to
        the host in a single copy: -> (flat int32 tensor, (boxes, scores, classes, valid, kept) views)."""
        flat, v = self._alloc_block(_detection_fields(n, self.T))
        return flat, tuple(v)

    def _alloc_block(self, fields):
        """-> (a new int32 device block for `fields`, its views)."""
        flat = self.torch.empty(_block_len(fields), dtype=self.torch.int32, device=self.device)
        return flat, _block_views(flat, fields)

    def decode_nms_device(self, n, outs=None, iou_threshold=-1.0, score_threshold=-1.0, box_map=None):
        """Decode + NMS of the heads in the workspace.  box_map: a contiguous float32 cuda tensor [n,4] of (ax, bx, ay, by) rows
        (`preprocess_u8_batch`, prepost.box_map) -- the kept boxes are then mapped to each source image before the clip
        (y4_decode_nms_mapped); everything but the boxes is unchanged.  With `nms_merge` on both go through y4_decode_nms_merged."""
        outs = outs or self.alloc_outputs(n)
        b, s, c, v, k = outs
        if box_map is not None and (tuple(box_map.shape) != (n, 4) or box_map.dtype != self.torch.float32 or not box_map.is_contiguous()):
            raise ValueError(f"box_map must be a contiguous float32 tensor [{n},4], got {box_map.dtype} {tuple(box_map.shape)}")
        with self.torch.cuda.device(self.device):
            if self.nms_merge:
                if k is None:                              # (the merge reads the kept indices)
                    k = self.torch.empty((n, self.T), dtype=self.torch.int32, device=self.device)
                ext.check(self.lib.y4_decode_nms_merged(self.handle, n, float(iou_threshold), float(score_threshold),
                                                        ext.ptr(box_map), ext.ptr(self._merge_counts(n)), ext.ptr(b), ext.ptr(s),
                                                        ext.ptr(c), ext.ptr(v), ext.ptr(k), ext.stream_ptr()))
            elif box_map is None:
                ext.check(self.lib.y4_decode_nms(self.handle, n, float(iou_threshold), float(score_threshold), ext.ptr(b),
                                                 ext.ptr(s), ext.ptr(c), ext.ptr(v), ext.ptr(k), ext.stream_ptr()))
            else:
                ext.check(self.lib.y4_decode_nms_mapped(self.handle, n, float(iou_threshold), float(score_threshold),
                                                        ext.ptr(box_map), ext.ptr(b), ext.ptr(s), ext.ptr(c), ext.ptr(v),
                                                        ext.ptr(k), ext.stream_ptr()))
        return outs

    # ---------------------------------------------------------------- VOC mAP matching
    def alloc_map_outputs_flat(self, n):
        """What `Yolov4.evaluate_map` needs of a batch as views of ONE int32 device block -- scores, classes, valid and the
        tp mask of `map_match_device` -- so that they reach the host in a single copy (`map_outputs_to_host`); the boxes
        are a tensor of their own and stay on the device.  -> (flat int32 tensor, outs for `decode_nms_device` (boxes, scores,
        classes, valid, no kept indices), tp_mask int32 view [n, max_total])."""
        flat, (scores, classes, valid, tp_mask) = self._alloc_block(self._map_fields(n, "int32"))
        boxes = self.torch.empty((n, self.T, 4), dtype=self.torch.float32, device=self.device)
        return flat, (boxes, scores, classes, valid, None), tp_mask

    def _map_fields(self, n, mask_dtype):
        T = self.T
        return [("float32", (n, T)), ("float32", (n, T)), ("int32", (n,)), (mask_dtype, (n, T))]

    def map_outputs_to_host(self, flat, n):
        """The one copy of `alloc_map_outputs_flat`'s block -> (scores float32 [n,T], classes float32 [n,T], valid int32 [n],
        tp_mask uint32 [n,T]) as numpy views of it."""
        return tuple(_block_views(flat.cpu().numpy(), self._map_fields(n, "uint32")))

    def _check_match_inputs(self, n, scale_dev, gt_dev, gt_count_dev):
        """The ground-truth tensors of `map_match_device` and `coco_match_device` for n images -> max_gt, or ValueError."""
        torch = self.torch
        if gt_dev.dim() != 3 or gt_dev.shape[0] != n or gt_dev.shape[2] != 5 or gt_dev.dtype != torch.float32 \
                or not gt_dev.is_contiguous():
            raise ValueError(f"gt_dev must be a contiguous float32 tensor [{n},max_gt,5], got {gt_dev.dtype} {tuple(gt_dev.shape)}")
        if tuple(scale_dev.shape) != (n, 2) or scale_dev.dtype != torch.float32 or not scale_dev.is_contiguous():
            raise ValueError(f"scale_dev must be a contiguous float32 tensor [{n},2], got {scale_dev.dtype} {tuple(scale_dev.shape)}")
        if tuple(gt_count_dev.shape) != (n,) or gt_count_dev.dtype != torch.int32 or not gt_count_dev.is_contiguous():
            raise ValueError(f"gt_count_dev must be a contiguous int32 tensor [{n}], got {gt_count_dev.dtype} {tuple(gt_count_dev.shape)}")
        return gt_dev.shape[1]

    def map_match_device(self, outs, scale_dev, gt_dev, gt_count_dev, iou_thresholds, debug=False, tp_mask=None):
        """y4_map_match on the outputs of `decode_nms_device` (outs = boxes, scores, classes, valid, ...): the kept boxes of
        each image, scaled to raw-image pixels by scale_dev (float32 cuda [n,2]: w, h), are matched against gt_dev (float32
        cuda [n,max_gt,5]: x1, y1, x2, y2, class in raw-image pixels, annotation order; gt_count_dev int32 [n]) by the rule of
        `evalmap.eval_map`, once per IoU threshold (1..16 of them).  -> tp_mask, an int32 cuda tensor [n,max_total] whose bit t
        says "true positive at iou_thresholds[t]" (written into `tp_mask` when given); with debug=True
        (tp_mask, best_iou float64 [n,max_total], match int32 [n,max_total], gt_used int32 [n,max_gt]).  Asynchronous."""
        torch = self.torch
        boxes, scores, classes, valid = outs[:4]
        n, T = scores.shape
        thr = [float(t) for t in iou_thresholds]
        max_gt = self._check_match_inputs(n, scale_dev, gt_dev, gt_count_dev)
        if tp_mask is None:
            tp_mask = torch.empty((n, T), dtype=torch.int32, device=self.device)
        elif tuple(tp_mask.shape) != (n, T) or tp_mask.dtype != torch.int32 or not tp_mask.is_contiguous():
            raise ValueError(f"tp_mask must be a contiguous int32 tensor [{n},{T}]")
        best = match = used = None
        if debug:
            best = torch.empty((n, T), dtype=torch.float64, device=self.device)
            match = torch.empty((n, T), dtype=torch.int32, device=self.device)
            used = torch.empty((n, max_gt), dtype=torch.int32, device=self.device)
        arr = (C.c_double * max(len(thr), 1))(*thr)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_map_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), ext.ptr(valid), n, T,
                                            ext.ptr(scale_dev), ext.ptr(gt_dev), ext.ptr(gt_count_dev), max_gt, arr, len(thr),
                                            ext.ptr(tp_mask), ext.ptr(best), ext.ptr(match), ext.ptr(used), ext.stream_ptr()))
        return (tp_mask, best, match, used) if debug else tp_mask

    # ---------------------------------------------------------------- COCO matching
    def _coco_fields(self, n, n_areas, max_gt, mask_dtype):
        T = self.T
        return [("float32", (n, T)), ("float32", (n, T)), ("int32", (n,)), ("int32", (n,)), ("int32", (n, T)),
                (mask_dtype, (n, n_areas, T)), (mask_dtype, (n, n_areas, T)), (mask_dtype, (n, max_gt))]

    def alloc_coco_outputs_flat(self, n, n_areas, max_gt):
        """What `Yolov4.evaluate_coco` needs of a batch as views of ONE int32 device block -- scores, classes, valid, the
        candidate counts of the tiled paths, and cls_rank, dt_match, dt_ignore, gt_ignore of `coco_match_device` -- so that they
        reach the host in a single copy (`coco_outputs_to_host`); the boxes are a tensor of their own and stay on the device.
        -> (flat int32 tensor, outs for `decode_nms_device` / `predict_tiled_device(outputs=)` (boxes, scores, classes, valid, no
        kept indices -- with `nms_merge` a tensor outside the block), cand_count int32 view [n], (cls_rank [n,max_total],
        dt_match [n,n_areas,max_total], dt_ignore, gt_ignore [n,max_gt]) int32 views)."""
        flat, (scores, classes, valid, cand, rank, dm, di, gi) = self._alloc_block(self._coco_fields(n, n_areas, max_gt, "int32"))
        boxes = self.torch.empty((n, self.T, 4), dtype=self.torch.float32, device=self.device)
        kept = self.torch.empty((n, self.T), dtype=self.torch.int32, device=self.device) if self.nms_merge else None
        return flat, (boxes, scores, classes, valid, kept), cand, (rank, dm, di, gi)

    def coco_outputs_to_host(self, flat, n, n_areas, max_gt):
        """The one copy of `alloc_coco_outputs_flat`'s block -> (scores float32 [n,T], classes float32 [n,T], valid int32 [n],
        cand_count int32 [n], cls_rank int32 [n,T], dt_match uint32 [n,A,T], dt_ignore uint32 [n,A,T], gt_ignore uint32
        [n,max_gt]) as numpy views of it."""
        return tuple(_block_views(flat.cpu().numpy(), self._coco_fields(n, n_areas, max_gt, "uint32")))

    def coco_match_device(self, outs, scale_dev, gt_dev, gt_count_dev, iou_thresholds, area_ranges, debug=False, out=None):
        """y4_coco_match on the outputs of `decode_nms_device` / `predict_tiled_device` / `predict_tta_device` (outs = boxes,
        scores, classes, valid, ...): the kept boxes of each image, scaled to raw-image pixels by scale_dev (float32 cuda [n,2]:
        w, h), are matched against gt_dev (float32 cuda [n,max_gt,5]; gt_count_dev int32 [n]) by COCO's rule (csrc/coco_match.hip),
        once per area range (1..4 rows [lo, hi]) and IoU threshold (1..16).  -> (cls_rank int32 [n,max_total], dt_match int32
        [n,A,max_total] with bit t "matched at iou_thresholds[t]", dt_ignore likewise, gt_ignore int32 [n,max_gt] with bit a) as
        cuda tensors -- `out`, the views of `alloc_coco_outputs_flat`, when given; with debug=True also match_row int32
        [n,A,T,max_total].  Asynchronous."""
        torch = self.torch
        boxes, scores, classes, valid = outs[:4]
        n, T = scores.shape
        thr = [float(t) for t in iou_thresholds]
        rng = np.asarray(area_ranges, dtype=np.float64)
        if rng.ndim != 2 or rng.shape[1] != 2:
            raise ValueError(f"area_ranges must be rows [lo, hi], got shape {rng.shape}")
        A = len(rng)
        max_gt = self._check_match_inputs(n, scale_dev, gt_dev, gt_count_dev)
        shapes = ((n, T), (n, A, T), (n, A, T), (n, max_gt))
        if out is None:
            out = tuple(torch.empty(shape, dtype=torch.int32, device=self.device) for shape in shapes)
        elif len(out) != 4 or any(tuple(o.shape) != shape or o.dtype != torch.int32 or not o.is_contiguous()
                                  for o, shape in zip(out, shapes)):
            raise ValueError(f"out must be contiguous int32 tensors of shapes {shapes}")
        rank, dm, di, gi = out
        rows = torch.empty((n, A, len(thr), T), dtype=torch.int32, device=self.device) if debug else None
        thr_arr = (C.c_double * max(len(thr), 1))(*thr)
        rng_arr = (C.c_double * max(rng.size, 1))(*rng.reshape(-1).tolist())
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_coco_match(ext.ptr(boxes), ext.ptr(scores), ext.ptr(classes), ext.ptr(valid), n, T,
                                             ext.ptr(scale_dev), ext.ptr(gt_dev), ext.ptr(gt_count_dev), max_gt, rng_arr, A,
                                             thr_arr, len(thr), ext.ptr(dm), ext.ptr(di), ext.ptr(rank), ext.ptr(gi),
                                             ext.ptr(rows), ext.stream_ptr()))
        return (rank, dm, di, gi, rows) if debug else (rank, dm, di, gi)

    def predict_device(self, imgs_dev, outs=None):
        """The whole hot path on device buffers: forward + decode + NMS (async on the current stream).  With `nms_merge` on:
        the forward, then the merged decode + NMS entry, on the same stream."""
        n = imgs_dev.shape[0]
        u8 = self._check_device_images(imgs_dev)
        outs = outs or self.alloc_outputs(n)
        if self.nms_merge:
            self.forward_device(imgs_dev)
            return self.decode_nms_device(n, outs)
        b, s, c, v, k = outs
        with self.torch.cuda.device(self.device):
            fn = self.lib.y4_predict_u8 if u8 else self.lib.y4_predict
            ext.check(fn(self.handle, ext.ptr(imgs_dev), n, ext.ptr(b), ext.ptr(s), ext.ptr(c),
                         ext.ptr(v), ext.ptr(k), ext.stream_ptr()))
        return outs

    def _chunks(self, imgs):
        t = self._to_device_images(imgs)
        if t.shape[0] == 0:                                 # Keras' Model.predict raises ValueError on an empty input as well
            raise ValueError("predict: no images (input of shape %s)" % (tuple(t.shape),))
        for i in range(0, t.shape[0], self.max_batch):     # Keras predict() chunks too (batch_size=32), invisibly
            yield t[i:i + self.max_batch]

    def _paired_chunks(self, imgs, count, rows="labels"):
        """`_chunks(imgs)` walked beside `count` per-image rows (the labels; rows="box_map": predict's map rows) -> (index of the
        chunk's first image, chunk).  ValueError before a chunk is handed out that has no rows, and at the end when rows are left
        over.  count None: nothing to pair, nothing refused."""
        more, left = {"labels": ("labels for {count} images, the images are more", "labels for {count} images, but {i0} images"),
                      "box_map": ("box_map has {count} rows, the images are more", "box_map has {count} rows for {i0} images")}[rows]
        i0 = 0
        for chunk in self._chunks(imgs):
            if count is not None and i0 + chunk.shape[0] > count:
                raise ValueError(more.format(count=count))
            yield i0, chunk
            i0 += chunk.shape[0]
        if count is not None and i0 != count:
            raise ValueError(left.format(count=count, i0=i0))

    def forward_heads(self, imgs):
        """yolo_model.predict(imgs): list of 3 float32 numpy arrays [N,g,g,3(C+5)] (raw logits)."""
        parts = [[], [], []]
        for chunk in self._chunks(imgs):
            self.forward_device(chunk)
            for i, o in enumerate(self.heads_device(chunk.shape[0])):
                parts[i].append(o.cpu().numpy())
        return [np.concatenate(p, axis=0) for p in parts]

    def predict(self, imgs, with_indices=False, iou_threshold=-1.0, score_threshold=-1.0, box_map=None):
        """inference_model.predict(imgs): [boxes [N,100,4], scores [N,100], classes [N,100], valid [N] int32]
        as fresh, writable host numpy arrays (the reference's export_prediction mutates them in place,
        models.py:167-168).  box_map [N,4] (a cuda tensor or an array; `preprocess_u8_batch`, prepost.box_map): the boxes
        come back normalised to each SOURCE image instead of the canvas (letterbox input); None: canvas-normalised."""
        acc = [[], [], [], [], []]
        if box_map is not None:
            torch = self.torch
            bm = box_map if isinstance(box_map, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(box_map, np.float32))
            box_map = bm.to(self.device, dtype=torch.float32).contiguous()
        for i0, chunk in self._paired_chunks(imgs, None if box_map is None else box_map.shape[0], "box_map"):
            n = chunk.shape[0]
            self.forward_device(chunk)
            bm = None if box_map is None else box_map[i0:i0 + n]
            outs = self.decode_nms_device(n, None, iou_threshold, score_threshold, box_map=bm)
            for i, o in enumerate(outs):
                acc[i].append(o.cpu().numpy())
        res = [np.concatenate(p, axis=0) for p in acc]
        return res if with_indices else res[:4]

    # ---------------------------------------------------------------- validation loss
    def _loss_max_boxes(self):
        return int(self.config.get("max_boxes", 100))

    def assign_device(self, boxes_dev):
        """y4_loss_assign: boxes_dev, a contiguous float32 cuda tensor [n, max_boxes, 5] (x1, y1, x2, y2, class in network-input
        pixels) -> (records int32 [n, max_boxes, 8 + mw], counts int32 [n], xywh float32 [n, max_boxes, 4]) on the device
        (yolo4hip/data.py describes the record).  counts[i] == -1: image i has a box off the grid or an unknown class."""
        torch = self.torch
        mb = self._loss_max_boxes()
        if boxes_dev.dtype != torch.float32 or boxes_dev.dim() != 3 or tuple(boxes_dev.shape[1:]) != (mb, 5) \
                or not boxes_dev.is_contiguous():
            raise ValueError(f"boxes must be a contiguous float32 tensor [n, max_boxes={mb}, 5], got {boxes_dev.dtype} "
                             f"{tuple(boxes_dev.shape)}")
        from .data import record_words
        n = boxes_dev.shape[0]
        rec = torch.empty((n, mb, record_words(self.num_classes)), dtype=torch.int32, device=self.device)
        cnt = torch.empty((n,), dtype=torch.int32, device=self.device)
        xywh = torch.empty((n, mb, 4), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_loss_assign(self.handle, n, ext.ptr(boxes_dev), mb, ext.ptr(xywh), ext.ptr(rec), ext.ptr(cnt),
                                              ext.stream_ptr()))
        return rec, cnt, xywh

    def upload_records(self, records, true_xywh):
        """Host records (a list of per-image int32 arrays, data.records_from_dense / records_from_boxes) and the
        [n, max_boxes, 4] xywh array -> the device triple `loss_device` takes."""
        from .data import pad_records
        torch = self.torch
        mb = self._loss_max_boxes()
        xywh = np.ascontiguousarray(true_xywh, dtype=np.float32)
        if xywh.ndim != 3 or xywh.shape != (len(records), mb, 4):
            raise ValueError(f"true boxes must be [{len(records)}, max_boxes={mb}, 4], got {xywh.shape}")
        rec, cnt = pad_records(records, mb, self.num_classes)
        return (torch.from_numpy(rec).to(self.device), torch.from_numpy(cnt).to(self.device),
                torch.from_numpy(xywh).to(self.device))

    def loss_device(self, n, boxes_dev=None, records=None, iou_loss_thresh=None):
        """The loss terms of the heads in the workspace (forward_device / set_heads): float32 cuda tensor [n, 3 scales, 3]
        = per image and scale the box, confidence and class sums (y4_loss).  Labels: `boxes_dev` [n, max_boxes, 5] (assigned
        on the device), or `records` = the (records, counts, xywh) triple of `assign_device` / `upload_records`."""
        torch = self.torch
        rec, cnt, xywh = self._labels(n, boxes_dev, records)
        thr = self._thr(iou_loss_thresh)
        fl = C.c_size_t()
        ext.check(self.lib.y4_loss_scratch_floats(self.handle, n, C.byref(fl)))
        scratch = torch.empty((fl.value,), dtype=torch.float32, device=self.device)
        out = torch.empty((n, 3, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_loss(self.handle, n, ext.ptr(rec), ext.ptr(cnt), ext.ptr(xywh), self._loss_max_boxes(), thr,
                                       ext.ptr(scratch), fl.value, ext.ptr(out), ext.stream_ptr()))
        return out

    def _check_boxes(self, boxes):
        """Host-side refusal of what the reference fails on (a centre off the grid, a class id without a class) before upload."""
        mb = self._loss_max_boxes()
        b = np.ascontiguousarray(boxes, dtype=np.float32)
        if b.ndim != 3 or b.shape[1:] != (mb, 5):
            raise ValueError(f"boxes must be [n, max_boxes={mb}, 5], got {b.shape}")
        H, W = self.img_hw
        used = np.arange(mb)[None, :] < (b[..., 2] - b[..., 0] > 0).sum(axis=1)[:, None]     # rows 0 .. (valid rows - 1)
        norm = np.empty(b.shape[:2] + (2,), dtype=np.float32)
        norm[...] = ((b[..., 0:2] + b[..., 2:4]) // 2) / np.array([W, H], dtype=np.int32)
        off = used & ~((norm >= 0) & (norm < 1)).all(axis=-1)
        cls = b[..., 4].astype(np.int32)
        bad_cls = used & ~((cls >= 0) & (cls < self.num_classes))
        if off.any():
            i, k = np.argwhere(off)[0]
            raise ValueError(f"image {i} box {k}: centre is outside the {H} x {W} input")
        if bad_cls.any():
            i, k = np.argwhere(bad_cls)[0]
            raise ValueError(f"image {i} box {k}: class id {cls[i, k]} outside [0, {self.num_classes})")
        return b

    def loss(self, imgs, boxes=None, records=None, true_xywh=None, iou_loss_thresh=None):
        """Forward + label assignment + loss, chunked by max_batch like `predict`: float32 numpy [N, 3, 3] per image and scale
        (box, confidence, class sums; `combine_loss` weighs them).  Labels: `boxes` [N, max_boxes, 5], assigned on the device,
        or host `records` (one int32 array per image) with `true_xywh` [N, max_boxes, 4]."""
        torch = self.torch
        if (boxes is None) == (records is None):
            raise ValueError("loss: give boxes or records")
        if boxes is not None:
            boxes_dev = torch.from_numpy(self._check_boxes(boxes)).to(self.device)
            count = boxes_dev.shape[0]
        else:
            triple = self.upload_records(records, true_xywh)
            count = len(records)
        parts = []
        for i0, chunk in self._paired_chunks(imgs, count):
            n = chunk.shape[0]
            self.forward_device(chunk)
            if boxes is not None:
                out = self.loss_device(n, boxes_dev=boxes_dev[i0:i0 + n], iou_loss_thresh=iou_loss_thresh)
            else:
                out = self.loss_device(n, records=tuple(t[i0:i0 + n] for t in triple), iou_loss_thresh=iou_loss_thresh)
            parts.append(out.cpu().numpy())
        return np.concatenate(parts, axis=0)

    # ---------------------------------------------------------------- fine-tuning (csrc/head_train.hip, csrc/block_train.hip)
    HEAD_CONVS = (93, 101, 109)
    BLOCK_CONVS = (92, 100, 108)
    # A trainable group, in the order a step runs them.  Its record in a conv's part of the Darknet stream: behind `skip`
    # vectors of cout floats, cout * (bias + cin * ksize^2) floats.  C entry points y4_<name>_grad / _adam and the scratch
    # query; `grad` is the gradient buffer's name in messages.  keep_scratch: heads take fresh float scratch per call, blocks
    # keep one byte buffer on the engine (hundreds of MB at batch 32).
    _GROUPS = {
        "heads": dict(name="head", convs=HEAD_CONVS, skip=0, bias=1, ksize=1, grad="dw", query="y4_head_grad_scratch_floats",
                      keep_scratch=False),
        "blocks": dict(name="block", convs=BLOCK_CONVS, skip=4, bias=0, ksize=3, grad="dk", query="y4_block_grad_scratch_bytes",
                       keep_scratch=True),
    }

    def _labels(self, n, boxes_dev, records):
        if (boxes_dev is None) == (records is None):
            raise ValueError("give boxes_dev or records")
        rec, cnt, xywh = self.assign_device(boxes_dev) if records is None else records
        if rec.shape[0] != n or cnt.shape[0] != n or xywh.shape[0] != n:
            raise ValueError(f"labels are for {rec.shape[0]} images, the batch has {n}")
        return rec, cnt, xywh

    def _thr(self, iou_loss_thresh):
        return float(self.config.get("iou_loss_thresh", 0.5) if iou_loss_thresh is None else iou_loss_thresh)

    def _img_weight(self, n, img_weight):
        torch = self.torch
        if img_weight is None:
            return torch.full((n,), 1.0 / n, dtype=torch.float32, device=self.device)
        if not isinstance(img_weight, torch.Tensor):
            img_weight = torch.from_numpy(np.ascontiguousarray(img_weight, dtype=np.float32))
        w = img_weight.to(self.device, dtype=torch.float32).contiguous()
        if tuple(w.shape) != (n,):
            raise ValueError(f"img_weight must have shape ({n},), got {tuple(w.shape)}")
        return w

    def loss_grad_device(self, n, boxes_dev=None, records=None, iou_loss_thresh=None, img_weight=None):
        """y4_loss_grad: the DENSE gradient of sum_i img_weight[i] * loss_i (default 1 / n: the batch mean) w.r.t. the raw heads
        in the workspace: three float32 cuda tensors [n, gh, gw, 3 (5 + C)].  For tests; training never builds these."""
        torch = self.torch
        rec, cnt, xywh = self._labels(n, boxes_dev, records)
        w = self._img_weight(n, img_weight)
        outs = [torch.empty((n, gh, gw, self.nout), dtype=torch.float32, device=self.device) for gh, gw in self.grids_hw]
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_loss_grad(self.handle, n, ext.ptr(rec), ext.ptr(cnt), ext.ptr(xywh), self._loss_max_boxes(),
                                            self._thr(iou_loss_thresh), ext.ptr(w), ext.ptr(outs[0]), ext.ptr(outs[1]),
                                            ext.ptr(outs[2]), ext.stream_ptr()))
        return outs

    # ---- one implementation per verb; the public head_* / block_* methods below name the group
    def _group_records(self, g):
        g, lt = self._GROUPS[g], self.layer_table()
        return [(int(lt[i]["weight_offset"] + g["skip"] * lt[i]["cout"]),
                 int(lt[i]["cout"] * (g["bias"] + lt[i]["cin"] * g["ksize"] ** 2))) for i in g["convs"]]

    def _group_floats(self, g):
        return sum(n for _, n in self._group_records(g))

    def _group_scratch(self, g, n):
        torch, g = self.torch, self._GROUPS[g]
        size = C.c_size_t()
        ext.check(getattr(self.lib, g["query"])(self.handle, n, C.byref(size)))
        if not g["keep_scratch"]:
            return torch.empty((size.value,), dtype=torch.float32, device=self.device)
        scratch = getattr(self, "_block_scratch", None)
        if scratch is None or scratch.numel() < size.value:
            scratch = self._block_scratch = torch.empty((size.value,), dtype=torch.uint8, device=self.device)
        return scratch

    def _group_grad_device(self, g, n, boxes_dev, records, iou_loss_thresh, img_weight, dw, accumulate, loss_scale=None,
                           overflow=None):
        """loss_scale (blocks only): the call goes through y4_block_grad_scaled, which ORs its flags into `overflow`"""
        torch = self.torch
        name, grad, total = self._GROUPS[g]["name"], self._GROUPS[g]["grad"], self._group_floats(g)
        rec, cnt, xywh = self._labels(n, boxes_dev, records)
        w = self._img_weight(n, img_weight)
        if dw is None:
            if accumulate:
                raise ValueError(f"{name}_grad_device: accumulate needs the {grad} to add to")
            dw = torch.empty((total,), dtype=torch.float32, device=self.device)
        if dw.dtype != torch.float32 or dw.numel() != total or not dw.is_contiguous():
            raise ValueError(f"{grad} must be a contiguous float32 tensor of {total} elements")
        scratch = self._group_scratch(g, n)
        scaled = () if loss_scale is None else (float(loss_scale), ext.ptr(overflow))
        with torch.cuda.device(self.device):
            ext.check(getattr(self.lib, f"y4_{name}_grad" + ("_scaled" if scaled else ""))(
                self.handle, n, ext.ptr(rec), ext.ptr(cnt), ext.ptr(xywh), self._loss_max_boxes(), self._thr(iou_loss_thresh),
                ext.ptr(w), *scaled, ext.ptr(scratch), scratch.numel(), ext.ptr(dw), total, 1 if accumulate else 0, ext.stream_ptr()))
        return dw

    def _group_state(self, g, flat):
        torch = self.torch
        flat = np.asarray(flat, dtype=np.float32)
        w = np.concatenate([flat[o:o + n] for o, n in self._group_records(g)])
        w = torch.from_numpy(np.ascontiguousarray(w)).to(self.device)
        return {"w": w, "m": torch.zeros_like(w), "v": torch.zeros_like(w), "t": 0}

    def _group_adam_step(self, g, state, dw, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7):
        state["t"] += 1
        with self.torch.cuda.device(self.device):
            ext.check(getattr(self.lib, f"y4_{self._GROUPS[g]['name']}_adam")(
                self.handle, ext.ptr(dw), ext.ptr(state["w"]), ext.ptr(state["m"]), ext.ptr(state["v"]), state["w"].numel(),
                float(lr), float(beta1), float(beta2), float(epsilon), int(state["t"]), ext.stream_ptr()))

    def _group_weights_to_flat(self, g, state, flat):
        w = state["w"].cpu().numpy()
        pos = 0
        for o, n in self._group_records(g):
            flat[o:o + n] = w[pos:pos + n]
            pos += n
        return flat

    # ---- the three detection convs
    def head_records(self):
        """[(float offset in the Darknet stream, floats)] of the records of convs 93 / 101 / 109: cout biases, then cout x cin
        weights.  The gradient, master-weight and moment buffers hold these three records back to back."""
        return self._group_records("heads")

    def head_floats(self):
        return self._group_floats("heads")

    def head_grad_device(self, n, boxes_dev=None, records=None, iou_loss_thresh=None, img_weight=None, dw=None, accumulate=False):
        """y4_head_grad after `forward_device` on n images (an engine with retain_head_inputs): the gradient of
        sum_i img_weight[i] * loss_i w.r.t. the weights and biases of convs 93 / 101 / 109 -> float32 cuda tensor
        [head_floats()] (`head_records` gives the layout), written into `dw` or, with accumulate=True, added to it."""
        return self._group_grad_device("heads", n, boxes_dev, records, iou_loss_thresh, img_weight, dw, accumulate)

    def head_state(self, flat):
        """The optimiser state for `head_adam_step`: float32 master weights (the three head records of the host stream `flat`,
        uploaded) and zero moments -> {'w', 'm', 'v', 't'}."""
        return self._group_state("heads", flat)

    def head_adam_step(self, state, dw, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7):
        """y4_head_adam: one step of Keras' Adam on the master weights of `state` with the gradient `dw`, and the re-pack: the
        next forward of this engine runs on the updated head convs."""
        self._group_adam_step("heads", state, dw, lr, beta1, beta2, epsilon)

    def head_weights_to_flat(self, state, flat):
        """Copy the master weights of `state` back into the host stream `flat` (in place)."""
        return self._group_weights_to_flat("heads", state, flat)

    # ---- the 3x3 convs in front of them
    def block_records(self):
        """[(float offset in the Darknet stream, floats)] of the KERNELS of convs 92 / 100 / 108: cout x cin x 3 x 3 weights in
        (out, in, kh, kw) order, behind the layer's four BatchNormalization vectors.  The gradient, master-weight and moment
        buffers hold these three kernels back to back."""
        return self._group_records("blocks")

    def block_floats(self):
        return self._group_floats("blocks")

    def block_grad_device(self, n, boxes_dev=None, records=None, iou_loss_thresh=None, img_weight=None, dk=None, accumulate=False,
                          loss_scale=None, overflow=None):
        """y4_block_grad after `forward_device` on n images (an engine with retain_head_inputs=2), BEFORE the step's
        `head_adam_step`: the gradient of sum_i img_weight[i] * loss_i w.r.t. the kernels of convs 92 / 100 / 108 -> float32 cuda
        tensor [block_floats()] (`block_records` gives the layout), written into `dk` or, with accumulate=True, added to it.

        loss_scale (a power of two; what an f16 engine needs): y4_block_grad_scaled -- dZ is multiplied by it before its
        rounding to the operand type and the sum divided by it.  -> (dk, overflow): `overflow` is an int32[1] device tensor the
        call ORs into and never clears (created zeroed when not given); bit 0 an inf / NaN in the stored dZ, bit 1 a non-finite
        sum.  When it is non-zero `dk` holds nothing usable."""
        if loss_scale is None:
            if overflow is not None:
                raise ValueError("block_grad_device: overflow needs a loss_scale")
            return self._group_grad_device("blocks", n, boxes_dev, records, iou_loss_thresh, img_weight, dk, accumulate)
        torch = self.torch
        if overflow is None:
            overflow = torch.zeros((1,), dtype=torch.int32, device=self.device)
        if overflow.dtype != torch.int32 or overflow.numel() != 1 or overflow.device != self.device:
            raise ValueError("overflow must be an int32 tensor of one element on the engine's device")
        dk = self._group_grad_device("blocks", n, boxes_dev, records, iou_loss_thresh, img_weight, dk, accumulate, loss_scale, overflow)
        return dk, overflow

    def block_state(self, flat):
        """The optimiser state for `block_adam_step`: float32 master kernels (the three kernels of the host stream `flat`,
        uploaded) and zero moments -> {'w', 'm', 'v', 't'}."""
        return self._group_state("blocks", flat)

    def block_adam_step(self, state, dk, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7):
        """y4_block_adam: one step of Keras' Adam on the master kernels of `state` with the gradient `dk`, and the re-pack: the
        next forward of this engine runs on the updated convs 92 / 100 / 108."""
        self._group_adam_step("blocks", state, dk, lr, beta1, beta2, epsilon)

    def block_weights_to_flat(self, state, flat):
        """Copy the master kernels of `state` back into the host stream `flat` (in place); the BatchNormalization vectors stay."""
        return self._group_weights_to_flat("blocks", state, flat)

    def _check_stream_batch(self, a, u8, yuv):
        """ValueError unless `a` (of dtype `u8`) is a batch `predict_stream` takes."""
        if yuv is not None:
            if a.dtype != u8 or a.ndim != 3 or not 1 <= a.shape[0] <= self.max_batch \
                    or a.shape[1] < 3 or a.shape[1] % 3 or a.shape[2] < 2 or a.shape[2] % 2:
                raise ValueError(f"expected uint8 [n<={self.max_batch}, h + h // 2, w] {yuv} batches with even h, w, got "
                                 f"{a.dtype} {tuple(a.shape)}")
        elif a.dtype != u8 or a.ndim != 4 or a.shape[3] != 3 or not 1 <= a.shape[0] <= self.max_batch:
            raise ValueError(f"expected uint8 [n<={self.max_batch},h,w,3] batches, got {a.dtype} {a.shape}")

    def _stream_setup(self, in_flight):
        """-> (the engines that compute `in_flight` batches at a time: this one and its siblings, the in_flight + 1 staging slots)."""
        sibs = getattr(self, "_stream_siblings", [])
        while len(sibs) < in_flight - 1:
            sibs.append(self.sibling())
        self._stream_siblings = sibs
        for e in sibs[:in_flight - 1]:
            self.copy_schedule_to(e)                       # (the engine may have been re-tuned since the sibling was made)
        nslots = in_flight + 1                             # one more staging slot than computing batches: the next upload runs ahead
        # the staging slots (pinned host buffers, device frames, output blocks, events) outlive the call: pinning tens of MB
        # costs milliseconds, which a short stream would pay again on every call
        cache = getattr(self, "_stream_slots", None)
        if cache is None or len(cache) != nslots:
            for sl in cache or []:                         # an abandoned generator may have left copies in flight on these buffers
                for ev in ("up", "ran", "done"):
                    if ev in sl:
                        sl[ev].synchronize()
            cache = self._stream_slots = [{} for _ in range(nslots)]
        for sl in cache:
            if "done" in sl:
                sl["done"].synchronize()
        return [self] + sibs[:in_flight - 1], cache

    def _stream_route(self, shape, letterbox, yuv, yuv_flags):
        """How batches of `shape` reach the network and where their boxes go -> (launch, table, maps).  launch: None -- RGB frames of
        the network's size are fed as they lie --, `Engine.resize_u8` -- equal RGB frames stretched, no table --, or the ragged method
        that reads `table`, the rows the batch preprocessors build for max_batch equal sources back to back: `resize_u8_ragged` for
        letterboxed RGB, `yuv_u8_ragged` for video, always.  maps: boxes are mapped under letterbox, unless the frame has the network's size."""
        (H, W), B = self.img_hw, self.max_batch
        if yuv is None:
            fh, fw = shape[1:3]
            if (fh, fw) == (H, W):
                return None, None, None
            if not letterbox:
                return Engine.resize_u8, None, None
            desc, maps = canvas.fit_table(ext.y4_image_desc, [(fh, fw)] * B, H, W, True)
            canvas.place_sources(desc, [(fh, fw, 3)] * B)
            return Engine.resize_u8_ragged, desc, maps
        from . import yuv as yuvmod
        layout = yuvmod.YuvFrame(np.empty(shape[1:], np.uint8), fmt=yuv)       # (the plane offsets of one frame)
        desc, maps = canvas.fit_table(ext.y4_yuv_desc, [(layout.h, layout.w)] * B, H, W, letterbox)
        canvas.place_sources(desc, [(layout.nbytes,)] * B, place=lambda d, k, off: layout.fill_desc(d, off, yuv_flags))
        return Engine.yuv_u8_ragged, desc, maps if letterbox and (layout.h, layout.w) != (H, W) else None

    def _stream_rekey(self, sl, key, compute):
        """(Re)allocate the staging of slot `sl` for key = (batch shape, letterbox, pad_value, yuv, yuv_flags)."""
        torch, dev = self.torch, self.device
        shape, letterbox, _, yuv, yuv_flags = key
        if "done" in sl:
            sl["done"].synchronize()
        sl["key"] = key
        sl["pin"] = torch.empty(shape, dtype=torch.uint8).pin_memory()
        sl["pin_np"] = sl["pin"].numpy()
        sl["u8"] = torch.empty(shape, dtype=torch.uint8, device=dev)
        sl["launch"], table, maps = self._stream_route(shape, letterbox, yuv, yuv_flags)
        # frames of another size are resized uint8 -> uint8 on the device; the /255 happens in the stem's load
        sl["net"] = None if sl["launch"] is None else \
            torch.empty((self.max_batch, self.img_hw[0], self.img_hw[1], 3), dtype=torch.uint8, device=dev)
        sl["table"] = None if table is None else torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
        sl["map"] = None if maps is None else torch.from_numpy(maps).to(dev)
        if table is not None:
            torch.cuda.current_stream().synchronize()      # (read by the compute streams)
        # one flat int32 block per slot holds all five outputs, so that results return in ONE small D2H copy
        fields = _detection_fields(self.max_batch, self.T)
        sl["flat"], sl["outs"] = self._alloc_block(fields)
        sl["flat_host"] = torch.empty(_block_len(fields), dtype=torch.int32).pin_memory()
        sl["host"] = _block_views(sl["flat_host"], fields)
        sl["up"], sl["done"], sl["free"], sl["ran"] = (torch.cuda.Event() for _ in range(4))
        sl["free"].record(compute)

    def predict_stream(self, batches, with_indices=False, in_flight=None, letterbox=False, pad_value=128, yuv=None,
                       matrix='bt601', full_range=False):
        """Pipelined `inference_model.predict` over an iterable of uint8 batches ([n,h,w,3] numpy arrays or pinned torch
        tensors, n <= max_batch, any h,w): yields one result list per batch, in order.  A pinned tensor is uploaded from where
        it lies and may be refilled as soon as the generator yields (its upload is waited for before every yield).  While batch i computes, batch i+1 crosses PCIe as uint8
        on a second HIP stream (pinned staging, 4x fewer bytes than float32) and batch i-1's results return to the
        host, so the PCIe-inclusive rate approaches the device rate.  No float image tensor exists: frames are resized
        uint8 -> uint8 on the device when needed (`y4_resize_u8`) and the `/ 255.` happens inside the stem's operand load
        (`y4_predict_u8`), bit-identical to `Yolov4.preprocess_img` (reference models.py:95-98) + float32 forward.
        `in_flight` batches compute at the same time, each on its own HIP stream and activation workspace (`sibling()`: shared
        packed weights), so that one batch's idle compute units are the other's (see `InFlight`); results are unchanged and still
        come in order.  Every batch in flight beyond the first costs one more activation workspace for the engine's lifetime
        (`act_bytes`: 2.9 GB at 608x608 / batch 32 / bf16 with `alias_workspace`, 8.0 GB without), so the default is 2 with an
        aliased workspace and 1 with the plain one; pass `in_flight` to choose.
        letterbox=True: frames are letterboxed instead of stretched (`y4_resize_u8_ragged` with one descriptor per frame, all the
        same rectangle) and the boxes come back normalised to the frame (`y4_decode_nms_mapped`): what
        `preprocess_u8_batch(letterbox=True)` + `predict(..., box_map=)` give, batch by batch.
        yuv='nv12' | 'nv21' | 'i420' | 'yv12': a batch is uint8 [n, h + h // 2, w] with even h, w -- n video frames in the
        rawvideo layout, tight pitches -- and crosses PCIe as it is, 1.5 bytes per pixel instead of 3.  One launch
        (`y4_yuv_u8_ragged`, the descriptor table built once per geometry) converts under `matrix` / `full_range` and writes the
        network batch, stretched or letterboxed, also when the frame already has the network's size: the results are those of
        this generator on the `yuv.to_rgb` frames.  yuv=None is the RGB path, launch for launch as before."""
        torch = self.torch
        dev = self.device
        yuv_flags = 0
        if yuv is not None:
            from . import yuv as yuvmod
            if yuv not in yuvmod.FORMATS:
                raise ValueError(f"yuv must be None or one of {yuvmod.FORMATS}, got {yuv!r}")
            yuv_flags = yuvmod.flags(matrix, full_range)
        copy_stream = torch.cuda.Stream(device=dev)        # uploads
        down_stream = torch.cuda.Stream(device=dev)        # results (its own stream: it waits for the compute stream)
        if in_flight is None:
            in_flight = 2 if self.alias_workspace else 1
        in_flight = max(1, int(in_flight))
        engines, slots = self._stream_setup(in_flight)
        nslots = len(slots)
        pending = []

        def finish(sl):
            sl["done"].synchronize()
            res = [t[:sl["n"]].numpy().copy() for t in sl["host"]]
            return res if with_indices else res[:4]

        with torch.cuda.device(dev):
            cstreams = [torch.cuda.current_stream()] + [torch.cuda.Stream(device=dev) for _ in engines[1:]]
            for bi, batch in enumerate(batches):
                pinned_in = isinstance(batch, torch.Tensor) and batch.is_pinned() and batch.is_contiguous()
                a = batch if pinned_in else np.ascontiguousarray(batch)
                self._check_stream_batch(a, torch.uint8 if pinned_in else np.uint8, yuv)
                sl = slots[bi % nslots]
                eng, compute = engines[bi % in_flight], cstreams[bi % in_flight]     # batches alternate engines; slots rotate on their own
                key = (tuple(a.shape), bool(letterbox), int(pad_value), yuv, yuv_flags)
                if sl.get("key") != key:
                    self._stream_rekey(sl, key, compute)
                n = sl["n"] = a.shape[0]
                sl["free"].synchronize()                   # the slot's previous uint8 frame has been consumed
                # plain single-threaded memcpy into the pinned staging buffer: torch's multi-threaded host copy leaves
                # its worker pool spinning, which stalls the HIP runtime's own threads for tens of ms (measured).
                # A batch that already is a pinned uint8 tensor is uploaded from where it lies.
                if not pinned_in:
                    np.copyto(sl["pin_np"], a)
                with torch.cuda.stream(copy_stream):
                    sl["u8"].copy_(batch if pinned_in else sl["pin"], non_blocking=True)
                    sl["up"].record(copy_stream)
                compute.wait_event(sl["up"])
                with torch.cuda.stream(compute):
                    if sl["launch"] is None:               # frames of the network's size: fed as they lie
                        frames = sl["u8"]
                    elif sl["table"] is None:              # equal frames, stretched: the non-ragged resize
                        frames = eng.resize_u8(sl["u8"], sl["net"])
                    else:                                  # one ragged launch over the slot's table (letterbox; video frames, always)
                        frames = sl["launch"](eng, sl["u8"], sl["table"], n, sl["net"], pad_value)
                    outs = tuple(t[:n] for t in sl["outs"])
                    if sl["map"] is None:
                        eng.predict_device(frames[:n], outs)
                    else:                                  # boxes mapped back to the frame in the NMS output
                        eng.forward_device(frames[:n])
                        eng.decode_nms_device(n, outs, box_map=sl["map"][:n])
                sl["free"].record(compute)                 # the stem has consumed the uint8 frames
                sl["ran"].record(compute)
                with torch.cuda.stream(down_stream):       # results leave on a third stream: compute and uploads never wait
                    down_stream.wait_event(sl["ran"])
                    sl["flat_host"].copy_(sl["flat"], non_blocking=True)
                    sl["done"].record(down_stream)
                if pinned_in:
                    # the upload reads the CALLER's pinned tensor: it must have left host memory before control returns
                    # to a loader that may refill that buffer (the engine's own staging buffer is guarded by sl["free"])
                    sl["up"].synchronize()
                pending.append(sl)
                if len(pending) >= nslots:                 # the oldest batch's slot is needed next: its results leave first
                    yield finish(pending.pop(0))
            while pending:
                yield finish(pending.pop(0))

    def conv_output(self, conv_idx, n):
        """Dense float32 NHWC copy of conv `conv_idx`'s output from the last forward (parity tap)."""
        torch = self.torch
        lt = self.layer_table()[conv_idx]
        dims = (C.c_int32 * 4)()
        ext.check(self.lib.y4_layer_dims(self.handle, conv_idx, dims))
        # upsampling convs (78, 85) store the 2x-upsampled tensor
        up = 2 if conv_idx in (78, 85) else 1
        out = torch.empty((n, dims[2] * up, dims[3] * up, lt["cout"]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            ext.check(self.lib.y4_get_conv_output(self.handle, conv_idx, n, ext.ptr(out), out.numel(), ext.stream_ptr()))
        return out.cpu().numpy()

    def get_tiles(self):
        """The 110 tile ids this engine runs (y4_get_tiles)."""
        tiles = (C.c_int32 * 110)()
        ext.check(self.lib.y4_get_tiles(self.handle, tiles, 110))
        return list(tiles)

    def autotune(self, n=None, reps=3):
        """Pick the fastest tile configuration per conv layer by measurement (results are bit-identical)."""
        n = int(n or self.max_batch)
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_autotune(self.handle, n, int(reps), ext.stream_ptr()))
        return self.get_tiles()

    def autotune_pair(self, other, stream, other_stream, n=None, reps=3, passes=15):
        """`autotune` with throughput as objective, for two batches in flight (`InFlight`): every candidate is timed on this
        engine and on its sibling `other` at once, each on its own HIP stream (y4_autotune_pair).  Both engines end up
        with the same choices; results stay bit-identical.  `passes`: which decisions use the two-stream objective -- bit 0
        tiles, 1 chains / LDS pairs, 2 the stage kernel, 3 the residual-block kernels (the rest: one launch at a time)."""
        n = int(n or self.max_batch)
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_autotune_pair(self.handle, other.handle, n, int(reps), C.c_void_p(stream.cuda_stream),
                                                C.c_void_p(other_stream.cuda_stream), int(passes)))
        return self.get_tiles()

    # ---------------------------------------------------------------- shipped schedules
    @property
    def shape_key(self):
        """The image-size part of schedule file names: the side of a square engine, '<H>x<W>' of a rectangular one."""
        H, W = self.img_hw
        return str(H) if H == W else f"{H}x{W}"

    def shipped_schedule(self):
        """The tuned schedule that ships with the package for this (image side, classes, batch, dtype), or None: the
        per-launch tile ids, the stage-kernel switch and the residual-block mask one `autotune` run chose on an MI355X
        (`yolo4hip/schedules/<side>_<classes>_<batch>_<dtype>.json`; the headline shape's file IS `profiles/r03/tiles.json`,
        the set the committed PMC passes profiled).  A schedule WITHOUT split-K or halo2 ids (`"splitk": false`, `"halo2": false`) is a
        pure scheduling choice: every such choice gives the same bits.  The batch-1 files carry split-K ids (`"splitk": true`), the
        batch-32 / 64 16-bit files since round 6 halo2 ids (`"halo2": true`: family 21, `schedule.uses_halo2`; conv_halo2_kernel.h, v_mfma_32x32x16):
        those sum the K loop in another, fixed fp32 order -- the same on every machine because the file is the same -- and are held
        to the oracle instead (tests/test_gpu_forward.py::test_splitk_latency_schedule_vs_oracle, tests/test_gpu_parity_full.py)."""
        import json
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "schedules",
                            f"{self.shape_key}_{self.num_classes}_{self.max_batch}_{self.dtype}.json")
        try:
            saved = json.load(open(path))
        except (OSError, ValueError):
            return None
        saved["path"] = path
        return saved

    # ---------------------------------------------------------------- no silent un-tuned shapes
    LATENCY_BATCH = 2          # engines for at most this many images are tuned for latency: split-K tile ids allowed

    def schedule_cache_path(self):
        """Where a schedule tuned on first use is kept: $YOLO4HIP_CACHE (default ~/.cache/yolo4hip) / schedules /
        <side>_<classes>_<batch>_<dtype>_<gfx arch>_<library version>.json (<H>x<W>_... for a rectangular engine)."""
        root = os.environ.get("YOLO4HIP_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "yolo4hip")
        arch = self.torch.cuda.get_device_properties(self.device).gcnArchName.split(":")[0]
        ver = self.lib.y4_version().decode().replace(" ", "_").replace("/", "_")
        return os.path.join(root, "schedules", f"{self.shape_key}_{self.num_classes}_{self.max_batch}_{self.dtype}_{arch}_{ver}.json")

    def ensure_schedule(self, tune=True, verbose=True, share=False):
        """Make sure this engine runs a TUNED schedule, and say which: (1) the one that ships with the package for this (image side,
        classes, batch, dtype), else (2) the one a previous process tuned on this machine (`schedule_cache_path`), else (3) tune
        now -- all fusions on, `autotune` on a synthetic batch of `max_batch` images (a full-size predict + a few launches per
        candidate tile: seconds at 160^2, about 20 s at 608^2 x 32), split-K offered only to latency-sized engines
        (`max_batch <= LATENCY_BATCH`) that ask for it (YOLO4HIP_LATENCY=1) -- and write it to the cache.  The weights must be
        loaded.  Every schedule without split-K ids gives the same bits; one with them is tested against the oracle instead
        (`"splitk": true` in the file).  `share=True` under an initialised torch.distributed group makes the call a COLLECTIVE:
        rank 0 resolves (1)-(3), the others take rank 0's schedule from a broadcast (source 'shared') -- one tuning run per job,
        the same tile set on every rank.  EVERY rank of the group must make the call, with the same (size, classes,
        batch, dtype): the shape travels with the schedule and a mismatch raises; a rank 0 that fails to resolve broadcasts the
        failure, so the others raise instead of waiting for the process group's timeout.  The tuned schedule is judged one batch at a time (`"in_flight": 1`) even
        when `predict_stream` later keeps two in flight; `bench.py --pair-passes` / `y4_autotune_pair` is the pair-judged variant.
        Returns (source, path): source in 'shipped' | 'cached' | 'tuned' | 'shared' | 'heuristic' (tune=False and nothing found)."""
        from . import dist as D
        rank, world = D.group_rank_world() if share else (0, 1)
        src, path, saved, err = "heuristic", None, None, None
        mine = [self.img_size if isinstance(self.img_size, int) else list(self.img_size), int(self.num_classes), int(self.max_batch),
                str(self.dtype)]
        if rank == 0:
            try:
                src, path, saved = self._resolve_schedule(tune)
            except Exception as e:                     # (a rank 0 that raised before the broadcast would leave the others hanging in it)
                if world == 1:
                    raise
                err = f"{type(e).__name__}: {e}"
        if world > 1:
            got = D.share_schedule({"schedule": saved, "error": err, "shape": mine} if rank == 0 else None, src=0)
            if got is None or got.get("error"):
                raise RuntimeError("ensure_schedule(share=True): rank 0 could not resolve a schedule" +
                                   (f" ({got['error']})" if got else ""))
            if rank != 0:
                if list(got["shape"]) != mine:
                    raise RuntimeError(f"ensure_schedule(share=True): rank 0 resolved a schedule for (size, classes, batch, dtype) = "
                                       f"{tuple(got['shape'])}, this rank's engine is {tuple(mine)} -- every rank must build the same engine")
                saved = got["schedule"]
                if saved is not None:
                    self._use_schedule(saved)
                    src, path = "shared", None
        self.schedule_source = (src, path)
        if verbose:
            self.say_schedule()
        return src, path

    def say_schedule(self):
        src, path = self.schedule_source
        what = {"shipped": "shipped with the package", "cached": "tuned earlier on this machine", "tuned": "tuned now (first use of this shape)",
                "shared": "rank 0's, received by broadcast", "heuristic": "NONE: built-in tile heuristic, fusion kernels off"}[src]
        print(f"schedule: {what}" + (f" [{os.path.basename(path)}]" if path else ""))

    def _all_fusions_on(self):
        if self.dtype != "f32":
            if self.img_hw[0] == self.img_hw[1] and self.img_hw[0] <= 640:      # (stem_down.hip: square inputs only)
                self.set_stem_fusion(True)
            self.set_chain_fusion(True)
            self.set_stage_fusion(True)
            self.set_res_fusion(True)

    def _use_schedule(self, saved):
        self._all_fusions_on()
        self.apply_schedule(saved)

    def _resolve_schedule(self, tune):
        """(source, path, schedule dict or None) of `ensure_schedule`'s steps (1)-(3) on THIS rank; the schedule is applied."""
        import json
        saved = self.shipped_schedule()
        if saved is not None and len(saved.get("tiles", [])) == 110:
            self._use_schedule(saved)
            return "shipped", saved["path"], saved
        path = self.schedule_cache_path()
        try:
            saved = json.load(open(path))
            if len(saved.get("tiles", [])) != 110:
                raise ValueError("stale")
            self._use_schedule(saved)
            return "cached", path, saved
        except (OSError, ValueError, ext.Y4Error):
            pass
        if not tune:
            return "heuristic", None, None
        torch = self.torch
        self._all_fusions_on()
        # split-K ids only on request: which of them win is decided by this machine's timing, and they change
        # the fp32 summation order -- a schedule tuned on first use would make low-order bits machine-dependent.  The
        # shipped batch-1 schedules have them (one fixed file, tested against the oracle); YOLO4HIP_LATENCY=1 opts in here.
        splitk = self.max_batch <= self.LATENCY_BATCH and os.environ.get("YOLO4HIP_LATENCY", "0") == "1"
        self.set_splitk(splitk)
        from . import weights as W
        imgs = torch.from_numpy(W.synth_images(self.max_batch, self.img_hw, seed=0)).to(self.device)
        self.predict_device(imgs)                      # real activations in the workspace
        self.autotune(self.max_batch, reps=3)
        self.set_splitk(False)
        saved = dict(schedule.describe(self), tuned_on=torch.cuda.get_device_properties(self.device).gcnArchName)
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = path + f".{os.getpid()}.tmp"
            json.dump(saved, open(tmp, "w"))
            os.replace(tmp, path)
        except OSError:
            path = None                                # read-only home: tuned for this process only
        return "tuned", path, saved

    def apply_schedule(self, saved):
        """Tiles / stage kernel / residual-block mask from a schedule dict (`shipped_schedule`, `bench.py --save-tiles`).  The
        fusion switches themselves (stem, chains, stage, residual blocks) must already be on: a schedule only narrows them."""
        self.set_tiles(saved["tiles"])
        if self.dtype != "f32" and "stage_fusion" in saved and self.stage_fusion_active():
            self.set_stage_fusion(bool(saved["stage_fusion"]))
        if self.dtype != "f32" and "res_fusion_mask" in saved and self.res_fusion_mask():
            self.set_res_fusion_mask(int(saved["res_fusion_mask"]))

    def set_tiles(self, tiles):
        arr = (C.c_int32 * len(tiles))(*[int(t) for t in tiles])
        ext.check(self.lib.y4_set_tiles(self.handle, arr, len(tiles)))

    def set_splitk(self, on=True):
        """Latency schedules: let `autotune` also offer split-K tile ids (the K loop of a tile split over 2 / 4 / 8 workgroups; for
        small batches, where the deep layers have fewer tiles than the GPU has compute units).  A split launch adds its partial
        sums in another fp32 order than the unsplit loop, so the tuned schedule then is part of the numerical result; off by
        default, and the schedules that ship for batch 1 say so (`"splitk": true`)."""
        ext.check(self.lib.y4_set_splitk(self.handle, int(bool(on))))

    def set_halo2(self, on=True):
        """Let `autotune` also offer the halo2 tiles (conv_halo2_kernel.h: one wave per SIMD, v_mfma_32x32x16, weights in registers)
        for the 3x3 stride-1 convs.  They sum the K axis in another fixed fp32 order than the 16x16x32 tiles, so -- as with split-K --
        a schedule that holds them (`"halo2": true`) is part of the numerical result and is tested against the oracle."""
        ext.check(self.lib.y4_set_halo2(self.handle, int(bool(on))))
        self.halo2 = bool(on)

    def set_subbatch(self, images, last_conv=16):
        """Run convs 0..last_conv over `images` images at a time (Infinity-Cache residency of the big early
        activations); 0 turns it off.  Results are unchanged."""
        ext.check(self.lib.y4_set_subbatch(self.handle, int(images), int(last_conv)))

    def set_stem_fusion(self, on=True):
        """Convs 0+1 as one kernel with conv 0's output kept in LDS (16-bit dtypes, square img_size <= 640).  Results are
        unchanged; conv_output(0) is unavailable while on."""
        ext.check(self.lib.y4_set_stem_fusion(self.handle, int(bool(on))))
        self.stem_fusion = bool(on)

    def set_chain_fusion(self, on=True):
        """3x3+Add -> 1x1 (-> 1x1 over the concat) runs of the 64-channel CSP stages as one kernel each (16-bit
        dtypes).  Returns the number of fused runs.  A chained conv issues the same MFMAs on the same 16-bit inputs in the
        same order as its own kernel, so every materialised tensor, the heads and the detections are BIT-IDENTICAL to the
        unfused path (tests/test_gpu_forward.py::test_chain_fusion_is_bit_identical): a pure scheduling knob."""
        r = self.lib.y4_set_chain_fusion(self.handle, int(bool(on)))
        if r < 0:
            ext.check(r)
        return r

    def set_stage_fusion(self, on=True):
        """Convs 2..7 (the 304^2 CSP stage at 608) as one spatially tiled kernel (16-bit dtypes; bit-identical results).
        Returns whether the stage kernel is active; `autotune` afterwards keeps it only if it measures faster."""
        r = self.lib.y4_set_stage_fusion(self.handle, int(bool(on)))
        if r < 0:
            ext.check(r)
        return bool(r)

    def stage_fusion_active(self):
        r = self.lib.y4_get_stage_fusion(self.handle)
        if r < 0:
            ext.check(r)
        return bool(r)

    def set_res_fusion(self, on=True):
        """Residual blocks of the 64- / 128-channel stages (1x1 -> 3x3 + Add) as one spatially tiled kernel each (16-bit
        dtypes; bit-identical).  Returns the number of such blocks; `autotune` afterwards keeps them per channel group
        only where they measure faster (`res_fusion_mask`: bit 0 = 128 channels, bit 1 = 64 channels)."""
        r = self.lib.y4_set_res_fusion(self.handle, int(bool(on)))
        if r < 0:
            ext.check(r)
        return r

    def res_fusion_mask(self):
        r = self.lib.y4_get_res_fusion(self.handle)
        if r < 0:
            ext.check(r)
        return r

    def set_res_fusion_mask(self, mask):
        ext.check(self.lib.y4_set_res_fusion_mask(self.handle, int(mask)))

    def conv_launches_per_step(self):
        """Launches of the conv kernel family (everything but the stem) in one predict under the current settings."""
        convs, total = C.c_int32(), C.c_int32()
        ext.check(self.lib.y4_launch_counts(self.handle, C.byref(convs), C.byref(total)))
        return convs.value

    def timing_begin(self, max_steps, coarse=False):
        ext.check(self.lib.y4_timing_begin(self.handle, int(max_steps), int(bool(coarse))))

    def timing_end(self):
        """-> ([(op name, mean ms)], steps recorded); synchronises the current stream."""
        cap = 256
        ms = (C.c_float * cap)()
        names = C.create_string_buffer(16 * cap)
        nops, steps = C.c_int(), C.c_int()
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_timing_end(self.handle, ms, names, cap, C.byref(nops), C.byref(steps),
                                             ext.stream_ptr()))
        return self._op_times(names, ms, nops.value), steps.value

    @staticmethod
    def _op_times(names, ms, n):
        """[(op name, ms)] from the 16-byte name slots and the times y4_timing_end / y4_profile fill in."""
        raw = names.raw
        return [(raw[16 * i:16 * i + 16].split(b"\0")[0].decode(), float(ms[i])) for i in range(n)]

    def profile(self, imgs_dev):
        n = imgs_dev.shape[0]
        cap = 256
        ms = (C.c_float * cap)()
        names = C.create_string_buffer(16 * cap)
        nops = C.c_int()
        with self.torch.cuda.device(self.device):
            ext.check(self.lib.y4_profile(self.handle, ext.ptr(imgs_dev), n, ms, names, cap, C.byref(nops),
                                          ext.stream_ptr()))
        return self._op_times(names, ms, nops.value)


LOSS_WEIGHTS = (3.54, 64.3, 1.0)      # reference loss.py:136-138: box (GIoU), confidence, class


def combine_loss(parts):
    """[N, 3 scales, 3 terms] -> (loss, box, conf, class) per image, float64 [N] each, weighted as the reference does
    (loss.py:136-140); the reference's scalar is `loss.mean()`."""
    terms = np.asarray(parts, dtype=np.float64).sum(axis=1) * np.array(LOSS_WEIGHTS)
    return terms.sum(axis=1), terms[:, 0], terms[:, 1], terms[:, 2]


class InFlight:
    """`depth` batches in flight on one GPU: the engine and depth-1 siblings (shared packed weights, own activation
    workspaces), each on its own HIP stream, used round-robin.  A batch's kernels run in order on its stream; kernels of
    different batches overlap wherever one leaves compute units idle (partial last rounds of its tiles, the 32-workgroup
    NMS, the sub-one-round 19^2 layers).  Measured at 608x608 / 80 classes / batch 32 / bf16: 5.57 -> 5.03 ms per batch
    with two in flight (three: 5.11).  Outputs are bit-identical to the single-stream path (tests/test_gpu_api.py)."""

    def __init__(self, engine, depth=2):
        torch = engine.torch
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.engines = [engine] + [engine.sibling() for _ in range(depth - 1)]
        with torch.cuda.device(engine.device):
            self.streams = [torch.cuda.Stream(device=engine.device) for _ in range(depth)]
        self.torch, self.depth, self._next = torch, depth, 0

    def autotune(self, n=None, reps=3, passes=15):
        """Tune engine 0 and its first sibling TOGETHER, with two batches in flight as the objective of the decisions in
        `passes` (y4_autotune_pair), and copy the result to the other siblings.  Both engines need activations in their
        workspaces (one predict each)."""
        torch = self.torch
        if self.depth < 2:
            return self.engines[0].autotune(n, reps)
        torch.cuda.synchronize(self.engines[0].device)
        tiles = self.engines[0].autotune_pair(self.engines[1], self.streams[0], self.streams[1], n, reps, passes)
        torch.cuda.synchronize(self.engines[0].device)
        for e in self.engines[2:]:
            self.engines[0].copy_schedule_to(e)
        return tiles

    def submit(self, imgs_dev, outs, host=None, flat=None):
        """predict_device(imgs_dev, outs) on the next slot's stream (asynchronous); with `host` / `flat` the results are
        also copied to the pinned host tensor.  The caller owns per-slot inputs / outputs: slot = call index % depth."""
        k = self._next
        self._next = (k + 1) % self.depth
        with self.torch.cuda.stream(self.streams[k]):
            self.engines[k].predict_device(imgs_dev, outs)
            if host is not None:
                host.copy_(flat, non_blocking=True)
        return k

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def close(self):
        for e in self.engines[1:]:
            e.close()
