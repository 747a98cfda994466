"""ctypes binding of libyolo4hip.so (the C ABI declared in include/yolo4hip.h).

There is deliberately NO fallback: if the shared library is missing, or a call fails, this raises.
PyTorch is used only to own device memory (`torch.empty(..., device='cuda')`) and streams; every
pointer handed to the library is a `tensor.data_ptr()`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# YOLO4HIP_LIB lets kernel experiments (scripts/, scratch builds) load an alternative build of the SAME ABI
LIB_PATH = os.environ.get("YOLO4HIP_LIB") or os.path.join(_HERE, "libyolo4hip.so")

F32, BF16, F16 = 0, 1, 2
DTYPE_IDS = {"f32": F32, "fp32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16, "f16": F16, "fp16": F16,
             "float16": F16}
DTYPE_NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
ACT_LINEAR, ACT_LEAKY, ACT_MISH = 0, 1, 2


class Y4Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libyolo4hip error {code}: {msg}")
        self.code = code


class y4_config(C.Structure):
    _fields_ = [("img_size", C.c_int32), ("num_classes", C.c_int32), ("max_batch", C.c_int32),
                ("dtype", C.c_int32), ("anchors", C.c_float * 18), ("xyscale", C.c_float * 3),
                ("strides", C.c_int32 * 3), ("iou_threshold", C.c_float), ("score_threshold", C.c_float),
                ("max_per_class", C.c_int32), ("max_total", C.c_int32)]


class y4_layer_desc(C.Structure):
    _fields_ = [("idx", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("act", C.c_int32), ("has_bn", C.c_int32), ("in_side", C.c_int32),
                ("out_side", C.c_int32), ("weight_offset", C.c_int64)]


WS_ZERO, WS_ACT, WS_TAIL, WS_SCRATCH = 0, 1, 2, 3
WS_KIND_NAMES = {WS_ZERO: "zero", WS_ACT: "act", WS_TAIL: "tail", WS_SCRATCH: "scratch"}


class y4_workspace_row(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("kind", C.c_int32), ("buffer", C.c_int32), ("first_op", C.c_int32),
                ("last_op", C.c_int32), ("offset", C.c_uint64), ("bytes", C.c_uint64), ("image_bytes", C.c_uint64)]


class y4_conv_desc(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("cin", C.c_int32),
                ("cout", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32),
                ("upsample", C.c_int32), ("out_f32", C.c_int32), ("in_cstride", C.c_int32),
                ("in_coff", C.c_int32), ("out_cstride", C.c_int32), ("out_coff", C.c_int32),
                ("res_cstride", C.c_int32), ("res_coff", C.c_int32), ("in_", C.c_void_p), ("wt", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("res", C.c_void_p), ("out", C.c_void_p),
                ("tile", C.c_int32), ("out2", C.c_void_p), ("out2_cstride", C.c_int32), ("out2_coff", C.c_int32),
                ("split", C.c_int32), ("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_size_t), ("wt_frag", C.c_void_p)]


class y4_image_desc(C.Structure):
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("pad_top", C.c_int32), ("pad_left", C.c_int32)]


class y4_window_desc(C.Structure):
    _fields_ = [("offset", C.c_int64), ("pitch", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32)]


class y4_view_desc(C.Structure):
    _fields_ = y4_window_desc._fields_ + [("flip", C.c_int32), ("reserved", C.c_int32 * 2)]


class y4_augment_desc(C.Structure):
    _fields_ = y4_image_desc._fields_ + [("flip", C.c_int32), ("hue", C.c_float), ("sat", C.c_float), ("val", C.c_float)]


class y4_yuv_desc(C.Structure):
    _fields_ = [("y_offset", C.c_int64), ("u_offset", C.c_int64), ("v_offset", C.c_int64), ("y_pitch", C.c_int32),
                ("c_pitch", C.c_int32), ("c_step", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("out_h", C.c_int32),
                ("out_w", C.c_int32), ("pad_top", C.c_int32), ("pad_left", C.c_int32), ("flags", C.c_int32)]


class y4_mosaic_cut(C.Structure):
    _fields_ = [("cut_y", C.c_int32), ("cut_x", C.c_int32)]


# every symbol include/yolo4hip.h declares: name -> (restype, argtypes)
_VP, _I, _F = C.c_void_p, C.c_int, C.c_float
SYMBOLS = {
    "y4_last_error": (C.c_char_p, []),
    "y4_version": (C.c_char_p, []),
    "y4_create": (_I, [C.POINTER(y4_config), C.POINTER(_VP)]),
    "y4_create_hw": (_I, [C.POINTER(y4_config), C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "y4_input_dims": (_I, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "y4_layer_dims": (_I, [_VP, _I, C.POINTER(C.c_int32)]),
    "y4_destroy": (_I, [_VP]),
    "y4_num_layers": (_I, [_VP]),
    "y4_layer_info": (_I, [_VP, _I, C.POINTER(y4_layer_desc)]),
    "y4_model_info": (_I, [_VP, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                           C.POINTER(C.c_int64)]),
    "y4_workspace_bytes": (_I, [_VP, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "y4_bind_workspace": (_I, [_VP, _VP, C.c_size_t, _VP, C.c_size_t]),
    "y4_workspace_map": (_I, [_VP, C.POINTER(y4_workspace_row), _I, C.POINTER(_I)]),
    "y4_conv_output_view": (_I, [_VP, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "y4_pack_weights": (_I, [_VP, _VP, C.c_size_t, _VP]),
    "y4_adopt_packed_weights": (_I, [_VP]),
    "y4_forward": (_I, [_VP, _VP, _I, _VP]),
    "y4_forward_u8": (_I, [_VP, _VP, _I, _VP]),
    "y4_forward_until": (_I, [_VP, _VP, _I, _I, _VP]),
    "y4_get_heads": (_I, [_VP, _I, _VP, _VP, _VP, _VP]),
    "y4_set_heads": (_I, [_VP, _I, _VP, _VP, _VP, _VP]),
    "y4_get_conv_output": (_I, [_VP, _I, _I, _VP, C.c_size_t, _VP]),
    "y4_decode_nms": (_I, [_VP, _I, _F, _F, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_decode_nms_mapped": (_I, [_VP, _I, _F, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_decode_nms_merged": (_I, [_VP, _I, _F, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_loss_assign": (_I, [_VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "y4_loss_scratch_floats": (_I, [_VP, _I, C.POINTER(C.c_size_t)]),
    "y4_loss": (_I, [_VP, _I, _VP, _VP, _VP, _I, _F, _VP, C.c_size_t, _VP, _VP]),
    "y4_set_box_loss": (_I, [_VP, _I]),
    "y4_get_box_loss": (_I, [_VP]),
    "y4_set_nms_rule": (_I, [_VP, _I, C.c_float, _I]),
    "y4_get_nms_rule": (_I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "y4_set_nms_soft": (_I, [_VP, _I, C.c_float, C.c_float, _I]),
    "y4_get_nms_soft": (_I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "y4_set_nms_matrix": (_I, [_VP, _I, C.c_float, C.c_float, _I]),
    "y4_get_nms_matrix": (_I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "y4_set_retain_head_inputs": (_I, [_VP, _I]),
    "y4_loss_grad": (_I, [_VP, _I, _VP, _VP, _VP, _I, _F, _VP, _VP, _VP, _VP, _VP]),
    "y4_head_grad_scratch_floats": (_I, [_VP, _I, C.POINTER(C.c_size_t)]),
    "y4_head_grad": (_I, [_VP, _I, _VP, _VP, _VP, _I, _F, _VP, _VP, C.c_size_t, _VP, C.c_size_t, _I, _VP]),
    "y4_head_adam": (_I, [_VP, _VP, _VP, _VP, _VP, C.c_size_t, _F, _F, _F, _F, _I, _VP]),
    "y4_block_grad_scratch_bytes": (_I, [_VP, _I, C.POINTER(C.c_size_t)]),
    "y4_block_grad": (_I, [_VP, _I, _VP, _VP, _VP, _I, _F, _VP, _VP, C.c_size_t, _VP, C.c_size_t, _I, _VP]),
    "y4_block_grad_scaled": (_I, [_VP, _I, _VP, _VP, _VP, _I, _F, _VP, _F, _VP, _VP, C.c_size_t, _VP, C.c_size_t, _I, _VP]),
    "y4_block_adam": (_I, [_VP, _VP, _VP, _VP, _VP, C.c_size_t, _F, _F, _F, _F, _I, _VP]),
    "y4_feature_row_bytes": (_I, [_VP, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "y4_feature_store": (_I, [_VP, _I, C.POINTER(C.c_int64), _VP, C.c_size_t, _VP]),
    "y4_feature_load": (_I, [_VP, _I, C.POINTER(C.c_int64), _VP, C.c_size_t, _VP]),
    "y4_forward_tail": (_I, [_VP, _I, _VP]),
    "y4_predict": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_predict_u8": (_I, [_VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_profile": (_I, [_VP, _VP, _I, _VP, _VP, _I, C.POINTER(_I), _VP]),
    "y4_set_workspace_aliasing": (_I, [_VP, _I]),
    "y4_autotune": (_I, [_VP, _I, _I, _VP]),
    "y4_autotune_pair": (_I, [_VP, _VP, _I, _I, _VP, _VP, _I]),
    "y4_get_tiles": (_I, [_VP, C.POINTER(C.c_int32), _I]),
    "y4_set_tiles": (_I, [_VP, C.POINTER(C.c_int32), _I]),
    "y4_copy_schedule": (_I, [_VP, _VP]),
    "y4_set_subbatch": (_I, [_VP, _I, _I]),
    "y4_set_stem_fusion": (_I, [_VP, _I]),
    "y4_set_chain_fusion": (_I, [_VP, _I]),
    "y4_set_stage_fusion": (_I, [_VP, _I]),
    "y4_get_stage_fusion": (_I, [_VP]),
    "y4_set_res_fusion": (_I, [_VP, _I]),
    "y4_get_res_fusion": (_I, [_VP]),
    "y4_set_res_fusion_mask": (_I, [_VP, _I]),
    "y4_rb_tile_table": (_I, [_I, _I, _I, _I, _I, C.POINTER(C.c_int32), _I]),
    "y4_launch_counts": (_I, [_VP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "y4_timing_begin": (_I, [_VP, _I, _I]),
    "y4_timing_end": (_I, [_VP, _VP, _VP, _I, C.POINTER(_I), C.POINTER(_I), _VP]),
    "y4_packed_conv_bytes": (_I, [_I, _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "y4_pack_conv_weights": (_I, [_I, _I, _I, _I, _VP, _VP, _VP]),
    "y4_pack_conv_frag32": (_I, [_I, _I, _I, _VP, _VP, _VP]),
    "y4_conv2d": (_I, [C.POINTER(y4_conv_desc), _VP]),
    "y4_conv_tile_count": (_I, []),
    "y4_conv_tile_desc": (_I, [_I, C.POINTER(C.c_int32)]),
    "y4_set_splitk": (_I, [_VP, _I]),
    "y4_set_halo2": (_I, [_VP, _I]),
    "y4_pack_stem_weights": (_I, [_VP, _VP, _I, _VP]),
    "y4_stem_conv": (_I, [_I, _VP, _I, _I, _I, _VP, _VP, _VP, _I, _I, _VP, _I, _I, _VP]),
    "y4_preprocess_u8": (_I, [_VP, _I, _I, _VP, _I, _I, _VP]),
    "y4_resize_u8": (_I, [_VP, _I, _I, _I, _VP, _I, _I, _VP]),
    "y4_resize_u8_ragged": (_I, [_VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_window_u8_ragged": (_I, [_VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_view_u8_ragged": (_I, [_VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_gather_scratch_bytes": (_I, [_VP, _I, _I, C.c_uint32, C.POINTER(C.c_size_t)]),
    "y4_gather_begin": (_I, [_VP, _I, _I, C.c_uint32, _VP, _VP]),
    "y4_decode_gather": (_I, [_VP, _I, _F, _VP, _VP, _VP, _I, _I, C.c_uint32, _VP, _VP]),
    "y4_decode_gather_views": (_I, [_VP, _I, _F, _VP, _VP, _VP, _I, _I, C.c_uint32, _VP, _VP]),
    "y4_nms_gathered": (_I, [_VP, _I, _I, C.c_uint32, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_nms_gathered_merged": (_I, [_VP, _I, _I, C.c_uint32, _F, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "y4_augment_u8_ragged": (_I, [_VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_mosaic_u8_ragged": (_I, [_VP, _VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_yuv_u8_ragged": (_I, [_VP, _VP, _I, _VP, _I, _I, _I, _VP]),
    "y4_map_match": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _I, C.POINTER(C.c_double), _I, _VP, _VP, _VP, _VP, _VP]),
    "y4_coco_match": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _I, C.POINTER(C.c_double), _I, C.POINTER(C.c_double), _I, _VP, _VP,
                           _VP, _VP, _VP, _VP]),
    "y4_anchor_step": (_I, [_VP, _I, _VP, _I, _VP, _VP, _VP, _VP]),
    "y4_anchor_fitness": (_I, [_VP, _I, _VP, _I, _I, _VP, _VP]),
    "y4_anchor_evolve": (_I, [_VP, _I, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP]),
    "y4_spp": (_I, [_I, _VP, _I, _I, _I, _VP]),
    "y4_spp_hw": (_I, [_I, _VP, _I, _I, _I, _I, _VP]),
}

_lib = None


def load():
    """dlopen the in-tree library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                              f"(or yolo-v4-tf.keras_amd/csrc/build.sh); there is no CPU fallback")
        # torch first: PyTorch-ROCm bundles its own libamdhip64; if this library were loaded before it, the process would
        # hold two HIP runtimes (the system one pulled in here, torch's later) and the one this library talks to then
        # reports "no ROCm-capable device" while torch.cuda works -- seen when build() and smoke() share a process
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)          # AttributeError if the .so does not export it
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def workspace_map(lib, handle):
    """y4_workspace_map as a list of dicts in the library's order (sorted by offset): name, kind ('zero' | 'act' | 'tail' |
    'scratch'), buffer, first_op, last_op, offset, bytes, image_bytes.  Host-only: works on a handle with no workspace bound."""
    count = C.c_int()
    check(lib.y4_workspace_map(handle, None, 0, C.byref(count)))
    rows = (y4_workspace_row * count.value)()
    check(lib.y4_workspace_map(handle, rows, count.value, C.byref(count)))
    return [dict(name=r.name.decode(), kind=WS_KIND_NAMES[r.kind], buffer=r.buffer, first_op=r.first_op, last_op=r.last_op,
                 offset=int(r.offset), bytes=int(r.bytes), image_bytes=int(r.image_bytes)) for r in rows]


def conv_output_view(lib, handle, conv_idx):
    """y4_conv_output_view -> (row index in `workspace_map`, channel offset, channel stride, materialised) of conv `conv_idx`'s
    output; materialised: does a forward under the current fusion switches write it?"""
    row, coff, cstride, stored = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.y4_conv_output_view(handle, conv_idx, C.byref(row), C.byref(coff), C.byref(cstride), C.byref(stored)))
    return row.value, coff.value, cstride.value, bool(stored.value)


def check(rc):
    if rc != 0:
        raise Y4Error(rc, load().y4_last_error().decode("utf-8", "replace"))
    return rc


def stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
