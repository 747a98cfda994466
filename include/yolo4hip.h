/* yolo4hip.h -- C ABI of libyolo4hip.so: the MI355X (gfx950) YOLOv4 inference hot path.
 *
 * The reference (taipingeric/yolo-v4-tf.keras) has no FFI: its hot path is the tf.keras graph executed by
 * `Model.predict` (reference models.py:113,159,514).  This ABI is the seam a host binds instead of
 * TensorFlow; each entry point cites the reference code it stands in for.  See INTEGRATION.md for the
 * ctypes binding that `yolo-v4-tf.keras_amd/yolo4hip/ext.py` uses.
 *
 * Conventions
 *   - every function returns 0 on success or a negative Y4_E* code; `y4_last_error()` gives the text
 *     (thread-local).  Nothing throws, nothing aborts.
 *   - all `*_dev` / workspace pointers are DEVICE pointers owned by the caller (the Python host owns them
 *     as torch-ROCm tensors).  A handle never allocates device memory: scratch comes out of the bound
 *     workspace.  (Only the standalone y4_conv2d lazily allocates one 256-byte zero page per process.)
 *   - every launch goes on the caller's `stream` (a hipStream_t passed as void*; NULL = default stream).
 *     Calls are asynchronous; the caller synchronises.  All calls on ONE handle must be enqueued in stream order (on one
 *     stream, or on streams the caller orders with events): a handle keeps host-side notes of what its workspace holds
 *     (which head wrote the objectness side array for how many images, whether the decode counters are clean) that are
 *     updated when a call is ENQUEUED, after its launches succeeded -- not when it completes.
 *   - activations are NHWC.  Images are float32 [n, H, W, 3] in [0,1] (what `Yolov4.preprocess_img`
 *     produces, reference models.py:95-98, after Keras' cast to float32).
 *   - one handle per process/GPU; a handle is not re-entrant.
 */
#ifndef YOLO4HIP_H
#define YOLO4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y4_OK 0
#define Y4_EINVAL (-22)      /* bad argument / unsupported shape */
#define Y4_ENOMEM (-12)      /* bound workspace too small */
#define Y4_ESTATE (-1)       /* call order (workspace not bound, weights not packed) */
#define Y4_EHIP (-5)         /* a HIP runtime call failed */

#define Y4_F32 0
#define Y4_BF16 1
#define Y4_F16 2

#define Y4_ACT_LINEAR 0
#define Y4_ACT_LEAKY 1       /* LeakyReLU(alpha=0.1), reference custom_layers.py:29-30 */
#define Y4_ACT_MISH 2        /* x*tanh(softplus(x)),  reference custom_layers.py:6-7  */

typedef struct y4_ctx* y4_handle;

/* Mirrors what `Yolov4.__init__` reads from `yolo_config` (reference models.py:26-37, config.py:1-17). */
typedef struct y4_config {
    int32_t img_size;          /* square input side, multiple of 32 (reference models.py:23-24); y4_create_hw takes H and W instead */
    int32_t num_classes;       /* len(class_names) (reference models.py:25,27) */
    int32_t max_batch;         /* largest n any call will pass */
    int32_t dtype;             /* Y4_F32 | Y4_BF16 | Y4_F16: storage/MFMA-input type; accumulation is fp32 */
    float anchors[18];         /* 3 scales x 3 anchors x (w,h) px at input resolution (config.py:4, models.py:29) */
    float xyscale[3];          /* config.py:6 */
    int32_t strides[3];        /* config.py:5 */
    float iou_threshold;       /* config.py:15 */
    float score_threshold;     /* config.py:16 */
    int32_t max_per_class;     /* 100: custom_layers.py:293 */
    int32_t max_total;         /* 100: custom_layers.py:294 */
} y4_config;

/* One row of the 110-conv plan, as built by the C++ runtime. */
typedef struct y4_layer_desc {
    int32_t idx, ksize, stride, cin, cout, act, has_bn, in_side, out_side;   /* sides: -1 on a non-square handle (y4_layer_dims) */
    int64_t weight_offset;     /* float offset of this layer's record in the Darknet stream (bn/bias first) */
} y4_layer_desc;

const char* y4_last_error(void);
const char* y4_version(void);

/* Replaces Yolov4.__init__ -> build_model (inference half), reference models.py:18-52,67-73: builds the
 * 110-conv CSPDarknet53+SPP+PANet plan, the decode and the NMS stages for this config.  Host-only. */
int y4_create(const y4_config* cfg, y4_handle* out);
/* Rectangular input: images are [n, img_h, img_w, 3] (the Keras Input shape, height first), each side a positive multiple of 32;
 * cfg->img_size is not read.  Scale s has gh = img_h / stride rows and gw = img_w / stride columns, raw heads are
 * [n, gh, gw, 3*(C+5)], cells row-major (row over H, column over W), and num_boxes = 3 * sum(gh * gw).  Boxes are normalised
 * x / img_w, y / img_h (the reference divides all four coordinates by input_shape[0], custom_layers.py:284: the same float32
 * division for a square input, so y4_create(cfg) == y4_create_hw(cfg, cfg->img_size, cfg->img_size) bit for bit).  Stem fusion
 * (y4_set_stem_fusion) is square-only; every other kernel and knob takes either shape. */
int y4_create_hw(const y4_config* cfg, int32_t img_h, int32_t img_w, y4_handle* out);
/* The handle's input rows / columns. */
int y4_input_dims(y4_handle h, int32_t* img_h, int32_t* img_w);
/* dims = {in_h, in_w, out_h, out_w} of layer `idx` (the stored tensor for the upsampling convs 78 / 85 is 2 out_h x 2 out_w). */
int y4_layer_dims(y4_handle h, int idx, int32_t dims[4]);
int y4_destroy(y4_handle h);

int y4_num_layers(y4_handle h);
int y4_layer_info(y4_handle h, int idx, y4_layer_desc* out);
/* per image: conv FLOPs (2*k*k*cin*cout*ho*wo summed), decoded boxes, padded channel count of a raw head */
int y4_model_info(y4_handle h, int64_t* flops_per_image, int32_t* num_boxes, int32_t* head_cstride,
                  int64_t* weight_floats);

/* Optional, BEFORE y4_workspace_bytes / y4_bind_workspace: let activation buffers whose lifetimes do not overlap share memory
 * (liveness over the op order, every fusable group of ops counted as one instant).  The activation workspace shrinks to about a
 * quarter and the working set the Infinity Cache sees becomes hotter; the price: intermediate tensors are not retained after a
 * forward (y4_get_conv_output then returns Y4_ESTATE) and sub-batching is refused.  Results are unchanged.  (Stands where
 * TensorFlow's memory planner stands in the reference; not in tree.) */
int y4_set_workspace_aliasing(y4_handle h, int on);
/* Device memory the caller must provide: `act` = activations + decode/NMS scratch for max_batch images,
 * `wts` = packed weights (+ per-channel scale/shift). */
int y4_workspace_bytes(y4_handle h, size_t* act_bytes, size_t* wts_bytes);
int y4_bind_workspace(y4_handle h, void* act_dev, size_t act_bytes, void* wts_dev, size_t wts_bytes);

/* A read-only map of the `act` workspace under the handle's current layout (aliasing, retention): one row per region, sorted by
 * offset; the rows cover [0, act_bytes) up to alignment gaps of at most 255 bytes.  Host-only, valid before the workspace is bound.
 *   Y4_WS_ZERO     the library keeps these bytes zero between calls: the zero page (never written), the candidate counters (the NMS
 *                  kernel of a list resets its counter; a decode not followed by its NMS makes the next decode clear them), the NMS
 *                  status word (only ever OR-ed, on a list overflow that the worst-case capacity rules out; nothing resets it),
 *                  the split-K tile counters (the last workgroup to arrive at a tile resets its counter)
 *   Y4_WS_ACT      one activation buffer, [max_batch] images of image_bytes each; first_op / last_op: its lifetime in op-index time as
 *                  the aliasing layout reads it (ACT rows share bytes under y4_set_workspace_aliasing, and only then)
 *   Y4_WS_TAIL     state of the detection tail: decoded boxes, candidate keys, the objectness side array (per image), and the
 *                  output scratch of y4_profile (image_bytes 0: packed for the n of the call)
 *   Y4_WS_SCRATCH  meaningless between calls: the split-K partial sums
 * Every region but the ZERO ones may hold anything when a call begins: no result depends on it. */
#define Y4_WS_ZERO 0
#define Y4_WS_ACT 1
#define Y4_WS_TAIL 2
#define Y4_WS_SCRATCH 3
typedef struct y4_workspace_row {
    char name[24];
    int32_t kind;              /* Y4_WS_* */
    int32_t buffer;            /* ACT: the buffer's number in the plan (row name "act<buffer>"); else -1 */
    int32_t first_op, last_op; /* ACT: lifetime, op indices (last_op = the op count: outlives the forward); else -1 */
    uint64_t offset, bytes;    /* bytes: what the region holds for max_batch images, without alignment slack */
    uint64_t image_bytes;      /* bytes == max_batch * image_bytes where the region is per image, else 0 */
} y4_workspace_row;                                  /* 64 bytes */
/* Writes min(capacity, count) rows and the row count (rows_out may be NULL with capacity 0). */
int y4_workspace_map(y4_handle h, y4_workspace_row* rows_out, int capacity, int* count_out);
/* Where conv `conv_idx` stores its output: the index of its ACT row in y4_workspace_map's order, and the channel offset and
 * channel stride (elements) of its view in that buffer's NHWC pixels -- what y4_get_conv_output reads.  materialised (may be NULL):
 * 1 when a forward under the current fusion switches writes that view, 0 while a fused kernel keeps the tensor on chip -- conv 0
 * under stem fusion, convs 2 .. 6 under the stage kernel, the 1x1 conv of a residual-block kernel, and inside a run that executes
 * as one kernel everything but its last conv and a head whose output has other readers.  y4_get_conv_output refuses the first
 * three; for a conv inside a run it copies the view as it is, i.e. what an earlier call left there.  Host-only. */
int y4_conv_output_view(y4_handle h, int conv_idx, int32_t* row, int32_t* channel_offset, int32_t* channel_stride,
                        int32_t* materialised);

/* Replaces utils.load_weights (reference utils.py:12-53) + Keras set_weights: `darknet_floats_dev` is the
 * float32 stream of a Darknet .weights file after its 20-byte header, already on the device: for conv
 * 0..109, [beta,gamma,mean,var] x cout (or cout biases for convs 93/101/109), then cout*cin*k*k weights in
 * (out,in,h,w) order.  Computes scale = gamma*rsqrt(var+1e-3), shift = beta-mean*scale (Keras BN eps) and
 * re-lays every kernel along the library's canonical K order -- [cout_pad][cin/KC][kh*kw][KC], KC = min(cin, 64) for 3x3 and cin for 1x1
 * kernels: 64-channel chunk, then tap, then channel -- in the handle's dtype inside the bound `wts` workspace. */
int y4_pack_weights(y4_handle h, const float* darknet_floats_dev, size_t n_floats, void* stream);
/* Multi-GPU: after rank 0 packed and the caller broadcast the whole `wts` workspace (RCCL), the other
 * ranks mark their copy as valid. */
int y4_adopt_packed_weights(y4_handle h);

/* Replaces yolo_model.predict(imgs) (reference models.py:50-52,514; graph custom_layers.py:100-198).
 * Raw heads stay inside the workspace (padded to head_cstride channels). */
int y4_forward(y4_handle h, const float* imgs_nhwc_dev, int n, void* stream);
/* The same on uint8 frames [n, H, W, 3] ALREADY at network size, BEFORE the `/ 255.` of Yolov4.preprocess_img (reference
 * models.py:95-98): the stem applies it inside its operand load, so no float image tensor exists and the frames cross
 * PCIe / HBM at 3 B per pixel.  Bit-identical to y4_forward on float32(double(v) / 255.) for every dtype.
 * Frames of another size go through y4_resize_u8 (cv2.resize's uint8 INTER_LINEAR arithmetic) first. */
int y4_forward_u8(y4_handle h, const uint8_t* imgs_nhwc_u8_dev, int n, void* stream);
/* y4_forward cut behind conv `last_conv` (0-based, the reference's creation order): the ops up to and including the launch
 * that computes it.  last_conv = 71 is `cspdarknet53` proper -- the five CSP stages, reference custom_layers.py:100-124, before the
 * SPP block's convs -- which bench.py times on its own (`backbone` in its line).  Y4_EINVAL when the conv does not end a launch
 * under the current fusion settings (a run that continues behind it is never cut). */
int y4_forward_until(y4_handle h, const float* imgs_nhwc_dev, int n, int last_conv, void* stream);
/* Dense float32 copies of the three raw heads, [n,gh,gw,3*(C+5)] each, as Keras returns them. */
int y4_get_heads(y4_handle h, int n, float* out_s_dev, float* out_m_dev, float* out_l_dev, void* stream);
/* Inverse of y4_get_heads: load dense float32 raw heads [n,gh,gw,3*(C+5)] into the workspace, so that
 * y4_decode_nms can be driven with arbitrary logits (decode/NMS known-answer tests; reference
 * predict_nonms feeds yolov4_head/nms with precomputed heads the same way, models.py:521-523). */
int y4_set_heads(y4_handle h, int n, const float* in_s_dev, const float* in_m_dev, const float* in_l_dev,
                 void* stream);
/* Debug/parity tap: dense float32 NHWC copy of conv `idx`'s output tensor (post BN/activation/residual;
 * for convs that write a concat slice, that slice). */
int y4_get_conv_output(y4_handle h, int conv_idx, int n, float* out_dev, size_t out_floats, void* stream);

/* Replaces yolov4_head/get_boxes + nms (reference custom_layers.py:201-298, i.e.
 * tf.image.combined_non_max_suppression) on the heads left by y4_forward.
 * boxes [n,max_total,4] (x1/W, y1/H, x2/W, y2/H, clipped to [0,1], zero padded; W = H = img_size when square), scores [n,max_total],
 * classes [n,max_total] (class id as float), valid [n] int32, kept_idx [n,max_total] int32 (box index
 * n = scale_offset + (row*gw+col)*3 + anchor, -1 padded; may be NULL).  iou/score thresholds < 0 mean
 * "use the config's" (predict_nonms passes its own, reference models.py:516-523). */
int y4_decode_nms(y4_handle h, int n, float iou_threshold, float score_threshold, float* boxes_dev,
                  float* scores_dev, float* classes_dev, int32_t* valid_dev, int32_t* kept_idx_dev,
                  void* stream);
/* y4_decode_nms with the boxes mapped back to each SOURCE image (letterbox input, see y4_resize_u8_ragged).  The reference
 * normalises boxes by the network input (custom_layers.py:284) and clips them to [0,1] (:297, clip_boxes=True); here each kept
 * box of image i is first mapped with box_map_dev[i] = {ax, bx, ay, by}: x1, x2 -> fmaf(x, ax, bx), y1, y2 -> fmaf(y, ay, by),
 * and then clipped to [0,1] -- to the image, not to the canvas.  The kept set, scores, classes, valid and kept_idx are those of
 * y4_decode_nms bit for bit (the map applies in the output stage, after NMS); box_map_dev == NULL is y4_decode_nms exactly.
 * Same handle-state rules (candidate counters, head notes, stream order) as y4_decode_nms.  Stretch input (reference
 * models.py:95-98) has the identity map {1, 0, 1, 0}. */
int y4_decode_nms_mapped(y4_handle h, int n, float iou_threshold, float score_threshold, const float* box_map_dev,
                         float* boxes_dev, float* scores_dev, float* classes_dev, int32_t* valid_dev, int32_t* kept_idx_dev,
                         void* stream);
/* The pair rule of the NMS stage: which earlier kept boxes a candidate is tested against, and with which measure.  Candidates are
 * visited in the order y4_decode_nms defines (score descending, then box index, then class); a candidate is kept unless an earlier
 * KEPT candidate -- of its own class (agnostic 0), of any class (agnostic 1) -- has a measure m with m > iou_threshold (strict):
 *     kind 0 (IoU, the default: tf.image.combined_non_max_suppression):   m = iou
 *     kind 1 (DIoU-NMS: Zheng et al. 2020, Darknet nms_kind=diounms with beta_nms = beta):
 *         iou = as for kind 0: corners min / max-normalised per axis, 0 if either area <= 0
 *         d2  = (cya - cyb)^2 + (cxa - cxb)^2          centres = 0.5 * (lo + hi) of the normalised corners
 *         c2  = (max(hi) - min(lo))_y^2 + (..)_x^2     squared diagonal of the enclosing box
 *         m   = c2 == 0 ? iou : iou - pow(d2 / c2, beta)          (beta == 1: the plain quotient, no pow)
 * all in float32 in this operation order, on the normalised canvas boxes (x / W, y / H) before the clip and before the box map of
 * y4_decode_nms_mapped -- where the IoU is computed.  On a rectangular canvas the centre distance is therefore in x / W and y / H
 * units, as in Darknet.  m <= iou: kind 1 keeps a superset of what kind 0 keeps among two boxes.
 * max_per_class counts per class under both settings of agnostic, and a candidate its class's cap turns away is not kept and
 * suppresses nothing; max_total is unchanged; with agnostic 1 the up to num_classes candidates of one box collapse to its best class.
 * Outputs keep their form.  Host-only state, settable at any time, no effect on the workspace, not a scheduling choice
 * (y4_copy_schedule does not carry it) and not in a checkpoint.  Read at the call by y4_decode_nms, y4_decode_nms_mapped, the
 * y4_predict* entry points, y4_nms_gathered and the merged forms of these (y4_decode_nms_merged, y4_nms_gathered_merged).  Y4_EINVAL for a kind other than 0 / 1, an agnostic other than 0 / 1, and a beta that is not finite or
 * is <= 0 (beta is validated also for kind 0, which ignores it).  Default (0, 1.0, 0): every entry point returns the bits it
 * returned before this call existed. */
int y4_set_nms_rule(y4_handle h, int kind, float beta, int agnostic);
int y4_get_nms_rule(y4_handle h, int* kind, float* beta, int* agnostic);
/* Soft-NMS (Bodla et al. 2017): a kept box multiplies the scores of its neighbours by a factor below 1 instead of deleting them; the
 * next box to keep is the maximum of the CURRENT scores.  method 0 (the default) is off: every entry point runs the NMS kernel it
 * ran before this call existed, bit for bit.  With method 1 / 2 / 3 every entry point that reads y4_set_nms_rule (see there; the
 * merged forms included) runs this rule instead, per candidate list (an image's, or a gathered group's), on the same keys and
 * unclipped boxes, under the same pair rule (kind, beta, agnostic), max_total, max_per_class and the call's iou_threshold:
 *   1. Participants P: the top_k largest keys of the list (score descending, then box index, then class), or all when the list
 *      is shorter.  Candidates outside P take no part -- a defined pre-NMS top-k, not an error: no status bit.  top_k <= 4096.
 *   2. Working scores w_j = s_j.
 *   3. While fewer than max_total boxes are kept: among the j of P that are neither kept nor turned away and have w_j > min_score
 *      (strict), take k with the largest key (w_j, then box index ascending, then class ascending); none: stop.
 *   4. If k's class already has max_per_class kept boxes, k is turned away: not kept, decays nothing.
 *   5. Otherwise k is kept with OUTPUT SCORE w_k, and for every other live j of k's class (of every class under agnostic 1), with
 *      m = the measure of y4_set_nms_rule of (B_j, B_k) in float32 (for kind 1 the penalty applies to every pair),
 *          method 1, gaussian:  w_j *= m > 0 ? expf(-(m * m) / sigma) : 1       (a NaN or negative measure decays nothing)
 *          method 2, linear:    w_j *= m > iou_threshold ? 1 - m : 1            (strict)
 *          method 3, hard:      w_j *= m > iou_threshold ? 0 : 1
 *      one float32 rounding per kept neighbour, in pick order.
 * Outputs keep their form: boxes through the box map and the clip, scores = w at the pick (non-increasing), classes, valid,
 * kept_idx, zero / -1 padded; the list's counter is reset and the overflow status bit set as by the NMS kernel.  Method 3 with
 * every list no longer than top_k returns the bits of method 0.  The same call gives the same bits (picks are by unique key; no
 * floating-point atomics).  The merged entry points run the merge behind it unchanged -- members are decided on the original boxes
 * and weighted with the original scores -- so only the boxes move.
 * min_score < 0: the config's score_threshold (the convention of iou_threshold < 0); a run-time score threshold of a call does not
 * change it.  Host-only state like y4_set_nms_rule: settable at any time, no effect on the workspace, not carried by
 * y4_copy_schedule, not in a checkpoint.  Y4_EINVAL, with nothing changed: a method outside 0 .. 3; sigma not finite or <= 0
 * (validated for every method); min_score NaN, infinite or >= 1; top_k outside 1 .. 4096; a null getter argument.  A call whose
 * (top_k, max_total, num_classes) needs more than 160 KB of LDS fails with Y4_EINVAL at the launch.  Default (0, 0.5, -1, 4096). */
int y4_set_nms_soft(y4_handle h, int method /* 0 off, 1 gaussian, 2 linear, 3 hard */, float sigma, float min_score, int top_k);
int y4_get_nms_soft(y4_handle h, int* method, float* sigma, float* min_score, int* top_k);
/* Matrix-NMS (Wang et al., SOLOv2, 2020): score decay like Soft-NMS, but every decayed score is a closed-form function of the pair
 * measures and the ORIGINAL score order -- no pick sequence.  method 0 (the default) is off: every entry point runs what it ran
 * before this call existed, bit for bit.  With method 1 / 2 every entry point that reads y4_set_nms_rule (the merged and gathered
 * forms included) runs this rule instead, per candidate list (an image's, or a gathered group's), on the same keys and unclipped
 * boxes, under the same pair rule (kind, beta, agnostic), max_total and max_per_class:
 *   1. Participants P: the top_k largest keys of the list, or all when the list is shorter (the select of y4_set_nms_soft: a
 *      defined pre-NMS top-k, no status bit).  top_k <= 4096.
 *   2. Order: by key, largest first (score descending, then box index ascending, then class ascending); i < j: i comes earlier.
 *      i and j interact iff they have the same class (always under agnostic 1).
 *   3. Pair measure: m_ij = the measure of y4_set_nms_rule of (B_i, B_j) in float32 (for kind 1 the penalty applies to every pair);
 *      only its positive part counts, m+ = m > 0 ? m : 0, so a NaN or negative measure decays nothing.
 *   4. Compensation: c_i = the maximum of m+_ki over the interacting k < i; 0 without such a k.
 *   5. Decay: d_j = the minimum of t_ij over the interacting i < j; 1 without such an i.
 *          method 1, gaussian:  t_ij = expf((c_i * c_i - m+_ij * m+_ij) / sigma)
 *          method 2, linear:    t_ij = (1 - m+_ij) / (1 - c_i) where c_i < 1; a term with c_i >= 1 is left out
 *      every product, difference, quotient and expf rounds once, in float32.
 *   6. Output score w_j = s_j * d_j, one rounding.  The call's iou_threshold plays no part in the decay (the merged entry points
 *      still decide with it which candidates a kept box absorbs).
 *   7. Result: the candidates with w_j > min_score (strict) are walked by key (w_j, then box index ascending, then class ascending),
 *      largest first; one whose class already holds max_per_class boxes is skipped (it has decayed the others all the same: decay
 *      is one-shot); the walk stops at max_total boxes.
 * Outputs keep their form: boxes through the box map and the clip, scores = w (non-increasing), classes, valid, kept_idx, zero / -1
 * padded; the list's counter is reset and the overflow status bit set as by the NMS kernel.  The same call gives the same bits
 * whatever order the list was written in (no floating-point atomics).  On a class of two candidates gaussian equals method 1 of
 * y4_set_nms_soft bit for bit (c = 0, and 0 * 0 - x is -x exactly).
 * min_score < 0: the config's score_threshold; a run-time score threshold of a call does not change it.  Host-only state like
 * y4_set_nms_soft: settable at any time, not carried by y4_copy_schedule, not in a checkpoint.  The two decay modes exclude each
 * other: Y4_EINVAL for method != 0 here while y4_set_nms_soft's method is != 0, and for y4_set_nms_soft(method != 0) while this
 * method is != 0.  Y4_EINVAL, with nothing changed, also for: a method outside 0 .. 2; sigma not finite or <= 0 (validated for every
 * method); min_score NaN, infinite or >= 1; top_k outside 1 .. 4096; a null getter argument.  A call whose (max_total, num_classes)
 * needs more than 160 KB of LDS fails with Y4_EINVAL at the launch.  Default (0, 0.5, -1, 4096). */
int y4_set_nms_matrix(y4_handle h, int method /* 0 off, 1 gaussian, 2 linear */, float sigma, float min_score, int top_k);
int y4_get_nms_matrix(y4_handle h, int* method, float* sigma, float* min_score, int* top_k);
/* ---- Gathered decode + NMS: ONE NMS over the candidates of several batch rows (tiled inference: the rows are windows of one
 * photo, see y4_window_u8_ragged).  Row i belongs to group g = row_group_dev[i] (a photo), has slot t = row_slot_dev[i] in it
 * (0 <= t < max_slots, distinct among a group's rows) and the map m = row_map_dev[i] = {ax, bx, ay, by} from its canvas-normalised
 * coordinates to the group's normalised coordinates.
 *
 * Scratch is the caller's (y4_gather_scratch_bytes; 256-byte aligned), per group: a list of group_cap 64-bit candidate keys, a box
 * table [max_slots * nbox][4] float32 and one counter on a 256-byte line of its own.  The sequence is
 *     y4_gather_begin                      zeroes the group counters (one small async memset)
 *     y4_decode_gather  (any number)       after a y4_forward* / y4_set_heads of n rows: runs the decode stage of y4_decode_nms on rows
 *                                          0 .. n-1 of the handle and merges every candidate (box b, class c, score s) of row i into
 *                                          group g's list with the id (t * nbox + b) * C + c, its box mapped with m -- x1, x2 ->
 *                                          fmaf(x, ax, bx), y1, y2 -> fmaf(y, ay, by), unclipped -- into the group's table.  A
 *                                          group's rows may lie in different calls (forward chunks).
 *     y4_nms_gathered                      cand_count_dev[g] = the candidates group g received; then the NMS kernel of y4_decode_nms
 *                                          over the n_groups lists, under the handle's y4_set_nms_rule, max_total and
 *                                          max_per_class.  iou_threshold < 0: the config's.
 * all on one stream, in this order.  Consequences:
 *   - candidates are visited by score descending, then slot, then box index, then class;
 *   - the map applies BEFORE the pair measure: IoU / DIoU are taken in the group's (the photo's) normalised coordinates.
 *     y4_decode_nms_mapped is the opposite: it maps in the output stage, after the decisions;
 *   - outputs have the form of y4_decode_nms for n_groups images, boxes clipped to [0,1] of the group; kept_idx is
 *     slot * nbox + box (-1 padded; may be NULL);
 *   - the order in which candidates arrive in a list varies from run to run; keys are unique and the NMS sorts them, so the outputs
 *     are the same bits on every run.
 * CAPACITY: a group that received more than group_cap candidates has lost the excess (which ones is not defined): cand_count_dev[g]
 * > group_cap tells the caller, who must not use that group's result; the outputs are still written and nothing is accessed out of
 * range.  group_cap is a capacity to choose, not a measurement: max_slots * nbox * C can never overflow.
 * Handle state: y4_decode_gather leaves the candidate counters of its n rows at zero, as the NMS stage of y4_decode_nms does, so
 * plain y4_decode_nms calls and gathered sequences may alternate on one handle.  The row tables live on the device; a row whose
 * group or slot is out of range contributes nothing; the caller owns everything else about them.
 * Y4_EINVAL before any launch: n_groups, max_slots or group_cap < 1; max_slots * nbox * C >= 2^31 (the ids a key holds); a null
 * pointer; scratch not 256-byte aligned; n outside [1, max_batch]. */
int y4_gather_scratch_bytes(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, size_t* bytes);
int y4_gather_begin(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev, void* stream);
int y4_decode_gather(y4_handle h, int n, float score_threshold, const int32_t* row_group_dev, const int32_t* row_slot_dev,
                     const float* row_map_dev /* [n][4] */, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev,
                     void* stream);
int y4_nms_gathered(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, float iou_threshold, void* scratch_dev,
                    int32_t* cand_count_dev /* [n_groups] */, float* boxes_dev, float* scores_dev, float* classes_dev,
                    int32_t* valid_dev, int32_t* kept_idx_dev, void* stream);
/* y4_decode_gather for rows whose map may MIRROR (test-time augmentation: a row is a flipped view of its photo, see
 * y4_view_u8_ragged): the same arguments, sequence, ids, capacity, status and handle-state rules as y4_decode_gather, and calls of
 * both may feed one group.  The only difference is which corner an axis reads when its scale is negative:
 *     x1' = fmaf(ax < 0 ? x2 : x1, ax, bx),   x2' = fmaf(ax < 0 ? x1 : x2, ax, bx),   and the same for y with ay.
 * fmaf is monotone, so a decoded box with x1 <= x2 is stored with x1' <= x2' (y alike) under every sign of the scale -- what
 * the pair measure of y4_nms_gathered and the componentwise mean of y4_nms_gathered_merged (no corner normalisation) take for
 * granted.  With ax >= 0 and ay >= 0 it stores the bits y4_decode_gather stores.  Same call, same bits. */
int y4_decode_gather_views(y4_handle h, int n, float score_threshold, const int32_t* row_group_dev, const int32_t* row_slot_dev,
                           const float* row_map_dev /* [n][4] */, int n_groups, int max_slots, uint32_t group_cap, void* scratch_dev,
                           void* stream);
/* ---- Merge-NMS (box voting; YOLOv5's merge=True, the box step of weighted box fusion): y4_decode_nms_mapped / y4_nms_gathered
 * followed by one more kernel that replaces each kept box by the score-weighted mean of the candidates it absorbed.  The kept set,
 * its order, scores, classes, valid and kept_idx are those of the plain entry point bit for bit; only the four floats of each kept
 * box change.  No handle state: the plain entry points are untouched, and these read the handle's y4_set_nms_rule as they do.
 *
 * For a kept box k with unclipped box B_k, class c_k and candidate id, in the coordinates where the pair measure is taken (the
 * canvas-normalised boxes before the clip and the box map; for a gathered group the group-normalised boxes behind the row map),
 * a candidate j of the list is a MEMBER when
 *     class_j == c_k (any class when the rule is agnostic)   and   m(B_j, B_k) > iou_threshold
 * with m the measure of y4_set_nms_rule: the same float32 function, operation order and strict comparison that suppresses.
 * Candidate k itself is a member by its id.  The list is every key below min(count, capacity), also the candidates the NMS never
 * visited because it had its max_total boxes, and those a cap turned away.  A candidate with a component that is not finite or of
 * magnitude above 2^8 is never a member; a kept box with such a component is written as the plain entry point writes it.
 * Accumulation is in integers, so the result does not depend on the order of the list (which varies from run to run):
 *     wq_j = llrint((double)score_j * 2^30),   t_j[c] = llrint((double)score_j * (double)B_j[c] * 2^30)    (nearest even)
 *     S_w = sum wq_j,  S[c] = sum t_j[c]  in int64;     B'_k[c] = (float)((double)S[c] / (double)S_w)      (S_w == 0: B_k stays)
 * componentwise on the four stored floats (no corner normalisation); then the box map (fmaf) and the clip to [0,1], as before.
 * A member's rounding is at most 2^-31 in numerator and denominator: B' lies within 2^-31 (1 + |mean|) / s_min of the float64
 * weighted mean (s_min the smallest member score), plus one float32 rounding.
 * cand_count_dev [n] / [n_groups] is an output: the lists' raw candidate counts (the merge reads them; the counters themselves
 * are zeroed by the NMS kernel).  kept_idx_dev is required.  A gathered group with more than group_cap candidates is reported
 * through cand_count_dev as by y4_nms_gathered and merged over its first group_cap keys; the caller discards its result.
 * Y4_EINVAL before any launch: a null output; a list capacity (nbox * C, or group_cap) of 2^25 keys or more, which the int64 sums
 * do not cover; otherwise as the plain entry points.  Same handle-state rules as the plain entry points. */
int y4_decode_nms_merged(y4_handle h, int n, float iou_threshold, float score_threshold, const float* box_map_dev /* may be NULL */,
                         int32_t* cand_count_dev /* [n] out */, float* boxes_dev, float* scores_dev, float* classes_dev,
                         int32_t* valid_dev, int32_t* kept_idx_dev /* required */, void* stream);
int y4_nms_gathered_merged(y4_handle h, int n_groups, int max_slots, uint32_t group_cap, float iou_threshold, void* scratch_dev,
                           int32_t* cand_count_dev /* [n_groups] */, float* boxes_dev, float* scores_dev, float* classes_dev,
                           int32_t* valid_dev, int32_t* kept_idx_dev /* required */, void* stream);
/* ---- Validation loss: the forward of the reference's yolo_loss (loss.py:119-212; training_model, models.py:54-65) over the raw
 * heads y4_forward / y4_set_heads left in the workspace.  (Its gradient: "Head fine-tuning" below.)
 *
 * A responsible-cell RECORD is words = 8 + ceil(num_classes / 32) int32 values
 *     [scale, row, col, anchor, bits(x), bits(y), bits(w), bits(h), class mask word 0, ...]
 * (label xywh in network-input pixels as float32 bit patterns; class c is bit c % 32 of mask word c / 32).  An image has at
 * most max_boxes records, sorted by (scale, row, col, anchor); records_dev is [n, max_boxes, words], counts_dev [n].
 *
 * y4_loss_assign: the label assignment of preprocess_true_boxes (utils.py:215-303) for boxes_dev [n, max_boxes, 5] float32
 * (x1, y1, x2, y2, class in network-input pixels; max_boxes <= 256) -> xywh_dev [n, max_boxes, 4] (its y_true_boxes_xywh) and
 * the records of every image: rows with w <= 0 dropped by compaction, the k-th valid row's (w, h) picking the anchor and row k
 * the cell, the later of two rows on one (cell, anchor) keeping its xywh while the class bits of both stay set.  Unused record
 * slots are zeroed.  counts_dev[i] = -1 flags an image with a used row whose centre is off the grid or whose class id is
 * outside [0, num_classes) (the reference's IndexError); that row makes no record. */
int y4_loss_assign(y4_handle h, int n, const float* boxes_dev, int max_boxes, float* xywh_dev, int32_t* records_dev,
                   int32_t* counts_dev, void* stream);
/* floats of scratch y4_loss needs for n images (caller-provided, like the decode outputs; no workspace growth) */
int y4_loss_scratch_floats(y4_handle h, int n, size_t* floats);
/* out_dev [n, 3 scales, 3] float32: per image and scale the sums over all cells and anchors of the box term (GIoU), the
 * confidence term and the class term, as loss.py runs them (decode without xyscale, epsilon 1e-7, divide_no_nan, the ignore
 * mask max IoU(pred, every row of xywh_dev) < iou_loss_thresh); the caller combines them 3.54 / 64.3 / 1 and averages over the
 * batch (loss.py:136-140).  iou_loss_thresh < 0 is refused.  Reduced without floating-point atomics in an order fixed by
 * the image's geometry: image i's nine values do not depend on n or on its position in the batch.  Records that point
 * outside the grids are ignored. */
int y4_loss(y4_handle h, int n, const int32_t* records_dev, const int32_t* counts_dev, const float* xywh_dev, int max_boxes,
            float iou_loss_thresh, float* scratch_dev, size_t scratch_floats, float* out_dev, void* stream);
/* The box term of the handle: kind 0 = GIoU (the default; what loss.py has switched on, loss.py:156), 1 = CIoU (the line under
 * it, loss.py:157: bbox_ciou, loss.py:63-113).  Host-only state, settable at any time, no effect on the workspace, not a
 * scheduling choice (y4_copy_schedule does not carry it); any other kind returns Y4_EINVAL.  It is read by y4_loss, y4_loss_grad,
 * y4_head_grad, y4_block_grad and y4_block_grad_scaled at the call.  With kind 1 the box term of a responsible lane is
 *     (2 - lw lh / input_area) * (1 - ciou),   ciou = iou - p2 / c2 - a v,
 *     iou = inter / (union + 1e-9), both areas taken from the corners (the predicted corners after min / max normalisation),
 *     p2 = squared distance of the centres, c2 = squared diagonal of the enclosing box (a plain division, no divide_no_nan),
 *     v = 4 (atan(pw / (ph + 1e-9)) - atan(lw / (lh + 1e-9)))^2 / pi^2,   a = v / (1 - iou + v)
 * with the weight 3.54 and everything around it (decode without xyscale, confidence and class terms, the ignore mask with its
 * own IoU and 1e-7) unchanged.  Its derivative is what TensorFlow's autodiff of that text gives w.r.t. (tx, ty, tw, th): the
 * reference has no stop_gradient, so a v = v^2 / (1 - iou + v) is differentiated as a whole (unlike Darknet's constant a), through
 * both uses of iou, through p2, and through c2 via the enclosing corners; at a tie of a maximum / minimum the strict comparison
 * decides, as for GIoU.  Where the reference itself is non-finite (1 - iou + v == 0, c2 == 0) the result is some non-finite
 * value; nothing else is non-finite.  With kind 0 every entry point returns the bits it returned before this switch existed. */
int y4_set_box_loss(y4_handle h, int kind);
/* -> the kind (0 / 1), or a negative error code */
int y4_get_box_loss(y4_handle h);

/* ---- Head fine-tuning: the three detection convs (93 / 101 / 109; reference custom_layers.py yolov4_neck, the three
 * conv(..., activation=None, batch_norm=False) calls) trained on a frozen backbone and neck -- in Keras terms every layer
 * trainable = False except those three, then Model.fit on training_model (reference models.py:54-65,79-84,100-107).  No other
 * layer has a gradient here.
 *
 * The objective is  sum_i img_weight[i] * (3.54 box_i + 64.3 conf_i + 1 class_i)  (loss.py:131-135; img_weight = 1 / N gives
 * the batch mean of loss.py:184-186).  Its derivative w.r.t. a raw head value is what TensorFlow's autodiff of loss.py gives:
 * through decode without xyscale (loss.py:206-207), through GIoU w.r.t. all four predicted values including the enclosing box and
 * divide_no_nan (loss.py:34-60), through BOTH factors of the confidence term (conf_focal is not a constant, loss.py:176-182),
 * sigmoid(x) - z for the class logits of responsible lanes (loss.py:165), and none through the ignore mask (a cast of a
 * comparison, loss.py:173).  At a tie of a maximum / minimum inside GIoU autodiff's choice is unspecified; here the strict
 * comparison decides.  Records that point outside the grids are ignored, as in y4_loss.  Same determinism rule as y4_loss: no
 * floating-point atomics, every sum in an order fixed by the geometry, the same call gives the same bits.
 *
 * The head convs' weights, their gradient, the float32 master copy and the Adam moments all use ONE layout: the three layers'
 * records one after the other (conv 93, 101, 109), each as it lies in the Darknet stream at y4_layer_info(...).weight_offset:
 * [cout biases][cout * cin weights in (out, in) order], cout = 3 * (5 + num_classes). */

/* BEFORE y4_workspace_bytes / y4_bind_workspace, default off: the outputs of convs 92 / 100 / 108 (the head convs' inputs) are
 * written to the workspace and live to the end of the forward also under workspace aliasing; with chain fusion on, the LDS pair
 * conv 92 -> conv 93 -- which otherwise keeps conv 92's output on chip -- stores it as well.  Results are unchanged; off leaves
 * y4_workspace_bytes, y4_launch_counts and every result exactly as they are.
 * on = 2 (the level y4_block_grad needs) additionally keeps the INPUTS of convs 92 / 100 / 108 -- the outputs of convs 91 / 99 / 107
 * -- alive to the end of the forward under workspace aliasing; a run that would keep one of them on chip stores it as well (the
 * launch count does not change; in this network each of them already has a reader outside every fused run, and the call returns
 * Y4_ESTATE if a plan ever breaks that).  Results are again unchanged; levels 0 and 1 behave exactly as before, and every other
 * non-zero value still means level 1. */
int y4_set_retain_head_inputs(y4_handle h, int on);
/* Parity / debugging entry, dense on purpose: the derivative above for the heads in the workspace, as three float32 tensors
 * [n, gh, gw, 3 * (5 + C)] (the layout of y4_get_heads).  Labels as y4_loss; img_weight_dev [n] float32. */
int y4_loss_grad(y4_handle h, int n, const int32_t* records_dev, const int32_t* counts_dev, const float* xywh_dev, int max_boxes,
                 float iou_loss_thresh, const float* img_weight_dev, float* out_s_dev, float* out_m_dev, float* out_l_dev,
                 void* stream);
/* floats of scratch y4_head_grad needs for n images */
int y4_head_grad_scratch_floats(y4_handle h, int n, size_t* floats);
/* The training path: the loss gradient fused with the weight gradient of the head convs, for the n images of the last y4_forward
 * (their raw heads AND the head convs' inputs are read from the workspace: Y4_ESTATE unless y4_set_retain_head_inputs is on).
 * dw_dev (layout above, dw_floats >= the three records) is written, or with accumulate != 0 added to:
 *     dW[o, c] = sum over images and cells of g[p, o] * X[p, c],   db[o] = sum g[p, o]
 * with g the derivative above, recomputed in registers and never stored: the three confidence rows of each layer in one pass
 * over X in strips of 64 cells, every other row from the at most max_boxes records per image.  X is converted up to float32
 * exactly; products and sums are float32 (fused multiply-add). */
int y4_head_grad(y4_handle h, int n, const int32_t* records_dev, const int32_t* counts_dev, const float* xywh_dev, int max_boxes,
                 float iou_loss_thresh, const float* img_weight_dev, float* scratch_dev, size_t scratch_floats, float* dw_dev,
                 size_t dw_floats, int accumulate, void* stream);
/* One step of Keras' Adam as the reference compiles it (models.py:83: Adam(learning_rate=1e-4), beta 0.9 / 0.999, epsilon 1e-7)
 * on the three records, t = 1, 2, ...:
 *     lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t),  m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,
 *     w -= lr_t * m / (sqrt(v) + epsilon)
 * on the caller's float32 master weights w_dev and moments m_dev, v_dev (n_floats = the three records exactly), followed by the
 * re-pack: the new weights go into the bound packed-weight workspace in the handle's dtype and canonical K order and the biases
 * into the layers' shift, by the kernels of y4_pack_weights -- a handle that loads the updated stream afresh holds the same bytes. */
int y4_head_adam(y4_handle h, const float* dw_dev, float* w_dev, float* m_dev, float* v_dev, size_t n_floats, float lr,
                 float beta1, float beta2, float epsilon, int t, void* stream);

/* ---- Fine-tuning of the 3x3 convs in front of the heads: convs 92 / 100 / 108 (reference custom_layers.py yolov4_neck, the
 * conv(x, 256 | 512 | 1024, 3) calls that feed the three detection convs; Conv + BatchNormalization + LeakyReLU(0.1)) -- in Keras
 * terms the KERNELS of these three convs and the weights and biases of convs 93 / 101 / 109 trainable, every other layer
 * trainable = False, including the three BatchNormalization layers, which run in inference mode (gamma, beta, moving mean and
 * variance untouched), as Keras runs a frozen BN.  No other layer has a gradient here.
 *
 * Per scale, with U the conv's input (the output of conv 91 / 99 / 107), A its output (the head conv's input),
 * s[c] = gamma[c] / sqrt(var[c] + 1e-3) (the scale y4_pack_weights folded), g the derivative of the objective of "Head fine-tuning"
 * w.r.t. the raw head, and Wh the head conv's weights as the forward used them (in the handle's dtype):
 *     dA[p, c]         = sum_o g[p, o] Wh[o, c]
 *     dZ[p, c]         = dA[p, c] * (A[p, c] > 0 ? 1 : 0.1) * s[c]          (TensorFlow's LeakyReLU gradient: 0.1 at exactly 0)
 *     dK[co,ci,kh,kw]  = sum over images, rows, columns of dZ[n,y,x,co] * U[n, y+kh-1, x+kw-1, ci]     ('same' zero padding)
 * dA uses g's structure -- three confidence terms per cell in anchor order, then the cell's records in record order -- and never
 * runs a full-width product over every cell; dZ is kept in scratch in the MFMA operand type (bf16 / fp16 for a 16-bit handle: one
 * rounding to nearest even; float32 for a float32 handle).  dK is an implicit GEMM over K = pixels on the matrix pipes
 * (v_mfma_f32_32x32x16_bf16 / _f16; v_mfma_f32_32x32x2_f32, exact float32, for a float32 handle) with float32 accumulation: K is cut
 * into (image, row strip) slices by the geometry alone, contiguous ranges of slices are summed in order into float32 partials in
 * scratch and a finish kernel adds the partials in range order.  No floating-point atomics: the same call gives the same bits.
 *
 * The gradient, the float32 master copy and the Adam moments use ONE layout: the three kernels one after the other (conv 92, 100,
 * 108), each cout * cin * 9 floats in the Darknet stream's (out, in, kh, kw) order, WITHOUT the four BatchNormalization vectors
 * that precede them in the stream (they lie at y4_layer_info(...).weight_offset + 4 * cout).
 * A float16 handle is refused (Y4_EINVAL) by y4_block_grad only: a 16-bit dZ in fp16 needs loss scaling, which
 * y4_block_grad_scaled provides; the scratch query and y4_block_adam take every dtype. */

/* bytes of scratch y4_block_grad needs for n images (dZ of the three scales, then the partials); 256-byte aligned.
 * Width limit of the weight gradient (two grid rows and their halo in LDS): a grid row of the stride-8 scale of at most 105 cells
 * on a float32 handle (an image 840 wide) and 200 cells on a bf16 or float16 handle (1600 wide); beyond it this call,
 * y4_block_grad and y4_block_grad_scaled return Y4_EINVAL before anything is launched. */
int y4_block_grad_scratch_bytes(y4_handle h, int n, size_t* bytes);
/* The gradient above for the n images of the last y4_forward: their raw heads, the head convs' inputs AND the inputs of convs
 * 92 / 100 / 108 are read from the workspace (Y4_ESTATE unless the retention level is 2: y4_set_retain_head_inputs(h, 2)).
 * Labels, iou_loss_thresh and img_weight_dev as y4_head_grad.  Call it BEFORE y4_head_adam of the same step: both gradients use
 * the head weights the forward used.  dk_dev (layout above, dk_floats >= the three kernels) is written, or with accumulate != 0
 * added to (one more float32 add per element). */
int y4_block_grad(y4_handle h, int n, const int32_t* records_dev, const int32_t* counts_dev, const float* xywh_dev, int max_boxes,
                  float iou_loss_thresh, const float* img_weight_dev, void* scratch_dev, size_t scratch_bytes, float* dk_dev,
                  size_t dk_floats, int accumulate, void* stream);
/* y4_block_grad with a loss scale, for float32, bf16 and float16 handles.  loss_scale must be a finite positive power of two
 * (Y4_EINVAL otherwise, before anything is launched): dZ, computed in float32 as above, is multiplied by it BEFORE its single
 * rounding to the operand type, and the ordered sum of the partials is multiplied by 1 / loss_scale before it is written or
 * added to dk_dev.  Both products are exact, so on a float32 or bf16 handle, away from under- and overflow, the result has the
 * bits of y4_block_grad; in fp16 the scale keeps the part of dZ that would round into the subnormals or to zero.
 * overflow_dev is one int32 in device memory that the call ORs into and never clears (the caller zeroes it, once for all the
 * chunks of a batch): bit 0 -- a stored dZ is inf or NaN (the scale is too large), bit 1 -- a sum is not finite.  When the word
 * is non-zero dk_dev holds nothing usable, including what was accumulated before.  It may be null on a float32 or bf16 handle
 * and is required on a float16 handle (Y4_EINVAL).  y4_block_grad is this call with scale 1 and no word.  The flags are raised
 * by integer atomicOr, one per workgroup at most, which is order-independent: the same call still gives the same bits. */
int y4_block_grad_scaled(y4_handle h, int n, const int32_t* records_dev, const int32_t* counts_dev, const float* xywh_dev,
                         int max_boxes, float iou_loss_thresh, const float* img_weight_dev, float loss_scale,
                         int32_t* overflow_dev, void* scratch_dev, size_t scratch_bytes, float* dk_dev, size_t dk_floats,
                         int accumulate, void* stream);
/* One step of the Adam rule of y4_head_adam (same element rule, lr_t in double on the host; pass the same t for both calls of a
 * step) on the caller's float32 master kernels k_dev and moments m_dev, v_dev (n_floats = the three kernels exactly), followed by
 * the re-pack of the three layers: the new kernels go into the bound packed-weight workspace in the handle's dtype and canonical K
 * order, and into the MFMA-fragment copy the halo2 tiles read where the layer has one, by the kernels of y4_pack_weights.  The
 * BatchNormalization is frozen, so scale and shift stay as y4_pack_weights folded them: a handle that loads the updated stream
 * afresh holds the same bytes over the whole weight workspace. */
int y4_block_adam(y4_handle h, const float* dk_dev, float* k_dev, float* m_dev, float* v_dev, size_t n_floats, float lr,
                  float beta1, float beta2, float epsilon, int t, void* stream);

/* ---- Cached frozen features.  Everything in front of the trainable convs is frozen, so for an image whose pixels do not change
 * the tensors the handle retains (y4_set_retain_head_inputs) are the same in every epoch.  A cache ROW is what one image
 * contributes at the handle's retention level, dense (no channel stride) in the handle's storage dtype, the three scales back to
 * back in the order of the heads (stride 8, 16, 32), each [rows, columns, channels]:
 *     level 1: the outputs of convs 92 / 100 / 108 (the head convs' inputs),
 *     level 2: the outputs of convs 91 / 99 / 107  (the inputs of convs 92 / 100 / 108).
 * The cache is caller-owned device memory of cache_rows * row_bytes bytes, 16-byte aligned.  A step on cached rows is
 * y4_feature_load -> y4_forward_tail -> y4_loss / y4_head_grad / y4_block_grad* / y4_get_heads / y4_decode_nms as after y4_forward;
 * by the canonical K order (a conv gives the same bits in whatever launch it runs) the results have the bits of the full forward. */

/* *row_bytes: the bytes of one row, a multiple of 256; offs[k]: the byte offset of scale k's tensor in it (each a multiple of
 * 256; the bytes between one tensor's end and the next offset are padding that no call reads or writes).  Either may be null.
 * Y4_ESTATE at retention level 0. */
int y4_feature_row_bytes(y4_handle h, size_t* row_bytes, size_t offs[3]);
/* After a forward of n images: image i's retained tensors are copied out of the workspace views into row slots_host[i] of the
 * cache.  ONE launch for the three scales and the n images (per 256 images), no host synchronisation: slots_host is a HOST
 * array that is read before the call returns and travels as a kernel argument.  A slot outside [0, cache_rows), a slot named
 * twice, n outside [1, max_batch] or a null / misaligned cache: Y4_EINVAL before anything is launched. */
int y4_feature_store(y4_handle h, int n, const int64_t* slots_host, void* cache_dev, size_t cache_rows, void* stream);
/* The inverse: row slots_host[i] is written into batch position i of the same views (a row may be named more than once).
 * Same launch, same refusals bar the repeated slot. */
int y4_feature_load(y4_handle h, int n, const int64_t* slots_host, const void* cache_dev, size_t cache_rows, void* stream);
/* Runs only the convs behind the cached tensors on what the workspace holds for n images -- level 1: convs 93 / 101 / 109;
 * level 2: convs 92, 93, 100, 101, 108, 109, in plan order -- and leaves the raw heads, the objectness side array and, at level
 * 2, the stored outputs of convs 92 / 100 / 108 as y4_forward leaves them.  A conv of the tail that the schedule fuses with a
 * conv outside the tail runs as its own launch (level 1: the LDS pair 92 -> 93); a run wholly inside the tail runs as the
 * schedule says.  Y4_ESTATE at retention level 0. */
int y4_forward_tail(y4_handle h, int n, void* stream);

/* Replaces inference_model.predict(imgs) (reference models.py:69-73,113,159) = forward + decode + NMS. */
int y4_predict(y4_handle h, const float* imgs_nhwc_dev, int n, float* boxes_dev, float* scores_dev,
               float* classes_dev, int32_t* valid_dev, int32_t* kept_idx_dev, void* stream);

int y4_predict_u8(y4_handle h, const uint8_t* imgs_nhwc_u8_dev, int n, float* boxes_dev, float* scores_dev,
                  float* classes_dev, int32_t* valid_dev, int32_t* kept_idx_dev, void* stream);

/* Per-op device time of one forward (+decode+NMS) in ms, measured with HIP events on `stream`
 * (synchronises).  `names` receives op names ('c17', 'spp', 'decode', 'nms', ...), 16 bytes each. */
int y4_profile(y4_handle h, const float* imgs_nhwc_dev, int n, float* op_ms, char* names, int cap,
               int* n_ops, void* stream);

/* Measured per-layer tile selection for batch n (call once after y4_pack_weights; optional).  Every tile
 * configuration gives bit-identical outputs, so this affects speed only.  y4_get_tiles reports the choice
 * per conv index (0 = built-in heuristic). */
int y4_autotune(y4_handle h, int n, int reps, void* stream);
/* The same with THROUGHPUT as objective, for two batches in flight: `h2` is a second handle of the same plan (own activation
 * workspace, may share the packed-weight workspace) that will run on `stream2` beside `h` on `stream`.  Every timed
 * launch is issued on both handles and the time until both streams are done counts, so a tile whose last round leaves
 * compute units idle is not charged for them (the neighbour stream fills them): the least WORK wins, not the shortest solitary
 * launch.  `pair_passes` says which decisions use that objective (the others are taken one launch at a time, as y4_autotune
 * does): bit 0 the tile of every conv, bit 1 chains / LDS pairs fused or separate, bit 2 the stage kernel, bit 3 the
 * residual-block kernels.  Both handles end up with the same choices.  (No reference counterpart: TensorFlow's executor
 * schedules the reference's graph; models.py:113,159.) */
int y4_autotune_pair(y4_handle h, y4_handle h2, int n, int reps, void* stream, void* stream2, int pair_passes);
int y4_get_tiles(y4_handle h, int32_t* tiles, int cap);
/* Restore a tile choice saved from y4_get_tiles (one entry per conv index; an id that does not fit its layer makes
 * the next forward fail with Y4_EINVAL rather than compute anything different).  The head conv of a fused run (see
 * y4_set_chain_fusion) carries two choices in its entry: -(run tile + 1000 * the conv's own tile for when the run is not in
 * force); a plain -t (older files) leaves the own tile as it is, so y4_set_tiles(y4_get_tiles()) restores a handle exactly. */
int y4_set_tiles(y4_handle h, const int32_t* tiles, int count);
/* Every scheduling choice of `src` -> `dst`, a second handle created from the same configuration (the sibling that runs a second
 * batch in flight): the `Schedule` (csrc/runtime.hip) -- tiles, each run's state, stage-kernel and residual-block verdicts, the
 * fusion switches, sub-batching, the halo2 permission.
 * (No reference counterpart: TensorFlow's executor schedules the reference's graph; models.py:113,159.) */
int y4_copy_schedule(y4_handle src, y4_handle dst);

/* Scheduling knob (results unchanged): run the ops up to and including conv `last_conv` over `images` images at a
 * time instead of the whole batch, so that the large early activations of a sub-batch are still resident in the
 * 256 MiB Infinity Cache when their consumer runs.  images <= 0 turns it off. */
int y4_set_subbatch(y4_handle h, int images, int last_conv);

/* Scheduling knob (16-bit dtypes, img_size <= 640; results unchanged): run convs 0 and 1 (reference
 * custom_layers.py:101-102) as one kernel that keeps conv 0's output -- the largest tensor of the network -- in LDS
 * instead of writing it to HBM and reading it back.  While on, y4_get_conv_output(0) fails with Y4_ESTATE and the
 * profile reports the pair under 'c0' ('c1' reads 0).  Y4_EINVAL if the dtype / size is not supported. */
int y4_set_stem_fusion(y4_handle h, int on);

/* Scheduling knob (16-bit dtypes): run each "3x3 conv + residual Add -> 1x1 conv [-> 1x1 conv over
 * Concatenate([., route])]" run of the CSP stages with 64-channel blocks (reference custom_layers.py:41-44, :66-69
 * and the conv that follows csp_block, :104/:109) as ONE kernel: the intermediate tensors stay in registers instead
 * of going through HBM; likewise "3x3 conv + Add -> the next block's 1x1 conv" of the 128- and 256-channel stages
 * through an LDS-resident tile.  A chained conv issues the same MFMAs on the same inputs in the same order as its own
 * kernel: results are bit-identical.  Returns the number of fusable runs (>= 0) when turned on, Y4_OK when turned off,
 * a negative Y4_E* code on error.  While on, y4_get_conv_output of a conv inside a run (not its last) reads a
 * tensor that is not materialised.  y4_autotune then also decides per run, by measurement, whether it executes as
 * one kernel or as separate ones; y4_get_tiles reports a fused run's head conv as MINUS its tile id (y4_set_tiles
 * accepts the same encoding; > 0 there means separate kernels, 0 fused with the built-in tile).  One run is an ALTERNATIVE:
 * "1x1 conv 64 -> 64 -> 1x1 conv over Concatenate([., route])" (custom_layers.py:66-69) is in force only while the three-conv run
 * it is the tail of cannot exist because that run's 3x3 conv executes inside a residual-block kernel (y4_set_res_fusion). */
int y4_set_chain_fusion(y4_handle h, int on);

/* Scheduling knob (16-bit dtypes; results unchanged): run the whole first CSP stage -- convs 2..7, reference
 * custom_layers.py:47-69 (csp_block with residual_bottleneck=True) and the transition conv :105 -- as ONE spatially tiled
 * kernel (csrc/csp_stage.hip): per 16x16-pixel tile the route / main-in / bottleneck / 3x3+Add / main-out / transition
 * convs run from LDS and registers, so only conv 1's output is read and conv 7's written.  Every conv issues the same
 * MFMAs on the same 16-bit inputs in the same order as its own kernel: bit-identical.  Returns 1 when the stage kernel
 * is active, 0 when off, a negative Y4_E* code on error (Y4_EINVAL for fp32).  y4_autotune afterwards keeps it only if
 * it measures faster than the separately tuned kernels (y4_get_stage_fusion tells).  While active,
 * y4_get_conv_output of convs 2..6 fails with Y4_ESTATE (not materialised). */
int y4_set_stage_fusion(y4_handle h, int on);
int y4_get_stage_fusion(y4_handle h);

/* Scheduling knob (16-bit dtypes; results unchanged): run every residual block "1x1 conv -> 3x3 conv + Add" of the 64- and
 * 128-channel CSP stages (reference custom_layers.py:34-44; the 152^2 and 76^2 stages at 608x608) as ONE spatially tiled
 * kernel (csrc/resblock.hip): the halo'd 18x18-pixel tile of the block input is brought into LDS once, the 1x1 conv runs
 * on it in place and the 3x3 conv reads all nine taps from that tile, streaming only its weights.  Bit-identical to the
 * separate kernels.  Returns the number of such blocks (>= 0) when turned on, Y4_OK when turned off, < 0 on error.
 * y4_autotune afterwards keeps it per channel group only where it measures faster; y4_get_res_fusion reports the groups
 * in use as a bit mask (1: 128 channels, 2: 64 channels) and y4_set_res_fusion_mask restores such a choice.  While a
 * block runs fused, y4_get_conv_output of its 1x1 conv fails with Y4_ESTATE (not materialised). */
int y4_set_res_fusion(y4_handle h, int on);
int y4_get_res_fusion(y4_handle h);
int y4_set_res_fusion_mask(y4_handle h, int mask);

/* Host only (no device is touched): the tile table the residual-block kernel walks for a batch of n maps of h x w pixels with
 * c (64 | 128) channels on `slots` workgroups (a multiple of 8: slots / 8 per XCD).  int32 quadruples: a header {grid, stride, a, b}
 * -- workgroups of the launch, entries per list, and the two constants of a tile's cost a + b * rows -- followed by `grid` lists of
 * `stride` entries {image, first output row, rows, tile column (16 pixels)}; a list ends at its first entry with rows = 0, and list i
 * runs on XCD i % 8.  Every column of every image is cut into heights from {16, 12, 8, 4} (c = 128) or {16, 8} (c = 64) that cover
 * its rows exactly once; only a column's last tile may hang over the lower edge, by less than the smallest height.
 * Returns the number of int32 values of the table (> 0), written to `out` when cap is at least that; < 0 on error. */
int y4_rb_tile_table(int32_t n, int32_t h, int32_t w, int32_t c, int32_t slots, int32_t* out, int32_t cap);

/* Kernel launches of one y4_predict under the current fusion / tile settings (whole batch, no sub-batching):
 * `conv_family` = launches of the conv kernels other than the stem (what bench.py's roofline is quoted on),
 * `total` = all launches including stem, SPP, decode and NMS. */
int y4_launch_counts(y4_handle h, int32_t* conv_family, int32_t* total);

/* Live per-op timing of the calls in between: while a session is open, each y4_predict (up to max_steps of
 * them) records a HIP event on its stream after every op, without synchronising.  y4_timing_end
 * synchronises the stream and returns the mean device time per op in ms ('c1'.., 'spp', 'decode', 'nms').
 * coarse != 0: events only where the op kind changes (stem | run of convs | spp | run of convs | decode | nms);
 * each run's time is reported under its first op, the others read 0 -- 7 events per step instead of 115. */
int y4_timing_begin(y4_handle h, int max_steps, int coarse);
int y4_timing_end(y4_handle h, float* op_ms_mean, char* names, int cap, int* n_ops, int* steps_recorded,
                  void* stream);

/* ---- standalone operators (same kernels as the plan uses; for unit tests and other hosts) ---- */

typedef struct y4_conv_desc {
    int32_t dtype;                 /* Y4_* of in/weights/out/res */
    int32_t n, h, w, cin;          /* input NHWC view: [n,h,w,in_cstride][..., in_coff:in_coff+cin] */
    int32_t cout, ksize, stride;   /* ksize 1|3; stride 1 ('same') | 2 (pad top/left 1, 'valid') */
    int32_t act;                   /* Y4_ACT_* */
    int32_t upsample;              /* 1: write each output pixel to its 2x2 nearest-upsampled block */
    int32_t out_f32;               /* 1: output buffer is float32 regardless of dtype */
    int32_t in_cstride, in_coff;
    int32_t out_cstride, out_coff;
    int32_t res_cstride, res_coff; /* residual view (same spatial dims as the output), used if res != NULL */
    const void* in;
    const void* wt;                /* packed by y4_pack_conv_weights */
    const float* scale;            /* [cout_pad] */
    const float* shift;            /* [cout_pad] */
    const void* res;
    void* out;
    int32_t tile;                  /* 0 = auto; otherwise a tile-config id (see y4_conv_tile_count) */
    /* optional second output view: channels [split, cout) are stored to out2 (channel c -> out2_coff + c - split).
     * Used to run a CSP block's route conv and main-in conv (same input, custom_layers.py:58-60) as ONE GEMM. */
    void* out2;
    int32_t out2_cstride, out2_coff, split;
    /* split-K (tile = base + 100 e: the base tile's K loop split 2^e ways, e = 1..3; for launches with fewer tiles than compute
     * units): device scratch of 16 KiB of tile counters, ZERO before the first use (every launch leaves them zero), followed by
     * 2^e x tiles x BM x BN floats of partial sums.  NULL / 0 when no split tile is used. */
    void* splitk_ws;
    size_t splitk_ws_bytes;
    /* halo2 tiles (schedule code 21: one wave per SIMD, v_mfma_32x32x16, weights read into registers): the same weights once more in
     * MFMA-fragment order, made from `wt` by y4_pack_conv_frag32.  NULL for every other tile. */
    const void* wt_frag;
} y4_conv_desc;

/* cout_pad (rows of the packed matrix) and bytes needed for a packed kernel */
int y4_packed_conv_bytes(int dtype, int cout, int cin, int ksize, int32_t* cout_pad, size_t* bytes);
/* Darknet (cout,cin,k,k) float32 on device -> packed [cout_pad][cin/KC][k*k][KC] dtype (KC = min(cin, 64) for k = 3, cin for k = 1: the
 * K order every conv kernel sums in); rows >= cout are zero */
int y4_pack_conv_weights(int dtype, int cout, int cin, int ksize, const float* oihw_dev, void* packed_dev,
                         void* stream);
/* 3x3 conv weights packed by y4_pack_conv_weights (16-bit dtypes, cin % 64 == 0) -> the layout the halo2 tiles read:
 * [cout_pad / 32 channel blocks][cin / 64 chunks][9 taps][4 k-steps of 16 channels][64 lanes][8 elements], lane l of a k-step = row
 * (l & 31) of the block in the accumulator layout's channel order, input channels 16 s + 8 (l >> 5) .. +7 of the chunk: one k-step's
 * v_mfma_f32_32x32x16 A operand of a block is 1 KB contiguous.  Same size as the packed matrix (y4_packed_conv_bytes). */
int y4_pack_conv_frag32(int dtype, int cout, int cin, const void* packed_dev, void* frag_dev, void* stream);
/* One conv() unit of the reference (custom_layers.py:5-31) + optional Add (custom_layers.py:44) +
 * optional UpSampling2D (custom_layers.py:147,159) + concat-slice store (custom_layers.py:68,...). */
int y4_conv2d(const y4_conv_desc* d, void* stream);
int y4_conv_tile_count(void);
/* Tile configuration `tile` (1 .. y4_conv_tile_count()): cfg = {BM pixels, BN channels, waves over pixels, waves over
 * channels, bytes of K per LDS row, schedule code (2..7 = ring stages, 12 = staggered 2-stage, 32 = 2-stage with the 32x32x16
 * MFMA)}.  All tiles with the 16x16x32 MFMA give bit-identical results; the 32x32x16 tiles agree among themselves. */
int y4_conv_tile_desc(int tile, int32_t cfg[6]);
/* Latency schedules (the reference's own call is one image: Yolov4.predict, models.py:109-127).  With few images the deep layers
 * have fewer output tiles than the GPU has compute units and each tile walks a long K loop alone; `on` lets y4_autotune also offer
 * split-K tile ids (base + 100 e: the K loop of a tile split over 2^e workgroups, the last one to finish adds the partial sums in
 * split order and runs the epilogue).  A split launch sums in another fp32 order than the unsplit one, so with this switch the
 * tuned schedule is part of the numerical result (like the 32x32x16 tiles; tested against the oracle); off by default. */
int y4_set_splitk(y4_handle h, int on);
/* The halo2 tiles (schedule code 21, conv_halo2_kernel.h: the 3x3 stride-1 convs of custom_layers.py:14-24 as a one-wave-per-SIMD kernel on
 * v_mfma_f32_32x32x16 with the weights read into registers in MFMA-fragment order) sum the K axis in k-steps of 16 instead of 32:
 * another fixed fp32 order than the 16x16x32 tiles.  `on` lets y4_autotune offer them too; the tuned schedule then is part of the
 * numerical result, exactly as with y4_set_splitk (tested against the oracle and for run-to-run determinism); off by default. */
int y4_set_halo2(y4_handle h, int on);
/* Stem conv (cin = 3, reference custom_layers.py:101): float32 images -> dtype.  `wk_dev` is an 8192-byte table
 * made by y4_pack_stem_weights from Darknet (cout,3,3,3) order: float32 [(ky*3+kx)*3+ci][cout] for the fp32
 * kernel, then (byte 4096 / 6144) the bf16 / fp16 MFMA weight fragments used by the 16-bit kernels. */
int y4_pack_stem_weights(const float* w_oihw_dev, float* wk_dev, int cout, void* stream);
int y4_stem_conv(int dtype, const float* imgs_dev, int n, int h, int w, const float* wk_dev,
                 const float* scale, const float* shift, int cout, int act, void* out_dev, int out_cstride,
                 int out_coff, void* stream);
/* Device-side Yolov4.preprocess_img (reference models.py:95-98: cv2.resize INTER_LINEAR stretch, then /255.):
 * uint8 RGB image [h,w,3] -> float32 [out_h,out_w,3] in [0,1], one image slot of the batch tensor y4_forward takes.
 * Saves the 4x fatter float32 host->device copy and the host-side float64 tensor. */
int y4_preprocess_u8(const uint8_t* img_dev, int h, int w, float* out_dev, int out_h, int out_w, void* stream);
/* The resize half of preprocess_img alone, batched: uint8 [n,h,w,3] -> uint8 [n,out_h,out_w,3] with cv2.resize's
 * uint8 INTER_LINEAR fixed-point arithmetic (what cv2.resize itself returns for a uint8 image). */
int y4_resize_u8(const uint8_t* imgs_dev, int n, int h, int w, uint8_t* out_dev, int out_h, int out_w, void* stream);
/* One image of a ragged batch for y4_resize_u8_ragged: a packed uint8 [h,w,3] source at byte `offset` of the source buffer,
 * resized to out_h x out_w and placed at (pad_top, pad_left) of the network canvas. */
typedef struct y4_image_desc {
    int64_t offset;
    int32_t h, w, out_h, out_w, pad_top, pad_left;
} y4_image_desc;
/* The resize half of preprocess_img over a batch of images of DIFFERENT sizes, in one launch: image i (desc_dev[i], a device
 * array of n descriptors) -> slot i of the uint8 [n,H,W,3] batch y4_forward_u8 / y4_predict_u8 take.  Canvas pixels inside
 * [pad_top, pad_top + out_h) x [pad_left, pad_left + out_w) are cv2.resize's uint8 INTER_LINEAR resize of the source to
 * out_w x out_h (the arithmetic of y4_resize_u8); every other pixel is `pad_value` (0..255) in all three channels.
 *   stretch   (reference models.py:95-98): out_h = H, out_w = W, pads 0 -- the same bytes as y4_resize_u8 on that image;
 *   letterbox (Darknet's letterbox_image geometry): the aspect-keeping rectangle, centred -- yolo4hip/prepost.py: letterbox_rect.
 * The arguments are checked on the host (NULL pointers, n, H, W, pad_value, an output of 2^31 bytes or more: Y4_EINVAL before
 * any launch), but the descriptors live on the device and are NOT checked: the caller owns the table's correctness (offsets
 * and sizes inside the source buffer, h, w, out_h, out_w >= 1, the rectangle inside the canvas). */
int y4_resize_u8_ragged(const uint8_t* src_dev, const y4_image_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                        int pad_value, void* stream);
/* One WINDOW of a source image for y4_window_u8_ragged: `offset` is the byte offset of the window's first pixel in the source
 * buffer (image offset + (y0 * image width + x0) * 3), `pitch` the bytes of a source row (3 * image width, >= 3 * w), h x w the
 * window; the rest as y4_image_desc. */
typedef struct y4_window_desc {
    int64_t offset;
    int32_t pitch;
    int32_t h, w;
    int32_t out_h, out_w, pad_top, pad_left;
} y4_window_desc;                                    /* 40 bytes */
/* y4_resize_u8_ragged on windows, crop and resize in one launch: slot i of the uint8 [n,H,W,3] batch holds the bytes
 * y4_resize_u8_ragged writes for a contiguous copy of window i with the same out_h, out_w, pad_top, pad_left.  The bilinear taps
 * therefore clamp at the WINDOW's edge, not the image's; a window with h == out_h and w == out_w is a plain copy; any number of
 * descriptors may point into one source image (overlapping tiles of a photo).  Host checks and the caller's ownership of the device
 * table as for y4_resize_u8_ragged (every window inside its image, pitch >= 3 * w). */
int y4_window_u8_ragged(const uint8_t* src_dev, const y4_window_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                        int pad_value, void* stream);
/* One VIEW of a window for y4_view_u8_ragged: the fields of y4_window_desc, then `flip` -- bit 0 mirrors the canvas left-right,
 * bit 1 up-down (0..3) --, padded to 48 bytes. */
typedef struct y4_view_desc {
    int64_t offset;
    int32_t pitch;
    int32_t h, w;
    int32_t out_h, out_w, pad_top, pad_left;         /* as y4_window_desc */
    int32_t flip;                                    /* bits 0 (left-right) and 1 (up-down) */
    int32_t reserved[2];                             /* not read */
} y4_view_desc;                                      /* 48 bytes */
/* y4_window_u8_ragged with a mirror of the CANVAS, still one launch: canvas pixel (y, x) of slot i is sourced from canvas pixel
 * (y', x') of the unflipped canvas, x' = W - 1 - x under bit 0 of flip and y' = H - 1 - y under bit 1 (the rule of
 * y4_augment_u8_ragged's flip, on both axes).  Slot i therefore holds np.flip, along the flipped axes, of the bytes
 * y4_window_u8_ragged writes for the same descriptor without `flip`, padding included; at flip == 0 it holds exactly those bytes.
 * The mirror applies to the coordinate a pixel is sourced from, never to where it is stored.  Any number of descriptors may point
 * into one source image (the views of one photo).  Host checks and the caller's ownership of the device table as for
 * y4_window_u8_ragged. */
int y4_view_u8_ragged(const uint8_t* src_dev, const y4_view_desc* desc_dev, int n, uint8_t* out_dev, int H, int W, int pad_value,
                      void* stream);
/* One image of a ragged batch for y4_augment_u8_ragged: the fields of y4_image_desc, then the augmentation of this image --
 * flip (0 / 1: mirror left-right) and the HSV factors (hue is added, sat and val multiply; 0, 1, 1 change nothing). */
typedef struct y4_augment_desc {
    int64_t offset;
    int32_t h, w, out_h, out_w, pad_top, pad_left;   /* as y4_image_desc */
    int32_t flip;                                    /* 0 / 1 */
    float   hue, sat, val;
} y4_augment_desc;                                   /* 48 bytes */
/* y4_resize_u8_ragged with the training-time augmentation of Yolov4.fit, still one launch: image i -> slot i of the uint8
 * [n,H,W,3] batch y4_forward_u8 takes.
 *   flip      canvas column x is sourced from canvas column x' = W - 1 - x (x' = x without flip);
 *   geometry  with yy = y - pad_top, xx = x' - pad_left: inside [0,out_h) x [0,out_w) the pixel is cv2.resize's uint8
 *             INTER_LINEAR resize of the source to out_w x out_h at (yy, xx) -- the arithmetic of y4_resize_u8_ragged --,
 *             otherwise `pad_value` in all three channels, without the colour transform.  The rectangle may lie partly or wholly
 *             outside the canvas (pad_top / pad_left negative, out_h > H, out_w > W); only its visible part is computed;
 *   colour    on resized pixels only, in float32, skipped when hue == 0 && sat == 1 && val == 1 (the bytes are then exactly the
 *             resize's): RGB / 255 -> HSV by the colorsys.rgb_to_hsv rule (hue in [0,1); S = 0 and H = 0 at max == 0 or
 *             max == min), H <- H + hue - floor(H + hue), S <- clamp(S * sat, 0, 1), V <- clamp(V * val, 0, 1), back by the
 *             colorsys.hsv_to_rgb rule, byte = clamp(floor(255 c + 0.5), 0, 255).
 * The arguments are checked on the host as in y4_resize_u8_ragged (NULL pointers, n in 1..65535, H, W > 0, pad_value in 0..255,
 * an output of 2^31 bytes or more: Y4_EINVAL before any launch).  The descriptors live on the device and are NOT checked: the
 * caller owns the table's correctness (offsets and sizes inside the source buffer, h, w, out_h, out_w >= 1, finite factors). */
int y4_augment_u8_ragged(const uint8_t* src_dev, const y4_augment_desc* desc_dev, int n, uint8_t* out_dev, int H, int W,
                         int pad_value, void* stream);
/* The cut of one mosaic canvas: rows [0, cut_y) x columns [0, cut_x) are tile 0's window, the three other rectangles the cut
 * divides the canvas into those of tiles 1 (top right), 2 (bottom left), 3 (bottom right). */
typedef struct y4_mosaic_cut { int32_t cut_y, cut_x; } y4_mosaic_cut;   /* 8 bytes */
/* Mosaic: four images around a cut on each canvas, one launch for the batch.  Canvas i has the four rows
 * tiles_dev[4 i + q], q = 0..3, and the cut cuts_dev[i]; its pixel (y, x) is pixel (y, x) of y4_augment_u8_ragged's rule
 * under row q = 2 (y >= cut_y) + (x >= cut_x), applied on the WHOLE H x W canvas: the flip mirrors about the canvas
 * (x' = W - 1 - x), pixels outside the row's rectangle are `pad_value`, colour is applied to resized pixels only and skipped
 * at (0, 1, 1) -- byte for byte the y4_augment_u8_ragged canvas of that row inside the row's window.  A canvas with the cut
 * (H, W) is row 4 i alone.  Rows may share a source (the same offset, h, w), within a canvas and across canvases.  The image
 * of a row whose window is empty (cut_y or cut_x at 0 or at H / W) is never read; the row itself only has to be readable.
 * The arguments are checked on the host as in y4_augment_u8_ragged, and cuts_dev against NULL (Y4_EINVAL before any launch).
 * The rows and cuts live on the device and are NOT checked: the caller owns their correctness -- every row with a non-empty
 * window as y4_augment_u8_ragged asks (offsets and sizes inside the source buffer, h, w, out_h, out_w >= 1, finite
 * factors), and 0 <= cut_y <= H, 0 <= cut_x <= W. */
int y4_mosaic_u8_ragged(const uint8_t* src_dev, const y4_augment_desc* tiles_dev /* [n][4] */,
                        const y4_mosaic_cut* cuts_dev /* [n] */, int n, uint8_t* out_dev, int H, int W, int pad_value,
                        void* stream);
/* One 8-bit 4:2:0 video frame for y4_yuv_u8_ragged: a luma plane h x w with row pitch y_pitch at byte y_offset of the source
 * buffer, and two chroma planes subsampled 2 x 2 -- ceil(h / 2) rows of ceil(w / 2) samples, so odd sizes are legal -- at
 * u_offset and v_offset with row pitch c_pitch and c_step bytes between two samples of one plane:
 *   NV12   v_offset = u_offset + 1, c_step = 2 (one interleaved UV plane);     NV21   u_offset = v_offset + 1, c_step = 2;
 *   I420   c_step = 1, the U plane before the V plane;                         YV12   c_step = 1, V before U.
 * A decoder surface with its own pitch is described in place.  out_h, out_w, pad_top, pad_left as y4_image_desc.
 * `flags`: bit 0 selects the BT.709 matrix (0: BT.601), bit 1 full range (0: limited range, Y 16..235, chroma 16..240). */
typedef struct y4_yuv_desc {
    int64_t y_offset, u_offset, v_offset;
    int32_t y_pitch, c_pitch, c_step;
    int32_t h, w, out_h, out_w, pad_top, pad_left;
    int32_t flags;
} y4_yuv_desc;                                       /* 64 bytes */
#define Y4_YUV_BT709 1
#define Y4_YUV_FULL_RANGE 2
/* Colour conversion and resize of video frames in one launch: frame i (desc_dev[i]) -> slot i of the uint8 [n,H,W,3] batch.
 * Slot i holds the bytes y4_resize_u8_ragged writes, with the same out_h, out_w, pad_top, pad_left and pad_value, for the packed
 * RGB frame that the following rule gives at SOURCE resolution:
 *   chroma   source pixel (y, x) takes U = src[u_offset + (y >> 1) * c_pitch + (x >> 1) * c_step], V likewise: sample replication,
 *            no siting and no chroma interpolation;
 *   colour   integers only, sums in int32, arithmetic shift.  C = Y - y0 (y0 = 16 limited range, 0 full range), D = U - 128,
 *            E = V - 128;
 *              R = clamp8((cy C + crv E + 8192) >> 14)
 *              G = clamp8((cy C + cgu D + cgv E + 8192) >> 14)
 *              B = clamp8((cy C + cbu D + 8192) >> 14)
 *            every coefficient is floor(c 2^14 + 0.5) of the real coefficient from (Kr, Kb); for limited range the luma scale is
 *            255/219 and the chroma scale 255/224:
 *                                  cy     crv    cgu     cgv    cbu
 *              BT.601 limited   19077   26149  -6419  -13320  33050      (flags 0)
 *              BT.601 full      16384   22970  -5638  -11700  29032      (flags 2)
 *              BT.709 limited   19077   29372  -3494   -8731  34610      (flags 1)
 *              BT.709 full      16384   25802  -3069   -7670  30402      (flags 3)
 *   resize   each of the four bilinear taps is converted, then the arithmetic of y4_resize_u8 runs on the converted taps; a
 *            frame with h == out_h and w == out_w is converted and copied.  Nothing is interpolated in YUV.
 * yolo4hip/yuv.py: to_rgb is the rule in NumPy.  The arguments are checked on the host as in y4_resize_u8_ragged (NULL pointers,
 * n in 1..65535, H, W > 0, pad_value in 0..255, an output of 2^31 bytes or more: Y4_EINVAL before any launch).  The descriptors
 * live on the device and are NOT checked: the caller owns the table's correctness (every plane inside the source buffer, c_step
 * 1 or 2, y_pitch >= w, c_pitch >= c_step * ceil(w / 2), h, w, out_h, out_w >= 1, the rectangle inside the canvas).  Bytes of the
 * pitch padding are never read. */
int y4_yuv_u8_ragged(const uint8_t* src_dev, const y4_yuv_desc* desc_dev, int n, uint8_t* out_dev, int H, int W, int pad_value,
                     void* stream);
/* ---- VOC mAP matching on the device: the per-image matching of `eval_map` (reference models.py:282-330; yolo4hip/evalmap.py) on
 * the boxes y4_decode_nms(_mapped) left on the device, so that a validation batch returns to the host as flags (yolo4hip/mapeval.py
 * turns them into AP).  No handle.  Per image, one workgroup:
 *   - detections are visited by score descending, slot ascending on ties (ranked here; the NMS output order is not relied upon);
 *   - each is compared with every ground-truth row < gt_count of its own class (int(class) on both sides).  Rows >= gt_count and
 *     slots >= valid may hold anything, NaN included: they are never read;
 *   - IoU with the devkit's inclusive-pixel `+ 1` widths and `iw <= 0 or ih <= 0` as "no overlap", in float64 and in the Python
 *     expression's operation order on the float32 pixel coordinates widened exactly (no contraction): every decision equals
 *     Python's on the same values;
 *   - the best row is the first with the strictly largest IoU (`ov > best` from -1); used rows take part in that choice;
 *   - per threshold t its own walk: true positive iff best >= iou_thresholds[t] and the best row is not yet used at t (it then
 *     is); otherwise a false positive -- no fallback to the second-best row.
 * No atomics; image i's outputs are the same bits at any n and at any position in the batch.
 * Y4_EINVAL: max_total > 256, max_gt > 256, n_thresholds outside 1..16, a negative n / max_total / max_gt, a null pointer.
 * Device counts are clamped to [0, max_total] / [0, max_gt]. */
int y4_map_match(const float* boxes_dev,  /* [n, max_total, 4], x1 y1 x2 y2 normalised: what y4_decode_nms(_mapped) wrote */
                 const float* scores_dev, const float* classes_dev, const int32_t* valid_dev,
                 int n, int max_total,
                 const float* scale_dev,      /* [n, 2] (w, h): pixel box = float32 product box * scale, as export_prediction's `*= w` */
                 const float* gt_dev,         /* [n, max_gt, 5] x1 y1 x2 y2 class, raw-image pixels, annotation order */
                 const int32_t* gt_count_dev, /* [n] */
                 int max_gt,
                 const double* iou_thresholds /* host */, int n_thresholds,
                 uint32_t* tp_mask_dev,   /* [n, max_total]: bit t = true positive at iou_thresholds[t]; 0 in slots >= valid */
                 double* best_iou_dev,    /* [n, max_total] or NULL: IoU of the best same-class box, -1 when none overlaps */
                 int32_t* match_dev,      /* [n, max_total] or NULL: index of that box, -1 */
                 uint32_t* gt_used_dev,   /* [n, max_gt] or NULL: bit t = used at threshold t when the image is done */
                 void* stream);
/* ---- COCO bbox matching on the device: COCOeval's per-image matching without crowd regions, beside the VOC rule above, on the
 * same inputs (yolo4hip/cocoeval.py turns the flags into AP / AR).  No handle.  Per image, one workgroup:
 *   - boxes as above: detection = float32 product box * scale, ground truth = the float32 annotation value, both widened to float64;
 *     all arithmetic float64 in the stated order, no contraction.  area = (x2 - x1) * (y2 - y1);
 *     iw = min(dx2, gx2) - max(dx1, gx1), ih likewise; iw <= 0 or ih <= 0: IoU 0, else i = iw * ih, IoU = i / (da + ga - i).  No `+ 1`;
 *   - per area range [lo, hi] a ground-truth row is ignored when area < lo or area > hi (both strict), a detection is out of range
 *     by the same test on its own area;
 *   - per (range, threshold) one walk over the detections by score descending, slot ascending on ties (a NaN score is never
 *     walked).  A detection takes, among the rows < gt_count of its class (int(class) on both sides) not yet matched in this
 *     walk, the non-ignored row with the largest IoU >= min(thr, 1 - 1e-10), the LAST such row in annotation order on equal IoU;
 *     if there is none, the ignored row chosen by the same rule.  That row is then matched.  The detection is matched, and
 *     ignored iff the row is; an unmatched detection is ignored iff it is out of range;
 *   - cls_rank: the 0-based position of the detection among the image's detections of its class in walk order (the host applies
 *     COCO's maxDets as cls_rank < maxDet: the walk is greedy in score order, so the cut changes no earlier decision).
 * No atomics; image i's outputs are the same bits at any n and at any position in the batch.
 * Y4_EINVAL: max_total > 256, max_gt > 256, n_thresholds outside 1..16, n_areas outside 1..4, a negative n / max_total / max_gt,
 * a null pointer (match_row_dev may be NULL).  Device counts are clamped to [0, max_total] / [0, max_gt]; slots >= valid and
 * rows >= gt_count are never read and are written as 0 / -1. */
int y4_coco_match(const float* boxes_dev,  /* [n, max_total, 4], x1 y1 x2 y2 normalised */
                  const float* scores_dev, const float* classes_dev, const int32_t* valid_dev,
                  int n, int max_total,
                  const float* scale_dev,      /* [n, 2] (w, h) */
                  const float* gt_dev,         /* [n, max_gt, 5] x1 y1 x2 y2 class, raw-image pixels, annotation order */
                  const int32_t* gt_count_dev, /* [n] */
                  int max_gt,
                  const double* area_ranges /* host [n_areas][2]: lo, hi */, int n_areas,
                  const double* iou_thresholds /* host */, int n_thresholds,
                  uint32_t* dt_match_dev,   /* [n, n_areas, max_total]: bit t = matched at iou_thresholds[t] under that range */
                  uint32_t* dt_ignore_dev,  /* [n, n_areas, max_total]: bit t = ignored there */
                  int32_t* cls_rank_dev,    /* [n, max_total]; -1 in slots that are not walked */
                  uint32_t* gt_ignore_dev,  /* [n, max_gt]: bit a = ignored under range a */
                  int32_t* match_row_dev,   /* [n, n_areas, n_thresholds, max_total] or NULL: the matched row, -1 */
                  void* stream);
/* ---- Data-set anchors on the device: IoU k-means (Lloyd steps) and a mutate-and-select evolution over the (w, h) of a data set's
 * label boxes at the network input (yolo4hip/anchors.py drives these; DESIGN.md "Dataset anchors").  No handle, no scratch.
 *   - pair measure iou64(box, anchor): the IoU of the two rectangles centred on each other exactly as y4_loss_assign computes it
 *     (one shared function): half sides (double)(w * 0.5f), box area (double)(w * h), a float32 product, the anchor widened to
 *     float64; intersection, union and quotient in float64, no contraction.  Best anchor: the first arg-max over j = 0 .. k - 1.
 *     The index a box gets here is therefore the anchor y4_loss_assign gives it under the same nine anchors;
 *   - fitness of a set: F = sum over the boxes of llrint(iou64(best) * 2^30), an int64; average IoU = F / n / 2^30;
 *   - Lloyd step: per anchor j over the boxes whose best anchor is j, cnt_j, SW_j = sum llrint((double)w * 2^16), SH_j likewise;
 *     next_j = ((float)((double)SW_j / (double)cnt_j / 65536.0), the same for h); an anchor with cnt_j == 0 keeps its value;
 *   - evolution, generation g: candidate p = fmaxf(best * mult[g][p], 1.0f) elementwise in float32; the winner is the first arg-max
 *     of the P fitness values and replaces best / F_best only if its fitness is strictly larger than F_best (accepted[g] = its
 *     index, else -1).  All G generations are enqueued without a host synchronise: per generation one fitness launch that builds
 *     its candidates from best_dev itself and one select launch.
 * Every sum is an integer sum (order-free): per-wave and per-workgroup partials and one 64-bit integer atomic per accumulator per
 * workgroup.  The same call gives the same bits.  Sides are expected in (0, 16384]: with n <= 2^22 every sum stays below 2^52.
 * Y4_EINVAL before any launch: n outside [1, 2^22], k outside [1, 16], P outside [1, 256], G outside [1, 4096], a null pointer
 * (assign_dev may be NULL), wh_dev or an int64 array not 8-byte aligned. */
int y4_anchor_step(const float* wh_dev,      /* [n, 2] (w, h) */
                   int n,
                   const float* anchors_dev, /* [k, 2] */
                   int k,
                   float* next_dev,          /* [k, 2]: the anchors after this step (not anchors_dev itself) */
                   int64_t* stats_dev,       /* [1 + 3 k]: F, cnt[k], SW[k], SH[k] of anchors_dev */
                   uint8_t* assign_dev,      /* [n] or NULL: the best anchor of every box */
                   void* stream);
int y4_anchor_fitness(const float* wh_dev, int n,
                      const float* sets_dev, /* [P, k, 2] */
                      int P, int k,
                      int64_t* f_dev,        /* [P] */
                      void* stream);
int y4_anchor_evolve(const float* wh_dev, int n,
                     float* best_dev,        /* [k, 2] in / out */
                     int64_t* fbest_dev,     /* [1] in / out: the fitness of best_dev */
                     const float* mult_dev,  /* [G, P, k, 2] */
                     int G, int P, int k,
                     int64_t* fhist_dev,     /* [G, P]: every candidate's fitness */
                     int32_t* accepted_dev,  /* [G]: the winning index, or -1 */
                     void* stream);
/* SPP (custom_layers.py:130-134): x = buf[..., 3c:4c] -> buf[..., 0:c]=maxpool13, [c:2c]=maxpool9,
 * [2c:3c]=maxpool5 (stride 1, 'same'), buf is [n,side,side,4c] */
int y4_spp(int dtype, void* buf_dev, int n, int side, int c, void* stream);
/* The same on an h x w plane (buf is [n,h,w,4c]); y4_spp(..., side, ...) == y4_spp_hw(..., side, side, ...). */
int y4_spp_hw(int dtype, void* buf_dev, int n, int h, int w, int c, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO4HIP_H */
