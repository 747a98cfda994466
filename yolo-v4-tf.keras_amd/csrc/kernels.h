// kernels.h -- launch-side interface between runtime.hip and the kernel files.
#pragma once
#include <initializer_list>

#include "common.h"

namespace y4 {

// conv_igemm.hip
// 1x1 convs chained onto a conv's register tile (conv_chain.h); d->out is then the head conv's own output view,
// written only if store_x, and the last tail writes `fin`.  16-bit dtypes, head cout == 64, Mish everywhere.
struct ConvChainDesc {
    int ntail, store_x;            // (concat_only: ntail = 2 with tail[0] unused -- the head feeds the conv over the concat directly)
    int concat_only;
    struct {
        const void* w;             // pack_tail_weights layout
        const float* scale;
        const float* shift;
        const void* src2;          // concat partner slice (64 channels) or null
        int src2_cstride, src2_coff, cout;
    } tail[2];
    void* fin;
    int fin_cstride, fin_coff;
};
// LDS pair: a following 1x1 conv with at most as many output channels as the head (128 or 256) runs from the head's
// tile kept in LDS.  `w` = that conv's ordinary packed weights; d->out is written only if store_x.
struct ConvPairDesc {
    const void* w;
    const float* scale;
    const float* shift;
    int act, cout, out_f32, store_x;
    void* fin;
    int fin_cstride, fin_coff;
    void* fin2;                    // tail = a fused CSP pair (cout = both convs' rows): rows >= split go here
    int fin2_cstride, fin2_coff, split;
};
// A head conv (float32 raw logits) also leaves its three OBJECTNESS logits per cell -- channels a * nf + 4 -- in a dense side
// array [image][cell of the image, the three scales back to back][4] (one 16-byte slot per cell), which is what decode's screen
// reads instead of three 64-byte sectors of the 1 KB cell (decode_nms.hip).  The written values are the stored logits themselves.
struct ConvObjDesc {
    float* obj;                    // slot of this launch's first image's first cell
    int nf, cells_per_img, cell_base;
};
int conv2d_launch(const y4_conv_desc* d, const char* zero_page, hipStream_t stream, const ConvChainDesc* chain = nullptr,
                  const ConvPairDesc* pair = nullptr, const ConvObjDesc* obj = nullptr);
int pack_tail_weights(int dtype, int cout, int cin, const float* oihw, void* packed, hipStream_t stream);
// (cout, cin, k, k) float32 -> 16-bit A fragments of the 16x16x32 MFMA in the canonical K order: THE fragment order of the chain
// tails, the stage blob and the residual-block blobs (layout: at pack_frag16_kernel, conv_igemm.hip)
int pack_frag16(int dtype, int cout, int cin, int ksize, const float* oihw, void* dst, hipStream_t stream);
// up to four tables of c <= 128 floats (scale, shift, scale, shift) -> consecutive slots of c floats: a blob's affine part
int copy_affine(int c, std::initializer_list<const float*> src, float* dst, hipStream_t stream);
int conv_tile_count();
bool weight_touch_enabled();          // conv_common.h: weight_touch (off with Y4_NO_WEIGHT_TOUCH=1, for A/B runs)
int conv_pick_tile(int dtype, int M, int cin, int cout);
int pack_conv_weights(int dtype, int cout, int cin, int ksize, const float* oihw, void* packed, hipStream_t stream);
// 3x3 packed weights -> MFMA-fragment order of the halo2 tiles (conv_halo2_kernel.h); same byte count
int pack_conv_frag32(int dtype, int cout, int cin, const void* packed, void* frag, hipStream_t stream);

// misc_kernels.hip
int stem_conv_launch(int dtype, const void* imgs, int img_u8, int n, int h, int w, const float* wk, const float* scale,
                     const float* shift, int cout, int act, void* out, int out_cstride, int out_coff, hipStream_t stream);
int resize_u8_launch(const uint8_t* img, int n, int h, int w, uint8_t* out, int H, int W, hipStream_t stream);
int pack_stem_weights(const float* w_oihw, float* wk, int cout, hipStream_t stream);
int preprocess_u8_launch(const uint8_t* img, int h, int w, float* out, int H, int W, hipStream_t stream);
int spp_launch(int dtype, void* buf, int n, int h, int w, int c, hipStream_t stream);
int view_to_f32_launch(int dtype, const void* src, float* dst, int64_t pixels, int cstride, int coff, int c,
                       hipStream_t stream);
int f32_to_view_launch(const float* src, float* dst, int64_t pixels, int cstride, int c, hipStream_t stream);
int fold_bn_launch(const float* rec, float* scale, float* shift, int cout, int cout_pad, int has_bn, hipStream_t stream);

// canvas_u8.hip: packed uint8 sources + a device-resident descriptor table -> the uint8 network batch, one kernel template
int resize_u8_ragged_launch(const uint8_t* src, const y4_image_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                            hipStream_t stream);
int window_u8_ragged_launch(const uint8_t* src, const y4_window_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                            hipStream_t stream);
int view_u8_ragged_launch(const uint8_t* src, const y4_view_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                          hipStream_t stream);
int augment_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                             hipStream_t stream);
int mosaic_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* tiles, const y4_mosaic_cut* cuts, int n, uint8_t* out, int H,
                            int W, int pad, hipStream_t stream);
// yuv_u8.hip: the same template on 8-bit 4:2:0 video frames, converted to RGB tap by tap
int yuv_u8_ragged_launch(const uint8_t* src, const y4_yuv_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                         hipStream_t stream);

// map_match.hip: VOC mAP matching of kept boxes against ground truth, one workgroup per image
int map_match_launch(const float* boxes, const float* scores, const float* classes, const int32_t* valid, int n, int max_total,
                     const float* scale, const float* gt, const int32_t* gt_count, int max_gt, const double* iou_thresholds,
                     int n_thresholds, uint32_t* tp_mask, double* best_iou, int32_t* match, uint32_t* gt_used, hipStream_t stream);

// coco_match.hip: COCO bbox matching (area ranges, ignore flags, matched rows leave the pool), one workgroup per image
int coco_match_launch(const float* boxes, const float* scores, const float* classes, const int32_t* valid, int n, int max_total,
                      const float* scale, const float* gt, const int32_t* gt_count, int max_gt, const double* area_ranges,
                      int n_areas, const double* iou_thresholds, int n_thresholds, uint32_t* dt_match, uint32_t* dt_ignore,
                      int32_t* cls_rank, uint32_t* gt_ignore, int32_t* match_row, hipStream_t stream);

// anchors.hip: the data-set anchor search -- one Lloyd step, the fitness of P anchor sets, G generations of mutate-and-select
int anchor_step_launch(const float* wh, int n, const float* anchors, int k, float* next, int64_t* stats, uint8_t* assign,
                       hipStream_t stream);
int anchor_fitness_launch(const float* wh, int n, const float* sets, int P, int k, int64_t* f, hipStream_t stream);
int anchor_evolve_launch(const float* wh, int n, float* best, int64_t* fbest, const float* mult, int G, int P, int k,
                         int64_t* fhist, int32_t* accepted, hipStream_t stream);

// stem_down.hip: convs 0+1 fused (16-bit dtypes), c0 stays in LDS
bool stem_down_supported(int dtype, int S);
int stem_down_launch(int dtype, const void* imgs, int img_u8, int n, int S, const void* stem_wk, const float* s0_scale,
                     const float* s0_shift, int act0, const void* w1_packed, const float* s1_scale, const float* s1_shift,
                     int act1, void* out, int out_cstride, int out_coff, hipStream_t stream);

// csp_stage.hip: convs 2..7 (the first CSP stage) as one spatially tiled persistent kernel (16-bit dtypes)
bool csp_stage_supported(int dtype, int h, int w);
size_t csp_stage_blob_bytes();
int pack_csp_stage(int dtype, const float* const* w, const float* const* scale, const float* const* shift, void* blob,
                   hipStream_t stream);
int csp_stage_launch(int dtype, const void* in, int n, int h, int w, int in_cstride, int in_coff, const void* blob, void* out,
                     int out_cstride, int out_coff, hipStream_t stream);

// resblock.hip: "1x1 conv -> 3x3 conv + Add" residual blocks with 64 / 128 channels as one spatially tiled kernel
bool resblock_supported(int dtype, int c);
size_t resblock_blob_bytes(int c);
int pack_resblock(int dtype, int c, const float* w1, const float* scale1, const float* shift1, const float* w3, const float* scale3,
                  const float* shift3, void* blob, hipStream_t stream);
int resblock_launch(int dtype, int c, const void* in, int n, int h, int w, int in_cstride, int in_coff, const void* blob, void* out,
                    int out_cstride, int out_coff, hipStream_t stream);
// host only: the tile table of an (n, h, w) map with c channels on `slots` workgroups, as the kernel reads it (y4_rb_tile_table)
int rb_tile_table(int n, int h, int w, int c, int slots, int32_t* out, int cap);

// decode_nms.hip
// Per-image candidate counters are spaced one per 256 bytes: packed into one cache line, the ~10^3 appends per
// image of a whole batch serialise on a single L2 line (measured: decode 195 us -> see DESIGN.md).
constexpr int COUNT_STRIDE = 64;     // uint32 words
struct DecodeK {
    const float* head[3];
    int gh[3], gw[3], stride[3], box_off[3];   // grid rows (over H) / columns (over W) per scale
    float xyscale[3], xyoff[3];      // xyoff = float(0.5*(xyscale-1)) computed in double like the reference
    float anchors[18];
    int cells_per_img;               // gh0*gw0 + gh1*gw1 + gh2*gw2
    int N, C, hcs, nbox;
    float img_h, img_w, score_thr;   // x1, x2 are divided by img_w, y1, y2 by img_h
    float* dboxes;                   // [N, nbox, 4] normalised x1,y1,x2,y2
    unsigned long long* keys;        // [N, cap]
    uint32_t* counts;                // [N * COUNT_STRIDE]: one counter per image, each on its own 256-byte line
    uint32_t cap;
    FastDiv div_cells, div_gw[3];    // cell id -> image, cell -> row (ids < 2^31: checked at y4_create)
    const float* obj;                // [N * cells_per_img][4]: the cells' objectness logits as the head convs left them (ConvObjDesc), or null
};
struct NmsK {
    const float* dboxes;             // [N, nbox, 4]
    const unsigned long long* keys;  // [N, cap]
    uint32_t* counts;                // [N * COUNT_STRIDE]; a block resets its image's counter once it has read it
    uint32_t cap;
    int N, C, nbox, max_total, max_per_class;
    float iou_thr;
    float* out_boxes;                // [N, max_total, 4]
    float* out_scores;               // [N, max_total]
    float* out_classes;              // [N, max_total]
    int32_t* out_valid;              // [N]
    int32_t* out_idx;                // [N, max_total] or null
    uint32_t* status;                // [1] bit0: candidate list overflowed its capacity
    FastDiv div_c;                   // id -> (box, class) without integer division (ids < 2^31 checked at y4_create)
    const float* box_map;            // [N][4] {ax, bx, ay, by} applied to the kept boxes before the clip, or null (identity)
    int kind;                        // y4_set_nms_rule: 0 suppress iff IoU > iou_thr, 1 iff IoU - (d2 / c2)^beta > iou_thr (DIoU-NMS)
    float beta;                      // (kind 1 only)
    int agnostic;                    // 1: a kept box suppresses later candidates of every class
};
int decode_launch(const DecodeK& k, hipStream_t stream, int clear_images);
// tuner aid (latency schedules): streams `bytes` of `p` through the L2s so that the next launch starts on cold weights
int l2_flush_launch(const void* p, size_t bytes, void* sink, hipStream_t stream);
int nms_launch(const NmsK& k, hipStream_t stream);

// soft_nms.hip (y4_set_nms_soft) and matrix_nms.hip (y4_set_nms_matrix): score decay over the same lists, with the same outputs,
// counter reset and status bit as nms_kernel (nms_list_begin).  The mode travels beside NmsK, which nms_kernel keeps as it is.
struct DecayK {
    int method;                      // soft: 1 gaussian, 2 linear, 3 hard; matrix: 1 gaussian, 2 linear (0, off, never gets here: nms_over)
    float sigma;                     // gaussian.  soft: w *= expf(-(m * m) / sigma); matrix: t = expf((c * c - m * m) / sigma)
    float min_score;                 // resolved, >= 0.  soft: a candidate takes part while its working score is > min_score;
                                     // matrix: a candidate is a result only if its decayed score is > min_score
    int top_k;                       // participants: the top_k largest keys of the list, 1 .. SORT_CAP
};
int soft_nms_launch(const NmsK& k, const DecayK& s, hipStream_t stream);
int matrix_nms_launch(const NmsK& k, const DecayK& s, hipStream_t stream);

// tiled.hip: the decode stage's per-row candidate lists -> one list per group
struct GatherK {
    const float* dboxes;             // [n, nbox, 4] what the decode stage wrote (canvas-normalised)
    const unsigned long long* keys;  // [n, cap]
    uint32_t* counts;                // [n * COUNT_STRIDE]; the row's workgroup resets its counter once it has read it
    uint32_t cap;
    int C, nbox;
    const int32_t* row_group;        // [n] group of a row
    const int32_t* row_slot;         // [n] its slot in the group's box table
    const float* row_map;            // [n][4] {ax, bx, ay, by}: canvas-normalised -> group-normalised
    int n_groups, max_slots;
    uint32_t group_cap;
    unsigned long long* gkeys;       // [n_groups, group_cap]
    float* gboxes;                   // [n_groups, max_slots * nbox, 4]
    uint32_t* gcounts;               // [n_groups * COUNT_STRIDE]
    uint32_t* status;                // [1] bit0, as NmsK
    FastDiv div_c;
};
// oriented (y4_decode_gather_views): an axis whose scale is negative reads its two corners swapped, so x1 <= x2 stays
int gather_launch(const GatherK& k, int n, bool oriented, hipStream_t stream);
int gather_counts_launch(const uint32_t* gcounts, int32_t* out, int n_groups, hipStream_t stream);

// box_merge.hip: merge-NMS (box voting) behind nms_kernel -- each kept box becomes the score-weighted mean of the candidates of
// its list that it absorbed.  Reads the candidate store nms_kernel read and the outputs it wrote; rewrites kept boxes only.
constexpr uint32_t MERGE_MAX_CAP = 1u << 25;   // list capacities below this keep the int64 sums in range (box_merge.hip)
struct MergeK {
    const float* dboxes;             // [N, nbox, 4] the unclipped boxes the pair measure is taken on
    const unsigned long long* keys;  // [N, cap]
    const int32_t* counts;           // [N] dense: the lists' raw counts, saved before nms_kernel zeroed the counters
    uint32_t cap;
    int N, C, nbox, max_total;
    float iou_thr;
    float* out_boxes;                // [N, max_total, 4] nms_kernel's boxes; the first out_valid[n] are rewritten
    const float* out_scores;         // [N, max_total]
    const float* out_classes;        // [N, max_total]
    const int32_t* out_valid;        // [N]
    const int32_t* out_idx;          // [N, max_total] box index of every kept box
    FastDiv div_c;
    const float* box_map;            // as NmsK: applied to the mean before the clip, or null
    int kind;                        // the handle's rule, as NmsK
    float beta;
    int agnostic;
};
int box_merge_launch(const MergeK& k, hipStream_t stream);

// loss.hip: the reference's yolo_loss forward over the raw heads, and the label assignment as responsible-cell records
// (record: int32 words [scale, row, col, anchor, bits of x, y, w, h, class mask words]; sorted by (scale, row, col, anchor))
struct LossAssignK {
    const float* boxes;              // [n, mb, 5] x1, y1, x2, y2, class in network-input pixels
    float* xywh;                     // [n, mb, 4] floor-centre x, y and w, h of every row
    int32_t* records;                // [n, mb, rw]
    int32_t* counts;                 // [n] records of the image, or -1: a used row is off the grid / has no such class
    int mb, rw, mw, C;
    int img_h, img_w;
    int gh[3], gw[3], lane_base[3];  // lane_base: first (cell, anchor) index of a scale among the image's 3 * cells lanes
    float anchors[18];
};
// what the loss forward and its gradients read: the raw heads in the workspace, the 256-lane strips, and one batch's labels
struct LossIn {
    const float* head[3];
    int gh[3], gw[3], strip_base[3], strips;   // strips: 256-lane workgroups per image, strip_base: the first one of a scale
    float stride[3], anchors[18];
    int C, hcs, mb, rw;
    float thresh, input_area;
    const int32_t* records;          // [n, mb, rw]
    const int32_t* counts;           // [n]
    const float* xywh;               // [n, mb, 4]
    const float* imgw;               // [n] weight of each image's loss (1 / N: the batch mean); null for the forward
    int box_kind;                    // the box term of a responsible lane: BOX_GIOU (loss.py:34-60) or BOX_CIOU (loss.py:63-113)
};
enum { BOX_GIOU = 0, BOX_CIOU = 1 };
struct LossK : LossIn {
    float* partials;                 // [n, strips, 3]
    float* out;                      // [n, 3 scales, 3] box, confidence, class sums
};
int loss_strips(const int* gh, const int* gw, int* strip_base);
int loss_assign_launch(const LossAssignK& k, int n, hipStream_t stream);
int loss_launch(const LossK& k, int n, hipStream_t stream);

// head_train.hip: the gradient of yolo_loss w.r.t. the raw heads, the weight gradient of the three head convs, Adam
struct GradK : LossIn {
    float* dense[3];                 // y4_loss_grad: [n, gh, gw, 3 (5 + C)] per scale
    // y4_head_grad
    const void* x[3];                // the head convs' inputs, dense NHWC [n, gh, gw, cin] in the handle's dtype
    int cin[3];
    int pstrip_base[3], pstrips[3];  // 64-cell strips of one image: the first one of a scale, their number per scale
    size_t part_base[3];             // float offset of a scale's strip partials [n, pstrips, 3 cin + 4] in `partials`
    float* partials;
    float* dw;                       // the three records [cout biases][cout x cin], conv 93 / 101 / 109 at dw_off
    size_t dw_off[3];
    int accumulate;
};
int head_grad_strips(const int* gh, const int* gw, int* pstrip_base, int* pstrips);
size_t head_grad_scratch_floats(const int* gh, const int* gw, const int* cin, int n, size_t* part_base);
int loss_grad_launch(const GradK& k, int n, hipStream_t stream);
int head_grad_launch(int dtype, const GradK& k, int n, hipStream_t stream);
int adam_launch(const float* g, float* w, float* m, float* v, size_t count, float lr_t, float b1, float b2, float eps, hipStream_t stream);

// block_train.hip: the gradient of the 3x3 convs in front of the heads (92 / 100 / 108); labels and heads travel in a GradK
struct BlockK {
    const void* u[3];                // the 3x3 convs' inputs, dense NHWC [n, gh, gw, cin] in the handle's dtype
    const void* a[3];                // their outputs (the head convs' inputs), dense NHWC [n, gh, gw, cout]
    const void* wh[3];               // the head convs' packed weights [3 (5 + C) rows][cout]
    const float* bn_scale[3];        // gamma / sqrt(var + eps) as fold_bn left it
    int cin[3], cout[3];
    int dstrip_base[3];              // 16-cell strips of one image: the first one of a scale
    void* dz[3];                     // scratch: dZ [n, gh, gw, cout] in the handle's dtype
    float* part[3];                  // scratch: wgrad partials [splits][9][cout][cin]
    float* dk;                       // the three kernels (out, in, kh, kw), conv 92 / 100 / 108 at dk_off
    size_t dk_off[3];
    int accumulate;
    float loss_scale;                // a power of two: dZ is stored times it, the summed dK divided by it
    int32_t* overflow;               // bit 0: an inf / NaN in the stored dZ, bit 1: a non-finite sum; ORed into, may be null
};
struct WgradK {
    const void* u;
    const void* dz;
    float* part;
    int n, H, W, cin, cout;
    int R, strips, slices, splits;   // rows of a K slice, slices per image, slices in all, contiguous slice ranges (= partials)
    int Wp, upitch, uchan, dchan;    // LDS image: padded row length of dZ, row pitch of U, channel pitches (elements)
};
int block_dgrad_strips(const int* gh, const int* gw, int* base);
size_t block_wgrad_geometry(int dtype, int n, int H, int W, int cin, int cout, WgradK& k);
size_t block_grad_scratch_bytes(int dtype, int n, const int* gh, const int* gw, const int* cin, const int* cout, size_t* dz_off,
                                size_t* part_off);
int block_grad_launch(int dtype, const GradK& k, const BlockK& b, int n, hipStream_t stream);

// feature_cache.hip: the retained tensors of a batch <-> dense cache rows, in 16-byte chunks.  A row is the three scales' tensors
// back to back; chunk r of a row belongs to the scale k with first[k] <= r, lies at chunk (r - first[k]) of that scale's
// tensor, i.e. in pixel (r - first[k]) / cpp[k] of the view, and at byte off[k] + 16 (r - first[k]) of the row.
constexpr int FEATURE_MAX_IMAGES = 256;      // images of one launch: their slots travel in the kernel argument
struct FeatureK {
    char* view[3];                   // the view's buffer at batch position 0
    uint64_t img_stride[3];          // bytes from one batch position of the buffer to the next
    uint32_t pix_stride[3], coff[3]; // bytes from one pixel to the next, and of the view's first channel
    uint32_t first[3];               // a scale's first chunk in the row (first[0] = 0)
    uint32_t off[3];                 // a scale's byte offset in the row
    FastDiv cpp[3];                  // chunks of one pixel (channels * element size / 16)
    FastDiv row;                     // chunks of a row without its padding; d = their number
    uint32_t total;                  // chunks of the launch: images * row.d < 2^31
    uint64_t row_bytes;
    char* cache;
    int32_t slot[FEATURE_MAX_IMAGES];
};
int feature_copy_launch(const FeatureK& k, bool store, hipStream_t stream);

}  // namespace y4
