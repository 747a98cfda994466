// map_match.hip -- y4_map_match: the matching step of VOC mAP (reference models.py:282-330, restated in yolo4hip/evalmap.py
// eval_map) on the boxes y4_decode_nms left on the device, so that a validation batch returns to the host as flags, not as boxes.
//
// Per image (one workgroup of 256 threads; max_total, max_gt <= 256, so a thread owns one detection slot / one ground-truth row):
//   load   slot d < valid: pixel box = float32(normalised box * scale) -- export_prediction's `boxes[:, [0, 2]] *= w` --, score,
//          int(class); row g < gt_count: the four pixel coordinates and int(class).  Slots >= valid and rows >= gt_count are never
//          read: they may hold anything.
//   rank   rank(d) = #{j : score_j > score_d or (score_j == score_d and j < d)}: eval_map's stable descending sort of one image's
//          detections (file order = slot order), computed here -- the NMS output order is not relied upon.
//   pairs  IoU(d, g) for every g of d's class in float64 with the inclusive-pixel `+ 1` widths, in the operation order of
//          evalmap._iou_inclusive (contraction off; the float32 coordinates widen exactly, and a float64 division is correctly
//          rounded), and the first g with the strictly largest IoU (`ov > best` from -1).  The 256 threads are P = 256 / D lanes per
//          detection, D = valid rounded up to a power of two: lane p scans rows p, p + P, ..., and the P partial results are
//          merged by (larger IoU, then smaller row) -- the first strict maximum of the whole scan.
//   walk   lanes t < n_thresholds of wave 0, one per threshold: the detections in rank order, true positive iff
//          best >= thr[t] and the best row is not yet used at t; the row is then used.  No second-best fallback.  Lane t keeps
//          its used bits in LDS words of its own ([row / 32][t]: no two lanes share a word, no bank conflict), the flags of one
//          detection over all thresholds come out of one ballot.
// No atomics, no cross-workgroup traffic: image i's outputs do not depend on n or on its position in the batch.
#include "kernels.h"

#pragma clang fp contract(off)   // keep the Python expression's float64 op order (no fused multiply-add)

namespace y4 {

constexpr int MAP_MAX = 256;     // slots and rows per image = threads of the workgroup
constexpr int MAP_THR = 16;      // thresholds = lanes of the walk

struct MapThresholds {
    double v[MAP_THR];
};

// evalmap._iou_inclusive(bb, gt) on float32 coordinates widened to float64; Python's min(a, b) is `b if b < a else a`
__device__ __forceinline__ double iou_inclusive(const float* bb, const float* gt) {
    const double b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
    const double g0 = gt[0], g1 = gt[1], g2 = gt[2], g3 = gt[3];
    const double iw = (g2 < b2 ? g2 : b2) - (g0 > b0 ? g0 : b0) + 1.0;
    const double ih = (g3 < b3 ? g3 : b3) - (g1 > b1 ? g1 : b1) + 1.0;
    if (iw <= 0.0 || ih <= 0.0) return -1.0;
    const double uni = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - iw * ih;
    return iw * ih / uni;
}

__global__ __launch_bounds__(MAP_MAX) void map_match_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const float* __restrict__ classes, const int32_t* __restrict__ valid,
                                                            int max_total, const float* __restrict__ scale,
                                                            const float* __restrict__ gt, const int32_t* __restrict__ gt_count,
                                                            int max_gt, const MapThresholds thr, int n_thr,
                                                            uint32_t* __restrict__ tp_mask, double* __restrict__ best_iou,
                                                            int32_t* __restrict__ match, uint32_t* __restrict__ gt_used) {
    __shared__ __attribute__((aligned(16))) float det_px[MAP_MAX][4];
    __shared__ __attribute__((aligned(16))) float gt_px[MAP_MAX][4];
    __shared__ float det_score[MAP_MAX];
    __shared__ int det_cls[MAP_MAX], gt_cls[MAP_MAX];
    __shared__ double part_best[MAP_MAX], det_best[MAP_MAX];
    __shared__ int part_match[MAP_MAX], det_match[MAP_MAX];
    __shared__ int rank_slot[MAP_MAX];
    __shared__ uint32_t tp_bits[MAP_MAX];
    __shared__ uint32_t used_w[MAP_MAX / 32][MAP_THR];

    const int t = threadIdx.x;
    const int64_t img = blockIdx.x;
    const int nv = min(max(valid[img], 0), max_total);
    const int ng = min(max(gt_count[img], 0), max_gt);

    if (t < nv) {
        const f32x4_t b = *(const f32x4_t*)(boxes + (img * max_total + t) * 4);
        const float sw = scale[img * 2], sh = scale[img * 2 + 1];
        det_px[t][0] = b[0] * sw; det_px[t][1] = b[1] * sh; det_px[t][2] = b[2] * sw; det_px[t][3] = b[3] * sh;
        det_score[t] = scores[img * max_total + t];
        det_cls[t] = (int)classes[img * max_total + t];
    }
    if (t < ng) {
        const float* row = gt + (img * max_gt + t) * 5;
        gt_px[t][0] = row[0]; gt_px[t][1] = row[1]; gt_px[t][2] = row[2]; gt_px[t][3] = row[3];
        gt_cls[t] = (int)row[4];
    }
    rank_slot[t] = -1;
    tp_bits[t] = 0;
    if (t < (MAP_MAX / 32) * MAP_THR) (&used_w[0][0])[t] = 0;
    __syncthreads();

    // ---- rank: score descending, slot ascending on ties
    if (t < nv) {
        const float s = det_score[t];
        int r = 0;
        for (int j = 0; j < nv; ++j) {
            const float sj = det_score[j];
            r += (sj > s || (sj == s && j < t)) ? 1 : 0;
        }
        rank_slot[r] = t;          // r < nv; a NaN score can only leave ranks empty, which the walk skips
    }

    // ---- pairs: P lanes per detection, lane `part` scans rows part, part + P, ...
    int lg = 0;
    while ((1 << lg) < nv) ++lg;                       // D = 1 << lg >= max(nv, 1), <= 256
    const int D = 1 << lg, P = MAP_MAX >> lg;
    {
        const int d = t & (D - 1), part = t >> lg;
        double best = -1.0;
        int m = -1;
        if (d < nv) {
            const int c = det_cls[d];
            for (int g = part; g < ng; g += P) {
                if (gt_cls[g] != c) continue;
                const double ov = iou_inclusive(det_px[d], gt_px[g]);
                if (ov > best) { best = ov; m = g; }
            }
        }
        part_best[t] = best;                           // [part][d]
        part_match[t] = m;
    }
    __syncthreads();
    if (t < nv) {
        double best = -1.0;
        int m = -1;
        for (int p = 0; p < P; ++p) {
            const double b = part_best[p * D + t];
            const int g = part_match[p * D + t];
            if (g >= 0 && (b > best || (b == best && g < m))) { best = b; m = g; }
        }
        det_best[t] = best;
        det_match[t] = m;
    }
    __syncthreads();

    // ---- walk: one lane per threshold
    if (t < n_thr) {
        double th = 0.0;
#pragma unroll
        for (int i = 0; i < MAP_THR; ++i)
            if (t == i) th = thr.v[i];
        for (int k = 0; k < nv; ++k) {
            const int slot = rank_slot[k];
            if (slot < 0) continue;
            const int g = det_match[slot];
            bool tp = false;
            if (g >= 0) {
                const uint32_t w = used_w[g >> 5][t], bit = 1u << (g & 31);
                tp = det_best[slot] >= th && !(w & bit);
                if (tp) used_w[g >> 5][t] = w | bit;
            }
            const uint64_t flags = __ballot(tp);
            if (t == 0) tp_bits[slot] = (uint32_t)flags;
        }
    }
    __syncthreads();

    if (t < max_total) {
        const int64_t o = img * max_total + t;
        tp_mask[o] = t < nv ? tp_bits[t] : 0u;
        if (best_iou) best_iou[o] = t < nv ? det_best[t] : -1.0;
        if (match) match[o] = t < nv ? det_match[t] : -1;
    }
    if (gt_used && t < max_gt) {
        uint32_t bits = 0;
        for (int i = 0; i < n_thr; ++i) bits |= ((used_w[t >> 5][i] >> (t & 31)) & 1u) << i;
        gt_used[img * max_gt + t] = t < ng ? bits : 0u;
    }
}

int map_match_launch(const float* boxes, const float* scores, const float* classes, const int32_t* valid, int n, int max_total,
                     const float* scale, const float* gt, const int32_t* gt_count, int max_gt, const double* iou_thresholds,
                     int n_thresholds, uint32_t* tp_mask, double* best_iou, int32_t* match, uint32_t* gt_used, hipStream_t stream) {
    Y4_REQUIRE(n >= 0 && max_total >= 0 && max_gt >= 0, Y4_EINVAL, "map_match: negative count (n %d, max_total %d, max_gt %d)", n,
               max_total, max_gt);
    Y4_REQUIRE(max_total <= MAP_MAX, Y4_EINVAL, "map_match: max_total %d > %d", max_total, MAP_MAX);
    Y4_REQUIRE(max_gt <= MAP_MAX, Y4_EINVAL, "map_match: max_gt %d > %d", max_gt, MAP_MAX);
    Y4_REQUIRE(n_thresholds >= 1 && n_thresholds <= MAP_THR, Y4_EINVAL, "map_match: n_thresholds %d outside 1..%d", n_thresholds,
               MAP_THR);
    Y4_REQUIRE(iou_thresholds, Y4_EINVAL, "map_match: null iou_thresholds");
    if (n == 0) return Y4_OK;
    Y4_REQUIRE(valid && scale && gt_count && tp_mask && (max_total == 0 || (boxes && scores && classes)) && (max_gt == 0 || gt),
               Y4_EINVAL, "map_match: null pointer");
    Y4_REQUIRE(((uintptr_t)boxes & 15) == 0, Y4_EINVAL, "map_match: boxes_dev must be 16-byte aligned");
    MapThresholds thr;
    for (int i = 0; i < MAP_THR; ++i) thr.v[i] = i < n_thresholds ? iou_thresholds[i] : 0.0;
    hipLaunchKernelGGL(map_match_kernel, dim3(n), dim3(MAP_MAX), 0, stream, boxes, scores, classes, valid, max_total, scale, gt,
                       gt_count, max_gt, thr, n_thresholds, tp_mask, best_iou, match, gt_used);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
