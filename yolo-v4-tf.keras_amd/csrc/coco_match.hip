// coco_match.hip -- y4_coco_match: the matching step of COCO's bbox protocol (COCOeval.evaluateImg, without crowd regions) on the
// boxes y4_decode_nms / y4_nms_gathered left on the device, beside y4_map_match: a validation batch returns to the host as flags
// (yolo4hip/cocoeval.py turns them into AP / AR), not as boxes.
//
// The rule, per image:
//   boxes  a detection box is the float32 product normalised box * (w, h) -- what y4_map_match forms --, a ground-truth box the
//          float32 annotation value; both widened to float64.  All arithmetic below is float64, contraction off, in this order.
//   area   (x2 - x1) * (y2 - y1).
//   IoU    iw = min(dx2, gx2) - max(dx1, gx1); ih likewise; iw <= 0 or ih <= 0: IoU 0; else i = iw * ih, u = da + ga - i, i / u.
//          No `+ 1`.
//   ignore per area range [lo, hi] a ground-truth row is ignored when area < lo or area > hi (both strict: an area of exactly
//          1024 belongs to small AND medium); a detection is out of range by the same test on its own area.
//   match  per (range, threshold thr) its own walk over the detections by score descending, slot ascending on ties.  Detection d
//          takes, among the rows of its class NOT YET MATCHED in this walk, the non-ignored row with the largest
//          IoU >= min(thr, 1 - 1e-10), the LAST such row in annotation order on equal IoU; if there is none, the ignored row
//          chosen by the same rule.  The row is then matched; d is matched, and ignored iff the row is.  An unmatched d is
//          ignored iff it is out of range.  (COCOeval's loop -- rows stably sorted by the ignore flag, `iou >= best`, break at the
//          first ignored row once a non-ignored one is held -- takes the same decisions.)
//   rank   cls_rank[d]: 0-based position of d among the image's detections of its class in walk order.  COCO cuts each
//          (image, class) list to maxDet; the walk is greedy in score order, so a later cut changes no earlier decision: the
//          kernel matches once and the host keeps cls_rank < maxDet.
//
// Per image one workgroup of 256 threads (max_total, max_gt <= 256: a thread owns one detection slot / one ground-truth row):
//   load   as map_match_kernel: slots < valid, rows < gt_count; the rest is never read.  Areas and the per-range flags here too.
//   rank   walk position and class rank by counting; a NaN score is never walked (cls_rank -1).
//   walk   n_areas * n_thresholds <= 64 walks = the lanes of wave 0, lane a * n_thresholds + t, each with its matched-row bits in
//          LDS words of its own ([row / 32][lane]).  All lanes visit the same (detection, row) pairs in the same order and differ
//          only in ignore flag and threshold, so a pair's IoU is needed once per workgroup: for the detection at walk position k
//          all 256 threads -- thread g for row g -- write its IoU row and the ballot of its candidate rows (same class,
//          IoU >= the smallest threshold) into buffer k & 1, one barrier, and wave 0 walks position k over the set bits while the
//          other three waves are already at position k + 1's row (the buffer wave 0 reads is next written two barriers later).
// No atomics, no cross-workgroup traffic: image i's outputs do not depend on n or on its position in the batch.
#include "kernels.h"

#pragma clang fp contract(off)   // keep the stated float64 op order (no fused multiply-add)

namespace y4 {

constexpr int COCO_MAX = 256;    // slots and rows per image = threads of the workgroup
constexpr int COCO_THR = 16;     // thresholds per range
constexpr int COCO_AREAS = 4;    // area ranges
constexpr int COCO_LANES = 64;   // walks = lanes of wave 0

struct CocoParams {
    double thr[COCO_THR];        // min(thr, 1 - 1e-10) already
    double lo[COCO_AREAS], hi[COCO_AREAS];
    double thr_min;              // the smallest of thr[]
};

__global__ __launch_bounds__(COCO_MAX) void coco_match_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                              const float* __restrict__ classes, const int32_t* __restrict__ valid,
                                                              int max_total, const float* __restrict__ scale,
                                                              const float* __restrict__ gt, const int32_t* __restrict__ gt_count,
                                                              int max_gt, const CocoParams prm, int n_thr, int n_areas,
                                                              uint32_t* __restrict__ dt_match, uint32_t* __restrict__ dt_ignore,
                                                              int32_t* __restrict__ cls_rank, uint32_t* __restrict__ gt_ignore,
                                                              int32_t* __restrict__ match_row) {
    __shared__ __attribute__((aligned(16))) float det_px[COCO_MAX][4];
    __shared__ double det_area[COCO_MAX];
    __shared__ float det_score[COCO_MAX];
    __shared__ int det_cls[COCO_MAX], gt_cls[COCO_MAX];
    __shared__ int rank_slot[COCO_MAX], det_crank[COCO_MAX];
    __shared__ uint32_t det_oor[COCO_MAX], gt_ign[COCO_MAX];            // bit a: out of range / ignored under range a
    __shared__ double iou_row[2][COCO_MAX];
    __shared__ uint64_t cand[2][COCO_MAX / 64];
    __shared__ uint32_t used_w[COCO_MAX / 32][COCO_LANES];
    __shared__ uint32_t dtm[COCO_AREAS][COCO_MAX], dti[COCO_AREAS][COCO_MAX];

    const int t = threadIdx.x;
    const int64_t img = blockIdx.x;
    const int nv = min(max(valid[img], 0), max_total);
    const int ng = min(max(gt_count[img], 0), max_gt);

    // ---- load: this thread's detection slot and its ground-truth row (the row stays in registers: thread g serves row g)
    float s = 0.f;
    if (t < nv) {
        const f32x4_t b = *(const f32x4_t*)(boxes + (img * max_total + t) * 4);
        const float sw = scale[img * 2], sh = scale[img * 2 + 1];
        const float x1 = b[0] * sw, y1 = b[1] * sh, x2 = b[2] * sw, y2 = b[3] * sh;
        det_px[t][0] = x1; det_px[t][1] = y1; det_px[t][2] = x2; det_px[t][3] = y2;
        const double area = ((double)x2 - (double)x1) * ((double)y2 - (double)y1);
        det_area[t] = area;
        uint32_t oor = 0;
#pragma unroll
        for (int a = 0; a < COCO_AREAS; ++a)
            if (a < n_areas && (area < prm.lo[a] || area > prm.hi[a])) oor |= 1u << a;
        det_oor[t] = oor;
        s = scores[img * max_total + t];
        det_score[t] = s;
        det_cls[t] = (int)classes[img * max_total + t];
    }
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, ga = 0.0;
    int gc = -1;
    uint32_t gign = 0;
    if (t < ng) {
        const float* row = gt + (img * max_gt + t) * 5;
        g0 = row[0]; g1 = row[1]; g2 = row[2]; g3 = row[3];
        gc = (int)row[4];
        ga = (g2 - g0) * (g3 - g1);
#pragma unroll
        for (int a = 0; a < COCO_AREAS; ++a)
            if (a < n_areas && (ga < prm.lo[a] || ga > prm.hi[a])) gign |= 1u << a;
    }
    gt_cls[t] = gc;
    gt_ign[t] = gign;
    rank_slot[t] = -1;
    det_crank[t] = -1;
#pragma unroll
    for (int a = 0; a < COCO_AREAS; ++a) { dtm[a][t] = 0; dti[a][t] = 0; }
    for (int i = t; i < (COCO_MAX / 32) * COCO_LANES; i += COCO_MAX) (&used_w[0][0])[i] = 0;
    __syncthreads();

    // ---- rank: score descending, slot ascending on ties; over the whole image and within the class.  A NaN score compares false
    //      both ways: it is counted by nobody and takes no rank, so the ranks 0 .. (walked - 1) are all filled
    if (t < nv && s == s) {
        const int c = det_cls[t];
        int r = 0, rc = 0;
        for (int j = 0; j < nv; ++j) {
            const float sj = det_score[j];
            const int before = (sj > s || (sj == s && j < t)) ? 1 : 0;
            r += before;
            rc += before & (det_cls[j] == c ? 1 : 0);
        }
        rank_slot[r] = t;
        det_crank[t] = rc;
    }
    __syncthreads();

    // ---- walk
    const int n_lanes = n_thr * n_areas;
    const bool live = t < n_lanes;
    const int la = live ? t / n_thr : 0, lt = live ? t % n_thr : 0;
    double th = 2.0;
#pragma unroll
    for (int i = 0; i < COCO_THR; ++i)
        if (lt == i) th = prm.thr[i];
    const uint32_t tmask = n_thr >= 32 ? 0xFFFFFFFFu : ((1u << n_thr) - 1u);

    for (int k = 0; k < nv; ++k) {
        const int slot = rank_slot[k];                 // the same value in every thread
        if (slot < 0) break;                           // walked < nv: NaN scores
        const int buf = k & 1;
        {   // thread t = row t of this detection's IoU row
            double v = 0.0;
            bool c = false;
            if (t < ng && gc == det_cls[slot]) {
                const double d0 = det_px[slot][0], d1 = det_px[slot][1], d2 = det_px[slot][2], d3 = det_px[slot][3];
                const double iw = (g2 < d2 ? g2 : d2) - (g0 > d0 ? g0 : d0);
                const double ih = (g3 < d3 ? g3 : d3) - (g1 > d1 ? g1 : d1);
                if (iw > 0.0 && ih > 0.0) {
                    const double i = iw * ih;
                    const double u = det_area[slot] + ga - i;
                    v = i / u;
                }
                c = v >= prm.thr_min;
            }
            iou_row[buf][t] = v;
            const uint64_t m = __ballot(c);
            if ((t & 63) == 0) cand[buf][t >> 6] = m;
        }
        __syncthreads();
        if (t < COCO_LANES) {
            double bn = th, bi = th;
            int mn = -1, mi = -1;
            for (int w = 0; w < COCO_MAX / 64; ++w) {
                uint64_t cm = cand[buf][w];
                while (cm) {
                    const int g = w * 64 + __builtin_ctzll(cm);
                    cm &= cm - 1;
                    if (!live || ((used_w[g >> 5][t] >> (g & 31)) & 1u)) continue;
                    const double v = iou_row[buf][g];
                    if ((gt_ign[g] >> la) & 1u) {
                        if (v >= bi) { bi = v; mi = g; }
                    } else {
                        if (v >= bn) { bn = v; mn = g; }
                    }
                }
            }
            const int m = mn >= 0 ? mn : mi;
            const bool matched = live && m >= 0;
            bool ignored = false;
            if (matched) {
                used_w[m >> 5][t] |= 1u << (m & 31);
                ignored = (gt_ign[m] >> la) & 1u;
            } else if (live) {
                ignored = (det_oor[slot] >> la) & 1u;
            }
            const uint64_t mb = __ballot(matched), ib = __ballot(ignored);
            if (t < n_areas) {
                dtm[t][slot] = (uint32_t)(mb >> (t * n_thr)) & tmask;
                dti[t][slot] = (uint32_t)(ib >> (t * n_thr)) & tmask;
            }
            if (match_row && live) match_row[(img * n_lanes + t) * max_total + slot] = m;
        }
    }
    __syncthreads();

    if (t < max_total) {
        for (int a = 0; a < n_areas; ++a) {
            const int64_t o = (img * n_areas + a) * max_total + t;
            dt_match[o] = dtm[a][t];                   // zero where nothing was walked
            dt_ignore[o] = dti[a][t];
        }
        const int cr = det_crank[t];
        cls_rank[img * max_total + t] = cr;
        if (match_row && cr < 0)                       // not walked: no lane wrote this slot
            for (int l = 0; l < n_lanes; ++l) match_row[(img * n_lanes + l) * max_total + t] = -1;
    }
    if (t < max_gt) gt_ignore[img * max_gt + t] = gign;   // zero in rows >= gt_count
}

int coco_match_launch(const float* boxes, const float* scores, const float* classes, const int32_t* valid, int n, int max_total,
                      const float* scale, const float* gt, const int32_t* gt_count, int max_gt, const double* area_ranges,
                      int n_areas, const double* iou_thresholds, int n_thresholds, uint32_t* dt_match, uint32_t* dt_ignore,
                      int32_t* cls_rank, uint32_t* gt_ignore, int32_t* match_row, hipStream_t stream) {
    Y4_REQUIRE(n >= 0 && max_total >= 0 && max_gt >= 0, Y4_EINVAL, "coco_match: negative count (n %d, max_total %d, max_gt %d)", n,
               max_total, max_gt);
    Y4_REQUIRE(max_total <= COCO_MAX, Y4_EINVAL, "coco_match: max_total %d > %d", max_total, COCO_MAX);
    Y4_REQUIRE(max_gt <= COCO_MAX, Y4_EINVAL, "coco_match: max_gt %d > %d", max_gt, COCO_MAX);
    Y4_REQUIRE(n_thresholds >= 1 && n_thresholds <= COCO_THR, Y4_EINVAL, "coco_match: n_thresholds %d outside 1..%d", n_thresholds,
               COCO_THR);
    Y4_REQUIRE(n_areas >= 1 && n_areas <= COCO_AREAS, Y4_EINVAL, "coco_match: n_areas %d outside 1..%d", n_areas, COCO_AREAS);
    Y4_REQUIRE(iou_thresholds, Y4_EINVAL, "coco_match: null iou_thresholds");
    Y4_REQUIRE(area_ranges, Y4_EINVAL, "coco_match: null area_ranges");
    if (n == 0) return Y4_OK;
    Y4_REQUIRE(valid && scale && gt_count && dt_match && dt_ignore && cls_rank && gt_ignore &&
                   (max_total == 0 || (boxes && scores && classes)) && (max_gt == 0 || gt),
               Y4_EINVAL, "coco_match: null pointer");
    Y4_REQUIRE(((uintptr_t)boxes & 15) == 0, Y4_EINVAL, "coco_match: boxes_dev must be 16-byte aligned");
    CocoParams prm;
    const double cap = 1.0 - 1e-10;
    prm.thr_min = 2.0;
    for (int i = 0; i < COCO_THR; ++i) {
        prm.thr[i] = 2.0;
        if (i < n_thresholds) {
            prm.thr[i] = iou_thresholds[i] < cap ? iou_thresholds[i] : cap;
            if (prm.thr[i] < prm.thr_min) prm.thr_min = prm.thr[i];
        }
    }
    for (int a = 0; a < COCO_AREAS; ++a) {
        prm.lo[a] = a < n_areas ? area_ranges[2 * a] : 0.0;
        prm.hi[a] = a < n_areas ? area_ranges[2 * a + 1] : 0.0;
    }
    hipLaunchKernelGGL(coco_match_kernel, dim3(n), dim3(COCO_MAX), 0, stream, boxes, scores, classes, valid, max_total, scale, gt,
                       gt_count, max_gt, prm, n_thresholds, n_areas, dt_match, dt_ignore, cls_rank, gt_ignore, match_row);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
