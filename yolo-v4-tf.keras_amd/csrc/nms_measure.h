// nms_measure.h -- the pair measure of the NMS stage, the single copy: nms_kernel (decode_nms.hip) suppresses with it and
// box_merge_kernel (box_merge.hip) decides with it which candidates a kept box absorbed.  Device code; float32 in this operation
// order on both sides.
#pragma once
#include "common.h"

#pragma clang fp contract(off)   // keep the reference's float32 op order (no fused multiply-add)

namespace y4 {

__device__ __forceinline__ float iou_tf(const float4 a, const float4 b) {
    const float ay0 = fminf(a.x, a.z), ax0 = fminf(a.y, a.w), ay1 = fmaxf(a.x, a.z), ax1 = fmaxf(a.y, a.w);
    const float by0 = fminf(b.x, b.z), bx0 = fminf(b.y, b.w), by1 = fmaxf(b.x, b.z), bx1 = fmaxf(b.y, b.w);
    const float area_a = (ay1 - ay0) * (ax1 - ax0);
    const float area_b = (by1 - by0) * (bx1 - bx0);
    if (area_a <= 0.f || area_b <= 0.f) return 0.f;
    const float iy0 = fmaxf(ay0, by0), ix0 = fmaxf(ax0, bx0), iy1 = fminf(ay1, by1), ix1 = fminf(ax1, bx1);
    const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
    return inter / (area_a + area_b - inter);
}

// The pair rule of y4_set_nms_rule: candidate `a` is suppressed by the kept box `b` iff their measure m > thr (strict).
// NMS_IOU: m = iou_tf (the call sites compile to what they were).  NMS_DIOU1 / NMS_DIOU: DIoU-NMS (Zheng et al. 2020; Darknet's
// nms_kind=diounms),
//   m = iou - (d2 / c2)^beta,   d2 = squared distance of the centres, c2 = squared diagonal of the enclosing box,
// on the same min/max-normalised corners as iou_tf and in float32 with this operation order; c2 == 0 (both boxes one point) gives
// iou.  The boxes are the normalised canvas boxes (x / W, y / H), so on a rectangular canvas the distance is in those units, as in
// Darknet.  beta == 1 is its own kind: a plain division, no powf.
// The penalty is >= 0 and a float32 subtraction of it cannot raise iou, so m > thr needs iou > thr: the penalty is computed only for
// the pairs IoU-NMS would suppress, and for every other pair the value returned is iou, an upper bound of m that is not above thr
// either -- the same decision on every pair (a NaN iou fails both tests), at IoU's cost for all but a few.
enum { NMS_IOU = 0, NMS_DIOU1 = 1, NMS_DIOU = 2 };
// Host side, for every launcher that instantiates on the measure: the rule of the handle -> the measure (kind 0 does not read beta,
// kind 1 with beta == 1 is its own), behind the check of the rule; `who` opens the message
inline int nms_measure_index(int kind, float beta) { return kind == 0 ? NMS_IOU : (beta == 1.0f ? NMS_DIOU1 : NMS_DIOU); }
inline int nms_rule_check(const char* who, int kind, float beta, int agnostic) {
    Y4_REQUIRE((kind == 0 || kind == 1) && (agnostic == 0 || agnostic == 1) && beta > 0.f, Y4_EINVAL,
               "%s: rule (kind %d, beta %g, agnostic %d)", who, kind, (double)beta, agnostic);
    return Y4_OK;
}
template <int KIND>
__device__ __forceinline__ float nms_measure(const float4 a, const float4 b, float thr, float beta) {
    const float iou = iou_tf(a, b);
    if (KIND == NMS_IOU) return iou;
    if (!(iou > thr)) return iou;
    const float ay0 = fminf(a.x, a.z), ax0 = fminf(a.y, a.w), ay1 = fmaxf(a.x, a.z), ax1 = fmaxf(a.y, a.w);
    const float by0 = fminf(b.x, b.z), bx0 = fminf(b.y, b.w), by1 = fmaxf(b.x, b.z), bx1 = fmaxf(b.y, b.w);
    const float dy = 0.5f * (ay0 + ay1) - 0.5f * (by0 + by1), dx = 0.5f * (ax0 + ax1) - 0.5f * (bx0 + bx1);
    const float d2 = dy * dy + dx * dx;
    const float ey = fmaxf(ay1, by1) - fminf(ay0, by0), ex = fmaxf(ax1, bx1) - fminf(ax0, bx0);
    const float c2 = ey * ey + ex * ex;
    if (c2 == 0.f) return iou;
    const float q = d2 / c2;
    return iou - (KIND == NMS_DIOU1 ? q : powf(q, beta));
}

}  // namespace y4
