// anchor_iou.h -- THE pair measure between a label box and an anchor: the IoU of the two rectangles centred on each other, as
// preprocess_true_boxes has it (reference utils.py:262-275, yolo4hip/data.py `_assign`).  One copy, used by the label assignment
// (loss.hip) and by the anchor search (anchors.hip), so that the anchor the search gives a box is the anchor y4_loss_assign
// gives it.
//   half sides of the box   (double)(bw * 0.5f)       -- float32 halving, exact
//   area of the box         (double)(bw * bh)         -- a float32 product in the reference
//   anchor sides            widened to double; halves, area, intersection, union and quotient in float64
// Callers compile with contraction off (-ffp-contract=off): no fused multiply-add may change a bit here.
#pragma once
#include "common.h"

namespace y4 {

__device__ __forceinline__ double anchor_iou64(float bw, float bh, float anchor_w, float anchor_h) {
    const double hbw = (double)(bw * 0.5f), hbh = (double)(bh * 0.5f);
    const double area_b = (double)(bw * bh);                              // a float32 product in the reference
    const double aw = (double)anchor_w, ah = (double)anchor_h;
    const double lo_x = fmax(-hbw, -(aw / 2.0)), hi_x = fmin(hbw, aw / 2.0);
    const double lo_y = fmax(-hbh, -(ah / 2.0)), hi_y = fmin(hbh, ah / 2.0);
    const double inter = fmax(hi_x - lo_x, 0.0) * fmax(hi_y - lo_y, 0.0);
    return inter / (area_b + aw * ah - inter);
}

// The first arg-max over anchors[0 .. k) (w, h pairs): strict `>` to replace, as np.argmax.  *best_iou gets the measure.
__device__ __forceinline__ int best_anchor(float bw, float bh, const float* anchors, int k, double* best_iou) {
    double best = 0.0;
    int best_a = 0;
    for (int a = 0; a < k; ++a) {
        const double iou = anchor_iou64(bw, bh, anchors[2 * a], anchors[2 * a + 1]);
        if (a == 0 || iou > best) { best = iou; best_a = a; }             // first arg-max on ties
    }
    *best_iou = best;
    return best_a;
}

}  // namespace y4
