// grad_common.h -- device helpers of the yolo_loss gradient w.r.t. the raw heads, shared by head_train.hip (the head convs'
// weight gradient) and block_train.hip (the gradient carried one block further back).  See DESIGN.md 7d.
#pragma once
#include "kernels.h"
#include "loss_common.h"

namespace y4 {
namespace {

constexpr float W_BOX = 3.54f, W_CONF = 64.3f;     // loss.py:131-133 (the class term's weight is 1)

// The image's true boxes with w > 0 as corners in LDS (loss_kernel's prologue) -> their number.  Called by every thread.
struct TrueBoxes {
    float x1[LOSS_THREADS], y1[LOSS_THREADS], x2[LOSS_THREADS], y2[LOSS_THREADS], area[LOSS_THREADS];
    int wave[4];
};
__device__ inline int load_true_boxes(const GradK& p, int img, TrueBoxes& tb) {
    const int tid = threadIdx.x;
    float bx = 0.f, by = 0.f, bw = 0.f, bh = 0.f;
    if (tid < p.mb) {
        const float* b = p.xywh + ((size_t)img * p.mb + tid) * 4;
        bx = b[0]; by = b[1]; bw = b[2]; bh = b[3];
    }
    int nb = 0;
    const int pos = compact_valid(tid < p.mb && bw > 0.f, tb.wave, &nb);
    if (pos >= 0) {
        tb.x1[pos] = bx - bw * 0.5f; tb.y1[pos] = by - bh * 0.5f;
        tb.x2[pos] = bx + bw * 0.5f; tb.y2[pos] = by + bh * 0.5f;
        tb.area[pos] = bw * bh;
    }
    return nb;
}

// s_resp[k] = the record of lane lane0 + k of scale s (k < nlanes), or -1.  Followed by a __syncthreads of the caller.
__device__ inline void map_records(const GradK& p, int img, int s, int lane0, int nlanes, int* s_resp) {
    const int tid = threadIdx.x;
    const int gh = p.gh[s], gw = p.gw[s];
    int count = p.counts[img];
    count = count < 0 ? 0 : (count > p.mb ? p.mb : count);
    if (tid < count) {
        const int32_t* r = p.records + ((size_t)img * p.mb + tid) * p.rw;
        if (r[0] == s && r[1] >= 0 && r[1] < gh && r[2] >= 0 && r[2] < gw && r[3] >= 0 && r[3] < 3) {
            const int k = (r[1] * gw + r[2]) * 3 + r[3] - lane0;
            if (k >= 0 && k < nlanes) s_resp[k] = tid;
        }
    }
}

// The decoded box of a lane, loss.py:206-207 (no xyscale)
struct PredBox {
    float sx, sy, pw, ph, x1, y1, x2, y2;
};
__device__ inline PredBox decode_lane(const GradK& p, int s, int a, int row, int col, const float* t) {
    PredBox b;
    b.sx = sigmoidf(t[0]); b.sy = sigmoidf(t[1]);
    const float px = (b.sx + (float)col) * p.stride[s], py = (b.sy + (float)row) * p.stride[s];
    b.pw = expf(t[2]) * p.anchors[(s * 3 + a) * 2]; b.ph = expf(t[3]) * p.anchors[(s * 3 + a) * 2 + 1];
    b.x1 = px - b.pw * 0.5f; b.y1 = py - b.ph * 0.5f; b.x2 = px + b.pw * 0.5f; b.y2 = py + b.ph * 0.5f;
    return b;
}

// d(64.3 * confidence term) / d(confidence logit) of one lane, loss.py:166-182: both factors of conf_focal * BCE carry a
// gradient, the ignore mask (a cast of a comparison) none.  With q = sigmoid(t), r = respond, m = r + bgd:
//     m * [ -2 (r - q) q (1 - q) * bce(t, r) + (r - q)^2 * (q - r) ]
__device__ inline float conf_grad(const GradK& p, const TrueBoxes& tb, int nb, const PredBox& b, float tc, bool responsible) {
    const float area_p = b.pw * b.ph;
    float max_iou = 0.0f;
    for (int j = 0; j < nb; ++j) {
        const float iw = fmaxf(fminf(b.x2, tb.x2[j]) - fmaxf(b.x1, tb.x1[j]), 0.0f);
        const float ih = fmaxf(fminf(b.y2, tb.y2[j]) - fmaxf(b.y1, tb.y1[j]), 0.0f);
        const float inter = iw * ih;
        const float uni = area_p + tb.area[j] - inter;
        max_iou = fmaxf(max_iou, inter / (uni + 1e-7f));
    }
    const float r = responsible ? 1.0f : 0.0f;
    const float m = r + (1.0f - r) * (max_iou < p.thresh ? 1.0f : 0.0f);
    const float q = sigmoidf(tc);
    const float d = r - q;
    return W_CONF * m * (-2.0f * d * q * (1.0f - q) * bce_logits(tc, r) + d * d * (q - r));
}

// d(3.54 * box term) / d(tx, ty, tw, th) of a responsible lane, loss.py:34-60 and :156-162: GIoU = iou - 1 + union / enclose
// (divide_no_nan: without the last term where enclose == 0), iou = inter / (union + 1e-7), union = area_p + area_l - inter.
//     d giou = (A - B) d inter + B d area_p + E d enclose,  A = 1 / (union + eps), B = -inter / (union + eps)^2 + 1 / enclose,
//     E = -union / enclose^2
// and the corners x1 = px - pw / 2, x2 = px + pw / 2 carry it to px (stride * s (1 - s) to tx) and pw (pw itself to tw).
__device__ inline void box_grad(const GradK& p, int s, const PredBox& b, const int32_t* r, float* g) {
    const float lx = __int_as_float(r[4]), ly = __int_as_float(r[5]), lw = __int_as_float(r[6]), lh = __int_as_float(r[7]);
    const float lx1 = lx - lw * 0.5f, ly1 = ly - lh * 0.5f, lx2 = lx + lw * 0.5f, ly2 = ly + lh * 0.5f;
    const float rx = fminf(b.x2, lx2) - fmaxf(b.x1, lx1), ry = fminf(b.y2, ly2) - fmaxf(b.y1, ly1);
    const float iw = fmaxf(rx, 0.0f), ih = fmaxf(ry, 0.0f);
    const float inter = iw * ih;
    const float uni = b.pw * b.ph + lw * lh - inter;
    const float ew = fmaxf(b.x2, lx2) - fminf(b.x1, lx1), eh = fmaxf(b.y2, ly2) - fminf(b.y1, ly1);
    const float enclose = ew * eh;
    const float A = 1.0f / (uni + 1e-7f);
    const float B = -inter * A * A + (enclose == 0.0f ? 0.0f : 1.0f / enclose);
    const float E = enclose == 0.0f ? 0.0f : -uni / (enclose * enclose);
    const float AB = A - B;
    // d giou / d corner
    const float gx1 = AB * (rx > 0.0f && b.x1 > lx1 ? -ih : 0.0f) + E * (b.x1 < lx1 ? -eh : 0.0f);
    const float gx2 = AB * (rx > 0.0f && b.x2 < lx2 ? ih : 0.0f) + E * (b.x2 > lx2 ? eh : 0.0f);
    const float gy1 = AB * (ry > 0.0f && b.y1 > ly1 ? -iw : 0.0f) + E * (b.y1 < ly1 ? -ew : 0.0f);
    const float gy2 = AB * (ry > 0.0f && b.y2 < ly2 ? iw : 0.0f) + E * (b.y2 > ly2 ? ew : 0.0f);
    const float gpx = gx1 + gx2, gpy = gy1 + gy2;
    const float gpw = 0.5f * (gx2 - gx1) + B * b.ph, gph = 0.5f * (gy2 - gy1) + B * b.pw;
    const float k = -W_BOX * (2.0f - lw * lh / p.input_area);            // d(box term) = -scale * d giou
    g[0] = k * gpx * p.stride[s] * b.sx * (1.0f - b.sx);
    g[1] = k * gpy * p.stride[s] * b.sy * (1.0f - b.sy);
    g[2] = k * gpw * b.pw;
    g[3] = k * gph * b.ph;
}

__device__ inline float class_grad(const int32_t* r, int c, float x) {
    const float z = (float)(((uint32_t)r[8 + (c >> 5)] >> (c & 31)) & 1u);
    return sigmoidf(x) - z;                                              // d BCE-with-logits(x, z) / dx
}

}  // namespace
}  // namespace y4
