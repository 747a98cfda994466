// loss_common.h -- what the yolo_loss forward (loss.hip) and its gradients (head_train.hip, block_train.hip) share on the device:
// the image's true boxes in LDS, the record map of a strip, the decode of a lane and its largest IoU.
#pragma once
#include "kernels.h"

namespace y4 {
namespace {

constexpr int LOSS_THREADS = 256;

// Compacts the rows with w > 0 of one image's [mb] rows into LDS order (row order kept): -> position of this thread's row, or
// -1; *total is the number of such rows.  One row per thread (mb <= LOSS_THREADS), called by every thread of the workgroup.
__device__ inline int compact_valid(bool valid, int* s_wave, int* total) {
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned long long bal = __ballot(valid);
    if ((tid & 63) == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const unsigned long long below = bal & ((1ull << (tid & 63)) - 1ull);
    return valid ? base + __popcll(below) : -1;
}

__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
// tf.nn.sigmoid_cross_entropy_with_logits, the stable form
__device__ inline float bce_logits(float x, float z) { return fmaxf(x, 0.0f) - x * z + log1pf(expf(-fabsf(x))); }


// The image's true boxes with w > 0 as corners in LDS -> their number (a row with w <= 0 intersects nothing: its IoU is 0, the
// maximum's starting value).  Called by every thread.
struct TrueBoxes {
    float x1[LOSS_THREADS], y1[LOSS_THREADS], x2[LOSS_THREADS], y2[LOSS_THREADS], area[LOSS_THREADS];
    int wave[4];
};
__device__ inline int load_true_boxes(const LossIn& p, int img, TrueBoxes& tb) {
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
__device__ inline void map_records(const LossIn& p, int img, int s, int lane0, int nlanes, int* s_resp) {
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
__device__ inline PredBox decode_lane(const LossIn& p, int s, int a, int row, int col, const float* t) {
    PredBox b;
    b.sx = sigmoidf(t[0]); b.sy = sigmoidf(t[1]);
    const float px = (b.sx + (float)col) * p.stride[s], py = (b.sy + (float)row) * p.stride[s];
    b.pw = expf(t[2]) * p.anchors[(s * 3 + a) * 2]; b.ph = expf(t[3]) * p.anchors[(s * 3 + a) * 2 + 1];
    b.x1 = px - b.pw * 0.5f; b.y1 = py - b.ph * 0.5f; b.x2 = px + b.pw * 0.5f; b.y2 = py + b.ph * 0.5f;
    return b;
}

// CIoU of a responsible lane's decoded box (centre px, py) with its label, loss.py:63-113 as it runs, and what its gradient
// needs again (grad_common.h: box_grad_ciou):  ciou = iou - p2 / c2 - a v,  iou = inter / (union + 1e-9) with both areas from
// the corners,  p2 the squared centre distance,  c2 the squared diagonal of the enclosing box (a plain division),
// v = 4 (atan(pw / (ph + 1e-9)) - atan(lw / (lh + 1e-9)))^2 / pi^2,  a = v / (1 - iou + v).  The reference's min / max
// normalisation of the corners is kept on the predicted box (a pw underflowed to 0 behaves as there); a label has w, h >= 0.
struct Ciou {
    float lx1, ly1, lx2, ly2;        // label corners
    float x1, y1, x2, y2, cw, ch;    // predicted corners after the normalisation, their differences
    float rx, ry, iw, ih, inter;     // raw and clamped intersection sides
    float A;                         // 1 / (union + 1e-9)
    float iou, ew, eh, c2, dx, dy, p2;
    float q, hq, dat, v, a;          // q = pw / (ph + 1e-9), hq = ph + 1e-9, dat = atan(q) - atan(label's)
    float ciou;
};
__device__ inline Ciou ciou_parts(const PredBox& b, float px, float py, float lx, float ly, float lw, float lh) {
    Ciou c;
    c.lx1 = lx - lw * 0.5f; c.ly1 = ly - lh * 0.5f; c.lx2 = lx + lw * 0.5f; c.ly2 = ly + lh * 0.5f;
    c.x1 = fminf(b.x1, b.x2); c.y1 = fminf(b.y1, b.y2); c.x2 = fmaxf(b.x1, b.x2); c.y2 = fmaxf(b.y1, b.y2);
    c.cw = c.x2 - c.x1; c.ch = c.y2 - c.y1;
    const float area_p = c.cw * c.ch, area_l = (c.lx2 - c.lx1) * (c.ly2 - c.ly1);
    c.rx = fminf(c.x2, c.lx2) - fmaxf(c.x1, c.lx1); c.ry = fminf(c.y2, c.ly2) - fmaxf(c.y1, c.ly1);
    c.iw = fmaxf(c.rx, 0.0f); c.ih = fmaxf(c.ry, 0.0f);
    c.inter = c.iw * c.ih;
    const float den = area_p + area_l - c.inter + 1e-9f;
    c.A = 1.0f / den;
    c.iou = c.inter / den;
    c.ew = fmaxf(c.x2, c.lx2) - fminf(c.x1, c.lx1); c.eh = fmaxf(c.y2, c.ly2) - fminf(c.y1, c.ly1);
    c.c2 = c.ew * c.ew + c.eh * c.eh;
    c.dx = px - lx; c.dy = py - ly;
    c.p2 = c.dx * c.dx + c.dy * c.dy;
    c.hq = b.ph + 1e-9f;
    c.q = b.pw / c.hq;
    c.dat = atanf(c.q) - atanf(lw / (lh + 1e-9f));
    c.v = 4.0f * (c.dat * c.dat) / 9.869604401089358f;
    c.a = c.v / (1.0f - c.iou + c.v);
    c.ciou = c.iou - c.p2 / c.c2 - c.a * c.v;
    return c;
}

// The largest IoU of a lane's decoded box with the image's true boxes, loss.py:166-170
__device__ inline float max_iou(const TrueBoxes& tb, int nb, const PredBox& b) {
    const float area_p = b.pw * b.ph;
    float best = 0.0f;
    for (int j = 0; j < nb; ++j) {
        const float iw = fmaxf(fminf(b.x2, tb.x2[j]) - fmaxf(b.x1, tb.x1[j]), 0.0f);
        const float ih = fmaxf(fminf(b.y2, tb.y2[j]) - fmaxf(b.y1, tb.y1[j]), 0.0f);
        const float inter = iw * ih;
        const float uni = area_p + tb.area[j] - inter;
        best = fmaxf(best, inter / (uni + 1e-7f));
    }
    return best;
}

}  // namespace
}  // namespace y4
