// grad_common.h -- the formulas of the yolo_loss gradient w.r.t. the raw heads, shared by head_train.hip (the head convs' weight
// gradient) and block_train.hip (the gradient carried one block further back); labels and decode are loss_common.h's.  See
// DESIGN.md 7d.
#pragma once
#include "kernels.h"
#include "loss_common.h"

namespace y4 {
namespace {

constexpr float W_BOX = 3.54f, W_CONF = 64.3f;     // loss.py:131-133 (the class term's weight is 1)

// d(64.3 * confidence term) / d(confidence logit) of one lane, loss.py:166-182: both factors of conf_focal * BCE carry a
// gradient, the ignore mask (a cast of a comparison) none.  With q = sigmoid(t), r = respond, m = r + bgd:
//     m * [ -2 (r - q) q (1 - q) * bce(t, r) + (r - q)^2 * (q - r) ]
__device__ inline float conf_grad(const LossIn& p, const TrueBoxes& tb, int nb, const PredBox& b, float tc, bool responsible) {
    const float r = responsible ? 1.0f : 0.0f;
    const float m = r + (1.0f - r) * (max_iou(tb, nb, b) < p.thresh ? 1.0f : 0.0f);
    const float q = sigmoidf(tc);
    const float d = r - q;
    return W_CONF * m * (-2.0f * d * q * (1.0f - q) * bce_logits(tc, r) + d * d * (q - r));
}

// d(3.54 * box term) / d(tx, ty, tw, th) of a responsible lane, loss.py:34-60 and :156-162: GIoU = iou - 1 + union / enclose
// (divide_no_nan: without the last term where enclose == 0), iou = inter / (union + 1e-7), union = area_p + area_l - inter.
//     d giou = (A - B) d inter + B d area_p + E d enclose,  A = 1 / (union + eps), B = -inter / (union + eps)^2 + 1 / enclose,
//     E = -union / enclose^2
// and the corners x1 = px - pw / 2, x2 = px + pw / 2 carry it to px (stride * s (1 - s) to tx) and pw (pw itself to tw).
__device__ inline void box_grad_giou(const LossIn& p, int s, const PredBox& b, const int32_t* r, float* g) {
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

// The same for the CIoU box term (y4_set_box_loss(h, 1)), loss.py:63-113 and :156-162 as autodiff runs it: there is no
// stop_gradient, so a v = v^2 / D, D = 1 - iou + v, is differentiated as a whole, through v and through the iou inside D:
//     d ciou = (1 - a^2) d iou - (2 a - a^2) d v - d p2 / c2 + p2 / c2^2 d c2
//     d iou = (A + inter A^2) d inter - inter A^2 d area_p,   A = 1 / (union + 1e-9),   area_p = (x2 - x1) (y2 - y1)
//     d c2 = 2 ew d ew + 2 eh d eh (the enclosing corners),   d p2 = 2 (px - lx) d px + 2 (py - ly) d py
//     d v = 8 / pi^2 (atan q - atan ql) / (1 + q^2) d q,   q = pw / (ph + 1e-9):  d q = d pw / (ph + 1e-9) - pw d ph / (ph + 1e-9)^2
// Ties of a maximum / minimum: the strict comparison decides.  The corner normalisation min(x1, x2) / max(x1, x2) is the identity
// for pw > 0 and carries the same sum to px at pw == 0, where the chain's factor pw zeroes the width's gradient anyway.
__device__ inline void box_grad_ciou(const LossIn& p, int s, const PredBox& b, const int32_t* r, float* g) {
    const float lx = __int_as_float(r[4]), ly = __int_as_float(r[5]), lw = __int_as_float(r[6]), lh = __int_as_float(r[7]);
    const float px = (b.sx + (float)r[2]) * p.stride[s], py = (b.sy + (float)r[1]) * p.stride[s];     // decode_lane's centre
    const Ciou c = ciou_parts(b, px, py, lx, ly, lw, lh);
    const float a2 = c.a * c.a;
    const float Ki = 1.0f - a2, Kv = a2 - 2.0f * c.a;
    const float Bi = -c.inter * c.A * c.A;
    const float cI = Ki * (c.A - Bi), cA = Ki * Bi;
    const float ic2 = 1.0f / c.c2;
    const float Ex = 2.0f * c.ew * (c.p2 * ic2 * ic2), Ey = 2.0f * c.eh * (c.p2 * ic2 * ic2);
    // d ciou / d corner: the intersection and the enclosing diagonal
    const float gx1 = cI * (c.rx > 0.0f && c.x1 > c.lx1 ? -c.ih : 0.0f) + (c.x1 < c.lx1 ? -Ex : 0.0f);
    const float gx2 = cI * (c.rx > 0.0f && c.x2 < c.lx2 ? c.ih : 0.0f) + (c.x2 > c.lx2 ? Ex : 0.0f);
    const float gy1 = cI * (c.ry > 0.0f && c.y1 > c.ly1 ? -c.iw : 0.0f) + (c.y1 < c.ly1 ? -Ey : 0.0f);
    const float gy2 = cI * (c.ry > 0.0f && c.y2 < c.ly2 ? c.iw : 0.0f) + (c.y2 > c.ly2 ? Ey : 0.0f);
    const float dvq = Kv * (8.0f / 9.869604401089358f) * c.dat / (1.0f + c.q * c.q);             // (d ciou / d v) (d v / d q)
    const float gpx = gx1 + gx2 - 2.0f * c.dx * ic2, gpy = gy1 + gy2 - 2.0f * c.dy * ic2;
    const float gpw = 0.5f * (gx2 - gx1) + cA * c.ch + dvq / c.hq;
    const float gph = 0.5f * (gy2 - gy1) + cA * c.cw - dvq * (b.pw / (c.hq * c.hq));
    const float k = -W_BOX * (2.0f - lw * lh / p.input_area);            // d(box term) = -scale * d ciou
    g[0] = k * gpx * p.stride[s] * b.sx * (1.0f - b.sx);
    g[1] = k * gpy * p.stride[s] * b.sy * (1.0f - b.sy);
    g[2] = k * gpw * b.pw;
    g[3] = k * gph * b.ph;
}

// the one place the kind (LossIn::box_kind, uniform over a launch) picks the box term's gradient
__device__ inline void box_grad(const LossIn& p, int s, const PredBox& b, const int32_t* r, float* g) {
    if (p.box_kind == BOX_CIOU) box_grad_ciou(p, s, b, r, g);
    else box_grad_giou(p, s, b, r, g);
}

__device__ inline float class_grad(const int32_t* r, int c, float x) {
    const float z = (float)(((uint32_t)r[8 + (c >> 5)] >> (c & 31)) & 1u);
    return sigmoidf(x) - z;                                              // d BCE-with-logits(x, z) / dx
}

}  // namespace
}  // namespace y4
