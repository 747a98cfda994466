// loss.hip -- the reference's yolo_loss forward (loss.py:119-212) over the raw float32 heads in the workspace, and the label
// assignment of preprocess_true_boxes (utils.py:215-303) as sparse responsible-cell records.  See DESIGN.md "Validation loss".
//
// Determinism rule: no floating-point atomics anywhere.  A (cell, anchor) lane's terms are reduced inside its wave by a fixed
// shuffle tree, the four waves of a workgroup are added in wave order, and a second kernel adds a scale's workgroup partials in
// strip order.  The tree depends on the image's geometry only, so image i's nine sums are the same bits whatever the batch
// size and wherever the image sits in the batch.
#include "anchor_iou.h"
#include "kernels.h"
#include "loss_common.h"

namespace y4 {

namespace {

// One workgroup per image, one thread per box row.
__global__ __launch_bounds__(LOSS_THREADS) void loss_assign_kernel(LossAssignK p) {
    __shared__ float s_w[LOSS_THREADS], s_h[LOSS_THREADS];
    __shared__ int s_vidx[LOSS_THREADS], s_cls[LOSS_THREADS], s_last[LOSS_THREADS];
    __shared__ uint32_t s_key[LOSS_THREADS];
    __shared__ int s_wave[4];
    const int img = blockIdx.x, tid = threadIdx.x;
    const bool row_ok = tid < p.mb;
    float cx = 0.f, cy = 0.f, w = 0.f, h = 0.f, clsf = 0.f;
    if (row_ok) {
        const float* b = p.boxes + ((size_t)img * p.mb + tid) * 5;
        const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        clsf = b[4];
        cx = floorf((x1 + x2) * 0.5f);            // (x1 + x2) // 2 on float32: the halving is exact
        cy = floorf((y1 + y2) * 0.5f);
        w = x2 - x1;
        h = y2 - y1;
        float* o = p.xywh + ((size_t)img * p.mb + tid) * 4;
        o[0] = cx; o[1] = cy; o[2] = w; o[3] = h;
    }
    s_w[tid] = w; s_h[tid] = h;
    s_key[tid] = 0xFFFFFFFFu; s_cls[tid] = 0; s_last[tid] = 0;
    int nvalid = 0;
    const int pos = compact_valid(row_ok && w > 0.f, s_wave, &nvalid);
    if (pos >= 0) s_vidx[pos] = tid;
    __syncthreads();

    // the k-th VALID row's (w, h) picks the anchor; row k of the uncompacted array gives the cell, the xywh and the class
    int bad = 0;
    if (tid < nvalid) {
        const int j = s_vidx[tid];
        const float bw = s_w[j], bh = s_h[j];
        double best;
        const int best_a = best_anchor(bw, bh, p.anchors, 9, &best);      // anchor_iou.h: the centred IoU, first arg-max on ties
        const int s = best_a / 3, a = best_a % 3;
        const float xn = (float)((double)cx / (double)p.img_w), yn = (float)((double)cy / (double)p.img_h);
        const double fc = floor((double)xn * (double)p.gw[s]), fr = floor((double)yn * (double)p.gh[s]);
        const bool cell_ok = fc >= 0.0 && fc < (double)p.gw[s] && fr >= 0.0 && fr < (double)p.gh[s];
        const bool cls_ok = clsf > -1.f && clsf < (float)p.C;
        if (cell_ok && cls_ok) {
            s_key[tid] = (uint32_t)(p.lane_base[s] + ((int)fr * p.gw[s] + (int)fc) * 3 + a);
            s_cls[tid] = (int)clsf;
        } else {
            bad = 1;
        }
    }
    const int any_bad = __syncthreads_or(bad);

    // last writer wins: the record of a key belongs to the last row that carries it
    const uint32_t key = s_key[tid];
    int last = 0;
    if (key != 0xFFFFFFFFu) {
        last = 1;
        for (int j = tid + 1; j < nvalid; ++j) last &= s_key[j] != key;
    }
    s_last[tid] = last;
    const int count = __syncthreads_count(last);

    int32_t* recs = p.records + (size_t)img * p.mb * p.rw;
    if (last) {
        int rank = 0;
        for (int j = 0; j < nvalid; ++j) rank += (s_last[j] && s_key[j] < key) ? 1 : 0;
        int32_t* r = recs + (size_t)rank * p.rw;
        int s = 2;
        if (key < (uint32_t)p.lane_base[1]) s = 0; else if (key < (uint32_t)p.lane_base[2]) s = 1;
        const int local = (int)key - p.lane_base[s];
        const int cell = local / 3;
        r[0] = s; r[1] = cell / p.gw[s]; r[2] = cell % p.gw[s]; r[3] = local % 3;
        r[4] = __float_as_int(cx); r[5] = __float_as_int(cy); r[6] = __float_as_int(w); r[7] = __float_as_int(h);
        for (int m = 0; m < p.mw; ++m) r[8 + m] = 0;
        for (int j = 0; j < nvalid; ++j)                                    // the class bits of every row on this cell stay set
            if (s_key[j] == key) r[8 + (s_cls[j] >> 5)] |= (int32_t)(1u << (s_cls[j] & 31));
    }
    for (int i = count * p.rw + tid; i < p.mb * p.rw; i += LOSS_THREADS) recs[i] = 0;
    if (tid == 0) p.counts[img] = any_bad ? -1 : count;
}

// grid (strips of one image, images); a strip is LOSS_THREADS consecutive (cell, anchor) lanes of ONE scale
__global__ __launch_bounds__(LOSS_THREADS) void loss_kernel(LossK p) {
    __shared__ TrueBoxes tb;
    __shared__ int s_resp[LOSS_THREADS];
    __shared__ float s_red[4][3];
    const int img = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    const int s = strip >= p.strip_base[2] ? 2 : (strip >= p.strip_base[1] ? 1 : 0);
    const int lane0 = (strip - p.strip_base[s]) * LOSS_THREADS;
    const int gh = p.gh[s], gw = p.gw[s];
    const int lanes = 3 * gh * gw;
    const int nb = load_true_boxes(p, img, tb);
    s_resp[tid] = -1;
    __syncthreads();
    map_records(p, img, s, lane0, LOSS_THREADS, s_resp);
    __syncthreads();

    float box_t = 0.f, conf_t = 0.f, cls_t = 0.f;
    const int lane = lane0 + tid;
    if (lane < lanes) {
        const int cell = lane / 3, a = lane - cell * 3;
        const int row = cell / gw, col = cell - row * gw;
        const float* t = p.head[s] + ((size_t)img * gh * gw + cell) * p.hcs + a * (p.C + 5);
        const float tc = t[4];
        const PredBox pb = decode_lane(p, s, a, row, col, t);              // loss.py:195-212: no xyscale here, unlike the inference decode
        const float px1 = pb.x1, py1 = pb.y1, px2 = pb.x2, py2 = pb.y2, area_p = pb.pw * pb.ph;
        const int ri = s_resp[tid];
        const float respond = ri >= 0 ? 1.0f : 0.0f;
        const float bgd = (1.0f - respond) * (max_iou(tb, nb, pb) < p.thresh ? 1.0f : 0.0f);
        const float d = respond - sigmoidf(tc);
        const float bce = bce_logits(tc, respond);
        conf_t = (d * d) * (respond * bce + bgd * bce);
        if (ri >= 0) {
            const int32_t* r = p.records + ((size_t)img * p.mb + ri) * p.rw;
            const float lx = __int_as_float(r[4]), ly = __int_as_float(r[5]), lw = __int_as_float(r[6]), lh = __int_as_float(r[7]);
            const float area_l = lw * lh;
            const float lx1 = lx - lw * 0.5f, ly1 = ly - lh * 0.5f, lx2 = lx + lw * 0.5f, ly2 = ly + lh * 0.5f;
            const float iw = fmaxf(fminf(px2, lx2) - fmaxf(px1, lx1), 0.0f);
            const float ih = fmaxf(fminf(py2, ly2) - fmaxf(py1, ly1), 0.0f);
            const float inter = iw * ih;
            const float uni = area_p + area_l - inter;
            const float iou = inter / (uni + 1e-7f);
            const float enclose = (fmaxf(px2, lx2) - fminf(px1, lx1)) * (fmaxf(py2, ly2) - fminf(py1, ly1));
            const float giou = iou - (enclose == 0.0f ? 0.0f : (enclose - uni) / enclose);      // divide_no_nan
            box_t = (2.0f - lw * lh / p.input_area) * (1.0f - giou);
            // No if / else on purpose: the GIoU block above stays the text it was, so that its bits cannot move, and CIoU
            // overwrites its result.  The spare GIoU costs at most max_boxes lanes per image; the kind is uniform over the launch.
            if (p.box_kind == BOX_CIOU) {                                  // y4_set_box_loss
                const float px = (pb.sx + (float)col) * p.stride[s], py = (pb.sy + (float)row) * p.stride[s];   // decode_lane's centre
                box_t = (2.0f - lw * lh / p.input_area) * (1.0f - ciou_parts(pb, px, py, lx, ly, lw, lh).ciou);
            }
            for (int c = 0; c < p.C; ++c) {
                const float z = (float)(((uint32_t)r[8 + (c >> 5)] >> (c & 31)) & 1u);
                cls_t += bce_logits(t[5 + c], z);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        box_t += __shfl_down(box_t, o);
        conf_t += __shfl_down(conf_t, o);
        cls_t += __shfl_down(cls_t, o);
    }
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = box_t; s_red[tid >> 6][1] = conf_t; s_red[tid >> 6][2] = cls_t; }
    __syncthreads();
    if (tid < 3) {
        float* o = p.partials + ((size_t)img * p.strips + strip) * 3;
        o[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// one workgroup per image: thread (scale, term) adds that scale's strip partials in strip order
__global__ __launch_bounds__(64) void loss_finish_kernel(LossK p) {
    const int img = blockIdx.x, tid = threadIdx.x;
    if (tid >= 9) return;
    const int s = tid / 3, c = tid - s * 3;
    const int end = s == 2 ? p.strips : p.strip_base[s + 1];
    const float* q = p.partials + (size_t)img * p.strips * 3;
    float acc = 0.0f;
    for (int k = p.strip_base[s]; k < end; ++k) acc += q[k * 3 + c];
    p.out[(size_t)img * 9 + tid] = acc;
}

}  // namespace

int loss_strips(const int* gh, const int* gw, int* strip_base) {
    int total = 0;
    for (int i = 0; i < 3; ++i) {
        if (strip_base) strip_base[i] = total;
        total += (3 * gh[i] * gw[i] + LOSS_THREADS - 1) / LOSS_THREADS;
    }
    return total;
}

int loss_assign_launch(const LossAssignK& k, int n, hipStream_t stream) {
    Y4_REQUIRE(k.mb >= 1 && k.mb <= LOSS_THREADS, Y4_EINVAL, "loss: max_boxes %d outside [1, %d]", k.mb, LOSS_THREADS);
    hipLaunchKernelGGL(loss_assign_kernel, dim3(n), dim3(LOSS_THREADS), 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int loss_launch(const LossK& k, int n, hipStream_t stream) {
    Y4_REQUIRE(k.mb >= 1 && k.mb <= LOSS_THREADS, Y4_EINVAL, "loss: max_boxes %d outside [1, %d]", k.mb, LOSS_THREADS);
    hipLaunchKernelGGL(loss_kernel, dim3(k.strips, n), dim3(LOSS_THREADS), 0, stream, k);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(n), dim3(64), 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
