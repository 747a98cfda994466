// head_train.hip -- fine-tuning of the three detection convs (93 / 101 / 109; reference custom_layers.py yolov4_neck, the three
// conv(..., activation=None, batch_norm=False) calls) on a frozen backbone and neck: the gradient of the reference's yolo_loss
// (loss.py:116-188, decode :191-211) w.r.t. the raw heads, the head convs' weight gradient fused with it, and Keras' Adam step.
// See DESIGN.md 7d.
//
// The gradient w.r.t. a raw head is three dense columns (every anchor's confidence logit) plus at most max_boxes sparse rows
// per image (x, y, w, h and class logits of the responsible lanes).  The training path never stores it: the confidence columns
// are recomputed per pixel strip, the sparse rows per record.
//
// Determinism rule of loss.hip: no floating-point atomics, every sum in an order fixed by the geometry.
//   confidence rows  pixel strip of HG_PIX cells: pixel p of the strip belongs to group p % G (G = 256 / (cin / 8)), a group adds
//                    its pixels in ascending order, the groups are added in group order; head_conf_finish_kernel adds the strip
//                    partials in (image, strip) order
//   sparse rows      one workgroup per (scale, anchor, logit) adds its records' products in (image, record) order
#include "kernels.h"
#include "loss_common.h"

namespace y4 {

namespace {

constexpr int HG_PIX = 64;                 // cells of a confidence strip (3 lanes each: 192 of the 256 threads compute a gradient)
constexpr int HG_VEC = 8;                  // channels per thread of the strip pass
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

// ---- y4_loss_grad: the dense gradient (parity / debugging).  grid (strips of one image, images) as loss_kernel.
__global__ __launch_bounds__(LOSS_THREADS) void loss_grad_kernel(GradK p) {
    __shared__ TrueBoxes tb;
    __shared__ int s_resp[LOSS_THREADS];
    const int img = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    const int s = strip >= p.strip_base[2] ? 2 : (strip >= p.strip_base[1] ? 1 : 0);
    const int lane0 = (strip - p.strip_base[s]) * LOSS_THREADS;
    const int gh = p.gh[s], gw = p.gw[s];
    const int lanes = 3 * gh * gw, nf = p.C + 5;
    const int nb = load_true_boxes(p, img, tb);
    s_resp[tid] = -1;
    __syncthreads();
    map_records(p, img, s, lane0, LOSS_THREADS, s_resp);
    __syncthreads();
    const int lane = lane0 + tid;
    if (lane >= lanes) return;
    const int cell = lane / 3, a = lane - cell * 3;
    const int row = cell / gw, col = cell - row * gw;
    const float* t = p.head[s] + ((size_t)img * gh * gw + cell) * p.hcs + a * nf;
    float* o = p.dense[s] + ((size_t)img * gh * gw + cell) * (3 * nf) + a * nf;
    const float wimg = p.imgw[img];
    const PredBox b = decode_lane(p, s, a, row, col, t);
    const int ri = s_resp[tid];
    o[4] = wimg * conf_grad(p, tb, nb, b, t[4], ri >= 0);
    if (ri >= 0) {
        const int32_t* r = p.records + ((size_t)img * p.mb + ri) * p.rw;
        float g[4];
        box_grad(p, s, b, r, g);
        for (int j = 0; j < 4; ++j) o[j] = wimg * g[j];
        for (int c = 0; c < p.C; ++c) o[5 + c] = wimg * class_grad(r, c, t[5 + c]);
    } else {
        for (int j = 0; j < 4; ++j) o[j] = 0.0f;
        for (int c = 0; c < p.C; ++c) o[5 + c] = 0.0f;
    }
}

// ---- y4_head_grad, the confidence rows.  grid (pixel strips of one image, images); a strip is HG_PIX cells of ONE scale.
// partial of (image, strip): [3 anchors][cin] weight sums, then 3 bias sums (row stride 3 * cin + 4 floats)
template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void head_conf_wgrad_kernel(GradK p) {
    using E = Elem<DT>;
    __shared__ TrueBoxes tb;
    __shared__ int s_resp[LOSS_THREADS];
    __shared__ float s_g[HG_PIX * 3];
    __shared__ float s_acc[LOSS_THREADS * 3 * HG_VEC];                          // [group][3 anchors][cin]: 256 * 3 * 8 floats whatever cin
    const int img = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    const int s = strip >= p.pstrip_base[2] ? 2 : (strip >= p.pstrip_base[1] ? 1 : 0);
    const int ls = strip - p.pstrip_base[s];
    const int cell0 = ls * HG_PIX;
    const int gh = p.gh[s], gw = p.gw[s], cells = gh * gw, cin = p.cin[s];
    const int nb = load_true_boxes(p, img, tb);
    s_resp[tid] = -1;
    __syncthreads();
    map_records(p, img, s, cell0 * 3, HG_PIX * 3, s_resp);
    __syncthreads();
    if (tid < HG_PIX * 3) {
        const int cell = cell0 + tid / 3, a = tid % 3;
        float g = 0.0f;
        if (cell < cells) {
            const int row = cell / gw, col = cell - row * gw;
            const float* t = p.head[s] + ((size_t)img * cells + cell) * p.hcs + a * (p.C + 5);
            const PredBox b = decode_lane(p, s, a, row, col, t);
            g = p.imgw[img] * conf_grad(p, tb, nb, b, t[4], s_resp[tid] >= 0);
        }
        s_g[tid] = g;
    }
    __syncthreads();
    const int tpr = cin / HG_VEC, groups = LOSS_THREADS / tpr;           // threads per pixel row, pixel groups
    const int tc = tid % tpr, grp = tid / tpr;
    float acc[3][HG_VEC];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < HG_VEC; ++k) acc[a][k] = 0.0f;
    const int npix = cells - cell0 < HG_PIX ? cells - cell0 : HG_PIX;
    const typename E::type* x = (const typename E::type*)p.x[s] + ((size_t)img * cells + cell0) * cin + tc * HG_VEC;
    for (int pix = grp; pix < npix; pix += groups) {
        float v[HG_VEC];
#pragma unroll
        for (int q = 0; q < HG_VEC / E::EPC; ++q) E::load_chunk(x + (size_t)pix * cin + q * E::EPC, v + q * E::EPC);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float g = s_g[pix * 3 + a];
#pragma unroll
            for (int k = 0; k < HG_VEC; ++k) acc[a][k] = fmaf(g, v[k], acc[a][k]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < HG_VEC; ++k) s_acc[(grp * 3 + a) * cin + tc * HG_VEC + k] = acc[a][k];
    __syncthreads();
    float* o = p.partials + p.part_base[s] + ((size_t)img * p.pstrips[s] + ls) * (3 * cin + 4);
    for (int e = tid; e < 3 * cin; e += LOSS_THREADS) {
        float sum = s_acc[e];
        for (int g = 1; g < groups; ++g) sum += s_acc[g * 3 * cin + e];
        o[e] = sum;
    }
    if (tid < 3) {
        float sum = 0.0f;
        for (int pix = 0; pix < npix; ++pix) sum += s_g[pix * 3 + tid];
        o[3 * cin + tid] = sum;
    }
}

// one scale per launch: thread e < 3 * cin adds weight (anchor e / cin, channel e % cin) over (image, strip), e - 3 * cin < 3 a bias
__global__ __launch_bounds__(LOSS_THREADS) void head_conf_finish_kernel(GradK p, int s, int n) {
    const int e = blockIdx.x * LOSS_THREADS + threadIdx.x;
    const int cin = p.cin[s], nf = p.C + 5;
    if (e >= 3 * cin + 3) return;
    const size_t stride = 3 * cin + 4;
    const float* q = p.partials + p.part_base[s] + e;
    const int total = n * p.pstrips[s];
    float acc = 0.0f;
#pragma unroll 8
    for (int k = 0; k < total; ++k) acc += q[k * stride];
    float* dw = p.dw + p.dw_off[s];
    float* o = e < 3 * cin ? dw + 3 * nf + (size_t)((e / cin) * nf + 4) * cin + e % cin : dw + (e - 3 * cin) * nf + 4;
    *o = p.accumulate ? *o + acc : acc;
}

// ---- y4_head_grad, the sparse rows.  grid (4 + C logits, 3 anchors, 3 scales): the workgroup owns output row
// anchor * (5 + C) + logit of one head conv.  256 (image, record) slots at a time are screened in parallel, the matching ones
// compacted in slot order into LDS with their gradient value, then every thread adds value * X[cell][its channels] in that order.
template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void head_sparse_wgrad_kernel(GradK p, int n) {
    using E = Elem<DT>;
    __shared__ float s_g[LOSS_THREADS];
    __shared__ int s_px[LOSS_THREADS];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    const int j = blockIdx.x < 4 ? blockIdx.x : blockIdx.x + 1;          // logit inside the anchor's group (4 is the confidence)
    const int a = blockIdx.y, s = blockIdx.z;
    const int gh = p.gh[s], gw = p.gw[s], cells = gh * gw, cin = p.cin[s], nf = p.C + 5;
    const typename E::type* x = (const typename E::type*)p.x[s];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bias = 0.0f;               // cin <= 4 * LOSS_THREADS (checked by the launcher)
    const int slots = n * p.mb;
    for (int base = 0; base < slots; base += LOSS_THREADS) {
        const int slot = base + tid;
        const int img = slot / p.mb, ri = slot - img * p.mb;
        bool valid = false;
        const int32_t* r = nullptr;
        if (slot < slots) {
            int count = p.counts[img];
            count = count < 0 ? 0 : (count > p.mb ? p.mb : count);
            r = p.records + (size_t)slot * p.rw;
            valid = ri < count && r[0] == s && r[3] == a && r[1] >= 0 && r[1] < gh && r[2] >= 0 && r[2] < gw;
        }
        int total = 0;
        const int pos = compact_valid(valid, s_wave, &total);
        if (valid) {
            const int cell = r[1] * gw + r[2];
            const float* t = p.head[s] + ((size_t)img * cells + cell) * p.hcs + a * nf;
            float g;
            if (j < 4) {
                float g4[4];
                box_grad(p, s, decode_lane(p, s, a, r[1], r[2], t), r, g4);
                g = g4[j];
            } else {
                g = class_grad(r, j - 5, t[j]);
            }
            s_g[pos] = p.imgw[img] * g;
            s_px[pos] = img * cells + cell;
        }
        __syncthreads();
        for (int e = 0; e < total; ++e) {
            const float g = s_g[e];
            const typename E::type* xr = x + (size_t)s_px[e] * cin;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (tid + k * LOSS_THREADS < cin) acc[k] = fmaf(g, E::ld(xr[tid + k * LOSS_THREADS]), acc[k]);
            bias += g;
        }
        __syncthreads();                                                  // s_g / s_px / s_wave are reused by the next round
    }
    const int row = a * nf + j;
    float* dw = p.dw + p.dw_off[s];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (tid + k * LOSS_THREADS < cin) {
            float* o = dw + 3 * nf + (size_t)row * cin + tid + k * LOSS_THREADS;
            *o = p.accumulate ? *o + acc[k] : acc[k];
        }
    if (tid == 0) dw[row] = p.accumulate ? dw[row] + bias : bias;
}

// ---- y4_head_adam: Keras' Adam (the reference compiles Adam(learning_rate=1e-4), models.py:83) with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
__global__ void head_adam_kernel(const float* __restrict__ g, float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                 size_t count, float lr_t, float b1, float b2, float eps) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * (gi * gi);
    m[i] = mi; v[i] = vi;
    w[i] = w[i] - lr_t * mi / (sqrtf(vi) + eps);
}

}  // namespace

int head_grad_strips(const int* gh, const int* gw, int* pstrip_base, int* pstrips) {
    int total = 0;
    for (int i = 0; i < 3; ++i) {
        const int k = (gh[i] * gw[i] + HG_PIX - 1) / HG_PIX;
        if (pstrip_base) pstrip_base[i] = total;
        if (pstrips) pstrips[i] = k;
        total += k;
    }
    return total;
}

size_t head_grad_scratch_floats(const int* gh, const int* gw, const int* cin, int n, size_t* part_base) {
    int pstrips[3];
    head_grad_strips(gh, gw, nullptr, pstrips);
    size_t total = 0;
    for (int i = 0; i < 3; ++i) {
        if (part_base) part_base[i] = total;
        total += (size_t)n * pstrips[i] * (3 * (size_t)cin[i] + 4);
    }
    return total;
}

int loss_grad_launch(const GradK& k, int n, hipStream_t stream) {
    Y4_REQUIRE(k.mb >= 1 && k.mb <= LOSS_THREADS, Y4_EINVAL, "loss gradient: max_boxes %d outside [1, %d]", k.mb, LOSS_THREADS);
    hipLaunchKernelGGL(loss_grad_kernel, dim3(k.strips, n), dim3(LOSS_THREADS), 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

template <int DT>
static int head_grad_launch_t(const GradK& k, int n, hipStream_t stream) {
    const int nstrips = k.pstrip_base[2] + k.pstrips[2];
    hipLaunchKernelGGL(head_conf_wgrad_kernel<DT>, dim3(nstrips, n), dim3(LOSS_THREADS), 0, stream, k);
    for (int s = 0; s < 3; ++s)
        hipLaunchKernelGGL(head_conf_finish_kernel, dim3((3 * k.cin[s] + 3 + LOSS_THREADS - 1) / LOSS_THREADS), dim3(LOSS_THREADS), 0,
                           stream, k, s, n);
    hipLaunchKernelGGL(head_sparse_wgrad_kernel<DT>, dim3(4 + k.C, 3, 3), dim3(LOSS_THREADS), 0, stream, k, n);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int head_grad_launch(int dtype, const GradK& k, int n, hipStream_t stream) {
    Y4_REQUIRE(k.mb >= 1 && k.mb <= LOSS_THREADS, Y4_EINVAL, "head gradient: max_boxes %d outside [1, %d]", k.mb, LOSS_THREADS);
    for (int s = 0; s < 3; ++s)
        Y4_REQUIRE(k.cin[s] % HG_VEC == 0 && LOSS_THREADS % (k.cin[s] / HG_VEC) == 0 && k.cin[s] <= 4 * LOSS_THREADS && (int64_t)n * k.gh[s] * k.gw[s] < (1ll << 31),
                   Y4_EINVAL, "head gradient: %d input channels / %d images of scale %d", k.cin[s], n, s);
    switch (dtype) {
        case Y4_F32: return head_grad_launch_t<Y4_F32>(k, n, stream);
        case Y4_BF16: return head_grad_launch_t<Y4_BF16>(k, n, stream);
        case Y4_F16: return head_grad_launch_t<Y4_F16>(k, n, stream);
        default: set_error("head gradient: bad dtype %d", dtype); return Y4_EINVAL;
    }
}

int head_adam_launch(const float* g, float* w, float* m, float* v, size_t count, float lr_t, float b1, float b2, float eps,
                     hipStream_t stream) {
    hipLaunchKernelGGL(head_adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, g, w, m, v, count, lr_t, b1, b2,
                       eps);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
