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
#include "grad_common.h"

namespace y4 {

namespace {

constexpr int HG_PIX = 64;                 // cells of a confidence strip (3 lanes each: 192 of the 256 threads compute a gradient)
constexpr int HG_VEC = 8;                  // channels per thread of the strip pass

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

// ---- y4_head_adam / y4_block_adam: Keras' Adam (the reference compiles Adam(learning_rate=1e-4), models.py:83) with lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
__global__ void adam_kernel(const float* __restrict__ g, float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
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

int adam_launch(const float* g, float* w, float* m, float* v, size_t count, float lr_t, float b1, float b2, float eps, hipStream_t stream) {
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, g, w, m, v, count, lr_t, b1, b2, eps);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
