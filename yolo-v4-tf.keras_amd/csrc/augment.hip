// augment.hip -- the training input of Yolov4.fit in one launch (y4_augment_u8_ragged, and y4_mosaic_u8_ragged: four such
// images around a cut on one canvas): the ragged resize of misc_kernels.hip
// (resize_u8_ragged_kernel) with a rectangle that may stick out of the canvas, a mirrored column index and an HSV colour
// transform.  All randomness is drawn on the host (yolo4hip/augment.py: draw_params); the kernel is a pure function of its
// descriptor table.  yolo4hip/augment.py: augment_host is its NumPy restatement, tests/augment_oracle.py the float64 one.
#include "kernels.h"
#include "resize_common.h"

namespace y4 {

// One resized pixel through the colour rule, in float32 (the translation unit is compiled with -ffp-contract=off):
//   RGB / 255 -> HSV as colorsys.rgb_to_hsv (hue in [0,1); S = 0 and H = 0 at max == 0 or max == min),
//   H <- H + hue - floor(H + hue), S <- clamp(S * sat, 0, 1), V <- clamp(V * val, 0, 1),
//   back as colorsys.hsv_to_rgb, byte = clamp(floor(255 c + 0.5), 0, 255).
__device__ __forceinline__ void hsv_px_u8(int v[3], float hue, float sat, float val) {
    const float r = (float)v[0] / 255.0f, g = (float)v[1] / 255.0f, b = (float)v[2] / 255.0f;
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const float range = maxc - minc;
    float h = 0.f, s = 0.f;
    if (range != 0.f) {                                    // (max == 0 implies max == min)
        s = range / maxc;
        const float rc = (maxc - r) / range, gc = (maxc - g) / range, bc = (maxc - b) / range;
        if (r == maxc) h = bc - gc;
        else if (g == maxc) h = 2.0f + rc - bc;
        else h = 4.0f + gc - rc;
        h = h / 6.0f;
        h = h - floorf(h);
    }
    h = h + hue;
    h = h - floorf(h);
    s = fminf(fmaxf(s * sat, 0.f), 1.f);
    const float vv = fminf(fmaxf(maxc * val, 0.f), 1.f);
    float c[3] = {vv, vv, vv};
    if (s != 0.f) {
        const float h6 = h * 6.0f;
        int i = (int)h6;                                   // 0..6 (h may round up to 1.0)
        const float f = h6 - (float)i;
        const float p = vv * (1.0f - s), q = vv * (1.0f - s * f), t = vv * (1.0f - s * (1.0f - f));
        i = i % 6;
        c[0] = (i == 0 || i == 5) ? vv : (i == 1 ? q : (i == 4 ? t : p));
        c[1] = (i == 1 || i == 2) ? vv : (i == 3 ? q : (i == 0 ? t : p));
        c[2] = (i == 3 || i == 4) ? vv : (i == 5 ? q : (i == 2 ? t : p));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = (int)floorf(255.0f * c[k] + 0.5f);
        v[k] = o < 0 ? 0 : (o > 255 ? 255 : o);
    }
}

// The shape of resize_u8_ragged_kernel: grid y = image (its descriptor is a wave-uniform load), grid x = PX consecutive CANVAS
// pixels per thread, stored wide.  A flipped image mirrors the column a canvas pixel is SOURCED from (x' = W - 1 - x), never
// where it is stored, so a flipped thread's stores are the same three dwords.  Pixels outside the rectangle are `pad`, without
// the colour transform; the rectangle may lie partly or wholly outside the canvas (only its visible part is computed).
template <int PX>
__global__ __launch_bounds__(256) void augment_u8_ragged_kernel(const uint8_t* __restrict__ src, const y4_augment_desc* __restrict__ desc,
                                                                uint8_t* __restrict__ out, int H, int W, int pad) {
    const int b = blockIdx.y;
    const y4_augment_desc d = desc[b];
    const int hw = H * W;                                  // < 2^31 (checked on the host)
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p0 >= hw) return;
    const uint8_t* img = src + d.offset;
    const bool colour = !(d.hue == 0.f && d.sat == 1.f && d.val == 1.f);
    uint8_t px[PX * 3];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int p = p0 + k;
        const int y = p / W, x = p - y * W;
        const int yy = y - d.pad_top, xx = (d.flip ? W - 1 - x : x) - d.pad_left;
        int v[3] = {pad, pad, pad};
        if (yy >= 0 && yy < d.out_h && xx >= 0 && xx < d.out_w) {
            resize_px_u8(img, d.h, d.w, d.out_h, d.out_w, yy, xx, v);
            if (colour) hsv_px_u8(v, d.hue, d.sat, d.val);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k * 3 + c] = (uint8_t)v[c];
    }
    store_px_u8<PX>(out + ((int64_t)b * hw + p0) * 3, px);
}

int augment_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                             hipStream_t stream) {
    if (int rc = ragged_args_check("augment_u8_ragged", src, desc, out, n, H, W, pad)) return rc;
    const int hw = H * W;
    if (hw % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL(augment_u8_ragged_kernel<4>, dim3((hw / 4 + 255) / 256, n), dim3(256), 0, stream, src, desc, out, H, W, pad);
    else
        hipLaunchKernelGGL(augment_u8_ragged_kernel<1>, dim3((hw + 255) / 256, n), dim3(256), 0, stream, src, desc, out, H, W, pad);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

// y4_mosaic_u8_ragged: four tiles around a cut on one canvas, in the shape of the kernel above.  Canvas pixel (y, x) belongs to
// tile q = 2 (y >= cut_y) + (x >= cut_x) and is pixel (y, x) of the SINGLE-image rule under that tile's row on the whole
// H x W canvas: the same resize_px_u8 / hsv_px_u8 / store_px_u8 calls, so its bytes are those of augment_u8_ragged_kernel on
// that row.  A canvas's four rows and its cut reach LDS once per workgroup (50 dwords, one per thread) and are read from
// there per pixel; a thread's PX pixels may lie on both sides of cut_x, so the tile is chosen per pixel.  A tile whose window
// is empty is never chosen: its image is never dereferenced.
template <int PX>
__global__ __launch_bounds__(256) void mosaic_u8_ragged_kernel(const uint8_t* __restrict__ src, const y4_augment_desc* __restrict__ tiles,
                                                               const y4_mosaic_cut* __restrict__ cuts, uint8_t* __restrict__ out,
                                                               int H, int W, int pad) {
    constexpr int TILE_WORDS = 4 * sizeof(y4_augment_desc) / 4, CUT_WORDS = sizeof(y4_mosaic_cut) / 4;
    __shared__ __attribute__((aligned(16))) uint32_t table[TILE_WORDS + CUT_WORDS];
    const int b = blockIdx.y;
    if (threadIdx.x < TILE_WORDS) table[threadIdx.x] = ((const uint32_t*)(tiles + 4 * (int64_t)b))[threadIdx.x];
    else if (threadIdx.x < TILE_WORDS + CUT_WORDS) table[threadIdx.x] = ((const uint32_t*)(cuts + b))[threadIdx.x - TILE_WORDS];
    __syncthreads();
    const int hw = H * W;                                  // < 2^31 (checked on the host)
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p0 >= hw) return;
    const y4_augment_desc* row = (const y4_augment_desc*)table;
    const int cut_y = (int)table[TILE_WORDS], cut_x = (int)table[TILE_WORDS + 1];
    uint8_t px[PX * 3];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int p = p0 + k;
        const int y = p / W, x = p - y * W;
        const y4_augment_desc d = row[2 * (y >= cut_y) + (x >= cut_x)];
        const bool colour = !(d.hue == 0.f && d.sat == 1.f && d.val == 1.f);
        const int yy = y - d.pad_top, xx = (d.flip ? W - 1 - x : x) - d.pad_left;
        int v[3] = {pad, pad, pad};
        if (yy >= 0 && yy < d.out_h && xx >= 0 && xx < d.out_w) {
            resize_px_u8(src + d.offset, d.h, d.w, d.out_h, d.out_w, yy, xx, v);
            if (colour) hsv_px_u8(v, d.hue, d.sat, d.val);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k * 3 + c] = (uint8_t)v[c];
    }
    store_px_u8<PX>(out + ((int64_t)b * hw + p0) * 3, px);
}

int mosaic_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* tiles, const y4_mosaic_cut* cuts, int n, uint8_t* out, int H,
                            int W, int pad, hipStream_t stream) {
    Y4_REQUIRE(cuts, Y4_EINVAL, "mosaic_u8_ragged: null pointer");
    if (int rc = ragged_args_check("mosaic_u8_ragged", src, tiles, out, n, H, W, pad)) return rc;
    const int hw = H * W;
    if (hw % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL(mosaic_u8_ragged_kernel<4>, dim3((hw / 4 + 255) / 256, n), dim3(256), 0, stream, src, tiles, cuts, out, H, W, pad);
    else
        hipLaunchKernelGGL(mosaic_u8_ragged_kernel<1>, dim3((hw + 255) / 256, n), dim3(256), 0, stream, src, tiles, cuts, out, H, W, pad);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
