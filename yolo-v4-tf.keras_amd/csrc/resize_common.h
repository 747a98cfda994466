// resize_common.h -- the uint8 bilinear arithmetic every resize kernel shares (misc_kernels.hip: preprocess / resize kernels,
// augment.hip: the training-input kernel), and the wide store of a thread's packed pixels.
#pragma once
#include "common.h"

namespace y4 {

// Yolov4.preprocess_img (reference models.py:95-98): cv2.resize(img, (W,H)) [INTER_LINEAR, plain stretch].  Restates OpenCV's
// uint8 fixed-point bilinear scheme (half-pixel centres, 11-bit coefficients, two rounding shifts) exactly like the host version
// yolo4hip/prepost.py: resize_bilinear, so both paths give identical bytes.
__device__ __forceinline__ void lin_coeff(int d, int dst, int src, int& s0, int& s1, int& a0, int& a1) {
    const double scale = (double)src / (double)dst;
    double f = ((double)d + 0.5) * scale - 0.5;
    int s = (int)floor(f);
    float fr = (float)(f - (double)s);
    if (s < 0) { fr = 0.f; s = 0; }
    if (s >= src - 1) { fr = 0.f; s = src - 1; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    a1 = (int)rintf(fr * 2048.0f);
    a0 = (int)rintf((1.0f - fr) * 2048.0f);
}

// One output pixel (row y, column x) of cv2.resize's uint8 INTER_LINEAR resize of `src` [h,w,3] to dw x dh, all three channels:
// the arithmetic every uint8 resize kernel here shares (prepost.py: resize_bilinear is its host restatement).
__device__ __forceinline__ void resize_px_u8(const uint8_t* __restrict__ src, int h, int w, int dh, int dw, int y, int x, int v[3]) {
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    lin_coeff(x, dw, w, x0, x1, ax0, ax1);
    lin_coeff(y, dh, h, y0, y1, ay0, ay1);
    const bool same = (h == dh && w == dw);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (same) {
            v[c] = src[(y * w + x) * 3 + c];
        } else {
            const int top = src[(y0 * w + x0) * 3 + c] * ax0 + src[(y0 * w + x1) * 3 + c] * ax1;   // x2048
            const int bot = src[(y1 * w + x0) * 3 + c] * ax0 + src[(y1 * w + x1) * 3 + c] * ax1;
            const int r = (((ay0 * (top >> 4)) >> 16) + ((ay1 * (bot >> 4)) >> 16) + 2) >> 2;
            v[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
        }
    }
}

// resize_px_u8 on a WINDOW of a larger image (y4_window_u8_ragged): `src` is the window's first pixel, `pitch` the bytes of a
// source row (>= 3 * w), h x w the window.  The coefficients and the tap clamp are those of the h x w window (lin_coeff clamps at
// src - 1 = the window's last row / column), never the image around it, so the pixel is what resize_px_u8 gives on a contiguous
// copy of the window.  A separate overload: the packed callers above keep their int index arithmetic.
__device__ __forceinline__ void resize_px_u8(const uint8_t* __restrict__ src, int64_t pitch, int h, int w, int dh, int dw, int y, int x,
                                             int v[3]) {
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    lin_coeff(x, dw, w, x0, x1, ax0, ax1);
    lin_coeff(y, dh, h, y0, y1, ay0, ay1);
    const bool same = (h == dh && w == dw);
    const uint8_t* r0 = src + (same ? y : y0) * pitch;
    const uint8_t* r1 = src + y1 * pitch;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (same) {
            v[c] = r0[x * 3 + c];
        } else {
            const int top = r0[x0 * 3 + c] * ax0 + r0[x1 * 3 + c] * ax1;   // x2048
            const int bot = r1[x0 * 3 + c] * ax0 + r1[x1 * 3 + c] * ax1;
            const int r = (((ay0 * (top >> 4)) >> 16) + ((ay1 * (bot >> 4)) >> 16) + 2) >> 2;
            v[c] = r < 0 ? 0 : (r > 255 ? 255 : r);
        }
    }
}

// A thread's PX consecutive RGB pixels -> memory: PX = 4 stores its 12 bytes as three dwords (`o` 4-byte aligned), so that a
// wave covers 768 contiguous bytes; PX = 1 stores three bytes.
template <int PX>
__device__ __forceinline__ void store_px_u8(uint8_t* __restrict__ o, const uint8_t px[PX * 3]) {
    static_assert(PX == 1 || PX == 4, "store_px_u8: PX is 1 or 4");
    if constexpr (PX == 4) {
        uint32_t* o32 = (uint32_t*)o;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o32[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = px[c];
    }
}

// The host-side argument checks of the ragged launches (y4_resize_u8_ragged, y4_augment_u8_ragged): everything that can be
// checked without reading the device-resident descriptor table.
inline int ragged_args_check(const char* who, const void* src, const void* desc, const void* out, int n, int H, int W, int pad) {
    Y4_REQUIRE(src && desc && out, Y4_EINVAL, "%s: null pointer", who);
    Y4_REQUIRE(n > 0 && n <= 65535, Y4_EINVAL, "%s: n = %d (1..65535)", who, n);
    Y4_REQUIRE(H > 0 && W > 0, Y4_EINVAL, "%s: canvas %d x %d", who, H, W);
    Y4_REQUIRE(pad >= 0 && pad <= 255, Y4_EINVAL, "%s: pad_value %d (0..255)", who, pad);
    Y4_REQUIRE((int64_t)n * H * W * 3 < (1ll << 31), Y4_EINVAL, "%s: output of %lld bytes (< 2^31)", who,
               (long long)n * H * W * 3);
    return Y4_OK;
}

}  // namespace y4
