// resize_common.h -- the uint8 bilinear arithmetic every resize kernel shares (misc_kernels.hip: preprocess / resize kernels,
// canvas_u8.hip: the descriptor-table kernel).
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

// One output pixel (row y, column x) of cv2.resize's uint8 INTER_LINEAR resize of an h x w source to dw x dh, all three channels:
// the arithmetic every uint8 resize kernel here shares (prepost.py: resize_bilinear is its host restatement).  `src` is the
// source's first pixel and `pitch` the bytes of a source row: 3 * w for a packed image, more for a WINDOW of a larger image
// (y4_window_u8_ragged).  The coefficients and the tap clamp are those of the h x w source (lin_coeff clamps at src - 1 = its last
// row / column), never of an image around it, so a window's pixel is that of a contiguous copy of the window.  P is the index
// width of the row offset: int for the packed callers, int64_t for a pitch.
template <class P>
__device__ __forceinline__ void resize_px_u8(const uint8_t* __restrict__ src, P pitch, int h, int w, int dh, int dw, int y, int x,
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

}  // namespace y4
