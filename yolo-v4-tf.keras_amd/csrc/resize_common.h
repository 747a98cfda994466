// resize_common.h -- the uint8 bilinear arithmetic every resize kernel shares (misc_kernels.hip: preprocess / resize kernels,
// canvas_u8.h: the descriptor-table kernel of canvas_u8.hip and yuv_u8.hip).
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

// A tap source says what source pixel (row, x) is, channel by channel: `row(y)` is whatever names source row y, `at(r, x, c)`
// the byte of channel c at column x of that row.  The bilinear arithmetic below is written once against it.  CHANNELS_SHARE_LOADS
// says whether the three channels of a tap come from the same loads (planes and a colour rule): the arithmetic is the same, only
// the copy-or-interpolate test then stands outside the channel loop, so that one block holds all three channels of a tap.
//
// PackedTap: packed RGB.  `src` is the source's first pixel and `pitch` the bytes of a source row: 3 * w for a packed image, more
// for a WINDOW of a larger image (y4_window_u8_ragged).  P is the index width of the row offset: int for the packed callers,
// int64_t for a pitch.
template <class P>
struct PackedTap {
    static constexpr bool CHANNELS_SHARE_LOADS = false;    // a channel is a byte of its own
    const uint8_t* __restrict__ src;
    P pitch;
    __device__ __forceinline__ const uint8_t* row(int y) const { return src + y * pitch; }
    __device__ __forceinline__ int at(const uint8_t* r, int x, int c) const { return r[x * 3 + c]; }
};

// One output pixel (row y, column x) of cv2.resize's uint8 INTER_LINEAR resize of an h x w source to dw x dh, all three channels:
// the arithmetic every uint8 resize kernel here shares (prepost.py: resize_bilinear is its host restatement).  The coefficients
// and the tap clamp are those of the h x w source (lin_coeff clamps at src - 1 = its last row / column), never of an image around
// it, so a window's pixel is that of a contiguous copy of the window.  A source of the output's size is copied.
template <class T>
__device__ __forceinline__ void resize_px_tap(const T& tap, int h, int w, int dh, int dw, int y, int x, int v[3]) {
    int x0, x1, ax0, ax1, y0, y1, ay0, ay1;
    lin_coeff(x, dw, w, x0, x1, ax0, ax1);
    lin_coeff(y, dh, h, y0, y1, ay0, ay1);
    const bool same = (h == dh && w == dw);
    const auto r0 = tap.row(same ? y : y0);
    const auto r1 = tap.row(y1);
    const auto lerp = [&](int c) __attribute__((always_inline)) {
        const int top = tap.at(r0, x0, c) * ax0 + tap.at(r0, x1, c) * ax1;   // x2048
        const int bot = tap.at(r1, x0, c) * ax0 + tap.at(r1, x1, c) * ax1;
        const int r = (((ay0 * (top >> 4)) >> 16) + ((ay1 * (bot >> 4)) >> 16) + 2) >> 2;
        return r < 0 ? 0 : (r > 255 ? 255 : r);
    };
    if constexpr (T::CHANNELS_SHARE_LOADS) {               // copy or interpolate is decided once: the channels of a tap are
        if (same) {                                        // then computed side by side and share its loads
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = tap.at(r0, x, c);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = lerp(c);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (same) v[c] = tap.at(r0, x, c);
            else v[c] = lerp(c);
        }
    }
}

// resize_px_tap on packed RGB.
template <class P>
__device__ __forceinline__ void resize_px_u8(const uint8_t* __restrict__ src, P pitch, int h, int w, int dh, int dw, int y, int x,
                                             int v[3]) {
    resize_px_tap(PackedTap<P>{src, pitch}, h, w, dh, dw, y, x, v);
}

}  // namespace y4
