// canvas_u8.h -- the one kernel template and the one launcher behind every launch that writes the uint8 network batch [n,H,W,3]
// through a device-resident descriptor table.  canvas_u8.hip instantiates it for packed RGB sources (resize, window, view,
// augment, mosaic), yuv_u8.hip for 4:2:0 video frames; the instantiations differ in the row source that says which descriptor
// governs a canvas pixel, and in the tap source (TapOf) that says what a source pixel of that descriptor is.
#pragma once
#include <type_traits>
#include "kernels.h"
#include "resize_common.h"

#pragma clang fp contract(off)   // hsv_px_u8 is float32 in the written order of operations; nothing may fuse

namespace y4 {

// One resized pixel through the colour rule, in float32:
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

// ---------------------------------------------------------------------------------------- row sources
// A row source answers: which descriptor governs canvas pixel (y, x) of slot b.  `open(b)` is called by every thread of the
// workgroup; `at(y, x)` gives the descriptor.  What a descriptor type carries beyond h, w and the canvas rectangle decides
// at compile time what the kernel does with it: a `pitch` (y4_window_desc, y4_view_desc) is the source row's bytes, a
// y4_view_desc has flip bits for both axes, a y4_augment_desc has a left-right flip and HSV, and a y4_yuv_desc names three
// planes instead of one packed image.
//
// One descriptor per slot, a wave-uniform load (scalar registers):
//   SlotRow<y4_image_desc>    a packed image;
//   SlotRow<y4_window_desc>   adds the pitch: a window of a larger image, many rows may read one image;
//   SlotRow<y4_view_desc>     a window whose canvas is mirrored (bit 0: left-right, bit 1: up-down);
//   SlotRow<y4_augment_desc>  adds flip and HSV, and a rectangle that may stick out of the canvas;
//   SlotRow<y4_yuv_desc>      an 8-bit 4:2:0 frame, converted to RGB tap by tap (yuv_u8.hip).
template <class D>
struct SlotRow {
    using Desc = D;
    const D* desc;
    struct Slot {
        D d;
        __device__ __forceinline__ const D& at(int, int) const { return d; }
    };
    __device__ __forceinline__ Slot open(int b) const { return {desc[b]}; }
};

// Mosaic adds the choice per pixel: four y4_augment_desc rows around a cut, pixel (y, x) under row 2 (y >= cut_y) + (x >= cut_x)
// on the WHOLE canvas.  A canvas's rows and its cut reach LDS once per workgroup (50 dwords, one per thread) and are read from
// there per pixel; a thread's PX pixels may lie on both sides of cut_x.  A row whose window is empty is never chosen, so its
// image is never dereferenced.
struct MosaicRows {
    using Desc = y4_augment_desc;
    const y4_augment_desc* desc;                           // [n][4]
    const y4_mosaic_cut* cuts;                             // [n]
    static constexpr int TILE_WORDS = 4 * sizeof(y4_augment_desc) / 4, CUT_WORDS = sizeof(y4_mosaic_cut) / 4;
    struct Slot {
        const uint32_t* table;
        __device__ __forceinline__ y4_augment_desc at(int y, int x) const {
            const int cut_y = (int)table[TILE_WORDS], cut_x = (int)table[TILE_WORDS + 1];
            return ((const y4_augment_desc*)table)[2 * (y >= cut_y) + (x >= cut_x)];
        }
    };
    __device__ __forceinline__ Slot open(int b) const {
        __shared__ __attribute__((aligned(16))) uint32_t table[TILE_WORDS + CUT_WORDS];
        if (threadIdx.x < TILE_WORDS) table[threadIdx.x] = ((const uint32_t*)(desc + 4 * (int64_t)b))[threadIdx.x];
        else if (threadIdx.x < TILE_WORDS + CUT_WORDS) table[threadIdx.x] = ((const uint32_t*)(cuts + b))[threadIdx.x - TILE_WORDS];
        __syncthreads();
        return {table};
    }
};

// ---------------------------------------------------------------------------------------- tap sources
// The bytes of a source row: the packed callers keep their int index arithmetic, a window's pitch indexes in 64 bits.
template <class D> __device__ __forceinline__ int src_pitch(const D& d) { return 3 * d.w; }
__device__ __forceinline__ int64_t src_pitch(const y4_window_desc& d) { return d.pitch; }
__device__ __forceinline__ int64_t src_pitch(const y4_view_desc& d) { return d.pitch; }

// What source pixels a descriptor of type D names (resize_common.h: a tap source).  Packed RGB at `offset` unless a descriptor
// type specialises it (yuv_u8.hip: three planes and the colour rule).
template <class D>
struct TapOf {
    __device__ __forceinline__ static auto make(const uint8_t* __restrict__ src, const D& d) {
        return PackedTap<decltype(src_pitch(d))>{src + d.offset, src_pitch(d)};
    }
};

// ------------------------------------------------------------------------------------------- kernel
// Grid y = canvas slot, grid x = PX consecutive CANVAS pixels per thread.  Pixels inside the descriptor's rectangle
// [pad_top, pad_top + out_h) x [pad_left, pad_left + out_w) are cv2.resize's uint8 INTER_LINEAR resize of the source to
// out_w x out_h (resize_px_tap), every other pixel is `pad` without the colour transform; the rectangle may lie partly or wholly
// outside the canvas (only its visible part is computed).  A flipped row mirrors the column a canvas pixel is SOURCED from
// (x' = W - 1 - x; a view's bit 1 likewise the row, y' = H - 1 - y), never where it is stored, so a flipped thread's stores are
// the same three dwords.  The source reads are
// gathers (two rows, bilinear taps) served from L1/L2; the writes are what this kernel can shape: with PX = 4 a thread stores its
// 12 bytes as three dwords and a wave covers 768 contiguous bytes, instead of 3 byte stores per pixel.  PX = 4 needs
// H * W % 4 == 0 (every network size: sides are multiples of 32) and a 4-byte aligned output; otherwise PX = 1.
template <int PX, class S>
__global__ __launch_bounds__(256) void canvas_u8_kernel(const uint8_t* __restrict__ src, const S rows, uint8_t* __restrict__ out,
                                                        int H, int W, int pad) {
    using D = typename S::Desc;
    constexpr bool AUGMENT = std::is_same<D, y4_augment_desc>::value;
    constexpr bool VIEW = std::is_same<D, y4_view_desc>::value;
    const int b = blockIdx.y;
    const typename S::Slot slot = rows.open(b);            // every thread: a source may stage its rows behind a barrier
    const int hw = H * W;                                  // < 2^31 (checked on the host)
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * PX;
    if (p0 >= hw) return;
    uint8_t px[PX * 3];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int p = p0 + k;
        const int y = p / W, x = p - y * W;
        const D d = slot.at(y, x);
        int xs = x, ys = y;
        if constexpr (AUGMENT) xs = d.flip ? W - 1 - x : x;
        if constexpr (VIEW) {
            xs = (d.flip & 1) ? W - 1 - x : x;
            ys = (d.flip & 2) ? H - 1 - y : y;
        }
        const int yy = ys - d.pad_top, xx = xs - d.pad_left;
        int v[3] = {pad, pad, pad};
        if (yy >= 0 && yy < d.out_h && xx >= 0 && xx < d.out_w) {
            resize_px_tap(TapOf<D>::make(src, d), d.h, d.w, d.out_h, d.out_w, yy, xx, v);
            if constexpr (AUGMENT)
                if (!(d.hue == 0.f && d.sat == 1.f && d.val == 1.f)) hsv_px_u8(v, d.hue, d.sat, d.val);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k * 3 + c] = (uint8_t)v[c];
    }
    store_px_u8<PX>(out + ((int64_t)b * hw + p0) * 3, px);
}

// The host-side argument checks (everything that can be checked without reading the device-resident table), the PX choice and
// the grid.
template <class S>
static int canvas_u8_launch(const char* who, const uint8_t* src, const S rows, int n, uint8_t* out, int H, int W, int pad,
                            hipStream_t stream) {
    Y4_REQUIRE(src && rows.desc && out, Y4_EINVAL, "%s: null pointer", who);
    Y4_REQUIRE(n > 0 && n <= 65535, Y4_EINVAL, "%s: n = %d (1..65535)", who, n);
    Y4_REQUIRE(H > 0 && W > 0, Y4_EINVAL, "%s: canvas %d x %d", who, H, W);
    Y4_REQUIRE(pad >= 0 && pad <= 255, Y4_EINVAL, "%s: pad_value %d (0..255)", who, pad);
    Y4_REQUIRE((int64_t)n * H * W * 3 < (1ll << 31), Y4_EINVAL, "%s: output of %lld bytes (< 2^31)", who,
               (long long)n * H * W * 3);
    const int hw = H * W;
    if (hw % 4 == 0 && ((uintptr_t)out & 3) == 0)
        hipLaunchKernelGGL((canvas_u8_kernel<4, S>), dim3((hw / 4 + 255) / 256, n), dim3(256), 0, stream, src, rows, out, H, W, pad);
    else
        hipLaunchKernelGGL((canvas_u8_kernel<1, S>), dim3((hw + 255) / 256, n), dim3(256), 0, stream, src, rows, out, H, W, pad);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
