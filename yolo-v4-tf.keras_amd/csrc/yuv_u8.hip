// yuv_u8.hip -- y4_yuv_u8_ragged: 8-bit 4:2:0 video frames (NV12, NV21, I420, YV12, any pitch) -> the uint8 network batch
// [n,H,W,3] in one launch.  The kernel is canvas_u8.h's template with one more row source, SlotRow<y4_yuv_desc>, whose tap source
// reads three planes and converts to RGB with the integer rule of include/yolo4hip.h; the bilinear arithmetic is the shared
// resize_px_tap on the converted taps, so a slot holds the bytes y4_resize_u8_ragged writes for the converted frame.  Host
// restatement: yolo4hip/yuv.py: to_rgb; tests/yuv_oracle.py is the float64 statement of the matrices.
#include "canvas_u8.h"

namespace y4 {

static_assert(sizeof(y4_yuv_desc) == 64, "y4_yuv_desc is 64 bytes (include/yolo4hip.h)");

// Three plane reads and the colour rule.  The descriptor is wave-uniform, so the coefficients and plane bases are scalar; a
// thread's four taps share chroma samples wherever x0 >> 1 == x1 >> 1 or y0 >> 1 == y1 >> 1, which the caches serve.
struct YuvTap {
    static constexpr bool CHANNELS_SHARE_LOADS = true;     // R, G and B of a tap are one Y, one U and one V
    const uint8_t* __restrict__ yp;
    const uint8_t* __restrict__ up;
    const uint8_t* __restrict__ vp;
    int y_pitch, c_pitch, c_step;
    int y0, cy, crv, cgu, cgv, cbu;
    struct Row {
        const uint8_t *y, *u, *v;
    };
    __device__ __forceinline__ Row row(int y) const {
        const int64_t c = (int64_t)(y >> 1) * c_pitch;
        return {yp + (int64_t)y * y_pitch, up + c, vp + c};
    }
    __device__ __forceinline__ int at(const Row& r, int x, int c) const {
        const int cx = (x >> 1) * c_step;
        const int C = (int)r.y[x] - y0, D = (int)r.u[cx] - 128, E = (int)r.v[cx] - 128;
        const int s = cy * C + (c == 0 ? crv * E : (c == 1 ? cgu * D + cgv * E : cbu * D)) + 8192;
        const int o = s >> 14;
        return o < 0 ? 0 : (o > 255 ? 255 : o);
    }
};

template <>
struct TapOf<y4_yuv_desc> {
    __device__ __forceinline__ static YuvTap make(const uint8_t* __restrict__ src, const y4_yuv_desc& d) {
        const bool bt709 = d.flags & Y4_YUV_BT709, full = d.flags & Y4_YUV_FULL_RANGE;
        YuvTap t;
        t.yp = src + d.y_offset;
        t.up = src + d.u_offset;
        t.vp = src + d.v_offset;
        t.y_pitch = d.y_pitch;
        t.c_pitch = d.c_pitch;
        t.c_step = d.c_step;
        t.y0 = full ? 0 : 16;
        t.cy = full ? 16384 : 19077;
        t.crv = bt709 ? (full ? 25802 : 29372) : (full ? 22970 : 26149);
        t.cgu = bt709 ? (full ? -3069 : -3494) : (full ? -5638 : -6419);
        t.cgv = bt709 ? (full ? -7670 : -8731) : (full ? -11700 : -13320);
        t.cbu = bt709 ? (full ? 30402 : 34610) : (full ? 29032 : 33050);
        return t;
    }
};

int yuv_u8_ragged_launch(const uint8_t* src, const y4_yuv_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                         hipStream_t stream) {
    return canvas_u8_launch("yuv_u8_ragged", src, SlotRow<y4_yuv_desc>{desc}, n, out, H, W, pad, stream);
}

}  // namespace y4
