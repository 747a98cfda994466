// canvas_u8.hip -- every launch that writes the uint8 network batch [n,H,W,3] from packed uint8 sources through a device-resident
// descriptor table: y4_resize_u8_ragged (letterbox / mixed-size batches), y4_window_u8_ragged (tiled inference),
// y4_view_u8_ragged (test-time augmentation: a window, mirrored left-right and / or up-down), y4_augment_u8_ragged and
// y4_mosaic_u8_ragged (the training input of Yolov4.fit).  One kernel template, one launcher; the
// entry points differ only in the row source that says which descriptor governs a canvas pixel.  All randomness of the training
// input is drawn on the host (yolo4hip/augment.py: draw_params): the kernel is a pure function of its table.  Host restatements:
// prepost.py: letterbox, augment.py: augment_host / mosaic_host; tests/augment_oracle.py is the float64 colour oracle.
// The template itself (row sources, kernel, launcher) is canvas_u8.h, shared with yuv_u8.hip; this unit holds the five
// instantiations on packed RGB sources.
#include "canvas_u8.h"

namespace y4 {

int resize_u8_ragged_launch(const uint8_t* src, const y4_image_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                            hipStream_t stream) {
    return canvas_u8_launch("resize_u8_ragged", src, SlotRow<y4_image_desc>{desc}, n, out, H, W, pad, stream);
}

int window_u8_ragged_launch(const uint8_t* src, const y4_window_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                            hipStream_t stream) {
    return canvas_u8_launch("window_u8_ragged", src, SlotRow<y4_window_desc>{desc}, n, out, H, W, pad, stream);
}

int view_u8_ragged_launch(const uint8_t* src, const y4_view_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                          hipStream_t stream) {
    return canvas_u8_launch("view_u8_ragged", src, SlotRow<y4_view_desc>{desc}, n, out, H, W, pad, stream);
}

int augment_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* desc, int n, uint8_t* out, int H, int W, int pad,
                             hipStream_t stream) {
    return canvas_u8_launch("augment_u8_ragged", src, SlotRow<y4_augment_desc>{desc}, n, out, H, W, pad, stream);
}

int mosaic_u8_ragged_launch(const uint8_t* src, const y4_augment_desc* tiles, const y4_mosaic_cut* cuts, int n, uint8_t* out, int H,
                            int W, int pad, hipStream_t stream) {
    Y4_REQUIRE(cuts, Y4_EINVAL, "mosaic_u8_ragged: null pointer");
    return canvas_u8_launch("mosaic_u8_ragged", src, MosaicRows{tiles, cuts}, n, out, H, W, pad, stream);
}

}  // namespace y4
