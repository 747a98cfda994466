// loss_common.h -- device helpers shared by loss.hip (the yolo_loss forward) and head_train.hip (its gradient).
#pragma once
#include "kernels.h"

namespace y4 {
namespace {

constexpr int LOSS_THREADS = 256;

// Compacts the rows with w > 0 of one image's [mb] rows into LDS order (row order kept): -> position of this thread's row, or
// -1; *total is the number of such rows.  One row per thread (mb <= LOSS_THREADS), called by every thread of the workgroup.
__device__ inline int compact_valid(bool valid, int* s_wave, int* total) {
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned long long bal = __ballot(valid);
    if ((tid & 63) == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const unsigned long long below = bal & ((1ull << (tid & 63)) - 1ull);
    return valid ? base + __popcll(below) : -1;
}

__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
// tf.nn.sigmoid_cross_entropy_with_logits, the stable form
__device__ inline float bce_logits(float x, float z) { return fmaxf(x, 0.0f) - x * z + log1pf(expf(-fabsf(x))); }

}  // namespace
}  // namespace y4
