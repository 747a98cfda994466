// feature_cache.hip -- y4_feature_store / y4_feature_load: the tensors a handle retains after a forward (the head convs' inputs,
// or at retention level 2 the inputs of the 3x3 convs in front of them) copied between the workspace views and dense cache rows.
//
// A pure copy, bound by HBM: one launch moves the three scales of all images of the call in 16-byte chunks.  The grid is sized
// from the bytes -- 4 chunks per thread and pass, at most 8 workgroups per compute unit, a grid-stride loop for the rest.
// Consecutive lanes take consecutive chunks, so every load and store instruction of a wave covers 1 KB of consecutive row bytes
// (in a view with a channel stride: runs of one pixel's channels, >= 256 B), and the four loads of a pass are issued before the
// first store.  Where a chunk lies follows from its index alone (kernels.h: FeatureK); the images' rows come from the slot
// table in the kernel argument, so the call needs no upload and no synchronisation.
#include "kernels.h"

namespace y4 {

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_UNROLL = 4;

// Scale 0's value, stepped to scale 1's and 2's under the two comparisons (unsigned, wrapping).  Which scale a chunk belongs to
// differs from lane to lane at the two seams of a row: read as `k.field[scale]` -- or as a select between the three fields, which
// the compiler turns into the same thing -- every parameter is a per-lane load of the kernel argument, nine more loads per
// 16-byte chunk.  This form keeps the three values and their differences in scalar registers: two v_cndmask and two adds.
template <class T>
__device__ __forceinline__ T fc_pick(bool s1, bool s2, T a, T b, T c) {
    return a + (s1 ? b - a : (T)0) + (s2 ? c - b : (T)0);
}

// the two addresses of chunk g: in the workspace view and in the cache
__device__ __forceinline__ void feature_chunk(const FeatureK& k, uint32_t g, char*& view, char*& cache) {
    const uint32_t img = fastdiv(g, k.row);
    const uint32_t r = g - img * k.row.d;
    const bool s1 = r >= k.first[1], s2 = r >= k.first[2];
#define FC_PICK(T, field) fc_pick<T>(s1, s2, (T)k.field[0], (T)k.field[1], (T)k.field[2])
    const uint32_t q = r - FC_PICK(uint32_t, first);
    const FastDiv cpp{fc_pick(s1, s2, k.cpp[0].mul, k.cpp[1].mul, k.cpp[2].mul), fc_pick(s1, s2, k.cpp[0].shr, k.cpp[1].shr, k.cpp[2].shr),
                      fc_pick(s1, s2, k.cpp[0].d, k.cpp[1].d, k.cpp[2].d)};
    const uint32_t px = fastdiv(q, cpp);
    const uint32_t cc = q - px * cpp.d;
    // (relative to scale 0's buffer, so that the address stays a global one)
    view = k.view[0] + (FC_PICK(uint64_t, view) - (uint64_t)k.view[0] + (uint64_t)img * FC_PICK(uint64_t, img_stride) +
                        (uint64_t)px * FC_PICK(uint32_t, pix_stride) + FC_PICK(uint32_t, coff) + cc * 16u);
    cache = k.cache + (uint64_t)(uint32_t)k.slot[img] * k.row_bytes + FC_PICK(uint32_t, off) + (uint64_t)q * 16u;
#undef FC_PICK
}

template <bool STORE>
__global__ __launch_bounds__(FC_THREADS) void feature_copy_kernel(const FeatureK k) {
    const uint32_t stride = gridDim.x * FC_THREADS;
    for (uint32_t g0 = blockIdx.x * FC_THREADS + threadIdx.x; g0 < k.total; g0 += stride * FC_UNROLL) {
        char* view[FC_UNROLL];
        char* cache[FC_UNROLL];
        u32x4_t v[FC_UNROLL];
#pragma unroll
        for (int u = 0; u < FC_UNROLL; ++u) {
            const uint32_t g = g0 + (uint32_t)u * stride;
            // (g0 + u * stride cannot wrap: total < 2^31 and stride * FC_UNROLL <= 2^23, see feature_copy_launch)
            if (g < k.total) {
                feature_chunk(k, g, view[u], cache[u]);
                v[u] = *(const u32x4_t*)(STORE ? view[u] : cache[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < FC_UNROLL; ++u)
            if (g0 + (uint32_t)u * stride < k.total) *(u32x4_t*)(STORE ? cache[u] : view[u]) = v[u];
    }
}

}  // namespace

int feature_copy_launch(const FeatureK& k, bool store, hipStream_t stream) {
    int cus = 0;
    if (int r = cu_count(&cus)) return r;
    const uint32_t per_block = FC_THREADS * FC_UNROLL;
    uint32_t grid = (k.total + per_block - 1) / per_block;
    grid = grid < 1 ? 1 : grid > (uint32_t)cus * 8 ? (uint32_t)cus * 8 : grid;
    if (grid > 8192) grid = 8192;                    // (keeps stride * FC_UNROLL at 2^23: the chunk index cannot wrap)
    if (store)
        hipLaunchKernelGGL(feature_copy_kernel<true>, dim3(grid), dim3(FC_THREADS), 0, stream, k);
    else
        hipLaunchKernelGGL(feature_copy_kernel<false>, dim3(grid), dim3(FC_THREADS), 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
