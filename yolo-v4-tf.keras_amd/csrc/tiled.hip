// tiled.hip -- the gather of tiled (sliced) inference, Engine.predict_tiled (its window crops are canvas_u8.hip's):
//   gather_kernel            y4_decode_gather: the candidate lists the decode stage left for several batch rows (tiles) are merged
//                            into ONE list per group (photo), boxes mapped to the photo's normalised coordinates, on which the
//                            NMS kernel of decode_nms.hip then runs unchanged (y4_nms_gathered).  ORIENTED
//                            (y4_decode_gather_views, test-time augmentation) swaps the corners an axis reads when its
//                            scale is negative: a mirrored row stores x1 <= x2, which the merge's componentwise mean needs.
#include "candidates.h"
#include "kernels.h"

#pragma clang fp contract(off)   // the box map is an explicit fmaf; nothing else may fuse

namespace y4 {

// ------------------------------------------------------------------------------------------- gather
// One workgroup per batch row i (a tile): the row's whole candidate list is read by this one workgroup, which is what lets it
// leave the row's counter at zero behind a single barrier -- the duty nms_kernel has on the plain path.  Per pass of
// GATHER_THREADS keys: the id (box, class) of a key is re-based to the group's box table, slot * nbox + box, the key is appended to
// the group's list with ONE returning atomic per wave (wave_append, as the decode kernels append), and the box is written,
// mapped to the photo, to its own place in the group's table: rows of one group write disjoint slots, and the up to C
// candidates of one box store the same four floats.  The order of a group's list varies from run to run; its keys are unique
// and nms_kernel sorts them.
constexpr int GATHER_THREADS = 1024;
template <bool ORIENTED>
__global__ __launch_bounds__(GATHER_THREADS) void gather_kernel(const GatherK p) {
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    uint32_t cnt = p.counts[(size_t)i * COUNT_STRIDE];
    if (cnt > p.cap) {                                   // cannot happen (cap = nbox * C is exact); kept as on the plain path
        if (tid == 0) atomicOr(p.status, 1u);
        cnt = p.cap;
    }
    __syncthreads();
    if (tid == 0) p.counts[(size_t)i * COUNT_STRIDE] = 0;   // every thread has read it: zero for the handle's next decode
    const int g = p.row_group[i], t = p.row_slot[i];
    if (g < 0 || g >= p.n_groups || t < 0 || t >= p.max_slots) return;      // (uniform) a bad table row writes nothing
    const float ax = p.row_map[4 * i], bx = p.row_map[4 * i + 1], ay = p.row_map[4 * i + 2], by = p.row_map[4 * i + 3];
    const unsigned long long* keys = p.keys + (int64_t)i * p.cap;
    const float* rb = p.dboxes + (int64_t)i * p.nbox * 4;
    unsigned long long* gkeys = p.gkeys + (int64_t)g * p.group_cap;
    float* gb = p.gboxes + ((int64_t)g * p.max_slots + t) * p.nbox * 4;
    uint32_t* gcount = p.gcounts + (size_t)g * COUNT_STRIDE;
    const uint32_t id0 = (uint32_t)t * (uint32_t)p.nbox * (uint32_t)p.C;    // < 2^31 with every id of the slot (checked on the host)
    for (uint32_t k0 = 0; k0 < cnt; k0 += GATHER_THREADS) {                  // (uniform trip count)
        const uint32_t k = k0 + (uint32_t)tid;
        const bool have = k < cnt;
        const unsigned long long key = have ? keys[k] : 0ull;
        const uint32_t b = have ? cand_box_class(key, p.C, p.div_c).box : 0u;
        const bool ok = have && b < (uint32_t)p.nbox;                        // (a key is (box < nbox, class < C) by construction)
        const uint32_t pos = wave_append(gcount, ok, lane);
        if (ok) {
            if (pos < p.group_cap) gkeys[pos] = cand_key(cand_score(key), id0 + cand_id(key));     // the score word stays
            float4 o = *(const float4*)(rb + (int64_t)b * 4);
            if constexpr (ORIENTED) {                    // (uniform per row) a mirrored axis: its low corner comes from the high one
                const float x1 = ax < 0.f ? o.z : o.x, x2 = ax < 0.f ? o.x : o.z;
                const float y1 = ay < 0.f ? o.w : o.y, y2 = ay < 0.f ? o.y : o.w;
                o.x = x1; o.y = y1; o.z = x2; o.w = y2;
            }
            o.x = fmaf(o.x, ax, bx); o.y = fmaf(o.y, ay, by);
            o.z = fmaf(o.z, ax, bx); o.w = fmaf(o.w, ay, by);
            *(float4*)(gb + (int64_t)b * 4) = o;
        }
    }
}

int gather_launch(const GatherK& k, int n, bool oriented, hipStream_t stream) {
    if (oriented) hipLaunchKernelGGL(gather_kernel<true>, dim3(n), dim3(GATHER_THREADS), 0, stream, k);
    else hipLaunchKernelGGL(gather_kernel<false>, dim3(n), dim3(GATHER_THREADS), 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

// The groups' raw candidate counts -> a dense int32 array, read before nms_kernel consumes and zeroes the counters
__global__ __launch_bounds__(256) void gather_counts_kernel(const uint32_t* __restrict__ gcounts, int32_t* __restrict__ out, int n_groups) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < n_groups) out[g] = (int32_t)gcounts[(size_t)g * COUNT_STRIDE];
}

int gather_counts_launch(const uint32_t* gcounts, int32_t* out, int n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(gather_counts_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, stream, gcounts, out, n_groups);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
