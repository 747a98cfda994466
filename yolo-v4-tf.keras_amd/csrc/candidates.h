// candidates.h -- the candidate list that the decode kernels write, gather_kernel merges and nms_kernel reads (device code of
// decode_nms.hip and tiled.hip): the 64-bit key of a candidate and the wave-aggregated append to a list.
#pragma once
#include "common.h"

namespace y4 {

// A candidate is a 64-bit key  (score bits << 32) | ~id,  id = box_index * C + class  (< 2^31: checked on the host).  Scores are
// non-negative floats, whose bit patterns order as the values do, so sorting keys descending gives (score desc, box index asc, class
// asc) -- the tie order this build defines.  Keys of one list are unique and non-zero.
__device__ __forceinline__ uint32_t cand_make_id(uint32_t box, uint32_t cls, int C) { return box * (uint32_t)C + cls; }
__device__ __forceinline__ unsigned long long cand_key(float score, uint32_t id) {
    return ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(~id);
}
__device__ __forceinline__ uint32_t cand_id(unsigned long long key) { return ~(uint32_t)(key & 0xffffffffull); }
__device__ __forceinline__ float cand_score(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
struct CandBoxClass { uint32_t box; int cls; };
__device__ __forceinline__ CandBoxClass cand_box_class(unsigned long long key, int C, const FastDiv div_c) {
    const uint32_t id = cand_id(key);
    CandBoxClass r;
    r.box = fastdiv(id, div_c);
    r.cls = (int)(id - r.box * (uint32_t)C);
    return r;
}

// Room for `n` entries behind *count (a counter in global memory or in LDS), taken with ONE returning atomic by lane 0 and
// broadcast -> the first position.  All 64 lanes of the wave must be here, with the same `count` and `n`.
__device__ __forceinline__ uint32_t wave_reserve(uint32_t* count, uint32_t n, int lane) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, n);
    return __shfl(base, 0);
}

// The lanes with `take` each append one entry: ballot + popcount, one atomic per wave instead of one per entry (a thousand
// same-address atomics serialise) -> this lane's position, which means something on the `take` lanes only.  All 64 lanes of the
// wave must be here with the same `count`: every call site sits behind wave-uniform control flow alone (whole workgroups of 256
// or 1024 threads; the early returns in front of the sites depend on the block or wave index only).
__device__ __forceinline__ uint32_t wave_append(uint32_t* count, bool take, int lane) {
    const unsigned long long mask = __ballot(take);
    if (!mask) return 0u;                                      // wave-uniform
    return wave_reserve(count, (uint32_t)__popcll(mask), lane) + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

}  // namespace y4
