// box_merge.hip -- merge-NMS (box voting; YOLOv5's merge=True, the box step of weighted box fusion): behind nms_kernel each kept
// box is replaced by the score-weighted mean of the candidates it absorbed (y4_decode_nms_merged, y4_nms_gathered_merged).
//
// The kept set, its order, scores, classes, valid and kept_idx are nms_kernel's; only the four floats of a kept box change.
// For the kept box k of a list -- unclipped box B_k, class c_k, candidate id -- a candidate j of the list's first min(count, cap)
// keys (ALL of them, also those nms_kernel never visited because it had its max_total boxes) is a MEMBER when
//     class_j == c_k (any class under an agnostic rule)   and   nms_measure(B_j, B_k, thr, beta) > thr
// -- the float32 function and strict comparison that suppresses (nms_measure.h), on the boxes the pair measure is taken on: the
// canvas-normalised boxes of the decode stage, or the photo-normalised boxes of a gathered group's table.  Candidate k itself is a
// member by its id.  A candidate with a component that is not finite or of magnitude above 2^8 is never a member, and a kept box
// with such a component stays as nms_kernel wrote it.
//
// The mean is accumulated in integers, so that it does not depend on the order of the list (which varies from run to run) nor on
// the reduction tree:  wq_j = llrint(score_j * 2^30),  t_j[c] = llrint(score_j * B_j[c] * 2^30)  with both products formed exactly
// in float64 (24 x 24 significand bits) and rounded to nearest even; S_w = sum wq_j and S[c] = sum t_j[c] in int64;
//     B'_k[c] = (float)((double)S[c] / (double)S_w)        (S_w == 0: the box stays)
// componentwise on the stored floats, then the box map (fmaf) and the clip of nms_write_outputs.  |t_j| <= 2^38, so a list capacity
// below 2^25 (MERGE_MAX_CAP, checked on the host) keeps |S[c]| < 2^63.
//
// One workgroup per (list, kept slot): its threads stride over the list's keys, skip other classes before they touch the box
// table, accumulate five int64 sums each and reduce them through the wave and LDS; thread 0 writes the box.  No atomics, no scratch.
#include "candidates.h"
#include "kernels.h"
#include "nms_measure.h"

#pragma clang fp contract(off)

namespace y4 {

constexpr int MERGE_THREADS = 256;

// every component finite and of magnitude at most 2^8 (a NaN fails the comparison)
__device__ __forceinline__ bool merge_usable(const float4 b) {
    return fabsf(b.x) <= 256.f && fabsf(b.y) <= 256.f && fabsf(b.z) <= 256.f && fabsf(b.w) <= 256.f;
}

__device__ __forceinline__ long long merge_fixed(double x) { return (long long)__builtin_rint(x * 1073741824.0); }

template <int KIND>
__global__ __launch_bounds__(MERGE_THREADS) void box_merge_kernel(const MergeK p) {
    const int n = (int)(blockIdx.x / (uint32_t)p.max_total), slot = (int)(blockIdx.x - (uint32_t)n * (uint32_t)p.max_total);
    const int tid = threadIdx.x, lane = tid & 63;
    // (every early return below is uniform over the workgroup and in front of its only barrier)
    if (slot >= p.out_valid[n]) return;
    const int64_t o = (int64_t)n * p.max_total + slot;
    const int kbox = p.out_idx[o];
    if ((uint32_t)kbox >= (uint32_t)p.nbox) return;                        // (kept_idx is a box of the table by construction)
    const int kcls = (int)p.out_classes[o];
    const uint32_t kid = cand_make_id((uint32_t)kbox, (uint32_t)kcls, p.C);
    const float* gb = p.dboxes + (int64_t)n * p.nbox * 4;
    const float4 kb = *(const float4*)(gb + (int64_t)kbox * 4);
    if (!merge_usable(kb)) return;                                         // stays unmerged
    const int32_t raw = p.counts[n];
    const uint32_t cnt = raw <= 0 ? 0u : ((uint32_t)raw < p.cap ? (uint32_t)raw : p.cap);
    const unsigned long long* gk = p.keys + (int64_t)n * p.cap;

    long long s[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = tid; i < cnt; i += MERGE_THREADS) {
        const unsigned long long key = gk[i];
        const uint32_t id = cand_id(key);
        const CandBoxClass bc = cand_box_class(key, p.C, p.div_c);
        if (!p.agnostic && bc.cls != kcls) continue;
        if (bc.box >= (uint32_t)p.nbox) continue;                          // (a key is (box < nbox, class < C) by construction)
        const float4 cb = *(const float4*)(gb + (int64_t)bc.box * 4);
        if (!merge_usable(cb)) continue;
        if (id != kid && !(nms_measure<KIND>(cb, kb, p.iou_thr, p.beta) > p.iou_thr)) continue;
        const double w = (double)cand_score(key);
        s[0] += merge_fixed(w);
        s[1] += merge_fixed(w * (double)cb.x);
        s[2] += merge_fixed(w * (double)cb.y);
        s[3] += merge_fixed(w * (double)cb.z);
        s[4] += merge_fixed(w * (double)cb.w);
    }
    __shared__ long long part[MERGE_THREADS / 64][5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        long long v = s[c];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0) part[tid >> 6][c] = v;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        s[c] = 0;
        for (int w = 0; w < MERGE_THREADS / 64; ++w) s[c] += part[w][c];
    }
    if (s[0] == 0) return;                                                 // no weight: the box stays
    const double sw = (double)s[0];
    float4 b;
    b.x = (float)((double)s[1] / sw); b.y = (float)((double)s[2] / sw);
    b.z = (float)((double)s[3] / sw); b.w = (float)((double)s[4] / sw);
    if (p.box_map) {                                                       // as nms_write_outputs: map, then clip
        const float ax = p.box_map[4 * n], bx = p.box_map[4 * n + 1], ay = p.box_map[4 * n + 2], by = p.box_map[4 * n + 3];
        b.x = fmaf(b.x, ax, bx); b.y = fmaf(b.y, ay, by);
        b.z = fmaf(b.z, ax, bx); b.w = fmaf(b.w, ay, by);
    }
    b.x = fmaxf(fminf(b.x, 1.f), 0.f); b.y = fmaxf(fminf(b.y, 1.f), 0.f);
    b.z = fmaxf(fminf(b.z, 1.f), 0.f); b.w = fmaxf(fminf(b.w, 1.f), 0.f);
    *(float4*)(p.out_boxes + o * 4) = b;
}

int box_merge_launch(const MergeK& k, hipStream_t stream) {
    Y4_REQUIRE(k.cap < MERGE_MAX_CAP, Y4_EINVAL, "merge-NMS: a list capacity of %u keys is not below the 2^25 the int64 sums allow", k.cap);
    Y4_REQUIRE(k.N >= 1 && k.max_total >= 1 && (int64_t)k.N * k.max_total < (1ll << 31), Y4_EINVAL, "merge-NMS: %d lists of %d slots",
               k.N, k.max_total);
    if (int r = nms_rule_check("merge-NMS", k.kind, k.beta, k.agnostic)) return r;
    const dim3 grid((uint32_t)k.N * (uint32_t)k.max_total), block(MERGE_THREADS);
    const int measure = nms_measure_index(k.kind, k.beta);      // (as the NMS launchers choose it)
    if (measure == NMS_IOU) hipLaunchKernelGGL(box_merge_kernel<NMS_IOU>, grid, block, 0, stream, k);
    else if (measure == NMS_DIOU1) hipLaunchKernelGGL(box_merge_kernel<NMS_DIOU1>, grid, block, 0, stream, k);
    else hipLaunchKernelGGL(box_merge_kernel<NMS_DIOU>, grid, block, 0, stream, k);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
