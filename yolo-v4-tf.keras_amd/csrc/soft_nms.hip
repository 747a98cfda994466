// soft_nms.hip -- Soft-NMS (Bodla et al. 2017) over a candidate list: y4_set_nms_soft.  Where nms_kernel deletes a neighbour of a
// kept box, this kernel multiplies the neighbour's score by a factor below 1, so the next box to keep is the maximum of the
// CURRENT scores and the output order is not the input order: nothing of nms_kernel's "an earlier candidate is decided before a
// later one" holds, hence a kernel of its own.  It shares nms_kernel's candidate store, LDS carve-up, selectors and output stage
// (nms_phases.h) and the pair measure (nms_measure.h).
//
// The rule, per list (include/yolo4hip.h states it for callers):
//   P = the top_k largest keys (all when the list is shorter: the exact radix select, never the histogram pivot);
//   w_j = s_j; then, until max_total boxes are kept: k = the live j (not kept, not turned away, w_j > min_score) with the largest
//   key cand_key(w_j, id_j); none -> stop; k's class full (max_per_class) -> k is turned away, decays nothing; else k is kept with
//   score w_k and every other live j of its class (of any class: AGN) gets w_j *= f(m), m = nms_measure<KIND>(B_j, B_k, -inf, beta):
//     gaussian  f = m > 0 ? expf(-(m * m) / sigma) : 1        linear  f = m > iou_thr ? 1 - m : 1        hard  f = m > iou_thr ? 0 : 1
//
// Schedule: one workgroup of NMS_THREADS per list, the participants in REGISTERS (up to SORT_CAP / NMS_THREADS per thread: id,
// working score, box, class, kept boxes of its class so far), in the order nms_take_chunk left them -- which varies from run to
// run and does not matter: a pick is an arg-max over unique keys and every w_j depends on the pick sequence alone.  A pick is a
// wave maximum by shuffles, one 16-byte slot per wave in LDS, ONE workgroup barrier (the slots are double-buffered by pick
// parity), a 16-lane maximum over the slots, and the winner's box read from the chunk's box table in LDS by its position.  The
// class cap needs no per-class words: every candidate counts the kept boxes of its own class and the winner's count travels in
// its slot.  No floating-point atomics anywhere.
#include "candidates.h"
#include "kernels.h"
#include "nms_measure.h"
#include "nms_phases.h"

#pragma clang fp contract(off)   // keep the float32 op order of the rule (no fused multiply-add)

namespace y4 {

enum { SOFT_GAUSSIAN = 1, SOFT_LINEAR = 2, SOFT_HARD = 3 };
constexpr int SOFT_WAVES = NMS_THREADS / 64;

// what a wave publishes per pick: its best live key, where that candidate sits in the chunk, the kept boxes of its class so far
struct SoftSlot { unsigned long long key; uint32_t pos, same; };
static_assert(sizeof(SoftSlot) == 16, "two buffers of SOFT_WAVES slots of 16 bytes behind nms_kernel's layout");

// nms_kernel's layout with the pick slots behind it, 16-byte aligned
__host__ __device__ inline uint32_t soft_slots_offset(int max_total, int C) { return (nms_lds_layout(max_total, C).bytes + 15u) & ~15u; }
static size_t soft_lds_bytes(int max_total, int C) { return (size_t)soft_slots_offset(max_total, C) + 2 * SOFT_WAVES * sizeof(SoftSlot); }

template <int METHOD>
__device__ __forceinline__ float soft_factor(float m, float iou_thr, float sigma) {
    if (METHOD == SOFT_GAUSSIAN) return m > 0.f ? expf(-(m * m) / sigma) : 1.f;      // (a NaN or negative measure decays nothing)
    if (METHOD == SOFT_LINEAR) return m > iou_thr ? 1.f - m : 1.f;
    return m > iou_thr ? 0.f : 1.f;
}

template <int KIND, bool AGN, int METHOD>
__global__ __launch_bounds__(NMS_THREADS) void soft_nms_kernel(const NmsK p, const DecayK sp) {
    extern __shared__ __attribute__((aligned(16))) char nsm[];
    const NmsLds L(nsm, p.max_total, p.C);
    SoftSlot* const slots = (SoftSlot*)(nsm + soft_slots_offset(p.max_total, p.C));
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const NmsList list = nms_list_begin(p, L, n, tid);

    // ---- participants: exactly the top_k largest keys, unsorted, and their boxes
    uint32_t m2;
    const uint32_t m = nms_take_top_k(L, list.gk, list.cnt, (uint32_t)sp.top_k, tid, &m2);
    nms_load_boxes(L, list.gb, p, m, tid);

    uint32_t id[NMS_NE], same[NMS_NE];
    float w[NMS_NE];
    float4 box[NMS_NE];
    int cls[NMS_NE];
    bool live[NMS_NE];
#pragma unroll
    for (int e = 0; e < NMS_NE; ++e) {
        const uint32_t pos = (uint32_t)(tid + NMS_THREADS * e);
        const bool have = pos < m;
        const unsigned long long key = have ? L.skey[pos] : 0ull;
        id[e] = cand_id(key);
        w[e] = cand_score(key);
        box[e] = have ? L.sbox[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
        cls[e] = cand_box_class(key, p.C, p.div_c).cls;
        same[e] = 0;
        live[e] = have && w[e] > sp.min_score;
    }

    // ---- the pick loop.  Every exit and `continue` is workgroup-uniform: all threads read the same slots
    const bool cap_binds = p.max_per_class < p.max_total;
    int kept = 0;
    for (int r = 0; kept < p.max_total; ++r) {
        unsigned long long best = 0;
        uint32_t bpos = 0, bsame = 0;
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            const unsigned long long k = live[e] ? cand_key(w[e], id[e]) : 0ull;
            if (k > best) { best = k; bpos = (uint32_t)(tid + NMS_THREADS * e); bsame = same[e]; }
        }
        unsigned long long wmax = best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(wmax, o);
            wmax = v > wmax ? v : wmax;
        }
        SoftSlot* const buf = slots + (r & 1) * SOFT_WAVES;          // (pick r + 2 writes here again: two barriers later)
        if (wmax == 0ull ? lane == 0 : best == wmax) {               // (working keys are unique: one lane)
            SoftSlot s;
            s.key = wmax; s.pos = bpos; s.same = bsame;
            buf[wv] = s;
        }
        __syncthreads();
        const unsigned long long skey = buf[lane & (SOFT_WAVES - 1)].key;
        unsigned long long kmax = skey;
#pragma unroll
        for (int o = SOFT_WAVES / 2; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(kmax, o);
            kmax = v > kmax ? v : kmax;
        }
        if (kmax == 0ull) break;                                     // no live candidate is left
        const int widx = __ffsll((long long)__ballot(skey == kmax)) - 1;      // (< SOFT_WAVES: lanes 0 .. 15 hold every slot)
        const uint32_t wpos = buf[widx].pos, wsame = buf[widx].same;
        const int wcls = cand_box_class(kmax, p.C, p.div_c).cls;
        // the winner leaves the pool, kept or turned away
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e)
            if ((uint32_t)(tid + NMS_THREADS * e) == wpos) live[e] = false;
        if (cap_binds && (int)wsame >= p.max_per_class) continue;    // its class is full: not kept, decays nothing
        const float4 kb = L.sbox[wpos];
        if (tid == 0) L.keep((uint32_t)kept, kb, wcls, kmax, cand_box_class(kmax, p.C, p.div_c).box);     // score = w at the pick
        ++kept;
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            if (!live[e]) continue;
            const bool mine = cls[e] == wcls;
            if (mine) ++same[e];
            if (AGN || mine) {
                const float f = soft_factor<METHOD>(nms_measure<KIND>(box[e], kb, -INFINITY, p.beta), p.iou_thr, sp.sigma);
                w[e] = w[e] * f;
                live[e] = w[e] > sp.min_score;
            }
        }
    }
    if (tid == 0) L.w->kept = (uint32_t)kept;
    __syncthreads();
    nms_write_outputs(p, L, n, tid);
}

struct SoftKernel { template <int KIND, bool AGN, int METHOD> static constexpr auto kernel = soft_nms_kernel<KIND, AGN, METHOD>; };

int soft_nms_launch(const NmsK& k, const DecayK& s, hipStream_t stream) {
    const size_t lds = soft_lds_bytes(k.max_total, k.C);
    Y4_REQUIRE(lds <= 160 * 1024 && k.max_total <= 1024 && s.top_k >= 1 && s.top_k <= SORT_CAP, Y4_EINVAL,
               "soft nms: top_k %d, max_total %d and %d classes need %zu bytes of LDS", s.top_k, k.max_total, k.C, lds);
    if (int r = nms_rule_check("soft nms", k.kind, k.beta, k.agnostic)) return r;
    Y4_REQUIRE(s.method >= SOFT_GAUSSIAN && s.method <= SOFT_HARD && s.sigma > 0.f && s.min_score >= 0.f, Y4_EINVAL,
               "soft nms: mode (method %d, sigma %g, min_score %g)", s.method, (double)s.sigma, (double)s.min_score);
    return nms_dispatch<SoftKernel>(std::make_index_sequence<6 * 3>(), s.method, lds, stream, k, s);
}

}  // namespace y4
