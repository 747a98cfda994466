// matrix_nms.hip -- Matrix-NMS (Wang et al., SOLOv2, 2020) over a candidate list: y4_set_nms_matrix.  Like Soft-NMS it decays scores
// instead of deleting boxes, but every decayed score is a closed-form function of the pair measures and the ORIGINAL score order, so
// there is no pick sequence: two data-parallel passes over the pairs and one more sort.  It shares nms_kernel's candidate store, LDS
// carve-up, selectors, sorts and output stage (nms_phases.h) and the pair measure (nms_measure.h).
//
// The rule, per list (include/yolo4hip.h states it for callers):
//   P = the top_k largest keys (all when the list is shorter: the exact radix select), ordered by key, largest first; i < j: i is
//   earlier.  i and j interact iff they have one class (always: AGN).  m+_ij = max(nms_measure<KIND>(B_i, B_j, -inf, beta), 0), a
//   NaN counting as 0.
//     c_i = max over interacting k < i of m+_ki                      (0 without such a k)
//     d_j = min over interacting i < j of t_ij                       (1 without such an i)
//       gaussian  t = expf((c_i * c_i - m+ * m+) / sigma)            linear  t = (1 - m+) / (1 - c_i) where c_i < 1, else no term
//     w_j = s_j * d_j
//   The j with w_j > min_score, by cand_key(w_j, id_j) descending; one whose class already has max_per_class boxes is skipped; the
//   first max_total are the result, with scores w_j.
//
// Schedule: one workgroup of NMS_THREADS per list, position tid + NMS_THREADS * e of the ordered list in the registers of thread tid.
// Class-aware launches order the participants by (class, key) -- a second sort, of (class, rank) words in the upper half of the box
// slots, which the sorts' exchange buffer leaves free -- so that a candidate's partners are the positions in front of it in its own
// class SEGMENT, [slo, q); agnostic launches keep the key order, where the segment is the whole list.  A wave walks i over the
// segments of its 64 positions with wave-uniform LDS reads (a broadcast each) and every lane tests slo <= i < q for itself: at
// most 64 wasted iterations.  Two facts keep pass 2 short: the first candidate of a segment has c = 0, so d <= 1 always, and a
// pair with m+ = 0 has t >= 1 under either method -- such pairs are passed over.  A candidate is skipped by the class cap iff
// max_per_class keys of its class are larger than its own (a skipped one still counts for the later ones of its class, which are
// skipped too), so the cap is one more pass over the segment, taken only when the cap can bind, that zeroes the keys it turns
// away; the walk is then "the first max_total keys after the sort".  Maximum and minimum are taken per thread in a fixed loop: no
// atomics on scores, the same bits whatever order the list arrived in.
#include "candidates.h"
#include "kernels.h"
#include "nms_measure.h"
#include "nms_phases.h"

#pragma clang fp contract(off)   // keep the float32 op order of the rule (no fused multiply-add)

namespace y4 {

enum { MATRIX_GAUSSIAN = 1, MATRIX_LINEAR = 2 };

// nms_kernel's layout with [SORT_CAP] floats behind it, 16-byte aligned: c of every position
__host__ __device__ inline uint32_t matrix_c_offset(int max_total, int C) { return (nms_lds_layout(max_total, C).bytes + 15u) & ~15u; }
static size_t matrix_lds_bytes(int max_total, int C) { return (size_t)matrix_c_offset(max_total, C) + (size_t)SORT_CAP * 4; }

// keys in (class ascending, key descending) order in ord[0 .. m): -> the number of positions with a class below c
__device__ __forceinline__ uint32_t matrix_first_of(const unsigned long long* ord, uint32_t m, int c, int C, const FastDiv div_c) {
    uint32_t lo = 0, n = m;
    while (n > 0) {
        const uint32_t half = n >> 1;
        if (cand_box_class(ord[lo + half], C, div_c).cls < c) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    return lo;
}

__device__ __forceinline__ void matrix_sort(const NmsLds& X, uint32_t m, uint32_t m2, int tid) {
    if (m2 <= (uint32_t)NMS_THREADS) nms_rank_sort(X, m, m2, tid);
    else nms_sort_regs<NMS_NE>(X.skey, X.xbuf(), m2, tid);
}

template <int KIND, bool AGN, int METHOD>
__global__ __launch_bounds__(NMS_THREADS) void matrix_nms_kernel(const NmsK p, const DecayK mp) {
    extern __shared__ __attribute__((aligned(16))) char nsm[];
    const NmsLds L(nsm, p.max_total, p.C);
    float* const c_a = (float*)(nsm + matrix_c_offset(p.max_total, p.C));
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const NmsList list = nms_list_begin(p, L, n, tid);
    const float* gb = list.gb;

    // ---- participants: exactly the top_k largest keys, sorted descending
    uint32_t m2;
    const uint32_t m = nms_take_top_k(L, list.gk, list.cnt, (uint32_t)mp.top_k, tid, &m2);
    matrix_sort(L, m, m2, tid);

    // ---- the ordered list in skey: the key order (AGN), or (class ascending, key descending)
    if (!AGN) {
        NmsLds X = L;
        X.skey = (unsigned long long*)L.sbox + SORT_CAP;        // (the exchange buffer is the lower half of the box slots)
        // (C - class, m2 - rank): unique, non-zero, descending = class ascending, then rank ascending
        for (uint32_t i = tid; i < m2; i += NMS_THREADS)
            X.skey[i] = i < m ? ((unsigned long long)(uint32_t)(p.C - cand_box_class(L.skey[i], p.C, p.div_c).cls) << 32) | (unsigned long long)(m2 - i) : 0ull;
        __syncthreads();
        matrix_sort(X, m, m2, tid);
        unsigned long long moved[NMS_NE];
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
            moved[e] = q < m ? L.skey[m2 - (uint32_t)(X.skey[q] & 0xffffffffull)] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
            if (q < m) L.skey[q] = moved[e];
        }
        __syncthreads();
    }
    unsigned long long* const ord = L.skey;
    nms_load_boxes(L, gb, p, m, tid);                                  // sbox[q] = the box of ord[q]; ends with a barrier

    unsigned long long key[NMS_NE];
    float4 box[NMS_NE];
    int cls[NMS_NE];
    uint32_t slo[NMS_NE];                   // the first position of this candidate's segment
    uint32_t lo[NMS_NE], hi[NMS_NE];        // wave-uniform: the positions this wave's pair loops visit for register e
#pragma unroll
    for (int e = 0; e < NMS_NE; ++e) {
        const uint32_t q = (uint32_t)(tid + NMS_THREADS * e), base = (uint32_t)((tid & ~63) + NMS_THREADS * e);
        const bool have = q < m;
        key[e] = have ? ord[q] : 0ull;
        box[e] = have ? L.sbox[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        cls[e] = cand_box_class(key[e], p.C, p.div_c).cls;
        slo[e] = AGN || !have ? 0u : matrix_first_of(ord, m, cls[e], p.C, p.div_c);
        lo[e] = hi[e] = 0;
        if (base < m) {                                                // (wave-uniform; lane 0 holds position `base`)
            hi[e] = base + 64 < m ? base + 64 : m;
            lo[e] = __shfl(slo[e], 0);
        }
    }

    // ---- pass 1: c_j = the largest m+ against an earlier candidate of its segment
#pragma unroll
    for (int e = 0; e < NMS_NE; ++e) {
        const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
        float c = 0.f;
        for (uint32_t i = lo[e]; i < hi[e]; ++i) {
            if (i >= slo[e] && i < q && q < m) {
                const float ms = nms_measure<KIND>(L.sbox[i], box[e], -INFINITY, p.beta);
                c = ms > c ? ms : c;                                   // (a NaN or negative measure changes nothing)
            }
        }
        if (q < m) c_a[q] = c;
    }
    __syncthreads();

    // ---- pass 2: d_j, and the decayed key
    const bool cap_binds = p.max_per_class < p.max_total;
#pragma unroll
    for (int e = 0; e < NMS_NE; ++e) {
        const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
        float d = 1.f;
        for (uint32_t i = lo[e]; i < hi[e]; ++i) {
            if (i >= slo[e] && i < q && q < m) {
                const float ms = nms_measure<KIND>(L.sbox[i], box[e], -INFINITY, p.beta);
                if (ms > 0.f) {                                        // (m+ = 0: t >= 1, and d <= 1 already)
                    const float ci = c_a[i];
                    if (METHOD == MATRIX_GAUSSIAN) {
                        const float t = expf((ci * ci - ms * ms) / mp.sigma);
                        d = t < d ? t : d;
                    } else if (ci < 1.f) {
                        const float t = (1.f - ms) / (1.f - ci);
                        d = t < d ? t : d;
                    }
                }
            }
        }
        const float w = cand_score(key[e]) * d;
        key[e] = q < m && w > mp.min_score ? cand_key(w, cand_id(key[e])) : 0ull;
    }
    unsigned long long* const dkey = ord;         // the decayed keys take the places of the original ones (each thread read its own)
    if (cap_binds) {
        // ---- the class cap: a key with max_per_class larger keys of its class in front of it is turned away
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e)
            // (class-aware: the end of the last lane's segment, from the ORIGINAL keys -- before anybody overwrites them)
            hi[e] = hi[e] == 0 ? 0u : (AGN ? m : __shfl(matrix_first_of(ord, m, cls[e] + 1, p.C, p.div_c), (int)(hi[e] - 1u) & 63));
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
            if (q < m) dkey[q] = key[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NMS_NE; ++e) {
            // every position of the classes this wave holds (their decayed order is not the original one)
            int larger = 0;
            for (uint32_t i = lo[e]; i < hi[e]; ++i) {
                const unsigned long long k = dkey[i];
                larger += k > key[e] && cand_box_class(k, p.C, p.div_c).cls == cls[e] ? 1 : 0;      // (a key above a live one is live)
            }
            if (larger >= p.max_per_class) key[e] = 0ull;
        }
        __syncthreads();
    }
    if (tid == 0) L.w->chunk_count = 0;
    __syncthreads();                               // (also: every pair loop has read its boxes; the sort takes their slots)
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < NMS_NE; ++e) {
        const uint32_t q = (uint32_t)(tid + NMS_THREADS * e);
        if (q < m) dkey[q] = key[e];
        mine += key[e] != 0ull ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if (lane == 0 && mine) atomicAdd(&L.w->chunk_count, mine);
    __syncthreads();
    const uint32_t live = L.w->chunk_count;
    __syncthreads();

    // ---- the result: the first max_total decayed keys
    matrix_sort(L, live, m2, tid);
    const uint32_t kept = live < (uint32_t)p.max_total ? live : (uint32_t)p.max_total;
    for (uint32_t i = tid; i < kept; i += NMS_THREADS) {
        const unsigned long long k = dkey[i];
        const CandBoxClass bc = cand_box_class(k, p.C, p.div_c);
        L.keep(i, *(const float4*)(gb + (int64_t)bc.box * 4), bc.cls, k, bc.box);
    }
    if (tid == 0) L.w->kept = kept;
    __syncthreads();
    nms_write_outputs(p, L, n, tid);
}

struct MatrixKernel { template <int KIND, bool AGN, int METHOD> static constexpr auto kernel = matrix_nms_kernel<KIND, AGN, METHOD>; };

int matrix_nms_launch(const NmsK& k, const DecayK& s, hipStream_t stream) {
    const size_t lds = matrix_lds_bytes(k.max_total, k.C);
    Y4_REQUIRE(lds <= 160 * 1024 && k.max_total <= 1024 && s.top_k >= 1 && s.top_k <= SORT_CAP, Y4_EINVAL,
               "matrix nms: top_k %d, max_total %d and %d classes need %zu bytes of LDS", s.top_k, k.max_total, k.C, lds);
    if (int r = nms_rule_check("matrix nms", k.kind, k.beta, k.agnostic)) return r;
    Y4_REQUIRE(s.method >= MATRIX_GAUSSIAN && s.method <= MATRIX_LINEAR && s.sigma > 0.f && s.min_score >= 0.f, Y4_EINVAL,
               "matrix nms: mode (method %d, sigma %g, min_score %g)", s.method, (double)s.sigma, (double)s.min_score);
    return nms_dispatch<MatrixKernel>(std::make_index_sequence<6 * 2>(), s.method, lds, stream, k, s);
}

}  // namespace y4
