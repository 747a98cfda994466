// nms_phases.h -- the phases that nms_kernel (decode_nms.hip), soft_nms_kernel (soft_nms.hip) and matrix_nms_kernel (matrix_nms.hip)
// share, the single copy: the LDS carve-up of a workgroup that owns one candidate list, the list prologue (count, overflow bit, counter
// reset), the selectors that extract the best keys of the list (count, histogram pivot, exact radix select, gather), the sorts, the box
// gather and the output stage; and the table their three launchers dispatch through.  Include it after candidates.h and kernels.h.
#pragma once
#include <utility>

#include "candidates.h"
#include "kernels.h"
#include "nms_measure.h"

#pragma clang fp contract(off)   // keep the reference's float32 op order (no fused multiply-add)

namespace y4 {

constexpr int NMS_THREADS = 1024;
constexpr int SORT_CAP = 4096;
constexpr int NMS_NE = SORT_CAP / NMS_THREADS;      // keys per thread of a full chunk: the participants / positions a decay kernel holds in registers
constexpr int PAR_MAX_C = 1024;      // class count up to which the round-parallel greedy pass has its per-class LDS words
constexpr uint32_t PAR_NONE = 0xffffffffu;

// iou_tf and nms_measure, the pair measure of y4_set_nms_rule: nms_measure.h (box_merge.hip decides membership with the same copy)

// Bitonic sort of skey[0 .. m2) (m2 a power of two >= 64, <= NE * NMS_THREADS), descending, with the keys in registers
// (element tid + NMS_THREADS * e): partners less than 64 apart are exchanged by wave shuffles and partners NMS_THREADS or
// more apart sit in the same thread, so only the stages with 64 <= j < NMS_THREADS go through LDS (`xbuf`, m2 keys) and a
// workgroup barrier -- 14 of the 78 stages at 4096 keys.  (Chunks of at most 1024 keys take nms_rank_sort.)
template <int NE>
__device__ __forceinline__ void nms_sort_regs(unsigned long long* skey, unsigned long long* xbuf, uint32_t m2, int tid) {
    unsigned long long v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) v[e] = (uint32_t)(tid + NMS_THREADS * e) < m2 ? skey[tid + NMS_THREADS * e] : 0ull;
    for (uint32_t k = 2; k <= m2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (NE > 1 && j >= (uint32_t)NMS_THREADS) {          // partner = another register of this thread
                const int de = (int)(j / NMS_THREADS);
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int pe = e ^ de;
                    if (pe > e && pe < NE) {
                        const uint32_t i = (uint32_t)(tid + NMS_THREADS * e);
                        const bool desc = (i & k) == 0;
                        const unsigned long long a = v[e], b = v[pe];
                        if (desc ? a < b : a > b) { v[e] = b; v[pe] = a; }
                    }
                }
            } else if (j >= 64) {                                // partner in another wave: through LDS
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    if ((uint32_t)(tid + NMS_THREADS * e) < m2) xbuf[tid + NMS_THREADS * e] = v[e];
                __syncthreads();
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const uint32_t i = (uint32_t)(tid + NMS_THREADS * e);
                    if (i < m2) {
                        const unsigned long long b = xbuf[i ^ j];
                        const bool want_max = ((i & j) == 0) == ((i & k) == 0);
                        v[e] = want_max ? (v[e] > b ? v[e] : b) : (v[e] < b ? v[e] : b);
                    }
                }
                __syncthreads();
            } else {                                             // partner in this wave: shuffle
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    if (NE > 1 && (uint32_t)(NMS_THREADS * e) >= m2) continue;      // (uniform) nothing lives in this register
                    const uint32_t i = (uint32_t)(tid + NMS_THREADS * e);
                    const unsigned long long b = __shfl_xor(v[e], (int)j);
                    const bool want_max = ((i & j) == 0) == ((i & k) == 0);
                    v[e] = want_max ? (v[e] > b ? v[e] : b) : (v[e] < b ? v[e] : b);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if ((uint32_t)(tid + NMS_THREADS * e) < m2) skey[tid + NMS_THREADS * e] = v[e];
    __syncthreads();
}

// ---- nms_kernel's dynamic LDS.  nms_lds_layout states it ONCE: the kernel carves by it (NmsLds) and the host asks it for the size.
struct NmsLdsLayout { uint32_t skey, sbox, kbox, kcls, kscore, kidx, hist, words, pfirst, pcount, pflag, bytes; };
__host__ __device__ inline NmsLdsLayout nms_lds_layout(int max_total, int C) {
    const uint32_t T = (uint32_t)max_total, par_c = C <= PAR_MAX_C ? (uint32_t)C : 0u;
    NmsLdsLayout o;
    uint32_t at = 0;
    o.skey = at;   at += SORT_CAP * 8;               // [SORT_CAP] the chunk's keys
    o.sbox = at;   at += SORT_CAP * 16;              // [SORT_CAP] the chunk's boxes; scratch of the selectors and sorts before that
    o.kbox = at;   at += T * 16;                     // [max_total] the kept list: box, class, score, box index
    o.kcls = at;   at += T * 4;
    o.kscore = at; at += T * 4;
    o.kidx = at;   at += T * 4;
    o.hist = at;   at += 256 * 4;                    // [256] digit histogram of the exact select
    o.words = at;  at += 64;                         // NmsWords
    o.pfirst = at; at += 2 * par_c * 4;              // [2][C] lowest undecided position of a class
    o.pcount = at; at += par_c * 4;                  // [C] kept boxes of a class
    o.pflag = at;  at += (NMS_THREADS + 16) * 4;     // [NMS_THREADS] candidate was kept; then [16] per-wave kept counts
    o.bytes = at;
    return o;
}

// The words through which the phases of nms_kernel talk to each other
struct NmsWords {
    uint32_t chunk_count;      // keys taken into the chunk (nms_take_chunk)
    uint32_t kept;             // kept boxes so far
    uint32_t remaining;        // keys below the cutoff (nms_count_below)
    uint32_t pivot_bin1;       // nms_histogram_pivot: 1 + the pivot bin; stays 0 when not even the top bin fits
    uint32_t suffix;           // ... the keys in the bins from the pivot bin up
    uint32_t digit;            // nms_select_pivot: the digit chosen in this pass
    uint32_t need;             // ... keys still needed inside that digit
    uint32_t unused0;
    uint32_t undecided[2];     // nms_pass_parallel: lowest undecided position (two alternating buffers)
    uint32_t kept_front[2];    // ... kept candidates in front of it
    uint32_t unused1[4];
};
static_assert(sizeof(NmsWords) == 64, "nms_lds_layout reserves 64 bytes");

struct NmsLds {
    unsigned long long* skey;
    float4* sbox;
    float4* kbox;
    int* kcls;
    float* kscore;
    int* kidx;
    uint32_t* hist;
    NmsWords* w;
    uint32_t *pfirst, *pcount, *pflag;
    __device__ __forceinline__ NmsLds(char* base, int max_total, int C) {
        const NmsLdsLayout o = nms_lds_layout(max_total, C);
        skey = (unsigned long long*)(base + o.skey);
        sbox = (float4*)(base + o.sbox);
        kbox = (float4*)(base + o.kbox);
        kcls = (int*)(base + o.kcls);
        kscore = (float*)(base + o.kscore);
        kidx = (int*)(base + o.kidx);
        hist = (uint32_t*)(base + o.hist);
        w = (NmsWords*)(base + o.words);
        pfirst = (uint32_t*)(base + o.pfirst);
        pcount = (uint32_t*)(base + o.pcount);
        pflag = (uint32_t*)(base + o.pflag);
    }
    // The box slots hold boxes from nms_load_boxes on.  Before that, within one chunk, they are:
    __device__ __forceinline__ uint32_t* score_bins() const { return (uint32_t*)sbox; }               // [1024] nms_histogram_pivot's bins
    __device__ __forceinline__ uint32_t* wave_suffix() const { return (uint32_t*)sbox + 1024; }       // [16] ... and its per-wave sums
    __device__ __forceinline__ unsigned long long* xbuf() const { return (unsigned long long*)sbox; } // [SORT_CAP] the sorts' exchange buffer
    __device__ __forceinline__ uint32_t* wave_kept() const { return pflag + NMS_THREADS; }            // [16] behind the flags
    // one entry of the kept list
    __device__ __forceinline__ void keep(uint32_t slot, const float4 box, int cls, unsigned long long key, uint32_t box_index) const {
        kbox[slot] = box;
        kcls[slot] = cls;
        kscore[slot] = cand_score(key);
        kidx[slot] = (int)box_index;
    }
};

// ---- the list of workgroup n: its length, clamped to the capacity (an overflow raises the status bit), its keys and its box table.
// Zeroes the kept count and, once every thread has read the list's counter, the counter: it is left at zero for the next step's decode
// (which therefore needs no memset launch in front of it; decode_launch clears only when a decode was NOT followed by its NMS), and
// counts_clean, the gather path and the merged forms depend on every kernel over a list doing so.
struct NmsList { uint32_t cnt; const unsigned long long* gk; const float* gb; };
__device__ __forceinline__ NmsList nms_list_begin(const NmsK& p, const NmsLds& L, int n, int tid) {
    uint32_t cnt = p.counts[(size_t)n * COUNT_STRIDE];
    if (cnt > p.cap) {
        if (tid == 0) atomicOr(p.status, 1u);
        cnt = p.cap;
    }
    const unsigned long long* gk = p.keys + (int64_t)n * p.cap;
    const float* gb = p.dboxes + (int64_t)n * p.nbox * 4;
    if (tid == 0) L.w->kept = 0;
    __syncthreads();
    if (tid == 0) p.counts[(size_t)n * COUNT_STRIDE] = 0;
    return NmsList{cnt, gk, gb};
}

// ---- how many keys remain below the cutoff?
__device__ __forceinline__ uint32_t nms_count_below(const NmsLds& L, const unsigned long long* gk, uint32_t cnt, unsigned long long cutoff, int tid) {
    if (tid == 0) L.w->remaining = 0;
    __syncthreads();
    {
        uint32_t local = 0;
        for (uint32_t i = tid; i < cnt; i += NMS_THREADS) local += gk[i] < cutoff ? 1u : 0u;
        for (int o = 32; o > 0; o >>= 1) local += __shfl_down(local, o);
        if ((tid & 63) == 0 && local) atomicAdd(&L.w->remaining, local);
    }
    __syncthreads();
    return L.w->remaining;
}

// The FIRST chunk's pivot.  The first chunk need not hold EXACTLY chunk_cap keys: one histogram pass over 1024 score bins (score
// bits >> 14 from 0.25 up: any monotonic map of the key would do) and a suffix sum say from which bin up at most chunk_cap keys lie;
// that bin's lowest key is the pivot.  ~2 us where the exact radix select (nms_select_pivot) takes eight passes, each with a
// serial scan of its 256 bins.  (A top bin that alone overflows the chunk -- a thousand equal scores -- falls through
// to the exact select.)  -> true and *pivot when the histogram gave one.
__device__ __forceinline__ bool nms_histogram_pivot(const NmsLds& L, const unsigned long long* gk, uint32_t cnt, uint32_t chunk_cap, int tid,
                                                    unsigned long long* pivot) {
    constexpr uint32_t BASE = 0x3e800000u >> 14;
    uint32_t* const hb = L.score_bins();                        // (the box slots are not in use yet)
    uint32_t* const wsum = L.wave_suffix();
    const int lane = tid & 63, wv = tid >> 6;
    hb[tid] = 0;
    if (tid == 0) L.w->pivot_bin1 = 0;
    __syncthreads();
    for (uint32_t i = tid; i < cnt; i += NMS_THREADS) {
        const int x = (int)((uint32_t)(gk[i] >> 46)) - (int)BASE;
        atomicAdd(&hb[x < 0 ? 0 : (x > 1023 ? 1023 : x)], 1u);
    }
    __syncthreads();
    uint32_t suf = hb[tid];                                 // keys in bins tid .. 1023: the wave's suffix sum, then the later waves'
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_down(suf, o);
        suf += lane + o < 64 ? v : 0u;
    }
    if (lane == 0) wsum[wv] = suf;
    __syncthreads();
    for (int w = wv + 1; w < NMS_THREADS / 64; ++w) suf += wsum[w];
    // the lowest bin whose suffix fits the chunk (bin 0's suffix is `remaining`: it never does)
    if (tid > 0 && suf <= chunk_cap && suf + hb[tid - 1] > chunk_cap) { L.w->pivot_bin1 = (uint32_t)tid + 1u; L.w->suffix = suf; }
    __syncthreads();
    // (one 2^-9-wide score bin holding more than a chunk while the bins above it are nearly empty would give a first
    //  chunk of a few keys and leave the image to the slow later passes: a suffix under half a chunk falls through to the exact
    //  radix select, which fills the chunk)
    const uint32_t pb = L.w->pivot_bin1 != 0 && 2u * L.w->suffix >= chunk_cap ? L.w->pivot_bin1 : 0u;
    if (pb != 0) *pivot = (unsigned long long)((pb - 1u + BASE) << 14) << 32;       // the bin's lowest key
    __syncthreads();
    return pb != 0;
}

// Exact radix select: -> the chunk_cap-th largest key below the cutoff, eight passes of one digit each.
__device__ __forceinline__ unsigned long long nms_select_pivot(const NmsLds& L, const unsigned long long* gk, uint32_t cnt, unsigned long long cutoff,
                                                               uint32_t chunk_cap, int tid) {
    unsigned long long prefix = 0, pmask = 0;
    uint32_t need = chunk_cap;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += NMS_THREADS) L.hist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < cnt; i += NMS_THREADS) {
            const unsigned long long k = gk[i];
            if (k < cutoff && (k & pmask) == prefix) atomicAdd(&L.hist[(k >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            int d = 255;
            for (; d > 0; --d) {
                if (acc + L.hist[d] >= need) break;
                acc += L.hist[d];
            }
            L.w->need = need - acc;                  // still needed inside digit d
            L.w->digit = (uint32_t)d;
        }
        __syncthreads();
        need = L.w->need;
        prefix |= (unsigned long long)L.w->digit << shift;
        pmask |= 255ull << shift;
        __syncthreads();
    }
    return prefix;                                    // keys are unique: exactly chunk_cap keys in [pivot, cutoff)
}

// ---- gather the chunk: the keys in [pivot, cutoff) -> skey[0 .. m), zero padded to m2, the next power of two (>= 64).  -> m
__device__ __forceinline__ uint32_t nms_take_chunk(const NmsLds& L, const unsigned long long* gk, uint32_t cnt, unsigned long long cutoff,
                                                   unsigned long long pivot, uint32_t chunk_cap, int tid, uint32_t* m2_out) {
    if (tid == 0) L.w->chunk_count = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < cnt; i0 += NMS_THREADS) {      // one LDS atomic per wave and pass, not per key (wave_append)
        const uint32_t i = i0 + tid;
        const unsigned long long k = i < cnt ? gk[i] : 0ull;
        const bool take = i < cnt && k < cutoff && k >= pivot;
        const uint32_t pos = wave_append(&L.w->chunk_count, take, tid & 63);
        if (take && pos < chunk_cap) L.skey[pos] = k;
    }
    __syncthreads();
    const uint32_t m = L.w->chunk_count < chunk_cap ? L.w->chunk_count : chunk_cap;
    uint32_t m2 = 64;
    while (m2 < m) m2 <<= 1;
    for (uint32_t i = m + tid; i < m2; i += NMS_THREADS) L.skey[i] = 0;
    __syncthreads();
    *m2_out = m2;
    return m;
}

// ---- the participants of a decay kernel: EXACTLY the top_k largest keys of the list (all when it is shorter) -> skey[0 .. m),
// unsorted -- the exact radix select, never the histogram pivot.  -> m
__device__ __forceinline__ uint32_t nms_take_top_k(const NmsLds& L, const unsigned long long* gk, uint32_t cnt, uint32_t top_k, int tid,
                                                   uint32_t* m2_out) {
    unsigned long long pivot = 0;
    if (cnt > top_k) pivot = nms_select_pivot(L, gk, cnt, ~0ull, top_k, tid);
    return nms_take_chunk(L, gk, cnt, ~0ull, pivot, top_k, tid, m2_out);
}

// Rank sort of skey[0 .. m2), m2 <= NMS_THREADS, descending: a thread's key goes to position (number of larger keys); keys are
// unique.  No dependent chain, two barriers.  In-kernel timestamps at ~1000 keys: 22 us, the same as the 55 dependent exchange
// stages of a bitonic network in LDS or in registers with shuffles, and as broadcasting the keys with v_readlane instead of LDS
// reads (16 waves on one CU: LDS cycles of the broadcast reads here, instruction issue there) -- kept because it is the
// shortest; the whole kernel went 80 -> 76.5 us with it and the wave-aggregated gather of nms_take_chunk.
// Round 4: the ranks come from a merge instead of all pairs -- every wave sorts its 64 keys in registers (21 shuffle
// stages), the sorted runs go back to LDS, and a key's rank is its place in its own run plus, per other run, the number
// of larger keys found by a 6-step binary search (the searches of the runs are independent chains): ~600 instructions
// per thread instead of ~3 500.
__device__ __forceinline__ void nms_rank_sort(const NmsLds& L, uint32_t m, uint32_t m2, int tid) {
    unsigned long long* const skey = L.skey;
    unsigned long long* const xbuf = L.xbuf();
    unsigned long long key = (uint32_t)tid < m2 ? skey[tid] : 0ull;
    const int lane = tid & 63, wv = tid >> 6;
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned long long o = __shfl_xor(key, j);
            const bool want_max = ((lane & j) == 0) == ((lane & k) == 0);      // descending run
            key = (want_max ? o > key : o < key) ? o : key;
        }
    __syncthreads();
    if ((uint32_t)tid < m2) skey[tid] = key;
    __syncthreads();
    uint32_t rank = (uint32_t)lane;
    const int nruns = (int)(m2 >> 6);
    for (int r = 0; r < nruns; ++r) {
        if (r == wv) continue;                               // (wave-uniform)
        const unsigned long long* run = skey + r * 64;
        uint32_t lo = 0;                                     // number of keys of the run known to be larger
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) lo += run[lo + st - 1] > key ? (uint32_t)st : 0u;
        lo += run[lo] > key ? 1u : 0u;                       // (lo <= 63 here)
        rank += lo;
    }
    __syncthreads();
    if ((uint32_t)tid < m2 && key != 0ull) xbuf[rank] = key;  // (keys are unique and non-zero; the zero padding stays behind position m)
    __syncthreads();
    if ((uint32_t)tid < m) skey[tid] = xbuf[tid];
    __syncthreads();
}

// ---- gather the chunk's boxes into LDS
__device__ __forceinline__ void nms_load_boxes(const NmsLds& L, const float* gb, const NmsK& p, uint32_t m, int tid) {
    for (uint32_t i = tid; i < m; i += NMS_THREADS)
        L.sbox[i] = *(const float4*)(gb + (int64_t)cand_box_class(L.skey[i], p.C, p.div_c).box * 4);
    __syncthreads();
}

// ---- outputs: clipped boxes, zero padded (clip_boxes=True, pad to max_total); with a box map (y4_decode_nms_mapped) each
// kept box is first mapped from the canvas to its source image, x -> fmaf(x, ax, bx), y -> fmaf(y, ay, by), so the clip is to
// the image.  Only the written boxes change: which boxes are kept was decided before, on the canvas boxes.
__device__ __forceinline__ void nms_write_outputs(const NmsK& p, const NmsLds& L, int n, int tid) {
    const int kept = (int)L.w->kept;
    float ax = 1.f, bx = 0.f, ay = 1.f, by = 0.f;
    if (p.box_map) { ax = p.box_map[4 * n]; bx = p.box_map[4 * n + 1]; ay = p.box_map[4 * n + 2]; by = p.box_map[4 * n + 3]; }
    for (int i = tid; i < p.max_total; i += NMS_THREADS) {
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        float s = 0.f, c = 0.f;
        int id = -1;
        if (i < kept) {
            b = L.kbox[i];
            if (p.box_map) {
                b.x = fmaf(b.x, ax, bx); b.y = fmaf(b.y, ay, by);
                b.z = fmaf(b.z, ax, bx); b.w = fmaf(b.w, ay, by);
            }
            b.x = fmaxf(fminf(b.x, 1.f), 0.f); b.y = fmaxf(fminf(b.y, 1.f), 0.f);
            b.z = fmaxf(fminf(b.z, 1.f), 0.f); b.w = fmaxf(fminf(b.w, 1.f), 0.f);
            s = L.kscore[i]; c = (float)L.kcls[i]; id = L.kidx[i];
        }
        *(float4*)(p.out_boxes + ((int64_t)n * p.max_total + i) * 4) = b;
        p.out_scores[(int64_t)n * p.max_total + i] = s;
        p.out_classes[(int64_t)n * p.max_total + i] = c;
        if (p.out_idx) p.out_idx[(int64_t)n * p.max_total + i] = id;
    }
    if (tid == 0) p.out_valid[n] = kept;
}

// ---- host side: the launchers' dispatch.  F names a kernel template: F::kernel<KIND, AGN, METHOD> is its instantiation for a
// measure (nms_measure.h), the agnostic flag and a method 1 .. NMETHODS; I counts the 6 * NMETHODS of them.  Launches the one of the
// rule in `k` and of `method`, one workgroup per list, through launch_lds -- one table per kernel template,
// [measure][agnostic][method - 1].  more: what the kernel takes behind NmsK
template <class F, class... Args, size_t... I>
int nms_dispatch(std::index_sequence<I...>, int method, size_t lds, hipStream_t stream, const NmsK& k, const Args&... more) {
    constexpr size_t NM = sizeof...(I) / 6;
    using Launch = int (*)(int, dim3, dim3, size_t, hipStream_t, const NmsK&, const Args&...);
    static const Launch table[] = {launch_lds<F::template kernel<(int)(I / (2 * NM)), (I / NM) % 2 != 0, (int)(I % NM) + 1>, NmsK, Args...>...};
    const size_t at = ((size_t)nms_measure_index(k.kind, k.beta) * 2 + (size_t)k.agnostic) * NM + (size_t)(method - 1);
    return table[at](160 * 1024, dim3(k.N), dim3(NMS_THREADS), lds, stream, k, more...);
}

}  // namespace y4
