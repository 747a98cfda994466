// anchors.hip -- y4_anchor_step / y4_anchor_fitness / y4_anchor_evolve: the data-set anchor search (IoU k-means, then a mutate-and-
// select evolution) on the device.  See DESIGN.md "Dataset anchors" and yolo4hip/anchors.py, which drives these from the host.
//
// The pair measure is anchor_iou.h's centred IoU, the one loss_assign_kernel uses, so the anchor a box gets here is the anchor
// y4_loss_assign gives it.  Everything that is summed is an integer:
//   fitness  F = sum over boxes of llrint(iou64(best anchor) * 2^30)            int64
//   Lloyd    cnt_j, SW_j = sum llrint((double)w * 2^16), SH_j likewise          int64, over the boxes whose best anchor is j
// so the sums do not depend on the order of addition and 64-bit integer atomics are allowed: a thread adds into registers (F) or
// LDS (cnt, SW, SH), a wave reduces F by shuffles, a workgroup adds its waves in LDS, and ONE global atomic per accumulator per
// workgroup carries the result out.  The same call gives the same bits.  With n <= 2^22 and sides <= 16384 every sum stays below
// 2^52 and converts to double exactly.  No workgroup waits for another; phases are separate launches on one stream.
#include "anchor_iou.h"
#include "kernels.h"

#pragma clang fp contract(off)   // the rule is stated operation by operation (no fused multiply-add)

namespace y4 {

namespace {

constexpr int ANC_THREADS = 256;
constexpr int ANC_MAX_K = 16;        // anchors of a set
constexpr int ANC_MAX_P = 256;       // candidate sets of a generation = threads of the select workgroup
constexpr int ANC_BOXES = 4;         // boxes a fitness thread keeps in registers
constexpr int ANC_SETS = 16;         // candidate sets one fitness workgroup holds in LDS
constexpr int ANC_MAX_BLOCKS = 1024; // workgroups along the boxes (256 CUs x 4); more boxes are walked grid-stride

typedef unsigned long long u64;      // the atomics' type; two's complement makes the unsigned add the int64 add

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__device__ __forceinline__ long long iou_q30(double iou) { return llrint(iou * 1073741824.0); }     // the scaling is exact
__device__ __forceinline__ long long side_q16(float s) { return llrint((double)s * 65536.0); }

// stats = [F, cnt[k], SW[k], SH[k]], zero on entry
__global__ __launch_bounds__(ANC_THREADS) void anchor_step_kernel(const float2* __restrict__ wh, int n,
                                                                   const float* __restrict__ anchors, int k,
                                                                   u64* __restrict__ stats, uint8_t* __restrict__ assign) {
    __shared__ float s_anc[2 * ANC_MAX_K];
    __shared__ u64 s_acc[1 + 3 * ANC_MAX_K];
    const int tid = threadIdx.x;
    if (tid < 2 * k) s_anc[tid] = anchors[tid];
    if (tid < 1 + 3 * k) s_acc[tid] = 0;
    __syncthreads();
    long long f = 0;
    for (int i = blockIdx.x * ANC_THREADS + tid; i < n; i += gridDim.x * ANC_THREADS) {
        const float2 b = wh[i];
        double iou;
        const int a = best_anchor(b.x, b.y, s_anc, k, &iou);
        f += iou_q30(iou);
        atomicAdd(&s_acc[1 + a], (u64)1);
        atomicAdd(&s_acc[1 + k + a], (u64)side_q16(b.x));
        atomicAdd(&s_acc[1 + 2 * k + a], (u64)side_q16(b.y));
        if (assign) assign[i] = (uint8_t)a;
    }
    f = wave_sum(f);
    if ((tid & 63) == 0) atomicAdd(&s_acc[0], (u64)f);
    __syncthreads();
    if (tid < 1 + 3 * k && s_acc[tid] != 0) atomicAdd(&stats[tid], s_acc[tid]);
}

// thread j: the mean of cluster j in 16.16 fixed point, or the anchor itself when the cluster is empty
__global__ __launch_bounds__(64) void anchor_next_kernel(const float* __restrict__ anchors, int k,
                                                         const long long* __restrict__ stats, float* __restrict__ next) {
    const int j = threadIdx.x;
    if (j >= k) return;
    const long long cnt = stats[1 + j];
    float w = anchors[2 * j], h = anchors[2 * j + 1];
    if (cnt != 0) {
        w = (float)((double)stats[1 + k + j] / (double)cnt / 65536.0);
        h = (float)((double)stats[1 + 2 * k + j] / (double)cnt / 65536.0);
    }
    next[2 * j] = w;
    next[2 * j + 1] = h;
}

// grid (box tiles, groups of ANC_SETS sets).  mult == null: set p is sets[p]; else `sets` is ONE set (best) and candidate p is
// fmaxf(best * mult[p], 1.0f) elementwise in float32.  f[P] zero on entry.
__global__ __launch_bounds__(ANC_THREADS) void anchor_fitness_kernel(const float2* __restrict__ wh, int n,
                                                                      const float* __restrict__ sets,
                                                                      const float* __restrict__ mult, int P, int k,
                                                                      u64* __restrict__ f) {
    __shared__ float s_set[ANC_SETS * 2 * ANC_MAX_K];
    __shared__ u64 s_f[ANC_SETS];
    const int tid = threadIdx.x;
    const int p0 = blockIdx.y * ANC_SETS;
    const int np = min(ANC_SETS, P - p0);
    const int row = 2 * k;
    for (int e = tid; e < np * row; e += ANC_THREADS) {
        const int src = p0 * row + e;
        s_set[e] = mult ? fmaxf(sets[e % row] * mult[src], 1.0f) : sets[src];
    }
    if (tid < ANC_SETS) s_f[tid] = 0;
    __syncthreads();

    constexpr int TILE = ANC_THREADS * ANC_BOXES;
    for (int base = blockIdx.x * TILE; base < n; base += gridDim.x * TILE) {
        float bw[ANC_BOXES], bh[ANC_BOXES];
        bool ok[ANC_BOXES];
#pragma unroll
        for (int b = 0; b < ANC_BOXES; ++b) {
            const int i = base + b * ANC_THREADS + tid;
            ok[b] = i < n;
            const float2 v = ok[b] ? wh[i] : make_float2(1.0f, 1.0f);
            bw[b] = v.x; bh[b] = v.y;
        }
        for (int p = 0; p < np; ++p) {
            const float* set = s_set + p * row;
            double best[ANC_BOXES];
            for (int a = 0; a < k; ++a) {                                  // anchors outside, boxes inside: four divisions in flight
                const float aw = set[2 * a], ah = set[2 * a + 1];
#pragma unroll
                for (int b = 0; b < ANC_BOXES; ++b) {
                    const double iou = anchor_iou64(bw[b], bh[b], aw, ah);
                    if (a == 0 || iou > best[b]) best[b] = iou;
                }
            }
            long long q = 0;
#pragma unroll
            for (int b = 0; b < ANC_BOXES; ++b) q += ok[b] ? iou_q30(best[b]) : 0;
            q = wave_sum(q);
            if ((tid & 63) == 0) atomicAdd(&s_f[p], (u64)q);
        }
    }
    __syncthreads();
    if (tid < np && s_f[tid] != 0) atomicAdd(&f[p0 + tid], s_f[tid]);
}

// One workgroup: the first arg-max of f[0 .. P); it replaces best / fbest only if strictly larger than fbest.
__global__ __launch_bounds__(ANC_MAX_P) void anchor_select_kernel(float* __restrict__ best, long long* __restrict__ fbest,
                                                                  const float* __restrict__ mult, int P, int k,
                                                                  const long long* __restrict__ f, int32_t* __restrict__ accepted) {
    __shared__ long long s_v[ANC_MAX_P / 64];
    __shared__ int s_i[ANC_MAX_P / 64];
    __shared__ int s_win;
    const int tid = threadIdx.x;
    long long v = tid < P ? f[tid] : -1;                                   // a fitness is never negative
    int idx = tid;
    for (int o = 32; o > 0; o >>= 1) {
        const long long ov = __shfl_down(v, o);
        const int oi = __shfl_down(idx, o);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if ((tid & 63) == 0) { s_v[tid >> 6] = v; s_i[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < ANC_MAX_P / 64; ++w)
            if (s_v[w] > v) { v = s_v[w]; idx = s_i[w]; }                  // waves in index order: strict `>` keeps the first
        const int win = v > *fbest ? idx : -1;
        if (win >= 0) *fbest = v;
        *accepted = win;
        s_win = win;
    }
    __syncthreads();
    const int win = s_win;
    if (win >= 0 && tid < 2 * k) best[tid] = fmaxf(best[tid] * mult[win * 2 * k + tid], 1.0f);
}

int anchor_check(const char* who, const void* wh, int n, int k) {
    Y4_REQUIRE(n >= 1 && n <= (1 << 22), Y4_EINVAL, "%s: n %d outside [1, 2^22]", who, n);
    Y4_REQUIRE(k >= 1 && k <= ANC_MAX_K, Y4_EINVAL, "%s: k %d outside [1, %d]", who, k, ANC_MAX_K);
    Y4_REQUIRE(wh && ((uintptr_t)wh & 7) == 0, Y4_EINVAL, "%s: wh_dev must be non-null and 8-byte aligned", who);
    return Y4_OK;
}

dim3 fitness_grid(int n, int P) {
    const int tile = ANC_THREADS * ANC_BOXES;
    return dim3(min((n + tile - 1) / tile, ANC_MAX_BLOCKS), (P + ANC_SETS - 1) / ANC_SETS);
}

}  // namespace

int anchor_step_launch(const float* wh, int n, const float* anchors, int k, float* next, int64_t* stats, uint8_t* assign,
                       hipStream_t stream) {
    if (int rc = anchor_check("anchor_step", wh, n, k)) return rc;
    Y4_REQUIRE(anchors && next && stats && ((uintptr_t)stats & 7) == 0, Y4_EINVAL,
               "anchor_step: anchors_dev, next_dev and stats_dev (8-byte aligned) must be non-null");
    Y4_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int64_t) * (1 + 3 * k), stream));
    const int blocks = min((n + ANC_THREADS - 1) / ANC_THREADS, ANC_MAX_BLOCKS);
    hipLaunchKernelGGL(anchor_step_kernel, dim3(blocks), dim3(ANC_THREADS), 0, stream, (const float2*)wh, n, anchors, k, (u64*)stats,
                       assign);
    hipLaunchKernelGGL(anchor_next_kernel, dim3(1), dim3(64), 0, stream, anchors, k, (const long long*)stats, next);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int anchor_fitness_launch(const float* wh, int n, const float* sets, int P, int k, int64_t* f, hipStream_t stream) {
    if (int rc = anchor_check("anchor_fitness", wh, n, k)) return rc;
    Y4_REQUIRE(P >= 1 && P <= ANC_MAX_P, Y4_EINVAL, "anchor_fitness: P %d outside [1, %d]", P, ANC_MAX_P);
    Y4_REQUIRE(sets && f && ((uintptr_t)f & 7) == 0, Y4_EINVAL, "anchor_fitness: sets_dev and f_dev (8-byte aligned) must be non-null");
    Y4_CHECK_HIP(hipMemsetAsync(f, 0, sizeof(int64_t) * P, stream));
    hipLaunchKernelGGL(anchor_fitness_kernel, fitness_grid(n, P), dim3(ANC_THREADS), 0, stream, (const float2*)wh, n, sets,
                       (const float*)nullptr, P, k, (u64*)f);
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int anchor_evolve_launch(const float* wh, int n, float* best, int64_t* fbest, const float* mult, int G, int P, int k,
                         int64_t* fhist, int32_t* accepted, hipStream_t stream) {
    if (int rc = anchor_check("anchor_evolve", wh, n, k)) return rc;
    Y4_REQUIRE(P >= 1 && P <= ANC_MAX_P, Y4_EINVAL, "anchor_evolve: P %d outside [1, %d]", P, ANC_MAX_P);
    Y4_REQUIRE(G >= 1 && G <= 4096, Y4_EINVAL, "anchor_evolve: G %d outside [1, 4096]", G);
    Y4_REQUIRE(best && fbest && mult && fhist && accepted && ((uintptr_t)fbest & 7) == 0 && ((uintptr_t)fhist & 7) == 0, Y4_EINVAL,
               "anchor_evolve: best_dev, fbest_dev, mult_dev, fhist_dev (8-byte aligned) and accepted_dev must be non-null");
    Y4_CHECK_HIP(hipMemsetAsync(fhist, 0, sizeof(int64_t) * (size_t)G * P, stream));
    const dim3 grid = fitness_grid(n, P);
    for (int g = 0; g < G; ++g) {                                          // no host synchronise: 2 G launches on one stream
        const float* m = mult + (size_t)g * P * 2 * k;
        int64_t* f = fhist + (size_t)g * P;
        hipLaunchKernelGGL(anchor_fitness_kernel, grid, dim3(ANC_THREADS), 0, stream, (const float2*)wh, n, (const float*)best, m, P,
                           k, (u64*)f);
        hipLaunchKernelGGL(anchor_select_kernel, dim3(1), dim3(ANC_MAX_P), 0, stream, best, (long long*)fbest, m, P, k,
                           (const long long*)f, accepted + g);
    }
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

}  // namespace y4
