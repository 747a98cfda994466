// decode_nms.hip -- the tail of the reference's inference_model (models.py:68-73):
//   yolov4_head/get_boxes (custom_layers.py:201-258)  -> decode_kernel
//   nms() = tf.image.combined_non_max_suppression (custom_layers.py:261-298) -> nms_kernel
//
// decode_kernel: one lane per box reads its objectness logit; boxes whose sigmoid(obj) alone is not above the
// score threshold cannot yield candidates and are dropped at once; the wave then sweeps the class logits of
// the surviving boxes (coalesced), forms score = sigmoid(obj)*sigmoid(cls) and appends the ones with
// score > score_threshold (strict) to the image's candidate list with ONE wave-aggregated atomic per pass
// (ballot + popcount).  Only surviving boxes are decoded to coordinates.  A candidate is a 64-bit key (candidates.h), which also
// defines the tie order.
// Rectangular inputs (H x W): scale s has gh = H / stride rows and gw = W / stride columns, cells row-major; box index =
// box_off[s] + (row * gw + col) * 3 + anchor.  x1 and x2 are divided by W, y1 and y2 by H (the reference divides all four by
// input_shape[0], custom_layers.py:284 -- for a square input the same float32 division, bit for bit).
//
// nms_kernel: one workgroup per image.  Class-aware greedy NMS is done in ONE pass over the globally
// sorted candidates (suppression only against kept boxes of the same class): this visits every class's
// candidates in that class's own descending order, so the per-class kept sets equal TensorFlow's
// per-class greedy runs, and the kept boxes come out already in the final descending-score order; the
// pass stops after max_total kept boxes (a class's 101st kept box can never be in the overall top 100, so
// max_per_class is enforced with a same-class count).  Candidates are taken in chunks in descending key order
// (radix-select of the chunk pivot when an image has more than a chunk holds): the first of at most NMS_THREADS keys
// -- merge-rank sorted, and decided ROUND-PARALLEL, one candidate per thread (round 4; see the greedy pass) --, the
// later ones, which only an image that has not filled max_total from its best 1024 candidates reaches, of at most
// SORT_CAP keys through the register bitonic network and wave 0's pass over 64 candidates at a time.
// IoU is TensorFlow's: corners min/max-normalised, 0 if either area <= 0, suppress iff IoU > threshold.
// That is the default pair rule; y4_set_nms_rule selects DIoU-NMS (nms_measure) and / or class-agnostic suppression (nms_kernel's AGN).
#include "candidates.h"
#include "kernels.h"
#include "nms_measure.h"
#include "nms_phases.h"

#pragma clang fp contract(off)   // keep the reference's float32 op order (no fused multiply-add)

namespace y4 {

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// score = sigmoid(obj) * sigmoid(class logit x) > score_thr (strict)?  -> *score when it is.  Cheap screen first (v_exp_f32 +
// v_rcp_f32, ~1e-6 relative): the exact float32 sigmoid (IEEE expf + division, what the decision is defined on) runs only for
// scores within 0.2 % of the cut.  (A NaN logit fails the screen: it is no candidate at any threshold.)
__device__ __forceinline__ bool decode_score(float s_obj, float x, float score_thr, float* score) {
    const float approx = s_obj * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
    if (!(approx > 0.998f * score_thr)) return false;
    *score = s_obj * sigmoid_f(x);
    return *score > score_thr;
}

// custom_layers.py:251-256: the four box logits t of anchor `a` in cell (row, col) of scale s -> normalised x1, y1, x2, y2
// (cells are row-major: row over H, column over W)
__device__ __forceinline__ float4 decode_box(const DecodeK& p, int s, int a, int row, int col, float t0, float t1, float t2, float t3) {
    const float bx = ((sigmoid_f(t0) * p.xyscale[s]) - p.xyoff[s] + (float)col) * (float)p.stride[s];
    const float by = ((sigmoid_f(t1) * p.xyscale[s]) - p.xyoff[s] + (float)row) * (float)p.stride[s];
    const float bw = expf(t2) * p.anchors[(s * 3 + a) * 2 + 0];
    const float bh = expf(t3) * p.anchors[(s * 3 + a) * 2 + 1];
    float4 o;
    o.x = (bx - bw / 2.0f) / p.img_w;
    o.y = (by - bh / 2.0f) / p.img_h;
    o.z = (bx + bw / 2.0f) / p.img_w;
    o.w = (by + bh / 2.0f) / p.img_h;
    return o;
}

// One lane per (cell, anchor) box.  Because score = sigmoid(obj)*sigmoid(cls) <= sigmoid(obj) in float32
// (sigmoid <= 1), a box whose objectness alone is not > score_threshold cannot produce a candidate: each lane
// reads just its objectness logit first (4 bytes) and the wave then sweeps, cooperatively and coalesced, the
// class logits of the few boxes that pass (ballot loop).  Only those boxes are decoded to coordinates.
__global__ __launch_bounds__(256) void decode_kernel(const DecodeK p) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;          // box id over all images
    const int n = (int)(t / p.nbox);
    const int b = (int)(t - (int64_t)n * p.nbox);                        // box index within the image
    const bool in_range = n < p.N;
    const int nf = 5 + p.C;
    int s = 0, a = 0, cell = 0;
    const float* cellp = nullptr;
    float s_obj = 0.f;
    if (in_range) {
        const int c3 = b / 3;
        a = b - c3 * 3;
        const int n0 = p.gh[0] * p.gw[0], n1 = n0 + p.gh[1] * p.gw[1];
        s = c3 >= n1 ? 2 : (c3 >= n0 ? 1 : 0);
        cell = c3 - (s == 2 ? n1 : (s == 1 ? n0 : 0));
        cellp = p.head[s] + ((int64_t)n * p.gh[s] * p.gw[s] + cell) * p.hcs + a * nf;
        s_obj = sigmoid_f(cellp[4]);
    }
    unsigned long long todo = __ballot(in_range && s_obj > p.score_thr);
    while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        // broadcast lane j's box
        const float* bp = (const float*)__shfl((unsigned long long)(uintptr_t)cellp, j);
        const float so = __shfl(s_obj, j);
        const int bn = __shfl(n, j), bb = __shfl(b, j);
        unsigned long long* keys = p.keys + (int64_t)bn * p.cap;
        for (int c0 = 0; c0 < p.C; c0 += 64) {
            const int c = c0 + lane;
            float sc = 0.f;
            const bool hit = c < p.C && decode_score(so, bp[5 + c], p.score_thr, &sc);
            const uint32_t pos = wave_append(p.counts + (size_t)bn * COUNT_STRIDE, hit, lane);
            if (hit && pos < p.cap) keys[pos] = cand_key(sc, cand_make_id((uint32_t)bb, (uint32_t)c, p.C));
        }
        if (lane == j) {
            // (only boxes that can be candidates are ever read back by the NMS stage)
            const int gw = p.gw[s];
            const int row = cell / gw, col = cell - row * gw;
            *(float4*)(p.dboxes + ((int64_t)n * p.nbox + b) * 4) = decode_box(p, s, a, row, col, cellp[0], cellp[1], cellp[2], cellp[3]);
        }
    }
}

// Variant for cells of at most 256 values (C <= 80): one wavefront per grid cell, the cell's 3*(5+C) logits are
// read fully coalesced straight into registers (<= 4 per lane, one memory round trip), the three objectness
// logits are broadcast by shuffles, and the 73 % of cells where no anchor can pass exit right there.
// (Round 2 also tried 4 cells per wave with all 16 full-cell loads issued up front: 0.123 ms against 0.114 for one cell per
// wave; the objectness pre-screen of decode_cell_kernel below is what removed traffic instead.)

struct DecodeCell { int n, s, rem; const float* src; };
__device__ __forceinline__ DecodeCell decode_locate(const DecodeK& p, int64_t cellid) {
    DecodeCell c;
    c.n = (int)fastdiv((uint32_t)cellid, p.div_cells);
    c.rem = (int)cellid - c.n * p.cells_per_img;
    c.s = 0;
    const int c0 = p.gh[0] * p.gw[0], c1 = p.gh[1] * p.gw[1];
    if (c.rem >= c0) { c.rem -= c0; c.s = 1; if (c.rem >= c1) { c.rem -= c1; c.s = 2; } }
    c.src = p.head[c.s] + ((int64_t)c.n * p.gh[c.s] * p.gw[c.s] + c.rem) * p.hcs;
    return c;
}

// A wave's candidates are staged in its own LDS slice and go out with ONE returning atomic per flush (image change, slice
// nearly full, end of the wave's cells) instead of one per cell: the atomic's round trip -- the wave can do nothing until it
// knows where to write -- was paid 4-5 times per wave, and an image's counter took four times the same-address atomics.
// The order of an image's candidate list is irrelevant (NMS sorts it; keys are unique).
constexpr int DC_STAGE = 512;               // keys per wave slice; a cell yields at most 3 * C <= 240
struct DecodeStage { unsigned long long* slice; uint32_t fill; int img; };
__device__ __forceinline__ void decode_flush(const DecodeK& p, DecodeStage& st, int lane) {
    if (st.fill) {
        const uint32_t base = wave_reserve(p.counts + (size_t)st.img * COUNT_STRIDE, st.fill, lane);
        unsigned long long* keys = p.keys + (int64_t)st.img * p.cap;
        for (uint32_t i = lane; i < st.fill; i += 64)
            if (base + i < p.cap) keys[base + i] = st.slice[i];
        st.fill = 0;
    }
}

__device__ __forceinline__ void decode_one_cell(const DecodeK& p, const DecodeCell& cl, const float (&v)[4], const float (&so)[3], int lane,
                                                DecodeStage& st) {
    const int n = cl.n, s = cl.s, rem = cl.rem;
    const int nf = 5 + p.C, nval = 3 * nf;
    // so[a] = sigmoid(objectness of anchor a): the screen's value for this cell (the same float32 logit through the same sigmoid_f)
    const int box0 = p.box_off[s] + rem * 3;
    if (n != st.img || st.fill + 3 * p.C > DC_STAGE) { decode_flush(p, st, lane); st.img = n; }     // wave-uniform
    unsigned long long key[4];
    unsigned long long mask[4];
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        bool hit = false;
        key[k] = 0;
        if (e < nval) {
            const int a = e >= 2 * nf ? 2 : (e >= nf ? 1 : 0);
            const int f = e - a * nf;
            const float sa = a == 0 ? so[0] : (a == 1 ? so[1] : so[2]);
            float sc;
            if (f >= 5 && sa > p.score_thr && decode_score(sa, v[k], p.score_thr, &sc)) {
                hit = true;
                key[k] = cand_key(sc, cand_make_id((uint32_t)(box0 + a), (uint32_t)(f - 5), p.C));
            }
        }
        mask[k] = __ballot(hit);
        total += (uint32_t)__popcll(mask[k]);
    }
    if (total) {                              // into the wave's slice; no atomic here
        uint32_t base = st.fill;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if ((mask[k] >> lane) & 1ull)
                st.slice[base + (uint32_t)__popcll(mask[k] & ((1ull << lane) - 1ull))] = key[k];
            base += (uint32_t)__popcll(mask[k]);
        }
        st.fill = base;
    }
}

// A wave first SCREENS 16 consecutive cells: lane (c, a) = (lane >> 2, lane & 3 < 3) reads the one objectness logit of
// (cell c, anchor a) -- 48 four-byte loads, three 64-byte sectors per cell instead of its 1 KB -- and the ballot of
// sigmoid(obj) > threshold (the same float32 decision decode_one_cell makes) says which cells can have candidates at all
// (27 % on the synthetic heads).  Only those are then read in full, one at a time.  HBM bytes per cell 1024 -> ~470.
// Round 4: DC_SCREEN is a template parameter -- a few images (the reference's own call is ONE) are 1 421 waves of 16 cells on 1 024
// SIMDs, each walking its ~4 flagged cells one after the other with nothing beside it to hide the loads; 4 cells per wave are four
// times the waves with a quarter of the chain (34 -> see LABNOTES.md section 4.4).  The candidate lists' order differs, NMS sorts them.
constexpr int DC_SCREEN = 16, DC_SCREEN_SMALL = 4;
template <int DC_SCREEN>
__global__ __launch_bounds__(256) void decode_cell_kernel(const DecodeK p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t cell0 = ((int64_t)blockIdx.x * 4 + wave) * DC_SCREEN, ncell = (int64_t)p.N * p.cells_per_img;
    if (cell0 >= ncell) return;
    const int nf = 5 + p.C, nval = 3 * nf;
    const int c = lane >> 2, a = lane & 3;
    bool pass = false;
    float sig = 0.f;                          // sigmoid(objectness) of this lane's (cell, anchor)
    if (a < 3 && c < DC_SCREEN && cell0 + c < ncell) {
        // round 4: from the head convs' dense objectness array when they wrote one (one coalesced 16 bytes per cell: the same
        // float32 logits), else from the cell itself
        if (p.obj) sig = sigmoid_f(p.obj[(cell0 + c) * 4 + a]);
        else {
            const DecodeCell cl = decode_locate(p, cell0 + c);
            sig = sigmoid_f(cl.src[a * nf + 4]);
        }
        pass = sig > p.score_thr;
    }
    // Round 4: the box of every (cell, anchor) that passed -- the condition under which decode_one_cell used to compute it on 3 of its
    // 64 lanes, once per flagged cell -- is computed HERE, one per lane, for all of the wave's cells at once (decode_box; the four
    // box logits come from the cell: its lines are read by the full-cell load anyway)
    if (pass) {
        const DecodeCell cl = decode_locate(p, cell0 + c);
        const int s = cl.s, gw = p.gw[s];
        const float* tp = cl.src + a * nf;
        const float t0 = tp[0], t1 = tp[1], t2 = tp[2], t3 = tp[3];
        const int row = (int)fastdiv((uint32_t)cl.rem, p.div_gw[s]), col = cl.rem - row * gw;
        *(float4*)(p.dboxes + ((int64_t)cl.n * p.nbox + p.box_off[s] + cl.rem * 3 + a) * 4) = decode_box(p, s, a, row, col, t0, t1, t2, t3);
    }
    unsigned long long m = __ballot(pass);
    if (!m) return;
    auto next_cell = [&](DecodeCell& cl, float (&v)[4], float (&so)[3]) {        // pops the lowest flagged cell and issues its loads
        const int cc = (__ffsll((long long)m) - 1) >> 2;
        m &= ~(0xFull << (4 * cc));
        cl = decode_locate(p, cell0 + cc);
#pragma unroll
        for (int k = 0; k < 3; ++k) so[k] = __shfl(sig, cc * 4 + k);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (lane + 64 * k < nval) ? cl.src[lane + 64 * k] : 0.f;
    };
    __shared__ unsigned long long stage[4][DC_STAGE];
    DecodeStage st{stage[wave], 0u, -1};
    DecodeCell cur, nxt;
    float vc[4], vn[4], sc[3], sn[3];
    next_cell(cur, vc, sc);
    while (true) {                                                // wave-uniform: the next flagged cell's loads fly under this one
        const bool more = m != 0;
        if (more) next_cell(nxt, vn, sn);
        decode_one_cell(p, cur, vc, sc, lane, st);
        if (!more) break;
        cur = nxt;
#pragma unroll
        for (int k = 0; k < 4; ++k) vc[k] = vn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) sc[k] = sn[k];
    }
    decode_flush(p, st, lane);
}

// ------------------------------------------------------------------------------------------- NMS
// the constants, the LDS layout, the list prologue, the selectors, the sorts, nms_load_boxes and nms_write_outputs: nms_phases.h
// (soft_nms.hip and matrix_nms.hip run the same copies)

// ---- greedy pass, ROUND-PARALLEL on every wave: the usual case (all of the image's candidates in one chunk of at most
// NMS_THREADS; round 4).  One candidate per thread; in a round the lowest undecided candidate of every class (an LDS atomicMin per
// class) is final -- every earlier kept box of its class was such a head in an earlier round and it survived the test
// against it then -- so it is kept (class cap permitting) and the class's other undecided candidates test against it.
// The rounds stop once the candidates in front of the lowest undecided one hold max_total kept boxes; the kept boxes'
// ranks in sorted order are their output slots.  Same decisions as the sequential rule (same tests on the same pairs),
// in as many rounds as the busiest class among the leading candidates has kept boxes (bench input: ~7) of two
// barriers each, where the wave-0 pass below visits candidates 64 at a time at ~10 us per batch.
// (The first chunk: m <= NMS_THREADS; the kept lists it leaves are what the wave-0 pass of a later chunk continues from.)
template <int KIND>
__device__ __forceinline__ void nms_pass_parallel(const NmsK& p, const NmsLds& L, uint32_t m, int tid) {
    NmsWords* const w = L.w;
    uint32_t* const pfirst = L.pfirst;
    uint32_t* const pcount = L.pcount;
    uint32_t* const pflag = L.pflag;
    const uint32_t t = (uint32_t)tid;
    const int lane = tid & 63;
    const bool cap_binds = p.max_per_class < p.max_total;
    bool und = t < m, keptf = false;
    const unsigned long long key = und ? L.skey[t] : 0ull;
    const float4 cb = und ? L.sbox[t] : make_float4(0.f, 0.f, 0.f, 0.f);
    const CandBoxClass bc = cand_box_class(key, p.C, p.div_c);
    const int cls = und ? bc.cls : 0;
    for (int c = tid; c < p.C; c += NMS_THREADS) { pfirst[c] = PAR_NONE; pfirst[p.C + c] = PAR_NONE; pcount[c] = 0; }
    if (tid == 0) { w->undecided[0] = PAR_NONE; w->undecided[1] = PAR_NONE; w->kept_front[0] = 0; w->kept_front[1] = 0; }
    __syncthreads();
    for (int r = 0;; ++r) {
        const int b = r & 1;
        uint32_t* const first = pfirst + b * p.C;
        if (und) atomicMin(&first[cls], t);
        {
            const unsigned long long mk = __ballot(und);
            if (mk && lane == __ffsll((long long)mk) - 1) atomicMin(&w->undecided[b], t);
        }
        __syncthreads();
        const uint32_t U = w->undecided[b];                 // every candidate in front of U is decided
        {
            const unsigned long long mk = __ballot(keptf && t < U);
            if (mk && lane == 0) atomicAdd(&w->kept_front[b], (uint32_t)__popcll(mk));
        }
        const uint32_t h = und ? first[cls] : PAR_NONE;
        const bool head = und && h == t;
        if (head) {
            keptf = !cap_binds || (int)pcount[cls] < p.max_per_class;      // (the class's only head this round)
            if (keptf) pcount[cls] = pcount[cls] + 1;
            pflag[t] = keptf ? 1u : 0u;
            und = false;
        }
        if (tid == 0) { w->undecided[b ^ 1] = PAR_NONE; w->kept_front[b ^ 1] = 0; }     // (last read before this round's first barrier)
        __syncthreads();
        if (U == PAR_NONE || w->kept_front[b] >= (uint32_t)p.max_total) break;   // uniform
        if (head) first[cls] = PAR_NONE;                    // (every thread read it before the barrier; next use: round r + 2)
        if (und) {
            // a head that the class cap turned away suppresses nothing -- and everything later in its class is turned away too
            if (pflag[h] == 0u) und = false;
            else if (nms_measure<KIND>(cb, L.sbox[h], p.iou_thr, p.beta) > p.iou_thr) und = false;
        }
    }
    // output slot = number of kept candidates in front (sorted order)
    const unsigned long long mk = __ballot(keptf);
    uint32_t* const wtot = L.wave_kept();
    if (lane == 0) wtot[tid >> 6] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t slot = (uint32_t)__popcll(mk & ((1ull << lane) - 1ull)), total = 0;
    for (int wv = 0; wv < NMS_THREADS / 64; ++wv) {
        const uint32_t c = wtot[wv];
        slot += wv < (tid >> 6) ? c : 0u;
        total += c;
    }
    if (keptf && slot < (uint32_t)p.max_total) L.keep(slot, cb, cls, key, bc.box);
    if (tid == 0) w->kept = total < (uint32_t)p.max_total ? total : (uint32_t)p.max_total;
}

// ---- greedy pass on wave 0 (call it with tid < 64), 64 sorted candidates at a time, one per lane, continuing from the kept
// list.  The sequential rule "keep a candidate unless an EARLIER KEPT box of its class overlaps it" is evaluated in two steps
// that give exactly the sequential result: (1) every lane tests its candidate against the boxes kept before this batch (uniform
// loop over the kept list in LDS; the IoU only for the rare same-class pairs); (2) the batch's survivors are visited in order --
// the lowest surviving lane is final, it is kept, its class and box are broadcast, and later same-class lanes test
// against it.  Per candidate that is a few instructions instead of the ~90 of one-candidate-per-iteration on a wave
// that retires one instruction per ~10 cycles (in-kernel timestamps: 41 us of this kernel were this pass).
template <int KIND, bool AGN>
__device__ __forceinline__ void nms_pass_wave0(const NmsK& p, const NmsLds& L, uint32_t m, int tid) {
    int kept = (int)L.w->kept;
    const bool cap_binds = p.max_per_class < p.max_total;
    for (uint32_t t0 = 0; t0 < m && kept < p.max_total; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)tid;
        const bool valid = t < m;
        const unsigned long long key = valid ? L.skey[t] : 0ull;
        const float4 cb = valid ? L.sbox[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        const CandBoxClass bc = cand_box_class(key, p.C, p.div_c);
        const int cls = valid ? bc.cls : -1;
        bool sup = !valid;
        int same = 0;                                   // kept boxes of this lane's class so far
        // (1) against the boxes kept before this batch: their classes come into registers 64 at a time and are
        // broadcast with v_readlane (an LDS read per kept box would put its latency into every iteration)
        for (int j0 = 0; j0 < kept; j0 += 64) {
            const int kc_reg = j0 + tid < kept ? L.kcls[j0 + tid] : -2;
            const int jn = kept - j0 < 64 ? kept - j0 : 64;
            for (int j = 0; j < jn; ++j) {
                if (AGN) {                                  // every kept box is tested; the class cap counts its own
                    same += __builtin_amdgcn_readlane(kc_reg, j) == cls ? 1 : 0;
                    sup = sup || (nms_measure<KIND>(cb, L.kbox[j0 + j], p.iou_thr, p.beta) > p.iou_thr);
                } else if (__builtin_amdgcn_readlane(kc_reg, j) == cls) {
                    ++same;
                    sup = sup || (nms_measure<KIND>(cb, L.kbox[j0 + j], p.iou_thr, p.beta) > p.iou_thr);
                }
            }
        }
        unsigned long long alive = __ballot(!sup);      // (2) survivors in order
        while (alive && kept < p.max_total) {
            const int c = __ffsll((long long)alive) - 1;           // wave-uniform
            alive &= alive - 1;
            const int ccls = __builtin_amdgcn_readlane(cls, c);
            if (cap_binds && __builtin_amdgcn_readlane(same, c) >= p.max_per_class) continue;   // class is full
            float4 kb;
            kb.x = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cb.x), c));
            kb.y = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cb.y), c));
            kb.z = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cb.z), c));
            kb.w = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(cb.w), c));
            if (tid == c) L.keep((uint32_t)kept, cb, cls, key, bc.box);
            ++kept;
            bool hit = false;
            if (tid > c && !sup && (AGN || cls == ccls)) {
                if (!AGN || cls == ccls) ++same;
                hit = nms_measure<KIND>(cb, kb, p.iou_thr, p.beta) > p.iou_thr;
            }
            sup = sup || hit;
            alive &= ~__ballot(hit);
        }
    }
    if (tid == 0) L.w->kept = (uint32_t)kept;
}


// The driver: chunks of the image's candidates in descending key order until max_total boxes are kept or none remain.
// KIND: the pair measure (nms_measure).  AGN: class-agnostic suppression -- a kept box suppresses later candidates of every class;
// max_per_class still counts per class, and a candidate its class's cap turns away is not kept and suppresses nothing.  The
// round-parallel pass keys its heads by class, which is what makes its rounds independent; with one head slot for all classes it
// would decide one kept box per round behind two workgroup barriers -- the sequence wave 0 walks without them -- so an agnostic
// launch takes the wave-0 pass on the first chunk too, as C > PAR_MAX_C does.
template <int KIND, bool AGN>
__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const NmsK p) {
    extern __shared__ __attribute__((aligned(16))) char nsm[];
    const NmsLds L(nsm, p.max_total, p.C);
    const int n = blockIdx.x, tid = threadIdx.x;
    // nms_list_begin (nms_phases.h), statement for statement: this kernel keeps its own copy, the call changes its listing
    uint32_t cnt = p.counts[(size_t)n * COUNT_STRIDE];
    if (cnt > p.cap) {
        if (tid == 0) atomicOr(p.status, 1u);
        cnt = p.cap;
    }
    const unsigned long long* gk = p.keys + (int64_t)n * p.cap;
    const float* gb = p.dboxes + (int64_t)n * p.nbox * 4;
    if (tid == 0) L.w->kept = 0;
    unsigned long long cutoff = ~0ull;           // exclusive upper bound of keys still to visit
    __syncthreads();
    if (tid == 0) p.counts[(size_t)n * COUNT_STRIDE] = 0;

    while (true) {
        const uint32_t remaining = nms_count_below(L, gk, cnt, cutoff, tid);
        if (remaining == 0) break;
        // pivot = chunk_cap-th largest key below the cutoff (0 when everything fits).  The FIRST chunk is at most NMS_THREADS
        // keys -- what the merge-rank sort and the round-parallel pass take, and nearly always all that max_total kept boxes
        // need; the later ones SORT_CAP
        const uint32_t chunk_cap = cutoff == ~0ull ? (uint32_t)NMS_THREADS : (uint32_t)SORT_CAP;
        unsigned long long pivot = 0;
        bool have_pivot = false;
        if (cutoff == ~0ull && remaining > chunk_cap) have_pivot = nms_histogram_pivot(L, gk, cnt, chunk_cap, tid, &pivot);
        if (remaining > chunk_cap && !have_pivot) pivot = nms_select_pivot(L, gk, cnt, cutoff, chunk_cap, tid);
        uint32_t m2;
        const uint32_t m = nms_take_chunk(L, gk, cnt, cutoff, pivot, chunk_cap, tid, &m2);
        // sort the chunk, descending
        if (m2 <= (uint32_t)NMS_THREADS) nms_rank_sort(L, m, m2, tid);
        else nms_sort_regs<SORT_CAP / NMS_THREADS>(L.skey, L.xbuf(), m2, tid);
        nms_load_boxes(L, gb, p, m, tid);
        const bool par = !AGN && p.C <= PAR_MAX_C && cutoff == ~0ull;
        if (par) nms_pass_parallel<KIND>(p, L, m, tid);
        else if (tid < 64) nms_pass_wave0<KIND, AGN>(p, L, m, tid);
        __syncthreads();
        if ((int)L.w->kept >= p.max_total || pivot == 0) break;
        cutoff = pivot;
        __syncthreads();
    }
    __syncthreads();
    nms_write_outputs(p, L, n, tid);
}

struct NmsKernel { template <int KIND, bool AGN, int> static constexpr auto kernel = nms_kernel<KIND, AGN>; };      // (no methods)

size_t nms_lds_bytes(int max_total, int classes) { return nms_lds_layout(max_total, classes).bytes; }

int decode_launch(const DecodeK& k, hipStream_t stream, int clear_images) {
    // the per-image candidate counters are zero between steps (nms_kernel resets its image's); `clear_images` > 0: the caller
    // cannot vouch for that (first use, or a decode whose NMS never ran) -- clear that many counters first
    if (clear_images > 0) Y4_CHECK_HIP(hipMemsetAsync(k.counts, 0, sizeof(uint32_t) * (size_t)clear_images * COUNT_STRIDE, stream));
    if (3 * (5 + k.C) <= 256) {
        const int64_t cells = (int64_t)k.N * k.cells_per_img;
        Y4_REQUIRE(cells < (1ll << 31), Y4_EINVAL, "decode: %lld cells exceed the 2^31 the cell -> image mapping divides exactly", (long long)cells);
        // fewer than eight 16-cell waves per SIMD of the chip (up to 5 images at 608^2): 4-cell waves
        if (cells < (int64_t)DC_SCREEN * 8192)
            hipLaunchKernelGGL(decode_cell_kernel<DC_SCREEN_SMALL>, dim3((int)((cells + 4 * DC_SCREEN_SMALL - 1) / (4 * DC_SCREEN_SMALL))), dim3(256), 0, stream, k);
        else
            hipLaunchKernelGGL(decode_cell_kernel<DC_SCREEN>, dim3((int)((cells + 4 * DC_SCREEN - 1) / (4 * DC_SCREEN))), dim3(256), 0, stream, k);
    } else {
        const int64_t boxes = (int64_t)k.N * k.nbox;
        hipLaunchKernelGGL(decode_kernel, dim3((int)((boxes + 255) / 256)), dim3(256), 0, stream, k);
    }
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int nms_launch(const NmsK& k, hipStream_t stream) {
    const size_t lds = nms_lds_bytes(k.max_total, k.C);
    Y4_REQUIRE(lds <= 160 * 1024 && k.max_total <= 1024, Y4_EINVAL, "nms: max_total %d needs %zu bytes of LDS", k.max_total, lds);
    if (int r = nms_rule_check("nms", k.kind, k.beta, k.agnostic)) return r;
    return nms_dispatch<NmsKernel>(std::make_index_sequence<6>(), 1, lds, stream, k);
}

}  // namespace y4
