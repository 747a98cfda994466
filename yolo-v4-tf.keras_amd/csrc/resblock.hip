// resblock.hip -- one residual block of a CSP stage as ONE spatially tiled kernel (16-bit dtypes, C = 128 or 64 channels):
//     y = x + Mish(BN(conv3x3(Mish(BN(conv1x1(x))))))            reference custom_layers.py:34-44 (residual_block)
// i.e. the 8 blocks of the 76x76 stage (C = 128) and the 2 blocks of the 152x152 stage (C = 64) at 608x608.
//
// Why.  As implicit GEMMs these 3x3 convs have N = C <= 128 output channels, so the M x N tile that bounds the staging
// traffic per FLOP cannot grow: every K-tile re-stages the activation rows of all 9 taps through L2 -> LDS
// (15-18 bytes per KFLOP against 9 for the 256-channel layers) and they run at 0.65 PFLOP/s.  Here a workgroup owns a
// tile of up to 16x16 pixels: the halo'd tile of x (all C channels) is brought into LDS ONCE, the 1x1 conv runs on it IN
// PLACE (x is pixel-local for a 1x1, so each wave overwrites exactly the rows it read), and the 3x3 conv then reads its
// pixel operand for all 9 taps straight from that tile at shifted rows -- nothing but the 3x3 weights (C*C*2 bytes per
// tap, fragment ordered, lane-linear LDS-DMA through a 4-slot ring) is streamed during the K loop, and the 1x1's
// output never exists in HBM.  Cost: the 1-pixel halo ring of the 1x1 conv is recomputed (1.27x of 10 % of the FLOPs),
// and a tensor whose width is not a multiple of 16 (76, 52, 44) has partially filled edge tiles in that direction.
//
// Tiles and rows.  A tile is 16 columns wide and `rows` output rows high: 16, 12, 8 or 4 at C = 128, 16 or 8 at C = 64 (a multiple of the
// wave rows WM of the 3x3 phase).  The kernel is compiled for the full height -- LDS map, ring, register budget -- and holds one copy of
// the tile body per height (`tile_body`, RbGeom<C, TY>): a tile of `rows` rows loads, computes and stores NOTHING beyond them -- no x pieces
// of halo rows >= rows + 2, no 1x1 fragments of those rows, no 3x3 iterations, residual loads, epilogue or stores of output rows >= rows.
// The host cuts every column of the map into such heights that sum to H (76 = 16 * 4 + 12: no dead rows), deals the tiles to the
// workgroups as balanced lists (rb_build_rows: a whole launch is ONE round), and the workgroup walks its list: one 16-byte entry per
// tile (image, first row, rows, tile column), terminated by rows = 0.  Same MFMAs per output pixel in the same order whatever the
// tile's height and list: bit-identical.
//
// Counted waits.  A wave's vector-memory operations retire in order, and every counted (non-zero) vmcnt wait of the kernel lies in the
// 3x3 loop, i.e. between the tile barrier at the top of a tile -- vmcnt(0): the x pieces, stream steps 0..3 and the previous tile's output
// stores have ALL retired -- and the loop's last wait, again vmcnt(0).  In that window a wave issues exactly: PPW weight pieces per stream
// step (stage_w: unconditional, the same for every wave and every height) and, at the top of step NSTEPS - 4, the 2 * MREP residual loads
// of ITS tile body (MREP = rows / WM is a compile-time constant of the body, and so is the `extra` its three following waits allow).  The
// x pieces are issued at the hand-over, after the loop's vmcnt(0) and before the next tile's vmcnt(0): how many of them a wave issues or
// skips (load_x: wave-uniform, by the NEXT tile's rows) changes no counted wait.  The table entries come through scalar loads, which
// vmcnt does not count.  In the ISA of each instance the s_waitcnt vmcnt(N > 0) are those of wait_vmcnt_lgkm_then_barrier_n inside the
// 3x3 loops, N in {PPW, 2 PPW, PPW + 2 MREP, 2 PPW + 2 MREP}, and the compiler's own in front of the epilogue's first use of the residual
// registers -- behind the loop's vmcnt(0) and ahead of the next tile's loads, where nothing is in flight (profiles/rb_rows/).  (The 12-row body is new; the 16-, 8- and 4-row bodies' waits are those of the earlier
// per-height kernels.)
//
// Numerics: every conv issues the same MFMAs (v_mfma_f32_16x16x32, K ascending in the canonical order of common.h: 64-channel block, tap, channel) on the
// same 16-bit inputs as its conv_igemm kernel and the same fp32 epilogue -> bit-identical to the unfused path.
#include <algorithm>
#include <array>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "conv_chain.h"

#include "phase_trace.h"

namespace y4 {

#ifdef RB_TRACE
// In-kernel phase trace (kernel experiments only; scripts/phase_trace.py resblock): workgroup RB_TR_WG records s_memtime per wave at
// fixed points of the FULL-height tiles among its tiles RB_TR_T0 .. +2 into rb_trace_buf[tile][wave][point]; y4_rb_trace_read() copies it out.
__device__ unsigned long long rb_trace_buf[3 * 8 * 16];
#define RB_TR_WG 8
#define RB_TR_T0 1
#endif

constexpr int RB_T = 16, RB_H = RB_T + 2, RB_WAVES = 8;

// TY = output rows of a tile: 16 (the full 16x16 tile) or less (the same 16 columns).  TY = 16 is the geometry the kernel is launched
// with (LDS map, ring); the smaller ones give a short tile's body its row counts (HR, NFA, MREP).
template <int C, int TY = RB_T> struct RbGeom {
    static constexpr int HR = TY + 2;                  // halo'd rows of the tile (halo'd width: RB_H)
    static constexpr int HROWS = HR * RB_H;            // pixel rows of the LDS tile (no fragment reads past the last one)
    static constexpr int NFA = HR + (2 * HR + 15) / 16;                  // pixel fragments of the 1x1 phase: rows + the two halo columns
    static constexpr int CPR = C / 8;                  // 16-byte chunks of data per pixel row of the LDS tile
    // Rows are PADDED by one chunk instead of XOR-swizzled: 16 lanes reading one chunk of 16 consecutive rows then hit 16
    // different 4-bank groups for ANY first row and chunk (row stride 272 B = 68 banks = 4 mod 64; 144 B = 36 banks), and
    // every fragment address of the 3x3 loop is "lane base + compile-time constant" -- no address VALU, one base VGPR.
    static constexpr int ROWB = C * 2 + 16;            // bytes per pixel row incl. the pad chunk
    static constexpr int XT_PIECES = (HROWS * (CPR + 1) + 63) / 64;        // 1 KB LDS-DMA pieces that fill the tile
    static constexpr int NF = C / 16;                  // output-channel fragments of a conv
    static constexpr int KS1 = C / 32;                 // MFMA k-steps of the 1x1 conv
    // The weights of both convs form ONE stream of equal steps of 64 input channels (2 MFMA k-steps x NF fragments x 1 KB):
    // P steps of the 1x1 conv, then 9 * P steps of the 3x3 conv (64-channel block, then tap: common.h).  They go through a 4-slot LDS ring, three
    // steps ahead of their use, with counted vmcnt waits -- an L2 round trip (~1 us under load) is longer than one step.
    static constexpr int STEP_BYTES = 2 * NF * 1024;
    static constexpr int P = KS1 / 2;                  // steps of the 1x1 conv
    static constexpr int NSTEPS = 10 * P;              // whole stream
    static constexpr int RING = 4;
    static constexpr int PPW = STEP_BYTES / 1024 / RB_WAVES;      // LDS-DMA pieces a wave issues per step
    static constexpr int AFF_BYTES = 4 * C * 4;        // scale1, shift1, scale3, shift3
    static constexpr int AFF_PAD = (AFF_BYTES + 1023) / 1024 * 1024;
    static constexpr int BLOB_BYTES = AFF_PAD + NSTEPS * STEP_BYTES;      // [affine | W1 | W3]
    static constexpr int L_AFF = 0, L_RING = AFF_PAD, L_XT = L_RING + RING * STEP_BYTES;
    // the weight touch's own TOUCH_LDS bytes (conv_common.h): the slack behind the tile's last pixel row inside its last 1 KB piece
    // -- written by that piece's surplus lanes and by the touch, read by nobody -- or, where the slack is smaller, one more KB
    static constexpr int XT_SLACK = XT_PIECES * 1024 - HROWS * (CPR + 1) * 16;
    static constexpr int LDS = L_XT + XT_PIECES * 1024 + (XT_SLACK >= TOUCH_LDS ? 0 : 1024);
    static constexpr int L_TOUCH = LDS - TOUCH_LDS;
    static constexpr int WN = NF / 4, WM = RB_WAVES / WN, MREP = TY / WM;         // wave grid of the 3x3 phase; NREP = 4
    static_assert(C != 64 || 2 * LDS <= 160 * 1024, "C = 64: two workgroups per compute unit (resblock_launch)");
    static_assert(LDS <= 160 * 1024 && MREP >= 1 && MREP * WM == TY && PPW >= 1 && PPW * RB_WAVES * 1024 == STEP_BYTES && NFA <= 3 * RB_WAVES,
                  "resblock geometry");
};

// one tile: rows [y0, y0 + rows) x columns [16 tx, 16 tx + 16) of image n; rows = 0 ends a list
struct alignas(16) RbTile { int n, y0, rows, tx; };

struct ResBlockK {
    const char* in;              // x view
    char* out;                   // y view
    const char* blob;            // RbGeom<C>::BLOB_BYTES (pack_resblock)
    int in_cstride, in_coff, out_cstride, out_coff;
    unsigned in_bytes, out_bytes;
    int N, H, W;                 // images, rows / columns of the block's tensors
    const RbTile* tab;           // this launch's tile lists (rb_build_rows): workgroup b walks entries [b * stride, ..) up to the first with rows = 0
    int stride;                  // entries per list, the terminator included
    int touch;                   // weight touch (conv_common.h) of the block's blob at kernel start
};

template <int DT, int C>
__global__ __launch_bounds__(64 * RB_WAVES, C == 64 ? 4 : 2) void resblock_kernel(const ResBlockK p) {
    using E = Elem<DT>;
    using G = RbGeom<C>;
    constexpr int ROWB = G::ROWB, CPR = G::CPR, NF = G::NF;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane & 15, g = lane >> 4;
    const int wm = wave / G::WN, wn = wave - wm * G::WN;
    const float* const aff = (const float*)(smem + G::L_AFF);
    char* const XT = smem + G::L_XT;
    char* const ring = smem + G::L_RING;

    // this workgroup's list: entry = (image, first output row, rows, tile column)
    // (read through the constant address space: the table is read-only for the life of the launch, and a wave-uniform constant load is
    // a scalar load -- a vector load here would join the wave's vector-memory queue in front of the tile barrier)
    typedef const __attribute__((address_space(4))) RbTile* RbList;
    const RbList list = (RbList)(p.tab + (size_t)blockIdx.x * p.stride);
    auto entry = [&](int j) {
        return RbTile{__builtin_amdgcn_readfirstlane(list[j].n), __builtin_amdgcn_readfirstlane(list[j].y0),
                      __builtin_amdgcn_readfirstlane(list[j].rows), __builtin_amdgcn_readfirstlane(list[j].tx)};
    };

    const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.blob, G::BLOB_BYTES);
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(p.in, p.in_bytes), rs_out = make_rsrc(p.out, p.out_bytes);
    // the blob (affine tables + both convs' weight streams: every tile streams all of it) -> this XCD's L2, shared out over the
    // workgroups (conv_common.h: weight_touch); the dwords land in LDS bytes of their own (RbGeom::L_TOUCH)
    if (p.touch != 0) weight_touch(rb, smem + G::L_TOUCH, 0, G::BLOB_BYTES, wave, RB_WAVES, lane);
    // affine -> LDS once per workgroup
    for (int u = wave; u < G::AFF_PAD / 1024; u += RB_WAVES)
        buffer_load16_lds(rb, smem + __builtin_amdgcn_readfirstlane(u * 1024), u * 1024 + lane * 16, 0);
    // step `st` of the weight stream -> ring slot st % RING (fragment ordered in memory: a plain lane-linear copy);
    // every wave issues exactly PPW pieces per step, which is what the counted waits below rely on
    auto stage_w = [&](int st) {
        char* const dst = ring + (st & (G::RING - 1)) * G::STEP_BYTES;
#pragma unroll
        for (int k = 0; k < G::PPW; ++k) {
            const int u = wave + k * RB_WAVES;
            buffer_load16_lds(rb, dst + __builtin_amdgcn_readfirstlane(u * 1024), G::AFF_PAD + u * 1024 + lane * 16, st * G::STEP_BYTES);
        }
    };
    // halo'd tile of x -> XT: the tile's rows + 2 halo'd rows (out-of-image pixels read as zeros; pixel rows behind them are not
    // loaded -- nobody reads them)
    // The tile is written lane-linearly in 16-byte slots (slot = piece * 64 + lane; a pixel row is CPR data slots + the pad slot), a
    // wave takes pieces wave, wave + 8, ...: from one piece to the next every lane's slot advances by the same 512, so its (row,
    // column, chunk) and its byte offset advance by constants plus two carries.  ~15 VALU instructions per piece instead of the ~35
    // of two divisions by constants and the full offset polynomial: the wave issues one VALU instruction per ~9 cycles, and the
    // trace priced the 12 pieces of a C=128 tile at 3.3 k cycles of the epilogue they are issued under.
    auto load_x = [&](const RbTile e) {
        const int n = e.n, yo = e.y0, tx = e.tx;
        const int hr = min(e.rows, RB_T) + 2;                                 // halo'd rows of THIS tile (never past the LDS tile)
        const int pieces = (hr * RB_H * (CPR + 1) + 63) >> 6;               // (<= G::XT_PIECES)
        const int y0 = yo - 1, x0 = tx * RB_T - 1;
        constexpr int SPR = CPR + 1, DSLOT = RB_WAVES * 64, DHP = DSLOT / SPR, DCH = DSLOT % SPR, DHY = DHP / RB_H, DHX = DHP % RB_H;
        static_assert(DCH + SPR - 1 < 2 * SPR && DHX + RB_H < 2 * RB_H, "one carry per step");
        int slot0 = wave * 64 + lane;
        asm volatile("" : "+v"(slot0));        // (per tile: hoisted out of the tile loop, the pieces' positions would cost ~3 registers each)
        const int hp0 = slot0 / SPR;
        int ch = slot0 - hp0 * SPR, hy = hp0 / RB_H;
        int hx = hp0 - hy * RB_H;
        const int pix_b = p.in_cstride * 2, row_b = p.W * pix_b;           // bytes per pixel / per image row of the view
        int off = (((n * p.H + y0) * p.W + x0) * p.in_cstride + p.in_coff) * 2 + hy * row_b + hx * pix_b + ch * 16;
        const int d_off = DHY * row_b + DHX * pix_b + DCH * 16, c_ch = pix_b - SPR * 16, c_hx = row_b - RB_H * pix_b;
#pragma unroll
        for (int k = 0; k * RB_WAVES < G::XT_PIECES; ++k) {
            const int u = wave + k * RB_WAVES;
            if (u < pieces) {                                               // (wave-uniform: the pieces of rows this tile does not have are skipped)
                const bool ok = ch < CPR && hy < hr && (unsigned)(y0 + hy) < (unsigned)p.H && (unsigned)(x0 + hx) < (unsigned)p.W;
                buffer_load16_lds(rs_in, XT + __builtin_amdgcn_readfirstlane(u * 1024), ok ? off : (int)0x80000000, 0);
            }
            ch += DCH; hx += DHX; hy += DHY; off += d_off;
            if (ch >= SPR) { ch -= SPR; hx += 1; off += c_ch; }
            if (hx >= RB_H) { hx -= RB_H; hy += 1; off += c_hx; }
        }
    };
    RbTile cur = entry(0);
    if (cur.rows != 0) { load_x(cur); stage_w(0); stage_w(1); stage_w(2); stage_w(3); }

#ifdef RB_TRACE
    int tr_i = 0;
    unsigned long long tr_t[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // One tile of TY rows, `cur`; `nxt` is the list's next entry (rows = 0: none), whose loads go out under this tile's epilogue.
    auto tile_body = [&](auto ty_c, const RbTile nxt) __attribute__((always_inline)) {
        constexpr int TY = decltype(ty_c)::value;
        using T = RbGeom<C, TY>;
        constexpr int MREP = T::MREP;
        const int n = cur.n, y_out0 = cur.y0, tx = cur.tx;
        // A short tile's body derives its lane constants (fragment rows, LDS bases) afresh per tile: hoisted out of the tile loop beside
        // the full tile's, they would sit in registers the full tile's body has no room for.  At C = 64, which runs at its 128-register
        // cap, the full tile's body does so too: two bodies' worth of hoisted constants spilled (a few dozen VALU instructions per tile).
        int lane_t = lane;
        if constexpr (TY != RB_T || C == 64) asm volatile("" : "+v"(lane_t));
        const int lane = lane_t, q = lane & 15, g = lane >> 4;
#ifdef RB_TRACE
        const bool tr_on = TY == RB_T && C == RB_TRACE && blockIdx.x == RB_TR_WG && tr_i >= RB_TR_T0 && tr_i < RB_TR_T0 + 3;
#endif
        PHASE_POINT(0);                           // arrives at the tile barrier
        wait_vmcnt_then_barrier<0>();          // x tile and stream steps 0..3 landed; all waves left the previous tile
        PHASE_POINT(1);                           // barrier passed

        // residual = x at this lane's output pixels / channels: read a second time from memory under the 3x3 loop, not from the x tile
        // in LDS in front of the 1x1 phase (same bytes, one more barrier; measured neutral: LABNOTES.md section 4.1c)
        u32x4 res[MREP][2];

        // ================= phase A: t = Mish(BN(conv1x1(x))) on the halo'd tile, IN PLACE; zero outside the image.
        // TY + 2 row fragments + the fragments holding the two halo columns (21 at TY = 16); a wave takes fragments wave, wave+8,
        // wave+16 TOGETHER, so that each weight fragment is read from LDS once per wave and 16-24 MFMAs are independent.
        auto phase_a = [&](auto nfr_c) {
            constexpr int NFR = decltype(nfr_c)::value;
            char* row[NFR];
            bool inside[NFR];
#pragma unroll
            for (int k = 0; k < NFR; ++k) {
                const int f = wave + k * RB_WAVES;
                int hy, hx;
                if (f < T::HR) { hy = f; hx = 1 + q; }
                else { const int pp = min((f - T::HR) * 16 + q, 2 * T::HR - 1); hy = pp >> 1; hx = (pp & 1) * (RB_H - 1); }
                const int r = hy * RB_H + hx;
                row[k] = XT + r * ROWB;
                const int gy = y_out0 - 1 + hy, gx = tx * RB_T - 1 + hx;
                inside[k] = (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            }
            f32x4 acc[NFR][NF];
#pragma unroll
            for (int k = 0; k < NFR; ++k)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[k][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < G::KS1; ++s) {
                u32x4 xf[NFR], wf[NF];
#pragma unroll
                for (int k = 0; k < NFR; ++k) xf[k] = *(const u32x4*)(row[k] + (s * 4 + g) * 16);
#pragma unroll
                for (int j = 0; j < NF; ++j) wf[j] = *(const u32x4*)(ring + (s >> 1) * G::STEP_BYTES + (((s & 1) * NF + j) * 64 + lane) * 16);
#pragma unroll
                for (int k = 0; k < NFR; ++k)
#pragma unroll
                    for (int j = 0; j < NF; ++j) Mma<DT>::run(acc[k][j], wf[j], xf[k]);
            }
#pragma unroll
            for (int c = 0; c < NF / 2; ++c) {
                float sc[8], sh[8];
#pragma unroll
                for (int h = 0; h < 8; h += 4) {
                    const int ch = chunk_channel(0, c, g) + h;
                    const f32x4 s4 = *(const f32x4*)(aff + ch), h4 = *(const f32x4*)(aff + C + ch);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { sc[h + e] = s4[e]; sh[h + e] = h4[e]; }
                }
#pragma unroll
                for (int k = 0; k < NFR; ++k) {
                    float v[8];
                    bn_act4<true, Y4_ACT_MISH>(acc[k][2 * c], sc, sh, v);
                    bn_act4<true, Y4_ACT_MISH>(acc[k][2 * c + 1], sc + 4, sh + 4, v + 4);
                    u32x4 pk;
                    E::store_chunk(&pk, v);
                    if (!inside[k]) pk = u32x4{0u, 0u, 0u, 0u};
                    *(u32x4*)(row[k] + (4 * c + g) * 16) = pk;
                }
            }
        };
        // NFA fragments over 8 waves: fragments wave, wave + 8, wave + 16 (wave-uniform counts)
        if (wave + 2 * RB_WAVES < T::NFA) phase_a(std::integral_constant<int, 3>{});
        else if (wave + RB_WAVES < T::NFA) phase_a(std::integral_constant<int, 2>{});
        else if (wave < T::NFA) phase_a(std::integral_constant<int, 1>{});
        PHASE_POINT(2);                           // 1x1 phase done (MFMAs, Mish, in-place stores issued)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        PHASE_POINT(3);                           // mid barrier passed

        // ================= phase C: y = x + Mish(BN(conv3x3(t))): 9 taps x C/64 stream steps, weights through the ring.
        // Software pipelined at MFMA k-step (32-channel) granularity: the fragments of half-step h+1 are read from LDS
        // while the 4*MREP MFMAs of half-step h issue; the wait + barrier that admits the next stream step sits between
        // the two halves of a step.  Fully unrolled (taps, slots and wait counts are compile-time).
        {
            // residual = x at this lane's output pixels / channels, straight from memory (its round trip hides under the loop)
            // (through the buffer descriptors: one 32-bit offset per access -- a dead pixel's is out of range, its load reads zeros and
            // its store is dropped -- instead of 64-bit pointer arithmetic per access)
            int pix[MREP];
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                const int gy = y_out0 + wm * MREP + i, gx = tx * RB_T + q;
                pix[i] = gy < p.H && gx < p.W ? (n * p.H + gy) * p.W + gx : -1;
            }
            auto load_res = [&]() {
#pragma unroll
                for (int i = 0; i < MREP; ++i) {
                    const int o = pix[i] < 0 ? (int)0x80000000 : (pix[i] * p.in_cstride + p.in_coff) * 2;
#pragma unroll
                    for (int c = 0; c < 2; ++c) res[i][c] = buffer_load16(rs_in, o + chunk_channel(wn * 64, c, g) * 2);
                }
            };
            // The residual is needed in the epilogue only: its 2 MREP loads go out at the top of stream step S0, four steps before the
            // end of the loop instead of in front of it, and stay in flight beside the stream's own loads: a wave's loads retire in
            // order, so the counted waits of steps S0 .. S0 + 2 allow that many more outstanding.  Likewise stream step 3, whose ring
            // slot is free from the start, is issued with steps 0..2 at the tile hand-over instead of behind the mid barrier (that
            // stretch was on the tile's critical path: LABNOTES.md section 4.1c, "Late round 4").
            constexpr int S0 = G::NSTEPS - 4, RES_LOADS = 2 * MREP;
            f32x4 acc[MREP][4];
#pragma unroll
            for (int i = 0; i < MREP; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            // stream steps 4 .. P+3 (their slots < P held the 1x1 weights)
#pragma unroll
            for (int st = 4; st <= G::P + 3; ++st) stage_w(st);
            const char* const xbase = XT + ((wm * MREP) * RB_H + q) * ROWB + g * 16;       // fragment 0, tap (0, 0), chunk g
            u32x4 xf[2][MREP], wf[2][4];
            auto read_frags = [&](int buf, int st, int kk) {              // all arguments are compile-time after unrolling
                const int ks = st - G::P;
                const int cb = ks / 9, tap = ks - cb * 9;                  // tap `tap` of 64-channel block `cb`: the canonical K order (common.h)
                const int ky = tap / 3, kx = tap - ky * 3;
                const char* const wst = ring + (st & (G::RING - 1)) * G::STEP_BYTES;
#pragma unroll
                for (int i = 0; i < MREP; ++i) {
                    xf[buf][i] = *(const u32x4*)(xbase + ((i + ky) * RB_H + kx) * ROWB + (cb * 8 + kk * 4) * 16);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[buf][j] = *(const u32x4*)(wst + ((kk * NF + wn * 4 + j) * 64 + lane) * 16);
            };
            auto mma = [&](int buf) {
#pragma unroll
                for (int i = 0; i < MREP; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        Mma<DT>::run(acc[i][j], wf[buf][j], xf[buf][i]);
            };
            PHASE_POINT(4);                           // residual loads + stream steps issued
            read_frags(0, G::P, 0);                                        // step P landed at the top of the tile
#pragma unroll
            for (int st = G::P; st < G::NSTEPS; ++st) {
                if (st == G::P + 3 * G::P) PHASE_POINT(5);                    // a third of the stream done
                if (st == G::P + 6 * G::P) PHASE_POINT(6);                    // two thirds
                if (st == S0) load_res();
                // sched_barrier: hipcc otherwise re-serialises the pipeline into "read one fragment, wait for it, 4 MFMAs"
                // (fewer live registers, but every wait exposes the LDS latency); pinned, the 8-12 reads of the next
                // half-step are all in flight while the 4*MREP MFMAs of this one issue
                read_frags(1, st, 1);
                __builtin_amdgcn_sched_barrier(0);
                mma(0);
                __builtin_amdgcn_sched_barrier(0);
                if (st + 1 < G::NSTEPS) {
                    // step st+1 has landed when only the younger steps (issued through st+3) are still in flight; the
                    // barrier also proves every wave has read slot(st) to the end, which the next stage_w overwrites: the
                    // wait includes lgkmcnt(0) -- the kk = 1 reads of slot(st) issued above are not consumed before mma(1),
                    // so without it "read to the end" would hold by timing only (they have had all of mma(0) to land: free)
                    constexpr int LAST = G::NSTEPS - 1;
                    const int younger = (st + 3 < LAST ? st + 3 : LAST) - (st + 1);
                    // (st is a compile-time constant after unrolling: one of the variants survives)
                    const int extra = st >= S0 && st <= S0 + 2 ? RES_LOADS : 0;
                    static_assert(S0 > G::P && 2 * G::PPW + RES_LOADS < 64, "window of the residual's loads");
                    wait_vmcnt_lgkm_then_barrier_n<2 * G::PPW + RES_LOADS>(younger == 0 ? 0 : (younger >= 2 ? 2 : 1) * G::PPW + extra);
                    if (st + 4 < G::NSTEPS) stage_w(st + 4);
                    read_frags(0, st + 1, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                mma(1);
                __builtin_amdgcn_sched_barrier(0);
            }
            PHASE_POINT(7);                           // all taps done
            // every wave is done with the tile and the ring: bring in the next tile under this tile's epilogue
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            PHASE_POINT(8);                           // end barrier passed
            // The residual has landed (the loop's last counted wait was vmcnt(0)), but the compiler does not know: its own wait in
            // front of the first use would sit behind the next tile's loads issued below and, counted conservatively, hold the
            // epilogue until most of THOSE have landed too.  Using the registers here puts that wait where it costs nothing.
#pragma unroll
            for (int i = 0; i < MREP; ++i)
#pragma unroll
                for (int c = 0; c < 2; ++c) asm volatile("" : "+v"(res[i][c]));
            if (nxt.rows != 0) { load_x(nxt); stage_w(0); stage_w(1); stage_w(2); stage_w(3); }
            PHASE_POINT(9);                           // next tile's loads issued
            float sc3[16], sh3[16];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int h = 0; h < 8; h += 4) {
                    const int ch = chunk_channel(wn * 64, c, g) + h;
                    const f32x4 s4 = *(const f32x4*)(aff + 2 * C + ch), h4 = *(const f32x4*)(aff + 3 * C + ch);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { sc3[c * 8 + h + e] = s4[e]; sh3[c * 8 + h + e] = h4[e]; }
                }
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                float v[16];
#pragma unroll
                for (int j = 0; j < 4; ++j) bn_act4<true, Y4_ACT_MISH>(acc[i][j], sc3 + j * 4, sh3 + j * 4, v + j * 4);
                const int o = pix[i] < 0 ? (int)0x80000000 : (pix[i] * p.out_cstride + p.out_coff) * 2;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    float rv[8];
                    E::load_chunk(&res[i][c], rv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[c * 8 + e] += rv[e];      // residual Add (custom_layers.py:44), after the activation
                    u32x4 pk;
                    E::store_chunk(&pk, v + c * 8);
                    // write-back stores; nt / write-through cache policy bits were slower or neutral (LABNOTES.md section 4.1c)
                    buffer_store16<0>(rs_out, pk, o + chunk_channel(wn * 64, c, g) * 2);
                }
            }
        }
        PHASE_POINT(10);                          // epilogue done, stores issued
#ifdef RB_TRACE
        if (tr_on && lane == 0) {
#pragma unroll
            for (int k = 0; k < 11; ++k) rb_trace_buf[((tr_i - RB_TR_T0) * 8 + wave) * 16 + k] = tr_t[k];
        }
        ++tr_i;
#endif
    };

    for (int j = 1; cur.rows != 0; ++j) {
        const RbTile nxt = entry(j);
        // (wave-uniform; the host admits no other height -- rb_build_rows -- and an entry that is none of them would run as the smallest)
        if constexpr (C == 128) {
            if (cur.rows == 16) tile_body(std::integral_constant<int, 16>{}, nxt);
            else if (cur.rows == 12) tile_body(std::integral_constant<int, 12>{}, nxt);
            else if (cur.rows == 8) tile_body(std::integral_constant<int, 8>{}, nxt);
            else tile_body(std::integral_constant<int, 4>{}, nxt);
        } else {
            if (cur.rows == 16) tile_body(std::integral_constant<int, 16>{}, nxt);
            else tile_body(std::integral_constant<int, 8>{}, nxt);
        }
        cur = nxt;
    }
}

PHASE_TRACE_READER(y4_rb_trace_read, rb_trace_buf)

// ------------------------------------------------------------------------------------------------ tile tables (host)
// The tile set of one launch and its deal to the workgroups, as the kernel reads it: int32 quadruples -- a header {grid, stride, a, b}
// and then grid lists of `stride` entries {image, first row, rows, tile column}, each list closed by an entry with rows = 0.  List b
// belongs to workgroup b, which runs on XCD b % 8.  A function of (n, h, w, c, slots) alone.
struct RbTable {
    std::vector<int32_t> v;
    int grid = 0, stride = 0;
};

// allowed heights: the multiples of the 3x3 phase's wave rows (RbGeom::WM: 4 at C = 128, 8 at C = 64) up to 16, tallest first
static int rb_heights(int c, int out[4]) {
    const int wm = c == 128 ? RbGeom<128>::WM : RbGeom<64>::WM;
    int k = 0;
    for (int t = RB_T; t >= wm; t -= wm) out[k++] = t;
    return k;
}
// A tile's cost in cycles, a + b * rows, from the phase trace of the full C = 128 tile (LABNOTES.md section 4.1c: 45.9 k cycles): the 3x3 loop
// (26.6 k) and the epilogue (~4.8 k) scale with rows, the 1x1 phase (~8.8 k over 18 halo'd rows) with rows + 2 -> b = 2.45 k per row;
// its two halo rows, the hand-over, the issue of the stream steps and the three barriers do not -> a = 6.7 k.  C = 64 (22.2 k cycles per
// tile) has no breakdown of its own: the same shares.
static void rb_cost_model(int c, int* a, int* b) {
    if (c == 128) { *a = 6700; *b = 2450; }
    else { *a = 3240; *b = 1185; }
}

// `m` lists for jobs of the given costs: longest-processing-time-first, then first-fit-decreasing under a capacity found by bisection
// below the LPT result (MULTIFIT): LPT alone misses a perfect packing such as 26 x [16 16 16] + [16 16 12] + 4 x [12 12 12 12] + [12 12 12]
// -- it spreads the tall tiles evenly first and then has to stack the short ones on lists that are already level.
// where[i] = list of job i; returns the longest list's cost.
static int64_t rb_deal(const std::vector<int>& cost, int m, std::vector<int>& where) {
    const int nj = (int)cost.size();
    std::vector<int> order(nj);
    for (int i = 0; i < nj; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
    where.assign(nj, 0);
    if (nj == 0) return 0;
    std::vector<int64_t> load(m, 0);
    int64_t total = 0;
    for (int i : order) {
        int best = 0;
        for (int j = 1; j < m; ++j)
            if (load[j] < load[best]) best = j;
        where[i] = best; load[best] += cost[i]; total += cost[i];
    }
    int64_t hi = *std::max_element(load.begin(), load.end());
    int64_t lo = std::max<int64_t>((total + m - 1) / m, cost[order[0]]);
    std::vector<int> trial(nj);
    while (lo < hi) {
        const int64_t cap = (lo + hi) / 2;
        std::fill(load.begin(), load.end(), 0);
        bool fits = true;
        int64_t longest = 0;
        for (int i : order) {
            int j = 0;
            while (j < m && load[j] + cost[i] > cap) ++j;
            if (j == m) { fits = false; break; }
            trial[i] = j; load[j] += cost[i]; longest = std::max(longest, load[j]);
        }
        if (fits) { where = trial; hi = longest; }
        else lo = cap + 1;
    }
    return hi;
}

// lists (one vector of tiles per workgroup, workgroup b on XCD b % 8) -> table
static void rb_emit(const std::vector<std::vector<RbTile>>& lists, int c, RbTable& t) {
    size_t longest = 0;
    for (const auto& l : lists) longest = std::max(longest, l.size());
    t.grid = (int)lists.size(); t.stride = (int)longest + 1;
    int a, b;
    rb_cost_model(c, &a, &b);
    t.v.assign(4 + (size_t)t.grid * t.stride * 4, 0);
    t.v[0] = t.grid; t.v[1] = t.stride; t.v[2] = a; t.v[3] = b;
    for (int l = 0; l < t.grid; ++l)
        for (size_t j = 0; j < lists[l].size(); ++j) {
            int32_t* e = t.v.data() + 4 + ((size_t)l * t.stride + j) * 4;
            e[0] = lists[l][j].n; e[1] = lists[l][j].y0; e[2] = lists[l][j].rows; e[3] = lists[l][j].tx;
        }
}

// The exact-row tile set of an (n, h, w) map and its deal to `slots` workgroups (a multiple of 8), slots / 8 per XCD.
// Every column is cut into tiles of one body height `hc` and a remainder from the smaller heights, summing to h rounded up to the smallest
// height (so at most one tile per column hangs over the lower edge, by less than that height).  The tiles, in (image, row, column)
// order, are cut into 8 contiguous ranges of equal cost, one per XCD -- an XCD's L2 then holds neighbouring tiles' shared halo rows
// -- and each range is dealt to its XCD's lists (rb_deal).  The body height is the one whose longest list is cheapest, the taller on a
// tie: 16 for a batch that fills the slots several times over, a smaller one for a batch with fewer full tiles than slots.
static void rb_build_rows(int n, int h, int w, int c, int slots, RbTable& out) {
    int hs[4], a, b;
    const int nh = rb_heights(c, hs), hmin = hs[nh - 1], tiles_x = (w + RB_T - 1) / RB_T, m = slots / 8;
    rb_cost_model(c, &a, &b);
    const int hp = (h + hmin - 1) / hmin * hmin;
    int64_t best_span = -1;
    std::vector<std::vector<RbTile>> best;
    for (int pi = 0; pi < nh; ++pi) {
        const int hc = hs[pi];
        std::vector<int> cut;                            // heights of one column, top to bottom
        int left = hp;
        for (; left >= hc; left -= hc) cut.push_back(hc);
        for (int k = pi + 1; k < nh; ++k)
            for (; left >= hs[k]; left -= hs[k]) cut.push_back(hs[k]);
        std::vector<RbTile> tiles;
        std::vector<int> cost;
        for (int i = 0; i < n; ++i) {
            int y0 = 0;
            for (int rows : cut) {
                for (int tx = 0; tx < tiles_x; ++tx) { tiles.push_back(RbTile{i, y0, rows, tx}); cost.push_back(a + b * rows); }
                y0 += rows;
            }
        }
        int64_t total = 0, before = 0;
        for (int v : cost) total += v;
        std::vector<std::vector<int>> of_xcd(8);        // tile indices per XCD: by the midpoint of the tile's share of the total cost
        for (size_t i = 0; i < tiles.size(); ++i) {
            of_xcd[std::min<int64_t>(7, (2 * before + cost[i]) * 8 / (2 * total))].push_back((int)i);
            before += cost[i];
        }
        std::vector<std::vector<RbTile>> lists((size_t)slots);
        int64_t span = 0;
        int used = 1;                                    // lists in use on the fullest XCD
        for (int x = 0; x < 8; ++x) {
            std::vector<int> cx, where;
            for (int i : of_xcd[x]) cx.push_back(cost[i]);
            span = std::max(span, rb_deal(cx, m, where));
            // the XCD's lists, costliest first (its empty ones last, behind the launch's grid), each in (image, row, column) order
            std::vector<int64_t> load(m, 0);
            for (size_t k = 0; k < cx.size(); ++k) load[where[k]] += cx[k];
            std::vector<int> rank(m), pos(m);
            for (int j = 0; j < m; ++j) rank[j] = j;
            std::stable_sort(rank.begin(), rank.end(), [&](int p, int q) { return load[p] > load[q]; });
            for (int j = 0; j < m; ++j) { pos[rank[j]] = j; if (load[rank[j]] > 0) used = std::max(used, j + 1); }
            for (size_t k = 0; k < cx.size(); ++k) lists[(size_t)pos[where[k]] * 8 + x].push_back(tiles[of_xcd[x][k]]);
        }
        lists.resize((size_t)used * 8);
        if (best_span < 0 || span < best_span) { best_span = span; best.swap(lists); }
    }
    rb_emit(best, c, out);
}

// Y4_RB_ROWS=0 (A/B measurements): the tile set and walk of the kernel's earlier form as tables.  Every tile is 16 rows high, dead rows
// below the map included; workgroup b of `grid` strides through its XCD's eighth of the tiles; the tiles of the last, partial round
// run as half / quarter tiles in a second launch when all their parts fit one round (Y4_RB_PARTS=0: never).
static void rb_build_static(int n, int h, int w, int c, int slots, bool parts_on, std::vector<RbTable>& out) {
    const int tiles_x = (w + RB_T - 1) / RB_T, tiles_y = (h + RB_T - 1) / RB_T, per_img = tiles_x * tiles_y, ntiles = n * per_img;
    const int maxp = c == 128 ? 4 : 2;
    const int full = ntiles / slots * slots, rem = ntiles - full;
    int parts = 1;
    if (parts_on && rem > 0)
        for (int pp = 2; pp <= maxp; pp *= 2)
            if (rem * pp <= slots) parts = pp;
    auto walk = [&](int t_begin, int t_end, int np) {
        const int span = t_end - t_begin, ty = RB_T / np;
        int grid = std::min(slots, (span + 7) & ~7);
        if (grid < 8) grid = 8;
        std::vector<std::vector<RbTile>> lists((size_t)grid);
        for (int blk = 0; blk < grid; ++blk) {
            const int xcd = blk & 7, bi = blk >> 3, nb_x = (grid - xcd + 7) >> 3;
            const int t_lo = t_begin + (int)((int64_t)span * xcd / 8), t_hi = t_begin + (int)((int64_t)span * (xcd + 1) / 8);
            for (int t = t_lo + bi; t < t_hi; t += nb_x) {
                const int f = t / np, part = t - f * np, img = f / per_img, r = f - img * per_img;
                lists[blk].push_back(RbTile{img, r / tiles_x * RB_T + part * ty, ty, r % tiles_x});
            }
        }
        out.emplace_back();
        rb_emit(lists, c, out.back());
    };
    if (parts == 1) { walk(0, ntiles, 1); return; }
    if (full > 0) walk(0, full, 1);
    walk(full * parts, ntiles * parts, parts);
}

// Y4_RB_ROWS=0: the static walk above instead of exact rows and dealt lists (results are the same either way)
static bool rb_rows_enabled() {
    static const bool on = [] { const char* e = getenv("Y4_RB_ROWS"); return !(e && e[0] == '0'); }();
    return on;
}
// Y4_RB_PARTS=0 (with Y4_RB_ROWS=0) runs every tile as a full 16x16 tile
static bool rb_parts_enabled() {
    static const bool on = [] { const char* e = getenv("Y4_RB_PARTS"); return !(e && e[0] == '0'); }();
    return on;
}
// Y4_RB_SLOTS=<k> (tests): at most k workgroup slots (a multiple of 8, at least 8), so that a small map's lists hold several tiles
static int rb_slots_cap() {
    static const int cap = [] { const char* e = getenv("Y4_RB_SLOTS"); return e && e[0] ? std::max(8, atoi(e) & ~7) : 0; }();
    return cap;
}

// The tables of a shape on the current device, built and uploaded on first use and kept for the life of the process: a read-only
// buffer of their own, outside every handle's workspace, shared by every handle (and stream) that runs the shape.  The upload is a
// synchronous copy: a shape's first launch must not lie inside a stream capture (run the shape once before capturing).
struct RbLaunch { const RbTile* tab; int grid, stride; };
static int rb_tables(int n, int h, int w, int c, int slots, const std::vector<RbLaunch>** out) {
    static std::mutex mu;
    static std::map<std::array<int, 6>, std::vector<RbLaunch>> cache;
    int dev = 0;
    Y4_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    const std::array<int, 6> key{dev, n, h, w, c, slots};
    auto it = cache.find(key);
    if (it == cache.end()) {
        std::vector<RbTable> tabs;
        if (rb_rows_enabled()) { tabs.emplace_back(); rb_build_rows(n, h, w, c, slots, tabs.back()); }
        else rb_build_static(n, h, w, c, slots, rb_parts_enabled(), tabs);
        // one buffer for the shape's tables; the entry is inserted only once it is whole (an error returns with nothing kept)
        std::vector<int32_t> all;
        std::vector<RbLaunch> ls;
        for (const RbTable& t : tabs) all.insert(all.end(), t.v.begin(), t.v.end());
        char* d = nullptr;
        Y4_CHECK_HIP(hipMalloc((void**)&d, all.size() * sizeof(int32_t)));
        if (hipError_t e = hipMemcpy(d, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice)) {
            (void)hipFree(d);
            Y4_CHECK_HIP(e);
        }
        size_t at = 0;
        for (const RbTable& t : tabs) {
            ls.push_back(RbLaunch{(const RbTile*)(d + at * sizeof(int32_t)) + 1, t.grid, t.stride});       // (+ 1: behind the header)
            at += t.v.size();
        }
        it = cache.emplace(key, std::move(ls)).first;
    }
    *out = &it->second;
    return Y4_OK;
}

// ------------------------------------------------------------------------------------------------ launch
bool resblock_supported(int dtype, int c) { return dtype != Y4_F32 && (c == 128 || c == 64); }
size_t resblock_blob_bytes(int c) { return c == 128 ? RbGeom<128>::BLOB_BYTES : RbGeom<64>::BLOB_BYTES; }

template <int DT, int C>
static int resblock_run(ResBlockK& k, const std::vector<RbLaunch>& ls, hipStream_t stream) {
    constexpr int lds = RbGeom<C>::LDS;
    for (const RbLaunch& l : ls) {
        k.tab = l.tab; k.stride = l.stride;
        if (int r = launch_lds<resblock_kernel<DT, C>>(lds, dim3(l.grid), dim3(64 * RB_WAVES), lds, stream, k)) return r;
    }
    return Y4_OK;
}

int resblock_launch(int dtype, int c, const void* in, int n, int h, int w, int in_cstride, int in_coff, const void* blob, void* out,
                    int out_cstride, int out_coff, hipStream_t stream) {
    Y4_REQUIRE(resblock_supported(dtype, c), Y4_EINVAL, "resblock: dtype %d / %d channels not supported", dtype, c);
    Y4_REQUIRE(in && blob && out && n > 0 && h > 0 && w > 0, Y4_EINVAL, "resblock: null pointer / empty batch");
    Y4_REQUIRE(in_cstride % 8 == 0 && in_coff % 8 == 0 && out_cstride % 8 == 0 && out_coff % 8 == 0, Y4_EINVAL,
               "resblock: views not 16-byte aligned");
    const int64_t in_bytes = (int64_t)n * h * w * in_cstride * 2;
    const int64_t out_bytes = (int64_t)n * h * w * out_cstride * 2;
    Y4_REQUIRE(in_bytes < (1ll << 31) && out_bytes < (1ll << 31), Y4_EINVAL,
               "resblock: input (%lld B) or output (%lld B) exceeds the 2 GiB buffer-descriptor range", (long long)in_bytes, (long long)out_bytes);
    ResBlockK k{};
    k.in = (const char*)in; k.out = (char*)out; k.blob = (const char*)blob;
    k.in_cstride = in_cstride; k.in_coff = in_coff; k.out_cstride = out_cstride; k.out_coff = out_coff;
    k.in_bytes = (unsigned)in_bytes; k.out_bytes = (unsigned)out_bytes;
    k.N = n; k.H = h; k.W = w;
    k.touch = weight_touch_enabled() ? 1 : 0;
    int cus = 0;
    if (int r = cu_count(&cus)) return r;
    // `slots` workgroups fit the GPU at once, the same number on every XCD: one per CU for C = 128 (LDS), two for C = 64 (79 KB
    // each: their phases overlap)
    int slots = std::max(8, (cus & ~7) * (c == 64 ? 2 : 1));
    if (rb_slots_cap() > 0) slots = std::min(slots, rb_slots_cap());
    const std::vector<RbLaunch>* ls = nullptr;
    if (int r = rb_tables(n, h, w, c, slots, &ls)) return r;
    if (c == 128) return dtype == Y4_BF16 ? resblock_run<Y4_BF16, 128>(k, *ls, stream) : resblock_run<Y4_F16, 128>(k, *ls, stream);
    return dtype == Y4_BF16 ? resblock_run<Y4_BF16, 64>(k, *ls, stream) : resblock_run<Y4_F16, 64>(k, *ls, stream);
}

int rb_tile_table(int n, int h, int w, int c, int slots, int32_t* out, int cap) {
    Y4_REQUIRE(n > 0 && h > 0 && w > 0 && (c == 128 || c == 64) && slots >= 8 && slots % 8 == 0 && slots <= 4096 &&
                   (int64_t)n * ((h + 3) / 4) * ((w + 15) / 16) < (1 << 22),
               Y4_EINVAL, "y4_rb_tile_table: bad shape (%d, %d, %d), channels %d or slots %d (a multiple of 8)", n, h, w, c, slots);
    RbTable t;
    rb_build_rows(n, h, w, c, slots, t);
    const int count = (int)t.v.size();
    if (out && cap >= count) std::copy(t.v.begin(), t.v.end(), out);
    return count;
}

// ------------------------------------------------------------------------------------------------ weight packing
// w1 / w3: Darknet-order float32 kernels of the block's 1x1 and 3x3 convs (device); scale / shift: their folded BN
int pack_resblock(int dtype, int c, const float* w1, const float* scale1, const float* shift1, const float* w3, const float* scale3,
                  const float* shift3, void* blob, hipStream_t stream) {
    Y4_REQUIRE(resblock_supported(dtype, c) && w1 && w3 && scale1 && shift1 && scale3 && shift3 && blob, Y4_EINVAL, "pack_resblock: bad argument");
    const int w1_bytes = c * c * 2, aff_pad = (4 * c * 4 + 1023) / 1024 * 1024;
    char* b = (char*)blob;                           // [affine | W1 fragments | W3 fragments]: pack_frag16's layout (conv_igemm.hip)
    if (int r = pack_frag16(dtype, c, c, 1, w1, b + aff_pad, stream)) return r;
    if (int r = pack_frag16(dtype, c, c, 3, w3, b + aff_pad + w1_bytes, stream)) return r;
    return copy_affine(c, {scale1, shift1, scale3, shift3}, (float*)b, stream);
}

}  // namespace y4
