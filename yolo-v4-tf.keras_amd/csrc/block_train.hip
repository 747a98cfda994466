// block_train.hip -- fine-tuning of the 3x3 convs in front of the heads (92 / 100 / 108; reference custom_layers.py yolov4_neck, the
// conv(x, 256 | 512 | 1024, 3) calls that feed the three detection convs): the loss gradient carried through the head conv and
// the LeakyReLU / frozen BatchNormalization of the block, and the 3x3 weight gradient as an implicit GEMM on the matrix pipes.
// See DESIGN.md 7e.
//
// Per scale, with U the block's input, A its output (the head conv's input), s = gamma / sqrt(var + eps) the folded BN scale,
// g the loss derivative w.r.t. the raw head (grad_common.h; never stored) and Wh the head conv's weights as the forward used them:
//     dA[p, c]        = sum_o g[p, o] Wh[o, c]
//     dZ[p, c]        = dA[p, c] * (A[p, c] > 0 ? 1 : 0.1) * s[c]
//     dK[co,ci,kh,kw] = sum_{n,y,x} dZ[n,y,x,co] U[n, y+kh-1, x+kw-1, ci]          ('same' zero padding)
//
// Loss scale S (a power of two; 1 on the unscaled entry): dZ is multiplied by S in float32 before its single rounding to the operand
// type, so that fp16 keeps what would otherwise round into its subnormals, and the ordered sum of the partials is multiplied by
// 1 / S.  Both are exact in float32.  A stored dZ that is inf / NaN raises bit 0 of the caller's overflow word, a non-finite sum
// bit 1: one integer atomicOr per workgroup at most, which is order-independent.
//
// Determinism rule of loss.hip: no floating-point atomics, every sum in an order fixed by the geometry.
//   dA   one thread per element: the three confidence terms in anchor order, then the cell's records in record order (a cell's
//        records are its anchors in ascending order), each record's logits in ascending order
//   dK   K = pixels is cut into slices (image, strip of R rows); a workgroup adds a contiguous range of slices in slice order into
//        its MFMA accumulators -- inside a slice row pair by row pair, left to right -- and writes one float32 partial;
//        block_wgrad_finish_kernel adds the partials in range order
#include <cmath>

#include "conv_common.h"
#include "grad_common.h"

namespace y4 {

namespace {

constexpr int DG_PIX = 16;                 // cells of a dgrad strip: at most 48 responsible lanes, whose sparse rows fit LDS
constexpr int DG_VEC = 8;                  // channels per thread and step
constexpr int WG_TILE = 64;                // a wgrad workgroup owns 64 output x 64 input channels, all nine taps
constexpr int WG_TARGET = 512;             // workgroups a wgrad launch aims at (2 per compute unit)

// does a 16-byte chunk as Elem<DT>::store_chunk wrote it hold an inf or a NaN?
template <int DT>
__device__ __forceinline__ bool chunk_not_finite(const u32x4& c) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (DT == Y4_F32) {
            bad |= (c[i] & 0x7fffffffu) >= 0x7f800000u;
        } else {
            constexpr uint32_t EXP = DT == Y4_F16 ? 0x7c00u : 0x7f80u;
            bad |= (c[i] & 0x7fffu) >= EXP || ((c[i] >> 16) & 0x7fffu) >= EXP;
        }
    }
    return bad;
}

// ---- head dgrad + activation backward: grid (strips of DG_PIX cells of one image, images)
template <int DT>
__global__ __launch_bounds__(LOSS_THREADS) void block_dgrad_kernel(GradK p, BlockK b) {
    using E = Elem<DT>;
    using T = typename E::type;
    extern __shared__ float s_sp[];                                       // [DG_PIX * 3 lanes][5 + C]: the sparse rows' gradient
    __shared__ TrueBoxes tb;
    __shared__ int s_resp[LOSS_THREADS];
    __shared__ float s_g[DG_PIX * 3];
    const int img = blockIdx.y, strip = blockIdx.x, tid = threadIdx.x;
    const int s = strip >= b.dstrip_base[2] ? 2 : (strip >= b.dstrip_base[1] ? 1 : 0);
    const int cell0 = (strip - b.dstrip_base[s]) * DG_PIX;
    const int gh = p.gh[s], gw = p.gw[s], cells = gh * gw, nf = p.C + 5;
    const int nb = load_true_boxes(p, img, tb);
    s_resp[tid] = -1;
    __syncthreads();
    map_records(p, img, s, cell0 * 3, DG_PIX * 3, s_resp);
    __syncthreads();
    const float wimg = p.imgw[img];
    if (tid < DG_PIX * 3) {
        const int cell = cell0 + tid / 3, a = tid % 3;
        float g = 0.0f;
        if (cell < cells) {
            const int row = cell / gw, col = cell - row * gw;
            const float* t = p.head[s] + ((size_t)img * cells + cell) * p.hcs + a * nf;
            g = wimg * conf_grad(p, tb, nb, decode_lane(p, s, a, row, col, t), t[4], s_resp[tid] >= 0);
        }
        s_g[tid] = g;
    }
    for (int idx = tid; idx < DG_PIX * 3 * nf; idx += LOSS_THREADS) {
        const int lane = idx / nf, j = idx - lane * nf;
        const int ri = s_resp[lane];
        float g = 0.0f;
        if (ri >= 0 && j != 4) {
            const int cell = cell0 + lane / 3, a = lane % 3;
            const int row = cell / gw, col = cell - row * gw;
            const float* t = p.head[s] + ((size_t)img * cells + cell) * p.hcs + a * nf;
            const int32_t* r = p.records + ((size_t)img * p.mb + ri) * p.rw;
            if (j < 4) {
                float g4[4];
                box_grad(p, s, decode_lane(p, s, a, row, col, t), r, g4);
                g = g4[j];
            } else {
                g = class_grad(r, j - 5, t[j]);
            }
            g = wimg * g;
        }
        s_sp[idx] = g;
    }
    __syncthreads();
    const int cout = b.cout[s], vpc = cout / DG_VEC;
    const T* wh = (const T*)b.wh[s];                                       // head weights [3 (5 + C) rows][cout], as packed
    const T* act = (const T*)b.a[s] + ((size_t)img * cells + cell0) * cout;
    T* dz = (T*)b.dz[s] + ((size_t)img * cells + cell0) * cout;
    const float* sc = b.bn_scale[s];
    int bad = 0;
    for (int v = tid; v < DG_PIX * vpc; v += LOSS_THREADS) {
        const int cl = v / vpc, c = (v - cl * vpc) * DG_VEC;
        if (cell0 + cl >= cells) break;                                   // (v ascends: every later one is outside too)
        float acc[DG_VEC], w[DG_VEC];
#pragma unroll
        for (int k = 0; k < DG_VEC; ++k) acc[k] = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float g = s_g[cl * 3 + a];
#pragma unroll
            for (int q = 0; q < DG_VEC / E::EPC; ++q) E::load_chunk(wh + (size_t)(a * nf + 4) * cout + c + q * E::EPC, w + q * E::EPC);
#pragma unroll
            for (int k = 0; k < DG_VEC; ++k) acc[k] = fmaf(g, w[k], acc[k]);
        }
        for (int a = 0; a < 3; ++a) {
            if (s_resp[cl * 3 + a] < 0) continue;
            for (int j = 0; j < nf; ++j) {
                if (j == 4) continue;
                const float g = s_sp[(cl * 3 + a) * nf + j];
#pragma unroll
                for (int q = 0; q < DG_VEC / E::EPC; ++q) E::load_chunk(wh + (size_t)(a * nf + j) * cout + c + q * E::EPC, w + q * E::EPC);
#pragma unroll
                for (int k = 0; k < DG_VEC; ++k) acc[k] = fmaf(g, w[k], acc[k]);
            }
        }
        float av[DG_VEC];
#pragma unroll
        for (int q = 0; q < DG_VEC / E::EPC; ++q) E::load_chunk(act + (size_t)cl * cout + c + q * E::EPC, av + q * E::EPC);
#pragma unroll
        for (int k = 0; k < DG_VEC; ++k) acc[k] = acc[k] * (av[k] > 0.0f ? 1.0f : 0.1f) * sc[c + k] * b.loss_scale;
#pragma unroll
        for (int q = 0; q < DG_VEC / E::EPC; ++q) {
            u32x4 pk;
            E::store_chunk(&pk, acc + q * E::EPC);
            bad |= chunk_not_finite<DT>(pk);
            *(u32x4*)(dz + (size_t)cl * cout + c + q * E::EPC) = pk;
        }
    }
    // (the break above leaves the loop, not the kernel: every thread votes)
    if (__syncthreads_or(bad) && tid == 0 && b.overflow) atomicOr(b.overflow, 1);
}

// ---- the 3x3 weight gradient: grid (cin / 64, cout / 64, K splits), 4 waves; wave (wm, wn) owns 32 output x 32 input channels.
// LDS holds both operands of a slice TRANSPOSED, [channel][row][column], so that the K axis (pixels) is the contiguous one:
//     uT  [64 ci][R + 2 halo rows][upitch]     column xh = x + 1 (x = -1 .. ), zero outside the image
//     dT  [64 co][R rows][Wp]                  zero beyond the image's rows / columns
// 16-bit (bf16 and fp16 alike: the staging only moves bits): a k-step of v_mfma_f32_32x32x16 is 8 columns of two rows (lane half
// h takes row 2q + h); the B operand of tap (kh, kw) is the 16-byte row read at column x0 shifted by kw elements in registers
// (one extra dword), so nine taps cost three wide LDS reads.  float32: a k-step of v_mfma_f32_32x32x2_f32 is one column of two rows, operands are single dwords.
template <int DT>
__global__ __launch_bounds__(256) void block_wgrad_kernel(WgradK p) {
    using T = typename Elem<DT>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char wg_smem[];
    T* uT = (T*)wg_smem;
    T* dT = uT + (size_t)WG_TILE * p.uchan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const int ci0 = blockIdx.x * WG_TILE, co0 = blockIdx.y * WG_TILE, split = blockIdx.z;
    const int s0 = (int)((int64_t)split * p.slices / p.splits), s1 = (int)((int64_t)(split + 1) * p.slices / p.splits);
    const T* U = (const T*)p.u;
    const T* DZ = (const T*)p.dz;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[t][j] = 0.0f;
    for (int sl = s0; sl < s1; ++sl) {
        const int img = sl / p.strips, y0 = (sl - img * p.strips) * p.R;
        __syncthreads();                                                  // the previous slice's reads are done
        if constexpr (DT == Y4_F32) {
            const int items = (p.R + 2) * p.upitch * 16;
            for (int it = tid; it < items; it += 256) {
                const int cv = it & 15, pp = it >> 4, hr = pp / p.upitch, xh = pp - hr * p.upitch;
                const int y = y0 - 1 + hr, x = xh - 1;
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (y >= 0 && y < p.H && x >= 0 && x < p.W) v = *(const f32x4*)(U + (((size_t)img * p.H + y) * p.W + x) * p.cin + ci0 + cv * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) uT[(cv * 4 + i) * p.uchan + pp] = v[i];
            }
            const int ditems = p.R * p.Wp * 16;
            for (int it = tid; it < ditems; it += 256) {
                const int cv = it & 15, pp = it >> 4, hr = pp / p.Wp, x = pp - hr * p.Wp;
                const int y = y0 + hr;
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (y < p.H && x < p.W) v = *(const f32x4*)(DZ + (((size_t)img * p.H + y) * p.W + x) * p.cout + co0 + cv * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) dT[(cv * 4 + i) * p.dchan + pp] = v[i];
            }
        } else {
            // two neighbouring columns per thread: every LDS store is a full dword
            uint32_t* uT32 = (uint32_t*)uT;
            uint32_t* dT32 = (uint32_t*)dT;
            const int hp = p.upitch / 2, items = (p.R + 2) * hp * 8;
            for (int it = tid; it < items; it += 256) {
                const int cv = it & 7, pp = it >> 3, hr = pp / hp, xh = (pp - hr * hp) * 2;
                const int y = y0 - 1 + hr, x = xh - 1;
                u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                if (y >= 0 && y < p.H) {
                    const T* row = U + (((size_t)img * p.H + y) * p.W) * p.cin + ci0 + cv * 8;
                    if (x >= 0 && x < p.W) v0 = *(const u32x4*)(row + (size_t)x * p.cin);
                    if (x + 1 < p.W) v1 = *(const u32x4*)(row + (size_t)(x + 1) * p.cin);
                }
                const int base = (hr * p.upitch + xh) / 2;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uT32[(cv * 8 + 2 * i) * (p.uchan / 2) + base] = (v0[i] & 0xffffu) | (v1[i] << 16);
                    uT32[(cv * 8 + 2 * i + 1) * (p.uchan / 2) + base] = (v0[i] >> 16) | (v1[i] & 0xffff0000u);
                }
            }
            const int dhp = p.Wp / 2, ditems = p.R * dhp * 8;
            for (int it = tid; it < ditems; it += 256) {
                const int cv = it & 7, pp = it >> 3, hr = pp / dhp, x = (pp - hr * dhp) * 2;
                const int y = y0 + hr;
                u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                if (y < p.H) {
                    const T* row = DZ + (((size_t)img * p.H + y) * p.W) * p.cout + co0 + cv * 8;
                    if (x < p.W) v0 = *(const u32x4*)(row + (size_t)x * p.cout);
                    if (x + 1 < p.W) v1 = *(const u32x4*)(row + (size_t)(x + 1) * p.cout);
                }
                const int base = (hr * p.Wp + x) / 2;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dT32[(cv * 8 + 2 * i) * (p.dchan / 2) + base] = (v0[i] & 0xffffu) | (v1[i] << 16);
                    dT32[(cv * 8 + 2 * i + 1) * (p.dchan / 2) + base] = (v0[i] >> 16) | (v1[i] & 0xffff0000u);
                }
            }
        }
        __syncthreads();
        const T* da = dT + (size_t)(wm * 32 + r) * p.dchan;
        const T* ub = uT + (size_t)(wn * 32 + r) * p.uchan;
        for (int q = 0; q < p.R / 2; ++q) {
            const int yl = 2 * q + h;
            if constexpr (DT == Y4_F32) {
                for (int x = 0; x < p.W; ++x) {
                    const float a = da[yl * p.Wp + x];
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
                            acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ub[(yl + kh) * p.upitch + x + kw], acc[kh * 3 + kw], 0, 0, 0);
                }
            } else {
                for (int x0 = 0; x0 < p.Wp; x0 += 8) {
                    const u32x4 a = *(const u32x4*)(da + yl * p.Wp + x0);
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh) {
                        const T* row = ub + (yl + kh) * p.upitch + x0;
                        const u32x4 c = *(const u32x4*)row;
                        const uint32_t c4 = *(const uint32_t*)(row + 8);
                        const u32x4 b1 = {(c[0] >> 16) | (c[1] << 16), (c[1] >> 16) | (c[2] << 16), (c[2] >> 16) | (c[3] << 16), (c[3] >> 16) | (c4 << 16)};
                        const u32x4 b2 = {c[1], c[2], c[3], c4};
                        Mma32<DT>::run(acc[kh * 3 + 0], a, c);
                        Mma32<DT>::run(acc[kh * 3 + 1], a, b1);
                        Mma32<DT>::run(acc[kh * 3 + 2], a, b2);
                    }
                }
            }
        }
    }
    // accumulator register j of lane (r, h): row (j & 3) + 8 (j >> 2) + 4 h of the 32 output channels, column r of the input channels
    const size_t plane = (size_t)p.cout * p.cin;
    float* o = p.part + (size_t)split * 9 * plane + (size_t)(co0 + wm * 32 + 4 * h) * p.cin + ci0 + wn * 32 + r;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 16; ++j) o[t * plane + (size_t)((j & 3) + 8 * (j >> 2)) * p.cin] = acc[t][j];
}

// partials [splits][9 taps][cout][cin] -> dK [cout][cin][3][3] (the Darknet stream's order), added in split order, then unscaled
__global__ __launch_bounds__(256) void block_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ dk, int cout, int cin,
                                                                 int splits, int accumulate, float inv_scale, int32_t* overflow) {
    const size_t plane = (size_t)cout * cin, total = 9 * plane;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (e < total) {
        const int t = (int)(e / plane);
        const size_t oc = e - (size_t)t * plane;
        float acc = 0.0f;
        for (int s = 0; s < splits; ++s) acc += part[(size_t)s * total + e];
        acc *= inv_scale;
        bad = (__float_as_uint(acc) & 0x7fffffffu) >= 0x7f800000u;
        float* o = dk + oc * 9 + t;
        *o = accumulate ? *o + acc : acc;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0 && overflow) atomicOr(overflow, 2);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

int block_dgrad_strips(const int* gh, const int* gw, int* base) {
    int total = 0;
    for (int i = 0; i < 3; ++i) {
        if (base) base[i] = total;
        total += (gh[i] * gw[i] + DG_PIX - 1) / DG_PIX;
    }
    return total;
}

// the wgrad geometry of one layer for n images of H x W cells: rows per slice, LDS pitches, K splits -> LDS bytes.  0: two rows
// of the grid with their halo do not fit 160 KB of LDS -- a row of more than 105 cells (float32) or 200 cells (bf16), which is an
// image wider than 840 / 1600 pixels at the stride-8 scale (fp16 as bf16)
size_t block_wgrad_geometry(int dtype, int n, int H, int W, int cin, int cout, WgradK& k) {
    const int es = elem_size(dtype);
    k.n = n; k.H = H; k.W = W; k.cin = cin; k.cout = cout;
    size_t lds = 0;
    for (int R = W >= 64 ? 2 : 4; R >= 2; R -= 2) {
        k.R = R;
        if (dtype == Y4_F32) {
            k.Wp = W; k.upitch = W + 2;
            k.uchan = ((R + 2) * k.upitch) | 1;                          // odd dword pitch: 32 channels read 32 banks
            k.dchan = (R * k.Wp) | 1;
        } else {
            k.Wp = (int)round_up(W, 8); k.upitch = k.Wp + 8;
            k.uchan = (R + 2) * k.upitch; if ((k.uchan / 8) % 2 == 0) k.uchan += 8;      // an odd number of 16-byte units
            k.dchan = R * k.Wp; if ((k.dchan / 8) % 2 == 0) k.dchan += 8;
        }
        lds = (size_t)WG_TILE * ((size_t)k.uchan + k.dchan) * es;
        if (lds <= 64 * 1024) break;
    }
    if (lds > 160 * 1024) return 0;
    k.strips = (H + k.R - 1) / k.R;
    k.slices = n * k.strips;
    const int tiles = (cin / WG_TILE) * (cout / WG_TILE);
    k.splits = (WG_TARGET + tiles - 1) / tiles;
    if (k.splits > k.slices) k.splits = k.slices;
    if (k.splits < 1) k.splits = 1;
    return lds;
}

// -> bytes, 0 when a scale's geometry is unsupported
size_t block_grad_scratch_bytes(int dtype, int n, const int* gh, const int* gw, const int* cin, const int* cout, size_t* dz_off,
                                size_t* part_off) {
    size_t off = 0;
    for (int i = 0; i < 3; ++i) {
        if (dz_off) dz_off[i] = off;
        off = align256(off + (size_t)n * gh[i] * gw[i] * cout[i] * elem_size(dtype));
    }
    for (int i = 0; i < 3; ++i) {
        WgradK k{};
        if (!block_wgrad_geometry(dtype, n, gh[i], gw[i], cin[i], cout[i], k)) return 0;
        if (part_off) part_off[i] = off;
        off = align256(off + (size_t)k.splits * 9 * cout[i] * cin[i] * sizeof(float));
    }
    return off;
}

template <int DT>
static int block_grad_launch_t(const GradK& k, const BlockK& b, int n, hipStream_t stream) {
    WgradK w[3]{};
    size_t lds[3];
    for (int s = 0; s < 3; ++s) {                                         // every check before the first launch
        lds[s] = block_wgrad_geometry(DT, n, k.gh[s], k.gw[s], b.cin[s], b.cout[s], w[s]);
        Y4_REQUIRE(lds[s] > 0, Y4_EINVAL, "block gradient: a grid row of %d cells does not fit the LDS tile", k.gw[s]);
        w[s].u = b.u[s]; w[s].dz = b.dz[s]; w[s].part = b.part[s];
    }
    const int nstrips = block_dgrad_strips(k.gh, k.gw, nullptr);
    const size_t sp_bytes = (size_t)DG_PIX * 3 * (k.C + 5) * sizeof(float);
    hipLaunchKernelGGL(block_dgrad_kernel<DT>, dim3(nstrips, n), dim3(LOSS_THREADS), sp_bytes, stream, k, b);
    for (int s = 0; s < 3; ++s) {
        if (int r = launch_lds<block_wgrad_kernel<DT>>(160 * 1024, dim3(w[s].cin / WG_TILE, w[s].cout / WG_TILE, w[s].splits), dim3(256), lds[s], stream, w[s])) return r;
        const size_t total = (size_t)9 * w[s].cout * w[s].cin;
        hipLaunchKernelGGL(block_wgrad_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float*)b.part[s],
                           b.dk + b.dk_off[s], w[s].cout, w[s].cin, w[s].splits, b.accumulate, 1.0f / b.loss_scale, b.overflow);
    }
    Y4_CHECK_HIP(hipGetLastError());
    return Y4_OK;
}

int block_grad_launch(int dtype, const GradK& k, const BlockK& b, int n, hipStream_t stream) {
    Y4_REQUIRE(k.mb >= 1 && k.mb <= LOSS_THREADS, Y4_EINVAL, "block gradient: max_boxes %d outside [1, %d]", k.mb, LOSS_THREADS);
    Y4_REQUIRE((size_t)DG_PIX * 3 * (k.C + 5) * sizeof(float) <= 48 * 1024, Y4_EINVAL, "block gradient: %d classes", k.C);
    int exp2 = 0;
    Y4_REQUIRE(std::isnormal(b.loss_scale) && b.loss_scale > 0.0f && std::frexp(b.loss_scale, &exp2) == 0.5f, Y4_EINVAL,
               "block gradient: loss scale %g is not a finite positive power of two", (double)b.loss_scale);
    for (int s = 0; s < 3; ++s)
        Y4_REQUIRE(b.cin[s] % WG_TILE == 0 && b.cout[s] % WG_TILE == 0 && (int64_t)n * k.gh[s] * k.gw[s] < (1ll << 31), Y4_EINVAL,
                   "block gradient: %d -> %d channels / %d images of scale %d", b.cin[s], b.cout[s], n, s);
    switch (dtype) {
        case Y4_F32: return block_grad_launch_t<Y4_F32>(k, b, n, stream);
        case Y4_BF16: return block_grad_launch_t<Y4_BF16>(k, b, n, stream);
        case Y4_F16: return block_grad_launch_t<Y4_F16>(k, b, n, stream);
        default: set_error("block gradient: dtype %d is not supported", dtype); return Y4_EINVAL;
    }
}

}  // namespace y4
