// Depthwise 3x3 convolution for gfx950 (CDNA4), NHWC bf16: forward, input
// gradient and weight gradient for groups == C == K (one filter per
// channel), padding 1, stride 1 or 2, any C % 8 == 0 (the depthwise convs of
// MobileNetV1).
//
// Why not conv_igemm or conv_grouped. A depthwise 3x3 does 9 MACs per output
// element and reduces over no channels: an MFMA tile has nothing to multiply.
// Forward and dgrad are streaming stencils, wgrad is a per-channel reduction
// over all pixels; all three are bound by bytes moved (an estimate: about 450
// VALU ops against 160 B per lane and output row in the forward, see
// profiles/conv_dw.md for what was measured). So the aim is: request every
// input byte from HBM about once, write the output once, keep the taps in
// registers.
//
// Unit of work. A lane owns 8 consecutive channels, so every global access is
// 16 B. The C/8 channel lanes are cut into equal slabs of at most 32 lanes
// (256 channels, 512 contiguous bytes per pixel); blockIdx.y is the slab, so
// C has no upper limit. `lps` lanes span a pixel and the 256 / lps pixel
// groups of a block take further pixels; where lps does not divide 256 the
// lanes past the last whole group idle (the rule of se_reduce_kernel). In
// its prologue a lane loads its 8 channels x 9 taps as they are stored,
// [C][9] bf16: 144 contiguous bytes, nine 16-B loads, widened to 72 fp32
// registers that live as long as the block (flipped for dgrad; a stride-2
// dgrad class keeps only its 1, 2 or 4 taps). No packed copy, no arena.
//
// Forward and dgrad: a register sliding window over rows, not an LDS tile.
// A pixel group owns a strip of TW output columns and walks down `th` output
// rows of it. It holds the NR source rows of one output row, NV = S*(TW-1) +
// NC vectors each, as packed bf16 (4 VGPRs per vector); per step it loads
// only the min(S, NR) rows that enter the window, one step ahead of their
// use, and shifts the rest. Every tap of every output then comes from
// registers.
//   stride 1 (fwd, dgrad): TW = 4, window 3 x 6 vectors = 72 VGPRs, 24 more
//     for the row in flight, 72 taps: 241 VGPRs, two waves per SIMD.
//     Column halo 6/4, row halo (th + 2)/th.
//   stride 2 fwd: TW = 2, window 3 x 5 vectors = 60 VGPRs, 40 in flight; two
//     of three rows are new at every step, one is reused. TW = 4 would need
//     3 x 9 vectors and 72 VGPRs in flight.
//   stride 2 dgrad: one parity class (h%2, w%2) per blockIdx.z, a stride-1
//     stencil on dy with 1/2/2/4 taps and a 1..2 x 4..5 window. Every dx
//     element belongs to one class and every class has a tap, so dx is
//     written exactly once and nothing is zeroed beforehand; odd extents
//     give unequal classes, the blocks past a smaller class's units return.
// The halo columns a strip shares with its neighbours are requested twice,
// but the neighbour is the next pixel group of the same block (units are
// numbered strips-innermost), so the second request is served by the CU's
// vector cache, not by HBM. An LDS halo tile (16-B global_load_lds as in
// conv_grouped.hip) would save those requests but adds an LDS write and nine
// LDS reads per input vector, a barrier pair per tile, and a channel-lane to
// LDS-slot map that has to stay conflict-free for every lps from 1 to 32;
// conv_grouped.hip needs the tile because an MFMA fragment gathers channels
// of 16 pixels across lanes, and here no lane ever reads another lane's
// channels. The forward and dgrad kernels therefore use no LDS and no
// barrier.
// Out-of-image taps read a 16-B zero page and contribute a zero vector. The nine
// products are accumulated at fp32 in fixed (r, s) order with fused
// multiply-adds, rounded to bf16 once and stored as 16 B.
//
// Weight gradient. dw[c][r][s] = sum over (n, p, q) of dy[n,p,q,c] *
// x[n, p*s+r-1, q*s+s-1, c]. A lane holds 72 fp32 accumulators. A unit is one
// (image, output row); a block takes a chunk of `upc` consecutive units and
// one channel slab, its pixel group g the units g, g + G, ... of the chunk.
// Along its row a group slides a 3 x 3 window of x vectors (36 VGPRs), S new
// columns and one dy vector per pixel, loaded one pixel ahead. The x rows a
// group shares with the groups of the rows above and below run in the same
// block at the same time. At the end the groups fold through LDS in
// ascending order, one tap per pass (256 lanes x 8 floats = 8 KiB; a lane
// writes and reads 32 contiguous bytes, two ds b128 accesses, so a pass has
// no bank conflict beyond the width of the access), and group 0 stores the
// block's result once into slab[chunk][C][9]; wgrad_slab_fold_kernel sums
// the slabs in chunk order. One chunk writes the result directly. No
// atomics, nothing pre-zeroed, the same bits on every run.
//
// Constraints (bindings): C == K == groups, C % 8 == 0, 3x3, padding 1,
// stride 1|2.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// Scalar-lane fp32 VALU ops only (no packed fp32 forms), like the other
// kernel files added after the BN set.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

constexpr int DW_THREADS = 256;
constexpr int DW_SLAB_LANES = 32;   // channel lanes per slab at most
constexpr int DW_CUS = 256;

constexpr int DW_FWD = 0, DW_DGRAD1 = 1, DW_DGRAD2 = 2;

// A 16-B load that is always issued: outside the image it reads a zero page,
// so the window code has no branch around its loads.
__device__ __align__(16) static const unsigned short dw_zero16[8] = {0};

__device__ __forceinline__ uint4 dw_ld(const unsigned short* p, bool ok) {
    return *(const uint4*)(ok ? p : dw_zero16);
}

// Helpers of this file's own: under the target attribute above the HIP
// header functions (__uint_as_float, __syncthreads) would stay calls.
__device__ __forceinline__ float dw_bits_f32(unsigned u) {
    return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ void dw_unpack(const uint4& raw, float (&f)[8]) {
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = dw_bits_f32(w[i] << 16);
        f[2 * i + 1] = dw_bits_f32(w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ void dw_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The lane's taps as stored, [8 channels][9 taps] bf16 in nine 16-B loads:
// element e = ch * 9 + tap.
struct DwTaps {
    unsigned wd[36];
    __device__ __forceinline__ void load(const unsigned short* w, long c8) {
        const uint4* p = (const uint4*)(w + c8 * 72);
        #pragma unroll
        for (int i = 0; i < 9; ++i) {
            const uint4 q = p[i];
            wd[4 * i] = q.x;  wd[4 * i + 1] = q.y;
            wd[4 * i + 2] = q.z;  wd[4 * i + 3] = q.w;
        }
    }
    __device__ __forceinline__ float at(int ch, int tap) const {
        const int e = ch * 9 + tap;
        const unsigned v = wd[e >> 1];
        return dw_bits_f32((e & 1) ? (v & 0xffff0000u) : (v << 16));
    }
};

// Geometry of one fwd / dgrad launch. Source image SH x SW, output OH x OW
// (forward: x -> y; dgrad: dy -> dx), C channels on both sides. th: output
// rows per unit (of a parity class for the stride-2 dgrad).
struct DwArgs {
    const unsigned short* src;
    const unsigned short* w;
    unsigned short* out;
    int N, SH, SW, OH, OW, C, lps, th;
};

// out[oh][ow] = sum over i < NR, j < NC of
//   src[oh*S + R0 + i][ow*S + R0 + j] * w[tap(i, j)]
// on the OHc x OWc outputs (oh*OS + PA, ow*OS + PB) of the output image.
template <int MODE, int S, int PA, int PB>
__device__ __forceinline__ void dw_body(const DwArgs& a) {
    constexpr int NR = MODE == DW_DGRAD2 ? 1 + PA : 3;
    constexpr int NC = MODE == DW_DGRAD2 ? 1 + PB : 3;
    constexpr int R0 = MODE == DW_DGRAD2 ? 0 : -1;
    constexpr int OS = MODE == DW_DGRAD2 ? 2 : 1;
    constexpr int TW = S == 1 ? 4 : 2;
    constexpr int NV = S * (TW - 1) + NC;
    constexpr int NN = S < NR ? S : NR;       // rows entering per step

    const int lps = a.lps, G = DW_THREADS / lps;
    const int pg = threadIdx.x / lps, cl = threadIdx.x - pg * lps;
    const long c8 = (long)blockIdx.y * lps + cl;
    const int OHc = (a.OH - PA + OS - 1) / OS, OWc = (a.OW - PB + OS - 1) / OS;
    const int strips = (OWc + TW - 1) / TW, segs = (OHc + a.th - 1) / a.th;
    const long units = (long)a.N * segs * strips;
    const long unit = (long)blockIdx.x * G + pg;
    if (pg >= G || c8 * 8 >= a.C || unit >= units) return;

    // ---- prologue: the lane's taps, in the order the stencil reads them ---
    float wf[NR][NC][8];
    {
        DwTaps t;
        t.load(a.w, c8);
        #pragma unroll
        for (int i = 0; i < NR; ++i)
            #pragma unroll
            for (int j = 0; j < NC; ++j) {
                // dgrad at stride 2: even h takes r = 1 at p = hh; odd h
                // takes r = 2 at p = hh and r = 0 at p = hh + 1
                const int r = MODE == DW_FWD ? i : MODE == DW_DGRAD1 ? 2 - i
                              : (PA == 0 ? 1 : 2 - 2 * i);
                const int s = MODE == DW_FWD ? j : MODE == DW_DGRAD1 ? 2 - j
                              : (PB == 0 ? 1 : 2 - 2 * j);
                #pragma unroll
                for (int e = 0; e < 8; ++e) wf[i][j][e] = t.at(e, r * 3 + s);
            }
    }

    const int strip = (int)(unit % strips);
    const long us = unit / strips;
    const int seg = (int)(us % segs), n = (int)(us / segs);
    const int oh0 = seg * a.th, oh1 = min(oh0 + a.th, OHc), ow0 = strip * TW;
    const unsigned short* sp = a.src + (long)n * a.SH * a.SW * a.C + c8 * 8;
    unsigned short* op = a.out + (long)n * a.OH * a.OW * a.C + c8 * 8;
    const int col0 = ow0 * S + R0;
    const int SH = a.SH, SW = a.SW, C = a.C;

    auto load_row = [=](int row, bool want, uint4 (&dst)[NV]) {
        const bool rok = want && (unsigned)row < (unsigned)SH;
        const unsigned short* rp = sp + (long)row * SW * C;
        #pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = col0 + k;
            dst[k] = dw_ld(rp + (long)col * C,
                           rok && (unsigned)col < (unsigned)SW);
        }
    };

    uint4 win[NR][NV];
    #pragma unroll
    for (int i = 0; i < NR; ++i) load_row(oh0 * S + R0 + i, true, win[i]);

    for (int oh = oh0; oh < oh1; ++oh) {
        // the rows that enter the window at the next step, in flight while
        // this step computes
        uint4 nxt[NN][NV];
        #pragma unroll
        for (int k = 0; k < NN; ++k) {
            load_row((oh + 1) * S + R0 + NR - NN + k, oh + 1 < oh1, nxt[k]);
        }
        #pragma unroll
        for (int t = 0; t < TW; ++t) {
            const int ow = ow0 + t;
            if (ow >= OWc) break;
            float acc[8];
            #pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            #pragma unroll
            for (int i = 0; i < NR; ++i)
                #pragma unroll
                for (int j = 0; j < NC; ++j) {
                    float xf[8];
                    dw_unpack(win[i][t * S + j], xf);
                    #pragma unroll
                    for (int e = 0; e < 8; ++e)
                        acc[e] = __builtin_fmaf(xf[e], wf[i][j][e], acc[e]);
                }
            uint4 o;
            o.x = (unsigned)f32_to_bf16bits(acc[0]) |
                  ((unsigned)f32_to_bf16bits(acc[1]) << 16);
            o.y = (unsigned)f32_to_bf16bits(acc[2]) |
                  ((unsigned)f32_to_bf16bits(acc[3]) << 16);
            o.z = (unsigned)f32_to_bf16bits(acc[4]) |
                  ((unsigned)f32_to_bf16bits(acc[5]) << 16);
            o.w = (unsigned)f32_to_bf16bits(acc[6]) |
                  ((unsigned)f32_to_bf16bits(acc[7]) << 16);
            *(uint4*)(op + ((long)(oh * OS + PA) * a.OW + ow * OS + PB) *
                               a.C) = o;
        }
        #pragma unroll
        for (int i = 0; i + NN < NR; ++i)
            #pragma unroll
            for (int v = 0; v < NV; ++v) win[i][v] = win[i + NN][v];
        #pragma unroll
        for (int k = 0; k < NN; ++k)
            #pragma unroll
            for (int v = 0; v < NV; ++v) win[NR - NN + k][v] = nxt[k][v];
    }
}

template <int MODE, int S>
__global__ __launch_bounds__(DW_THREADS)
void conv_dw_kernel(const DwArgs a) {
    if constexpr (MODE != DW_DGRAD2) {
        dw_body<MODE, S, 0, 0>(a);
    } else {
        if (blockIdx.z == 0) dw_body<MODE, 1, 0, 0>(a);
        else if (blockIdx.z == 1) dw_body<MODE, 1, 0, 1>(a);
        else if (blockIdx.z == 2) dw_body<MODE, 1, 1, 0>(a);
        else dw_body<MODE, 1, 1, 1>(a);
    }
}

// ---- plan -----------------------------------------------------------------
// Channel slabs: the C/8 channel lanes in the fewest equal slabs of at most
// 32. fwd / dgrad: strips of 4 output columns (2 for the stride-2 forward)
// walked th rows down; th starts at the whole extent (no row halo) and is
// halved, not below 4 rows (row halo 1.5), while the grid has fewer than four
// blocks per CU. wgrad: about four blocks per CU, but no chunk with fewer
// units than the block has pixel groups or with fewer than 128 pixels: a
// block reads 32 B per lane and pixel (8 channels of x and of dy) and its
// slab costs 288 B per lane to store and 288 B to fold, so from there on the
// slabs add under a seventh to the traffic.
ConvDwPlan conv_dw_plan(int N, int H, int W, int C, int stride, int mode) {
    ConvDwPlan p;
    const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
    const int c8 = C / 8;
    p.nslab = (c8 + DW_SLAB_LANES - 1) / DW_SLAB_LANES;
    p.lps = (c8 + p.nslab - 1) / p.nslab;
    p.groups = DW_THREADS / p.lps;
    p.classes = 1;
    if (mode == CONV_DW_WGRAD) {
        const long U = (long)N * P;
        long want = 4L * DW_CUS / p.nslab;   // chunks
        if (want < 1) want = 1;
        long upc = (U + want - 1) / want;
        const long umin = (128 + Q - 1) / Q;
        if (upc < umin) upc = umin;
        if (upc < p.groups) upc = p.groups;
        if (upc > U) upc = U;
        p.th = 1;
        p.tw = Q;
        p.upc = (int)upc;
        p.nch = (int)((U + upc - 1) / upc);
        p.blocks = (long)p.nch * p.nslab;
        return p;
    }
    int eh = P, ew = Q;
    p.tw = stride == 1 ? 4 : 2;
    if (mode == CONV_DW_DGRAD) {
        eh = (H + stride - 1) / stride;
        ew = (W + stride - 1) / stride;
        p.tw = 4;
        p.classes = stride * stride;
    }
    const long strips = (ew + p.tw - 1) / p.tw;
    auto blocks = [&](int th) {
        const long units = (long)N * ((eh + th - 1) / th) * strips;
        return (units + p.groups - 1) / p.groups * p.nslab * p.classes;
    };
    int th = eh;
    while (th > 4 && blocks(th) < 4L * DW_CUS) th = (th + 1) / 2;
    p.th = th;
    p.nch = 1;
    p.upc = p.groups;
    p.blocks = blocks(th);
    return p;
}

void conv_dw_launch(const void* src, const void* w, void* out,
                    const ConvGeom& g, ConvMode mode, hipStream_t stream) {
    const bool fwd = mode == CONV_FWD;
    const ConvDwPlan p = conv_dw_plan(g.N, g.H, g.W, g.C, g.sy,
                                      fwd ? CONV_DW_FWD : CONV_DW_DGRAD);
    DwArgs a;
    a.src = (const unsigned short*)src;
    a.w = (const unsigned short*)w;
    a.out = (unsigned short*)out;
    a.N = g.N;
    a.SH = fwd ? g.H : g.P;  a.SW = fwd ? g.W : g.Q;
    a.OH = fwd ? g.P : g.H;  a.OW = fwd ? g.Q : g.W;
    a.C = g.C;  a.lps = p.lps;  a.th = p.th;
    const dim3 grid((unsigned)(p.blocks / (p.nslab * p.classes)),
                    (unsigned)p.nslab, (unsigned)p.classes);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(DW_THREADS), 0, stream, a);
    };
    if (fwd) {
        if (g.sy == 1) launch(conv_dw_kernel<DW_FWD, 1>);
        else launch(conv_dw_kernel<DW_FWD, 2>);
    } else if (g.sy == 1) {
        launch(conv_dw_kernel<DW_DGRAD1, 1>);
    } else {
        launch(conv_dw_kernel<DW_DGRAD2, 1>);
    }
}

// ---- wgrad ----------------------------------------------------------------
struct DwWgradArgs {
    const unsigned short* dy;   // [N,P,Q,C]
    const unsigned short* x;    // [N,H,W,C]
    float* ws;                  // nch == 1: [C][9]; else [nch][C][9]
    int N, H, W, P, Q, C, lps, upc, nch;
};

template <int S>
__global__ __launch_bounds__(DW_THREADS)
void conv_dw_wgrad_kernel(const DwWgradArgs a) {
    constexpr int NK = S;   // x columns entering the window per pixel
    __shared__ __align__(16) float fold[DW_THREADS * 8];
    const int lps = a.lps, G = DW_THREADS / lps;
    const int pg = threadIdx.x / lps, cl = threadIdx.x - pg * lps;
    const long c8 = (long)blockIdx.y * lps + cl;
    const int chunk = blockIdx.x;
    const bool live = pg < G && c8 * 8 < a.C;

    float acc[9][8];
    #pragma unroll
    for (int t = 0; t < 9; ++t)
        #pragma unroll
        for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;

    if (live) {
        const long U = (long)a.N * a.P;
        const long u_end = min(U, ((long)chunk + 1) * a.upc);
        for (long u = (long)chunk * a.upc + pg; u < u_end; u += G) {
            const int n = (int)(u / a.P), p = (int)(u - (long)n * a.P);
            const unsigned short* xp = a.x + (long)n * a.H * a.W * a.C + c8 * 8;
            const unsigned short* dyp =
                a.dy + ((long)n * a.P + p) * a.Q * a.C + c8 * 8;
            const int h0 = p * S - 1, H = a.H, W = a.W, C = a.C;
            auto load_x = [=](int r, int col, bool want) {
                const int h = h0 + r;
                return dw_ld(xp + ((long)h * W + col) * C,
                             want && (unsigned)h < (unsigned)H &&
                                 (unsigned)col < (unsigned)W);
            };
            uint4 xw[3][3];
            #pragma unroll
            for (int r = 0; r < 3; ++r)
                #pragma unroll
                for (int j = 0; j < 3; ++j) xw[r][j] = load_x(r, j - 1, true);
            uint4 dyv = dw_ld(dyp, true);
            for (int q = 0; q < a.Q; ++q) {
                // the next pixel's operands, in flight during this one's FMAs
                const bool more = q + 1 < a.Q;
                uint4 nxt[3][NK];
                #pragma unroll
                for (int r = 0; r < 3; ++r)
                    #pragma unroll
                    for (int k = 0; k < NK; ++k)
                        nxt[r][k] = load_x(r, (q + 1) * S + 2 - NK + k, more);
                const uint4 dyn = dw_ld(dyp + (long)(q + 1) * a.C, more);
                float d[8];
                dw_unpack(dyv, d);
                #pragma unroll
                for (int r = 0; r < 3; ++r)
                    #pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        float xf[8];
                        dw_unpack(xw[r][j], xf);
                        #pragma unroll
                        for (int e = 0; e < 8; ++e)
                            acc[r * 3 + j][e] =
                                __builtin_fmaf(d[e], xf[e], acc[r * 3 + j][e]);
                    }
                #pragma unroll
                for (int r = 0; r < 3; ++r) {
                    #pragma unroll
                    for (int j = 0; j + NK < 3; ++j) xw[r][j] = xw[r][j + NK];
                    #pragma unroll
                    for (int k = 0; k < NK; ++k) xw[r][3 - NK + k] = nxt[r][k];
                }
                dyv = dyn;
            }
        }
    }

    // fold the pixel groups in ascending order, one tap per pass; group 0
    // stores channel c8*8 + e, tap t at [c][t]
    float* o = a.ws + (a.nch > 1 ? (long)chunk * a.C * 9 : 0) + c8 * 72;
    #pragma unroll
    for (int t = 0; t < 9; ++t) {
        #pragma unroll
        for (int e = 0; e < 8; ++e) fold[threadIdx.x * 8 + e] = acc[t][e];
        dw_barrier();
        if (live && pg == 0) {
            float s[8];
            #pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = 0.f;
            for (int gi = 0; gi < G; ++gi) {
                const float* f = fold + (gi * lps + cl) * 8;
                #pragma unroll
                for (int e = 0; e < 8; ++e) s[e] += f[e];
            }
            #pragma unroll
            for (int e = 0; e < 8; ++e) o[e * 9 + t] = s[e];
        }
        dw_barrier();
    }
}

void conv_dw_wgrad_launch(const void* dy, const void* x, float* ws,
                          const ConvGeom& g, hipStream_t stream) {
    const ConvDwPlan p =
        conv_dw_plan(g.N, g.H, g.W, g.C, g.sy, CONV_DW_WGRAD);
    DwWgradArgs a;
    a.dy = (const unsigned short*)dy;
    a.x = (const unsigned short*)x;
    a.ws = ws;
    a.N = g.N;  a.H = g.H;  a.W = g.W;  a.P = g.P;  a.Q = g.Q;
    a.C = g.C;  a.lps = p.lps;  a.upc = p.upc;  a.nch = p.nch;
    const dim3 grid((unsigned)p.nch, (unsigned)p.nslab);
    if (g.sy == 1)
        hipLaunchKernelGGL(conv_dw_wgrad_kernel<1>, grid, dim3(DW_THREADS), 0,
                           stream, a);
    else
        hipLaunchKernelGGL(conv_dw_wgrad_kernel<2>, grid, dim3(DW_THREADS), 0,
                           stream, a);
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
