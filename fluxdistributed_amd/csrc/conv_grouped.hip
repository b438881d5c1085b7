// Grouped 3x3 convolution for gfx950 (CDNA4), NHWC bf16: forward, input
// gradient and weight gradient for groups with cpg = C/g = K/g in
// {4, 8, 16, 32} channels, padding 1, stride 1 or 2 (the 3x3 convs of the
// ResNeXt bottlenecks).
//
// Why not conv_igemm. With 4..32 input channels per output channel a grouped
// conv does 36..288 MACs per output element against about 4 bytes of
// traffic: by the instruction and bandwidth rates it is memory-bound by more
// than an order of magnitude (an estimate, see profiles/conv_grouped.md for
// what was measured). So the aim is: read the input once, write the output
// once, keep the weights in registers. No im2col row is ever built.
//
// Unit of work: a 16-channel output block. For cpg >= 16 it lies inside one
// group and reduces over that group's cpg input channels; for cpg < 16 the
// 16/cpg neighbouring groups are merged into one 16x16 block-diagonal weight
// block per tap, zeros off the diagonal. Either way it is one loop of
// v_mfma_f32_16x16x32_bf16 over G = max(cpg, 16) input channels x taps:
//   G = 32: one MFMA per tap (K = 32 input channels);
//   G = 16: one MFMA per PAIR of taps (lane groups fq = 0,1 carry tap 2j,
//           fq = 2,3 tap 2j+1), an odd tap count padded with a zero tap.
// The MFMA lanes wasted on the zeros at cpg 4 and 8 are deliberate.
//
// MFMA orientation (fr = lane & 15, fq = lane >> 4): the WEIGHTS are the row
// operand, A[i = output channel fr][k = fq*8 .. +7], the activations the
// column operand, B[k = fq*8 .. +7][j = pixel fr], so D[i = 4*fq + v][j = fr]
// leaves a lane with four consecutive output channels of one pixel: 8 B per
// lane in the epilogue, one bf16 round from the fp32 accumulator.
//
// Weights are read as stored, [K][3][3][cpg] (the channels_last weight). A
// wave owns one 16-block of a 64-channel slab; in its prologue it gathers
// the A fragments of every MFMA step (for dgrad: the group's block
// transposed and the taps flipped; for cpg < 16: zeros off the diagonal) and
// keeps them in registers, 4 VGPRs per step, 36 at most (cpg 32, 9 taps).
// There is no packed copy of the weight and nothing to register or cache.
//
// Forward and dgrad. A block of four waves owns a spatial tile x a
// 64-channel slab of one image and runs over `ipb` images with the same
// weights. Per image it stages the source tile with its halo into LDS once
// (16-B global_load_lds; pixels outside the image come from a 16-B zero
// page), 128 B per pixel. Each tap is then ONE 16-B LDS read per lane at a
// shifted pixel: 8 consecutive channels of a pixel are an MFMA B fragment as
// they lie. Halo extents: forward (s*(th-1) + 3) x (s*(tw-1) + 3); dgrad at
// stride 1 (th+2) x (tw+2) with the taps flipped; dgrad at stride 2 runs one
// parity class (h%2, w%2) per blockIdx.z, with 1/2/2/4 taps and a
// (th+1) x (tw+1) halo of dy. Every dx element belongs to exactly one class
// and every class has a tap, so dx is written once everywhere and nothing is
// zeroed beforehand.
//
// LDS layout and the bank argument. Tile position p (row-major over the halo
// tile) holds its pixel's eight 16-B channel granules; granule g sits in
// slot g ^ ((p >> 1) & 7) (source-side swizzle: the stager picks the source
// granule for each slot). With 64 banks x 4 B a 16-B unit's place modulo
// 256 B is (p & 1)*8 + slot. The 16 lanes of one fq read the same granule of
// 16 pixels; along a tile row those are 16 consecutive positions, and
// p -> (p & 1, (p >> 1) & 7) is a bijection of p mod 16, so the 16 units are
// distinct: conflict-free for every tap shift. At stride 2 the forward reads
// every other column, which would fold that onto 8 units; so the stride-2
// tile is stored with its columns de-interleaved (even columns, then odd
// columns, per row), and a tap again reads 16 consecutive positions. Not
// covered by the argument: a 16-pixel group that wraps to the next tile row
// (tw < 16) continues at a position that is not the next one modulo 16, and
// a hardware pass that mixes lanes of two fq. Neither has been
// counter-profiled.
//
// Weight gradient. Per 16-block and tap,
//   D[16 out][16 in] += dy^T[16][32 pixels] . x[32 pixels][16 in],
// the reduction running along pixels; both operands are [pixel][channel] in
// LDS, so ds_read_tr16_b64 serves the fragments: in a 16-lane group lane l
// reads 8 B (4 channels) of pixel l>>2 and receives 4 pixels of channel l.
// The x halo tile and the dy tile are staged once per spatial tile in the
// layout above and all 9 taps read them; x addresses of pixels past the
// tile's end point at a zero pixel kept behind the tile, their dy rows are
// staged as zeros. 9 x (G/16) accumulator tiles per wave, 36 or 72 VGPRs.
// A block takes a chunk of whole (image, tile) units; chunk c stores its
// result once into slab c ([nch][K][9*cpg] fp32) and wgrad_slab_fold_kernel
// sums the slabs in order: no atomics, no pre-zeroing, the same bits on
// every run. One chunk writes the result directly. For cpg < 16 only the
// diagonal sub-blocks are stored.
//
// Constraints (bindings): C == K, C % 64 == 0, 3x3, padding 1, stride 1|2.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// No packed fp32 VALU ops in this file (the MFMA is the only arithmetic).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

typedef __attribute__((ext_vector_type(8))) short cg_short8;
typedef __attribute__((ext_vector_type(4))) short cg_short4;
typedef __attribute__((ext_vector_type(4))) float cg_f32x4;

__device__ __align__(16) static const unsigned short cg_zero16[8] = {0};

#define FDA_CG_GLDS16(gptr, lptr)                                           \
    __builtin_amdgcn_global_load_lds(                                       \
        (const __attribute__((address_space(1))) void*)(gptr),              \
        (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

constexpr int CG_PIX = 64;      // bf16 per LDS pixel: one 64-channel slab
constexpr int CG_WAVES = 4;     // one 16-block each

// Halo tile of a (th x tw) output tile as it lies in LDS: lh rows of lwp
// positions. deint: each row holds its even columns, then (from hw) its odd
// columns.
struct CgLayout {
    int lh, lw, lwp, hw, nreal;
    bool deint;
};
__host__ __device__ __forceinline__ CgLayout cg_layout(int lh, int lw,
                                                       bool deint) {
    CgLayout L;
    L.lh = lh;
    L.lw = lw;
    L.hw = (lw + 1) / 2;
    L.lwp = deint ? 2 * L.hw : lw;
    L.nreal = lh * L.lwp;
    L.deint = deint;
    return L;
}
// forward / wgrad x tile: every pixel a 3x3 tap of the tile's outputs reads
__host__ __device__ __forceinline__ CgLayout cg_layout_x(int th, int tw,
                                                         int s) {
    return cg_layout(s * (th - 1) + 3, s * (tw - 1) + 3, s == 2);
}

// element offset of granule g of tile position pos
__device__ __forceinline__ int cg_lds_off(int pos, int g) {
    return pos * CG_PIX + ((g ^ ((pos >> 1) & 7)) << 3);
}

// Stage npos (a multiple of 8) tile positions, 8 per DMA: positions >=
// L.nreal and pixels outside the SH x SW image read the zero page. img: the
// image's first element of this channel slab; Cs: channels per pixel there.
__device__ __forceinline__ void cg_stage(const unsigned short* __restrict__ img,
                                         unsigned short* lds, int npos,
                                         const CgLayout& L, int row0,
                                         int col0, int SH, int SW, int Cs,
                                         int wid, int lane) {
    const int ndma = npos >> 3;
    for (int d = wid; d < ndma; d += CG_WAVES) {
        const int pos = d * 8 + (lane >> 3);
        const int row = pos / L.lwp, cp = pos - row * L.lwp;
        const int col = !L.deint ? cp
                        : (cp >= L.hw ? 2 * (cp - L.hw) + 1 : 2 * cp);
        const int gr = row0 + row, gc = col0 + col;
        const int g = (lane & 7) ^ ((pos >> 1) & 7);
        const bool ok = pos < L.nreal && (unsigned)gr < (unsigned)SH &&
                        (unsigned)gc < (unsigned)SW;
        const unsigned short* sp =
            ok ? img + ((long)gr * SW + gc) * Cs + g * 8 : cg_zero16;
        FDA_CG_GLDS16(sp, lds + d * 512);
    }
}

// Geometry of one fwd / dgrad launch. Source image SH x SW, output OH x OW
// (forward: x -> y; dgrad: dy -> dx), C channels on both sides.
struct CgArgs {
    const unsigned short* src;
    const unsigned short* w;
    unsigned short* out;
    int N, SH, SW, OH, OW, C, cpg, s, th, tw, tiles_w, tiles, ipb;
};

constexpr int CG_FWD = 0, CG_DGRAD1 = 1, CG_DGRAD2 = 2;

// NT taps; (pa, pb): the parity class of a stride-2 dgrad.
template <int G, int MODE, int NT>
__device__ __forceinline__ void cg_body(const CgArgs& a, int pa, int pb,
                                        unsigned short* lds) {
    constexpr int NS = (G == 32) ? NT : (NT + 1) / 2;   // MFMA steps
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int c0 = blockIdx.y * 64;
    const int kb = c0 + wid * 16;

    const int OHc = (MODE == CG_DGRAD2) ? (a.OH - pa + 1) / 2 : a.OH;
    const int OWc = (MODE == CG_DGRAD2) ? (a.OW - pb + 1) / 2 : a.OW;
    const int tile = blockIdx.x % a.tiles, nb = blockIdx.x / a.tiles;
    const int oh0 = (tile / a.tiles_w) * a.th;
    const int ow0 = (tile % a.tiles_w) * a.tw;
    if (oh0 >= OHc || ow0 >= OWc) return;   // a smaller class: whole block
    const int eth = min(a.th, OHc - oh0), etw = min(a.tw, OWc - ow0);
    const int npx = eth * etw;

    const CgLayout L = (MODE == CG_FWD)      ? cg_layout_x(a.th, a.tw, a.s)
                       : (MODE == CG_DGRAD1) ? cg_layout(a.th + 2, a.tw + 2, false)
                                             : cg_layout(a.th + 1, a.tw + 1, false);
    const int npos = (L.nreal + 7) & ~7;
    const int row0 = (MODE == CG_FWD) ? a.s * oh0 - 1
                     : (MODE == CG_DGRAD1) ? oh0 - 1 : oh0;
    const int col0 = (MODE == CG_FWD) ? a.s * ow0 - 1
                     : (MODE == CG_DGRAD1) ? ow0 - 1 : ow0;
    const int ps = (MODE == CG_FWD) ? a.s : 1;   // source rows per output row

    // ---- prologue: this lane's tap of every step, and its A fragment -----
    const int oc = kb + fr;                       // the lane's output channel
    const int rb = (G == 32) ? (kb & ~31) + fq * 8 : kb + (fq & 1) * 8;
    int delta[NS];
    cg_short8 wr[NS];
    #pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int t = (G == 32) ? j : 2 * j + (fq >> 1);
        const bool live = t < NT;
        const int tt = live ? t : 0;
        int dr, dc, wtap;
        if (MODE == CG_DGRAD2) {
            const int nS = pb + 1;
            const int ri = tt / nS, si = tt - ri * nS;
            // even h: r = 1 reads p = hh; odd h: r = 0 reads hh + 1, r = 2 hh
            const int r = pa == 0 ? 1 : 2 * ri;
            const int sc = pb == 0 ? 1 : 2 * si;
            dr = (pa == 1 && ri == 0) ? 1 : 0;
            dc = (pb == 1 && si == 0) ? 1 : 0;
            wtap = r * 3 + sc;
        } else {
            dr = tt / 3;
            dc = tt - dr * 3;
            wtap = (MODE == CG_FWD) ? tt : 8 - tt;
        }
        delta[j] = dr * L.lwp + (L.deint ? (dc & 1) * L.hw + (dc >> 1) : dc);
        cg_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            if (MODE == CG_FWD && a.cpg >= 8) {
                // 8 input channels aligned to 8 lie in one group
                if (rb / a.cpg == oc / a.cpg)
                    v = *(const cg_short8*)(a.w + ((long)oc * 9 + wtap) * a.cpg +
                                            rb % a.cpg);
            } else {
                #pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int rc = rb + e;
                    if (rc / a.cpg != oc / a.cpg) continue;
                    v[e] = (MODE == CG_FWD)
                        ? (short)a.w[((long)oc * 9 + wtap) * a.cpg + rc % a.cpg]
                        : (short)a.w[((long)rc * 9 + wtap) * a.cpg + oc % a.cpg];
                }
            }
        }
        wr[j] = v;
    }
    // granule of the 64-channel slab this lane reads
    const int gsel = (G == 32) ? (wid >> 1) * 4 + fq : wid * 2 + (fq & 1);

    const int n_end = min(a.N, (nb + 1) * a.ipb);
    for (int n = nb * a.ipb; n < n_end; ++n) {
        __syncthreads();   // the previous image's reads are done
        cg_stage(a.src + (long)n * a.SH * a.SW * a.C + c0, lds, npos, L, row0,
                 col0, a.SH, a.SW, a.C, wid, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int p16 = 0; p16 < npx; p16 += 16) {
            const int idx = p16 + fr;
            const bool valid = idx < npx;
            const int idc = valid ? idx : 0;
            const int ph = idc / etw, pw = idc - ph * etw;
            const int base = ps * ph * L.lwp + pw;
            cg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int pos = base + delta[j];
                const cg_short8 b =
                    *(const cg_short8*)(lds + cg_lds_off(pos, gsel));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[j], b, acc,
                                                              0, 0, 0);
            }
            if (!valid) continue;
            int h = oh0 + ph, wc = ow0 + pw;
            if (MODE == CG_DGRAD2) { h = 2 * h + pa; wc = 2 * wc + pb; }
            uint2 o;
            o.x = (unsigned)f32_to_bf16bits(acc[0]) |
                  ((unsigned)f32_to_bf16bits(acc[1]) << 16);
            o.y = (unsigned)f32_to_bf16bits(acc[2]) |
                  ((unsigned)f32_to_bf16bits(acc[3]) << 16);
            *(uint2*)(a.out + (((long)n * a.OH + h) * a.OW + wc) * a.C + kb +
                      4 * fq) = o;
        }
    }
}

template <int G, int MODE>
__global__ __launch_bounds__(CG_WAVES * 64)
void conv_grouped_kernel(const CgArgs a) {
    extern __shared__ __align__(16) unsigned short cg_lds[];
    if constexpr (MODE != CG_DGRAD2) {
        cg_body<G, MODE, 9>(a, 0, 0, cg_lds);
    } else {
        const int pa = blockIdx.z >> 1, pb = blockIdx.z & 1;
        if (pa + pb == 0) cg_body<G, MODE, 1>(a, pa, pb, cg_lds);
        else if (pa + pb == 1) cg_body<G, MODE, 2>(a, pa, pb, cg_lds);
        else cg_body<G, MODE, 4>(a, pa, pb, cg_lds);
    }
}

// ---- plan -----------------------------------------------------------------
// Tiles: the largest whose halo tile (and, for wgrad, dy tile) fit 48 KiB of
// LDS, so three blocks share a CU: 16x16 outputs (stride-1 fwd and dgrad, a
// parity class of the stride-2 dgrad), 8x8 (stride-2 fwd, whose halo is
// 17x17), 8x16 / 8x8 for wgrad. An extent is cut into equal tiles, not into
// full tiles and a remainder. fwd / dgrad: a block runs over ipb images so
// that its waves keep their weights for about 256 pixels, halved while the
// grid has fewer than four blocks per CU. wgrad: as many chunks as give
// every CU its three blocks, but no chunk under 9*cpg pixels: a block reads
// 256 B per pixel (64 channels of x and of dy) and stores a slab of
// 64 x 9*cpg floats, so from there on it stores no more than it reads. (A
// floor of 1024 pixels left the 7x7 and 14x14 shapes of ResNeXt-50 with 80
// blocks on 256 CUs and behind the library: profiles/conv_grouped.md.)
constexpr int CG_CUS = 256;

static int cg_cut(int extent, int tmax, int* ntiles) {
    *ntiles = (extent + tmax - 1) / tmax;
    return (extent + *ntiles - 1) / *ntiles;
}

ConvGroupedPlan conv_grouped_plan(int N, int H, int W, int C, int cpg,
                                  int stride, int mode) {
    ConvGroupedPlan p;
    const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
    int eh, ew, mh, mw;
    p.classes = 1;
    if (mode == CONV_GROUPED_WGRAD) {
        eh = P; ew = Q; mh = 8; mw = stride == 1 ? 16 : 8;
    } else if (mode == CONV_GROUPED_FWD) {
        eh = P; ew = Q; mh = mw = stride == 1 ? 16 : 8;
    } else {
        eh = (H + stride - 1) / stride; ew = (W + stride - 1) / stride;
        mh = mw = 16;
        p.classes = stride * stride;
    }
    p.th = cg_cut(eh, mh, &p.tiles_h);
    p.tw = cg_cut(ew, mw, &p.tiles_w);
    const int tiles = p.tiles_h * p.tiles_w, px = p.th * p.tw;
    const long slabs = C / 64;
    CgLayout L;
    if (mode == CONV_GROUPED_DGRAD)
        L = stride == 1 ? cg_layout(p.th + 2, p.tw + 2, false)
                        : cg_layout(p.th + 1, p.tw + 1, false);
    else
        L = cg_layout_x(p.th, p.tw, stride);
    if (mode == CONV_GROUPED_WGRAD) {
        const long U = (long)N * tiles;
        long nch = (long)CG_CUS * 3 / slabs;
        nch = nch < 1 ? 1 : (nch > U ? U : nch);
        long upc = (U + nch - 1) / nch;
        const long umin = (9 * cpg + px - 1) / px;
        if (upc < umin) upc = umin;
        p.upc = (int)upc;
        p.nch = (int)((U + upc - 1) / upc);
        p.ipb = 1;
        p.blocks = p.nch * slabs;
        // x tile + zero pixel, rounded to whole DMAs; dy tile in 32-pixel steps
        p.lds_bytes = (size_t)(((L.nreal + 1 + 7) & ~7) + ((px + 31) & ~31)) *
                      CG_PIX * 2;
        return p;
    }
    int ipb = 256 / px;
    ipb = ipb < 1 ? 1 : (ipb > N ? N : ipb);
    auto blocks = [&](int i) {
        return (long)tiles * ((N + i - 1) / i) * slabs * p.classes;
    };
    while (ipb > 1 && blocks(ipb) < 4 * CG_CUS) ipb /= 2;
    p.ipb = ipb;
    p.nch = 1;
    p.upc = 0;
    p.blocks = blocks(ipb);
    p.lds_bytes = (size_t)((L.nreal + 7) & ~7) * CG_PIX * 2;
    return p;
}

void conv_grouped_launch(const void* src, const void* w, void* out,
                         const ConvGeom& g, int cpg, ConvMode mode,
                         hipStream_t stream) {
    const bool fwd = mode == CONV_FWD;
    const ConvGroupedPlan p = conv_grouped_plan(
        g.N, g.H, g.W, g.C, cpg, g.sy,
        fwd ? CONV_GROUPED_FWD : CONV_GROUPED_DGRAD);
    CgArgs a;
    a.src = (const unsigned short*)src;
    a.w = (const unsigned short*)w;
    a.out = (unsigned short*)out;
    a.N = g.N;
    a.SH = fwd ? g.H : g.P;  a.SW = fwd ? g.W : g.Q;
    a.OH = fwd ? g.P : g.H;  a.OW = fwd ? g.Q : g.W;
    a.C = g.C;  a.cpg = cpg;  a.s = g.sy;
    a.th = p.th;  a.tw = p.tw;  a.tiles_w = p.tiles_w;
    a.tiles = p.tiles_h * p.tiles_w;  a.ipb = p.ipb;
    const dim3 grid((unsigned)(a.tiles * ((g.N + p.ipb - 1) / p.ipb)),
                    (unsigned)(g.C / 64), (unsigned)p.classes);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(CG_WAVES * 64), p.lds_bytes,
                           stream, a);
    };
    const bool g32 = cpg == 32;
    if (fwd) {
        if (g32) launch(conv_grouped_kernel<32, CG_FWD>);
        else launch(conv_grouped_kernel<16, CG_FWD>);
    } else if (g.sy == 1) {
        if (g32) launch(conv_grouped_kernel<32, CG_DGRAD1>);
        else launch(conv_grouped_kernel<16, CG_DGRAD1>);
    } else {
        if (g32) launch(conv_grouped_kernel<32, CG_DGRAD2>);
        else launch(conv_grouped_kernel<16, CG_DGRAD2>);
    }
}

// ---- wgrad ----------------------------------------------------------------
struct CgWgradArgs {
    const unsigned short* dy;   // [N,P,Q,C]
    const unsigned short* x;    // [N,H,W,C]
    float* ws;                  // nch == 1: [C][9*cpg]; else [nch][C][9*cpg]
    int N, H, W, P, Q, C, cpg, s, th, tw, tiles_w, tiles, upc, nch;
};

__device__ __forceinline__ cg_short4 cg_tr16(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) cg_short4*)(p));
}

template <int G>
__global__ __launch_bounds__(CG_WAVES * 64)
void conv_grouped_wgrad_kernel(const CgWgradArgs a) {
    constexpr int CT = G / 16;   // 16-wide input-channel tiles per block
    extern __shared__ __align__(16) unsigned short cg_lds[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = blockIdx.x;
    const int c0 = blockIdx.y * 64;
    const int kb = c0 + wid * 16;
    const int cb = (G == 32) ? (kb & ~31) : kb;   // first input channel

    const CgLayout L = cg_layout_x(a.th, a.tw, a.s);
    const int zpos = L.nreal;                      // the zero pixel
    const int xpos = (L.nreal + 1 + 7) & ~7;
    unsigned short* lds_x = cg_lds;
    unsigned short* lds_dy = cg_lds + xpos * CG_PIX;

    cg_f32x4 acc[9][CT];
    #pragma unroll
    for (int t = 0; t < 9; ++t)
        #pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[t][ct] = cg_f32x4{0.f, 0.f, 0.f, 0.f};

    // tr16 operand reads: this lane supplies 4 channels of pixel (fr >> 2)
    // of its window: granule and the 8-B half of it
    const int sub = (fr & 1) * 4;
    const int g_dy = wid * 2 + ((fr >> 1) & 1);
    const int g_x = ((cb - c0) >> 3) + ((fr >> 1) & 1);

    const long U = (long)a.N * a.tiles;
    const long u_end = min(U, ((long)chunk + 1) * a.upc);
    for (long u = (long)chunk * a.upc; u < u_end; ++u) {
        const int n = (int)(u / a.tiles), tile = (int)(u % a.tiles);
        const int p0 = (tile / a.tiles_w) * a.th;
        const int q0 = (tile % a.tiles_w) * a.tw;
        const int eth = min(a.th, a.P - p0), etw = min(a.tw, a.Q - q0);
        const int npx = eth * etw;
        const int nsteps = (npx + 31) >> 5;
        __syncthreads();   // the previous unit's reads are done
        cg_stage(a.x + (long)n * a.H * a.W * a.C + c0, lds_x, xpos, L,
                 a.s * p0 - 1, a.s * q0 - 1, a.H, a.W, a.C, wid, lane);
        // dy: position = pixel index within the tile, zeros past npx
        const unsigned short* dyn = a.dy + (long)n * a.P * a.Q * a.C + c0;
        for (int d = wid; d < nsteps * 4; d += CG_WAVES) {
            const int pos = d * 8 + (lane >> 3);
            const int ph = pos / etw, pw = pos - ph * etw;
            const int g = (lane & 7) ^ ((pos >> 1) & 7);
            const unsigned short* sp =
                pos < npx ? dyn + ((long)(p0 + ph) * a.Q + q0 + pw) * a.C + g * 8
                          : cg_zero16;
            FDA_CG_GLDS16(sp, lds_dy + d * 512);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int st = 0; st < nsteps; ++st) {
            cg_short4 af[2];
            int bpos[2];
            #pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int idx = st * 32 + fq * 8 + hf * 4 + (fr >> 2);
                af[hf] = cg_tr16(lds_dy + cg_lds_off(idx, g_dy) + sub);
                const int ph = idx / etw, pw = idx - ph * etw;
                bpos[hf] = idx < npx ? a.s * ph * L.lwp + pw : -1;
            }
            cg_short8 av;
            #pragma unroll
            for (int e = 0; e < 4; ++e) { av[e] = af[0][e]; av[e + 4] = af[1][e]; }
            #pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int dr = t / 3, dc = t % 3;
                const int delta =
                    dr * L.lwp + (L.deint ? (dc & 1) * L.hw + (dc >> 1) : dc);
                #pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    cg_short4 bf[2];
                    #pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const int pos = bpos[hf] < 0 ? zpos : bpos[hf] + delta;
                        bf[hf] = cg_tr16(lds_x + cg_lds_off(pos, g_x + 2 * ct) +
                                         sub);
                    }
                    cg_short8 bv;
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bv[e] = bf[0][e];
                        bv[e + 4] = bf[1][e];
                    }
                    acc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        av, bv, acc[t][ct], 0, 0, 0);
                }
            }
        }
    }

    // D[i = 4*fq + v][j = fr]: output channel kb + i, input channel
    // cb + 16*ct + j; stored where the two share a group
    const long n_out = (long)a.C * 9 * a.cpg;
    float* o = a.ws + (a.nch > 1 ? (long)chunk * n_out : 0);
    #pragma unroll
    for (int t = 0; t < 9; ++t)
        #pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int ic = cb + 16 * ct + fr;
            #pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int k = kb + 4 * fq + v;
                if (ic / a.cpg == k / a.cpg)
                    o[((long)k * 9 + t) * a.cpg + ic % a.cpg] = acc[t][ct][v];
            }
        }
}

void conv_grouped_wgrad_launch(const void* dy, const void* x, float* ws,
                               const ConvGeom& g, int cpg,
                               hipStream_t stream) {
    const ConvGroupedPlan p =
        conv_grouped_plan(g.N, g.H, g.W, g.C, cpg, g.sy, CONV_GROUPED_WGRAD);
    CgWgradArgs a;
    a.dy = (const unsigned short*)dy;
    a.x = (const unsigned short*)x;
    a.ws = ws;
    a.N = g.N;  a.H = g.H;  a.W = g.W;  a.P = g.P;  a.Q = g.Q;
    a.C = g.C;  a.cpg = cpg;  a.s = g.sy;
    a.th = p.th;  a.tw = p.tw;  a.tiles_w = p.tiles_w;
    a.tiles = p.tiles_h * p.tiles_w;  a.upc = p.upc;  a.nch = p.nch;
    const dim3 grid((unsigned)p.nch, (unsigned)(g.C / 64));
    if (cpg == 32)
        hipLaunchKernelGGL(conv_grouped_wgrad_kernel<32>, grid,
                           dim3(CG_WAVES * 64), p.lds_bytes, stream, a);
    else
        hipLaunchKernelGGL(conv_grouped_wgrad_kernel<16>, grid,
                           dim3(CG_WAVES * 64), p.lds_bytes, stream, a);
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
