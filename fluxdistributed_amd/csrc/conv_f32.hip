// Implicit-GEMM 2D convolution for gfx950 (CDNA4), NHWC fp32: forward,
// input gradient and weight gradient on the true-fp32 matrix instruction
// v_mfma_f32_16x16x4_f32 (gfx950 has no xf32 MFMA). fp32 operands, fp32
// accumulate, fp32 store with no rounding step.
//
// The GEMM views are those of conv_igemm.hip:
//   fwd    y[m][k]      = sum_{rs,c} x_gather[m][rs,c] * w[k][rs][c]
//   dgrad  dx[m][c]     = sum_{rs,k} dy_gather[m][rs,k] * w[k][rs][c]
//   wgrad  dw[k][rs][c] = sum_m      dy[m][k]           * x_gather[m][rs,c]
// and so is the staging: 16-B global_load_lds whose per-lane source
// addresses do the im2col gather (a 16-B granule is 4 floats), a 16-B zero
// page for out-of-bounds taps and rows, two LDS buffers with the next
// K-step's DMA in flight across the MFMA phase, source offsets that advance
// incrementally within a filter tap, (h%sy, w%sx) parity classes on
// blockIdx.z for a strided dgrad. What differs is the operand layout of the
// instruction, and with it everything between the LDS and the accumulator.
//
// Lane layout (CDNA3/4 ISA, v_mfma_f32_16x16x4_f32; fr = lane & 15,
// fq = lane >> 4): a lane holds ONE scalar of each operand,
//   A[i = fr][k = fq],  B[k = fq][j = fr],  D[i = 4*fq + v][j = fr], v = 0..3.
// Two freedoms follow, and the kernels use both.
//
// (1) The reduction index may be permuted inside a staged K-step, as long as
// A and B agree. Where the reduction runs along LDS rows (fwd A and B, dgrad
// A: [row][32 floats]) a lane reads one ds_read_b128 at reduction offsets
// kg*16 + fq*4 + e, e = 0..3, and component e feeds the e-th of four
// consecutive MFMAs: MFMA e of group kg reduces over {kg*16 + fq*4 + e}.
//
// (2) The rows/columns of a fragment may be any 16 of the wave's 64, as long
// as the epilogue knows which. Where the reduction index is the LDS ROW and
// the output channel runs along it (dgrad B = the weight as stored,
// [k][c-contiguous]; wgrad dy [m][k] and x [m][c]) a lane reads one
// ds_read_b128 at channels 4*fr .. 4*fr+3 and component t becomes its scalar
// for fragment t: fragment t holds the channels {4*fr + t}. The forward gets
// the same column assignment for free by having the stager place weight row
// 4*(p&15) + (p>>4) into LDS row p. So in every kernel a lane ends up with
// four consecutive output channels of a row across its four column
// fragments, and the epilogue stores 16 B per lane straight from the
// accumulators, 256 contiguous bytes per 16 lanes, with no LDS round trip.
// The dgrad needs no transposed weight and the wgrad no transpose reads.
//
// LDS bank argument (64 banks x 4 B = 256 B per cycle; a ds_read_b128 of a
// wave is served in four passes of 16 lanes, so the floor is 4 passes, and
// it is reached iff the 16 lanes of each pass touch 16 distinct 16-B units
// modulo 256 B):
//  - reduction-contiguous tiles have 128-B rows; granule g of row r is kept
//    in slot g ^ (r & 7) (source-side swizzle, the stager picks the source
//    granule for each slot). A lane reads row base+fr, slot (kg*4+fq)^(r&7):
//    the unit modulo 256 B is (r&1)*8 + slot. Within one fq the 16 rows give
//    slot = const ^ (r&7), all 8 slots twice, once per row parity: 16
//    distinct units. A pass that mixes lanes of two fq groups (the hardware's
//    pass is not simply lanes 0..15) takes disjoint row sets from them, e.g.
//    rows {0-3,12-15} at g and {4-11} at g^1, which enumerates to all 16
//    units as well. This is byte for byte the access pattern of the bf16
//    kernel's BK=64 tiles, for which SQ_LDS_BANK_CONFLICT measured 0.
//  - channel-contiguous tiles have rows of 256 B (64 channels) or 512 B
//    (128), both multiples of 256 B, and are stored unswizzled. A lane reads
//    row f(fq), bytes (wave column + 4*fr)*4: the unit modulo 256 B is fr,
//    whatever the row. Any pass whose 16 lanes have 16 distinct fr (a whole
//    fq group, or quarters of different groups as above) is conflict-free.
// Neither pattern has been counter-profiled in this file yet; the first is
// the measured one of conv_igemm.hip, the second is argued only.
//
// Work split. The wave tile is 64x64 (4x4 fragments, 16 accumulator
// registers x 4). One K-step stages 32 reduction values: 128 MFMAs of 8
// passes each per wave against 8 (128x128 block) or 16 (64x64 block) 1-KiB
// DMAs, so the kernels are MFMA-bound by a wide margin and the block tile is
// chosen for grid fill, not for LDS reuse (conv_f32_plan):
//   128x128, 4 waves, 2 x 32 KiB LDS    64x64, 1 wave, 2 x 16 KiB LDS
// No split-K. The wgrad cuts the pixel axis into chunks of whole 32-pixel
// K-steps; the block of chunk c stores its tile once into slab[c][K][R*S*C]
// and wgrad_slab_fold_kernel (elementwise.hip) sums the slabs in chunk
// order, so there are no atomics, no pre-zeroing and the same bits on every
// run; a one-chunk plan writes the result directly (conv_f32_wgrad_plan).
//
// Constraints (bindings): C % 64 == 0, K % 64 == 0, dilation 1, groups 1.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// No packed fp32 VALU ops in this file (the MFMA is the only arithmetic).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __align__(16) static const float conv_f32_zero16[4] = {0.f, 0.f,
                                                                  0.f, 0.f};

#define FDA_F32_GLDS16(gptr, lptr)                                          \
    __builtin_amdgcn_global_load_lds(                                       \
        (const __attribute__((address_space(1))) void*)(gptr),              \
        (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

constexpr int FBK = 32;         // reduction values per K-step (128-B rows)
constexpr int FKG = FBK / 16;   // groups of four MFMAs per K-step
constexpr int GLDS_F = 256;     // floats one 64-lane 16-B DMA writes

template <int MODE, int BM, int BN>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64)
void conv_f32_kernel(const float* __restrict__ src,
                     const float* __restrict__ wgt, float* __restrict__ out,
                     int N, int H, int W, int C, int K, int P, int Q, int R,
                     int S, int sy, int sx, int py, int px) {
    static_assert(MODE == CONV_FWD || MODE == CONV_DGRAD, "fwd or dgrad");
    constexpr int NW = (BM / 64) * (BN / 64);   // waves per block
    constexpr int WN = BN / 64;
    constexpr int A_ELEMS = BM * FBK;
    constexpr int B_ELEMS = BN * FBK;
    constexpr int BUF_ELEMS = A_ELEMS + B_ELEMS;
    constexpr int AI = BM / (8 * NW);   // A DMAs per wave per K-step
    constexpr int BI = BN / (8 * NW);   // B DMAs per wave per K-step
    // dgrad B tile [32 k][BN c]: granules per row, rows per DMA
    constexpr int GPRB = BN / 4;
    constexpr int RPGB = 64 / GPRB;

    const int OC = (MODE == CONV_DGRAD) ? C : K;
    const int RC = (MODE == CONV_FWD) ? C : K;

    int a = 0, b = 0, OH, OW, r0 = 0, s0 = 0, nR = R, nS = S;
    if (MODE == CONV_FWD) {
        OH = P; OW = Q;
    } else {
        a = blockIdx.z / sx;  b = blockIdx.z % sx;
        OH = (H - a + sy - 1) / sy;
        OW = (W - b + sx - 1) / sx;
        r0 = (a + py) % sy;  nR = (R - r0 + sy - 1) / sy;
        s0 = (b + px) % sx;  nS = (S - s0 + sx - 1) / sx;
        if (OH <= 0 || OW <= 0) return;
        if (nR < 0) nR = 0;
        if (nS < 0) nS = 0;
    }
    const long M = (long)N * OH * OW;
    const long m0 = (long)blockIdx.x * BM;
    if (m0 >= M) return;
    const int n0 = blockIdx.y * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wm = wid / WN;
    const int wn = wid % WN;

    extern __shared__ float lds_f32[];   // [2][BUF_ELEMS]

    // ---- per-lane staging descriptors ------------------------------------
    // reduction-contiguous tiles: a DMA covers 8 rows of 8 granules
    const int cslot = lane & 7;
    int a_row[AI];
    long a_pix[AI];
    int a_hb[AI], a_wb[AI];
    bool a_mok[AI];
    #pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int row = (wid * AI + i) * 8 + (lane >> 3);
        a_row[i] = row;
        const long m = m0 + row;
        const bool mok = m < M;
        const long mm = mok ? m : 0;
        const int ow = (int)(mm % OW);
        const int oh = (int)((mm / OW) % OH);
        const int n = (int)(mm / ((long)OW * OH));
        a_mok[i] = mok;
        if (MODE == CONV_FWD) {
            a_hb[i] = oh * sy - py;
            a_wb[i] = ow * sx - px;
            a_pix[i] = ((long)n * H) * W * C;
        } else {
            a_hb[i] = oh + (a + py) / sy;
            a_wb[i] = ow + (b + px) / sx;
            a_pix[i] = ((long)n * P) * Q * K;
        }
    }

    const int cblocks = RC / FBK;
    const int T = nR * nS * cblocks;
    const long RSC = (long)R * S * C;
    // within a tap the B source advances by one K-step: 32 floats along a
    // weight row (fwd), 32 whole weight rows (dgrad)
    const long b_step = (MODE == CONV_FWD) ? FBK : FBK * RSC;

    long a_goff[AI];
    bool a_okc[AI];
    long b_goff[BI];
    int last_rsi = -1;
    auto stage = [&](int buf, int it) {
        const int rsi = it / cblocks;
        const int ri = rsi / nS, si = rsi % nS;
        float* base = lds_f32 + buf * BUF_ELEMS;
        if (rsi != last_rsi) {
            last_rsi = rsi;
            const int cb = (it % cblocks) * FBK;
            #pragma unroll
            for (int i = 0; i < AI; ++i) {
                const int cs = (cslot ^ (a_row[i] & 7)) * 4;
                bool ok = a_mok[i];
                long off;
                if (MODE == CONV_FWD) {
                    const int h = a_hb[i] + ri, w = a_wb[i] + si;
                    ok = ok && (unsigned)h < (unsigned)H &&
                         (unsigned)w < (unsigned)W;
                    off = a_pix[i] + ((long)h * W + w) * C + cb + cs;
                } else {
                    const int p = a_hb[i] - ri, q = a_wb[i] - si;
                    ok = ok && (unsigned)p < (unsigned)P &&
                         (unsigned)q < (unsigned)Q;
                    off = a_pix[i] + ((long)p * Q + q) * K + cb + cs;
                }
                a_goff[i] = off;
                a_okc[i] = ok;
            }
            const int r = r0 + ri * ((MODE == CONV_FWD) ? 1 : sy);
            const int s = s0 + si * ((MODE == CONV_FWD) ? 1 : sx);
            const int rs = r * S + s;
            #pragma unroll
            for (int i = 0; i < BI; ++i) {
                if (MODE == CONV_FWD) {
                    // LDS row p holds output channel 4*(p&15) + (p>>4) of
                    // its 64-channel wave column (freedom (2) above)
                    const int p = (wid * BI + i) * 8 + (lane >> 3);
                    const int ch = (p & ~63) + ((p & 15) << 2) + ((p >> 4) & 3);
                    b_goff[i] = (long)(n0 + ch) * RSC + (long)rs * C + cb +
                                (cslot ^ (p & 7)) * 4;
                } else {
                    // the weight as stored: row k, BN contiguous c of tap rs
                    const int kr = (wid * BI + i) * RPGB + lane / GPRB;
                    b_goff[i] = (long)(cb + kr) * RSC + (long)rs * C + n0 +
                                (lane % GPRB) * 4;
                }
            }
        } else {
            #pragma unroll
            for (int i = 0; i < AI; ++i) a_goff[i] += FBK;
            #pragma unroll
            for (int i = 0; i < BI; ++i) b_goff[i] += b_step;
        }
        #pragma unroll
        for (int i = 0; i < AI; ++i) {
            const float* sp = a_okc[i] ? src + a_goff[i] : conv_f32_zero16;
            FDA_F32_GLDS16(sp, base + (wid * AI + i) * GLDS_F);
        }
        #pragma unroll
        for (int i = 0; i < BI; ++i)
            FDA_F32_GLDS16(wgt + b_goff[i],
                           base + A_ELEMS + (wid * BI + i) * GLDS_F);
    };

    // ---- fragment read offsets (floats into an LDS buffer) ---------------
    const int fr = lane & 15, fq = lane >> 4;
    int a_off[4][FKG];
    int b_off[4][FKG];   // fwd: [ni][kg]; dgrad: [e][kg]
    #pragma unroll
    for (int kg = 0; kg < FKG; ++kg) {
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = wm * 64 + mi * 16 + fr;
            a_off[mi][kg] = row * FBK + (((kg * 4 + fq) ^ (row & 7)) << 2);
        }
        #pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (MODE == CONV_FWD) {
                const int row = wn * 64 + t * 16 + fr;
                b_off[t][kg] = A_ELEMS + row * FBK +
                               (((kg * 4 + fq) ^ (row & 7)) << 2);
            } else {
                b_off[t][kg] = A_ELEMS + (kg * 16 + fq * 4 + t) * BN +
                               wn * 64 + 4 * fr;
            }
        }
    }

    f32x4 acc[4][4];
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop: the one barrier per K-step of conv_igemm_kernel ------
    if (T > 0) stage(0, 0);
    for (int it = 0; it < T; ++it) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (it + 1 < T) stage((it + 1) & 1, it + 1);
        const float* buf = lds_f32 + (it & 1) * BUF_ELEMS;
        f32x4 af[4][FKG], bf[4][FKG];
        #pragma unroll
        for (int kg = 0; kg < FKG; ++kg) {
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi][kg] = *(const f32x4*)(buf + a_off[mi][kg]);
            #pragma unroll
            for (int t = 0; t < 4; ++t)
                bf[t][kg] = *(const f32x4*)(buf + b_off[t][kg]);
        }
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kg = 0; kg < FKG; ++kg)
            #pragma unroll
            for (int e = 0; e < 4; ++e)
                #pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    #pragma unroll
                    for (int ni = 0; ni < 4; ++ni) {
                        const float bv = (MODE == CONV_FWD) ? bf[ni][kg][e]
                                                            : bf[e][kg][ni];
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            af[mi][kg][e], bv, acc[mi][ni], 0, 0, 0);
                    }
        __builtin_amdgcn_s_setprio(0);
    }

    // ---- epilogue: D row = 4*fq + v; column fragment ni holds channel
    // 4*fr + ni, so {acc[mi][0..3][v]} are 16 contiguous output bytes -------
    const int cbase = n0 + wn * 64 + 4 * fr;
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long m = m0 + wm * 64 + mi * 16 + fq * 4 + v;
            if (m >= M) continue;
            long o;
            if (MODE == CONV_FWD) {
                o = m * OC;
            } else {
                const int ww = (int)(m % OW);
                const int hh = (int)((m / OW) % OH);
                const int n = (int)(m / ((long)OW * OH));
                o = (((long)n * H + a + (long)sy * hh) * W + b +
                     (long)sx * ww) * C;
            }
            const f32x4 val = {acc[mi][0][v], acc[mi][1][v], acc[mi][2][v],
                               acc[mi][3][v]};
            *(f32x4*)(out + o + cbase) = val;
        }
}

// Tile choice. Every config runs the same 64x64 wave tiles, so the number of
// waves is fixed by the problem and the kernel is MFMA-bound: the tile only
// decides how the waves spread over the 256 CUs. 128x128 quarters the DMA
// bytes per MFMA and is taken when the output channels allow it and its
// grid still gives every CU a block; otherwise single-wave 64x64 blocks
// spread the same waves over all CUs. M is the row count of one parity
// class: the classes of a strided dgrad only add blocks, and a rule without
// them is one conv_f32_config can state from (M, C, K, R, S) alone.
ConvF32Plan conv_f32_plan(long M, int OC, int classes) {
    ConvF32Plan p;
    const bool big = OC % 128 == 0 && ((M + 127) / 128) * (OC / 128) >= 256;
    p.bm = p.bn = big ? 128 : 64;
    p.blocks = ((M + p.bm - 1) / p.bm) * (OC / p.bn) * classes;
    return p;
}

template <int MODE, int BM, int BN>
static void launch_f32(const float* src, const float* wgt, float* out,
                       const ConvGeom& g, hipStream_t stream) {
    constexpr ConvMode mode = (ConvMode)MODE;
    const dim3 grid((unsigned)((g.rows(mode) + BM - 1) / BM),
                    (unsigned)(g.oc(mode) / BN), (unsigned)g.classes(mode));
    const size_t shmem = 2 * (BM + BN) * FBK * sizeof(float);   // <= 64 KiB
    hipLaunchKernelGGL((conv_f32_kernel<MODE, BM, BN>), grid,
                       dim3((BM / 64) * (BN / 64) * 64), shmem, stream, src,
                       wgt, out, g.N, g.H, g.W, g.C, g.K, g.P, g.Q, g.R, g.S,
                       g.sy, g.sx, g.py, g.px);
}

void conv_f32_launch(const float* src, const float* wgt, float* out,
                     const ConvGeom& g, ConvMode mode, hipStream_t stream) {
    const ConvF32Plan p = conv_f32_plan(g.rows(mode), g.oc(mode),
                                        g.classes(mode));
    if (mode == CONV_DGRAD) {
        if (p.bm == 128) launch_f32<CONV_DGRAD, 128, 128>(src, wgt, out, g, stream);
        else launch_f32<CONV_DGRAD, 64, 64>(src, wgt, out, g, stream);
    } else {
        if (p.bm == 128) launch_f32<CONV_FWD, 128, 128>(src, wgt, out, g, stream);
        else launch_f32<CONV_FWD, 64, 64>(src, wgt, out, g, stream);
    }
}

// ---- wgrad ----------------------------------------------------------------
// Both operand tiles are [32 pixels][TCH channels], channel-contiguous, as
// they lie in memory. MFMA step s takes pixel 4*s + fq in lane group fq: one
// ds_read_b128 of dy (k = 4*fr .. +3) and one of x (c = 4*fr .. +3) feed the
// 16 MFMAs of the wave's 4x4 fragments. D row 4*fq + v of fragment (ki, ci)
// is output channel k = 4*(4*fq + v) + ki, column fr is c = 4*fr + ci.
constexpr int FW_MB = 32;        // pixels per K-step
constexpr int FW_MIN_STEPS = 4;  // shortest chunk, in K-steps

template <int TCH>
__global__ __launch_bounds__((TCH / 64) * (TCH / 64) * 64)
void conv_f32_wgrad_kernel(const float* __restrict__ dy,   // [M][K]
                           const float* __restrict__ x,    // [N,H,W,C]
                           float* __restrict__ ws,  /* nch == 1: [K][RS*C];
                                                       else [nch][K][RS*C] */
                           int N, int H, int W, int C, int K, int P, int Q,
                           int R, int S, int sy, int sx, int py, int px,
                           int nch, int mch) {
    constexpr int MB = FW_MB;
    constexpr int WT = TCH / 64;             // waves per tile axis
    constexpr int NW = WT * WT;
    constexpr int TILE = MB * TCH;           // floats per operand tile
    constexpr int GPRW = TCH / 4;            // granules per pixel row
    constexpr int RPGW = 64 / GPRW;          // pixel rows per DMA
    constexpr int GI = TILE / (GLDS_F * NW); // DMAs per wave per operand

    const WgradCoords bc = wgrad_block_coords(blockIdx.x, K / TCH, C / TCH,
                                              R * S, nch);
    const int rs = bc.rs, chunk = bc.chunk;
    const int r = rs / S, s = rs % S;
    const int k0 = bc.ktile * TCH, c0 = bc.ctile * TCH;
    const long M = (long)N * P * Q;
    const long mb0 = (long)chunk * mch;
    const long mend = (mb0 + mch < M) ? mb0 + mch : M;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wk = wid / WT, wc = wid % WT;

    extern __shared__ float lds_f32[];       // [2][2 * TILE]

    f32x4 acc[4][4];
    #pragma unroll
    for (int ki = 0; ki < 4; ++ki)
        #pragma unroll
        for (int ci = 0; ci < 4; ++ci) acc[ki][ci] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane pixel coordinates, advanced by constant-delta carries as in
    // conv_wgrad_kernel (no division per K-step)
    const int gch = (lane % GPRW) * 4;
    int st_q[GI], st_p[GI], st_n[GI];
    long st_m[GI], st_dyoff[GI];
    #pragma unroll
    for (int i = 0; i < GI; ++i) {
        const long m = mb0 + (wid * GI + i) * RPGW + lane / GPRW;
        st_m[i] = m;
        st_q[i] = (int)(m % Q);
        st_p[i] = (int)((m / Q) % P);
        st_n[i] = (int)(m / ((long)Q * P));
        st_dyoff[i] = m * K + k0 + gch;
    }
    const int dQ = MB % Q, dP = (MB / Q) % P, dN0 = MB / (Q * P);
    const long dDY = (long)MB * K;

    auto stage = [&](int buf) {
        float* base = lds_f32 + buf * 2 * TILE;
        #pragma unroll
        for (int i = 0; i < GI; ++i) {
            const float* sp =
                (st_m[i] < mend) ? dy + st_dyoff[i] : conv_f32_zero16;
            FDA_F32_GLDS16(sp, base + (wid * GI + i) * GLDS_F);
        }
        #pragma unroll
        for (int i = 0; i < GI; ++i) {
            const float* sp = conv_f32_zero16;
            if (st_m[i] < mend) {
                const int hh = st_p[i] * sy - py + r;
                const int ww = st_q[i] * sx - px + s;
                if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                    sp = x + (((long)st_n[i] * H + hh) * W + ww) * C + c0 + gch;
            }
            FDA_F32_GLDS16(sp, base + TILE + (wid * GI + i) * GLDS_F);
        }
        #pragma unroll
        for (int i = 0; i < GI; ++i) {
            st_m[i] += MB;
            st_dyoff[i] += dDY;
            int q = st_q[i] + dQ;
            int p = st_p[i] + dP;
            int n = st_n[i] + dN0;
            if (q >= Q) { q -= Q; ++p; }
            if (p >= P) { p -= P; ++n; }
            if (p >= P) { p -= P; ++n; }
            st_q[i] = q; st_p[i] = p; st_n[i] = n;
        }
    };

    const int fr = lane & 15, fq = lane >> 4;
    const int a_off = fq * TCH + wk * 64 + 4 * fr;
    const int b_off = TILE + fq * TCH + wc * 64 + 4 * fr;

    const int nsteps = (int)((mend - mb0 + MB - 1) / MB);
    if (nsteps > 0) stage(0);
    for (int it = 0; it < nsteps; ++it) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (it + 1 < nsteps) stage((it + 1) & 1);
        const float* buf = lds_f32 + (it & 1) * 2 * TILE;
        f32x4 af[MB / 4], bf[MB / 4];
        #pragma unroll
        for (int st = 0; st < MB / 4; ++st) {
            af[st] = *(const f32x4*)(buf + a_off + st * 4 * TCH);
            bf[st] = *(const f32x4*)(buf + b_off + st * 4 * TCH);
        }
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int st = 0; st < MB / 4; ++st)
            #pragma unroll
            for (int ki = 0; ki < 4; ++ki)
                #pragma unroll
                for (int ci = 0; ci < 4; ++ci)
                    acc[ki][ci] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        af[st][ki], bf[st][ci], acc[ki][ci], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    }

    // epilogue: every element of the tile stored once (rows past mend were
    // staged as zeros), 16 B per lane, into the chunk's slab or the result
    const long RSC = (long)R * S * C;
    float* o = ws + (nch > 1 ? (long)chunk * K * RSC : 0);
    const int cc = c0 + wc * 64 + 4 * fr;
    #pragma unroll
    for (int ki = 0; ki < 4; ++ki)
        #pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int kk = k0 + wk * 64 + 4 * (4 * fq + v) + ki;
            const f32x4 val = {acc[ki][0][v], acc[ki][1][v], acc[ki][2][v],
                               acc[ki][3][v]};
            *(f32x4*)(o + kk * RSC + (long)rs * C + cc) = val;
        }
}

// Chunk plan, by the rule of conv_wgrad_plan: whole K-steps per chunk, even
// chunk lengths, and as many chunks as keep the grid within one resident
// wave of blocks: 256 CUs x 2 blocks of four waves (128x128 tile, 64 KiB
// LDS) or x 4 single-wave blocks (64x64 tile, 32 KiB), i.e. one or two waves
// per SIMD. The 128 tile needs both channel counts to divide by 128 and is
// taken only where its tiles alone put a block on a quarter of the CUs; below that
// the 64 tile's four times as many blocks need fewer, longer chunks for the
// same fill. A chunk is at least FW_MIN_STEPS K-steps, so that the slab
// store of a 64x64 tile is paid per 128 pixels at the least.
constexpr int FW_CUS = 256;

WgradF32Plan conv_f32_wgrad_plan(long M, int C, int K, int R, int S) {
    WgradF32Plan p;
    const long tiles128 = (long)(K / 128) * (C / 128) * R * S;
    const long tiles64 = (long)(K / 64) * (C / 64) * R * S;
    const bool big = K % 128 == 0 && C % 128 == 0 && tiles128 >= FW_CUS / 4;
    p.tile = big ? 128 : 64;
    const long tiles = big ? tiles128 : tiles64;
    const long slots = FW_CUS * (big ? 2 : 4);
    long nch = slots / tiles;
    if (nch < 1) nch = 1;
    long mch = ((M + nch - 1) / nch + FW_MB - 1) / FW_MB * FW_MB;
    if (mch < FW_MIN_STEPS * FW_MB) mch = FW_MIN_STEPS * FW_MB;
    p.mch = (int)mch;
    p.nch = (int)((M + mch - 1) / mch);
    p.nwg = tiles * p.nch;
    return p;
}

void conv_f32_wgrad_launch(const float* dy, const float* x, float* ws,
                           const ConvGeom& g, hipStream_t stream) {
    const WgradF32Plan p =
        conv_f32_wgrad_plan(g.rows(CONV_FWD), g.C, g.K, g.R, g.S);
    auto launch = [&](auto kern, int tch) {
        const size_t shmem = 2 * 2 * FW_MB * tch * sizeof(float);
        hipLaunchKernelGGL(kern, dim3((unsigned)p.nwg),
                           dim3((tch / 64) * (tch / 64) * 64), shmem, stream,
                           dy, x, ws, g.N, g.H, g.W, g.C, g.K, g.P, g.Q, g.R,
                           g.S, g.sy, g.sx, g.py, g.px, p.nch, p.mch);
    };
    if (p.tile == 128) launch(conv_f32_wgrad_kernel<128>, 128);
    else launch(conv_f32_wgrad_kernel<64>, 64);
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
