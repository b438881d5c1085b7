// Narrow pointwise (1x1) convolution for gfx950 (CDNA4), NHWC bf16: forward,
// input gradient and weight gradient for C % 8 == 0 and K % 8 == 0 with
// 8 <= C, K <= 256, stride 1, padding 0, groups 1 (the pointwise halves of
// depthwise-separable blocks whose channel counts are not multiples of 64).
//
// Why not conv_igemm with tail masking. With M = N*H*W pixels a 1x1 conv is a
// skinny GEMM y[M][K] = x[M][C] . w[K][C]^T that does C*K/(C+K) MACs per byte
// moved: 21 for 32 -> 64, 64 for 128 -> 128. By the instruction and bandwidth
// rates it is memory-bound by a wide margin (an estimate, see
// profiles/conv_pw.md for what was measured), and the whole weight is at most
// 128 KiB. So the aim is the one of conv_grouped.hip: read the activation
// once, write the output once, keep the weight in registers. No im2col
// gather, no K loop through LDS, no transposed weight copy.
//
// Forward and dgrad are one kernel, y[m][o] = sum_r src[m][r] * Wf[o][r]:
//   forward: src = x,  r over C, o over K, Wf = w as stored;
//   dgrad:   src = dy, r over K, o over C, Wf = w transposed, gathered once
//            in the prologue from the stored [K][C] weight (element loads).
// MFMA orientation as in conv_grouped.hip (fr = lane & 15, fq = lane >> 4):
// the WEIGHTS are the row operand of v_mfma_f32_16x16x32_bf16,
// A[i = output fr][k = 8*fq .. +7], the activations the column operand,
// B[k = 8*fq .. +7][j = pixel fr]. Eight consecutive channels of a pixel are
// a B fragment as they lie in memory: one 16-B global load per lane and
// reduction step. D[i = 4*fq + v][j = fr] leaves a lane with four consecutive
// output channels of one pixel: one bf16 round from the fp32 accumulator and
// one 8-B store.
//
// A wave owns an output slab of at most 64 channels (four 16-row blocks) and
// keeps the A fragments of the whole reduction, 4 x NS x 4 VGPRs with
// NS = ceil(red / 32) MFMA steps, 128 at most, for its life. It walks
// 16-pixel tiles of M; the B fragments of its next tile are loaded before
// the MFMAs of the current one (NS x 4 VGPRs in flight). Blocks of a slab
// past the true output extent are skipped wave-uniformly.
//
// Several slabs (more than 64 outputs): the slabs of one pixel tile are waves
// of ONE block, nslab x pgs waves with pgs = 4 / nslab pixel groups, and each
// wave loads the tile's B fragments itself. That is a deliberate deviation
// from staging the tile once in LDS: the two to four waves that want the same
// 16 x red bf16 (8 KiB at most) run on one CU at the same time, so the
// repeated requests are served by the CU's vector cache and HBM sees the
// tile once, which is the argument conv_dw.hip makes for its column halo.
// An LDS tile would save the repeated requests at the price of a barrier
// pair per 16 pixels between waves that otherwise never meet. With one slab
// (K <= 64 forward, C <= 64 dgrad: every MobileNetV1 shape at width 0.25 up
// to 64 outputs, and 32 -> 64 at width 1.0) nothing is requested twice. Not
// counter-profiled. Forward and dgrad use no LDS and no barrier.
//
// Tails. The reduction is padded to a multiple of 32 and the outputs to a
// multiple of 16. A reduction granule at or past the true extent is zero in
// BOTH operands: the activation bytes there belong to the next pixel and
// 0 * Inf is NaN, so that load is not issued and the register is zeroed.
// Pixel columns at or past M are neither loaded nor stored; output rows past
// the true extent are not stored. A pixel is an MFMA column, so a non-finite
// value in one pixel reaches no other.
//
// Weight gradient. dw[k][c] = sum_m dy[m][k] * x[m][c], the reduction running
// along pixels; both operands are [pixel][channel]. A block owns a 64 x 64
// (k-slab, c-slab) pair of dw and one chunk of pixels. Per round it stages
// 128 pixels x 64 channels of dy and of x into LDS with 16-B global_load_lds
// in the layout of conv_grouped.hip (128 B per pixel, granule g of pixel p in
// slot g ^ ((p >> 1) & 7); the bank argument there covers it, the reads here
// are the unshifted ones); rows past the chunk's end and granules past C or K
// come from a 16-B zero page. ds_read_tr16_b64 serves both fragments. Wave w
// owns rows 16w .. 16w+15 of the k-slab against all 64 columns: four
// accumulator tiles, 16 VGPRs. That is narrower than a 64 x 64 tile per
// wave: the four waves share ONE staged tile pair, where a pixel split
// between waves would need a cross-wave fold at the end. A wave whose rows
// lie past K only stages. Chunk c stores once into slab[c][K][C] (fp32) and
// wgrad_slab_fold_kernel sums the slabs in order (in two levels past 32
// slabs, see the plan); one chunk writes the result directly. No atomics,
// nothing pre-zeroed, the same bits on every run.
//
// Constraints (bindings): C, K % 8 == 0 in [8, 256], 1x1, stride 1, padding
// 0, M = N*H*W <= INT32_MAX.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// No packed fp32 VALU ops in this file (the MFMA is the only arithmetic).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

typedef __attribute__((ext_vector_type(8))) short pw_short8;
typedef __attribute__((ext_vector_type(4))) short pw_short4;
typedef __attribute__((ext_vector_type(4))) float pw_f32x4;

__device__ __align__(16) static const unsigned short pw_zero16[8] = {0};

#define FDA_PW_GLDS16(gptr, lptr)                                           \
    __builtin_amdgcn_global_load_lds(                                       \
        (const __attribute__((address_space(1))) void*)(gptr),              \
        (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

constexpr int PW_CUS = 256;
constexpr int PW_WAVES = 4;     // per block at most
constexpr int PW_PT = 128;      // wgrad: pixels staged per round
constexpr int PW_PIX = 64;      // wgrad: bf16 per LDS pixel, one 64-ch slab
constexpr int PW_FOLD1 = 32;    // wgrad: most slabs one ordered fold sums

// ---- forward / dgrad ------------------------------------------------------
// src [M][red], w [K][C] as stored, out [M][OC]. Forward: red = C, OC = K;
// dgrad: red = K, OC = C.
struct PwArgs {
    const unsigned short* src;
    const unsigned short* w;
    unsigned short* out;
    int M, red, OC, C, nslab, pgs, ntiles, dgrad;
};

// The B fragments of 16-pixel tile t: granule 4*j + fq of pixel 16*t + fr.
template <int NS>
__device__ __forceinline__ void pw_load_tile(const PwArgs& a, long t, int fr,
                                             int fq, pw_short8 (&b)[NS]) {
    const long m = t * 16 + fr;
    const bool ok = m < a.M;
    const unsigned short* row = a.src + m * a.red;
    #pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int r0 = j * 32 + fq * 8;
        pw_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ok && r0 < a.red) v = *(const pw_short8*)(row + r0);
        b[j] = v;
    }
}

template <int NS>
__global__ __launch_bounds__(PW_WAVES * 64)
void conv_pw_kernel(const PwArgs a) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int slab = wid % a.nslab, pg = wid / a.nslab;
    const int o0 = slab * 64;
    const int nbv = min(4, (a.OC - o0 + 15) >> 4);   // live 16-row blocks

    // ---- prologue: the A fragments of the slab, for the wave's life ------
    pw_short8 wr[4][NS];
    #pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int o = o0 + nb * 16 + fr;
        #pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int r0 = j * 32 + fq * 8;
            pw_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (o < a.OC && r0 < a.red) {
                if (!a.dgrad) {
                    v = *(const pw_short8*)(a.w + (long)o * a.C + r0);
                } else {
                    #pragma unroll
                    for (int e = 0; e < 8; ++e)
                        v[e] = (short)a.w[(long)(r0 + e) * a.C + o];
                }
            }
            wr[nb][j] = v;
        }
    }

    const long tstride = (long)gridDim.x * a.pgs;
    long t = (long)blockIdx.x * a.pgs + pg;
    pw_short8 b[NS], bn[NS];
    pw_load_tile<NS>(a, t, fr, fq, b);
    for (; t < a.ntiles; t += tstride) {
        pw_load_tile<NS>(a, t + tstride, fr, fq, bn);
        const long m = t * 16 + fr;
        #pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            if (nb >= nbv) break;
            pw_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int j = 0; j < NS; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[nb][j], b[j],
                                                              acc, 0, 0, 0);
            const int o = o0 + nb * 16 + 4 * fq;   // o % 4 == 0, OC % 8 == 0
            if (m < a.M && o < a.OC) {
                uint2 q;
                q.x = (unsigned)f32_to_bf16bits(acc[0]) |
                      ((unsigned)f32_to_bf16bits(acc[1]) << 16);
                q.y = (unsigned)f32_to_bf16bits(acc[2]) |
                      ((unsigned)f32_to_bf16bits(acc[3]) << 16);
                *(uint2*)(a.out + m * a.OC + o) = q;
            }
        }
        #pragma unroll
        for (int j = 0; j < NS; ++j) b[j] = bn[j];
    }
}

// ---- plan -----------------------------------------------------------------
// fwd / dgrad: one wave per output slab and pgs = 4 / nslab pixel groups per
// block. A wave keeps its weights for tpw = 16 tiles (256 pixels, the figure
// of the grouped plan), halved while the grid has fewer than four blocks per
// CU. wgrad: as many chunks as give every CU three blocks (three 32-KiB
// blocks share a CU), in whole 128-pixel rounds: a round reads 32 KiB and
// the block stores a slab of 16 KiB, so no chunk stores more than it reads.
// The ordered fold walks the slabs one after the other, about 85 ns each as
// measured (profiles/conv_pw.md): 724 slabs of a 32 -> 64 weight cost more
// than the wgrad kernel itself. Past PW_FOLD1 slabs the fold therefore runs
// in two levels: nch is rounded up to g * s with g = ceil(sqrt(nch)), the
// chunks past M run no round and store zeros, the first fold sums the s
// slabs j*g + i of every i (the slabs read as [s][g*K*C]) and the second the
// g results, both in order.
ConvPwPlan conv_pw_plan(long M, int C, int K, int mode) {
    ConvPwPlan p = {};
    p.nch = 1;
    if (mode == CONV_PW_WGRAD) {
        p.kslabs = (K + 63) / 64;
        p.cslabs = (C + 63) / 64;
        const long pairs = (long)p.kslabs * p.cslabs;
        long nch = (long)PW_CUS * 3 / pairs;
        nch = nch < 1 ? 1 : nch;
        long mch = (M + nch - 1) / nch;
        mch = (mch + PW_PT - 1) / PW_PT * PW_PT;
        p.mch = (int)mch;
        p.nch = (int)((M + mch - 1) / mch);
        p.fold_g = 1;
        if (p.nch > PW_FOLD1) {
            int g = 1;
            while (g * g < p.nch) ++g;
            p.fold_g = g;
            p.nch = g * ((p.nch + g - 1) / g);
        }
        p.blocks = p.nch * pairs;
        return p;
    }
    const int OC = mode == CONV_PW_FWD ? K : C;
    p.nslab = (OC + 63) / 64;
    p.pgs = PW_WAVES / p.nslab;
    const long ntiles = (M + 15) / 16;
    const long groups = (ntiles + p.pgs - 1) / p.pgs;
    int tpw = 16;
    while (tpw > 1 && (groups + tpw - 1) / tpw < 4 * PW_CUS) tpw /= 2;
    p.tpw = tpw;
    p.gx = (int)((groups + tpw - 1) / tpw);
    p.blocks = p.gx;
    return p;
}

void conv_pw_launch(const void* src, const void* w, void* out, long M, int C,
                    int K, int mode, hipStream_t stream) {
    const ConvPwPlan p = conv_pw_plan(M, C, K, mode);
    PwArgs a;
    a.src = (const unsigned short*)src;
    a.w = (const unsigned short*)w;
    a.out = (unsigned short*)out;
    a.M = (int)M;
    a.dgrad = mode == CONV_PW_DGRAD;
    a.red = a.dgrad ? K : C;
    a.OC = a.dgrad ? C : K;
    a.C = C;
    a.nslab = p.nslab;
    a.pgs = p.pgs;
    a.ntiles = (int)((M + 15) / 16);
    const dim3 grid((unsigned)p.gx), block((unsigned)(p.nslab * p.pgs * 64));
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, stream, a);
    };
    switch ((a.red + 31) / 32) {
        case 1: launch(conv_pw_kernel<1>); break;
        case 2: launch(conv_pw_kernel<2>); break;
        case 3: launch(conv_pw_kernel<3>); break;
        case 4: launch(conv_pw_kernel<4>); break;
        case 5: launch(conv_pw_kernel<5>); break;
        case 6: launch(conv_pw_kernel<6>); break;
        case 7: launch(conv_pw_kernel<7>); break;
        default: launch(conv_pw_kernel<8>); break;
    }
}

// ---- wgrad ----------------------------------------------------------------
struct PwWgradArgs {
    const unsigned short* dy;   // [M][K]
    const unsigned short* x;    // [M][C]
    float* ws;                  // nch == 1: [K][C]; else [nch][K][C]
    int M, C, K, mch, nch, cslabs;
};

// element offset of granule g of staged pixel pos
__device__ __forceinline__ int pw_lds_off(int pos, int g) {
    return pos * PW_PIX + ((g ^ ((pos >> 1) & 7)) << 3);
}

__device__ __forceinline__ pw_short4 pw_tr16(const unsigned short* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) pw_short4*)(p));
}

__global__ __launch_bounds__(PW_WAVES * 64)
void conv_pw_wgrad_kernel(const PwWgradArgs a) {
    __shared__ __align__(16) unsigned short pw_lds[2 * PW_PT * PW_PIX];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = blockIdx.x;
    const int k0 = (blockIdx.y / a.cslabs) * 64;
    const int c0 = (blockIdx.y % a.cslabs) * 64;
    const int kb = k0 + wid * 16;
    const bool live = kb < a.K;                      // wave-uniform
    const int nct = min(4, (a.C - c0 + 15) >> 4);    // live 16-column tiles
    unsigned short* lds_dy = pw_lds;
    unsigned short* lds_x = pw_lds + PW_PT * PW_PIX;

    pw_f32x4 acc[4];
    #pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = pw_f32x4{0.f, 0.f, 0.f, 0.f};

    // tr16 operand reads: this lane supplies 4 channels of pixel (fr >> 2)
    // of its window: granule and the 8-B half of it
    const int sub = (fr & 1) * 4;
    const int gh = (fr >> 1) & 1;
    const int g_dy = wid * 2 + gh;

    const long m_beg = (long)chunk * a.mch;
    const long m_end = min((long)a.M, m_beg + a.mch);
    for (long m0 = m_beg; m0 < m_end; m0 += PW_PT) {
        const int npx = (int)min((long)PW_PT, m_end - m0);
        const int nsteps = (npx + 31) >> 5;
        const int nd = nsteps * 4;     // DMAs per operand, 8 pixels each
        __syncthreads();   // the previous round's reads are done
        // d < nd: dy, then x; d is wave-uniform and so is the operand
        for (int d = wid; d < 2 * nd; d += PW_WAVES) {
            const bool isx = d >= nd;
            const int dd = isx ? d - nd : d;
            const int pos = dd * 8 + (lane >> 3);
            const int g = (lane & 7) ^ ((pos >> 1) & 7);
            const int CH = isx ? a.C : a.K;
            const int ch = (isx ? c0 : k0) + g * 8;
            const unsigned short* sp =
                (pos < npx && ch < CH)
                    ? (isx ? a.x : a.dy) + (m0 + pos) * CH + ch
                    : pw_zero16;
            FDA_PW_GLDS16(sp, (isx ? lds_x : lds_dy) + dd * 512);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!live) continue;
        for (int st = 0; st < nsteps; ++st) {
            const int idx0 = st * 32 + fq * 8 + (fr >> 2);
            pw_short8 av;
            {
                const pw_short4 a0 = pw_tr16(lds_dy + pw_lds_off(idx0, g_dy) + sub);
                const pw_short4 a1 =
                    pw_tr16(lds_dy + pw_lds_off(idx0 + 4, g_dy) + sub);
                #pragma unroll
                for (int e = 0; e < 4; ++e) { av[e] = a0[e]; av[e + 4] = a1[e]; }
            }
            #pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (ct >= nct) break;
                const pw_short4 b0 =
                    pw_tr16(lds_x + pw_lds_off(idx0, 2 * ct + gh) + sub);
                const pw_short4 b1 =
                    pw_tr16(lds_x + pw_lds_off(idx0 + 4, 2 * ct + gh) + sub);
                pw_short8 bv;
                #pragma unroll
                for (int e = 0; e < 4; ++e) { bv[e] = b0[e]; bv[e + 4] = b1[e]; }
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    av, bv, acc[ct], 0, 0, 0);
            }
        }
    }
    if (!live) return;

    // D[i = 4*fq + v][j = fr]: dw row kb + i, column c0 + 16*ct + j
    float* o = a.ws + (a.nch > 1 ? (long)chunk * a.K * a.C : 0);
    #pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int c = c0 + 16 * ct + fr;
        #pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int k = kb + 4 * fq + v;
            if (k < a.K && c < a.C) o[(long)k * a.C + c] = acc[ct][v];
        }
    }
}

void conv_pw_wgrad_launch(const void* dy, const void* x, float* ws, long M,
                          int C, int K, hipStream_t stream) {
    const ConvPwPlan p = conv_pw_plan(M, C, K, CONV_PW_WGRAD);
    PwWgradArgs a;
    a.dy = (const unsigned short*)dy;
    a.x = (const unsigned short*)x;
    a.ws = ws;
    a.M = (int)M;  a.C = C;  a.K = K;
    a.mch = p.mch;  a.nch = p.nch;  a.cslabs = p.cslabs;
    const dim3 grid((unsigned)p.nch, (unsigned)(p.kslabs * p.cslabs));
    hipLaunchKernelGGL(conv_pw_wgrad_kernel, grid, dim3(PW_WAVES * 64), 0,
                       stream, a);
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
