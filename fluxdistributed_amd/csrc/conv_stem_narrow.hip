// Narrow stem convolution for gfx950 (CDNA4), NHWC bf16: forward and weight
// gradient of a 3x3 conv with Cin in {1, 2, 3} input channels, padding 1,
// stride 1 or 2, K % 8 == 0 output channels in [8, 64] (the MobileNetV1
// stem at every width, K = 8 .. 32). There is no dgrad: stem inputs are data.
//
// One observation carries the design. The whole reduction is 9 * Cin <= 27
// values, which fits ONE K-step of v_mfma_f32_16x16x32_bf16. A tile of 16
// pixels x 16 output channels is therefore exactly one MFMA and the kernel
// has no K loop. At one MFMA per 512 B of output it is bound by the output
// write (77 MB for 96x3x224x224 -> 32 at stride 2, against 29 MB of input;
// byte counts, see profiles/conv_stem_narrow.md for what was measured).
//
// No packed copy of the input. The CONV_STEM kernels of conv_igemm.hip read
// an 8-channel, spatially padded copy that torch ops build for every call.
// Here a block stages the source rows of its th x tw output tile, halo
// included, into LDS once, as they lie in memory: the (tw-1)*stride + 3
// pixels of a source row are (..)*Cin contiguous bf16 whatever Cin is. Where
// a tap leaves the image the staged element is zero, so the compute loop
// has no border case. All nine taps are served from that LDS image.
//
// The gather. In (r, s, c) order the reduction index is j = (r*3 + s)*Cin + c
// = r * 3*Cin + (s*Cin + c): one filter row of a pixel's patch is 3*Cin
// contiguous elements of one staged row. The stored channels_last weight
// [K][3][3][Cin] is [K][9*Cin] with exactly that j. MFMA orientation as in
// conv_grouped.hip and conv_pw.hip (fr = lane & 15, fq = lane >> 4): the
// WEIGHTS are the row operand, A[i = channel fr][k = 8*fq .. +7], the patch
// the column operand, B[k = 8*fq .. +7][j = pixel fr], and
// D[i = 4*fq + v][j = fr] leaves a lane with four consecutive output channels
// of one pixel: one bf16 round and one 8-B store.
//
// A lane gathers its 8 reduction values with eight 2-byte LDS reads of the
// DENSE image at offsets (r_e * pitch + o_e) that depend on fq alone and
// are computed once. The alternative, a 4-channel padded image read 8 B at
// a time, does not fit: 9 taps x 4 channels are 36 > 32 reduction slots, so
// it would cost a second MFMA per tile and a channel-padding pass in the
// staging loop, to save LDS reads in a kernel that is bound by its global
// stores. Banks: for one e the 16 lanes of an fq group read pixels
// stride*Cin*2 = 2 .. 12 B apart, at most 48 consecutive dwords, so inside
// a group every dword is distinct or shared (a broadcast); the four groups
// read up to three different staged rows, and the row pitch is an odd
// number of dwords so that the rows do not start on one bank, but two
// groups can still meet on a bank (2-way at worst for stride 1, up to 3-way
// at stride 2). Not counter-profiled.
//
// A wave gathers its ceil(K/16) A fragments (at most 16 VGPRs) once in the
// prologue from the stored weight with element loads (a weight row is
// 18*Cin bytes, not 16-B aligned) and keeps them while it walks the 16-pixel
// tiles of its block: tile u of the th * tw/16 goes to wave u % 4.
//
// Zero padding. Reduction slots 9*Cin .. 31 are zero in BOTH operands: the
// weight register is zeroed and the LDS read is not issued. A slot that is
// zero on one side only is a bug, 0 * Inf is NaN (conv_pw.hip documents the
// same trap). Rows of a 16-block at or past K (K % 16 == 8) are zero in A
// and are not stored. Pixel columns at or past Q are neither gathered nor
// stored. A pixel is an MFMA column, so a non-finite input reaches exactly
// the outputs whose window holds it.
//
// Weight gradient. dw[k][j] = sum_m dy[m][k] * patch[m][j], j padded to 32,
// the reduction running over pixels, 32 per MFMA: dy^T is the row operand,
// A[i = channel fr][k = pixel 8*fq + e], and the patch matrix is two
// 16-column fragments, B[k = pixel 8*fq + e][j = 16*jt + fr] (one when
// 9*Cin <= 16). A unit is an (image, th x tw output tile) with tw a
// multiple of 32 and th * tw <= 256; a block takes a chunk of consecutive
// units. Per unit it stages the x halo tile as the forward does and the dy
// tile as [pixel][K padded to 16] with a pitch of Kp/2 + 1 dwords, both
// once. An MFMA step is 32 consecutive pixels of one output row; step t goes
// to wave t % 4. For a lane, j and with it (r, o) is fixed and the 8 pixels
// are stride*Cin elements apart: eight 2-byte reads at constant offsets.
// The dy reads are 2-byte reads too; the odd dword pitch puts the four fq
// groups (8 pixels apart) on disjoint banks. Pixels of a step at or past Q
// are zero in both operands: dy is staged as zero there and the patch read
// is not issued (its bytes are real pixels of the image at stride 2).
// Accumulators: ceil(K/16) x 2 tiles, at most 32 VGPRs, kept over the whole
// chunk. At the end the four waves' accumulators meet through LDS and are
// added in wave order, and the block stores once into its fp32 slab;
// wgrad_slab_fold_kernel sums the slabs in chunk order (in two levels past
// 32 slabs, as conv_pw does). No atomics, nothing pre-zeroed, the same bits
// on every run. The result is [K][9*Cin] fp32, the channels_last weight
// order.
//
// Constraints (bindings): Cin in {1, 2, 3}, K % 8 == 0 in [8, 64], 3x3,
// padding 1, stride 1 or 2, N*H*W <= INT32_MAX.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// No packed fp32 VALU ops in this file (the MFMA is the only arithmetic).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

typedef __attribute__((ext_vector_type(8))) short sn_short8;
typedef __attribute__((ext_vector_type(4))) float sn_f32x4;

constexpr int SN_CUS = 256;
constexpr int SN_WAVES = 4;
constexpr int SN_THREADS = SN_WAVES * 64;
constexpr int SN_TH_MAX = 4;      // output rows of a tile
constexpr int SN_TW_MAX = 128;    // output columns of a tile
constexpr int SN_WG_PIX = 256;    // wgrad: th * tw at most
constexpr int SN_FOLD1 = 32;      // wgrad: most slabs one ordered fold sums

// Elements between staged rows of `el` elements: an odd number of dwords.
__host__ __device__ constexpr int sn_pitch(int el) {
    return (((el + 1) / 2) | 1) * 2;
}
constexpr int SN_ROWS_MAX = (SN_TH_MAX - 1) * 2 + 3;
constexpr int SN_X_ELEMS =
    SN_ROWS_MAX * sn_pitch(((SN_TW_MAX - 1) * 2 + 3) * 3);
constexpr int SN_DY_DWORDS = SN_WG_PIX * (64 / 2 + 1);
static_assert(SN_DY_DWORDS >= SN_WAVES * 4 * 2 * 256,
              "the wave fold reuses the dy tile");

struct SnArgs {
    const unsigned short* x;    // [N][H][W][Cin]
    const unsigned short* w;    // fwd: [K][9*Cin]
    const unsigned short* dy;   // wgrad: [N][P][Q][K]
    unsigned short* y;          // fwd: [N][P][Q][K]
    float* ws;                  // wgrad: nch == 1 ? [K][9*Cin] : [nch][..]
    int N, H, W, P, Q, K, stride;
    int th, tw, tiles_h, tiles_w;
    int nch, upc, units;        // wgrad
};

// Source rows and columns of the th x tw output tile at (oh0, ow0), halo
// included, into LDS; zero where the image ends.
template <int CIN>
__device__ __forceinline__ void sn_stage_x(const SnArgs& a, int n, int oh0,
                                           int ow0, unsigned short* lds,
                                           int pitch) {
    const int nrows = (a.th - 1) * a.stride + 3;
    const int rowel = ((a.tw - 1) * a.stride + 3) * CIN;
    const int ih0 = oh0 * a.stride - 1;
    const int e0 = (ow0 * a.stride - 1) * CIN;   // element of the image row
    const int wel = a.W * CIN;
    for (int rr = 0; rr < nrows; ++rr) {
        const int ih = ih0 + rr;
        const bool rok = ih >= 0 && ih < a.H;
        const unsigned short* src =
            a.x + ((long)n * a.H + (rok ? ih : 0)) * wel;
        for (int e = threadIdx.x; e < rowel; e += SN_THREADS) {
            const int ge = e0 + e;
            unsigned short v = 0;
            if (rok && ge >= 0 && ge < wel) v = src[ge];
            lds[rr * pitch + e] = v;
        }
    }
}

// ---- forward ----------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(SN_THREADS)
void conv_stem_narrow_fwd_kernel(const SnArgs a) {
    __shared__ __align__(16) unsigned short sn_x[SN_X_ELEMS];
    constexpr int RED = 9 * CIN;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;

    int b = blockIdx.x;
    const int tx = b % a.tiles_w;  b /= a.tiles_w;
    const int ty = b % a.tiles_h;
    const int n = b / a.tiles_h;
    const int oh0 = ty * a.th, ow0 = tx * a.tw;
    const int pitch = sn_pitch(((a.tw - 1) * a.stride + 3) * CIN);

    sn_stage_x<CIN>(a, n, oh0, ow0, sn_x, pitch);

    // ---- prologue: the A fragments of every 16-row block ------------------
    const int nbv = (a.K + 15) >> 4;
    sn_short8 wr[4];
    #pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int o = nb * 16 + fr;
        sn_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = fq * 8 + e;
            if (o < a.K && j < RED) v[e] = (short)a.w[o * RED + j];
        }
        wr[nb] = v;
    }
    // where reduction value 8*fq + e of a pixel lies, relative to the pixel's
    // first element in its first source row
    int off[8];
    #pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = fq * 8 + e;
        const int r = j / (3 * CIN);
        off[e] = j < RED ? r * pitch + (j - r * 3 * CIN) : -1;
    }
    __syncthreads();

    const int upr = a.tw >> 4;            // 16-pixel tiles per tile row
    const int nunits = a.th * upr;
    for (int u = wid; u < nunits; u += SN_WAVES) {
        const int ry = u / upr, cx = u - ry * upr;
        const int oh = oh0 + ry;
        if (oh >= a.P) break;                       // wave-uniform
        if (ow0 + cx * 16 >= a.Q) continue;         // wave-uniform
        const int ow = ow0 + cx * 16 + fr;
        const bool ok = ow < a.Q;
        const unsigned short* base =
            sn_x + ry * a.stride * pitch + (cx * 16 + fr) * a.stride * CIN;
        sn_short8 bv = {0, 0, 0, 0, 0, 0, 0, 0};
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            if (ok && off[e] >= 0) bv[e] = (short)base[off[e]];
        unsigned short* yp = a.y + (((long)n * a.P + oh) * a.Q + ow) * a.K;
        #pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            if (nb >= nbv) break;
            sn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[nb], bv, acc, 0,
                                                          0, 0);
            const int o = nb * 16 + 4 * fq;   // o % 4 == 0, K % 8 == 0
            if (ok && o < a.K) {
                uint2 q;
                q.x = (unsigned)f32_to_bf16bits(acc[0]) |
                      ((unsigned)f32_to_bf16bits(acc[1]) << 16);
                q.y = (unsigned)f32_to_bf16bits(acc[2]) |
                      ((unsigned)f32_to_bf16bits(acc[3]) << 16);
                *(uint2*)(yp + o) = q;
            }
        }
    }
}

// ---- plan -------------------------------------------------------------------
// A tile is th x tw outputs: the columns of an image go in the fewest tiles
// of at most SN_TW_MAX, evenly, in whole MFMA widths (16 pixels forward, 32
// wgrad). Forward: th = 4 rows, halved while the grid has fewer than four
// blocks per CU; a wave walks upw of the th * tw/16 MFMA tiles. wgrad: th is
// what keeps th * tw <= 256 pixels (at most 4); the (image, tile) units go
// in as many chunks as give every CU three blocks, and past SN_FOLD1 slabs
// the fold runs in two levels as in conv_pw.hip: nch is rounded up to g * s
// with g = ceil(sqrt(nch)), the chunks past the last unit store zeros.
ConvStemNarrowPlan conv_stem_narrow_plan(int N, int H, int W, int Cin, int K,
                                         int stride, int mode) {
    (void)Cin;  (void)K;
    ConvStemNarrowPlan p = {};
    const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
    const int mw = mode == CONV_STEM_NARROW_WGRAD ? 32 : 16;
    p.tiles_w = (Q + SN_TW_MAX - 1) / SN_TW_MAX;
    p.tw = ((Q + p.tiles_w - 1) / p.tiles_w + mw - 1) / mw * mw;
    p.nch = 1;
    p.fold_g = 1;
    if (mode == CONV_STEM_NARROW_WGRAD) {
        p.th = SN_WG_PIX / p.tw < SN_TH_MAX ? SN_WG_PIX / p.tw : SN_TH_MAX;
        p.tiles_h = (P + p.th - 1) / p.th;
        const long units = (long)N * p.tiles_h * p.tiles_w;
        long nch = units < 3L * SN_CUS ? units : 3L * SN_CUS;
        const long upc = (units + nch - 1) / nch;
        nch = (units + upc - 1) / upc;
        p.upc = (int)upc;
        p.nch = (int)nch;
        if (p.nch > SN_FOLD1) {
            int g = 1;
            while (g * g < p.nch) ++g;
            p.fold_g = g;
            p.nch = g * ((p.nch + g - 1) / g);
        }
        p.upw = (p.th * (p.tw / 32) + SN_WAVES - 1) / SN_WAVES;
        p.blocks = p.nch;
        return p;
    }
    p.th = SN_TH_MAX;
    while (p.th > 1 &&
           (long)N * ((P + p.th - 1) / p.th) * p.tiles_w < 4L * SN_CUS)
        p.th /= 2;
    p.tiles_h = (P + p.th - 1) / p.th;
    p.upw = (p.th * (p.tw / 16) + SN_WAVES - 1) / SN_WAVES;
    p.upc = 1;
    p.blocks = (long)N * p.tiles_h * p.tiles_w;
    return p;
}

static SnArgs sn_args(int N, int H, int W, int K, int stride,
                      const ConvStemNarrowPlan& p) {
    SnArgs a = {};
    a.N = N;  a.H = H;  a.W = W;  a.K = K;  a.stride = stride;
    a.P = (H - 1) / stride + 1;
    a.Q = (W - 1) / stride + 1;
    a.th = p.th;  a.tw = p.tw;  a.tiles_h = p.tiles_h;  a.tiles_w = p.tiles_w;
    a.nch = p.nch;  a.upc = p.upc;
    a.units = N * p.tiles_h * p.tiles_w;
    return a;
}

void conv_stem_narrow_launch(const void* x, const void* w, void* y, int N,
                             int H, int W, int Cin, int K, int stride,
                             hipStream_t stream) {
    const ConvStemNarrowPlan p =
        conv_stem_narrow_plan(N, H, W, Cin, K, stride, CONV_STEM_NARROW_FWD);
    SnArgs a = sn_args(N, H, W, K, stride, p);
    a.x = (const unsigned short*)x;
    a.w = (const unsigned short*)w;
    a.y = (unsigned short*)y;
    const dim3 grid((unsigned)p.blocks), block(SN_THREADS);
    switch (Cin) {
        case 1: hipLaunchKernelGGL(conv_stem_narrow_fwd_kernel<1>, grid, block,
                                   0, stream, a); break;
        case 2: hipLaunchKernelGGL(conv_stem_narrow_fwd_kernel<2>, grid, block,
                                   0, stream, a); break;
        default: hipLaunchKernelGGL(conv_stem_narrow_fwd_kernel<3>, grid,
                                    block, 0, stream, a); break;
    }
}

// ---- wgrad ------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(SN_THREADS)
void conv_stem_narrow_wgrad_kernel(const SnArgs a) {
    __shared__ __align__(16) unsigned short sn_x[SN_X_ELEMS];
    __shared__ __align__(16) unsigned int sn_dy[SN_DY_DWORDS];
    constexpr int RED = 9 * CIN;
    constexpr int NJT = RED > 16 ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int chunk = blockIdx.x;
    const int nbv = (a.K + 15) >> 4;
    const int G = nbv * 2;                  // 16-B granules of a staged pixel
    const int dpitch = nbv * 8 + 1;         // dwords per staged dy pixel
    const int pitch = sn_pitch(((a.tw - 1) * a.stride + 3) * CIN);
    const int sc = a.stride * CIN;          // elements between output pixels

    // this lane's patch columns: j = 16*jt + fr -> filter row r, offset o
    int boff[NJT];
    #pragma unroll
    for (int jt = 0; jt < NJT; ++jt) {
        const int j = jt * 16 + fr;
        const int r = j / (3 * CIN);
        boff[jt] = j < RED ? r * pitch + (j - r * 3 * CIN) : -1;
    }

    sn_f32x4 acc[4][NJT];
    #pragma unroll
    for (int nb = 0; nb < 4; ++nb)
        #pragma unroll
        for (int jt = 0; jt < NJT; ++jt)
            acc[nb][jt] = sn_f32x4{0.f, 0.f, 0.f, 0.f};

    const int spr = a.tw >> 5;              // 32-pixel steps per tile row
    const int nsteps = a.th * spr;
    const int npix = a.th * a.tw;
    const int u_beg = chunk * a.upc;
    const int u_end = min(a.units, u_beg + a.upc);
    for (int u = u_beg; u < u_end; ++u) {
        int t = u;
        const int tx = t % a.tiles_w;  t /= a.tiles_w;
        const int ty = t % a.tiles_h;
        const int n = t / a.tiles_h;
        const int oh0 = ty * a.th, ow0 = tx * a.tw;
        __syncthreads();   // the previous unit's reads are done
        sn_stage_x<CIN>(a, n, oh0, ow0, sn_x, pitch);
        for (int i = threadIdx.x; i < npix * G; i += SN_THREADS) {
            const int pix = i / G, g = i - pix * G;
            const int ry = pix / a.tw, px = pix - ry * a.tw;
            const int oh = oh0 + ry, ow = ow0 + px;
            uint4 v = {0u, 0u, 0u, 0u};
            if (oh < a.P && ow < a.Q && g * 8 < a.K)
                v = *(const uint4*)(a.dy +
                                    (((long)n * a.P + oh) * a.Q + ow) * a.K +
                                    g * 8);
            unsigned int* d = sn_dy + pix * dpitch + g * 4;
            d[0] = v.x;  d[1] = v.y;  d[2] = v.z;  d[3] = v.w;
        }
        __syncthreads();
        const unsigned short* ldy = (const unsigned short*)sn_dy;
        for (int st = wid; st < nsteps; st += SN_WAVES) {
            const int ry = st / spr, cx = st - ry * spr;
            if (oh0 + ry >= a.P) break;                  // wave-uniform
            if (ow0 + cx * 32 >= a.Q) continue;          // wave-uniform
            const int p0 = cx * 32 + fq * 8;             // first of 8 pixels
            sn_short8 bv[NJT];
            #pragma unroll
            for (int jt = 0; jt < NJT; ++jt) {
                const unsigned short* bp =
                    sn_x + ry * a.stride * pitch + p0 * sc + boff[jt];
                sn_short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                #pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (boff[jt] >= 0 && ow0 + p0 + e < a.Q)
                        v[e] = (short)bp[e * sc];
                bv[jt] = v;
            }
            const unsigned short* ap =
                ldy + (ry * a.tw + p0) * dpitch * 2 + fr;
            #pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                if (nb >= nbv) break;
                sn_short8 av;
                #pragma unroll
                for (int e = 0; e < 8; ++e)
                    av[e] = (short)ap[e * dpitch * 2 + nb * 16];
                #pragma unroll
                for (int jt = 0; jt < NJT; ++jt)
                    acc[nb][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        av, bv[jt], acc[nb][jt], 0, 0, 0);
            }
        }
    }

    // ---- the four waves' tiles meet in LDS, added in wave order ----------
    __syncthreads();
    float* fold = (float*)sn_dy;            // [wave][nb][jt][v][lane]
    #pragma unroll
    for (int nb = 0; nb < 4; ++nb)
        #pragma unroll
        for (int jt = 0; jt < NJT; ++jt)
            #pragma unroll
            for (int v = 0; v < 4; ++v)
                fold[wid * 2048 + (nb * 2 + jt) * 256 + v * 64 + lane] =
                    acc[nb][jt][v];
    __syncthreads();
    // D[i = 4*fq + v][j = fr]: dw row 16*nb + i, column 16*jt + j
    float* o = a.ws + (a.nch > 1 ? (long)chunk * a.K * RED : 0);
    for (int idx = threadIdx.x; idx < 2048; idx += SN_THREADS) {
        const int nb = idx >> 9, jt = (idx >> 8) & 1, v = (idx >> 6) & 3;
        const int ln = idx & 63;
        const int k = nb * 16 + 4 * (ln >> 4) + v;
        const int j = jt * 16 + (ln & 15);
        if (jt < NJT && k < a.K && j < RED)
            o[k * RED + j] = ((fold[idx] + fold[2048 + idx]) +
                              fold[4096 + idx]) + fold[6144 + idx];
    }
}

void conv_stem_narrow_wgrad_launch(const void* dy, const void* x, float* ws,
                                   int N, int H, int W, int Cin, int K,
                                   int stride, hipStream_t stream) {
    const ConvStemNarrowPlan p =
        conv_stem_narrow_plan(N, H, W, Cin, K, stride, CONV_STEM_NARROW_WGRAD);
    SnArgs a = sn_args(N, H, W, K, stride, p);
    a.dy = (const unsigned short*)dy;
    a.x = (const unsigned short*)x;
    a.ws = ws;
    const dim3 grid((unsigned)p.nch), block(SN_THREADS);
    switch (Cin) {
        case 1: hipLaunchKernelGGL(conv_stem_narrow_wgrad_kernel<1>, grid,
                                   block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(conv_stem_narrow_wgrad_kernel<2>, grid,
                                   block, 0, stream, a); break;
        default: hipLaunchKernelGGL(conv_stem_narrow_wgrad_kernel<3>, grid,
                                    block, 0, stream, a); break;
    }
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
