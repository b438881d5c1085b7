// Implicit-GEMM 2D convolution for gfx950 (CDNA4), NHWC bf16.
//
// MI355X-native replacement for the conv layer the reference gets for free
// from cuDNN via NNlibCUDA (Flux conv):
// hand-written MFMA kernels — v_mfma_f32_16x16x32_bf16 tiles, LDS staging
// via global_load_lds (direct HBM->LDS DMA), source-side XOR swizzle for
// bank-conflict-free ds_read_b128 fragment reads (guide T2 / rule 21),
// double-buffered with the staging DMA in flight across the compute phase.
//
// GEMM view (forward):
//   M = N*P*Q output pixels, Nd = K output channels, Kd = R*S*C
//   y[m][k] = sum_kd A[m][kd] * B[kd][k]
//   A = im2col gather of x (never materialized: the per-lane source
//       addresses of the LDS DMA do the gather; out-of-bounds rows read a
//       16-B zero page)
//   B = w[k][r][s][c] (torch channels_last conv weight = [K][R*S*C] rows)
//
// DGRAD: dx[n,h,w,c] = sum_{r,s,k} dy[n,(h+py-r)/sy,(w+px-s)/sx,k]*w[k,r,s,c].
// For stride > 1 the output pixels are partitioned by (h%sy, w%sx) parity
// class (blockIdx.z); each class iterates only its own valid filter taps,
// so no MFMA work is spent on divisibility-masked zero rows (a 4x saving
// for 3x3 stride-2). B = pre-transposed weights wt[rs*C + c][k]
// (k-contiguous rows).
//
// Tile geometry (templated; wave tile fixed at 64x64 = 4x4 fragments of
// 16x16 so every config runs 32 MFMAs per K-step per wave — the
// MFMA-per-glds ratio is what sets throughput, guide §5 ladder):
//   OC % 128 == 0 : BM=128 x BN=128, 4 waves as 2x2, LDS 2x32 KiB
//   OC % 128 != 0 : BM=256 x BN=64,  4 waves as 4x1, LDS 2x40 KiB
// Each tile has a second config for grids big enough to fill it: BK=32
// K-steps on a 3-buffer counted ring (3x16 KiB at 3 blocks/CU, 3x20 KiB at
// 2). Tile, ring and split-K are decided in one place, conv_igemm_plan
// (a ConvPlan from a ConvGeom and a mode): conv_dispatch obeys it and the
// bindings size their workspaces from it. Kernels in this file: conv_igemm_kernel
// fwd+dgrad x 2 tiles x {BK64 2-buf, BK32 3-ring} (8) + the stem (1), the
// four fwd configs and the stem once more with the inference epilogue
// (EpiInfer: eval BN + residual + ReLU before the single bf16 round),
// conv_wgrad_kernel FT2 / FT2-stem / FT4 (3) and FT2 / FT4 once more with
// the slab epilogue (2), conv_skcombine_kernel (plain
// and EpiInfer), wt_transpose_kernel. Variants that were measured and rejected are
// recorded in profiles/ab_conv8.md, profiles/ab_bigtile.md and
// docs/wgrad_study.md, not kept here.
// fp32 accumulate, bf16 store. Staging source offsets advance
// incrementally within a filter tap (full address math only on tap
// changes). The fwd epilogue can also emit per-channel sum/sumsq
// partials of the rounded output for the downstream BatchNorm (`stats`),
// and small-M deep-K shapes split the K loop over blockIdx.z into fp32
// partials (`skpart`) folded by conv_skcombine_kernel — layer4-sized
// grids otherwise fill only ~30% of the 256 CUs. A non-split-K dgrad
// stores dx (and reads the deferred junction gradient `accsrc`) through
// the LDS staging of the inference epilogue, 16 B per lane; the forward
// and stem training epilogues stay in fragment order, since they read
// nothing and take their stats from the fragment registers
// (profiles/step_profile_r4.md).
//
// This file also contains: the CONV_STEM mode (small-C stems on a
// channel-padded C=8 image, r-only tap loop), the wgrad kernel
// (reduction along the pixel axis via ds_read_tr16_b64 hardware
// transpose reads from an m4-grouped LDS image, window positions
// permuted for bank-conflict-free half-wave reads, chunks accumulated with
// fp32 atomics or stored as per-chunk fp32 slabs for an ordered fold,
// profiles/wgrad_slab.md), and the batched weight transposer for the dgrad B
// layout. The wgrad grid is 1-D: a block id maps through an XCD-contiguous
// logical id, pixel chunk slowest, to (k-tile, c-tile, tap, chunk)
// (wgrad_block_coords, fda_kernels.h), so the blocks that stage one
// chunk's dy and x tiles run back to back behind one XCD's L2; and
// conv_wgrad_plan sizes the chunks so the grid is one resident wave of
// blocks (profiles/wgrad_raster.md).
//
// Constraints (host wrapper): staged reduction channels (C fwd / K dgrad)
// and output channels multiples of 64, dilation 1, groups 1; everything
// else (grouped/dilated convs) falls back to the library path.

#include <hip/hip_runtime.h>
#include <cassert>
#include <cstdlib>
#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

__device__ __align__(16) static const unsigned short conv_zero16[8] = {0};

#define FDA_GLDS16(gptr, lptr)                                              \
    __builtin_amdgcn_global_load_lds(                                       \
        (const __attribute__((address_space(1))) void*)(gptr),              \
        (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

// CONV_STEM: small-C stem conv on a channel-padded (C=8) pre-padded input.
// Taps are r-only: each K-step covers one filter row r as 64 virtual
// channels = 8 pixels (s=0..7, s==7 zero-padded in wpad) x 8 channels
// (c>=3 zero). B reads wpad[k][r][64]; A granules are whole 16-B pixels.

constexpr int BK = 64;

// The inference epilogue (EpiInfer, fda_kernels.h) is passed to
// conv_igemm_kernel / conv_skcombine_kernel as the optional trailing EPI
// argument; the training instantiations pass none, so their code and
// argument lists are those of a kernel without it.
template <class E>
__device__ __forceinline__ const E& epi_of(const E& e) { return e; }

// NW = waves per block = (BM/64)*(BN/64): 4 for both the 128x128 and the
// 256x64 config (256 threads, at least 2 blocks/CU).
template <int MODE, int BM, int BN, int WN, int NBUF = 2, int BKT = BK,
          class... EPI>
__global__ __launch_bounds__((BM / 64) * (BN / 64) * 64,
                             512 / ((BM / 64) * (BN / 64) * 64))
void conv_igemm_kernel(
    const unsigned short* __restrict__ src,
    const unsigned short* __restrict__ wgt,
    unsigned short* __restrict__ out,
    int N, int H, int W, int C,
    int K, int P, int Q,
    int R, int S, int sy, int sx, int py, int px,
    float* __restrict__ stats, /* [mtiles][2][OC] or null: per-channel
                                 sum/sumsq of the rounded output — feeds the
                                 BN reduce+finalize directly (the separate
                                 bn_stats read pass is skipped) */
    float* __restrict__ skpart, /* split-K: fp32 partial output
                                 [SK][M][OC], reduced by
                                 conv_skcombine_kernel. Small-M late layers
                                 fill only ~30% of the chip otherwise. */
    int SK,
    const unsigned short* __restrict__ accsrc
        /* non-null (dgrad): bf16 tensor with the OUTPUT's layout added into
           the result before the store — the residual-junction grad
           (d/d identity) fused into dx so autograd's separate
           CUDAFunctor_add pass disappears (ops/conv.py junction stash) */
    ,
    EPI... epi /* none (training) or one EpiInfer (fwd/stem inference) */
    ) {
    static_assert(sizeof...(EPI) <= 1, "at most one epilogue functor");
    constexpr bool FUSED = sizeof...(EPI) == 1;
    static_assert(!FUSED || MODE != CONV_DGRAD, "inference epilogue is fwd");
    constexpr int NW = (BM / 64) * (BN / 64);   // waves per block
    constexpr int A_ELEMS = BM * BKT;
    constexpr int B_ELEMS = BN * BKT;
    constexpr int BUF_ELEMS = A_ELEMS + B_ELEMS;
    // one glds = 64 lanes x 16 B = 512/BKT rows of BKT elements
    constexpr int RPG = 512 / BKT;       // rows per glds (8 @64, 16 @32)
    constexpr int GPR = BKT / 8;         // 16-B granules per row (8 / 4)
    constexpr int KH = BKT / 32;         // mfma k-halves per staged tile
    // granule swizzle: BK64 keeps the proven row&7; BK32 folds row>>2 in
    // (plain row&3 repeats banks every 4 rows: 4-way b128 conflicts; the
    // fold reaches the 2-way floor of 4 slots over 8 same-phase rows)
    auto swz = [](int row) {
        return BKT == 64 ? (row & 7) : ((row ^ (row >> 2)) & (GPR - 1));
    };
    constexpr int AI = BM / (RPG * NW);  // A glds per wave per tile
    constexpr int BI = BN / (RPG * NW);  // B glds per wave per tile

    const int OC = (MODE == CONV_DGRAD) ? C : K;
    const int RC = (MODE == CONV_FWD) ? C : ((MODE == CONV_STEM) ? 64 : K);

    int a = 0, b = 0, OH, OW, r0 = 0, s0 = 0, nR = R, nS = S;
    int sk = 0, zrest = blockIdx.z;
    if (SK > 1) { sk = zrest % SK; zrest /= SK; }
    if (MODE != CONV_DGRAD) {
        OH = P; OW = Q;
        if (MODE == CONV_STEM) nS = 1;   // taps iterate r only
    } else {
        a = zrest / sx;  b = zrest % sx;
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
    const int wm = wid / WN;             // wave row (64-pixel granularity)
    const int wn = wid % WN;             // wave col (64-channel granularity)

    extern __shared__ unsigned short lds[];   // [NBUF][BUF_ELEMS]
    constexpr int GPW = AI + BI;              // glds per wave per tile

    // ---- per-lane staging descriptors ------------------------------------
    int a_row[AI];
    long a_pix[AI];
    int a_hb[AI], a_wb[AI];
    bool a_mok[AI];
    const int cslot = lane % GPR;
    #pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int row = (wid * AI + i) * RPG + lane / GPR;
        a_row[i] = row;
        const long m = m0 + row;
        const bool mok = m < M;
        const long mm = mok ? m : 0;
        const int ow = (int)(mm % OW);
        const int oh = (int)((mm / OW) % OH);
        const int n = (int)(mm / ((long)OW * OH));
        a_mok[i] = mok;
        if (MODE == CONV_STEM) {
            a_hb[i] = oh * sy;           // input pre-padded: no -py
            a_wb[i] = ow * sx;
            a_pix[i] = ((long)n * H) * W * 8;
        } else if (MODE == CONV_FWD) {
            a_hb[i] = oh * sy - py;
            a_wb[i] = ow * sx - px;
            a_pix[i] = ((long)n * H) * W * C;
        } else {
            a_hb[i] = oh + (a + py) / sy;
            a_wb[i] = ow + (b + px) / sx;
            a_pix[i] = ((long)n * P) * Q * K;
        }
    }
    int b_row[BI];
    #pragma unroll
    for (int i = 0; i < BI; ++i)
        b_row[i] = (wid * BI + i) * RPG + lane / GPR;

    const int cblocks = RC / BKT;
    const int T = nR * nS * cblocks;

    // Incremental staging offsets: stage() is called with strictly
    // increasing `it` (prologue, then it+NBUF-1), so within one filter tap
    // the source offsets just advance by BK; the full per-row address math
    // (multiply + bounds check) runs only on tap changes — it was
    // comparable to the whole MFMA phase per K-step otherwise.
    long a_goff[AI];
    bool a_okc[AI];
    long b_goff[BI];
    int last_rsi = -1;
    auto stage = [&](int buf, int it) {
        const int rsi = it / cblocks;
        const int ri = rsi / nS, si = rsi % nS;
        unsigned short* base = lds + buf * BUF_ELEMS;
        if (rsi != last_rsi) {
            last_rsi = rsi;
            const int cb = (it % cblocks) * BKT;  // 0 except NBUF>1 prologue
            #pragma unroll
            for (int i = 0; i < AI; ++i) {
                const int cs = (cslot ^ swz(a_row[i])) * 8;
                bool ok = a_mok[i];
                long off = 0;
                if (MODE == CONV_STEM) {
                    off = a_pix[i] + ((long)(a_hb[i] + ri) * W + a_wb[i]) * 8 + cs;
                } else if (MODE == CONV_FWD) {
                    const int h = a_hb[i] + ri, w = a_wb[i] + si;
                    ok = ok && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
                    off = a_pix[i] + ((long)h * W + w) * C + cb + cs;
                } else {
                    const int p = a_hb[i] - ri, q = a_wb[i] - si;
                    ok = ok && (unsigned)p < (unsigned)P && (unsigned)q < (unsigned)Q;
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
                const int row = b_row[i];
                const int cs = (cslot ^ swz(row)) * 8;
                if (MODE == CONV_STEM)
                    b_goff[i] = ((long)(n0 + row) * R + ri) * 64 + cs;
                else if (MODE == CONV_FWD)
                    b_goff[i] = (long)(n0 + row) * R * S * C + (long)rs * C + cb + cs;
                else
                    b_goff[i] = (long)((long)rs * C + n0 + row) * K + cb + cs;
            }
        } else {
            #pragma unroll
            for (int i = 0; i < AI; ++i) a_goff[i] += BKT;
            #pragma unroll
            for (int i = 0; i < BI; ++i) b_goff[i] += BKT;
        }
        #pragma unroll
        for (int i = 0; i < AI; ++i) {
            const unsigned short* sp = a_okc[i] ? src + a_goff[i] : conv_zero16;
            FDA_GLDS16(sp, base + (wid * AI + i) * RPG * BKT);
        }
        #pragma unroll
        for (int i = 0; i < BI; ++i) {
            FDA_GLDS16(wgt + b_goff[i],
                       base + A_ELEMS + (wid * BI + i) * RPG * BKT);
        }
    };

    // ---- fragment read offsets (elements into an lds buffer) -------------
    int a_off[4][KH], b_off[4][KH];
    {
        const int fr = lane & 15, fq = lane >> 4;
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                const int row = wm * 64 + mi * 16 + fr;
                const int slot = ((kh * 4 + fq) ^ swz(row)) & (GPR - 1);
                a_off[mi][kh] = row * BKT + slot * 8;
            }
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni)
            #pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                const int row = wn * 64 + ni * 16 + fr;
                const int slot = ((kh * 4 + fq) ^ swz(row)) & (GPR - 1);
                b_off[ni][kh] = A_ELEMS + row * BKT + slot * 8;
            }
    }

    floatx4 acc[4][4];
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop: double buffer; tile t+1's DMA in flight over tile t's
    // compute, drained at the iteration boundary (guide T3 minimum form) ---
    int it0 = 0, itN = T;
    if (SK > 1) {
        const int chunk = (T + SK - 1) / SK;
        it0 = sk * chunk;
        itN = it0 + chunk < T ? it0 + chunk : T;
        if (it0 >= itN) itN = it0;       // empty slice: epilogue writes 0
    }
    if (it0 < itN) stage(it0 % NBUF, it0);
    if (NBUF > 2 && it0 + 1 < itN) stage((it0 + 1) % NBUF, it0 + 1);
    for (int it = it0; it < itN; ++it) {
        // tile `it` landed chip-wide: each wave drains its own DMA, the
        // barrier joins all waves. This is the loop's ONLY barrier — the
        // next K-step's staging targets the buffer every wave finished
        // reading before it arrived here. With NBUF==3 the counted wait
        // leaves tile it+1's DMA in flight across the barrier (T4).
        if (NBUF > 2 && it + 1 < itN) {
            static_assert(NBUF == 2 || GPW == 4 || GPW == 5,
                          "counted ring: state the vmcnt for this GPW");
            if constexpr (GPW == 4)
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        // stage-before-reads: tried the other order in r2 (reads first so
        // their latency hides under stage's address math) — measured
        // +314 us/step on fwd+dgrad: delaying the glds issue shrinks the
        // DMA's flight window over the MFMA phase, which costs more than
        // the lgkm stall it saves. (The wgrad kernel is the opposite case:
        // hipcc force-drains DMA before tr16 reads, so there reads-first
        // is required — see conv_wgrad_kernel.)
        if (it + NBUF - 1 < itN) stage((it + NBUF - 1) % NBUF, it + NBUF - 1);
        const unsigned short* buf = lds + (it % NBUF) * BUF_ELEMS;
        short8 af[4][KH], bf[4][KH];
        #pragma unroll
        for (int kh = 0; kh < KH; ++kh) {
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi][kh] = *(const short8*)(buf + a_off[mi][kh]);
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                bf[ni][kh] = *(const short8*)(buf + b_off[ni][kh]);
        }
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int kh = 0; kh < KH; ++kh)
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi][kh], bf[ni][kh], acc[mi][ni], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        // no end-of-iteration barrier: the next iteration's vmcnt + top
        // barrier already orders buffer reuse (a wave reaches that barrier
        // only after its lgkm-waited fragment reads of this buffer), and
        // the final iteration needs no sync before the epilogue.
    }

    // ---- epilogue: C/D map col=lane&15, row=(lane>>4)*4+j ----------------
    const int fcol = lane & 15, frow0 = (lane >> 4) * 4;
    float ssum[4] = {0.f, 0.f, 0.f, 0.f};   // per-ni channel sums (rounded y)
    float sq[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (FUSED) {
        // y = bf16(relu(affine(acc) + residual)), LDS-staged: the wave's
        // 64x64 fp32 tile goes through the staging LDS in two 32-row
        // passes (34 KiB per block, inside every config's allocation), then
        // every lane handles 8 consecutive channels of a row: 16-B residual
        // read, 16-B store. Row stride 68 floats: the four rows a fragment
        // write touches land on distinct 16-bank groups. (Storing in
        // fragment order, 2 B per lane, measured slower on every shape and
        // slower than the unfused pair with a residual:
        // profiles/infer_fused.md.)
        const auto& e = epi_of(epi...);
        constexpr int SROW = 68;
        static_assert(NW * 32 * SROW * 4 <= NBUF * BUF_ELEMS * 2,
                      "staging passes must fit the block's own LDS");
        float* st = (float*)lds + wid * (32 * SROW);
        const int cg = lane & 7, rr = lane >> 3;
        const int cbase = n0 + wn * 64 + cg * 8;
        const float4 s0 = *(const float4*)(e.scale + cbase);
        const float4 s1 = *(const float4*)(e.scale + cbase + 4);
        const float4 h0 = *(const float4*)(e.shift + cbase);
        const float4 h1 = *(const float4*)(e.shift + cbase + 4);
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        #pragma unroll
        for (int half = 0; half < 2; ++half) {
            // every wave has read its last fragments (first pass) / its
            // staged rows (second pass) before the LDS is overwritten
            __syncthreads();
            #pragma unroll
            for (int mi2 = 0; mi2 < 2; ++mi2)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    #pragma unroll
                    for (int j = 0; j < 4; ++j)
                        st[(mi2 * 16 + frow0 + j) * SROW + ni * 16 + fcol] =
                            acc[half * 2 + mi2][ni][j];
            __syncthreads();
            #pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int lr = it * 8 + rr;
                const long m = m0 + wm * 64 + half * 32 + lr;
                if (m >= M) continue;
                const float* sp = st + lr * SROW + cg * 8;
                const float4 a0 = *(const float4*)sp;
                const float4 a1 = *(const float4*)(sp + 4);
                float v[8] = {a0.x, a0.y, a0.z, a0.w,
                              a1.x, a1.y, a1.z, a1.w};
                const long o = m * OC + cbase;
                float rf[8];
                if (e.residual)
                    unpack_f32<unsigned short, 8>(
                        *(const uint4*)(e.residual + o), rf);
                unsigned short ov[8];
                #pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float t = bn_affine(v[k], sc[k], sh[k]);
                    if (e.residual) t += rf[k];
                    if (e.relu) t = fmaxf(t, 0.f);
                    ov[k] = f32_to_bf16bits(t);
                }
                *(uint4*)(out + o) = *(uint4*)ov;
            }
        }
        return;
    }
    if constexpr (MODE == CONV_DGRAD) {
        if (skpart == nullptr) {
            // dx = bf16(acc + accsrc), staged through the LDS exactly like
            // the inference epilogue above (two 32-row passes, row stride
            // 68 floats): every lane then owns 8 consecutive channels of a
            // row, reads the deferred junction grad as one 16-B load and
            // stores 16 B. Per element the arithmetic is that of the
            // fragment-order form it replaces (one fp32 add, one round),
            // so dx is bit-identical to it. The row's pixel address is
            // computed per row, which is all the stride-2 parity classes
            // need; a class with no filter tap (1x1 stride 2) stores its
            // zeros 16 B at a time.
            constexpr int SROW = 68;
            static_assert(NW * 32 * SROW * 4 <= NBUF * BUF_ELEMS * 2,
                          "staging passes must fit the block's own LDS");
            float* st = (float*)lds + wid * (32 * SROW);
            const int cg = lane & 7, rr = lane >> 3;
            const int cbase = n0 + wn * 64 + cg * 8;
            #pragma unroll
            for (int half = 0; half < 2; ++half) {
                // every wave has read its last fragments (first pass) / its
                // staged rows (second pass) before the LDS is overwritten
                __syncthreads();
                #pragma unroll
                for (int mi2 = 0; mi2 < 2; ++mi2)
                    #pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
                        #pragma unroll
                        for (int j = 0; j < 4; ++j)
                            st[(mi2 * 16 + frow0 + j) * SROW + ni * 16 + fcol] =
                                acc[half * 2 + mi2][ni][j];
                __syncthreads();
                #pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int lr = it * 8 + rr;
                    const long m = m0 + wm * 64 + half * 32 + lr;
                    if (m >= M) continue;
                    const int ww = (int)(m % OW);
                    const int hh = (int)((m / OW) % OH);
                    const int n = (int)(m / ((long)OW * OH));
                    const long o = (((long)n * H + a + (long)sy * hh) * W + b +
                                    (long)sx * ww) * C + cbase;
                    const float* sp = st + lr * SROW + cg * 8;
                    const float4 a0 = *(const float4*)sp;
                    const float4 a1 = *(const float4*)(sp + 4);
                    float v[8] = {a0.x, a0.y, a0.z, a0.w,
                                  a1.x, a1.y, a1.z, a1.w};
                    if (accsrc != nullptr) {
                        float rf[8];
                        unpack_f32<unsigned short, 8>(
                            *(const uint4*)(accsrc + o), rf);
                        #pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] += rf[k];
                    }
                    unsigned short ov[8];
                    #pragma unroll
                    for (int k = 0; k < 8; ++k) ov[k] = f32_to_bf16bits(v[k]);
                    *(uint4*)(out + o) = *(uint4*)ov;
                }
            }
            return;
        }
    }
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long m = m0 + wm * 64 + mi * 16 + frow0 + j;
            if (m >= M) continue;
            const long obase = m * OC;
            if (skpart != nullptr) {
                // split-K: fp32 partials, linear by m (the dgrad split path
                // is stride-1 only, where its pixel offset is m*OC too)
                float* prow = skpart + ((long)sk * M + m) * OC + n0 + wn * 64;
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    prow[ni * 16 + fcol] = acc[mi][ni][j];
                continue;
            }
            // fwd / stem only from here on: a non-split dgrad left above.
            // Fragment order, 2 B per lane: these read nothing, and their
            // stats come straight from the fragment registers.
            if constexpr (MODE != CONV_DGRAD) {
                unsigned short* orow = out + obase + n0 + wn * 64;
                const unsigned short* arow =
                    accsrc ? accsrc + obase + n0 + wn * 64 : nullptr;
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    float v = acc[mi][ni][j];
                    if (arow) v += bf16bits_to_f32(arow[ni * 16 + fcol]);
                    const unsigned short us = f32_to_bf16bits(v);
                    orow[ni * 16 + fcol] = us;
                    if (stats != nullptr) {
                        const float v = bf16bits_to_f32(us);
                        ssum[ni] += v;
                        sq[ni] += v * v;
                    }
                }
            }
        }
    }

    if (MODE != CONV_DGRAD && stats != nullptr) {
        // fold the four 16-row lane groups, then the waves sharing this
        // channel column, then write this m-tile's [2][OC] partial slice
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            #pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                ssum[ni] += __shfl_xor(ssum[ni], off, 64);
                sq[ni] += __shfl_xor(sq[ni], off, 64);
            }
        }
        float* sf = (float*)lds;             // staging LDS is free now
        __builtin_amdgcn_s_barrier();
        if ((lane >> 4) == 0) {
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                sf[(wid * 4 + ni) * 16 + fcol] = ssum[ni];
                sf[NW * 64 + (wid * 4 + ni) * 16 + fcol] = sq[ni];
            }
        }
        __builtin_amdgcn_s_barrier();
        if (wm == 0 && (lane >> 4) == 0) {
            float* prow = stats + (long)blockIdx.x * 2 * OC + n0 + wn * 64;
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                float s = ssum[ni], z = sq[ni];
                for (int w2 = wid + WN; w2 < NW; w2 += WN) {
                    s += sf[(w2 * 4 + ni) * 16 + fcol];
                    z += sf[NW * 64 + (w2 * 4 + ni) * 16 + fcol];
                }
                prow[ni * 16 + fcol] = s;
                prow[OC + ni * 16 + fcol] = z;
            }
        }
    }
}

template <int MODE, int BM, int BN, int WN, int NBUF = 2, int BKT = BK,
          class... EPI>
static void launch_cfg(const void* src, const void* wgt, void* out,
                       const ConvGeom& g, int SK, hipStream_t stream,
                       float* stats, float* skpart, const void* accsrc,
                       EPI... epi) {
    constexpr ConvMode mode = (ConvMode)MODE;
    constexpr unsigned NTHREADS = (BM / 64) * (BN / 64) * 64;
    dim3 grid((unsigned)((g.rows(mode) + BM - 1) / BM),
              (unsigned)(g.oc(mode) / BN), (unsigned)(g.classes(mode) * SK));
    const size_t shmem = NBUF * (BM * BKT + BN * BKT) * sizeof(unsigned short);
    if (shmem > 65536) {
        static bool raised = [] {
            hipFuncSetAttribute(
                (const void*)&conv_igemm_kernel<MODE, BM, BN, WN, NBUF, BKT,
                                                EPI...>,
                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            return true;
        }();
        (void)raised;
    }
    hipLaunchKernelGGL((conv_igemm_kernel<MODE, BM, BN, WN, NBUF, BKT, EPI...>),
                       grid, dim3(NTHREADS), shmem, stream,
                       (const unsigned short*)src,
                       (const unsigned short*)wgt, (unsigned short*)out,
                       g.N, g.H, g.W, g.C, g.K, g.P, g.Q, g.R, g.S, g.sy,
                       g.sx, g.py, g.px, stats, skpart, SK,
                       (const unsigned short*)accsrc, epi...);
}

// ---- split-K combine: y = bf16(sum_sk part) (+ BN stats partials) --------
// EPI as in conv_igemm_kernel: with one EpiInfer the folded fp32 sum goes
// through the inference epilogue before its single bf16 round.
template <class... EPI>
__global__ __launch_bounds__(256) void conv_skcombine_kernel(
    const float* __restrict__ part, unsigned short* __restrict__ y,
    float* __restrict__ stats, long M, int OC, int SK,
    const unsigned short* __restrict__ accsrc, EPI... epi) {
    static_assert(sizeof...(EPI) <= 1, "at most one epilogue functor");
    __shared__ float smem[2048];          // 256 threads x 8 lanes
    const int V = 8;
    const int tpr = OC / V;               // threads per row (OC <= 2048)
    const int rpb = 256 / tpr;
    const int lane_c = threadIdx.x % tpr;
    const int sub_r = threadIdx.x / tpr;
    const int c0 = lane_c * V;
    float s[V], q[V];
    #pragma unroll
    for (int k = 0; k < V; ++k) s[k] = q[k] = 0.f;
    for (long r = (long)blockIdx.x * rpb + sub_r; r < M;
         r += (long)gridDim.x * rpb) {
        float v[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) v[k] = 0.f;
        for (int z = 0; z < SK; ++z) {
            const float* p = part + ((long)z * M + r) * OC + c0;
            float4 a = *(const float4*)p;
            float4 b = *(const float4*)(p + 4);
            v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
            v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
        }
        if constexpr (sizeof...(EPI) == 1) {
            const auto& e = epi_of(epi...);
            const float4 s0 = *(const float4*)(e.scale + c0);
            const float4 s1 = *(const float4*)(e.scale + c0 + 4);
            const float4 h0 = *(const float4*)(e.shift + c0);
            const float4 h1 = *(const float4*)(e.shift + c0 + 4);
            const float sc[V] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            const float sh[V] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
            float rf[V];
            if (e.residual != nullptr)
                unpack_f32<unsigned short, V>(
                    *(const uint4*)(e.residual + r * OC + c0), rf);
            unsigned short o[V];
            #pragma unroll
            for (int k = 0; k < V; ++k) {
                float t = bn_affine(v[k], sc[k], sh[k]);
                if (e.residual != nullptr) t += rf[k];
                if (e.relu) t = fmaxf(t, 0.f);
                o[k] = f32_to_bf16bits(t);
            }
            *(uint4*)(y + r * OC + c0) = *(uint4*)o;
            continue;
        }
        if (accsrc != nullptr) {
            unsigned short av[V];
            *(uint4*)av = *(const uint4*)(accsrc + r * OC + c0);
            #pragma unroll
            for (int k = 0; k < V; ++k) v[k] += bf16bits_to_f32(av[k]);
        }
        unsigned short o[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            o[k] = f32_to_bf16bits(v[k]);
            if (stats != nullptr) {
                const float vr = bf16bits_to_f32(o[k]);
                s[k] += vr;
                q[k] += vr * vr;
            }
        }
        *(uint4*)(y + r * OC + c0) = *(uint4*)o;
    }
    if (stats == nullptr) return;
    // fold the rpb row-groups, write this block's [2][OC] partial slice
    float* outp = stats + (long)blockIdx.x * 2 * OC;
    #pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float* loc = pass == 0 ? s : q;
        #pragma unroll
        for (int k = 0; k < V; ++k) smem[threadIdx.x * V + k] = loc[k];
        __syncthreads();
        if (sub_r == 0) {
            float acc[V];
            #pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0.f;
            for (int rr = 0; rr < rpb; ++rr) {
                const float* sp = smem + (rr * tpr + lane_c) * V;
                #pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += sp[k];
            }
            #pragma unroll
            for (int k = 0; k < V; ++k)
                outp[pass * OC + lane_c * V + k] = acc[k];
        }
        __syncthreads();
    }
}

static int conv_skcombine_blocks(long M, int OC) {
    // OC > 2048 has no combine kernel; the bindings refuse such a plan
    const int rpb = OC <= 2048 ? 256 / (OC / 8) : 1;
    long b = (M + rpb - 1) / rpb;
    return (int)(b < 512 ? b : 512);
}

void conv_skcombine_launch(const float* part, void* y, float* stats, long M,
                           int OC, int SK, hipStream_t stream,
                           const void* accsrc, const EpiInfer* epi) {
    assert(epi == nullptr || (stats == nullptr && accsrc == nullptr));
    const dim3 grid(conv_skcombine_blocks(M, OC));
    if (epi != nullptr)
        hipLaunchKernelGGL(conv_skcombine_kernel<EpiInfer>, grid, dim3(256),
                           0, stream, part, (unsigned short*)y,
                           (float*)nullptr, M, OC, SK,
                           (const unsigned short*)nullptr, *epi);
    else
        hipLaunchKernelGGL(conv_skcombine_kernel<>, grid, dim3(256), 0,
                           stream, part, (unsigned short*)y, stats, M, OC, SK,
                           (const unsigned short*)accsrc);
}

void conv_stem_fwd_launch(const void* src, const void* wgt, void* out,
                          const ConvGeom& g, hipStream_t stream, float* stats,
                          const EpiInfer* epi) {
    if (epi != nullptr)
        launch_cfg<CONV_STEM, 256, 64, 1, 2, BK, EpiInfer>(
            src, wgt, out, g, 1, stream, nullptr, nullptr, nullptr, *epi);
    else
        launch_cfg<CONV_STEM, 256, 64, 1>(src, wgt, out, g, 1, stream, stats,
                                          nullptr, nullptr);
}

static bool conv_bk32() {
    // BK=32 x NBUF=3 rings (FLUXDIST_CONV_BK32, 0 = off, default 1 = on,
    // gated by grid fill in conv_igemm_plan). 128x128: 48 KB LDS/block -> 3
    // blocks/CU (12 waves) vs the BK64 default's 2; measured -9..-28% on
    // the big-M layer-1/2 legs, +17% on the small-M 14x14 legs (294 blocks
    // can't feed 3 blocks/CU — profiles/ab_conv8.md addendum), hence the
    // gate. 256x64: same 2 blocks/CU and 3.2:1 MFMA:glds ratio as BK64, but
    // with a second tile in flight (2 x 60 KB fits; 3 x 80 KB at BK64 never
    // did).
    static const bool v = [] {
        const char* e = getenv("FLUXDIST_CONV_BK32");
        return e ? atoi(e) != 0 : true;
    }();
    return v;
}

// The one place that decides tile geometry, split-K and ring for a conv
// launch, and with them the grid and the workspace shapes.
ConvPlan conv_igemm_plan(const ConvGeom& g, ConvMode mode) {
    const int OC = g.oc(mode);
    const long M = g.rows(mode);
    ConvPlan p;
    // tile geometry: a function of the output channel count alone (the
    // stem has the 256x64 kernel only)
    const bool big = OC % 128 == 0 && mode != CONV_STEM;
    p.bm = big ? 128 : 256;
    p.bn = big ? 128 : 64;
    const long mtiles = (M + p.bm - 1) / p.bm;
    const long blocks1 = mtiles * (OC / p.bn) * g.classes(mode);
    // split-K only when the launch would underfill the 256-CU chip AND the
    // K-loop is deep enough to amortize the fp32 partial round-trip (T < 48
    // measured a net loss: 14x14 / 1x1 shapes regressed up to 3x on a
    // blanket trigger — the 4-6x slab traffic dominates at shallow T, those
    // legs are traffic-bound, not fill-bound). Never for the stem, nor for
    // a strided dgrad, whose parity classes already fan out (and whose
    // partials would not be linear in m).
    p.sk = 1;
    if (mode != CONV_STEM && g.classes(mode) == 1 && g.depth(mode) >= 48) {
        if (blocks1 < 192) p.sk = 4;
        else if (blocks1 < 384) p.sk = 2;
    }
    p.blocks = blocks1 * p.sk;
    // The BK32 rings need the grid to fill their blocks/CU: >= ~576 blocks
    // at 3 blocks/CU (128x128), >= 512 at 2 (256x64); below that the lost
    // per-block depth outweighs the extra overlap.
    p.ring = mode != CONV_STEM && conv_bk32() &&
             p.blocks >= (p.bn == 128 ? 576 : 512);
    p.stats_rows = mode == CONV_DGRAD ? 0
                 : p.sk > 1 ? conv_skcombine_blocks(M, OC) : mtiles;
    return p;
}

template <int MODE, class... EPI>
static void conv_dispatch(const void* src, const void* wgt, void* out,
                          const ConvGeom& g, const ConvPlan& p,
                          hipStream_t stream, float* stats, float* skpart,
                          const void* accsrc, EPI... epi) {
    if (p.bn == 128) {
        if (p.ring)
            launch_cfg<MODE, 128, 128, 2, 3, 32, EPI...>(
                src, wgt, out, g, p.sk, stream, stats, skpart, accsrc, epi...);
        else
            launch_cfg<MODE, 128, 128, 2, 2, BK, EPI...>(
                src, wgt, out, g, p.sk, stream, stats, skpart, accsrc, epi...);
    } else {
        if (p.ring)
            launch_cfg<MODE, 256, 64, 1, 3, 32, EPI...>(
                src, wgt, out, g, p.sk, stream, stats, skpart, accsrc, epi...);
        else
            launch_cfg<MODE, 256, 64, 1, 2, BK, EPI...>(
                src, wgt, out, g, p.sk, stream, stats, skpart, accsrc, epi...);
    }
}

void conv_igemm_launch(const void* src, const void* wgt, void* out,
                       const ConvGeom& g, ConvMode mode, const ConvPlan& plan,
                       hipStream_t stream, float* stats, float* skpart,
                       const void* accsrc, const EpiInfer* epi) {
    assert(epi == nullptr || (mode == CONV_FWD && stats == nullptr &&
                              accsrc == nullptr));
    if (mode == CONV_DGRAD)
        conv_dispatch<CONV_DGRAD>(src, wgt, out, g, plan, stream, stats,
                                  skpart, accsrc);
    else if (epi != nullptr && plan.sk == 1)
        conv_dispatch<CONV_FWD, EpiInfer>(src, wgt, out, g, plan, stream,
                                          nullptr, nullptr, nullptr, *epi);
    else
        conv_dispatch<CONV_FWD>(src, wgt, out, g, plan, stream, stats, skpart,
                                accsrc);
}

// ---- batched conv-weight transpose ----------------------------------------
// One launch transposes every conv weight w[k][rs*C+c] -> wt[rs*C+c][k] for
// the dgrad B-tiles (replaces 36 per-layer permute kernels per step).
// Per tensor: 2D 64x64 LDS-tiled transpose, read coalesced along rc, write
// coalesced along k. All conv weights have K and RS*C multiples of 64.
__global__ __launch_bounds__(256) void wt_transpose_kernel(
    const long* __restrict__ src_ptrs,   // device addresses of w tensors
    long* __restrict__ dst_ptrs,         // device addresses of wt slices
    const int* __restrict__ Ks, const int* __restrict__ RCs,
    const int* __restrict__ tile_counts) {
    const int t = blockIdx.y;
    const int K = Ks[t], RC = RCs[t];
    const int kt = K / 64, rt = RC / 64;
    if ((int)blockIdx.x >= tile_counts[t]) return;
    const int tk = blockIdx.x % kt, trc = blockIdx.x / kt;
    (void)rt;
    const unsigned short* src = (const unsigned short*)src_ptrs[t];
    unsigned short* dst = (unsigned short*)dst_ptrs[t];

    __shared__ unsigned short tile[64][64 + 8];  // +8 bf16 pad: no bank dup
    const int tid = threadIdx.x;
    // read: 64 k-rows x 64 rc; thread reads 16 elems, 8-contig along rc
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int kk = (tid / 8) + i * 32;           // 0..63
        const int rc = (tid % 8) * 8;                // 0..56 step 8
        const unsigned short* sp =
            src + (long)(tk * 64 + kk) * RC + trc * 64 + rc;
        #pragma unroll
        for (int e = 0; e < 8; ++e) tile[kk][rc + e] = sp[e];
    }
    __syncthreads();
    // write: 64 rc-rows x 64 k; thread writes 16 elems, 8-contig along k
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int rc = (tid / 8) + i * 32;
        const int kk = (tid % 8) * 8;
        unsigned short* dp =
            dst + (long)(trc * 64 + rc) * K + tk * 64 + kk;
        #pragma unroll
        for (int e = 0; e < 8; ++e) dp[e] = tile[kk + e][rc];
    }
}

void wt_transpose_launch(const long* src_ptrs, long* dst_ptrs, const int* Ks,
                         const int* RCs, const int* tile_counts, int ntensors,
                         int max_tiles, hipStream_t stream) {
    dim3 grid((unsigned)max_tiles, (unsigned)ntensors);
    hipLaunchKernelGGL(wt_transpose_kernel, grid, dim3(256), 0, stream,
                       src_ptrs, dst_ptrs, Ks, RCs, tile_counts);
}

typedef __attribute__((ext_vector_type(4))) short short4_;

// ---- wgrad: dw[k][rs][c] = sum_m dy[m][k] * x_gather[m][c] ----------------
// GEMM with the reduction along the M (pixel) axis — both operands are
// [m][channel] in memory, so the MFMA fragments (which want 8 elements
// along the reduction per lane) are served by gfx950's ds_read_tr16_b64
// hardware transpose-read from an "m4-grouped" LDS image:
//   image element (m, ch) at  kb*1024 + (ch&15) + (m&3)*16 + (m>>2)*64
//   (kb = ch/16); built directly by global_load_lds (16-B chunks are
//   8-channel runs of one m row); read back with per-16-lane-group window
//   addressing: lane addr = kb*2048B + (ks*8 + (lane>>4)*2)*128B +
//   (lane&15)*8B, second half of the fragment at immediate offset +128B.
// Each block owns a (32*FT)k x (32*FT)c output tile (FT = fragments per
// wave axis: 2 -> 64x64 tile / 8 MFMAs per K-step, 4 -> 128x128 tile /
// 32 MFMAs — chosen by channel divisibility; the bigger tile quadruples
// the MFMA-per-glds ratio) for one (r,s) tap and one M-chunk of pixels
// (conv_wgrad_plan sizes it; the stem uses 8 * WG_MCH); chunks accumulate
// into an fp32 workspace with atomicAdd (WG_ATOMIC), or each chunk stores
// its tile into its own fp32 slab (WG_SLAB) and wgrad_slab_fold_kernel sums
// the slabs in chunk order.
constexpr int WG_BM = 64;      // m per K-step
constexpr int WG_MCH = 2048;   // chunk of small problems, the stem's unit

template <int FT, bool STEM = false, int EPI = WG_ATOMIC>
__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(
    const unsigned short* __restrict__ dy,   // [M][K] (NHWC out grad)
    const unsigned short* __restrict__ x,    // [N,H,W,C]
    float* __restrict__ ws,  /* WG_ATOMIC: [K][RS*C] fp32, pre-zeroed,
                                accumulated with atomicAdd across chunks;
                                WG_SLAB: [nch][K][RS*C] fp32, every element
                                stored once */
    int N, int H, int W, int C, int K, int P, int Q,
    int R, int S, int sy, int sx, int py, int px, int nch, int mch) {
    constexpr int MB = WG_BM;                // m per K-step
    constexpr int TCH = 32 * FT;             // tile channels per operand
    constexpr int TILE_ELEMS = MB * TCH;     // one operand tile
    constexpr int GI = MB * TCH / 2048;      // glds per wave per operand
    constexpr int NWIN = MB / 4;             // tr16 windows (4 m x 16 ch)
    constexpr int KSN = MB / 32;             // MFMA m-halves per K-step
    // 1-D grid, chunk-major and XCD-contiguous: the blocks of one pixel
    // chunk (every tap, every tile pair) stage the same dy bytes and nearly
    // the same x bytes, so they get adjacent logical ids and with them one
    // XCD's L2 (wgrad_block_coords, fda_kernels.h).
    const WgradCoords bc = wgrad_block_coords(blockIdx.x, K / TCH, C / TCH,
                                              R * S, nch);
    const int rs = bc.rs;
    const int chunk = bc.chunk;
    const int r = rs / S, s = rs % S;
    const int k0 = bc.ktile * TCH;
    const int c0 = bc.ctile * TCH;
    const long M = (long)N * P * Q;
    const long mb0 = (long)chunk * mch;
    const long mend = (mb0 + mch < M) ? mb0 + mch : M;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wk = wid >> 1;          // 2x2 waves over [TCH k][TCH c]
    const int wc = wid & 1;

    extern __shared__ unsigned short lds[];   // [ring][2*TILE_ELEMS]

    const floatx4 zero4 = {0.f, 0.f, 0.f, 0.f};
    floatx4 acc[FT][FT];
    #pragma unroll
    for (int ki = 0; ki < FT; ++ki)
        #pragma unroll
        for (int ci = 0; ci < FT; ++ci) acc[ki][ci] = zero4;

    // Per-lane staging coordinates, advanced INCREMENTALLY: stage() is
    // called with strictly sequential m-bases (prologue 0,1 then it+2), so
    // each lane tracks its pixel (n,p,q) with constant-delta carries — no
    // per-iteration division (those were ~3x the MFMA issue time here).
    int st_q[GI], st_p[GI], st_n[GI], st_ch[GI];
    long st_dyoff[GI];
    long st_m[GI];
    #pragma unroll
    for (int i = 0; i < GI; ++i) {
        const int ln = (wid * GI + i) * 64 + lane;
        const int e8 = ln * 8;
        const int kb = e8 / (MB * 16);
        const int rr = e8 % (MB * 16);
        // window position -> window index: evens in the low half of the
        // positions, odds in the high half, so the two windows a
        // half-wave tr-reads simultaneously sit on different 128-B bank
        // halves (2-way conflict measured at 6.3% of wave cycles with
        // the linear layout)
        const int pos = rr >> 6;
        const int v = (pos < NWIN / 2) ? pos * 2
                                       : (pos - NWIN / 2) * 2 + 1;
        const int ml = (v << 2) + ((rr & 63) >> 4);
        const int ch = (kb << 4) + (rr & 15);
        st_ch[i] = ch;
        const long m = mb0 + ml;
        st_m[i] = m;
        st_q[i] = (int)(m % Q);
        st_p[i] = (int)((m / Q) % P);
        st_n[i] = (int)(m / ((long)Q * P));
        st_dyoff[i] = m * K + k0 + ch;
    }
    const int dQ = MB % Q, dP = (MB / Q) % P, dN0 = MB / (Q * P);
    const long dDY = (long)MB * K;

    auto stage = [&](int buf) {
        unsigned short* base = lds + buf * 2 * TILE_ELEMS;
        #pragma unroll
        for (int i = 0; i < GI; ++i) {
            const unsigned short* sp =
                (st_m[i] < mend) ? dy + st_dyoff[i] : conv_zero16;
            FDA_GLDS16(sp, base + (wid * GI + i) * 512);
        }
        #pragma unroll
        for (int i = 0; i < GI; ++i) {
            const unsigned short* sp = conv_zero16;
            if (st_m[i] < mend) {
                if (STEM) {
                    // pre-padded C=8 image; virtual channel = pixel s x 8ch
                    const int hh = st_p[i] * sy + r;
                    const int ww = st_q[i] * sx;
                    sp = x + (((long)st_n[i] * H + hh) * W + ww) * 8 +
                         st_ch[i];
                } else {
                    const int hh = st_p[i] * sy - py + r;
                    const int ww = st_q[i] * sx - px + s;
                    if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W)
                        sp = x + (((long)st_n[i] * H + hh) * W + ww) * C +
                             c0 + st_ch[i];
                }
            }
            FDA_GLDS16(sp, base + TILE_ELEMS + (wid * GI + i) * 512);
        }
        // advance MB pixels (bounded carries; dP < P, so p needs at most
        // two conditional wraps after the q carry)
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

    const int l15 = lane & 15, lg = lane >> 4;

    // ring of RING tile-pairs, counted vmcnt: tile t+2's DMA stays in
    // flight across the barrier while tile t computes (2*FT glds per wave
    // per tile-pair). FT=4 uses a 2-deep ring (96 KiB would exceed 1
    // block/CU headroom at 3).
    constexpr int RING = (FT == 2) ? 3 : 2;
    const int nsteps = (int)((mend - mb0 + MB - 1) / MB);
    if (nsteps > 0) stage(0);
    if (RING > 2 && nsteps > 1) stage(1);
    for (int it = 0; it < nsteps; ++it) {
        if (RING > 2 && it + 1 < nsteps) {
            static_assert(2 * GI == 4 || 2 * GI == 8,
                          "counted ring: state the vmcnt for this GI");
            if constexpr (2 * GI == 4)
                asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        // NOTE: the next tile's stage() is issued AFTER the tr reads below.
        // hipcc (ROCm 7.2) conservatively emits `s_waitcnt vmcnt(0)` before
        // every ds_read_b64_tr_b16 cluster (the intrinsic is ordered
        // against pending LDS-DMA writes it cannot alias-analyze), so a
        // stage issued before the reads is fully drained before any MFMA
        // runs — the r1 kernel had ZERO DMA/compute overlap here (the
        // measured WAIT_INST 38.6%). Reads-then-stage makes the inserted
        // drain wait only for data this iteration needs anyway, and the
        // DMA now flies over the MFMA cluster.
        const unsigned short* buf = lds + (it % RING) * 2 * TILE_ELEMS;
        short4_ a[FT][KSN][2], b[FT][KSN][2];   // [fi][ks][half]
        #pragma unroll
        for (int fi = 0; fi < FT; ++fi)
            #pragma unroll
            for (int ks = 0; ks < KSN; ++ks) {
                const int kb_a = wk * FT + fi;
                const int kb_b = wc * FT + fi;
                const int v0 = ks * 8 + lg * 2;          // window indices
                const int p0 = (v0 >> 1);                // v0 even -> low half
                const int p1 = p0 + NWIN / 2;            // v0+1 odd -> high
                const unsigned short* pa =
                    buf + kb_a * (MB * 16) + l15 * 4;
                const unsigned short* pb =
                    buf + TILE_ELEMS + kb_b * (MB * 16) + l15 * 4;
                a[fi][ks][0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4_*)(pa + p0 * 64));
                a[fi][ks][1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4_*)(pa + p1 * 64));
                b[fi][ks][0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4_*)(pb + p0 * 64));
                b[fi][ks][1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) short4_*)(pb + p1 * 64));
            }
        if (it + RING - 1 < nsteps) stage((it + RING - 1) % RING);
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int ks = 0; ks < KSN; ++ks)
            #pragma unroll
            for (int ki = 0; ki < FT; ++ki)
                #pragma unroll
                for (int ci = 0; ci < FT; ++ci) {
                    short8 af, bf;
                    #pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        af[e] = a[ki][ks][0][e];
                        af[e + 4] = a[ki][ks][1][e];
                        bf[e] = b[ci][ks][0][e];
                        bf[e + 4] = b[ci][ks][1][e];
                    }
                    acc[ki][ci] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af, bf, acc[ki][ci], 0, 0, 0);
                }
        __builtin_amdgcn_s_setprio(0);
        // end barrier dropped: the next iteration's wait + top barrier
        // orders buffer reuse for every ring depth.
    }

    // epilogue: out[i=k][j=c]; C/D map col=lane&15, row=(lane>>4)*4+jj
    const int fcol = lane & 15, frow0 = (lane >> 4) * 4;
    const long RSC = (long)R * S * C;
    // WG_SLAB: the whole tile goes to the chunk's own slab, once, with plain
    // stores (rows past mend were staged as zeros, so a ragged last chunk
    // still writes every element). Stored from the fragment layout, four
    // 64-B row pieces per wave-instruction: the LDS-staged 16-B form of the
    // dgrad epilogue measured the same here (profiles/wgrad_slab.md).
    float* o = ws;
    if constexpr (EPI == WG_SLAB) o += (long)chunk * K * RSC;
    #pragma unroll
    for (int ki = 0; ki < FT; ++ki)
        #pragma unroll
        for (int ci = 0; ci < FT; ++ci)
            #pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int kk = k0 + wk * 16 * FT + ki * 16 + frow0 + jj;
                const int cc = c0 + wc * 16 * FT + ci * 16 + fcol;
                float* p = &o[kk * RSC + (long)rs * C + cc];
                if constexpr (EPI == WG_SLAB) *p = acc[ki][ci][jj];
                else atomicAdd(p, acc[ki][ci][jj]);
            }
}

void conv_stem_wgrad_launch(const void* dy, const void* x, float* ws,
                            const ConvGeom& g, hipStream_t stream) {
    // Output is tiny (K x R*64), so small chunks would hammer the same
    // fp32 addresses with atomics (588 hits/address measured at 2048):
    // use 16k-pixel chunks.
    const long M = g.rows(CONV_STEM);
    constexpr int STEM_MCH = 8 * WG_MCH;    // 16k pixels: balances atomic fan-in per address against block count (32k measured 472 us/step vs 254 at 16k)
    const int nch = (int)((M + STEM_MCH - 1) / STEM_MCH);
    // block order (chunk, r, ktile): the seven r taps of a chunk share dy
    const dim3 grid((unsigned)((g.K / 64) * g.R * nch));
    const size_t shmem = 3 * 2 * (WG_BM * 64) * sizeof(unsigned short);
    hipLaunchKernelGGL((conv_wgrad_kernel<2, true>), grid, dim3(256), shmem,
                       stream, (const unsigned short*)dy,
                       (const unsigned short*)x, ws, g.N, g.H, g.W, 64, g.K,
                       g.P, g.Q, g.R, 1, g.sy, g.sx, 0, 0, nch, STEM_MCH);
}

// Chunk plan. The grid is sized to ONE resident wave of blocks: 256 CUs x 2
// blocks (FT4: 64 KiB LDS, 176 VGPRs) or x 3 (FT2: 48 KiB LDS), and never
// more, since a few blocks past the resident slots run as a second wave
// behind the first (792 blocks on 768 slots measured 47 us where 720 take
// 39). More chunks mean more fp32 atomics (K*RS*C*4 bytes per chunk at about
// 1.3 TB/s chip-wide), which is what keeps the count from going higher:
// twice the slots measured slower on every shape. A 1x1 filter has no taps
// that share operand tiles and its atomic epilogue weighs more against its
// short K-loop, so it takes half the slots (12.4 us against 13.5 at all of
// them and 24.5 at the old 2048-pixel chunks). Chunks are whole 64-pixel
// K-steps, of even length (4704 pixels in 3 chunks are 1600+1600+1504, not
// 2048+2048+608), and no shorter than the shortest measured, 7 K-steps.
// profiles/wgrad_raster.md has the candidates per shape.
// Up to 2 * WG_MCH pixels the plan stays at one or two WG_MCH chunks: with
// at most two addends per address the fp32 sum does not depend on the
// order the atomics arrive in, so small problems keep giving the same bits
// from run to run (the small-model DDP tests compare runs bit for bit),
// and nothing was measured there.
constexpr int WG_CUS = 256;
constexpr int WG_MIN_MCH = 7 * WG_BM;

// tile/chunk plan: FT (fragments per wave axis), pixels per chunk, chunks,
// and the 1-D grid (tile pairs x taps x chunks)
WgradPlan conv_wgrad_plan(long M, int C, int K, int R, int S) {
    WgradPlan p;
    // FT=4 quarters the block count; only worth it when the grid still
    // fills the 256 CUs (small-M 1x1 shapes measured 1.4x slower on it)
    const long tiles4 = (long)(K / 128) * (C / 128) * R * S;
    const long tiles2 = (long)(K / 64) * (C / 64) * R * S;
    const long blocks4_max = tiles4 * ((M + WG_MCH - 1) / WG_MCH);
    p.ft = (K % 128 == 0 && C % 128 == 0 && blocks4_max >= 192) ? 4 : 2;
    const long tiles = p.ft == 4 ? tiles4 : tiles2;
    const long slots = WG_CUS * (p.ft == 4 ? 2 : 3);
    long nch = (R * S == 1 ? slots / 2 : slots) / tiles;
    if (nch < 1) nch = 1;
    long mch = ((M + nch - 1) / nch + WG_BM - 1) / WG_BM * WG_BM;
    if (mch < WG_MIN_MCH) mch = WG_MIN_MCH;
    if (M <= 2 * WG_MCH) mch = WG_MCH;
    p.mch = (int)mch;
    p.nch = (int)((M + mch - 1) / mch);
    p.nwg = tiles * p.nch;
    return p;
}

// Slabs or atomics. One or two chunks stay on atomics: at most two addends
// per address are order-independent already, and a fold would only add a
// pass. Beyond that the slab path trades nch*n*4 bytes of atomics (about
// 1.3 TB/s) for as many bytes of plain stores, the fold's read of them and
// one more dependent launch, about 5 us: measured per call, it saves 5 to
// 10 us at 28 to 33 MB (the four FT4 flagship shapes) and loses 1 to 13 us
// at 5.5 to 12.4 MB (the six FT2 ones), with break-even near 13 MB by that
// model. The threshold sits between the two measured groups
// (profiles/wgrad_slab.md).
constexpr long WG_SLAB_MIN_BYTES = 24L << 20;

bool conv_wgrad_use_slabs(const WgradPlan& p, long n) {
    return p.nch >= 3 && (long)p.nch * n * 4 >= WG_SLAB_MIN_BYTES;
}

void conv_wgrad_launch(const void* dy, const void* x, float* ws,
                       const ConvGeom& g, hipStream_t stream, int epi) {
    const WgradPlan p = conv_wgrad_plan(g.rows(CONV_FWD), g.C, g.K, g.R, g.S);
    // one argument list for both tile sizes and every epilogue
    auto launch = [&](auto kern, size_t shmem) {
        hipLaunchKernelGGL(kern, dim3((unsigned)p.nwg), dim3(256), shmem,
                           stream, (const unsigned short*)dy,
                           (const unsigned short*)x, ws, g.N, g.H, g.W, g.C,
                           g.K, g.P, g.Q, g.R, g.S, g.sy, g.sx, g.py, g.px,
                           p.nch, p.mch);
    };
    dispatch_flag(epi == WG_SLAB, [&](auto slab) {
        constexpr int EPI = decltype(slab)::value ? WG_SLAB : WG_ATOMIC;
        if (p.ft == 4)
            launch(conv_wgrad_kernel<4, false, EPI>,
                   2 * 2 * (WG_BM * 128) * sizeof(unsigned short));
        else
            launch(conv_wgrad_kernel<2, false, EPI>,
                   3 * 2 * (WG_BM * 64) * sizeof(unsigned short));
    });
}

}  // namespace fda
