// Squeeze-and-Excitation (Hu et al. 2018) block tail, NHWC bf16:
//
//   z[n][c] = mean_hw u[n][hw][c]                      squeeze
//   h[n][j] = relu(b1[j] + sum_c W1[j][c] z[n][c])     C -> Cr
//   s[n][c] = sigmoid(b2[c] + sum_j W2[c][j] h[n][j])  Cr -> C
//   out     = relu(u * s[n][c] + identity)             scale, add, ReLU
//
// The op is bound by memory: the two matrix products are at most 2*N*C*Cr
// MACs (50 M at N=96, C=2048) while u, identity and out are full
// activations. So the streaming passes are the design and the products are
// small fp32 VALU loops.
//
// Why VALU and not the MFMA: the GEMM has M = N images, a few tens of MFLOP
// per block of the network, and z and h would have to be rounded to bf16 to
// feed the bf16 MFMA, a round the reference formula does not have. z, h, s
// and every partial stay fp32; the weights are read as stored (nn.Linear
// layouts, bf16), no packed copies, no arena.
//
// Forward, three launches:
//   se_reduce_kernel<false>  (squeeze) grid (hw-chunk, image). A lane owns 8
//       consecutive channels (one 16-B load per row), C/8 lanes span a row,
//       the block's other lanes take further rows. fp32 per lane, row groups
//       folded through LDS in ascending order, one plain store of
//       part[n][chunk][C]. No atomics, nothing pre-zeroed. se_plan cuts HW
//       into nsplit chunks so small-N, large-HW shapes fill the chip.
//   se_excite_fwd_kernel     one block per ipb images, so a weight fragment
//       read once serves all of them. Folds the partials in chunk order,
//       z = sum * fl32(1/HW) into LDS (and memory, for backward). FC1: a
//       wave per row j, lanes stride over c with 16-B loads of W1, fp32 FMA,
//       shuffle reduce, bias, ReLU; h into LDS (and memory). FC2: a lane per
//       channel c reads its Cr-long row of W2 in 16-B (Cr % 8 == 0) or 8-B
//       pieces, bias, s = 1 / (1 + exp(-a)).
//   se_scale_add_relu_fwd_kernel  grid (row-chunk, image), 16 B per lane, a
//       lane keeps its 8 values of s in registers over the rows it walks:
//       out = bf16(max(fmaf(f32(u), s, f32(identity)), 0)), one round.
//
// Backward, four launches (g = gout, saved u, out, s, h, z):
//   se_reduce_kernel<true>   dspart[n][chunk][c] = sum_hw (out > 0 ? g*u : 0)
//   se_excite_bwd_kernel     ds folded in chunk order; da2 = ds*s*(1-s);
//       dh[j] = sum_c W2[c][j] da2[c] (lanes span a row of W2 in 8-B pieces,
//       row groups folded through LDS in ascending order); da1 = h > 0 ? dh
//       : 0; dzs[c] = fl32(1/HW) * sum_j W1[j][c] da1[j] (a lane owns 8
//       channels, j ascending).
//   se_param_grad_kernel     a lane owns 4 consecutive elements of dW1, dW2,
//       db1 or db2 and loops over n in increasing order at fp32: the same
//       bits on every run, rounded once to bf16.
//   se_scale_bwd_apply_kernel  du = bf16(fmaf(mg, s, dzs)), mg = out > 0 ?
//       g : 0; gidentity = out > 0 ? g : +0 (a copy of the bits).
//
// Constraints (bindings): C % 64 == 0, 64 <= C <= 2048; Cr % 4 == 0,
// 4 <= Cr <= 128. When 256 % (C/8) != 0 the lanes past the last whole row
// group idle.

#include <hip/hip_runtime.h>
#include "fda_common.h"
#include "fda_kernels.h"

// The fp32 arithmetic of this file is compiled to scalar-lane VALU ops only
// (no packed fp32 forms), like the other kernel files added after the BN set.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace fda {

constexpr int SE_THREADS = 256;
constexpr int SE_IPB_MAX = 4;

SePlan se_plan(int N, int HW, int C) {
    SePlan p;
    const int rpb = SE_THREADS / (C / 8);   // rows a block covers per pass
    int cap = HW / (2 * rpb);               // >= 2 rows per lane and chunk
    if (cap < 1) cap = 1;
    int ns = (1024 + N - 1) / N;            // ~4 blocks per CU over the batch
    if (ns > cap) ns = cap;
    if (ns > 64) ns = 64;
    p.rpc = (HW + ns - 1) / ns;
    p.nsplit = (HW + p.rpc - 1) / p.rpc;    // no empty chunk
    p.ipb = N > 512 ? SE_IPB_MAX : (N > 1 ? 2 : 1);
    return p;
}

// (row group, channel lane) of a thread in the streaming kernels
struct SeLane {
    int tpr, rpb, sub_r, lane_c;
    bool active;
};
__device__ __forceinline__ SeLane se_lane(int C) {
    SeLane L;
    L.tpr = C >> 3;
    L.rpb = SE_THREADS / L.tpr;
    L.sub_r = (int)threadIdx.x / L.tpr;
    L.lane_c = (int)threadIdx.x - L.sub_r * L.tpr;
    L.active = L.sub_r < L.rpb;
    return L;
}

__device__ __forceinline__ void se_load8(const float* p, float (&f)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void se_store8(float* p, const float (&f)[8]) {
    *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
    *(float4*)(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// One row's 8 terms of the reduction: u (squeeze) or out > 0 ? g*u : 0. The
// product of two bf16 values is exact in fp32.
template <bool BWD>
__device__ __forceinline__ void se_row_terms(
    const unsigned short* __restrict__ u, const unsigned short* __restrict__ g,
    const unsigned short* __restrict__ out, size_t off, float (&t)[8]) {
    const uint4 ur = *(const uint4*)(u + off);
    if constexpr (BWD) {
        const uint4 gr = *(const uint4*)(g + off);
        const uint4 orw = *(const uint4*)(out + off);
        float gf[8], of[8];
        unpack_f32<unsigned short, 8>(ur, t);
        unpack_f32<unsigned short, 8>(gr, gf);
        unpack_f32<unsigned short, 8>(orw, of);
        #pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = of[k] > 0.f ? gf[k] * t[k] : 0.f;
    } else {
        unpack_f32<unsigned short, 8>(ur, t);
    }
}

template <bool BWD>
__global__ __launch_bounds__(SE_THREADS) void se_reduce_kernel(
    const unsigned short* __restrict__ u, const unsigned short* __restrict__ g,
    const unsigned short* __restrict__ out, float* __restrict__ part, int HW,
    int C, int rpc) {
    __shared__ __attribute__((aligned(16))) float smem[SE_THREADS * 8];
    const int n = blockIdx.y, chunk = blockIdx.x, nsplit = gridDim.x;
    const SeLane L = se_lane(C);
    const int r0 = chunk * rpc;
    const int r1 = r0 + rpc < HW ? r0 + rpc : HW;
    float acc[8];
    #pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    if (L.active) {
        const size_t base = (size_t)n * HW * C + (size_t)L.lane_c * 8;
        int r = r0 + L.sub_r;
        // two rows' loads in flight; the adds stay in row order
        for (; r + L.rpb < r1; r += 2 * L.rpb) {
            float t0[8], t1[8];
            se_row_terms<BWD>(u, g, out, base + (size_t)r * C, t0);
            se_row_terms<BWD>(u, g, out, base + (size_t)(r + L.rpb) * C, t1);
            #pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += t0[k];
            #pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += t1[k];
        }
        if (r < r1) {
            float t0[8];
            se_row_terms<BWD>(u, g, out, base + (size_t)r * C, t0);
            #pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += t0[k];
        }
    }
    se_store8(smem + threadIdx.x * 8, acc);
    __syncthreads();
    if (L.active && L.sub_r == 0) {
        float t[8];
        #pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = 0.f;
        for (int rr = 0; rr < L.rpb; ++rr) {
            float v[8];
            se_load8(smem + (rr * L.tpr + L.lane_c) * 8, v);
            #pragma unroll
            for (int k = 0; k < 8; ++k) t[k] += v[k];
        }
        se_store8(part + ((size_t)n * nsplit + chunk) * C + L.lane_c * 8, t);
    }
}

// fold the nsplit partials of images [n0, n0 + ni) in chunk order
__device__ __forceinline__ float se_fold_part(const float* __restrict__ part,
                                              int n, int c, int nsplit,
                                              int C) {
    const float* p = part + (size_t)n * nsplit * C + c;
    float s = p[0];
    for (int k = 1; k < nsplit; ++k) s += p[(size_t)k * C];
    return s;
}

__global__ __launch_bounds__(SE_THREADS) void se_excite_fwd_kernel(
    const float* __restrict__ part, const unsigned short* __restrict__ w1,
    const unsigned short* __restrict__ b1,
    const unsigned short* __restrict__ w2,
    const unsigned short* __restrict__ b2, float* __restrict__ z,
    float* __restrict__ h, float* __restrict__ s, int N, int C, int Cr,
    int nsplit, int ipb, float inv_hw) {
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    float* zs = se_lds;             // [ipb][C]
    float* hs = se_lds + ipb * C;   // [ipb][Cr]
    const int n0 = blockIdx.x * ipb;
    const int ni = N - n0 < ipb ? N - n0 : ipb;
    const int tid = threadIdx.x;

    for (int idx = tid; idx < ni * C; idx += SE_THREADS) {
        const int i = idx / C, c = idx - i * C;
        const float zv = se_fold_part(part, n0 + i, c, nsplit, C) * inv_hw;
        zs[idx] = zv;
        z[(size_t)(n0 + i) * C + c] = zv;
    }
    __syncthreads();

    // FC1: a wave per row j
    const int lane = tid & (WAVE - 1), wid = tid / WAVE;
    for (int j = wid; j < Cr; j += SE_THREADS / WAVE) {
        float acc[SE_IPB_MAX];
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) acc[i] = 0.f;
        for (int c8 = lane; c8 < (C >> 3); c8 += WAVE) {
            float wf[8];
            unpack_f32<unsigned short, 8>(
                *(const uint4*)(w1 + (size_t)j * C + c8 * 8), wf);
            #pragma unroll
            for (int i = 0; i < SE_IPB_MAX; ++i) {
                if (i < ni) {
                    float zf[8];
                    se_load8(zs + i * C + c8 * 8, zf);
                    #pragma unroll
                    for (int k = 0; k < 8; ++k)
                        acc[i] = __fmaf_rn(wf[k], zf[k], acc[i]);
                }
            }
        }
        const float bj = bf16bits_to_f32(b1[j]);
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) {
            const float t = wave_reduce_sum(acc[i]);
            if (lane == 0 && i < ni) {
                const float hv = fmaxf(t + bj, 0.f);
                hs[i * Cr + j] = hv;
                h[(size_t)(n0 + i) * Cr + j] = hv;
            }
        }
    }
    __syncthreads();

    // FC2: a lane per channel c
    for (int c = tid; c < C; c += SE_THREADS) {
        float acc[SE_IPB_MAX];
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) acc[i] = 0.f;
        const unsigned short* row = w2 + (size_t)c * Cr;
        if ((Cr & 7) == 0) {
            for (int j = 0; j < Cr; j += 8) {
                float wf[8];
                unpack_f32<unsigned short, 8>(*(const uint4*)(row + j), wf);
                #pragma unroll
                for (int i = 0; i < SE_IPB_MAX; ++i) {
                    if (i < ni) {
                        #pragma unroll
                        for (int k = 0; k < 8; ++k)
                            acc[i] = __fmaf_rn(wf[k], hs[i * Cr + j + k],
                                               acc[i]);
                    }
                }
            }
        } else {
            for (int j = 0; j < Cr; j += 4) {
                const uint2 raw = *(const uint2*)(row + j);
                const float wf[4] = {
                    __uint_as_float(raw.x << 16),
                    __uint_as_float(raw.x & 0xffff0000u),
                    __uint_as_float(raw.y << 16),
                    __uint_as_float(raw.y & 0xffff0000u)};
                #pragma unroll
                for (int i = 0; i < SE_IPB_MAX; ++i) {
                    if (i < ni) {
                        #pragma unroll
                        for (int k = 0; k < 4; ++k)
                            acc[i] = __fmaf_rn(wf[k], hs[i * Cr + j + k],
                                               acc[i]);
                    }
                }
            }
        }
        const float bc = bf16bits_to_f32(b2[c]);
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) {
            if (i < ni) {
                const float a = acc[i] + bc;
                s[(size_t)(n0 + i) * C + c] =
                    __fdiv_rn(1.f, 1.f + expf(-a));
            }
        }
    }
}

__global__ __launch_bounds__(SE_THREADS) void se_scale_add_relu_fwd_kernel(
    const unsigned short* __restrict__ u,
    const unsigned short* __restrict__ idn, const float* __restrict__ s,
    unsigned short* __restrict__ out, int HW, int C, int rpc) {
    const int n = blockIdx.y;
    const SeLane L = se_lane(C);
    if (!L.active) return;
    const int r0 = blockIdx.x * rpc;
    const int r1 = r0 + rpc < HW ? r0 + rpc : HW;
    float sv[8];
    se_load8(s + (size_t)n * C + L.lane_c * 8, sv);
    const size_t base = (size_t)n * HW * C + (size_t)L.lane_c * 8;
    for (int r = r0 + L.sub_r; r < r1; r += L.rpb) {
        const size_t off = base + (size_t)r * C;
        const uint4 ur = *(const uint4*)(u + off);
        const uint4 ir = *(const uint4*)(idn + off);
        float uf[8], rf[8];
        unpack_f32<unsigned short, 8>(ur, uf);
        unpack_f32<unsigned short, 8>(ir, rf);
        unsigned short ov[8];
        #pragma unroll
        for (int k = 0; k < 8; ++k)
            ov[k] = f32_to_bf16bits(
                fmaxf(__fmaf_rn(uf[k], sv[k], rf[k]), 0.f));
        *(uint4*)(out + off) = *(const uint4*)ov;
    }
}

__global__ __launch_bounds__(SE_THREADS) void se_excite_bwd_kernel(
    const float* __restrict__ dspart, const float* __restrict__ s,
    const float* __restrict__ h, const unsigned short* __restrict__ w1,
    const unsigned short* __restrict__ w2, float* __restrict__ da2,
    float* __restrict__ da1, float* __restrict__ dzs, int N, int C, int Cr,
    int nsplit, int ipb, float inv_hw) {
    extern __shared__ __attribute__((aligned(16))) float se_lds[];
    float* d2s = se_lds;                   // [ipb][C]
    float* d1s = d2s + ipb * C;            // [ipb][Cr]
    float* red = d1s + ipb * Cr;           // [ipb][SE_THREADS * 4]
    const int n0 = blockIdx.x * ipb;
    const int ni = N - n0 < ipb ? N - n0 : ipb;
    const int tid = threadIdx.x;

    for (int idx = tid; idx < ni * C; idx += SE_THREADS) {
        const int i = idx / C, c = idx - i * C;
        const float ds = se_fold_part(dspart, n0 + i, c, nsplit, C);
        const float sv = s[(size_t)(n0 + i) * C + c];
        const float d = ds * sv * (1.f - sv);
        d2s[idx] = d;
        da2[(size_t)(n0 + i) * C + c] = d;
    }
    __syncthreads();

    // dh[j] = sum_c W2[c][j] da2[c]: Cr/4 lanes span a row of W2 in 8-B
    // pieces (thread t reads elements 4t.. of each pass: fully coalesced),
    // the other lanes take further rows
    {
        const int tpr = Cr >> 2, rg = SE_THREADS / tpr;
        const int sub = tid / tpr, lj = tid - sub * tpr;
        float acc[SE_IPB_MAX][4];
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i)
            #pragma unroll
            for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;
        if (sub < rg) {
            for (int c = sub; c < C; c += rg) {
                const uint2 raw = *(const uint2*)(w2 + (size_t)c * Cr + lj * 4);
                const float wf[4] = {
                    __uint_as_float(raw.x << 16),
                    __uint_as_float(raw.x & 0xffff0000u),
                    __uint_as_float(raw.y << 16),
                    __uint_as_float(raw.y & 0xffff0000u)};
                #pragma unroll
                for (int i = 0; i < SE_IPB_MAX; ++i) {
                    if (i < ni) {
                        const float d = d2s[i * C + c];
                        #pragma unroll
                        for (int k = 0; k < 4; ++k)
                            acc[i][k] = __fmaf_rn(wf[k], d, acc[i][k]);
                    }
                }
            }
        }
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) {
            if (i < ipb)
                *(float4*)(red + (i * SE_THREADS + tid) * 4) =
                    make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
        __syncthreads();
        if (tid < Cr) {
            const int j4 = tid >> 2, k = tid & 3;
            for (int i = 0; i < ni; ++i) {
                float dh = 0.f;
                for (int gi = 0; gi < rg; ++gi)
                    dh += red[(i * SE_THREADS + gi * tpr + j4) * 4 + k];
                const float hv = h[(size_t)(n0 + i) * Cr + tid];
                const float d = hv > 0.f ? dh : 0.f;
                d1s[i * Cr + tid] = d;
                da1[(size_t)(n0 + i) * Cr + tid] = d;
            }
        }
        __syncthreads();
    }

    // dzs[c] = fl32(1/HW) * sum_j W1[j][c] da1[j]: a lane owns 8 channels
    for (int c8 = tid; c8 < (C >> 3); c8 += SE_THREADS) {
        float acc[SE_IPB_MAX][8];
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i)
            #pragma unroll
            for (int k = 0; k < 8; ++k) acc[i][k] = 0.f;
        #pragma unroll 4
        for (int j = 0; j < Cr; ++j) {
            float wf[8];
            unpack_f32<unsigned short, 8>(
                *(const uint4*)(w1 + (size_t)j * C + c8 * 8), wf);
            #pragma unroll
            for (int i = 0; i < SE_IPB_MAX; ++i) {
                if (i < ni) {
                    const float d = d1s[i * Cr + j];
                    #pragma unroll
                    for (int k = 0; k < 8; ++k)
                        acc[i][k] = __fmaf_rn(wf[k], d, acc[i][k]);
                }
            }
        }
        #pragma unroll
        for (int i = 0; i < SE_IPB_MAX; ++i) {
            if (i < ni) {
                float o[8];
                #pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = acc[i][k] * inv_hw;
                se_store8(dzs + (size_t)(n0 + i) * C + c8 * 8, o);
            }
        }
    }
}

// 4 consecutive outputs out[e0..e0+3] = bf16(sum_n a[n*lda + ia] *
// b[n*ldb + e0' + k]): a is the scalar operand, b the 4-wide one.
__device__ __forceinline__ void se_param_group(
    const float* __restrict__ a, int lda, int ia, const float* __restrict__ b,
    int ldb, int ib, int N, unsigned short* __restrict__ dst) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) {
        const float av = a == nullptr ? 1.f : a[(size_t)n * lda + ia];
        const float4 bv = *(const float4*)(b + (size_t)n * ldb + ib);
        acc[0] = __fmaf_rn(av, bv.x, acc[0]);
        acc[1] = __fmaf_rn(av, bv.y, acc[1]);
        acc[2] = __fmaf_rn(av, bv.z, acc[2]);
        acc[3] = __fmaf_rn(av, bv.w, acc[3]);
    }
    unsigned short o[4];
    #pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = f32_to_bf16bits(acc[k]);
    *(uint2*)dst = *(const uint2*)o;
}

// Groups of 4 elements, in this order: dW1 [Cr][C], dW2 [C][Cr], db2 [C],
// db1 [Cr].
__global__ __launch_bounds__(SE_THREADS) void se_param_grad_kernel(
    const float* __restrict__ da2, const float* __restrict__ da1,
    const float* __restrict__ h, const float* __restrict__ z,
    unsigned short* __restrict__ dw1, unsigned short* __restrict__ db1,
    unsigned short* __restrict__ dw2, unsigned short* __restrict__ db2, int N,
    int C, int Cr) {
    const int gw = (C * Cr) >> 2;   // groups per weight
    int e = blockIdx.x * SE_THREADS + threadIdx.x;
    if (e < gw) {                   // dW1[j][c] = sum_n da1[n][j] z[n][c]
        const int j = (e * 4) / C, c = (e * 4) - j * C;
        se_param_group(da1, Cr, j, z, C, c, N, dw1 + (size_t)e * 4);
        return;
    }
    e -= gw;
    if (e < gw) {                   // dW2[c][j] = sum_n da2[n][c] h[n][j]
        const int c = (e * 4) / Cr, j = (e * 4) - c * Cr;
        se_param_group(da2, C, c, h, Cr, j, N, dw2 + (size_t)e * 4);
        return;
    }
    e -= gw;
    if (e < (C >> 2)) {             // db2 = sum_n da2
        se_param_group(nullptr, 0, 0, da2, C, e * 4, N, db2 + e * 4);
        return;
    }
    e -= C >> 2;
    if (e < (Cr >> 2))              // db1 = sum_n da1
        se_param_group(nullptr, 0, 0, da1, Cr, e * 4, N, db1 + e * 4);
}

__global__ __launch_bounds__(SE_THREADS) void se_scale_bwd_apply_kernel(
    const unsigned short* __restrict__ g,
    const unsigned short* __restrict__ out, const float* __restrict__ s,
    const float* __restrict__ dzs, unsigned short* __restrict__ du,
    unsigned short* __restrict__ gid, int HW, int C, int rpc) {
    const int n = blockIdx.y;
    const SeLane L = se_lane(C);
    if (!L.active) return;
    const int r0 = blockIdx.x * rpc;
    const int r1 = r0 + rpc < HW ? r0 + rpc : HW;
    float sv[8], dz[8];
    se_load8(s + (size_t)n * C + L.lane_c * 8, sv);
    se_load8(dzs + (size_t)n * C + L.lane_c * 8, dz);
    const size_t base = (size_t)n * HW * C + (size_t)L.lane_c * 8;
    for (int r = r0 + L.sub_r; r < r1; r += L.rpb) {
        const size_t off = base + (size_t)r * C;
        unsigned short gv[8], ov[8], dv[8], iv[8];
        *(uint4*)gv = *(const uint4*)(g + off);
        *(uint4*)ov = *(const uint4*)(out + off);
        #pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool pos = bf16bits_to_f32(ov[k]) > 0.f;
            const float mg = pos ? bf16bits_to_f32(gv[k]) : 0.f;
            dv[k] = f32_to_bf16bits(__fmaf_rn(mg, sv[k], dz[k]));
            iv[k] = pos ? gv[k] : (unsigned short)0;
        }
        *(uint4*)(du + off) = *(const uint4*)dv;
        *(uint4*)(gid + off) = *(const uint4*)iv;
    }
}

// ---- launchers --------------------------------------------------------------

static size_t se_excite_lds(int C, int Cr, int ipb, bool bwd) {
    return (size_t)ipb * (C + Cr + (bwd ? SE_THREADS * 4 : 0)) * sizeof(float);
}

void se_fwd_launch(const void* u, const void* identity, const void* w1,
                   const void* b1, const void* w2, const void* b2, void* out,
                   float* s, float* h, float* z, float* part, int N, int HW,
                   int C, int Cr, hipStream_t st) {
    typedef const unsigned short* bp;
    const SePlan p = se_plan(N, HW, C);
    const dim3 grid(p.nsplit, N), block(SE_THREADS);
    const float inv_hw = 1.f / (float)HW;
    hipLaunchKernelGGL(se_reduce_kernel<false>, grid, block, 0, st, (bp)u,
                       (bp) nullptr, (bp) nullptr, part, HW, C, p.rpc);
    hipLaunchKernelGGL(se_excite_fwd_kernel, dim3((N + p.ipb - 1) / p.ipb),
                       block, se_excite_lds(C, Cr, p.ipb, false), st, part,
                       (bp)w1, (bp)b1, (bp)w2, (bp)b2, z, h, s, N, C, Cr,
                       p.nsplit, p.ipb, inv_hw);
    hipLaunchKernelGGL(se_scale_add_relu_fwd_kernel, grid, block, 0, st,
                       (bp)u, (bp)identity, s, (unsigned short*)out, HW, C,
                       p.rpc);
}

void se_bwd_launch(const void* gout, const void* out, const void* u,
                   const float* s, const float* h, const float* z,
                   const void* w1, const void* w2, void* du, void* gidentity,
                   void* dw1, void* db1, void* dw2, void* db2, float* part,
                   float* da2, float* da1, float* dzs, int N, int HW, int C,
                   int Cr, hipStream_t st) {
    typedef const unsigned short* bp;
    typedef unsigned short* bo;
    const SePlan p = se_plan(N, HW, C);
    const dim3 grid(p.nsplit, N), block(SE_THREADS);
    const float inv_hw = 1.f / (float)HW;
    hipLaunchKernelGGL(se_reduce_kernel<true>, grid, block, 0, st, (bp)u,
                       (bp)gout, (bp)out, part, HW, C, p.rpc);
    hipLaunchKernelGGL(se_excite_bwd_kernel, dim3((N + p.ipb - 1) / p.ipb),
                       block, se_excite_lds(C, Cr, p.ipb, true), st, part, s,
                       h, (bp)w1, (bp)w2, da2, da1, dzs, N, C, Cr, p.nsplit,
                       p.ipb, inv_hw);
    const int groups = (2 * C * Cr + C + Cr) / 4;
    hipLaunchKernelGGL(se_param_grad_kernel,
                       dim3((groups + SE_THREADS - 1) / SE_THREADS), block, 0,
                       st, da2, da1, h, z, (bo)dw1, (bo)db1, (bo)dw2, (bo)db2,
                       N, C, Cr);
    hipLaunchKernelGGL(se_scale_bwd_apply_kernel, grid, block, 0, st,
                       (bp)gout, (bp)out, s, dzs, (bo)du, (bo)gidentity, HW,
                       C, p.rpc);
}

}  // namespace fda

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
