// Common device helpers for fluxdistributed_amd gfx950 kernels.
// CDNA4: wavefront = 64 lanes; block sizes are multiples of 64.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

namespace fda {

constexpr int WAVE = 64;

// ---- dtype plumbing --------------------------------------------------------
// bf16 <-> f32: load via bit-shift (exact), store via RNE intrinsic.
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ __forceinline__ float bf16bits_to_f32(unsigned short u) {
    union { unsigned int i; float f; } c;
    c.i = (unsigned int)u << 16;
    return c.f;
}
__device__ __forceinline__ unsigned short f32_to_bf16bits(float f) {
    // round-to-nearest-even
    union { float f; unsigned int i; } c;
    c.f = f;
    unsigned int x = c.i;
    unsigned int lsb = (x >> 16) & 1u;
    x += 0x7fffu + lsb;
    return (unsigned short)(x >> 16);
}

template <typename T> struct VecWidth;
template <> struct VecWidth<float> { static constexpr int value = 4; };           // 16 B
template <> struct VecWidth<unsigned short> { static constexpr int value = 8; };  // 16 B (bf16 bits)

template <typename T>
__device__ __forceinline__ float load_f32(const T* p) {
    if constexpr (sizeof(T) == 2) return bf16bits_to_f32(*(const unsigned short*)p);
    else return *(const float*)p;
}
template <typename T>
__device__ __forceinline__ void store_f32(T* p, float v) {
    if constexpr (sizeof(T) == 2) *(unsigned short*)p = f32_to_bf16bits(v);
    else *(float*)p = v;
}

// One 16 B register load -> V floats (bf16: pure shifts/masks, exact). Going
// through the uint4 value keeps the load a single dwordx4 the scheduler can
// issue early; aliasing a T[V] array let the compiler split and sink it.
template <typename T, int V>
__device__ __forceinline__ void unpack_f32(const uint4& raw, float (&f)[V]) {
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    if constexpr (sizeof(T) == 2) {
        static_assert(V == 8, "16 B of bf16");
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(w[i] << 16);
            f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    } else {
        static_assert(V == 4, "16 B of fp32");
        #pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(w[i]);
    }
}

// ---- BatchNorm affine, shared by every kernel that evaluates it ------------
// The forward finalize, bn_apply and the kernels that recompute the ReLU
// mask from x must agree bit for bit, so the expressions live here once.
// Explicit intrinsics, so no kernel's result depends on how the compiler
// chose to contract a*b+c there.
__device__ __forceinline__ float bn_scale_of(float weight, float invstd) {
    return __fmul_rn(weight, invstd);
}
__device__ __forceinline__ float bn_shift_of(float bias, float mean,
                                             float scale) {
    return __fmaf_rn(-mean, scale, bias);
}
__device__ __forceinline__ float bn_affine(float x, float scale, float shift) {
    return __fmaf_rn(x, scale, shift);
}
// Backward dx of one element: g is the (masked) output gradient, k1/k2 the
// finalize's sum_g/m and sum_g_xhat/m. Shared by the generic and the fused
// stem backward-apply kernels, which must agree bit for bit.
__device__ __forceinline__ float bn_bwd_dx(float g, float xhat, float k1,
                                           float k2, float weight,
                                           float invstd) {
    return (g - k1 - xhat * k2) * weight * invstd;
}
// Round V floats through the storage dtype: what a store_f32 + load_f32
// round trip yields, kept in registers.
template <typename T, int V>
__device__ __forceinline__ void round_storage(float (&f)[V]) {
    if constexpr (sizeof(T) == 2) {
        #pragma unroll
        for (int i = 0; i < V; ++i) {
            T t;
            store_f32(&t, f[i]);
            f[i] = load_f32(&t);
        }
    }
}

// True iff a non-residual ReLU BN's stored activation is positive: the value
// bn_apply stores, max(affine(x), 0) rounded to the storage dtype, as the
// backward kernels would load it from `out`.
template <typename T>
__device__ __forceinline__ bool bn_relu_positive(float x, float scale,
                                                 float shift) {
    T t;
    store_f32(&t, fmaxf(bn_affine(x, scale, shift), 0.f));
    return load_f32(&t) > 0.f;
}

// xcd_contiguous_block (the XCD-aware block remap) lives in fda_kernels.h:
// the bindings decode block ids with it on the host.

// ---- wave / block reductions ----------------------------------------------
__device__ __forceinline__ float wave_reduce_sum(float v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;  // valid in lane 0 of the wave
}
__device__ __forceinline__ float wave_reduce_max(float v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, WAVE));
    return v;
}

// Block-wide reduce for blockDim.x <= 1024 (multiple of 64). `scratch` needs
// blockDim.x/64 floats. Result broadcast to all threads.
__device__ __forceinline__ float block_reduce_sum(float v, float* scratch) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    const int nw = blockDim.x / WAVE;
    v = wave_reduce_sum(v);
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float r = (lane < nw) ? scratch[lane] : 0.f;
    r = wave_reduce_sum(r);
    r = __shfl(r, 0, WAVE);
    __syncthreads();
    if (threadIdx.x == 0) scratch[0] = r;
    __syncthreads();
    return scratch[0];
}
__device__ __forceinline__ float block_reduce_max(float v, float* scratch) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
    const int nw = blockDim.x / WAVE;
    v = wave_reduce_max(v);
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float r = (lane < nw) ? scratch[lane] : -INFINITY;
    r = wave_reduce_max(r);
    r = __shfl(r, 0, WAVE);
    __syncthreads();
    if (threadIdx.x == 0) scratch[0] = r;
    __syncthreads();
    return scratch[0];
}

// V per-channel fp32 accumulators of one thread. A struct, so that the fold
// below can take them by value: an array passed by reference is not split
// into scalars until the helper has been inlined, and the compiler then
// keeps it as one <V x float> through the accumulation loop, which costs
// registers (bn_bwd_stats_kernel<bf16> lost a wave per SIMD that way).
template <int V> struct ChanAcc { float v[V]; };

// Fold the (s, q) accumulators of a block laid out as (blockDim.x / tpr row
// groups) x (tpr threads, V channels each) over its row groups, and store
// the totals as one partial row: out[0][c] = sum s, out[1][c] = sum q, the
// two halves `stride` floats apart. One array per pass through `smem`
// (blockDim.x * V floats), groups added in ascending order by the first
// group's threads — the order every partial row is defined by. Fully
// unrolled, so s and q stay in registers.
template <int V>
__device__ __forceinline__ void block_fold_rows(ChanAcc<V> s, ChanAcc<V> q,
                                                float* smem, float* out,
                                                int tpr, int stride) {
    const int rpb = blockDim.x / tpr;
    const int lane_c = threadIdx.x % tpr;
    const int sub_r = threadIdx.x / tpr;
    #pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float* loc = pass == 0 ? s.v : q.v;
        #pragma unroll
        for (int k = 0; k < V; ++k) smem[threadIdx.x * V + k] = loc[k];
        __syncthreads();
        if (sub_r == 0) {
            float acc[V];
            #pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0.f;
            for (int rr = 0; rr < rpb; ++rr) {
                const float* src = smem + (rr * tpr + lane_c) * V;
                #pragma unroll
                for (int k = 0; k < V; ++k) acc[k] += src[k];
            }
            #pragma unroll
            for (int k = 0; k < V; ++k)
                out[pass * stride + lane_c * V + k] = acc[k];
        }
        __syncthreads();
    }
}

}  // namespace fda
