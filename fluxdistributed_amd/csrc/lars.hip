// LARS on the flat optimizer buffers: per-segment squared norms, trust
// ratios, global-norm clipping and the momentum update (ops/fused_optim.py,
// FusedLARS; the definition is in docs/training.md).
//
// A segment is one parameter's slice of a flat group buffer. Work is
// distributed by a chunk table built on the host (lars_plan, bindings.cpp):
// a row {segment id, start element, count} is a run of at most LARS_CHUNK of
// the parameter's own elements that starts a multiple of 64 elements into
// the segment, so every 16-B access is aligned and a 2.4 M-element conv
// weight spreads over hundreds of blocks while a BN vector takes one.
//
//   lars_norms_kernel  one block per chunk, one launch per flat group:
//                      partials[chunk] = {sum w^2, sum g^2} (double). fp32
//                      squares per lane, then wave shuffle -> LDS -> global
//                      partials; no atomics, so bitwise reproducible.
//   lars_fold_kernel   one block for the whole optimizer: folds every
//                      segment's partials in double in a fixed order, then
//                      gnorm, clip and coef_s = lr * trust_s. lr comes from
//                      device memory, so a captured graph follows a schedule.
//   lars_step_kernel   one block per chunk, one launch per flat group:
//                      u = clip g + wd_s w; v = mom v + coef_s u; w -= v;
//                      P = round(w). Returns at once when gnorm is not finite.
//
// The tables live in device memory, out of the bindings' reach: a row the
// kernels cannot trust (segment id >= S, misaligned start, range outside
// [0, n)) yields NaN partials in the norms pass and is skipped by the step
// pass without a single access through it; the NaN makes gnorm non-finite,
// which skips the whole step.
#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

namespace {

constexpr int LARS_THREADS = 256;
constexpr int LARS_FOLD_GROUP = 16;   // lanes that fold one segment together
constexpr int LARS_FOLD_GROUPS = LARS_THREADS / LARS_FOLD_GROUP;

struct LarsRow { int seg, start, count; bool ok; };

// Row `chunk` of the table, and whether its accesses stay inside [0, n).
// n and start are multiples of 64, so start + count <= n also covers the
// whole 16-B vector that holds the row's last element.
__device__ __forceinline__ LarsRow lars_row(const int* __restrict__ table,
                                            int chunk, long long n, int S) {
    const int* r = table + (long long)chunk * LARS_ROW_INTS;
    LarsRow row{r[0], r[1], r[2], false};
    row.ok = row.seg >= 0 && row.seg < S && row.start >= 0 &&
             (row.start & 63) == 0 && row.count >= 0 &&
             row.count <= LARS_CHUNK &&
             (long long)row.start + row.count <= n;
    return row;
}

__device__ __forceinline__ bool lars_finite(float v) {
    return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

template <typename T, int V, bool MASTER>
__global__ __launch_bounds__(LARS_THREADS) void lars_norms_kernel(
    const T* __restrict__ P, const T* __restrict__ G,
    const float* __restrict__ M, const int* __restrict__ table,
    double* __restrict__ partials, long long n, int S) {
    __shared__ double red[2 * (LARS_THREADS / WAVE)];
    const LarsRow row = lars_row(table, blockIdx.x, n, S);
    if (!row.ok) {   // block-uniform
        if (threadIdx.x == 0) {
            const double qnan = (double)__int_as_float(0x7fc00000);
            partials[2 * (long long)blockIdx.x] = qnan;
            partials[2 * (long long)blockIdx.x + 1] = qnan;
        }
        return;
    }
    float sw = 0.f, sg = 0.f;
    for (int e = threadIdx.x * V; e < row.count; e += LARS_THREADS * V) {
        const long long i = ((long long)row.start + e) / V;
        float g[V], w[V];
        unpack_f32<T, V>(((const uint4*)G)[i], g);
        if constexpr (MASTER) {
            #pragma unroll
            for (int k = 0; k < V / 4; ++k)
                *(float4*)(w + 4 * k) = ((const float4*)M)[i * (V / 4) + k];
        } else {
            unpack_f32<T, V>(((const uint4*)P)[i], w);
        }
        // only the last vector of a parameter can hold padding
        const int own = row.count - e;
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            if (k < own) {
                sw += w[k] * w[k];
                sg += g[k] * g[k];
            }
        }
    }
    double dw = (double)sw, dg = (double)sg;
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        dw += __shfl_down(dw, off, WAVE);
        dg += __shfl_down(dg, off, WAVE);
    }
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    if (lane == 0) {
        red[2 * wid] = dw;
        red[2 * wid + 1] = dg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dw = dg = 0.0;
        for (int i = 0; i < LARS_THREADS / WAVE; ++i) {
            dw += red[2 * i];
            dg += red[2 * i + 1];
        }
        partials[2 * (long long)blockIdx.x] = dw;
        partials[2 * (long long)blockIdx.x + 1] = dg;
    }
}

// seg_meta row: {first chunk, end chunk, flags}; flag bit 0 = adapt (trust
// ratio), bit 1 = decay (weight decay). 16 lanes fold one segment: lane l
// adds chunks first+l, first+l+16, ... in ascending order, then a 4-step
// shuffle tree; the 16 groups' gradient totals meet in LDS and every thread
// adds them in group order. All of it is a fixed order.
__global__ __launch_bounds__(LARS_THREADS) void lars_fold_kernel(
    const double* __restrict__ partials, int total_chunks,
    const int* __restrict__ seg_meta, int S, const float* __restrict__ lr_p,
    float eta, float wd, float eps, float max_grad_norm,
    float* __restrict__ coef, float* stats, int* __restrict__ skipped) {
    __shared__ double red[LARS_FOLD_GROUPS];
    const int grp = threadIdx.x / LARS_FOLD_GROUP;
    const int gl = threadIdx.x % LARS_FOLD_GROUP;
    float* const Ws = stats + LARS_STATS_HEAD;
    float* const Gs = Ws + S;

    double gtot = 0.0;
    for (int s = grp; s < S; s += LARS_FOLD_GROUPS) {
        const int lo = seg_meta[s * LARS_SEG_INTS];
        const int hi = seg_meta[s * LARS_SEG_INTS + 1];
        double w = 0.0, g = 0.0;
        if (lo >= 0 && hi >= lo && hi <= total_chunks) {
            for (int c = lo + gl; c < hi; c += LARS_FOLD_GROUP) {
                w += partials[2 * (long long)c];
                g += partials[2 * (long long)c + 1];
            }
        } else {
            w = g = (double)__int_as_float(0x7fc00000);
        }
        #pragma unroll
        for (int off = LARS_FOLD_GROUP / 2; off > 0; off >>= 1) {
            w += __shfl_down(w, off, LARS_FOLD_GROUP);
            g += __shfl_down(g, off, LARS_FOLD_GROUP);
        }
        if (gl == 0) {
            Ws[s] = (float)w;
            Gs[s] = (float)g;
            gtot += g;
        }
    }
    if (gl == 0) red[grp] = gtot;
    // phase two needs every segment's sums and the global norm
    __syncthreads();
    double gsum = 0.0;
    #pragma unroll
    for (int i = 0; i < LARS_FOLD_GROUPS; ++i) gsum += red[i];
    const float gnorm = (float)sqrt(gsum);
    const double clip =
        max_grad_norm > 0.f
            ? fmin(1.0, (double)max_grad_norm / ((double)gnorm + 1e-6))
            : 1.0;
    if (threadIdx.x == 0) {
        stats[0] = gnorm;
        stats[1] = (float)clip;
        if (!lars_finite(gnorm)) *skipped += 1;
    }
    const double lr = (double)lr_p[0];
    for (int s = threadIdx.x; s < S; s += LARS_THREADS) {
        const int flags = seg_meta[s * LARS_SEG_INTS + 2];
        const double wn = sqrt((double)Ws[s]);
        const double gn = (double)(float)clip * sqrt((double)Gs[s]);
        const double wds = (flags & 2) ? (double)wd : 0.0;
        double trust = 1.0;
        if ((flags & 1) && wn > 0.0 && gn > 0.0)
            trust = (double)eta * wn / (gn + wds * wn + (double)eps);
        coef[s] = (float)(lr * trust);
    }
}

template <typename T, int V, bool MASTER>
__global__ __launch_bounds__(LARS_THREADS) void lars_step_kernel(
    T* __restrict__ P, const T* __restrict__ G, float* __restrict__ M,
    float* __restrict__ Vm, const int* __restrict__ table,
    const int* __restrict__ seg_meta, const float* __restrict__ coef,
    const float* __restrict__ stats, long long n, int S, float mom,
    float wd) {
    if (!lars_finite(stats[0])) return;   // skipped step: nothing is written
    const LarsRow row = lars_row(table, blockIdx.x, n, S);
    if (!row.ok) return;
    // block-uniform
    const float clip = stats[1];
    const float cf = coef[row.seg];
    const float wds = (seg_meta[row.seg * LARS_SEG_INTS + 2] & 2) ? wd : 0.f;
    // whole padded vectors: padding holds zeros and stays zero
    for (int e = threadIdx.x * V; e < row.count; e += LARS_THREADS * V) {
        const long long i = ((long long)row.start + e) / V;
        T pv[V];
        float g[V], mv[V], vv[V];
        unpack_f32<T, V>(((const uint4*)G)[i], g);
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            *(float4*)(vv + 4 * k) = ((const float4*)Vm)[i * (V / 4) + k];
            if constexpr (MASTER)
                *(float4*)(mv + 4 * k) = ((const float4*)M)[i * (V / 4) + k];
        }
        if constexpr (!MASTER) unpack_f32<T, V>(((const uint4*)P)[i], mv);
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            const float u = clip * g[k] + wds * mv[k];
            vv[k] = mom * vv[k] + cf * u;
            mv[k] -= vv[k];
            store_f32(pv + k, mv[k]);
        }
        ((uint4*)P)[i] = *(const uint4*)pv;
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            ((float4*)Vm)[i * (V / 4) + k] = *(float4*)(vv + 4 * k);
            if constexpr (MASTER)
                ((float4*)M)[i * (V / 4) + k] = *(float4*)(mv + 4 * k);
        }
    }
}

}  // namespace

void lars_norms_launch(const void* P, const void* G, const float* M,
                       const int32_t* table, int nchunks, double* partials,
                       int64_t n, int S, bool has_master, DT dt,
                       hipStream_t s) {
    if (nchunks < 1) return;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int VW = decltype(v)::value;
        auto launch = [&](auto MA) {
            hipLaunchKernelGGL((lars_norms_kernel<T, VW, MA.value>),
                               dim3((unsigned)nchunks), dim3(LARS_THREADS), 0,
                               s, (const T*)P, (const T*)G, M, table, partials,
                               (long long)n, S);
        };
        // bf16 params always step through their fp32 master
        if constexpr (sizeof(T) == 2) launch(std::true_type{});
        else dispatch_flag(has_master, launch);
    });
}

void lars_fold_launch(const double* partials, int total_chunks,
                      const int32_t* seg_meta, int S, const float* lr,
                      float eta, float wd, float eps, float max_grad_norm,
                      float* coef, float* stats, int* skipped,
                      hipStream_t s) {
    hipLaunchKernelGGL(lars_fold_kernel, dim3(1), dim3(LARS_THREADS), 0, s,
                       partials, total_chunks, seg_meta, S, lr, eta, wd, eps,
                       max_grad_norm, coef, stats, skipped);
}

void lars_step_launch(void* P, const void* G, float* M, float* V,
                      const int32_t* table, int nchunks,
                      const int32_t* seg_meta, const float* coef,
                      const float* stats, int64_t n, int S, float mom,
                      float wd, bool has_master, DT dt, hipStream_t s) {
    if (nchunks < 1) return;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int VW = decltype(v)::value;
        auto launch = [&](auto MA) {
            hipLaunchKernelGGL((lars_step_kernel<T, VW, MA.value>),
                               dim3((unsigned)nchunks), dim3(LARS_THREADS), 0,
                               s, (T*)P, (const T*)G, M, V, table, seg_meta,
                               coef, stats, (long long)n, S, mom, wd);
        };
        if constexpr (sizeof(T) == 2) launch(std::true_type{});
        else dispatch_flag(has_master, launch);
    });
}

}  // namespace fda
