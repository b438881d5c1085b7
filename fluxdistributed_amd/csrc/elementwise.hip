// Elementwise fused kernels: logit cross-entropy (fwd computes loss AND
// dlogits in one read), residual add+ReLU fwd/bwd, fused flat optimizers.
//
// Reference behaviors re-implemented MI355X-native:
//   loss:      /root/reference/src/ddp_tasks.jl:28 (logitcrossentropy)
//   optimizer: Optimisers.Momentum / ADAM applied leaf-wise at
//              ddp_tasks.jl:168 -> here ONE kernel over a flat buffer.
//
// All streaming kernels are 16 B/lane vectorized (guide G13), grid-stride,
// blocks of 256 (4 waves).
#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

// --------------------------------------------------------------------------
// Fused logit cross-entropy. One block (256 threads) per row; the row is
// staged once in LDS as f32, then max/sumexp/dlogits run from LDS.
// loss += -(x_t - m - log(sum)) / N  (atomic, one lane per row)
// dlogits = (softmax - onehot) / N
// --------------------------------------------------------------------------
template <typename T>
__global__ void ce_fwd_kernel(const T* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              float* __restrict__ loss, T* __restrict__ dlogits,
                              int N, int C, int ldl) {
    // ldl: logits row stride in elements (>= C). The FC head computes
    // logits in a %64-padded buffer (ops/linear.py), so CE reads the
    // padded rows in place instead of forcing a contiguity copy.
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* row = smem;            // C floats
    float* scratch = smem + C;    // block-reduce scratch (<= 16 floats)

    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const T* xrow = logits + (int64_t)n * ldl;
        T* drow = dlogits + (int64_t)n * C;
        const int t = (int)target[n];

        float lmax = -INFINITY;
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float v = load_f32(xrow + c);
            row[c] = v;
            lmax = fmaxf(lmax, v);
        }
        __syncthreads();
        const float m = block_reduce_max(lmax, scratch);

        float lsum = 0.f;
        for (int c = threadIdx.x; c < C; c += blockDim.x)
            lsum += __expf(row[c] - m);
        const float sum = block_reduce_sum(lsum, scratch);
        const float inv_sum = 1.f / sum;
        const float inv_n = 1.f / (float)N;

        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            float d = __expf(row[c] - m) * inv_sum;
            if (c == t) d -= 1.f;
            store_f32(drow + c, d * inv_n);
        }
        if (threadIdx.x == 0)
            atomicAdd(loss, -(row[t] - m - __logf(sum)) * inv_n);
        __syncthreads();  // protect `row` before next grid-stride iteration
    }
}

void ce_fwd_launch(const void* logits, const int64_t* target, float* loss,
                   void* dlogits, int N, int C, int ldl, DT dt,
                   hipStream_t s) {
    dim3 grid(N < 2048 ? N : 2048), block(256);
    size_t shmem = (C + 16) * sizeof(float);
    dispatch_dtype(dt, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL(ce_fwd_kernel<T>, grid, block, shmem, s,
                           (const T*)logits, target, loss, (T*)dlogits, N, C,
                           ldl);
    });
}

// --------------------------------------------------------------------------
// add+ReLU fwd/bwd, 16B/lane vectorized with scalar tail.
// --------------------------------------------------------------------------
template <typename T, int V>
__global__ void add_relu_fwd_kernel(const T* __restrict__ x,
                                    const T* __restrict__ r,
                                    T* __restrict__ out, int64_t n) {
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        T xv[V], rv[V], ov[V];
        *(uint4*)xv = ((const uint4*)x)[i];
        *(uint4*)rv = ((const uint4*)r)[i];
        #pragma unroll
        for (int k = 0; k < V; ++k)
            store_f32(ov + k, fmaxf(to_f32(load_f32(xv + k)) + load_f32(rv + k), 0.f));
        ((uint4*)out)[i] = *(uint4*)ov;
    }
    // tail
    const int64_t base = nv * V;
    for (int64_t i = base + blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        store_f32(out + i, fmaxf(load_f32(x + i) + load_f32(r + i), 0.f));
}

template <typename T, int V>
__global__ void add_relu_bwd_kernel(const T* __restrict__ gout,
                                    const T* __restrict__ out,
                                    T* __restrict__ gx, int64_t n) {
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        T gv[V], ov[V], rv[V];
        *(uint4*)gv = ((const uint4*)gout)[i];
        *(uint4*)ov = ((const uint4*)out)[i];
        #pragma unroll
        for (int k = 0; k < V; ++k)
            store_f32(rv + k, load_f32(ov + k) > 0.f ? load_f32(gv + k) : 0.f);
        ((uint4*)gx)[i] = *(uint4*)rv;
    }
    const int64_t base = nv * V;
    for (int64_t i = base + blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        store_f32(gx + i, load_f32(out + i) > 0.f ? load_f32(gout + i) : 0.f);
}

void add_relu_fwd_launch(const void* x, const void* r, void* out, int64_t n,
                         DT dt, hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((add_relu_fwd_kernel<T, V>),
                           dim3(grid_1d(n / V, 4096)), dim3(256), 0, s,
                           (const T*)x, (const T*)r, (T*)out, n);
    });
}

void add_relu_bwd_launch(const void* gout, const void* out, void* gx, int64_t n,
                         DT dt, hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((add_relu_bwd_kernel<T, V>),
                           dim3(grid_1d(n / V, 4096)), dim3(256), 0, s,
                           (const T*)gout, (const T*)out, (T*)gx, n);
    });
}

// --------------------------------------------------------------------------
// Fused flat optimizers. One launch updates the whole model. 4 f32 / 8 bf16
// elements per lane; flat buffers are 64-element aligned so n % V == 0 holds
// for the padded length (binding asserts).
// --------------------------------------------------------------------------
template <typename T, int V, bool MASTER, bool NESTEROV>
__global__ void sgd_step_kernel(T* __restrict__ P, const T* __restrict__ G,
                                float* __restrict__ M, float* __restrict__ Vm,
                                int64_t n, float lr, float mom, float wd) {
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        T gv[V], pv[V];
        float mv[V], vv[V];
        *(uint4*)gv = ((const uint4*)G)[i];
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            *(float4*)(vv + 4 * k) = ((const float4*)Vm)[i * (V / 4) + k];
            if constexpr (MASTER)
                *(float4*)(mv + 4 * k) = ((const float4*)M)[i * (V / 4) + k];
        }
        if constexpr (!MASTER) {
            *(uint4*)pv = ((const uint4*)P)[i];
            #pragma unroll
            for (int k = 0; k < V; ++k) mv[k] = load_f32(pv + k);
        }
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            float g = load_f32(gv + k);
            if (wd != 0.f) g += wd * mv[k];
            vv[k] = mom * vv[k] + g;
            float upd = NESTEROV ? g + mom * vv[k] : vv[k];
            mv[k] -= lr * upd;
            store_f32(pv + k, mv[k]);
        }
        ((uint4*)P)[i] = *(uint4*)pv;
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            ((float4*)Vm)[i * (V / 4) + k] = *(float4*)(vv + 4 * k);
            if constexpr (MASTER)
                ((float4*)M)[i * (V / 4) + k] = *(float4*)(mv + 4 * k);
        }
    }
}

template <typename T, int V, bool MASTER>
__global__ void adam_step_kernel(T* __restrict__ P, const T* __restrict__ G,
                                 float* __restrict__ M, float* __restrict__ V1,
                                 float* __restrict__ V2, int64_t n, float lr,
                                 float b1, float b2, float eps, float wd,
                                 float inv_bc1, float inv_bc2) {
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        T gv[V], pv[V];
        float mv[V], m1[V], m2[V];
        *(uint4*)gv = ((const uint4*)G)[i];
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            *(float4*)(m1 + 4 * k) = ((const float4*)V1)[i * (V / 4) + k];
            *(float4*)(m2 + 4 * k) = ((const float4*)V2)[i * (V / 4) + k];
            if constexpr (MASTER)
                *(float4*)(mv + 4 * k) = ((const float4*)M)[i * (V / 4) + k];
        }
        if constexpr (!MASTER) {
            *(uint4*)pv = ((const uint4*)P)[i];
            #pragma unroll
            for (int k = 0; k < V; ++k) mv[k] = load_f32(pv + k);
        }
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            float g = load_f32(gv + k);
            if (wd != 0.f) g += wd * mv[k];
            m1[k] = b1 * m1[k] + (1.f - b1) * g;
            m2[k] = b2 * m2[k] + (1.f - b2) * g * g;
            float denom = __fsqrt_rn(m2[k] * inv_bc2) + eps;
            mv[k] -= lr * (m1[k] * inv_bc1) / denom;
            store_f32(pv + k, mv[k]);
        }
        ((uint4*)P)[i] = *(uint4*)pv;
        #pragma unroll
        for (int k = 0; k < V / 4; ++k) {
            ((float4*)V1)[i * (V / 4) + k] = *(float4*)(m1 + 4 * k);
            ((float4*)V2)[i * (V / 4) + k] = *(float4*)(m2 + 4 * k);
            if constexpr (MASTER)
                ((float4*)M)[i * (V / 4) + k] = *(float4*)(mv + 4 * k);
        }
    }
}

void sgd_step_launch(void* P, const void* G, float* M, float* V, int64_t n,
                     float lr, float mom, float wd, bool nesterov,
                     bool has_master, DT dt, hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int VW = decltype(v)::value;
        dispatch_flag(nesterov, [&](auto NE) {
            auto launch = [&](auto MA) {
                hipLaunchKernelGGL(
                    (sgd_step_kernel<T, VW, MA.value, NE.value>),
                    dim3(grid_1d(n / VW, 4096)), dim3(256), 0, s, (T*)P,
                    (const T*)G, M, V, n, lr, mom, wd);
            };
            // bf16 params always step through their fp32 master
            if constexpr (sizeof(T) == 2) launch(std::true_type{});
            else dispatch_flag(has_master, launch);
        });
    });
}

void adam_step_launch(void* P, const void* G, float* M, float* V, float* S,
                      int64_t n, float lr, float b1, float b2, float eps,
                      float wd, float bc1, float bc2, bool has_master, DT dt,
                      hipStream_t s) {
    const float i1 = 1.f / bc1, i2 = 1.f / bc2;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int VW = decltype(v)::value;
        auto launch = [&](auto MA) {
            hipLaunchKernelGGL((adam_step_kernel<T, VW, MA.value>),
                               dim3(grid_1d(n / VW, 4096)), dim3(256), 0, s,
                               (T*)P, (const T*)G, M, V, S, n, lr, b1, b2, eps,
                               wd, i1, i2);
        };
        // bf16 params always step through their fp32 master
        if constexpr (sizeof(T) == 2) launch(std::true_type{});
        else dispatch_flag(has_master, launch);
    });
}

// --------------------------------------------------------------------------
// Replica gradient mean for task-DDP (parallel/flatsync.py): the R flat G
// buffers of one dtype group become their mean, in place, in one launch.
//   mean = round(((g0 + g1) + ... + gR-1) / R)   fp32 sum in replica order,
// one correctly rounded division, one round to the storage dtype; the same
// 16 B then goes to all R buffers. The pointers travel by value in the
// kernel arguments (no device table, no H2D copy; the launch stays
// capturable) and R is a template parameter, so a lane issues its R loads
// back to back before the first add and before any store. Bit-exact against
// the torch definition: adds and one division only, nothing to contract.
// --------------------------------------------------------------------------
struct GradBufs { void* p[GRAD_MEAN_MAX_R]; };

template <typename T, int V, int R>
__global__ __launch_bounds__(256) void grad_mean_multi_kernel(
    GradBufs bufs, int64_t n, int* __restrict__ nonfinite) {
    const int64_t nv = n / V;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        uint4 raw[R];
        #pragma unroll
        for (int r = 0; r < R; ++r) raw[r] = ((const uint4*)bufs.p[r])[i];
        float acc[V];
        unpack_f32<T, V>(raw[0], acc);
        #pragma unroll
        for (int r = 1; r < R; ++r) {
            float f[V];
            unpack_f32<T, V>(raw[r], f);
            #pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += f[k];
        }
        T ov[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            store_f32(ov + k, __fdiv_rn(acc[k], (float)R));
            // Inf/NaN of the value as stored (all exponent bits set)
            bad |= (__float_as_uint(load_f32(ov + k)) & 0x7f800000u) ==
                   0x7f800000u;
        }
        const uint4 o = *(const uint4*)ov;
        #pragma unroll
        for (int r = 0; r < R; ++r) ((uint4*)bufs.p[r])[i] = o;
    }
    // failure case only: at most one vector atomic per lane, none otherwise
    if (nonfinite != nullptr && bad) atomicOr(nonfinite, 1);
}

template <typename T, int V, int R>
static void grad_mean_multi_dispatch(const GradBufs& bufs, int nbufs,
                                     int64_t n, int* nonfinite,
                                     hipStream_t s) {
    if constexpr (R <= GRAD_MEAN_MAX_R) {
        if (nbufs == R)
            hipLaunchKernelGGL((grad_mean_multi_kernel<T, V, R>),
                               dim3(grid_1d(n / V, 4096)), dim3(256), 0, s,
                               bufs, n, nonfinite);
        else
            grad_mean_multi_dispatch<T, V, R + 1>(bufs, nbufs, n, nonfinite,
                                                  s);
    }
}

void grad_mean_multi_launch(void* const* bufs, int R, int64_t n,
                            int* nonfinite, DT dt, hipStream_t s) {
    if (R < 1 || R > GRAD_MEAN_MAX_R) return;  // the binding refuses these
    GradBufs b{};
    for (int r = 0; r < R; ++r) b.p[r] = bufs[r];
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        grad_mean_multi_dispatch<T, V, 1>(b, R, n, nonfinite, s);
    });
}

// G_bf16 += cast(ws_f32): the direct-grad flush for one conv weight slice
// (replaces an aten cast kernel + an AccumulateGrad add per layer).
__global__ __launch_bounds__(256) void grad_accum_bf16_kernel(
    unsigned short* __restrict__ g, const float* __restrict__ ws, long n) {
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i0 + 8 <= n) {
        unsigned short gv[8];
        *(uint4*)gv = *(const uint4*)(g + i0);
        float wv[8];
        *(float4*)(wv) = *(const float4*)(ws + i0);
        *(float4*)(wv + 4) = *(const float4*)(ws + i0 + 4);
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            gv[e] = f32_to_bf16bits(bf16bits_to_f32(gv[e]) + wv[e]);
        *(uint4*)(g + i0) = *(const uint4*)gv;
    } else {
        for (long i = i0; i < n; ++i)
            g[i] = f32_to_bf16bits(bf16bits_to_f32(g[i]) + ws[i]);
    }
}

void grad_accum_bf16_launch(void* g, const float* ws, long n, hipStream_t s) {
    const long lanes = (n + 7) / 8;
    dim3 grid((unsigned)((lanes + 255) / 256));
    hipLaunchKernelGGL(grad_accum_bf16_kernel, grid, dim3(256), 0, s,
                       (unsigned short*)g, ws, n);
}

// Batched variant: all ~36 per-layer direct-grad flushes of one backward
// in a single launch (per-layer launches measured ~180 us/step, mostly
// launch+tail overhead). grid.y = tensor index, grid.x = 2048-element
// chunks of the largest tensor; short tensors early-exit.
__global__ __launch_bounds__(256) void grad_accum_batch_kernel(
    const long* __restrict__ g_ptrs, const long* __restrict__ ws_ptrs,
    const long* __restrict__ ns) {
    const long n = ns[blockIdx.y];
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i0 >= n) return;
    unsigned short* g = (unsigned short*)g_ptrs[blockIdx.y];
    const float* ws = (const float*)ws_ptrs[blockIdx.y];
    if (i0 + 8 <= n) {
        unsigned short gv[8];
        *(uint4*)gv = *(const uint4*)(g + i0);
        float wv[8];
        *(float4*)(wv) = *(const float4*)(ws + i0);
        *(float4*)(wv + 4) = *(const float4*)(ws + i0 + 4);
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            gv[e] = f32_to_bf16bits(bf16bits_to_f32(gv[e]) + wv[e]);
        *(uint4*)(g + i0) = *(const uint4*)gv;
    } else {
        for (long i = i0; i < n; ++i)
            g[i] = f32_to_bf16bits(bf16bits_to_f32(g[i]) + ws[i]);
    }
}

void grad_accum_batch_launch(const long* g_ptrs, const long* ws_ptrs,
                             const long* ns, int ntensors, long max_n,
                             hipStream_t s) {
    const long lanes = (max_n + 7) / 8;
    dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)ntensors);
    hipLaunchKernelGGL(grad_accum_batch_kernel, grid, dim3(256), 0, s,
                       g_ptrs, ws_ptrs, ns);
}

// Ordered fold of the wgrad slabs (conv_wgrad_kernel, WG_SLAB): element i of
// the result is ((slab[0][i] + slab[1][i]) + slab[2][i]) + ..., fp32 adds
// strictly in chunk order, no atomics and no split of the chunk range, so
// the bits do not depend on the run. A lane owns 4 consecutive elements (8
// measured slower alone and the same inside the flush,
// profiles/wgrad_slab.md) and reads 16 B per slab, four chunks' loads in
// flight before their adds. BF16: g = bf16(f32(g) + s), the expression of
// grad_accum_bf16_kernel; else out = s in fp32. n % 4 == 0.
template <bool BF16>
__global__ __launch_bounds__(256) void wgrad_slab_fold_kernel(
    const float* __restrict__ slab, int nch, long n, void* __restrict__ out) {
    constexpr int U = 4;
    const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const float* p = slab + i0;
    float4 s = *(const float4*)p;
    int c = 1;
    for (; c + U <= nch; c += U) {
        float4 t[U];
        #pragma unroll
        for (int u = 0; u < U; ++u)
            t[u] = *(const float4*)(p + (long)(c + u) * n);
        #pragma unroll
        for (int u = 0; u < U; ++u) {
            s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w;
        }
    }
    for (; c < nch; ++c) {
        const float4 t = *(const float4*)(p + (long)c * n);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    if constexpr (BF16) {
        unsigned short* g = (unsigned short*)out + i0;
        unsigned short gv[4];
        *(uint2*)gv = *(const uint2*)g;
        const float sv[4] = {s.x, s.y, s.z, s.w};
        #pragma unroll
        for (int e = 0; e < 4; ++e)
            gv[e] = f32_to_bf16bits(bf16bits_to_f32(gv[e]) + sv[e]);
        *(uint2*)g = *(const uint2*)gv;
    } else {
        *(float4*)((float*)out + i0) = s;
    }
}

void wgrad_slab_fold_launch(const float* slab, int nch, long n, void* out,
                            bool out_bf16, hipStream_t s) {
    const dim3 grid((unsigned)((n / 4 + 255) / 256));
    dispatch_flag(out_bf16, [&](auto b) {
        hipLaunchKernelGGL((wgrad_slab_fold_kernel<decltype(b)::value>), grid,
                           dim3(256), 0, s, slab, nch, n, out);
    });
}

// --------------------------------------------------------------------------
// FC head support (ops/linear.py): the Dense layer runs on the conv
// implicit-GEMM kernels with out_features padded to a multiple of 64
// (conv_igemm requires K % 64 == 0; the reference's FC is 512->1000).
// These three kernels keep that padding in-house — no aten copies.
// --------------------------------------------------------------------------

// dst[M][ldl] = src[M][C] with cols [C, ldl) zeroed (row padding)
__global__ __launch_bounds__(256) void pad_rows_bf16_kernel(
    unsigned short* __restrict__ dst, const unsigned short* __restrict__ src,
    long M, int C, int ldl) {
    const long nv = M * (long)(ldl / 8);
    const int cv = C / 8, lv = ldl / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (long)gridDim.x * blockDim.x) {
        const long m = i / lv;
        const int c8 = (int)(i % lv);
        uint4 v = {0, 0, 0, 0};
        if (c8 < cv) v = *(const uint4*)(src + m * C + c8 * 8);
        *(uint4*)(dst + m * ldl + c8 * 8) = v;
    }
}

void pad_rows_bf16_launch(void* dst, const void* src, long M, int C, int ldl,
                          hipStream_t s) {
    const long nv = M * (long)(ldl / 8);
    hipLaunchKernelGGL(pad_rows_bf16_kernel, dim3(grid_1d(nv, 4096)),
                       dim3(256), 0, s,
                       (unsigned short*)dst, (const unsigned short*)src,
                       M, C, ldl);
}

// y[M][ldl] += bias[ldl] (bias pre-padded with zeros)
__global__ __launch_bounds__(256) void bias_add_rows_bf16_kernel(
    unsigned short* __restrict__ y, const unsigned short* __restrict__ bias,
    long M, int ldl) {
    const long nv = M * (long)(ldl / 8);
    const int lv = ldl / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % lv);
        unsigned short yv[8], bv[8];
        *(uint4*)yv = *(const uint4*)(y + (i / lv) * ldl + c8 * 8);
        *(uint4*)bv = *(const uint4*)(bias + c8 * 8);
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            yv[e] = f32_to_bf16bits(bf16bits_to_f32(yv[e]) +
                                    bf16bits_to_f32(bv[e]));
        *(uint4*)(y + (i / lv) * ldl + c8 * 8) = *(uint4*)yv;
    }
}

void bias_add_rows_bf16_launch(void* y, const void* bias, long M, int ldl,
                               hipStream_t s) {
    const long nv = M * (long)(ldl / 8);
    hipLaunchKernelGGL(bias_add_rows_bf16_kernel, dim3(grid_1d(nv, 4096)),
                       dim3(256), 0, s,
                       (unsigned short*)y, (const unsigned short*)bias, M,
                       ldl);
}

// bias grad: g_bf16[c] += cast(sum_m dy[m][c]) for c < Cvalid.
// One block covers 256 columns; row reads are lane-consecutive (coalesced).
__global__ __launch_bounds__(256) void colsum_accum_bf16_kernel(
    unsigned short* __restrict__ g, const unsigned short* __restrict__ dy,
    long M, int ldl, int Cvalid) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ldl) return;
    float acc = 0.f;
    for (long m = 0; m < M; ++m) acc += bf16bits_to_f32(dy[m * ldl + c]);
    if (c < Cvalid)
        g[c] = f32_to_bf16bits(bf16bits_to_f32(g[c]) + acc);
}

void colsum_accum_bf16_launch(void* g, const void* dy, long M, int ldl,
                              int Cvalid, hipStream_t s) {
    dim3 grid((unsigned)((ldl + 255) / 256));
    hipLaunchKernelGGL(colsum_accum_bf16_kernel, grid, dim3(256), 0, s,
                       (unsigned short*)g, (const unsigned short*)dy, M, ldl,
                       Cvalid);
}

}  // namespace fda
