// Fused BatchNorm(+residual add)(+ReLU), NHWC, training + eval, fwd + bwd.
//
// Replaces 3 separate launches (BN, add, ReLU) per ResNet block with one
// stats pass + one apply pass (fwd) and one stats + one apply (bwd) — the
// "fused BN+ReLU" requirement of BASELINE.json's north star. Reference
// behavior: Flux BatchNorm in Metalhead blocks, with
// per-replica running stats that are never synced across replicas.
//
// Layout: x is [rows = N*H*W][C] with C contiguous (torch channels_last).
// Stats accumulate in fp32; bf16 IO is 16 B/lane vectorized.
#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

// block = 256 threads split into (rows-per-block) x (threads-per-row);
// threads-per-row = chunkC / V so each thread owns V consecutive channels.
// Each block writes PARTIAL per-channel sums to part[block][2*chunkC]
// (plain coalesced stores — a global atomicAdd per channel serializes on
// L2 and was measured 30x slower); bn_stats_reduce_kernel folds partials.
template <typename T, int V>
__global__ void bn_stats_kernel(const T* __restrict__ x,
                                float* __restrict__ part, int64_t rows, int C,
                                int c_base, int chunkC) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 256*V floats
    const int tpr = chunkC / V;
    const int rpb = blockDim.x / tpr;
    const int lane_c = threadIdx.x % tpr;
    const int sub_r = threadIdx.x / tpr;
    const int c0 = c_base + lane_c * V;

    ChanAcc<V> s, q;
    #pragma unroll
    for (int k = 0; k < V; ++k) s.v[k] = q.v[k] = 0.f;

    // 2 independent row streams per iteration for memory-level parallelism
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + sub_r; r < rows;
         r += 2 * stride) {
        T xv[V], xw[V];
        *(uint4*)xv = *(const uint4*)(x + r * C + c0);
        const bool second = r + stride < rows;
        if (second) *(uint4*)xw = *(const uint4*)(x + (r + stride) * C + c0);
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            float v = load_f32(xv + k);
            s.v[k] += v;
            q.v[k] += v * v;
        }
        if (second) {
            #pragma unroll
            for (int k = 0; k < V; ++k) {
                float v = load_f32(xw + k);
                s.v[k] += v;
                q.v[k] += v * v;
            }
        }
    }
    block_fold_rows<V>(s, q, smem, part + (int64_t)blockIdx.x * 2 * chunkC,
                       tpr, chunkC);
}

// Fold part[NB][2*chunkC] into two per-channel totals (s, q), then run a
// per-channel epilogue — all in one launch. The launch is latency-bound
// (<= 1024 rows, written a moment earlier by other XCDs, so every load is
// a trip to memory), so the shape is chosen to put every load in flight at
// once: block = 4 float4-lanes (16 channels) x 64 partial-subgroups, grid =
// chunkC/16, and each thread issues its (up to) FIN_ROWS row loads before
// the first add. NB <= 512 is one batch; larger NB loops batches. The 64
// subgroups fold by wave shuffles, then one LDS hop across the 4 waves.
// chunkC must be a multiple of 16.
struct BnTotals { float s, q; };

constexpr int FIN_LANES = 4;     // float4 lanes per block -> 16 channels
constexpr int FIN_SUBS = 64;     // partial-row subgroups per block
constexpr int FIN_ROWS = 8;      // rows in flight per thread
constexpr int FIN_CH = FIN_LANES * 4;

template <typename EPI>
__device__ __forceinline__ void bn_reduce_then(const float* __restrict__ part,
                                               int NB, int chunkC, int c_base,
                                               EPI&& epilogue) {
    __shared__ float sm[4][2 * FIN_CH];  // [wave][s(16) | q(16)]
    const int lane = threadIdx.x & (FIN_LANES - 1);
    const int sub = threadIdx.x >> 2;
    const int cc = blockIdx.x * FIN_CH + lane * 4;  // channel quad in chunk
    float4 s = {0, 0, 0, 0}, q = {0, 0, 0, 0};
    for (int b0 = sub; b0 < NB; b0 += FIN_SUBS * FIN_ROWS) {
        float4 a[FIN_ROWS], z[FIN_ROWS];
        #pragma unroll
        for (int j = 0; j < FIN_ROWS; ++j) {
            const int b = b0 + j * FIN_SUBS;
            a[j] = z[j] = float4{0, 0, 0, 0};
            if (b < NB) {
                const float* p = part + (int64_t)b * 2 * chunkC;
                a[j] = *(const float4*)(p + cc);
                z[j] = *(const float4*)(p + chunkC + cc);
            }
        }
        #pragma unroll
        for (int j = 0; j < FIN_ROWS; ++j) {
            s.x += a[j].x; s.y += a[j].y; s.z += a[j].z; s.w += a[j].w;
            q.x += z[j].x; q.y += z[j].y; q.z += z[j].z; q.w += z[j].w;
        }
    }
    // a wave holds 16 subgroups x 4 lanes: fold the subgroups by xor-shuffle
    float v[8] = {s.x, s.y, s.z, s.w, q.x, q.y, q.z, q.w};
    #pragma unroll
    for (int off = FIN_LANES; off < WAVE; off <<= 1) {
        #pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += __shfl_xor(v[k], off, WAVE);
    }
    const int wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) < FIN_LANES) {
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            sm[wave][lane * 4 + k] = v[k];
            sm[wave][FIN_CH + lane * 4 + k] = v[4 + k];
        }
    }
    __syncthreads();
    // one thread per channel: the epilogue's own loads run 16 wide
    if (threadIdx.x < FIN_CH) {
        const int t = threadIdx.x;
        BnTotals tot{sm[0][t] + sm[1][t] + sm[2][t] + sm[3][t],
                     sm[0][FIN_CH + t] + sm[1][FIN_CH + t] +
                         sm[2][FIN_CH + t] + sm[3][FIN_CH + t]};
        epilogue(c_base + blockIdx.x * FIN_CH + t, tot);
    }
}

__global__ void bn_fwd_reduce_finalize_kernel(
    const float* __restrict__ part, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ rm,
    float* __restrict__ rv, float* __restrict__ save_mean,
    float* __restrict__ save_invstd, float* __restrict__ ws, int NB,
    int chunkC, int c_base, int C, int64_t rows, float momentum, float eps) {
    bn_reduce_then(part, NB, chunkC, c_base, [&](int c, BnTotals t) {
        const float inv_m = 1.f / (float)rows;
        const float mean = t.s * inv_m;
        const float var = fmaxf(t.q * inv_m - mean * mean, 0.f);
        const float invstd = rsqrtf(var + eps);
        rm[c] += momentum * (mean - rm[c]);
        const float unbias = rows > 1 ? (float)rows / (float)(rows - 1) : 1.f;
        rv[c] += momentum * (var * unbias - rv[c]);
        save_mean[c] = mean;
        save_invstd[c] = invstd;
        const float scale = bn_scale_of(weight[c], invstd);
        ws[c] = scale;
        ws[C + c] = bn_shift_of(bias[c], mean, scale);
    });
}

__global__ void bn_bwd_reduce_finalize_kernel(
    const float* __restrict__ part, float* __restrict__ ws,
    float* __restrict__ gw, float* __restrict__ gb, int NB, int chunkC,
    int c_base, int C, int64_t rows, int training, int accum) {
    bn_reduce_then(part, NB, chunkC, c_base, [&](int c, BnTotals t) {
        // accum: gw/gb are flat-G slices (direct grad, += semantics)
        gb[c] = accum ? gb[c] + t.s : t.s;  // sum_g
        gw[c] = accum ? gw[c] + t.q : t.q;  // sum_g_xhat
        const float inv_m = training ? 1.f / (float)rows : 0.f;
        ws[c] = t.s * inv_m;       // k1
        ws[C + c] = t.q * inv_m;   // k2
    });
}

// Eval-mode finalize: scale/shift from running stats (no batch reduction).
__global__ void bn_eval_finalize_kernel(float* __restrict__ ws,
                                        const float* __restrict__ weight,
                                        const float* __restrict__ bias,
                                        const float* __restrict__ rm,
                                        const float* __restrict__ rv,
                                        float* __restrict__ save_mean,
                                        float* __restrict__ save_invstd,
                                        int C, float eps) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mean = rm[c];
    const float invstd = rsqrtf(rv[c] + eps);
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    const float scale = bn_scale_of(weight[c], invstd);
    ws[c] = scale;
    ws[C + c] = bn_shift_of(bias[c], mean, scale);
}

// Eval-mode fold of every BN layer of a model in one launch (inference
// path): layer t = blockIdx.y writes scale[C] then shift[C] at arena +
// offs[t], the ws layout of bn_eval_finalize_kernel and, through the shared
// helpers, its exact values. Pointer tables as in wt_transpose_kernel. A
// slice that would leave the arena is skipped rather than trusted.
__global__ __launch_bounds__(256) void bn_fold_eval_batch_kernel(
    const long* __restrict__ w_ptrs, const long* __restrict__ b_ptrs,
    const long* __restrict__ rm_ptrs, const long* __restrict__ rv_ptrs,
    const int* __restrict__ Cs, const long* __restrict__ offs,
    const float* __restrict__ eps, float* __restrict__ arena,
    long arena_len) {
    const int t = blockIdx.y;
    const int C = Cs[t];
    const long off = offs[t];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C || off < 0 || off + 2L * C > arena_len) return;
    const float invstd = rsqrtf(((const float*)rv_ptrs[t])[c] + eps[t]);
    const float scale = bn_scale_of(((const float*)w_ptrs[t])[c], invstd);
    arena[off + c] = scale;
    arena[off + C + c] = bn_shift_of(((const float*)b_ptrs[t])[c],
                                     ((const float*)rm_ptrs[t])[c], scale);
}

template <typename T, int V, bool RELU, bool RES>
__global__ void bn_apply_kernel(const T* __restrict__ x,
                                const T* __restrict__ res, T* __restrict__ out,
                                const float* __restrict__ scale,
                                const float* __restrict__ shift, int64_t nvec,
                                int C) {
    const int cvec = C / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cvec) * V;
        T xv[V], rv_[V], ov[V];
        *(uint4*)xv = ((const uint4*)x)[i];
        if constexpr (RES) *(uint4*)rv_ = ((const uint4*)res)[i];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            float v = bn_affine(load_f32(xv + k), scale[c0 + k], shift[c0 + k]);
            if constexpr (RES) v += load_f32(rv_ + k);
            if constexpr (RELU) v = fmaxf(v, 0.f);
            store_f32(ov + k, v);
        }
        ((uint4*)out)[i] = *(uint4*)ov;
    }
}

// ---- backward -------------------------------------------------------------

// XMASK (non-residual ReLU BN only): the ReLU mask comes from the recomputed
// activation (bn_relu_positive: the sign the rounded, stored relu(x*scale+
// shift) has) instead of a read of `out` — x and
// the statistics are loaded anyway, so the `out` pass bought only a sign.
// The expression is the forward's (fda_common.h), so the mask is the same
// bit for bit. `out` is not touched in that variant.
template <typename T, int V, bool RELU, bool XMASK = false>
__global__ void bn_bwd_stats_kernel(const T* __restrict__ gout,
                                    const T* __restrict__ x,
                                    const T* __restrict__ out,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    const float* __restrict__ weight,
                                    const float* __restrict__ bias,
                                    float* __restrict__ part, int64_t rows,
                                    int C, int c_base, int chunkC) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tpr = chunkC / V;
    const int rpb = blockDim.x / tpr;
    const int lane_c = threadIdx.x % tpr;
    const int sub_r = threadIdx.x / tpr;
    const int c0 = c_base + lane_c * V;

    float mu[V], is[V], sc[V], sh[V];
    ChanAcc<V> sg, sgx;
    #pragma unroll
    for (int k = 0; k < V; ++k) {
        mu[k] = mean[c0 + k];
        is[k] = invstd[c0 + k];
        sg.v[k] = sgx.v[k] = 0.f;
        if constexpr (XMASK) {
            sc[k] = bn_scale_of(weight[c0 + k], is[k]);
            sh[k] = bn_shift_of(bias[c0 + k], mu[k], sc[k]);
        }
    }
    for (int64_t r = (int64_t)blockIdx.x * rpb + sub_r; r < rows;
         r += (int64_t)gridDim.x * rpb) {
        T gv[V], xv[V], ov[V];
        *(uint4*)gv = *(const uint4*)(gout + r * C + c0);
        *(uint4*)xv = *(const uint4*)(x + r * C + c0);
        if constexpr (RELU && !XMASK)
            *(uint4*)ov = *(const uint4*)(out + r * C + c0);
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            float g = load_f32(gv + k);
            if constexpr (XMASK)
                g = bn_relu_positive<T>(load_f32(xv + k), sc[k], sh[k]) ? g : 0.f;
            else if constexpr (RELU)
                g = load_f32(ov + k) > 0.f ? g : 0.f;
            const float xhat = (load_f32(xv + k) - mu[k]) * is[k];
            sg.v[k] += g;
            sgx.v[k] += g * xhat;
        }
    }
    block_fold_rows<V>(sg, sgx, smem,
                       part + (int64_t)blockIdx.x * 2 * chunkC, tpr, chunkC);
}

template <typename T, int V, bool RELU, bool XMASK = false>
__global__ void bn_bwd_apply_kernel(const T* __restrict__ gout,
                                    const T* __restrict__ x,
                                    const T* __restrict__ out,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    const float* __restrict__ weight,
                                    const float* __restrict__ bias,
                                    const float* __restrict__ k1,
                                    const float* __restrict__ k2,
                                    T* __restrict__ gx,
                                    T* __restrict__ gres,  // may be null
                                    int64_t nvec, int C) {
    // gres: the residual-branch gradient relu_mask*gout — a byproduct of
    // this kernel's own mask computation (saves the separate add_relu_bwd
    // pass the residual path used to run).
    const int cvec = C / V;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cvec) * V;
        T gv[V], xv[V], ov[V], rv_[V], mv[V];
        *(uint4*)gv = ((const uint4*)gout)[i];
        *(uint4*)xv = ((const uint4*)x)[i];
        if constexpr (RELU && !XMASK) *(uint4*)ov = ((const uint4*)out)[i];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            const int c = c0 + k;
            float g = load_f32(gv + k);
            const float is = invstd[c];
            if constexpr (XMASK) {
                const float sc = bn_scale_of(weight[c], is);
                const float sh = bn_shift_of(bias[c], mean[c], sc);
                g = bn_relu_positive<T>(load_f32(xv + k), sc, sh) ? g : 0.f;
            } else if constexpr (RELU) {
                g = load_f32(ov + k) > 0.f ? g : 0.f;
            }
            store_f32(mv + k, g);
            const float xhat = (load_f32(xv + k) - mean[c]) * is;
            store_f32(rv_ + k,
                      bn_bwd_dx(g, xhat, k1[c], k2[c], weight[c], is));
        }
        ((uint4*)gx)[i] = *(uint4*)rv_;
        if (gres != nullptr) ((uint4*)gres)[i] = *(uint4*)mv;
    }
}

// ---- launchers ------------------------------------------------------------

static inline void stats_geom(int C, int V, int64_t rows, int& chunkC,
                              int& nchunks, int& grid, int& shmem) {
    const int maxC = 256 * V;
    chunkC = C < maxC ? C : maxC;
    nchunks = (C + chunkC - 1) / chunkC;
    const int tpr = chunkC / V;
    const int rpb = 256 / tpr;
    int64_t blocks = (rows + rpb - 1) / rpb;
    grid = (int)(blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks));
    shmem = 256 * V * (int)sizeof(float);
}

int bn_stats_partial_floats(int C, int64_t rows, DT dt) {
    const int V = dt == DT::BF16 ? 8 : 4;
    int chunkC, nchunks, grid, shmem;
    stats_geom(C, V, rows, chunkC, nchunks, grid, shmem);
    return grid * 2 * chunkC;
}

void bn_stats_launch(const void* x, float* ws, float* part,
                     const float* weight, const float* bias,
                     float* running_mean, float* running_var, float* save_mean,
                     float* save_invstd, int64_t rows, int C, float momentum,
                     float eps, DT dt, hipStream_t s) {
    const int V = dt == DT::BF16 ? 8 : 4;
    int chunkC, nchunks, grid, shmem;
    stats_geom(C, V, rows, chunkC, nchunks, grid, shmem);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c_base = ch * chunkC;
        const int cc = (C - c_base) < chunkC ? (C - c_base) : chunkC;
        dispatch_dtype(dt, [&](auto t, auto v) {
            using T = decltype(t);
            constexpr int V = decltype(v)::value;
            hipLaunchKernelGGL((bn_stats_kernel<T, V>), dim3(grid), dim3(256),
                               shmem, s, (const T*)x, part, rows, C, c_base,
                               cc);
        });
        bn_fwd_finalize_launch(part, grid, cc, c_base, weight, bias,
                               running_mean, running_var, save_mean,
                               save_invstd, ws, rows, C, momentum, eps, s);
    }
}

void bn_fwd_finalize_launch(const float* part, int NB, int chunkC, int c_base,
                            const float* weight, const float* bias, float* rm,
                            float* rv, float* save_mean, float* save_invstd,
                            float* ws, int64_t rows, int C, float momentum,
                            float eps, hipStream_t s) {
    hipLaunchKernelGGL(bn_fwd_reduce_finalize_kernel, dim3(chunkC / FIN_CH),
                       dim3(256), 0, s, part, weight, bias, rm, rv, save_mean,
                       save_invstd, ws, NB, chunkC, c_base, C, rows, momentum,
                       eps);
}

void bn_eval_finalize_launch(float* ws, const float* weight,
                             const float* bias, const float* running_mean,
                             const float* running_var, float* save_mean,
                             float* save_invstd, int C, float eps,
                             hipStream_t s) {
    hipLaunchKernelGGL(bn_eval_finalize_kernel, dim3((C + 255) / 256),
                       dim3(256), 0, s, ws, weight, bias, running_mean,
                       running_var, save_mean, save_invstd, C, eps);
}

void bn_fold_eval_batch_launch(const long* w_ptrs, const long* b_ptrs,
                               const long* rm_ptrs, const long* rv_ptrs,
                               const int* Cs, const long* offs,
                               const float* eps, float* arena, long arena_len,
                               int nlayers, int max_c, hipStream_t s) {
    dim3 grid((unsigned)((max_c + 255) / 256), (unsigned)nlayers);
    hipLaunchKernelGGL(bn_fold_eval_batch_kernel, grid, dim3(256), 0, s,
                       w_ptrs, b_ptrs, rm_ptrs, rv_ptrs, Cs, offs, eps, arena,
                       arena_len);
}

void bn_apply_launch(const void* x, const void* residual, void* out,
                     const float* ws, int64_t rows, int C, bool relu, DT dt,
                     hipStream_t s) {
    const float* scale = ws;
    const float* shift = ws + C;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        const int64_t nvec = rows * C / V;
        dispatch_flag(relu, [&](auto RELU) {
            dispatch_flag(residual != nullptr, [&](auto RES) {
                hipLaunchKernelGGL(
                    (bn_apply_kernel<T, V, RELU.value, RES.value>),
                    dim3(grid_1d(nvec, 4096)), dim3(256), 0, s, (const T*)x,
                    (const T*)residual, (T*)out, scale, shift, nvec, C);
            });
        });
    });
}

void bn_bwd_stats_launch(const void* gout, const void* x, const void* out,
                         const float* save_mean, const float* save_invstd,
                         float* ws, float* part, float* gw, float* gb,
                         int64_t rows, int C, bool relu, bool training,
                         bool accum_g, DT dt, hipStream_t s,
                         const float* weight, const float* bias) {
    // weight+bias given (non-residual ReLU BN): mask from x, `out` unread
    const bool xmask = relu && weight != nullptr && bias != nullptr;
    const int V = dt == DT::BF16 ? 8 : 4;
    int chunkC, nchunks, grid, shmem;
    stats_geom(C, V, rows, chunkC, nchunks, grid, shmem);
    for (int ch = 0; ch < nchunks; ++ch) {
        const int c_base = ch * chunkC;
        const int cc = (C - c_base) < chunkC ? (C - c_base) : chunkC;
        dispatch_dtype(dt, [&](auto t, auto v) {
            using T = decltype(t);
            constexpr int V = decltype(v)::value;
            auto launch = [&](auto RELU, auto XM) {
                hipLaunchKernelGGL(
                    (bn_bwd_stats_kernel<T, V, RELU.value, XM.value>),
                    dim3(grid), dim3(256), shmem, s, (const T*)gout,
                    (const T*)x, (const T*)out, save_mean, save_invstd,
                    weight, bias, part, rows, C, c_base, cc);
            };
            // XMASK exists only with RELU
            if (!relu) launch(std::false_type{}, std::false_type{});
            else dispatch_flag(xmask, [&](auto XM) { launch(std::true_type{}, XM); });
        });
        bn_bwd_finalize_launch(part, grid, cc, c_base, ws, gw, gb, rows, C,
                               training, accum_g, s);
    }
}

void bn_bwd_finalize_launch(const float* part, int NB, int chunkC, int c_base,
                            float* ws, float* gw, float* gb, int64_t rows,
                            int C, bool training, bool accum_g, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_reduce_finalize_kernel, dim3(chunkC / FIN_CH),
                       dim3(256), 0, s, part, ws, gw, gb, NB, chunkC, c_base,
                       C, rows, training ? 1 : 0, accum_g ? 1 : 0);
}

// Pre-fold for conv-epilogue partials: mtiles can reach ~4700 for the
// layer-1 shapes, and the single finalize launch only runs C/64 blocks —
// one CU streaming ~2.4 MB serially (~15-20 us per BN measured as the
// bn_*_reduce_finalize rows). Fold to NB2 rows first at full-grid width.
// NB2 = 256 (bindings.cpp): a prefold thread then loads at most two rows
// of a ~4700-row set, both in flight together, and the finalize that
// follows reads four rows per thread in a single batch.
__global__ __launch_bounds__(256) void bn_partial_prefold_kernel(
    const float* __restrict__ part, float* __restrict__ out, int NB,
    int NB2, int chunkC) {
    __shared__ float sm[2 * 1024];
    const int lane = threadIdx.x & 15;
    const int sub = threadIdx.x >> 4;
    const int cc = (blockIdx.x * 16 + lane) * 4;
    const int g = blockIdx.y;
    float4 sv = {0, 0, 0, 0}, qv = {0, 0, 0, 0};
    #pragma unroll 2
    for (int b = g + sub * NB2; b < NB; b += 16 * NB2) {
        const float* p = part + (int64_t)b * 2 * chunkC;
        const float4 a = *(const float4*)(p + cc);
        const float4 z = *(const float4*)(p + chunkC + cc);
        sv.x += a.x; sv.y += a.y; sv.z += a.z; sv.w += a.w;
        qv.x += z.x; qv.y += z.y; qv.z += z.z; qv.w += z.w;
    }
    *(float4*)(sm + (sub * 16 + lane) * 4) = sv;
    *(float4*)(sm + 1024 + (sub * 16 + lane) * 4) = qv;
    __syncthreads();
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        if (sub < off) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                sm[(sub * 16 + lane) * 4 + k] +=
                    sm[((sub + off) * 16 + lane) * 4 + k];
                sm[1024 + (sub * 16 + lane) * 4 + k] +=
                    sm[1024 + ((sub + off) * 16 + lane) * 4 + k];
            }
        }
        __syncthreads();
    }
    if (sub == 0) {
        float* o = out + (int64_t)g * 2 * chunkC;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[cc + k] = sm[(lane * 4 + k)];
            o[chunkC + cc + k] = sm[1024 + lane * 4 + k];
        }
    }
}

void bn_partial_prefold_launch(const float* part, float* out, int NB,
                               int NB2, int chunkC, hipStream_t s) {
    dim3 grid((unsigned)(chunkC / 64), (unsigned)NB2);
    hipLaunchKernelGGL(bn_partial_prefold_kernel, grid, dim3(256), 0, s,
                       part, out, NB, NB2, chunkC);
}

void bn_bwd_apply_launch(const void* gout, const void* x, const void* out,
                         const float* save_mean, const float* save_invstd,
                         const float* weight, const float* ws, void* gx,
                         void* gres, int64_t rows, int C, bool relu, DT dt,
                         hipStream_t s, const float* bias) {
    // bias given (non-residual ReLU BN): mask from x, `out` unread
    const bool xmask = relu && bias != nullptr && gres == nullptr;
    const float* k1 = ws;
    const float* k2 = ws + C;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        const int64_t nvec = rows * C / V;
        auto launch = [&](auto RELU, auto XM) {
            hipLaunchKernelGGL(
                (bn_bwd_apply_kernel<T, V, RELU.value, XM.value>),
                dim3(grid_1d(nvec, 4096)), dim3(256), 0, s, (const T*)gout,
                (const T*)x, (const T*)out, save_mean, save_invstd, weight,
                bias, k1, k2, (T*)gx, (T*)gres, nvec, C);
        };
        // XMASK exists only with RELU
        if (!relu) launch(std::false_type{}, std::false_type{});
        else dispatch_flag(xmask, [&](auto XM) { launch(std::true_type{}, XM); });
    });
}

}  // namespace fda
