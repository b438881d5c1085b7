// MaxPool2d NHWC fwd (+argmax) / bwd (gather over candidate windows).
// Reference site: ResNet stem 3x3 stride-2 pool (SURVEY.md §2.4 — "hand
// kernel + index mask"). Generic in kernel/stride/pad; ResNet uses 3x3 s2 p1.
//
// fwd: one thread computes V consecutive channels of one output pixel,
//      storing the window-position argmax (0..KH*KW-1) as one byte/channel.
// bwd: one thread computes V channels of one INPUT pixel by gathering the
//      <= ceil(K/S)^2 output windows that cover it — no atomics.
#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

template <typename T, int V>
__global__ void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ out,
                                   uint8_t* __restrict__ idx, int N, int H,
                                   int W, int C, int HO, int WO, int KH, int KW,
                                   int S, int P) {
    const int64_t total = (int64_t)N * HO * WO * (C / V);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int cv = (int)(i % (C / V));
        int64_t t = i / (C / V);
        const int wo = (int)(t % WO);
        t /= WO;
        const int ho = (int)(t % HO);
        const int n = (int)(t / HO);
        const int c0 = cv * V;

        float best[V];
        uint8_t barg[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            best[k] = -INFINITY;
            barg[k] = 0;
        }
        const int h0 = ho * S - P, w0 = wo * S - P;
        for (int kh = 0; kh < KH; ++kh) {
            const int hi = h0 + kh;
            if (hi < 0 || hi >= H) continue;
            for (int kw = 0; kw < KW; ++kw) {
                const int wi = w0 + kw;
                if (wi < 0 || wi >= W) continue;
                T xv[V];
                *(uint4*)xv = *(const uint4*)(
                    x + (((int64_t)n * H + hi) * W + wi) * C + c0);
                const uint8_t p = (uint8_t)(kh * KW + kw);
                #pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float v = load_f32(xv + k);
                    if (v > best[k]) {
                        best[k] = v;
                        barg[k] = p;
                    }
                }
            }
        }
        T ov[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) store_f32(ov + k, best[k]);
        const int64_t o = (((int64_t)n * HO + ho) * WO + wo) * C + c0;
        *(uint4*)(out + o) = *(uint4*)ov;
        #pragma unroll
        for (int k = 0; k < V; ++k) idx[o + k] = barg[k];
    }
}

// One block per (n, hi) input row: the ho window range is block-uniform
// (scalar branches, hoisted row base addresses) and the per-thread index
// math is shifts/adds only — the flat-index version spent its time on two
// integer divisions per element and per-thread window-bound branches
// (116 us/step vs ~30 us of actual traffic at the ResNet stem shape).
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(
    const T* __restrict__ gout, const uint8_t* __restrict__ idx,
    T* __restrict__ gx, int N, int H, int W,
    int C, int HO, int WO, int KH, int KW, int S, int P) {
    const int CV = C / V;
    const int hi = blockIdx.x % H;
    const int n = blockIdx.x / H;
    if (n >= N) return;

    const int ho_lo = max(0, (hi + P - KH + S) / S);
    const int ho_hi = min(HO - 1, (hi + P) / S);
    const T* grow = gout + ((int64_t)n * HO) * WO * C;
    const uint8_t* irow = idx + ((int64_t)n * HO) * WO * C;
    T* xrow = gx + (((int64_t)n * H + hi) * W) * C;

    // threads cover (wi, cv); W*CV per row, looped by the whole block
    for (int t = threadIdx.x; t < W * CV; t += blockDim.x) {
        const int cv = t % CV;        // CV is 8/16/32/64: strength-reduced
        const int wi = t / CV;
        const int c0 = cv * V;

        float acc[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.f;

        const int wo_lo = max(0, (wi + P - KW + S) / S);
        const int wo_hi = min(WO - 1, (wi + P) / S);
        for (int ho = ho_lo; ho <= ho_hi; ++ho) {
            const int kh = hi - (ho * S - P);
            if (kh < 0 || kh >= KH) continue;
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                const int kw = wi - (wo * S - P);
                if (kw < 0 || kw >= KW) continue;
                const uint8_t p = (uint8_t)(kh * KW + kw);
                const int64_t o = ((int64_t)ho * WO + wo) * C + c0;
                T gv[V];
                *(uint4*)gv = *(const uint4*)(grow + o);
                // V idx bytes in one word (per-byte loads were issue-bound)
                uint64_t ib;
                if constexpr (V == 8)
                    ib = *(const uint64_t*)(irow + o);
                else
                    ib = *(const uint32_t*)(irow + o);
                #pragma unroll
                for (int k = 0; k < V; ++k)
                    if (((ib >> (8 * k)) & 0xffu) == p)
                        acc[k] += load_f32(gv + k);
            }
        }
        T rv[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) store_f32(rv + k, acc[k]);
        *(uint4*)(xrow + (int64_t)wi * C + c0) = *(uint4*)rv;
    }
}

void maxpool_fwd_launch(const void* x, void* out, uint8_t* idx, int N, int H,
                        int W, int C, int HO, int WO, int KH, int KW, int S,
                        int P, DT dt, hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((maxpool_fwd_kernel<T, V>),
                           dim3(grid_1d((int64_t)N * HO * WO * C / V, 4096)),
                           dim3(256), 0, s, (const T*)x, (T*)out, idx, N, H, W,
                           C, HO, WO, KH, KW, S, P);
    });
}

void maxpool_bwd_launch(const void* gout, const uint8_t* idx, void* gx, int N,
                        int H, int W, int C, int HO, int WO, int KH, int KW,
                        int S, int P, DT dt, hipStream_t s) {
    const unsigned rows = (unsigned)((int64_t)N * H);
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((maxpool_bwd_kernel<T, V>), dim3(rows), dim3(256),
                           0, s, (const T*)gout, idx, (T*)gx, N, H, W, C, HO,
                           WO, KH, KW, S, P);
    });
}

// ---- fused stem tail: BN + ReLU + max-pool --------------------------------
// The stem activation (N x 112 x 112 x 64) is the largest tensor of the
// network and its passes run at HBM speed. Unfused, the post-ReLU tensor
// and the full-resolution pool gradient exist only to be read back by the
// next kernel. Fused: the forward reads x once and writes only the pooled
// tensor + argmax bytes; the backward gathers the pooled gradient through
// the argmax bytes and recomputes the ReLU mask from x, which it reads
// anyway for xhat.
//
// Numerics are those of the unfused chain: the activation is rounded
// through the storage dtype as bn_apply stores it (fda_common.h),
// the max follows maxpool_fwd_kernel's rule (strict >, kh-then-kw scan,
// first maximum wins), and the gathered gradient is rounded through the
// storage dtype where maxpool_bwd_kernel stored it.
//
// All three kernels give a thread V fixed channels (256 % (C/V) == 0, checked
// by the binding), so per-channel constants load once per thread.

// fwd: one block per (n, ho) output row, threads over (wo, cv). KS > 0 is
// a compile-time square window (KH == KW == KS): the window loop unrolls and
// — because out-of-image taps load a clamped, in-image address and are
// masked in the compare instead of skipped — all KS*KS loads are in flight
// before the first use. With skip branches each tap waited out its own
// memory latency in turn (75 us vs 34 us of traffic at the stem shape).
// KS == 0 takes KH/KW at run time.
template <typename T, int V, int KS>
__global__ __launch_bounds__(256) void bn_relu_maxpool_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, T* __restrict__ out,
    uint8_t* __restrict__ idx, int N, int H, int W, int C, int HO, int WO,
    int KH, int KW, int S, int P) {
    const int CV = C / V;
    // neighbouring output rows share input rows: keep them on one L2
    const int row = (int)xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int ho = row % HO;
    const int n = row / HO;
    if (n >= N) return;
    const int c0 = (threadIdx.x % CV) * V;
    float sc[V], sh[V];
    #pragma unroll
    for (int k = 0; k < V; ++k) {
        sc[k] = scale[c0 + k];
        sh[k] = shift[c0 + k];
    }
    const int h0 = ho * S - P;
    const T* ximg = x + (int64_t)n * H * W * C;
    const int64_t orow = ((int64_t)n * HO + ho) * WO * C;

    for (int t = threadIdx.x; t < WO * CV; t += blockDim.x) {
        const int wo = t / CV;       // CV is a power of two: a shift
        const int w0 = wo * S - P;
        float best[V];
        unsigned barg[V];
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            best[k] = -INFINITY;
            barg[k] = 0;
        }
        // address of tap (kh, kw), clamped into the image; `ok` masks it
        auto tap_ptr = [&](int kh, int kw, bool& ok) {
            const int hi = h0 + kh, wi = w0 + kw;
            ok = hi >= 0 && hi < H && wi >= 0 && wi < W;
            return (const uint4*)(ximg + ((int64_t)min(max(hi, 0), H - 1) * W +
                                          min(max(wi, 0), W - 1)) * C + c0);
        };
        // branch-free update: strict >, scan order, first maximum wins
        auto tap_max = [&](const uint4& raw, bool ok, unsigned p) {
            float f[V];
            unpack_f32<T, V>(raw, f);
            #pragma unroll
            for (int k = 0; k < V; ++k)
                f[k] = fmaxf(bn_affine(f[k], sc[k], sh[k]), 0.f);
            round_storage<T, V>(f);   // the value bn_apply would have stored
            #pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool take = ok & (f[k] > best[k]);
                best[k] = take ? f[k] : best[k];
                barg[k] = take ? p : barg[k];
            }
        };
        if constexpr (KS > 0) {
            uint4 raw[KS * KS];
            bool ok[KS * KS];
            #pragma unroll
            for (int j = 0; j < KS * KS; ++j)
                raw[j] = *tap_ptr(j / KS, j % KS, ok[j]);
            #pragma unroll
            for (int j = 0; j < KS * KS; ++j) tap_max(raw[j], ok[j], j);
        } else {
            for (int kh = 0; kh < KH; ++kh)
                for (int kw = 0; kw < KW; ++kw) {
                    bool ok;
                    const uint4 raw = *tap_ptr(kh, kw, ok);
                    tap_max(raw, ok, (unsigned)(kh * KW + kw));
                }
        }
        T ov[V];
        uint64_t ib = 0;
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            store_f32(ov + k, best[k]);
            ib |= (uint64_t)barg[k] << (8 * k);
        }
        const int64_t o = orow + (int64_t)wo * C + c0;
        *(uint4*)(out + o) = *(uint4*)ov;
        if constexpr (V == 8)
            *(uint64_t*)(idx + o) = ib;
        else
            *(uint32_t*)(idx + o) = (uint32_t)ib;
    }
}

// The gather of maxpool_bwd_kernel for V channels of input pixel (hi, wi):
// sums the pooled gradients of the windows whose argmax byte names the
// pixel, rounded through the storage dtype as that kernel stores it.
// At most 2 x 2 windows cover a pixel (ceil(K/S) <= 2, checked by the
// binding). All four are loaded — from a clamped, in-range address — and a
// window that does not cover the pixel gets the impossible argmax code 256
// instead of a skip branch, so the loads are in flight together; with skip
// branches every window waited out its own memory latency in turn, which is
// what bounds maxpool_bwd_kernel (104 us vs 34 us of traffic at the stem
// shape). Accumulation order (ho, then wo) is that kernel's.
struct PoolRowWin {   // the <= 2 pooled rows covering input row hi
    int ho[2];        // clamped row index
    int pbase[2];     // kh * KW, or 256 when the row does not cover hi
};

__device__ __forceinline__ PoolRowWin pool_row_windows(int hi, int HO, int KH,
                                                       int KW, int S, int P) {
    PoolRowWin r;
    const int ho_lo = max(0, (hi + P - KH + S) / S);
    const int ho_hi = min(HO - 1, (hi + P) / S);
    #pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int ho = ho_lo + a;
        const int kh = hi - (ho * S - P);
        const bool ok = ho <= ho_hi && kh >= 0 && kh < KH;
        r.ho[a] = min(ho, HO - 1);
        r.pbase[a] = ok ? kh * KW : 256;
    }
    return r;
}

// grow/irow point at image n of the pooled gradient / argmax bytes.
template <typename T, int V>
__device__ __forceinline__ void pool_gather(
    const T* __restrict__ grow, const uint8_t* __restrict__ irow,
    const PoolRowWin& rw, int wi, int c0, int C, int WO, int KW, int S, int P,
    float (&acc)[V]) {
    const int wo_lo = max(0, (wi + P - KW + S) / S);
    const int wo_hi = min(WO - 1, (wi + P) / S);
    uint4 gv[4];
    uint64_t ib[4];
    unsigned code[4];
    #pragma unroll
    for (int a = 0; a < 2; ++a) {
        #pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int wo = wo_lo + b;
            const int kw = wi - (wo * S - P);
            const bool ok = wo <= wo_hi && kw >= 0 && kw < KW;
            // pbase 256 keeps the sum >= 256: never equal to a byte
            code[a * 2 + b] = ok ? (unsigned)(rw.pbase[a] + kw) : 256u;
            const int64_t o =
                ((int64_t)rw.ho[a] * WO + min(wo, WO - 1)) * C + c0;
            gv[a * 2 + b] = *(const uint4*)(grow + o);
            if constexpr (V == 8)
                ib[a * 2 + b] = *(const uint64_t*)(irow + o);
            else
                ib[a * 2 + b] = *(const uint32_t*)(irow + o);
        }
    }
    #pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        float g[V];
        unpack_f32<T, V>(gv[j], g);
        // branch-free: a non-matching window adds an exact 0
        #pragma unroll
        for (int k = 0; k < V; ++k)
            acc[k] += (unsigned)((ib[j] >> (8 * k)) & 0xffu) == code[j]
                          ? g[k] : 0.f;
    }
    round_storage<T, V>(acc);
}

// bwd stats: sum_g and sum_g*xhat of the masked, gathered gradient into
// part[block][2][C] — the layout bn_bwd_reduce_finalize_kernel folds. Each
// block walks a contiguous range of (n, hi) input rows, so the pooled rows
// it gathers from are fetched once.
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_relu_maxpool_bwd_stats_kernel(
    const T* __restrict__ gout, const uint8_t* __restrict__ idx,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ part, int N, int H,
    int W, int C, int HO, int WO, int KH, int KW, int S, int P,
    int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 256*V
    const int CV = C / V;
    const int rpb = blockDim.x / CV;
    const int lane_c = threadIdx.x % CV;
    const int sub_r = threadIdx.x / CV;
    const int c0 = lane_c * V;

    float mu[V], is[V], sc[V], sh[V];
    ChanAcc<V> sg, sgx;
    #pragma unroll
    for (int k = 0; k < V; ++k) {
        mu[k] = mean[c0 + k];
        is[k] = invstd[c0 + k];
        sc[k] = bn_scale_of(weight[c0 + k], is[k]);
        sh[k] = bn_shift_of(bias[c0 + k], mu[k], sc[k]);
        sg.v[k] = sgx.v[k] = 0.f;
    }
    const int NR = N * H;
    const int r_begin = blockIdx.x * rows_per_block;
    const int r_end = min(NR, r_begin + rows_per_block);
    for (int row = r_begin; row < r_end; ++row) {
        const int hi = row % H;
        const int n = row / H;
        const PoolRowWin rw = pool_row_windows(hi, HO, KH, KW, S, P);
        const T* grow = gout + (int64_t)n * HO * WO * C;
        const uint8_t* irow = idx + (int64_t)n * HO * WO * C;
        const T* xrow = x + (int64_t)row * W * C;
        #pragma unroll 2
        for (int wi = sub_r; wi < W; wi += rpb) {
            const uint4 xraw = *(const uint4*)(xrow + (int64_t)wi * C + c0);
            float g[V], xf8[V];
            pool_gather<T, V>(grow, irow, rw, wi, c0, C, WO, KW, S, P, g);
            unpack_f32<T, V>(xraw, xf8);
            #pragma unroll
            for (int k = 0; k < V; ++k) {
                const float xf = xf8[k];
                const float gm =
                    bn_relu_positive<T>(xf, sc[k], sh[k]) ? g[k] : 0.f;
                const float xhat = (xf - mu[k]) * is[k];
                sg.v[k] += gm;
                sgx.v[k] += gm * xhat;
            }
        }
    }
    block_fold_rows<V>(sg, sgx, smem, part + (int64_t)blockIdx.x * 2 * C, CV,
                       C);
}

// bwd apply: one block per (n, hi) input row; writes gx for the stem wgrad.
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_relu_maxpool_bwd_apply_kernel(
    const T* __restrict__ gout, const uint8_t* __restrict__ idx,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ weight,
    const float* __restrict__ bias, const float* __restrict__ k1,
    const float* __restrict__ k2, T* __restrict__ gx, int N, int H, int W,
    int C, int HO, int WO, int KH, int KW, int S, int P) {
    const int CV = C / V;
    const int row = (int)xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int hi = row % H;
    const int n = row / H;
    if (n >= N) return;
    const int c0 = (threadIdx.x % CV) * V;

    float mu[V], is[V], sc[V], sh[V], wk[V], a1[V], a2[V];
    #pragma unroll
    for (int k = 0; k < V; ++k) {
        mu[k] = mean[c0 + k];
        is[k] = invstd[c0 + k];
        wk[k] = weight[c0 + k];
        sc[k] = bn_scale_of(wk[k], is[k]);
        sh[k] = bn_shift_of(bias[c0 + k], mu[k], sc[k]);
        a1[k] = k1[c0 + k];
        a2[k] = k2[c0 + k];
    }
    const PoolRowWin rw = pool_row_windows(hi, HO, KH, KW, S, P);
    const T* grow = gout + (int64_t)n * HO * WO * C;
    const uint8_t* irow = idx + (int64_t)n * HO * WO * C;
    const T* xrow = x + (int64_t)row * W * C;
    T* gxrow = gx + (int64_t)row * W * C;

    #pragma unroll 2
    for (int t = threadIdx.x; t < W * CV; t += blockDim.x) {
        const int wi = t / CV;
        T rv[V];
        const uint4 xraw = *(const uint4*)(xrow + (int64_t)wi * C + c0);
        float g[V], xf8[V];
        pool_gather<T, V>(grow, irow, rw, wi, c0, C, WO, KW, S, P, g);
        unpack_f32<T, V>(xraw, xf8);
        #pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xf = xf8[k];
            const float gm =
                bn_relu_positive<T>(xf, sc[k], sh[k]) ? g[k] : 0.f;
            const float xhat = (xf - mu[k]) * is[k];
            store_f32(rv + k,
                      bn_bwd_dx(gm, xhat, a1[k], a2[k], wk[k], is[k]));
        }
        *(uint4*)(gxrow + (int64_t)wi * C + c0) = *(uint4*)rv;
    }
}

void bn_relu_maxpool_fwd_launch(const void* x, const float* ws, void* out,
                                uint8_t* idx, int N, int H, int W, int C,
                                int HO, int WO, int KH, int KW, int S, int P,
                                DT dt, hipStream_t s) {
    const float* scale = ws;
    const float* shift = ws + C;
    const unsigned rows = (unsigned)((int64_t)N * HO);
    const int ks = KH == KW && (KH == 3 || KH == 2) ? KH : 0;
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        auto launch = [&](auto KS) {
            hipLaunchKernelGGL((bn_relu_maxpool_fwd_kernel<T, V, KS.value>),
                               dim3(rows), dim3(256), 0, s, (const T*)x, scale,
                               shift, (T*)out, idx, N, H, W, C, HO, WO, KH, KW,
                               S, P);
        };
        if (ks == 3) launch(std::integral_constant<int, 3>{});
        else if (ks == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 0>{});
    });
}

// Grid of the fused bwd stats pass == rows of its partial buffer. Capped at
// 1024 blocks (4 per CU): each row costs a block a dependent gather, so it
// wants more waves in flight than the streaming stats pass's 512; the
// finalize folds 1024 rows in two batches. Measured against a 512 cap at the
// stem shape: stats kernel 107 vs 120 us, finalize 5.1 vs 5.3 us
// (profiles/step_profile_r3.md).
static inline void pool_stats_geom(int64_t NR, int& grid, int& rows_per_block) {
    const int64_t cap = 1024;
    rows_per_block = (int)((NR + cap - 1) / cap);
    if (rows_per_block < 1) rows_per_block = 1;
    grid = (int)((NR + rows_per_block - 1) / rows_per_block);
    if (grid < 1) grid = 1;
}

int bn_relu_maxpool_bwd_blocks(int N, int H) {
    int grid, rpb;
    pool_stats_geom((int64_t)N * H, grid, rpb);
    return grid;
}

void bn_relu_maxpool_bwd_stats_launch(
    const void* gout, const uint8_t* idx, const void* x,
    const float* save_mean, const float* save_invstd, const float* weight,
    const float* bias, float* part, int N, int H, int W, int C, int HO,
    int WO, int KH, int KW, int S, int P, DT dt, hipStream_t s) {
    int grid, rpb;
    pool_stats_geom((int64_t)N * H, grid, rpb);
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((bn_relu_maxpool_bwd_stats_kernel<T, V>),
                           dim3(grid), dim3(256), 256 * V * sizeof(float), s,
                           (const T*)gout, idx, (const T*)x, save_mean,
                           save_invstd, weight, bias, part, N, H, W, C, HO, WO,
                           KH, KW, S, P, rpb);
    });
}

void bn_relu_maxpool_bwd_apply_launch(
    const void* gout, const uint8_t* idx, const void* x,
    const float* save_mean, const float* save_invstd, const float* weight,
    const float* bias, const float* ws, void* gx, int N, int H, int W, int C,
    int HO, int WO, int KH, int KW, int S, int P, DT dt, hipStream_t s) {
    const float* k1 = ws;
    const float* k2 = ws + C;
    const unsigned rows = (unsigned)((int64_t)N * H);
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((bn_relu_maxpool_bwd_apply_kernel<T, V>),
                           dim3(rows), dim3(256), 0, s, (const T*)gout, idx,
                           (const T*)x, save_mean, save_invstd, weight, bias,
                           k1, k2, (T*)gx, N, H, W, C, HO, WO, KH, KW, S, P);
    });
}

// ---- global average pool (AdaptiveMeanPool 1x1), NHWC -------------------
// "AdaptiveMeanPool / global avg pool fwd/bwd — warp
// reduction". fwd: y[n][c] = mean_hw x[n][h][w][c]; bwd: gx = gy/HW bcast.
template <typename T, int V>
__global__ __launch_bounds__(256) void gap_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, int N, int HW, int C) {
    // one thread per (n, c-vec): strided column reduction, fp32 accum
    const long nv = (long)N * (C / V);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / (C / V));
        const int c0 = (int)(i % (C / V)) * V;
        const T* base = x + ((long)n * HW) * C + c0;
        float acc[V];
        #pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (int r = 0; r < HW; ++r) {
            T v[V];
            *(uint4*)v = *(const uint4*)(base + (long)r * C);
            #pragma unroll
            for (int e = 0; e < V; ++e) acc[e] += load_f32(v + e);
        }
        T o[V];
        const float inv = 1.f / (float)HW;
        #pragma unroll
        for (int e = 0; e < V; ++e) store_f32(o + e, acc[e] * inv);
        *(uint4*)(y + (long)n * C + c0) = *(uint4*)o;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void gap_bwd_kernel(
    const T* __restrict__ gy, T* __restrict__ gx, int N, int HW, int C) {
    const long nv = (long)N * HW * (C / V);
    const float inv = 1.f / (float)HW;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (long)gridDim.x * blockDim.x) {
        const long row = i / (C / V);          // (n, hw)
        const int n = (int)(row / HW);
        const int c0 = (int)(i % (C / V)) * V;
        T g[V];
        *(uint4*)g = *(const uint4*)(gy + (long)n * C + c0);
        T o[V];
        #pragma unroll
        for (int e = 0; e < V; ++e) store_f32(o + e, load_f32(g + e) * inv);
        *(uint4*)(gx + row * C + c0) = *(uint4*)o;
    }
}

void gap_fwd_launch(const void* x, void* y, int N, int HW, int C, DT dt,
                    hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((gap_fwd_kernel<T, V>),
                           dim3(grid_1d((int64_t)N * (C / V), 1024)),
                           dim3(256), 0, s, (const T*)x, (T*)y, N, HW, C);
    });
}

void gap_bwd_launch(const void* gy, void* gx, int N, int HW, int C, DT dt,
                    hipStream_t s) {
    dispatch_dtype(dt, [&](auto t, auto v) {
        using T = decltype(t);
        constexpr int V = decltype(v)::value;
        hipLaunchKernelGGL((gap_bwd_kernel<T, V>),
                           dim3(grid_1d((int64_t)N * HW * (C / V), 4096)),
                           dim3(256), 0, s, (const T*)gy, (T*)gx, N, HW, C);
    });
}

}  // namespace fda
