// Device-side ImageNet preprocessing: uint8 HWC images of differing sizes ->
// Gaussian low-pass + bilinear resize (smallest side -> R) + centre crop +
// mean/std normalize (+ per-image standardize) -> NHWC fp32 / bf16.
//
// Blur and bilinear are both linear and separable, so one output sample is
//   v_c(o,p) = sum_y sum_x wy[o][y] * wx[p][x] * src[y][x][c] / 255
// with 1-D weights that are two Gaussians (the two bilinear taps t0, t0+1)
// blended by the bilinear fraction. Per axis that is 2r+2 taps at the
// "virtual" coordinates t0-r .. t0+r+1, reflected into the image the way
// F.pad(mode="reflect") does.
//
// preprocess_resample_kernel: one 256-thread block per (image, 32x32 output
//   tile). The tile's vertical footprint is walked in chunks of PP_CH virtual
//   rows: a horizontal pass filters each chunk row at the tile's 32 output
//   columns into an fp32 LDS strip, a vertical pass accumulates the strip
//   into the thread's output rows. LDS is fixed (24 KiB) for any image size
//   and any blur radius; the weights are evaluated in-kernel from sigma.
//   Lane = output column in both passes. Writes the tile to an fp32 scratch
//   [N][Cc][Cc][3] and the tile's sum / sum of squares (double) to
//   partials[N][tiles][2]: wave shuffle -> LDS -> global partials, no
//   atomics, so the result is bitwise reproducible.
// preprocess_apply_kernel: folds an image's partials in double (fixed
//   order), applies (v - mu) / (sd + 1e-5) (or only converts) and writes the
//   final output 16 B per lane; the elements before the first 16-B boundary
//   of an image and the ragged tail go out as scalars.
#include <algorithm>

#include "fda_common.h"
#include "fda_kernels.h"

namespace fda {

namespace {

constexpr int PP_TW = 32;        // output tile width  (lane = column)
constexpr int PP_TH = 32;        // output tile height
constexpr int PP_CH = 64;        // virtual source rows per LDS chunk
constexpr int PP_THREADS = 256;
constexpr int PP_RG = PP_THREADS / PP_TW;   // 8 row groups
constexpr int PP_HR = PP_CH / PP_RG;        // 8 chunk rows per thread
constexpr int PP_OR = PP_TH / PP_RG;        // 4 output rows per thread

// F.pad(mode="reflect") index; the clamp only matters for a zero-weight tap
__device__ __forceinline__ int pp_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// Bilinear source tap of resized coordinate X on an axis of n source and nn
// resized samples (align_corners=False), from integers: s = max(0,
// (X+0.5)*n/nn - 0.5), t0 = floor(s), lam = s - t0.
__device__ __forceinline__ void pp_tap(int X, int n, int nn, int& t0,
                                       float& lam) {
    long long num = (2LL * X + 1) * n - nn;
    if (num < 0) num = 0;
    const long long den = 2LL * nn;
    t0 = (int)(num / den);
    lam = (float)(num % den) / (float)den;
    if (t0 >= n - 1) lam = 0.f;   // second tap clamps onto the first
}

// Weight of virtual offset j in [-r, r+1] from t0:
//   (1-lam) * k[j] + lam * k[j-1],  k[i] = exp(-i^2 / 2 sigma^2) / sum(k)
__device__ __forceinline__ float pp_weight(int j, int r, float lam,
                                           float inv2s2, float invsum) {
    const float fj = (float)j, fi = (float)(j - 1);
    const float a = j <= r ? expf(-(fj * fj) * inv2s2) : 0.f;
    const float b = j > -r ? expf(-(fi * fi) * inv2s2) : 0.f;
    return ((1.f - lam) * a + lam * b) * invsum;
}

__device__ __forceinline__ double pp_wave_sum(double v) {
    #pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}

__global__ __launch_bounds__(PP_THREADS) void preprocess_resample_kernel(
    const uint8_t* __restrict__ arena, long long arena_bytes,
    const int* __restrict__ meta, float* __restrict__ scratch,
    double* __restrict__ partials, int Cc, int tiles_x, int tiles,
    int normalize) {
    __shared__ float strip[PP_CH * 3 * PP_TW];
    __shared__ double red[2 * (PP_THREADS / WAVE)];

    const int n = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int o0 = (tile / tiles_x) * PP_TH, p0 = (tile % tiles_x) * PP_TW;
    const int tx = threadIdx.x % PP_TW, tg = threadIdx.x / PP_TW;

    const int* m = meta + (long long)n * PREPROCESS_META_INTS;
    const long long off = (long long)(unsigned)m[0] | ((long long)m[1] << 32);
    const int h = m[2], w = m[3], nh = m[4], nw = m[5], top = m[6],
              left = m[7], r = m[8];
    const float sigma = __int_as_float(m[9]);

    const int p = p0 + tx;
    const bool pvalid = p < Cc;
    float* const simg = scratch + (long long)n * Cc * Cc * 3;

    // The meta table lives in device memory, out of the host checks' reach:
    // a row that would read outside the arena or the image yields NaNs.
    const bool ok = h > 0 && w > 0 && r >= 0 && r < min(h, w) && nh >= Cc &&
                    nw >= Cc && top >= 0 && left >= 0 && top <= nh - Cc &&
                    left <= nw - Cc && off >= 0 && (off & 15) == 0 &&
                    off <= arena_bytes &&
                    3LL * h * w <= arena_bytes - off &&
                    (r == 0 || sigma > 0.f);
    if (!ok) {   // block-uniform
        const float qnan = __int_as_float(0x7fc00000);
        #pragma unroll
        for (int k = 0; k < PP_OR; ++k) {
            const int o = o0 + tg + PP_RG * k;
            if (pvalid && o < Cc)
                for (int c = 0; c < 3; ++c)
                    simg[((long long)o * Cc + p) * 3 + c] = qnan;
        }
        if (threadIdx.x == 0) {
            partials[((long long)n * tiles + tile) * 2] = (double)qnan;
            partials[((long long)n * tiles + tile) * 2 + 1] = (double)qnan;
        }
        return;
    }

    const uint8_t* const src = arena + off;
    const float inv2s2 = r > 0 ? 1.f / (2.f * sigma * sigma) : 0.f;
    float ksum = 1.f;
    for (int i = 1; i <= r; ++i)
        ksum += 2.f * expf(-((float)i * (float)i) * inv2s2);
    const float invsum = 1.f / ksum;

    // this lane's column taps
    int x0;
    float lx;
    pp_tap(min(p, Cc - 1) + left, w, nw, x0, lx);

    // this thread's output rows and their taps
    int y0[PP_OR];
    float ly[PP_OR];
    #pragma unroll
    for (int k = 0; k < PP_OR; ++k)
        pp_tap(min(o0 + tg + PP_RG * k, Cc - 1) + top, h, nh, y0[k], ly[k]);

    // virtual-row footprint of the whole tile (block-uniform)
    int ya, yb;
    {
        float unused;
        pp_tap(o0 + top, h, nh, ya, unused);
        pp_tap(min(o0 + PP_TH, Cc) - 1 + top, h, nh, yb, unused);
        ya -= r;
        yb += r + 1;
    }

    float acc[PP_OR][3];
    #pragma unroll
    for (int k = 0; k < PP_OR; ++k)
        acc[k][0] = acc[k][1] = acc[k][2] = 0.f;

    for (int cb = ya; cb <= yb; cb += PP_CH) {
        const int rows = min(PP_CH, yb - cb + 1);

        // ---- horizontal pass: chunk rows tg, tg+8, ... at column p --------
        long long rowoff[PP_HR];
        float hacc[PP_HR][3];
        #pragma unroll
        for (int q = 0; q < PP_HR; ++q) {
            rowoff[q] = (long long)pp_reflect(cb + tg + PP_RG * q, h) * w * 3;
            hacc[q][0] = hacc[q][1] = hacc[q][2] = 0.f;
        }
        if (pvalid) {
            for (int j = -r; j <= r + 1; ++j) {
                const float wgt = pp_weight(j, r, lx, inv2s2, invsum);
                const int xo = pp_reflect(x0 + j, w) * 3;
                #pragma unroll
                for (int q = 0; q < PP_HR; ++q) {
                    if (tg + PP_RG * q < rows) {
                        const uint8_t* s = src + rowoff[q] + xo;
                        hacc[q][0] += wgt * (float)s[0];
                        hacc[q][1] += wgt * (float)s[1];
                        hacc[q][2] += wgt * (float)s[2];
                    }
                }
            }
        }
        #pragma unroll
        for (int q = 0; q < PP_HR; ++q) {
            const int row = tg + PP_RG * q;   // < PP_CH
            #pragma unroll
            for (int c = 0; c < 3; ++c)
                strip[(row * 3 + c) * PP_TW + tx] = hacc[q][c];
        }
        __syncthreads();

        // ---- vertical pass: the taps of each output row inside the chunk --
        #pragma unroll
        for (int k = 0; k < PP_OR; ++k) {
            if (pvalid && o0 + tg + PP_RG * k < Cc) {
                const int jlo = max(-r, cb - y0[k]);
                const int jhi = min(r + 1, cb + rows - 1 - y0[k]);
                for (int j = jlo; j <= jhi; ++j) {
                    const float wgt = pp_weight(j, r, ly[k], inv2s2, invsum);
                    const int row = y0[k] + j - cb;   // in [0, rows)
                    acc[k][0] += wgt * strip[(row * 3 + 0) * PP_TW + tx];
                    acc[k][1] += wgt * strip[(row * 3 + 1) * PP_TW + tx];
                    acc[k][2] += wgt * strip[(row * 3 + 2) * PP_TW + tx];
                }
            }
        }
        __syncthreads();
    }

    // ---- /255, normalize, scratch store, tile sum / sum of squares --------
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    float s1 = 0.f, s2 = 0.f;
    #pragma unroll
    for (int k = 0; k < PP_OR; ++k) {
        const int o = o0 + tg + PP_RG * k;
        if (pvalid && o < Cc) {
            #pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = acc[k][c] / 255.f;
                if (normalize) v = (v - mean[c]) / stdv[c];
                simg[((long long)o * Cc + p) * 3 + c] = v;
                s1 += v;
                s2 += v * v;
            }
        }
    }
    double d1 = pp_wave_sum((double)s1), d2 = pp_wave_sum((double)s2);
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    if (lane == 0) {
        red[2 * wid] = d1;
        red[2 * wid + 1] = d2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        d1 = d2 = 0.0;
        for (int i = 0; i < PP_THREADS / WAVE; ++i) {
            d1 += red[2 * i];
            d2 += red[2 * i + 1];
        }
        partials[((long long)n * tiles + tile) * 2] = d1;
        partials[((long long)n * tiles + tile) * 2 + 1] = d2;
    }
}

// T = float (V = 4) or unsigned short bf16 bits (V = 8): 16 B per store.
template <typename T, int V>
__global__ __launch_bounds__(PP_THREADS) void preprocess_apply_kernel(
    const float* __restrict__ scratch, const double* __restrict__ partials,
    T* __restrict__ out, long long L, int tiles, int standardize) {
    __shared__ double red[2 * (PP_THREADS / WAVE)];
    const int n = blockIdx.y;
    float mu = 0.f, den = 1.f;
    if (standardize) {
        const double* pp = partials + (long long)n * tiles * 2;
        double d1 = 0.0, d2 = 0.0;
        for (int t = threadIdx.x; t < tiles; t += PP_THREADS) {
            d1 += pp[2 * t];
            d2 += pp[2 * t + 1];
        }
        d1 = pp_wave_sum(d1);
        d2 = pp_wave_sum(d2);
        const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
        if (lane == 0) {
            red[2 * wid] = d1;
            red[2 * wid + 1] = d2;
        }
        __syncthreads();
        d1 = d2 = 0.0;   // every thread folds the same four pairs, in order
        for (int i = 0; i < PP_THREADS / WAVE; ++i) {
            d1 += red[2 * i];
            d2 += red[2 * i + 1];
        }
        const double mean = d1 / (double)L;
        // unbiased (n-1) estimator, as Tensor.std()
        const double var = fmax(d2 - d1 * mean, 0.0) / (double)(L - 1);
        mu = (float)mean;
        den = (float)sqrt(var) + 1e-5f;
    }

    const long long e0 = (long long)n * L;
    const float* sp = scratch + e0;
    T* op = out + e0;
    const long long head = min(L, (long long)((V - e0 % V) % V));
    const long long nvec = (L - head) / V;
    const long long tail = head + nvec * V;

    for (long long vi = (long long)blockIdx.x * PP_THREADS + threadIdx.x;
         vi < nvec; vi += (long long)gridDim.x * PP_THREADS) {
        const long long e = head + vi * V;   // (e0 + e) % V == 0
        float f[V];
        #pragma unroll
        for (int q = 0; q < V / 4; ++q)
            *(float4*)(f + 4 * q) = *(const float4*)(sp + e + 4 * q);
        T ov[V];
        #pragma unroll
        for (int q = 0; q < V; ++q)
            store_f32(ov + q, standardize ? (f[q] - mu) / den : f[q]);
        *(uint4*)(op + e) = *(const uint4*)ov;
    }
    if (blockIdx.x == 0) {
        // fewer than V elements on either side of the vector body
        long long e = -1;
        if (threadIdx.x < head) e = threadIdx.x;
        else if (threadIdx.x - head < L - tail) e = tail + (threadIdx.x - head);
        if (e >= 0) {
            const float v = sp[e];
            store_f32(op + e, standardize ? (v - mu) / den : v);
        }
    }
}

}  // namespace

int preprocess_tiles(int crop) {
    const int tx = (crop + PP_TW - 1) / PP_TW, ty = (crop + PP_TH - 1) / PP_TH;
    return tx * ty;
}

void preprocess_resample_launch(const uint8_t* arena, int64_t arena_bytes,
                                const int32_t* meta, float* scratch,
                                double* partials, int N, int crop,
                                bool normalize, hipStream_t s) {
    const int tiles = preprocess_tiles(crop);
    hipLaunchKernelGGL(preprocess_resample_kernel,
                       dim3((unsigned)((int64_t)N * tiles)), dim3(PP_THREADS),
                       0, s, arena, (long long)arena_bytes, meta, scratch,
                       partials, crop, (crop + PP_TW - 1) / PP_TW, tiles,
                       normalize ? 1 : 0);
}

void preprocess_apply_launch(const float* scratch, const double* partials,
                             void* out, int N, int crop, bool standardize,
                             DT dt, hipStream_t s) {
    const long long L = 3LL * crop * crop;
    const int tiles = preprocess_tiles(crop);
    const int V = dt == DT::BF16 ? 8 : 4;
    const long long nvec = L / V;
    const unsigned gx = (unsigned)std::min<long long>(
        32, std::max<long long>(1, (nvec + PP_THREADS - 1) / PP_THREADS));
    if (dt == DT::BF16)
        hipLaunchKernelGGL((preprocess_apply_kernel<unsigned short, 8>),
                           dim3(gx, (unsigned)N), dim3(PP_THREADS), 0, s,
                           scratch, partials, (unsigned short*)out, L, tiles,
                           standardize ? 1 : 0);
    else
        hipLaunchKernelGGL((preprocess_apply_kernel<float, 4>),
                           dim3(gx, (unsigned)N), dim3(PP_THREADS), 0, s,
                           scratch, partials, (float*)out, L, tiles,
                           standardize ? 1 : 0);
}

}  // namespace fda
