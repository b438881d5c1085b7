// Launcher API for the gfx950 kernels. bf16 tensors cross this boundary as
// raw unsigned short bit patterns (at::BFloat16 is bit-compatible).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

namespace fda {

enum class DT { F32 = 0, BF16 = 1 };

// Host-side dispatch for the launchers: calls f(T{}, V) with the storage
// type (bf16 bits / float) and its 16 B vector width as an integral
// constant; dispatch_flag does the same for a bool that selects a template
// flag. Inside the generic lambda:
//   using T = decltype(t); constexpr int V = decltype(v)::value;
template <typename F>
inline void dispatch_dtype(DT dt, F&& f) {
    if (dt == DT::BF16) f((unsigned short)0, std::integral_constant<int, 8>{});
    else f(0.f, std::integral_constant<int, 4>{});
}
template <typename F>
inline void dispatch_flag(bool flag, F&& f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// 1-D grid for n work items in blocks of 256: at least 1, at most cap
inline int grid_1d(int64_t n, int cap) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// fused logit cross-entropy: mean loss over N rows + dlogits in one pass
void ce_fwd_launch(const void* logits, const int64_t* target, float* loss,
                   void* dlogits, int N, int C, int ldl, DT dt,
                   hipStream_t s);

// out = relu(x + r)
void add_relu_fwd_launch(const void* x, const void* r, void* out, int64_t n,
                         DT dt, hipStream_t s);
// gx = gout * (out > 0)
void add_relu_bwd_launch(const void* gout, const void* out, void* gx, int64_t n,
                         DT dt, hipStream_t s);

// BatchNorm(+residual)(+ReLU), NHWC. ws is 2*C floats:
//   [0,C)  scale      [C,2C)  shift
// save_mean/save_invstd are separate C-float buffers.
int bn_stats_partial_floats(int C, int64_t rows, DT dt);
// training: stats partials + fused reduce/finalize (running-stat update,
// scale/shift into ws)
void bn_stats_launch(const void* x, float* ws, float* part,
                     const float* weight, const float* bias,
                     float* running_mean, float* running_var, float* save_mean,
                     float* save_invstd, int64_t rows, int C, float momentum,
                     float eps, DT dt, hipStream_t s);
// pre-fold big conv-epilogue partial sets to NB2 rows at full grid width
void bn_partial_prefold_launch(const float* part, float* out, int NB,
                               int NB2, int chunkC, hipStream_t s);
// fold part[NB][2][chunkC] (channels [c_base, c_base + chunkC) of C) and
// finalize: what bn_stats_launch runs per chunk, and the whole finalize for
// conv-epilogue partials (chunkC = C, c_base = 0)
void bn_fwd_finalize_launch(const float* part, int NB, int chunkC, int c_base,
                            const float* weight, const float* bias, float* rm,
                            float* rv, float* save_mean, float* save_invstd,
                            float* ws, int64_t rows, int C, float momentum,
                            float eps, hipStream_t s);

// eval: scale/shift from running stats
void bn_eval_finalize_launch(float* ws, const float* weight,
                             const float* bias, const float* running_mean,
                             const float* running_var, float* save_mean,
                             float* save_invstd, int C, float eps,
                             hipStream_t s);
void bn_apply_launch(const void* x, const void* residual, void* out,
                     const float* ws /*scale/shift*/, int64_t rows, int C,
                     bool relu, DT dt, hipStream_t s);
// eval fold of all BN layers of a model in one launch (device pointer
// tables): layer t writes scale[Cs[t]] then shift[Cs[t]] at arena + offs[t],
// bit-equal to bn_eval_finalize_launch's ws
void bn_fold_eval_batch_launch(const long* w_ptrs, const long* b_ptrs,
                               const long* rm_ptrs, const long* rv_ptrs,
                               const int* Cs, const long* offs,
                               const float* eps, float* arena, long arena_len,
                               int nlayers, int max_c, hipStream_t s);

// backward. ws is 2*C floats: [0,C) k1 = sum_g/m  [C,2C) k2 = sum_g_xhat/m
// (both 0 in eval mode).
// bwd: stats partials + fused reduce/finalize (gw, gb, k1/k2 into ws).
// With weight+bias (stats) / bias (apply) on a non-residual ReLU BN the
// ReLU mask is recomputed from x and `out` is never read.
void bn_bwd_stats_launch(const void* gout, const void* x, const void* out,
                         const float* save_mean, const float* save_invstd,
                         float* ws, float* part, float* gw, float* gb,
                         int64_t rows, int C, bool relu, bool training,
                         bool accum_g, DT dt, hipStream_t s,
                         const float* weight = nullptr,
                         const float* bias = nullptr);
void bn_bwd_apply_launch(const void* gout, const void* x, const void* out,
                         const float* save_mean, const float* save_invstd,
                         const float* weight, const float* ws, void* gx,
                         void* gres, int64_t rows, int C, bool relu, DT dt,
                         hipStream_t s, const float* bias = nullptr);
// fold part[NB][2][chunkC] backward partials: gw/gb (+= when accum), k1/k2
// into ws. Run per chunk by bn_bwd_stats_launch, and on the fused
// BN+ReLU+pool backward's partials (chunkC = C, c_base = 0).
void bn_bwd_finalize_launch(const float* part, int NB, int chunkC, int c_base,
                            float* ws, float* gw, float* gb, int64_t rows,
                            int C, bool training, bool accum_g, hipStream_t s);

// MaxPool2d NHWC with saved argmax byte per output element
void maxpool_fwd_launch(const void* x, void* out, uint8_t* idx, int N, int H,
                        int W, int C, int HO, int WO, int KH, int KW, int S,
                        int P, DT dt, hipStream_t s);
void maxpool_bwd_launch(const void* gout, const uint8_t* idx, void* gx, int N,
                        int H, int W, int C, int HO, int WO, int KH, int KW,
                        int S, int P, DT dt, hipStream_t s);

// Fused stem tail: BN + ReLU + max-pool (pool.hip). Needs 256 % (C/V) == 0
// (V = 8 bf16 / 4 fp32), KH*KW <= 255 and ceil(K/S) <= 2. fwd consumes the scale/shift the
// forward finalize left in ws and writes only the pooled tensor and its
// argmax bytes. bwd stats writes [bn_relu_maxpool_bwd_blocks][2][C]
// partials for bn_bwd_finalize_launch; bwd apply reads k1/k2 from ws.
void bn_relu_maxpool_fwd_launch(const void* x, const float* ws, void* out,
                                uint8_t* idx, int N, int H, int W, int C,
                                int HO, int WO, int KH, int KW, int S, int P,
                                DT dt, hipStream_t s);
int bn_relu_maxpool_bwd_blocks(int N, int H);
void bn_relu_maxpool_bwd_stats_launch(
    const void* gout, const uint8_t* idx, const void* x,
    const float* save_mean, const float* save_invstd, const float* weight,
    const float* bias, float* part, int N, int H, int W, int C, int HO,
    int WO, int KH, int KW, int S, int P, DT dt, hipStream_t s);
void bn_relu_maxpool_bwd_apply_launch(
    const void* gout, const uint8_t* idx, const void* x,
    const float* save_mean, const float* save_invstd, const float* weight,
    const float* bias, const float* ws, void* gx, int N, int H, int W, int C,
    int HO, int WO, int KH, int KW, int S, int P, DT dt, hipStream_t s);

// global average pool (NHWC): y[n][c] = mean_hw x; gx = gy/HW broadcast
void gap_fwd_launch(const void* x, void* y, int N, int HW, int C, DT dt,
                    hipStream_t s);
void gap_bwd_launch(const void* gy, void* gx, int N, int HW, int C, DT dt,
                    hipStream_t s);

// Implicit-GEMM conv, NHWC bf16 only (see conv_igemm.hip).
enum ConvMode { CONV_FWD = 0, CONV_DGRAD = 1, CONV_STEM = 2 };

// One conv's geometry, in the forward's terms for every mode: x [N,H,W,C],
// w [K][R][S][C], y [N,P,Q,K]. CONV_STEM: H, W are the padded image's, C = 8,
// S = 1 (taps iterate r only), no padding.
struct ConvGeom {
    int N, H, W, C, K, P, Q, R, S, sy, sx, py, px;
    // output channels
    int oc(ConvMode m) const { return m == CONV_DGRAD ? C : K; }
    // dgrad launches one z-class per (h % sy, w % sx) parity
    int classes(ConvMode m) const { return m == CONV_DGRAD ? sy * sx : 1; }
    // output rows M (dgrad: of the largest parity class)
    long rows(ConvMode m) const {
        return m == CONV_DGRAD
            ? (long)N * ((H + sy - 1) / sy) * ((W + sx - 1) / sx)
            : (long)N * P * Q;
    }
    // K-loop depth T in BK=64 steps (dgrad: over the whole filter, which is
    // what a stride-1 dgrad iterates)
    long depth(ConvMode m) const {
        return m == CONV_STEM ? R : (long)R * S * ((m == CONV_DGRAD ? K : C) / 64);
    }
};

// What a launch of that geometry runs: tile, split-K factor, BK32 3-buffer
// ring or BK64 2-buffer, grid size (all z-classes and split-K slices), and
// the row count of the BN stats partials [stats_rows][2][OC] a forward
// writes (m-tiles, or the combine kernel's blocks when sk > 1). The launcher
// obeys it and the bindings size skpart [sk][M][OC] and the partials from
// it, so workspace shapes always match what the kernels write.
struct ConvPlan {
    int bm, bn, sk;
    bool ring;
    long blocks;
    long stats_rows;
};
ConvPlan conv_igemm_plan(const ConvGeom& g, ConvMode mode);

// Inference epilogue: eval BN + residual + ReLU on the fp32 accumulator,
//   y = bf16(relu(fma(acc, scale[k], shift[k]) + residual[m][k]))
// rounded once. scale/shift: OC floats, 16-B aligned; residual: bf16 in the
// output's layout, 16-B aligned, or null.
struct EpiInfer {
    const float* scale;
    const float* shift;
    const unsigned short* residual;
    int relu;
};

// fwd:   src=x [N,H,W,C], wgt=w [K][R*S*C], out=y [N*P*Q][K]
// dgrad: src=dy [N,P,Q,K], wgt=wt [R*S*C][K] (pre-transposed), out=dx
// plan.sk > 1: skpart receives the fp32 partials and nothing else is
// written; conv_skcombine_launch then folds them into `out` and takes the
// stats / accsrc / epi arguments instead. accsrc: bf16 in the output's
// layout, added before the round. epi: forward only, and it excludes stats
// and accsrc (the inference kernels have neither), here and in the combine
// and stem launchers.
void conv_igemm_launch(const void* src, const void* wgt, void* out,
                       const ConvGeom& g, ConvMode mode, const ConvPlan& plan,
                       hipStream_t stream, float* stats = nullptr,
                       float* skpart = nullptr, const void* accsrc = nullptr,
                       const EpiInfer* epi = nullptr);

// split-K combine: y = bf16(sum over SK fp32 partials [SK][M][OC]), with
// optional BN stats partials [plan.stats_rows][2][OC], accsrc or inference
// epilogue. OC <= 2048.
void conv_skcombine_launch(const float* part, void* y, float* stats, long M,
                           int OC, int SK, hipStream_t stream,
                           const void* accsrc = nullptr,
                           const EpiInfer* epi = nullptr);

// stem conv (small C via channel-pad to 8, spatially pre-padded input):
// src [N,Hp,Wp,8], wgt wpad [K][R][64], out [N*P*Q][K]; g as CONV_STEM
void conv_stem_fwd_launch(const void* src, const void* wgt, void* out,
                          const ConvGeom& g, hipStream_t stream,
                          float* stats = nullptr,
                          const EpiInfer* epi = nullptr);
// dy [M][K]; x as above; ws [K][R*64] fp32 pre-zeroed
void conv_stem_wgrad_launch(const void* dy, const void* x, float* ws,
                            const ConvGeom& g, hipStream_t stream);

// XCD-aware block remap (bijective for any grid size): blocks that share
// `blockIdx % 8` share an L2, so give each such group a contiguous range
// of logical ids. A pure locality choice — any mapping is correct.
__host__ __device__ __forceinline__ unsigned xcd_contiguous_block(
    unsigned bid, unsigned nwg) {
    const unsigned q = nwg / 8, r = nwg % 8, xcd = bid % 8;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / 8;
}

// What a wgrad of M = N*P*Q pixels runs: FT fragments per wave axis (a
// (32*FT)k x (32*FT)c output tile per block), mch pixels per chunk (whole
// 64-pixel K-steps), nch chunks, and the 1-D grid of nwg =
// (K/tile)*(C/tile)*R*S*nch blocks. The launcher obeys it.
struct WgradPlan {
    int ft, mch, nch;
    long nwg;
};
WgradPlan conv_wgrad_plan(long M, int C, int K, int R, int S);

// Which (k-tile, c-tile, filter tap, pixel chunk) block `bid` of a wgrad
// grid owns. The logical id is XCD-contiguous and decoded chunk slowest,
//   L = ((chunk*RS + rs)*ctiles + ctile)*ktiles + ktile,
// so all blocks of a chunk, which stage the same dy tile and (for a 3x3
// filter) nearly the same x bytes, run back to back behind one L2. The stem
// is the case ctiles = 1, RS = R. One function for the kernel and for the
// binding that lets a test enumerate the grid.
struct WgradCoords {
    int ktile, ctile, rs, chunk;
};
__host__ __device__ __forceinline__ WgradCoords wgrad_block_coords(
    unsigned bid, int ktiles, int ctiles, int RS, int nch) {
    const unsigned nwg = (unsigned)(ktiles * ctiles * RS * nch);
    unsigned L = xcd_contiguous_block(bid, nwg);
    WgradCoords c;
    c.ktile = (int)(L % (unsigned)ktiles); L /= (unsigned)ktiles;
    c.ctile = (int)(L % (unsigned)ctiles); L /= (unsigned)ctiles;
    c.rs = (int)(L % (unsigned)RS);
    c.chunk = (int)(L / (unsigned)RS);
    return c;
}

// How the chunks of a wgrad meet. WG_ATOMIC: ws[K][RS*C] fp32 (pre-zeroed)
// += every chunk's tile, with atomicAdd. WG_SLAB: ws is [nch][K][RS*C] fp32
// and chunk c stores its tiles into slab c with plain stores, every element
// exactly once (no pre-zeroing); wgrad_slab_fold_launch sums the slabs.
constexpr int WG_ATOMIC = 0;
constexpr int WG_SLAB = 1;

// wgrad: dy^T @ im2col(x) into ws, by the plan of conv_wgrad_plan.
void conv_wgrad_launch(const void* dy, const void* x, float* ws,
                       const ConvGeom& g, hipStream_t stream,
                       int epi = WG_ATOMIC);

// Whether a body wgrad of that plan with n = K*R*S*C outputs takes the slab
// path where the caller has the choice (conv_igemm_wgrad, the train step).
bool conv_wgrad_use_slabs(const WgradPlan& p, long n);

// Ordered fold of wgrad slabs: s = slab[0] + slab[1] + ... + slab[nch-1],
// fp32 adds strictly in that order, so the sum is the same bits on every
// run. out_bf16: g = bf16(f32(g) + s), the direct-grad flush of
// grad_accum_bf16_launch; else out (fp32) = s. n % 4 == 0, 16-B aligned.
void wgrad_slab_fold_launch(const float* slab, int nch, long n, void* out,
                            bool out_bf16, hipStream_t s);

// batched conv-weight transpose: w[k][rc] -> wt[rc][k] for all tensors in
// one launch (device pointer arrays)
void wt_transpose_launch(const long* src_ptrs, long* dst_ptrs, const int* Ks,
                         const int* RCs, const int* tile_counts, int ntensors,
                         int max_tiles, hipStream_t stream);

// direct-grad flush: G_bf16 += cast(ws_f32), one conv-weight slice
void grad_accum_bf16_launch(void* g, const float* ws, long n, hipStream_t s);
// batched flush: all pending slices in one launch (device pointer arrays)
void grad_accum_batch_launch(const long* g_ptrs, const long* ws_ptrs,
                             const long* ns, int ntensors, long max_n,
                             hipStream_t s);

// FC-head padding helpers (Dense on the conv kernels, ops/linear.py)
void pad_rows_bf16_launch(void* dst, const void* src, long M, int C, int ldl,
                          hipStream_t s);
void bias_add_rows_bf16_launch(void* y, const void* bias, long M, int ldl,
                               hipStream_t s);
void colsum_accum_bf16_launch(void* g, const void* dy, long M, int ldl,
                              int Cvalid, hipStream_t s);

// Device-side image preprocessing (preprocess.hip): ragged uint8 HWC RGB
// images -> low-pass + bilinear resize + centre crop + normalize
// (+ per-image standardize) -> [N][crop][crop][3] fp32 / bf16.
//   arena: all images packed back to back, each at a 16-byte-aligned offset.
//   meta:  one row of PREPROCESS_META_INTS int32 words per image:
//     [0],[1] int64 byte offset into the arena (low word, high word)
//     [2] h   [3] w      source size
//     [4] nh  [5] nw     size after the resize (min(nh, nw) == resize)
//     [6] top [7] left   crop origin in the resized image
//     [8] r              Gaussian radius (0 = no blur)
//     [9] sigma          float bits (unused when r == 0)
//   A row that would read outside the arena, or with r >= min(h, w), yields
//   NaNs for that image instead of being trusted.
// resample writes the fp32 scratch [N][crop][crop][3] and per-tile
// sum / sum-of-squares partials [N][preprocess_tiles(crop)][2] (double);
// apply folds them per image (standardize) and writes the final dtype.
constexpr int PREPROCESS_META_INTS = 10;
int preprocess_tiles(int crop);
void preprocess_resample_launch(const uint8_t* arena, int64_t arena_bytes,
                                const int32_t* meta, float* scratch,
                                double* partials, int N, int crop,
                                bool normalize, hipStream_t s);
void preprocess_apply_launch(const float* scratch, const double* partials,
                             void* out, int N, int crop, bool standardize,
                             DT dt, hipStream_t s);

// flat fused optimizers. P: param dtype; M/V/S fp32; G param dtype.
void sgd_step_launch(void* P, const void* G, float* M, float* V, int64_t n,
                     float lr, float mom, float wd, bool nesterov,
                     bool has_master, DT dt, hipStream_t s);
void adam_step_launch(void* P, const void* G, float* M, float* V, float* S,
                      int64_t n, float lr, float b1, float b2, float eps,
                      float wd, float bc1, float bc2, bool has_master, DT dt,
                      hipStream_t s);

// LARS over the flat buffers (lars.hip). A segment is one parameter's slice;
// segments are numbered over all flat groups of an optimizer, S in total.
//   table:    this group's chunk table, nchunks rows of LARS_ROW_INTS int32
//             {segment id, start element in the group buffer, count of the
//             parameter's own elements}; count <= LARS_CHUNK, start % 64 == 0.
//   seg_meta: S rows of LARS_SEG_INTS int32 {first chunk, end chunk, flags}
//             over the concatenated tables; flag bit 0 = adapt, bit 1 = decay.
//   partials: {sum w^2, sum g^2} per chunk (double). norms writes this
//             group's nchunks rows; fold reads all total_chunks rows.
//   stats:    fp32 {gnorm, clip, W_0..W_S-1, G_0..G_S-1}; coef: fp32 [S].
//   lr:       one fp32 in device memory, read by the fold kernel.
// A table or seg_meta row the kernels cannot trust gives NaN sums, hence a
// non-finite gnorm, hence a step that writes nothing and bumps *skipped.
constexpr int LARS_CHUNK = 4096;
constexpr int LARS_ROW_INTS = 3;
constexpr int LARS_SEG_INTS = 3;
constexpr int LARS_STATS_HEAD = 2;
void lars_norms_launch(const void* P, const void* G, const float* M,
                       const int32_t* table, int nchunks, double* partials,
                       int64_t n, int S, bool has_master, DT dt,
                       hipStream_t s);
void lars_fold_launch(const double* partials, int total_chunks,
                      const int32_t* seg_meta, int S, const float* lr,
                      float eta, float wd, float eps, float max_grad_norm,
                      float* coef, float* stats, int* skipped, hipStream_t s);
void lars_step_launch(void* P, const void* G, float* M, float* V,
                      const int32_t* table, int nchunks,
                      const int32_t* seg_meta, const float* coef,
                      const float* stats, int64_t n, int S, float mom,
                      float wd, bool has_master, DT dt, hipStream_t s);

// Replica gradient mean (task-DDP flat sync): bufs is a HOST array of R
// device pointers (1 <= R <= GRAD_MEAN_MAX_R) to disjoint, 16 B-aligned flat
// buffers of n elements, n % V == 0. Each becomes
//   round(((b0 + b1) + ... + bR-1) / R),   fp32 sum, IEEE division, one round
// in place. nonfinite (device int, may be null) is OR-ed with 1 when any
// stored mean element is Inf/NaN.
constexpr int GRAD_MEAN_MAX_R = 16;
void grad_mean_multi_launch(void* const* bufs, int R, int64_t n,
                            int* nonfinite, DT dt, hipStream_t s);

}  // namespace fda
