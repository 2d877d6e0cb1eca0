// train.hip -- training-mode (batch-statistics) BatchNorm + ReLU + max over the neighbourhood,
// forward and backward, for the SA layers' shared MLP.
//
// Reference: PointNetSetAbstraction.forward in train mode, /root/reference/model/
// pointnet2_utils.py:167-172 (Conv2d 1x1 -> BatchNorm2d -> ReLU per layer, torch.max over the
// K neighbours), the same for the MSG scales (:211-221); the loop train_rotation.py:99-133 runs
// it under autograd.  BatchNorm2d in training normalises with the batch statistics over all
// B*S*K rows (biased variance), updates running_mean / running_var (unbiased) with momentum, and
// its backward couples every row of the batch through the two column sums below.
//
// The matmuls (Y = X W^T + b, dW = dY^T X, dX = dY W) are plain GEMMs and go to the library
// (hipBLASLt via torch.mm, pn2/train.py); what is here is everything around them, fused so each
// pass reads the [M, C] activations once:
//   pn2_bn_train_stats_f32    column sum / sum of squares of Y (float64 partials per row chunk),
//                             then mean, invstd, running-stat update
//   pn2_bn_relu_apply_f32     A = relu((Y - mean) * invstd * gamma + beta)  (no ReLU with
//                             PN2_LAYER_NO_RELU: PointNet-v1's conv3 + bn3 before its max)
//   pn2_group_max_f32         out[g][c] = max_k A[g*K + k][c] and its first argmax
//   pn2_bn_relu_backward_f32  dXn = dA * [A > 0] (unmasked with PN2_LAYER_NO_RELU; dA from the
//                             next layer, or scattered from the max: arg[g][c] == k ?
//                             dOut[g][c] : 0), its column sums
//                             S1 = sum dXn and S2 = sum dXn * xhat (= dbeta, dgamma; float64
//                             sums, xhat in float64 inside S2), then
//                             dY = gamma * invstd * (dXn - S1/M - xhat * S2/M); with
//                             PN2_LAYER_FROZEN_STATS (mean / invstd are running statistics, the
//                             eval-mode BatchNorm) dY = gamma * invstd * dXn
//   pn2_bn_relu_group_max_f32 apply + group max in one pass over Y, A never written (the pooled
//                             last layer of the frozen-statistics recompute, pn2/train.py)
// Layout: channels-last rows [M][C] with row stride ld (the SA path's layout), so every pass is
// a coalesced column-tiled sweep: a 256-thread block covers 64 columns x its row lanes of one
// row chunk; column sums reduce through LDS and chunk partials are merged in float64 by a
// per-column pass.  The templated sweeps come in two widths: W = 1, a thread per column (64
// column threads x 4 row lanes), and W = 4, a thread per 4 adjacent columns with one 16-byte
// load or store per row (16 column threads x 16 row lanes) when C and the strides are multiples
// of 4 and the bases 16-byte aligned (every SA / v1 layer; the host checks).  The 4-byte sweeps
// reached 2.9 (partial) and 3.9 TB/s (apply) at SSG training sizes.
#include "pn2_internal.h"
#include "bn_elem.h"  // xhat, the activation, dXn: shared with fc_train.hip

namespace pn2 {

constexpr int kTrCols = 64;     // columns per block
constexpr int kTrLanes = 4;     // row lanes per block of the one-column-per-thread sweeps
constexpr int kTrChunk = 1024;  // rows per chunk (partials per chunk), at most
constexpr int kTrChunkMin = 64;
constexpr int kTrMinBlocks = 2048;  // column sweeps: enough blocks to fill 256 CUs several times
constexpr int kTrUnroll = 8;    // rows in flight per thread in the column sweeps (W = 4: 4)

// W adjacent elements of a row: one 16-byte load for W = 4, through vector type V4.  The max
// kernels pass HIP's float4: with the compiler's own vector type the fused narrow one allocates
// 68 registers instead of 59 and loses a wave per SIMD; the backward sweeps allocate the same
// either way and measured 4-7% slower with float4.
template <typename T>
using tr_vec4 = T __attribute__((ext_vector_type(4)));

template <int W, typename T, typename V4 = tr_vec4<T>>
__device__ __forceinline__ void tr_load_row(const T *p, T (&v)[W]) {
    if constexpr (W == 4) {
        const V4 t = *reinterpret_cast<const V4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

// The block's two float64 column sums -> part[chunk blockIdx.y][p][C].  Row lane `lane` hands
// in its sums s[p][j] of columns col + j of the block's tile; each (p, column) is finished by
// one thread adding the LANES lane sums in ascending lane order.
template <int LANES, int W>
__device__ __forceinline__ void tr_col_reduce(const double (&s)[2][W], int lane, int col, int64_t C,
                                              double *__restrict__ part) {
    __shared__ double red[2][LANES][kTrCols];
#pragma unroll
    for (int j = 0; j < W; ++j) red[0][lane][col + j] = s[0][j], red[1][lane][col + j] = s[1][j];
    __syncthreads();
    if (threadIdx.x < 2 * kTrCols) {
        const int p = threadIdx.x / kTrCols, cl = threadIdx.x % kTrCols;
        const int64_t c = (int64_t)blockIdx.x * kTrCols + cl;
        if (c < C) {
            double t = red[p][0][cl];
            for (int l = 1; l < LANES; ++l) t += red[p][l][cl];
            part[((int64_t)blockIdx.y * 2 + p) * C + c] = t;
        }
    }
}

// partial column sums of Y and Y^2 over row chunk blockIdx.y -> part[chunk][2][C] (double).  The
// reduction is tr_col_reduce<kTrLanes, 1> written out, the first lane adding to its own registers:
// through the helper this kernel measured 6% slower on the 64-row chunks of the PointNet-v1 layers.
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float *__restrict__ Y, int64_t M,
                                                               int64_t C, int64_t ld, int64_t chunk,
                                                               double *__restrict__ part) {
    __shared__ double red[2][kTrLanes][kTrCols];
    const int tx = threadIdx.x & (kTrCols - 1), ty = threadIdx.x / kTrCols;
    const int64_t c = (int64_t)blockIdx.x * kTrCols + tx;
    const int64_t r0 = (int64_t)blockIdx.y * chunk;
    const int64_t r1 = r0 + chunk < M ? r0 + chunk : M;
    double s = 0.0, q = 0.0;
    if (c < C) {
        // kTrUnroll rows in flight per thread: the loop is load-latency bound otherwise
        int64_t r = r0 + ty;
        for (; r + (kTrUnroll - 1) * kTrLanes < r1; r += kTrUnroll * kTrLanes) {
            float v[kTrUnroll];
#pragma unroll
            for (int u = 0; u < kTrUnroll; ++u) v[u] = Y[(r + u * kTrLanes) * ld + c];
#pragma unroll
            for (int u = 0; u < kTrUnroll; ++u) s += (double)v[u], q += (double)v[u] * (double)v[u];
        }
        for (; r < r1; r += kTrLanes) {
            const double y = (double)Y[r * ld + c];
            s += y;
            q += y * y;
        }
    }
    red[0][ty][tx] = s;
    red[1][ty][tx] = q;
    __syncthreads();
    if (ty == 0 && c < C) {
        for (int l = 1; l < kTrLanes; ++l) s += red[0][l][tx], q += red[1][l][tx];
        part[((int64_t)blockIdx.y * 2 + 0) * C + c] = s;
        part[((int64_t)blockIdx.y * 2 + 1) * C + c] = q;
    }
}

// merge the chunk partials of column c; mean, invstd; running-stat update (torch's BatchNorm
// train-mode rule: biased variance normalises, unbiased variance enters running_var)
// sum of the nch chunk partials of column c (pair p of the [chunk][2][C] layout), one wave per
// column: each lane takes every 64th chunk, then a shuffle tree
__device__ __forceinline__ double wave_col_sum(const double *__restrict__ part, int64_t nch, int64_t C,
                                               int64_t c, int p) {
    const int lane = threadIdx.x;
    double s = 0.0;
    for (int64_t k = lane; k < nch; k += 64) s += part[(k * 2 + p) * C + c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__global__ __launch_bounds__(64) void bn_stats_final_kernel(const double *__restrict__ part, int64_t nch,
                                                            int64_t M, int64_t C, double eps,
                                                            double momentum, float *running_mean,
                                                            float *running_var,
                                                            float *__restrict__ mean_out,
                                                            float *__restrict__ invstd_out,
                                                            double *__restrict__ sxhat) {
    const int64_t c = blockIdx.x;
    const double s = wave_col_sum(part, nch, C, c, 0), q = wave_col_sum(part, nch, C, c, 1);
    if (threadIdx.x != 0) return;
    const double mean = s / (double)M;
    double var = q / (double)M - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + eps));
    // sum over rows of xhat = (y - mean_f32) * invstd_f32 with the rounded statistics the other
    // kernels use: the conv bias gradient (sum of dY) is -gamma*invstd*dgamma/M times this
    sxhat[c] = (s - (double)M * (double)mean_out[c]) * (double)invstd_out[c];
    if (running_mean && momentum > 0.0) {
        const double unb = M > 1 ? var * (double)M / (double)(M - 1) : var;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
    }
}

// elementwise sweeps: a block walks kTrEwRows rows of its column tile
constexpr int kTrEwRows = 64;

__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const float *__restrict__ Y, int64_t M,
                                                            int64_t C, int64_t ld,
                                                            const float *__restrict__ mean,
                                                            const float *__restrict__ invstd,
                                                            const float *__restrict__ gamma,
                                                            const float *__restrict__ beta,
                                                            float *__restrict__ A, int64_t lda,
                                                            int relu) {
    const int tx = threadIdx.x & (kTrCols - 1), ty = threadIdx.x / kTrCols;
    const int64_t c = (int64_t)blockIdx.x * kTrCols + tx;
    if (c >= C) return;
    const float mu = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    const int64_t r0 = (int64_t)blockIdx.y * kTrEwRows;
    const int64_t r1 = r0 + kTrEwRows < M ? r0 + kTrEwRows : M;
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += kTrLanes) {
        A[r * lda + c] = bn_act(Y[r * ld + c], mu, is, ga, be, relu);
    }
}

// one row's terms of S1 and S2
template <int W>
__device__ __forceinline__ void tr_bwd_sums(const float (&y)[W], const float (&d)[W], const float (&mu)[W],
                                            const float (&is)[W], const float (&ga)[W], const float (&be)[W],
                                            int relu, double (&s)[2][W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const float dd = bn_dxn(bn_xhat(y[j], mu[j], is[j]), ga[j], be[j], d[j], relu);
        s[0][j] += (double)dd;
        s[1][j] += (double)dd * bn_xhat64(y[j], mu[j], is[j]);
    }
}

// partial column sums of dXn and dXn * xhat over row chunk blockIdx.y, dA dense (the non-max
// layers) -> part[chunk][2][C]
template <int W>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(
    const float *__restrict__ Y, int64_t M, int64_t C, int64_t ld, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ dA, int64_t ldd, int relu, int64_t chunk, double *__restrict__ part) {
    constexpr int TX = kTrCols / W, TY = 256 / TX;
    constexpr int U = W == 4 ? 4 : kTrUnroll;  // rows in flight (two loads each)
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int64_t c = (int64_t)blockIdx.x * kTrCols + tx * W;
    const int64_t r0 = (int64_t)blockIdx.y * chunk;
    const int64_t r1 = r0 + chunk < M ? r0 + chunk : M;
    double s[2][W] = {};
    if (c < C) {  // W == 4: C % 4 == 0, so c < C covers c + 3
        float mu[W], is[W], ga[W], be[W];
        tr_load_row<W>(mean + c, mu), tr_load_row<W>(invstd + c, is);
        tr_load_row<W>(gamma + c, ga), tr_load_row<W>(beta + c, be);
        int64_t r = r0 + ty;
        for (; r + (U - 1) * TY < r1; r += U * TY) {
            float y[U][W], d[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) tr_load_row<W>(Y + (r + u * TY) * ld + c, y[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) tr_load_row<W>(dA + (r + u * TY) * ldd + c, d[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) tr_bwd_sums<W>(y[u], d[u], mu, is, ga, be, relu, s);
        }
        for (; r < r1; r += TY) {
            float y[W], d[W];
            tr_load_row<W>(Y + r * ld + c, y);
            tr_load_row<W>(dA + r * ldd + c, d);
            tr_bwd_sums<W>(y, d, mu, is, ga, be, relu, s);
        }
    }
    tr_col_reduce<TY, W>(s, ty, tx * W, C, part);
}

// The same column sums when dA is scattered from the max (the last layer): dXn is nonzero only
// on each group's argmax row, so S1 = sum_g mask * dOut[g][c] and S2 = sum_g mask * dOut[g][c] *
// xhat(Y[g*K + arg[g][c]][c]) read G = M/K gathered rows instead of sweeping all M (K = 32-64 x
// fewer bytes: the SA layers' widest Y, 268 MB at SSG, is the largest term of a training step).
// Chunk blockIdx.y covers groups [y*chunk, y*chunk + chunk); partials as above.
__global__ __launch_bounds__(256) void bn_bwd_partial_gather_kernel(
    const float *__restrict__ Y, int64_t G, int64_t C, int64_t ld, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ dOut, int64_t ldo, const int32_t *__restrict__ arg, int64_t K, int relu,
    int64_t chunk, double *__restrict__ part) {
    const int tx = threadIdx.x & (kTrCols - 1), ty = threadIdx.x / kTrCols;
    const int64_t c = (int64_t)blockIdx.x * kTrCols + tx;
    const int64_t g0 = (int64_t)blockIdx.y * chunk;
    const int64_t g1 = g0 + chunk < G ? g0 + chunk : G;
    double s[2][1] = {};
    if (c < C) {
        const float mu[1] = {mean[c]}, is[1] = {invstd[c]}, ga[1] = {gamma[c]}, be[1] = {beta[c]};
        for (int64_t g = g0 + ty; g < g1; g += kTrLanes) {
            const int64_t r = g * K + arg[g * C + c];
            const float y[1] = {Y[r * ld + c]}, d[1] = {dOut[g * ldo + c]};
            tr_bwd_sums<1>(y, d, mu, is, ga, be, relu, s);
        }
    }
    tr_col_reduce<kTrLanes, 1>(s, ty, tx, C, part);
}

// FROZEN (PN2_LAYER_FROZEN_STATS): mean / invstd are constants of the caller (running statistics),
// so dY carries no batch-statistics correction and sum_r dY = gamma*invstd*S1; sxhat is not read.
template <bool FROZEN>
__global__ __launch_bounds__(64) void bn_bwd_final_kernel(const double *__restrict__ part, int64_t nch,
                                                          int64_t M, int64_t C, const float *__restrict__ gamma,
                                                          const float *__restrict__ invstd,
                                                          const double *__restrict__ sxhat,
                                                          float *__restrict__ dbeta, float *__restrict__ dgamma,
                                                          float *__restrict__ dbias, double *__restrict__ sums) {
    const int64_t c = blockIdx.x;
    const double s1 = wave_col_sum(part, nch, C, c, 0), s2 = wave_col_sum(part, nch, C, c, 1);
    if (threadIdx.x != 0) return;
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
    sums[c] = s1;
    sums[C + c] = s2;
    if constexpr (FROZEN) {
        if (dbias) dbias[c] = (float)((double)gamma[c] * (double)invstd[c] * s1);
    } else {
        // sum_r dY = gamma*invstd*(s1 - M*(s1/M) - (s2/M)*sum_r xhat): the conv bias gradient
        if (dbias) dbias[c] = (float)(-(double)gamma[c] * (double)invstd[c] * (s2 / (double)M) * sxhat[c]);
    }
}

// dY = gamma * invstd * (dXn - S1/M - xhat * S2/M) (FROZEN: dY = gamma * invstd * dXn), dA dense
// [M][C] (ldd) or scattered from the max (dOut, arg, K).  Each thread holds 4 rows in flight per
// round; their loads are clamped to the last row, so they stay branch-free.
template <int W, bool FROZEN>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(
    const float *__restrict__ Y, int64_t M, int64_t C, int64_t ld, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ dA, int64_t ldd, const float *__restrict__ dOut, int64_t ldo,
    const int32_t *__restrict__ arg, int64_t K, int relu, const double *__restrict__ sums,
    float *__restrict__ dY, int64_t ldy) {
    constexpr int TX = kTrCols / W, TY = 256 / TX, U = 4;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int64_t c = (int64_t)blockIdx.x * kTrCols + tx * W;
    if (c >= C) return;
    float mu[W], is[W], ga[W], be[W], m1[W], m2[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        mu[j] = mean[c + j], is[j] = invstd[c + j], ga[j] = gamma[c + j], be[j] = beta[c + j];
        if constexpr (FROZEN)
            m1[j] = m2[j] = 0.f;
        else
            m1[j] = (float)(sums[c + j] / (double)M), m2[j] = (float)(sums[C + c + j] / (double)M);
    }
    const int64_t r0 = (int64_t)blockIdx.y * kTrEwRows;
    constexpr int ROUNDS = kTrEwRows / (U * TY);  // W = 1: 4, W = 4: 1
    for (int q = 0; q < ROUNDS; ++q) {
        const int64_t rb = r0 + ty + q * (U * TY);
        if (rb >= M) break;
        float y[U][W], d[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = rb + u * TY;
            const int64_t rr = r < M ? r : M - 1;
            tr_load_row<W>(Y + rr * ld + c, y[u]);
            if (dA) {
                tr_load_row<W>(dA + rr * ldd + c, d[u]);
            } else {
                // 32-bit division (the host checks M < 2^31): the 64-bit one is a long call sequence
                const uint32_t g = (uint32_t)rr / (uint32_t)K, k = (uint32_t)rr - g * (uint32_t)K;
                int32_t a[W];
                tr_load_row<W>(dOut + (int64_t)g * ldo + c, d[u]);
                tr_load_row<W>(arg + (int64_t)g * C + c, a);
#pragma unroll
                for (int j = 0; j < W; ++j) d[u][j] = a[j] == (int32_t)k ? d[u][j] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t r = rb + u * TY;
            if (r >= M) break;
            float o[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const float xh = bn_xhat(y[u][j], mu[j], is[j]);
                const float dd = bn_dxn(xh, ga[j], be[j], d[u][j], relu);
                if constexpr (FROZEN)
                    o[j] = ga[j] * is[j] * dd;
                else
                    o[j] = ga[j] * is[j] * (dd - m1[j] - xh * m2[j]);
            }
            if constexpr (W == 4)
                *reinterpret_cast<float4 *>(dY + r * ldy + c) = make_float4(o[0], o[1], o[2], o[3]);
            else
                dY[r * ldy + c] = o[0];
        }
    }
}

// ---- max over each K rows and its first argmax, with (ACT: pn2_bn_relu_group_max_f32) or
// without (pn2_group_max_f32) BatchNorm + ReLU applied to every element on the way in.  The
// fused form is the pooled last layer of the frozen-statistics recompute, whose activation A is
// only needed for its max and argmax: each element is bn_relu_apply_kernel's expression (this
// file is compiled without contraction, so the roundings are the same) and enters the same walk,
// so out and arg are those of apply followed by pn2_group_max_f32.  No LDS in the narrow kernel,
// 2 x 4 KiB in the wide one; the kernels read M*C*4 bytes once and write G*C*8: HBM-bound (the A
// round trip the fused form replaces is 2*M*C*4 bytes).

// (v, a) beats (m, b) in the max's order: NaN above every number, then value, then the first
// index (torch.max's first argmax)
__device__ __forceinline__ bool tr_better(float v, int32_t a, float m, int32_t b) {
    if (v != v) return m == m || a < b;
    if (m != m) return false;
    return v > m || (v == m && a < b);
}

// One row of a lane's walk in increasing row order: strict > keeps the first maximum, a NaN
// replaces a number only, the lane's first row replaces the start value.  Written as selects on
// one flag: as a branch around the two assignments, the last row of the unrolled round came out
// of the compiler updating m but not a when v was NaN (ROCm 7 clang, read in the ISA; caught by
// tests/test_gpu_train_kernels.py test_group_max with a NaN on row 121 of K = 257).
__device__ __forceinline__ void tr_take(float v, int32_t i, float &m, int32_t &a) {
    const bool t = (v > m) | ((v != v) & (m == m)) | (a == 0x7fffffff);
    m = t ? v : m;
    a = t ? i : a;
}

// the element that enters the max: ACT applies BatchNorm (+ ReLU), else the value as read
template <bool ACT>
__device__ __forceinline__ float tr_act(float y, float mu, float is, float ga, float be, int relu) {
    if constexpr (!ACT) return y;
    return bn_act(y, mu, is, ga, be, relu);
}

// the per-column BatchNorm constants of a thread's W columns (ACT only: the pointers are null
// otherwise and the values unused)
template <int W, bool ACT>
__device__ __forceinline__ void tr_act_consts(const float *mean, const float *invstd, const float *gamma,
                                              const float *beta, int64_t c, float (&mu)[W], float (&is)[W],
                                              float (&ga)[W], float (&be)[W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
        if constexpr (ACT)
            mu[j] = mean[c + j], is[j] = invstd[c + j], ga[j] = gamma[c + j], be[j] = beta[c + j];
        else
            mu[j] = is[j] = ga[j] = be[j] = 0.f;
    }
}

template <int W>
__device__ __forceinline__ void tr_store_max(float *out, int32_t *arg, const float (&m)[W], const int32_t (&a)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4 *>(out) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<int4 *>(arg) = make_int4(a[0], a[1], a[2], a[3]);
    } else {
        out[0] = m[0];
        arg[0] = a[0];
    }
}

// small K: one thread per (group, W columns); blockIdx.x walks the groups (G has no 65535 limit)
template <int W, bool ACT>
__global__ __launch_bounds__(256) void bn_relu_group_max_kernel(
    const float *__restrict__ Y, int64_t G, int64_t K, int64_t C, int64_t ld, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ out, int64_t ldo, int32_t *__restrict__ arg, int relu) {
    constexpr int TX = kTrCols / W, TY = 256 / TX;
    constexpr int U = W == 4 ? 4 : 8;  // rows in flight
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int64_t c = (int64_t)blockIdx.y * kTrCols + tx * W;
    const int64_t g = (int64_t)blockIdx.x * TY + ty;
    if (c >= C || g >= G) return;  // W == 4: C % 4 == 0, so c < C covers c + 3
    float mu[W], is[W], ga[W], be[W], m[W];
    int32_t a[W];
    tr_act_consts<W, ACT>(mean, invstd, gamma, beta, c, mu, is, ga, be);
#pragma unroll
    for (int j = 0; j < W; ++j) m[j] = -__builtin_inff(), a[j] = 0x7fffffff;
    const float *p = Y + g * K * ld + c;
    int64_t k = 0;
    for (; k + U <= K; k += U) {
        float v[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) tr_load_row<W, float, float4>(p + (k + u) * ld, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < W; ++j)
                tr_take(tr_act<ACT>(v[u][j], mu[j], is[j], ga[j], be[j], relu), (int32_t)(k + u), m[j], a[j]);
    }
    for (; k < K; ++k) {
        float v[W];
        tr_load_row<W, float, float4>(p + k * ld, v);
#pragma unroll
        for (int j = 0; j < W; ++j)
            tr_take(tr_act<ACT>(v[j], mu[j], is[j], ga[j], be[j], relu), (int32_t)k, m[j], a[j]);
    }
    tr_store_max<W>(out + g * ldo + c, arg + g * C + c, m, a);
}

// Large K (the group_all layer, a PointNet-v1 max over a cloud's N points): one block per (group,
// 64 columns), the K rows split over kTrWideLanes row lanes (U rows in flight each), lanes merged
// through LDS.  One thread per (group, column) walking all K rows would serialise K/8 dependent
// load rounds.  Each entry point keeps the block order it had before the two were merged: the
// plain max (the PointNet-v1 max over K = 1024 rows of 1024 columns) has its column tiles on
// grid.x, so that neighbouring blocks read the same rows -- with the groups there it measured
// 3.6% slower -- and the fused form its groups on grid.x.
constexpr int kTrWideLanes = 16;
constexpr int kTrWideK = 256;  // K from which the wide kernel is used

template <int W, bool ACT>
__global__ __launch_bounds__(kTrCols / W * kTrWideLanes) void bn_relu_group_max_wide_kernel(
    const float *__restrict__ Y, int64_t K, int64_t C, int64_t ld, const float *__restrict__ mean,
    const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
    float *__restrict__ out, int64_t ldo, int32_t *__restrict__ arg, int relu) {
    __shared__ float sv[kTrWideLanes][kTrCols];
    __shared__ int32_t sa[kTrWideLanes][kTrCols];
    constexpr int TX = kTrCols / W;
    constexpr int U = W == 4 ? 4 : 8;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const unsigned tile = ACT ? blockIdx.y : blockIdx.x;
    const int64_t c = (int64_t)tile * kTrCols + tx * W;
    const int64_t g = ACT ? blockIdx.x : blockIdx.y;  // the host uses this form for G < 65536 only
    float m[W];
    int32_t a[W];
#pragma unroll
    for (int j = 0; j < W; ++j) m[j] = -__builtin_inff(), a[j] = 0x7fffffff;
    if (c < C) {
        float mu[W], is[W], ga[W], be[W];
        tr_act_consts<W, ACT>(mean, invstd, gamma, beta, c, mu, is, ga, be);
        const float *p = Y + g * K * ld + c;
        int64_t k = ty;
        for (; k + (U - 1) * kTrWideLanes < K; k += U * kTrWideLanes) {
            float v[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) tr_load_row<W, float, float4>(p + (k + u * kTrWideLanes) * ld, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < W; ++j)
                    tr_take(tr_act<ACT>(v[u][j], mu[j], is[j], ga[j], be[j], relu),
                            (int32_t)(k + u * kTrWideLanes), m[j], a[j]);
        }
        for (; k < K; k += kTrWideLanes) {
            float v[W];
            tr_load_row<W, float, float4>(p + k * ld, v);
#pragma unroll
            for (int j = 0; j < W; ++j)
                tr_take(tr_act<ACT>(v[j], mu[j], is[j], ga[j], be[j], relu), (int32_t)k, m[j], a[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) sv[ty][tx * W + j] = m[j], sa[ty][tx * W + j] = a[j];
    __syncthreads();
    // the first 64 threads finish one column each: lane 0 holds row 0 (K >= 1), later lanes may be empty
    const int col = threadIdx.x;
    const int64_t cc = (int64_t)tile * kTrCols + col;
    if (col < kTrCols && cc < C) {
        float bm = sv[0][col];
        int32_t ba = sa[0][col];
        for (int l = 1; l < kTrWideLanes; ++l)
            if (sa[l][col] != 0x7fffffff && tr_better(sv[l][col], sa[l][col], bm, ba)) bm = sv[l][col], ba = sa[l][col];
        out[g * ldo + cc] = bm;
        arg[g * C + cc] = ba;
    }
}

// rows per partial chunk of the column sweeps: kTrChunk, halved while the grid (column tiles x
// chunks) would have fewer than kTrMinBlocks blocks -- PointNet-v1 layers have M = B*N = 32k
// rows (32 chunks of 1024: a 64-column layer would run on 32 workgroups), SA layers 500k
inline int64_t chunk_rows(int64_t M, int64_t C) {
    const int64_t tiles = (C + kTrCols - 1) / kTrCols;
    int64_t ch = kTrChunk;
    while (ch > kTrChunkMin && tiles * ((M + ch - 1) / ch) < kTrMinBlocks) ch >>= 1;
    return ch;
}
inline int64_t chunks(int64_t M, int64_t C) { const int64_t ch = chunk_rows(M, C); return (M + ch - 1) / ch; }
inline unsigned col_tiles(int64_t C) { return (unsigned)((C + kTrCols - 1) / kTrCols); }

// every pointer 16-byte aligned (null counts as aligned)
template <typename... P>
inline bool aligned16(P... p) { return ((... | (uintptr_t)p) & 15) == 0; }

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_bn_train_workspace_bytes(int64_t M, int64_t C) {
    if (M <= 0 || C <= 0) return 0;
    return chunks(M, C) * 2 * C * (int64_t)sizeof(double) + 3 * C * (int64_t)sizeof(double);
}

extern "C" int pn2_bn_train_stats_f32(const float *Y, int64_t M, int64_t C, int64_t ld, double eps,
                                      double momentum, float *running_mean, float *running_var,
                                      float *mean, float *invstd, double *sxhat, void *ws,
                                      int64_t ws_bytes, void *stream) {
    PN2_REQUIRE(Y && mean && invstd && sxhat && ws, "pn2_bn_train_stats_f32: null pointer");
    PN2_REQUIRE(M >= 1 && C >= 1 && ld >= C, "pn2_bn_train_stats_f32: bad shape");
    PN2_REQUIRE(ws_bytes >= pn2_bn_train_workspace_bytes(M, C), "pn2_bn_train_stats_f32: workspace too small");
    PN2_REQUIRE(momentum <= 0.0 || (running_mean && running_var), "pn2_bn_train_stats_f32: running stats");
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(col_tiles(C), (unsigned)chunks(M, C)), dim3(256), 0, st, Y, M,
                       C, ld, chunk_rows(M, C), part);
    PN2_LAUNCH_CHECK("bn_stats_partial_kernel");
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((unsigned)C), dim3(64), 0, st, part, chunks(M, C), M, C,
                       eps, momentum, running_mean, running_var, mean, invstd, sxhat);
    PN2_LAUNCH_CHECK("bn_stats_final_kernel");
    return PN2_OK;
}

extern "C" int pn2_bn_relu_apply_f32(const float *Y, int64_t M, int64_t C, int64_t ld, const float *mean,
                                     const float *invstd, const float *gamma, const float *beta, float *A,
                                     int64_t lda, int flags, void *stream) {
    PN2_REQUIRE(Y && mean && invstd && gamma && beta && A, "pn2_bn_relu_apply_f32: null pointer");
    PN2_REQUIRE(M >= 0 && C >= 1 && ld >= C && lda >= C, "pn2_bn_relu_apply_f32: bad shape");
    PN2_REQUIRE((flags & ~PN2_LAYER_NO_RELU) == 0, "pn2_bn_relu_apply_f32: unknown flags");
    if (M == 0) return PN2_OK;
    hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(col_tiles(C), (unsigned)((M + kTrEwRows - 1) / kTrEwRows)),
                       dim3(256), 0, as_stream(stream), Y, M, C, ld, mean, invstd, gamma, beta, A, lda,
                       (flags & PN2_LAYER_NO_RELU) ? 0 : 1);
    PN2_LAUNCH_CHECK("bn_relu_apply_kernel");
    return PN2_OK;
}

extern "C" int pn2_bn_train_forward_f32(const float *Y, int64_t M, int64_t C, int64_t ld, double eps,
                                        double momentum, float *running_mean, float *running_var,
                                        const float *gamma, const float *beta, float *A, int64_t lda,
                                        int flags, float *stats, double *sxhat, void *ws, int64_t ws_bytes,
                                        void *stream) {
    PN2_REQUIRE(stats, "pn2_bn_train_forward_f32: null pointer");
    const int rc = pn2_bn_train_stats_f32(Y, M, C, ld, eps, momentum, running_mean, running_var, stats,
                                          stats + C, sxhat, ws, ws_bytes, stream);
    if (rc != PN2_OK) return rc;
    return pn2_bn_relu_apply_f32(Y, M, C, ld, stats, stats + C, gamma, beta, A, lda, flags, stream);
}

// the max of both entry points (ACT: with the activation): wide from K = kTrWideK on while the
// groups fit grid.y, narrow otherwise
static bool max_is_wide(int64_t G, int64_t K) { return K >= kTrWideK && G < 65536; }

template <int W, bool ACT>
static int launch_group_max(const float *Y, int64_t G, int64_t K, int64_t C, int64_t ld, const float *mean,
                            const float *invstd, const float *gamma, const float *beta, float *out, int64_t ldo,
                            int32_t *arg, int relu, hipStream_t st) {
    constexpr int TX = kTrCols / W, TY = 256 / TX;
    if (max_is_wide(G, K)) {
        const dim3 grid = ACT ? dim3((unsigned)G, col_tiles(C)) : dim3(col_tiles(C), (unsigned)G);
        hipLaunchKernelGGL((bn_relu_group_max_wide_kernel<W, ACT>), grid,
                           dim3(TX * kTrWideLanes), 0, st, Y, K, C, ld, mean, invstd, gamma, beta, out, ldo, arg, relu);
        PN2_LAUNCH_CHECK("bn_relu_group_max_wide_kernel");
        return PN2_OK;
    }
    hipLaunchKernelGGL((bn_relu_group_max_kernel<W, ACT>), dim3((unsigned)((G + TY - 1) / TY), col_tiles(C)),
                       dim3(256), 0, st, Y, G, K, C, ld, mean, invstd, gamma, beta, out, ldo, arg, relu);
    PN2_LAUNCH_CHECK("bn_relu_group_max_kernel");
    return PN2_OK;
}

extern "C" int pn2_group_max_f32(const float *A, int64_t G, int64_t K, int64_t C, int64_t lda, float *out,
                                 int64_t ldo, int32_t *arg, void *stream) {
    PN2_REQUIRE(A && out && arg, "pn2_group_max_f32: null pointer");
    PN2_REQUIRE(G >= 0 && K >= 1 && K < ((int64_t)1 << 31) && C >= 1 && lda >= C && ldo >= C,
                "pn2_group_max_f32: bad shape");
    if (G == 0) return PN2_OK;
    // the wide form stays on one column per thread, as it was measured
    const bool vec4 = !max_is_wide(G, K) && (C % 4) == 0 && (lda % 4) == 0 && (ldo % 4) == 0 &&
                      aligned16(A, out, arg);
    return vec4 ? launch_group_max<4, false>(A, G, K, C, lda, nullptr, nullptr, nullptr, nullptr, out, ldo, arg, 0,
                                             as_stream(stream))
                : launch_group_max<1, false>(A, G, K, C, lda, nullptr, nullptr, nullptr, nullptr, out, ldo, arg, 0,
                                             as_stream(stream));
}

extern "C" int pn2_bn_relu_group_max_f32(const float *Y, int64_t G, int64_t K, int64_t C, int64_t ld,
                                         const float *mean, const float *invstd, const float *gamma,
                                         const float *beta, float *out, int64_t ldo, int32_t *arg, int flags,
                                         void *stream) {
    PN2_REQUIRE(Y && mean && invstd && gamma && beta && out && arg, "pn2_bn_relu_group_max_f32: null pointer");
    PN2_REQUIRE(G >= 0 && K >= 1 && K < ((int64_t)1 << 31) && C >= 1 && ld >= C && ldo >= C,
                "pn2_bn_relu_group_max_f32: bad shape");
    PN2_REQUIRE((flags & ~PN2_LAYER_NO_RELU) == 0, "pn2_bn_relu_group_max_f32: unknown flags");
    if (G == 0) return PN2_OK;
    const int relu = (flags & PN2_LAYER_NO_RELU) ? 0 : 1;
    const bool vec4 = (C % 4) == 0 && (ld % 4) == 0 && (ldo % 4) == 0 && aligned16(Y, out, arg);
    return vec4 ? launch_group_max<4, true>(Y, G, K, C, ld, mean, invstd, gamma, beta, out, ldo, arg, relu,
                                            as_stream(stream))
                : launch_group_max<1, true>(Y, G, K, C, ld, mean, invstd, gamma, beta, out, ldo, arg, relu,
                                            as_stream(stream));
}

// the backward's kernels for a column width and a statistics mode
struct BwdKernels {
    decltype(&bn_bwd_partial_kernel<1>) partial;
    decltype(&bn_bwd_final_kernel<false>) merge;
    decltype(&bn_bwd_apply_kernel<1, false>) apply;
};
template <int W, bool FROZEN>
static BwdKernels bwd_kernels() {
    return {bn_bwd_partial_kernel<W>, bn_bwd_final_kernel<FROZEN>, bn_bwd_apply_kernel<W, FROZEN>};
}
static BwdKernels pick_bwd_kernels(bool vec4, bool frozen) {
    if (vec4) return frozen ? bwd_kernels<4, true>() : bwd_kernels<4, false>();
    return frozen ? bwd_kernels<1, true>() : bwd_kernels<1, false>();
}

extern "C" int pn2_bn_relu_backward_f32(const float *Y, int64_t M, int64_t C, int64_t ld, const float *mean,
                                        const float *invstd, const float *gamma, const float *beta,
                                        const float *dA, int64_t ldd, const float *dOut, int64_t ldo,
                                        const int32_t *arg, int64_t K, const double *sxhat,
                                        float *dY, int64_t ldy, float *dgamma, float *dbeta,
                                        float *dbias, void *ws, int64_t ws_bytes, int flags, void *stream) {
    const bool frozen = (flags & PN2_LAYER_FROZEN_STATS) != 0;  // sxhat is not read
    PN2_REQUIRE(Y && mean && invstd && gamma && beta && dY && dgamma && dbeta && ws && (!dbias || sxhat || frozen),
                "pn2_bn_relu_backward_f32: null pointer");
    PN2_REQUIRE(dA || (dOut && arg && K >= 1 && M % K == 0), "pn2_bn_relu_backward_f32: need dA or (dOut, arg, K)");
    PN2_REQUIRE(M >= 1 && M < ((int64_t)1 << 31) && C >= 1 && ld >= C && ldy >= C && (!dA || ldd >= C) &&
                    (dA || ldo >= C),
                "pn2_bn_relu_backward_f32: bad shape");
    PN2_REQUIRE(ws_bytes >= pn2_bn_train_workspace_bytes(M, C), "pn2_bn_relu_backward_f32: workspace too small");
    PN2_REQUIRE((flags & ~(PN2_LAYER_NO_RELU | PN2_LAYER_FROZEN_STATS)) == 0, "pn2_bn_relu_backward_f32: unknown flags");
    const int relu = (flags & PN2_LAYER_NO_RELU) ? 0 : 1;
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(ws);
    double *sums = part + chunks(M, C) * 2 * C;
    const bool vec4 = (C % 4) == 0 && (ld % 4) == 0 && (ldy % 4) == 0 && ((dA ? ldd : ldo) % 4) == 0 &&
                      (dA ? aligned16(dA) : aligned16(dOut, arg)) &&
                      aligned16(Y, dY, mean, invstd, gamma, beta);
    const BwdKernels kn = pick_bwd_kernels(vec4, frozen);
    int64_t nch;
    if (dA) {
        nch = chunks(M, C);
        hipLaunchKernelGGL(kn.partial, dim3(col_tiles(C), (unsigned)nch), dim3(256), 0, st, Y, M, C, ld, mean, invstd,
                           gamma, beta, dA, ldd, relu, chunk_rows(M, C), part);
        PN2_LAUNCH_CHECK("bn_bwd_partial_kernel");
    } else {  // scattered from the max: only the G argmax rows contribute
        // The workspace holds chunks(M, C) partials.  chunk_rows(G, C) halves from another start
        // than chunk_rows(M, C), so with K no power of two G/gch can pass M/ch (C=4, K=3,
        // G=174678: 2730 against 2048); the group chunk is then doubled until it fits.
        const int64_t G = M / K, cap = chunks(M, C);
        int64_t gch = chunk_rows(G, C);
        while ((G + gch - 1) / gch > cap) gch <<= 1;
        nch = (G + gch - 1) / gch;
        hipLaunchKernelGGL(bn_bwd_partial_gather_kernel, dim3(col_tiles(C), (unsigned)nch), dim3(256), 0, st, Y, G, C,
                           ld, mean, invstd, gamma, beta, dOut, ldo, arg, K, relu, gch, part);
        PN2_LAUNCH_CHECK("bn_bwd_partial_gather_kernel");
    }
    hipLaunchKernelGGL(kn.merge, dim3((unsigned)C), dim3(64), 0, st, part, nch, M, C, gamma, invstd, sxhat, dbeta,
                       dgamma, dbias, sums);
    PN2_LAUNCH_CHECK("bn_bwd_final_kernel");
    hipLaunchKernelGGL(kn.apply, dim3(col_tiles(C), (unsigned)((M + kTrEwRows - 1) / kTrEwRows)), dim3(256), 0, st, Y,
                       M, C, ld, mean, invstd, gamma, beta, dA, ldd, dOut, ldo, arg, K, relu, sums, dY, ldy);
    PN2_LAUNCH_CHECK("bn_bwd_apply_kernel");
    return PN2_OK;
}
