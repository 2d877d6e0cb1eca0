// fc_train.hip -- a heads' fully connected layer under autograd, one launch each way
// (include/pn2.h states the contracts and the order rules):
//   forward    Y = X W^T + b, the BatchNorm1d column statistics of Y (batch or running), the
//              running-stat update, A = act(bn(Y))
//   backward   dXn = dA * [A > 0], dbeta, dgamma, dY, dbias = sum_r dY, dW = dY^T X
//
// Reference: fc1/bn1/relu, fc2/bn2/relu, fc3 of the heads under the training loops' autograd,
// the reference's model/pointnet2_cls_ssg.py:31-36, rotation_ssg.py:33-37,
// translation_ssg.py:23-26 (the mean MLP), pointnet_utils.py:33-40 (the T-Nets' FC tail)
// (pn2/train.py _FcBnTrain).
//
// One kernel template per direction, fc_fwd_kernel<kOneSlab> / fc_bwd_kernel<kOneSlab>.  A
// workgroup (256 threads = 4 waves) owns a block of kFcNB = 4 output columns and every row of
// them, walked in slabs of kFcRows = 64 rows: no workspace, no sum across workgroups, and a
// column's sum never leaves its wave.
//
// Forward, per slab: wave w owns column n0 + w, lane r the slab's row r (one accumulator per
// thread; lanes past the slab compute its row 0 again and store nothing).  The slab's X
// ([64][64] floats) and the 4 W rows ([4][64]) go through LDS in K-chunks of 64: 16-byte loads
// where base and leading dimension allow, dword loads else and in a chunk's ragged last group,
// zeros past K with no load issued; the next chunk's loads are issued before the current chunk's
// FMAs.  An X row is 68 floats apart in LDS: the ds_read_b128 of 16 consecutive rows fall on 16
// distinct 16-byte slots.  The W reads are wave-uniform (broadcast); the W chunk is 1/16 of the X
// chunk's bytes, so it is fetched again per slab instead of K-sized LDS.  The element's sum is
// ONE fma chain over ascending k from +0 (__fmaf_rn), then one add of the bias: the order is a
// function of K alone.  Y is stored.  The column statistics are a serial float64 walk over
// v_readlane of the slab's rows in order, done by every lane of the wave alike and carried from
// slab to slab: each lane then holds its column's mean / invstd without LDS or a barrier.
// Frozen statistics / no BN: A is written with Y.  Batch statistics: the activation needs the
// whole column's mean, so once it is known each thread reads its own Y elements back and writes A.
//
// Backward.  Sweep 1 (wave = column, lane = row): dXn and the float64 walks for dbeta / dgamma
// over all slabs.  Sweep 2, once per 1024 columns of dW: a slab's dY (dA and Y read again, dXn by
// the same expression), stored and walked for dbias in the first pass only, handed as [row][4
// columns] through 1 KB of LDS to the dW step: thread t owns the 4 consecutive k = 4t .. 4t+3
// (+ 1024 per pass) of all 4 columns' dW rows and continues, for the slab's rows in order, its
// fma chains: one 16-byte load of X[r][k..k+3] (coalesced, L2-resident), one broadcast
// ds_read_b128 of dY[r][0..3], 16 __fmaf_rn.  The dW accumulators stay in their thread's
// registers over all slabs.
//
// kOneSlab (B <= kFcRows; pn2_fc_bn_forward_f32 / pn2_fc_bn_backward_f32) is the same code with
// the slab loops at one trip, decided at compile time: y stays in its register from the GEMM to
// the activation (no read-back of Y); dXn and Y stay in registers from sweep 1 to sweep 2; the
// block's dY is put into LDS once and serves every pass over dW's columns.  Every float
// expression and every order of summation below is written once, so the any-B entries
// (pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32) give the one-slab entries' bits up
// to kFcRows rows by construction.
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile): an fma is only where
// __fmaf_rn says so; every other float operation rounds on its own.  xhat, the activation and
// dXn are bn_elem.h's, shared with train.hip.
#include "pn2_internal.h"
#include "bn_elem.h"

namespace pn2 {

constexpr int kFcRows = 64;            // rows of a slab: a row per lane (pn2_fc_train_max_rows)
constexpr int kFcNB = 4;               // output columns per workgroup: a column per wave
constexpr int kFcKC = 64;              // K chunk through LDS
constexpr int kFcG = kFcKC / 4;        // 16-byte groups per chunk row
constexpr int kFcLdx = kFcG + 1;       // LDS stride of an X row, in 16-byte slots (68 floats)
constexpr int kFcThreads = 256;
constexpr int kFcXI = kFcRows * kFcG / kFcThreads;  // X groups per thread and chunk (4)
constexpr int64_t kFcRowsMaxB = 1ll << 30;  // the slab loop's int row counter stays below 2^31
static_assert(kFcNB * 64 == kFcThreads, "a wave per column");
static_assert(kFcNB * kFcG <= 64, "the W chunk is fetched by the first wave");

enum { kFcNoBn = 0, kFcBatch = 1, kFcFrozen = 2 };

// row[k .. k+3], zeros from K on (no load issued there)
__device__ __forceinline__ float4 fc_fetch4(const float *__restrict__ row, int64_t k, int64_t K, bool vec) {
    if (vec && k + 4 <= K) return *reinterpret_cast<const float4 *>(row + k);
    float4 v;
    v.x = k < K ? row[k] : 0.f;
    v.y = k + 1 < K ? row[k + 1] : 0.f;
    v.z = k + 2 < K ? row[k + 2] : 0.f;
    v.w = k + 3 < K ? row[k + 3] : 0.f;
    return v;
}

// lane r's value, the same in every lane (r wave-uniform)
__device__ __forceinline__ float fc_lane(float v, int r) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
}

// sum over k of Xs[lane][k] * W[n0 + wave][k] for the slab of `rows` rows at Xs: the chunked K
// loop through sx / sw (file comment).  Every thread of the block calls it; ends on a barrier.
__device__ __forceinline__ float fc_slab_dot(const float *__restrict__ Xs, int64_t ldx, int rows,
                                             const float *__restrict__ W, int64_t ldw, int64_t n0, int64_t N,
                                             int64_t K, bool vecx, bool vecw, float4 *sx, float4 *sw) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int items = rows * kFcG;  // (row, group) pairs of the slab's X chunk
    float4 fx[kFcXI], fw;
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < kFcXI; ++q) {
            const int i = tid + q * kFcThreads;
            if (i < items) fx[q] = fc_fetch4(Xs + (int64_t)(i / kFcG) * ldx, k0 + (i % kFcG) * 4, K, vecx);
        }
        if (tid < kFcNB * kFcG) {
            const int64_t n = n0 + tid / kFcG;
            fw = n < N ? fc_fetch4(W + n * ldw, k0 + (tid % kFcG) * 4, K, vecw) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);

    float acc = 0.f;
    const int rr = lane < rows ? lane : 0;
    for (int64_t k0 = 0; k0 < K; k0 += kFcKC) {
#pragma unroll
        for (int q = 0; q < kFcXI; ++q) {
            const int i = tid + q * kFcThreads;
            if (i < items) sx[(i / kFcG) * kFcLdx + i % kFcG] = fx[q];
        }
        if (tid < kFcNB * kFcG) sw[tid] = fw;
        __syncthreads();
        if (k0 + kFcKC < K) fetch(k0 + kFcKC);  // in flight during this chunk's FMAs
        const int64_t left = K - k0;
        const int ng = left >= kFcKC ? kFcG : (int)((left + 3) / 4);  // the last group zero-padded
#pragma unroll 4
        for (int g = 0; g < ng; ++g) {
            const float4 x = sx[rr * kFcLdx + g], w = sw[wave * kFcG + g];
            acc = __fmaf_rn(x.x, w.x, acc);
            acc = __fmaf_rn(x.y, w.y, acc);
            acc = __fmaf_rn(x.z, w.z, acc);
            acc = __fmaf_rn(x.w, w.w, acc);
        }
        __syncthreads();
    }
    return acc;
}

// mean / invstd of a column from its float64 sums over B rows (biased variance, not below 0), and
// the running-statistics update (unbiased variance) by the wave's first lane
__device__ __forceinline__ void fc_batch_stats(double s, double q, int B, double eps, double momentum,
                                               float *running_mean, float *running_var, int64_t n, int lane,
                                               float &mu, float &is) {
    const double mean = s / (double)B;
    double var = q / (double)B - mean * mean;
    if (var < 0.0) var = 0.0;
    mu = (float)mean;
    is = (float)(1.0 / sqrt(var + eps));
    if (lane == 0 && running_mean && momentum > 0.0) {
        const double unb = B > 1 ? var * (double)B / (double)(B - 1) : var;
        running_mean[n] = (float)((1.0 - momentum) * (double)running_mean[n] + momentum * mean);
        running_var[n] = (float)((1.0 - momentum) * (double)running_var[n] + momentum * unb);
    }
}

template <bool kOneSlab>
__global__ __launch_bounds__(kFcThreads) void fc_fwd_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W, int64_t ldw,
    const float *__restrict__ bias, int B, int64_t N, int64_t K, double eps, double momentum,
    float *running_mean, float *running_var, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ Y, int64_t ldy, float *__restrict__ A,
    int64_t lda, float *__restrict__ stats, int mode, int relu, bool vecx, bool vecw) {
    __shared__ float4 sx[kFcRows * kFcLdx];
    __shared__ float4 sw[kFcNB * kFcG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * kFcNB;
    const int64_t n = n0 + wave;
    const bool live = n < N;  // wave-uniform; a wave past N still loads and keeps the barriers

    float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f, bi = 0.f;
    auto column_consts = [&] {
        if (!live) return;
        bi = bias[n];
        if (mode != kFcNoBn) ga = gamma[n], be = beta[n];
        if (mode == kFcFrozen) {
            mu = running_mean[n];
            is = (float)(1.0 / sqrt((double)running_var[n] + eps));
        }
    };
    if constexpr (!kOneSlab) column_consts();  // held over the slabs
    auto act = [&](float y) { return mode == kFcNoBn ? bn_relu(y, relu) : bn_act(y, mu, is, ga, be, relu); };

    float y = 0.f;            // one slab: kept from the GEMM to the activation
    double s = 0.0, q = 0.0;  // the column's float64 sums, carried over the slabs in row order
    for (int r0 = 0; r0 < (kOneSlab ? 1 : B); r0 += kFcRows) {
        const int rows = kOneSlab || B - r0 < kFcRows ? B - r0 : kFcRows;
        const float acc = fc_slab_dot(X + (int64_t)r0 * ldx, ldx, rows, W, ldw, n0, N, K, vecx, vecw, sx, sw);
        if constexpr (kOneSlab) column_consts();  // one slab: not held over the K loop
        y = acc + bi;
        if (live) {
            const int64_t r = (int64_t)r0 + lane;
            if (lane < rows) Y[r * ldy + n] = y;
            if (mode == kFcBatch) {
                for (int t = 0; t < rows; ++t) {  // ascending rows, every lane the same walk
                    const double v = (double)fc_lane(y, t);
                    s += v;
                    q += v * v;
                }
            } else if (lane < rows) {
                A[r * lda + n] = act(y);
            }
        }
    }
    if (!live || mode == kFcNoBn) return;  // no barrier from here on

    if (mode == kFcBatch) fc_batch_stats(s, q, B, eps, momentum, running_mean, running_var, n, lane, mu, is);
    if (lane == 0) stats[n] = mu, stats[N + n] = is;
    if (mode == kFcBatch) {  // the column's statistics are known only now
        if constexpr (kOneSlab) {
            if (lane < B) A[(int64_t)lane * lda + n] = act(y);
        } else {
            // each thread reads back the Y elements it stored itself (same thread, same address:
            // program order)
            for (int64_t r = lane; r < B; r += kFcRows) A[r * lda + n] = act(Y[r * ldy + n]);
        }
    }
}

template <bool kOneSlab>
__global__ __launch_bounds__(kFcThreads) void fc_bwd_kernel(
    const float *__restrict__ dA, int64_t ldd, const float *__restrict__ Y, int64_t ldy,
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ stats,
    const float *__restrict__ gamma, const float *__restrict__ beta, int B, int64_t N, int64_t K,
    float *__restrict__ dY, int64_t ldyy, float *__restrict__ dW, int64_t ldw,
    float *__restrict__ dbias, float *__restrict__ dgamma, float *__restrict__ dbeta, int mode,
    int relu, bool vecx, bool vecdw) {
    __shared__ float4 sdy[kFcRows];  // dY[slab row][the block's 4 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * kFcNB;
    const int64_t n = n0 + wave;
    const bool live = n < N;             // wave-uniform
    const int Bs = kOneSlab ? 1 : B;     // the slab loops' bound: one trip at compile time
    auto slab_rows = [&](int r0) { return kOneSlab || B - r0 < kFcRows ? B - r0 : kFcRows; };

    float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f, m1 = 0.f, m2 = 0.f;
    float dd = 0.f, y = 0.f;  // this lane's dXn and Y of the current slab
    // dXn of this lane's row of the slab at r0 (0 in a lane past the slab), and the row's Y
    auto load_dxn = [&](int r0, int rows) {
        const bool in = lane < rows;
        const int64_t r = (int64_t)r0 + lane;
        const float d = in ? dA[r * ldd + n] : 0.f;
        y = in ? Y[r * ldy + n] : 0.f;
        dd = mode == kFcNoBn ? bn_gate(y, d, relu) : bn_dxn(bn_xhat(y, mu, is), ga, be, d, relu);
    };

    if (live && mode != kFcNoBn) {  // sweep 1: dbeta, dgamma
        mu = stats[n], is = stats[N + n], ga = gamma[n], be = beta[n];
        double s1 = 0.0, s2 = 0.0;
        for (int r0 = 0; r0 < Bs; r0 += kFcRows) {
            const int rows = slab_rows(r0);
            load_dxn(r0, rows);
            for (int t = 0; t < rows; ++t) {
                const double dr = (double)fc_lane(dd, t);
                s1 += dr;
                s2 += dr * bn_xhat64(fc_lane(y, t), mu, is);
            }
        }
        if (lane == 0) dbeta[n] = (float)s1, dgamma[n] = (float)s2;
        if (mode == kFcBatch) m1 = (float)(s1 / (double)B), m2 = (float)(s2 / (double)B);
    }

    // a slab's dY (wave = column, lane = row) into sdy; first: stored, and walked for dbias
    double sb = 0.0;
    auto slab_dy = [&](int r0, int rows, bool first) {
        float dy = 0.f;
        if (live) {
            const bool in = lane < rows;
            // one slab under BN: dd and y are still sweep 1's
            if (!kOneSlab || mode == kFcNoBn) load_dxn(r0, rows);
            if (mode == kFcNoBn)
                dy = dd;
            else if (mode == kFcBatch)
                dy = ga * is * (dd - m1 - bn_xhat(y, mu, is) * m2);
            else
                dy = ga * is * dd;
            if (first) {
                if (in) dY[((int64_t)r0 + lane) * ldyy + n] = dy;
                for (int t = 0; t < rows; ++t) sb += (double)fc_lane(dy, t);
            }
            if (!in) dy = 0.f;
        }
        reinterpret_cast<float *>(sdy)[lane * kFcNB + wave] = dy;
        __syncthreads();
    };
    if constexpr (kOneSlab) slab_dy(0, B, true);  // once: it serves every pass over dW's columns

    // sweep 2, once per 1024 columns of dW: dW[n0 + c][k .. k+3] += dY[r][c] * X[r][k ..] over the
    // slabs' rows in order, one fma a step
    for (int64_t kb = 0; kb < K; kb += kFcThreads * 4) {
        const int64_t k = kb + (int64_t)tid * 4;
        float acc[kFcNB][4];
#pragma unroll
        for (int c = 0; c < kFcNB; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][j] = 0.f;
        for (int r0 = 0; r0 < Bs; r0 += kFcRows) {
            const int rows = slab_rows(r0);
            if constexpr (!kOneSlab) slab_dy(r0, rows, kb == 0);
            if (k < K) {
                const float *__restrict__ Xs = X + (int64_t)r0 * ldx;
#pragma unroll 4
                for (int t = 0; t < rows; ++t) {
                    const float4 x = fc_fetch4(Xs + (int64_t)t * ldx, k, K, vecx);
                    const float4 d4 = sdy[t];
                    const float xs[4] = {x.x, x.y, x.z, x.w}, ds[kFcNB] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int c = 0; c < kFcNB; ++c)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[c][j] = __fmaf_rn(ds[c], xs[j], acc[c][j]);
                }
            }
            if constexpr (!kOneSlab) __syncthreads();  // the slab's sdy is read before the next one is written
        }
        if (k < K) {
#pragma unroll
            for (int c = 0; c < kFcNB; ++c) {
                const int64_t col = n0 + c;
                if (col >= N) break;
                float *o = dW + col * ldw + k;
                if (vecdw && k + 4 <= K) {
                    *reinterpret_cast<float4 *>(o) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) o[j] = acc[c][j];
                }
            }
        }
    }
    if (live && lane == 0) dbias[n] = (float)sb;
}

static inline bool fc_vec(const float *p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

static int fc_mode(const char *what, const float *gamma, int flags, int64_t B, int &mode) {
    if (flags & ~(PN2_LAYER_NO_RELU | PN2_LAYER_FROZEN_STATS))
        return set_error(PN2_EINVAL, "%s: unknown flags %d", what, flags);
    mode = !gamma ? kFcNoBn : (flags & PN2_LAYER_FROZEN_STATS) ? kFcFrozen : kFcBatch;
    if (mode == kFcBatch && B == 1)
        return set_error(PN2_EINVAL, "%s: batch statistics need more than one row (B=1)", what);
    return PN2_OK;
}

static int fc_shape(const char *what, int64_t B, int64_t N, int64_t K, int64_t max_rows) {
    if (B < 1 || N < 1 || K < 1)
        return set_error(PN2_EINVAL, "%s: bad shape B=%lld N=%lld K=%lld", what, (long long)B, (long long)N,
                         (long long)K);
    if (B > max_rows)
        return set_error(PN2_EUNSUPPORTED, "%s: B=%lld above %lld rows", what, (long long)B, (long long)max_rows);
    if ((N + kFcNB - 1) / kFcNB >= (1ll << 31))
        return set_error(PN2_EUNSUPPORTED, "%s: N=%lld too large", what, (long long)N);
    return PN2_OK;
}

// the two forward entries: one validation, the one-slab or the any-B instantiation
static int fc_forward(const char *what, bool any_rows, const float *X, int64_t ldx, const float *W, int64_t ldw,
                      const float *bias, int64_t B, int64_t N, int64_t K, double eps, double momentum,
                      float *running_mean, float *running_var, const float *gamma, const float *beta, float *Y,
                      int64_t ldy, float *A, int64_t lda, float *stats, int flags, void *stream) {
    PN2_REQUIRE(X && W && bias && Y && A, "%s: null pointer", what);
    PN2_REQUIRE(!gamma || (beta && stats), "%s: null pointer (gamma without beta or stats)", what);
    int rc = fc_shape(what, B, N, K, any_rows ? kFcRowsMaxB : kFcRows);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(ldx >= K && ldw >= K && ldy >= N && lda >= N, "%s: a leading dimension is below its matrix width",
                what);
    int mode;
    rc = fc_mode(what, gamma, flags, B, mode);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(mode != kFcFrozen || (running_mean && running_var),
                "%s: null pointer (frozen statistics without running_mean / running_var)", what);
    PN2_REQUIRE(mode != kFcBatch || momentum <= 0.0 || (running_mean && running_var),
                "%s: null pointer (momentum without running_mean / running_var)", what);
    hipLaunchKernelGGL(any_rows ? fc_fwd_kernel<false> : fc_fwd_kernel<true>,
                       dim3((unsigned)((N + kFcNB - 1) / kFcNB)), dim3(kFcThreads), 0, as_stream(stream), X, ldx, W,
                       ldw, bias, (int)B, N, K, eps, momentum, running_mean, running_var, gamma, beta, Y, ldy, A,
                       lda, stats, mode, (flags & PN2_LAYER_NO_RELU) ? 0 : 1, fc_vec(X, ldx), fc_vec(W, ldw));
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

static int fc_backward(const char *what, bool any_rows, const float *dA, int64_t ldd, const float *Y, int64_t ldy,
                       const float *X, int64_t ldx, const float *stats, const float *gamma, const float *beta,
                       int64_t B, int64_t N, int64_t K, float *dY, int64_t ldyy, float *dW, int64_t ldw,
                       float *dbias, float *dgamma, float *dbeta, int flags, void *stream) {
    PN2_REQUIRE(dA && Y && X && dY && dW && dbias, "%s: null pointer", what);
    PN2_REQUIRE(!gamma || (beta && stats && dgamma && dbeta),
                "%s: null pointer (gamma without beta, stats, dgamma or dbeta)", what);
    int rc = fc_shape(what, B, N, K, any_rows ? kFcRowsMaxB : kFcRows);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(ldd >= N && ldy >= N && ldx >= K && ldyy >= N && ldw >= K,
                "%s: a leading dimension is below its matrix width", what);
    int mode;
    rc = fc_mode(what, gamma, flags, B, mode);
    if (rc != PN2_OK) return rc;
    hipLaunchKernelGGL(any_rows ? fc_bwd_kernel<false> : fc_bwd_kernel<true>,
                       dim3((unsigned)((N + kFcNB - 1) / kFcNB)), dim3(kFcThreads), 0, as_stream(stream), dA, ldd, Y,
                       ldy, X, ldx, stats, gamma, beta, (int)B, N, K, dY, ldyy, dW, ldw, dbias, dgamma, dbeta, mode,
                       (flags & PN2_LAYER_NO_RELU) ? 0 : 1, fc_vec(X, ldx), fc_vec(dW, ldw));
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_fc_train_max_rows(void) { return kFcRows; }

extern "C" int pn2_fc_bn_forward_f32(const float *X, int64_t ldx, const float *W, int64_t ldw,
                                     const float *bias, int64_t B, int64_t N, int64_t K, double eps,
                                     double momentum, float *running_mean, float *running_var,
                                     const float *gamma, const float *beta, float *Y, int64_t ldy, float *A,
                                     int64_t lda, float *stats, int flags, void *stream) {
    return fc_forward("pn2_fc_bn_forward_f32", false, X, ldx, W, ldw, bias, B, N, K, eps, momentum, running_mean,
                      running_var, gamma, beta, Y, ldy, A, lda, stats, flags, stream);
}

extern "C" int pn2_fc_bn_forward_rows_f32(const float *X, int64_t ldx, const float *W, int64_t ldw,
                                          const float *bias, int64_t B, int64_t N, int64_t K, double eps,
                                          double momentum, float *running_mean, float *running_var,
                                          const float *gamma, const float *beta, float *Y, int64_t ldy,
                                          float *A, int64_t lda, float *stats, int flags, void *stream) {
    return fc_forward("pn2_fc_bn_forward_rows_f32", true, X, ldx, W, ldw, bias, B, N, K, eps, momentum,
                      running_mean, running_var, gamma, beta, Y, ldy, A, lda, stats, flags, stream);
}

extern "C" int pn2_fc_bn_backward_f32(const float *dA, int64_t ldd, const float *Y, int64_t ldy,
                                      const float *X, int64_t ldx, const float *stats, const float *gamma,
                                      const float *beta, int64_t B, int64_t N, int64_t K, float *dY,
                                      int64_t ldyy, float *dW, int64_t ldw, float *dbias, float *dgamma,
                                      float *dbeta, int flags, void *stream) {
    return fc_backward("pn2_fc_bn_backward_f32", false, dA, ldd, Y, ldy, X, ldx, stats, gamma, beta, B, N, K, dY,
                       ldyy, dW, ldw, dbias, dgamma, dbeta, flags, stream);
}

extern "C" int pn2_fc_bn_backward_rows_f32(const float *dA, int64_t ldd, const float *Y, int64_t ldy,
                                           const float *X, int64_t ldx, const float *stats, const float *gamma,
                                           const float *beta, int64_t B, int64_t N, int64_t K, float *dY,
                                           int64_t ldyy, float *dW, int64_t ldw, float *dbias, float *dgamma,
                                           float *dbeta, int flags, void *stream) {
    return fc_backward("pn2_fc_bn_backward_rows_f32", true, dA, ldd, Y, ldy, X, ldx, stats, gamma, beta, B, N, K,
                       dY, ldyy, dW, ldw, dbias, dgamma, dbeta, flags, stream);
}
