// fc_train.hip -- a heads' fully connected layer under autograd, one launch each way
// (include/pn2.h states the contracts and the order rules):
//   pn2_fc_bn_forward_f32    Y = X W^T + b, the BatchNorm1d column statistics of Y (batch or
//                            running), the running-stat update, A = act(bn(Y))
//   pn2_fc_bn_backward_f32   dXn = dA * [A > 0], dbeta, dgamma, dY, dbias = sum_r dY,
//                            dW = dY^T X
//
// Reference: fc1/bn1/relu, fc2/bn2/relu, fc3 of the heads under the training loops' autograd,
// /root/reference/model/pointnet2_cls_ssg.py:31-36, rotation_ssg.py:33-37,
// translation_ssg.py:23-26 (the mean MLP), pointnet_utils.py:33-40 (the T-Nets' FC tail)
// (pn2/train.py _FcBnTrain).
//
// The whole batch (B <= kFcRows = 64 rows) fits one workgroup, so a workgroup that owns a block
// of kFcNB = 4 output columns owns every row of them: no workspace, no second pass, no sum
// across workgroups.  256 threads = 4 waves.
//
// Forward: wave w owns column n0 + w, lane r row r (one accumulator per thread; lanes past B
// compute row 0 again and store nothing).  X ([B][64] floats) and the 4 W rows ([4][64]) go
// through LDS in K-chunks of 64: 16-byte loads where base and leading dimension allow, dword
// loads else and in a chunk's ragged last group, zeros past K with no load issued; the next
// chunk's loads are issued before the current chunk's FMAs.  An X row is 68 floats apart in
// LDS: the ds_read_b128 of 16 consecutive rows fall on 16 distinct 16-byte slots.  The W reads
// are wave-uniform (broadcast).  The element's sum is ONE fma chain over ascending k from +0
// (__fmaf_rn), then one add of the bias: the order is a function of K alone.  The column
// statistics are a serial float64 walk over v_readlane of rows 0 .. B-1, done by every lane of
// the wave alike: each lane then holds its column's mean / invstd without LDS or a barrier.
//
// Backward: phase 1 has the forward's mapping (wave = column, lane = row): dXn, the float64
// walks for dbeta / dgamma, dY (stored, and kept in LDS as [row][4 columns]), the walk for
// dbias.  Phase 2: thread t owns the 4 consecutive k = 4t .. 4t+3 (+ 1024 per pass) of all 4
// columns' dW rows: for r = 0 .. B-1 in order, one 16-byte load of X[r][k..k+3] (coalesced; X is
// B*K*4 <= 256 KB, L2-resident), one broadcast ds_read_b128 of dY[r][0..3], 16 __fmaf_rn.  X is
// read once per workgroup.
//
// Any B (pn2_fc_bn_forward_rows_f32 / pn2_fc_bn_backward_rows_f32): the same workgroup, the same
// mapping and the same expressions, with the rows walked in slabs of kFcRows.  A workgroup still
// owns every row of its 4 columns, so a column's sum never leaves its wave: the float64
// accumulators are carried from slab to slab in row order, the dW accumulators stay in their
// thread's registers over all slabs.  Forward: per slab the K loop above (the slab's X chunk and
// the 4 W rows' chunk through LDS; the W chunk is 1/16 of the X chunk's bytes, so it is fetched
// again per slab instead of K-sized LDS), Y stored, s / q walked; with batch statistics the
// activation needs the whole column's mean, so a second sweep reads each thread's own Y
// elements back and writes A (frozen / no BN: A in the first sweep).  Backward: sweep 1 walks
// dbeta / dgamma over all slabs; sweep 2 computes a slab's dY (dA and Y read a second time, dXn
// by the same expression), stores it, walks dbias, hands the slab's [row][4 columns] to phase 2
// through the same 1 KB of LDS, and phase 2 continues its fma chains over the slab's rows.
// K > 1024 takes sweep 2 once per 1024 columns of dW (dY and dbias in the first only).  For
// B <= kFcRows every operation and its order are the one-slab kernels': the same bits.
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile): an fma is only where
// __fmaf_rn says so; every other float operation rounds on its own, as in train.hip, whose
// expressions for xhat, the activation and dY these kernels repeat.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kFcRows = 64;            // largest B: a row per lane (pn2_fc_train_max_rows)
constexpr int kFcNB = 4;               // output columns per workgroup: a column per wave
constexpr int kFcKC = 64;              // K chunk through LDS
constexpr int kFcG = kFcKC / 4;        // 16-byte groups per chunk row
constexpr int kFcLdx = kFcG + 1;       // LDS stride of an X row, in 16-byte slots (68 floats)
constexpr int kFcThreads = 256;
constexpr int kFcXI = kFcRows * kFcG / kFcThreads;  // X groups per thread and chunk (4)
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

__device__ __forceinline__ float fc_xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }

__global__ __launch_bounds__(kFcThreads) void fc_fwd_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W, int64_t ldw,
    const float *__restrict__ bias, int B, int64_t N, int64_t K, double eps, double momentum,
    float *running_mean, float *running_var, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ Y, int64_t ldy, float *__restrict__ A,
    int64_t lda, float *__restrict__ stats, int mode, int relu, bool vecx, bool vecw) {
    __shared__ float4 sx[kFcRows * kFcLdx];
    __shared__ float4 sw[kFcNB * kFcG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * kFcNB;
    const int items = B * kFcG;  // (row, group) pairs of an X chunk

    float4 fx[kFcXI], fw;
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int q = 0; q < kFcXI; ++q) {
            const int i = tid + q * kFcThreads;
            if (i < items) fx[q] = fc_fetch4(X + (int64_t)(i / kFcG) * ldx, k0 + (i % kFcG) * 4, K, vecx);
        }
        if (tid < kFcNB * kFcG) {
            const int64_t n = n0 + tid / kFcG;
            fw = n < N ? fc_fetch4(W + n * ldw, k0 + (tid % kFcG) * 4, K, vecw) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    fetch(0);

    float acc = 0.f;
    const int rr = lane < B ? lane : 0;
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

    const int64_t n = n0 + wave;  // wave-uniform
    if (n >= N) return;
    const float y = acc + bias[n];
    if (lane < B) Y[(int64_t)lane * ldy + n] = y;
    float a = y;
    if (mode != kFcNoBn) {
        float mu, is;
        if (mode == kFcBatch) {
            double s = 0.0, q = 0.0;
            for (int r = 0; r < B; ++r) {  // ascending rows, every lane the same walk
                const double v = (double)fc_lane(y, r);
                s += v;
                q += v * v;
            }
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
        } else {
            mu = running_mean[n];
            is = (float)(1.0 / sqrt((double)running_var[n] + eps));
        }
        if (lane == 0) stats[n] = mu, stats[N + n] = is;
        a = fc_xhat(y, mu, is) * gamma[n] + beta[n];
    }
    if (relu) a = a > 0.f ? a : 0.f;
    if (lane < B) A[(int64_t)lane * lda + n] = a;
}

__global__ __launch_bounds__(kFcThreads) void fc_bwd_kernel(
    const float *__restrict__ dA, int64_t ldd, const float *__restrict__ Y, int64_t ldy,
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ stats,
    const float *__restrict__ gamma, const float *__restrict__ beta, int B, int64_t N, int64_t K,
    float *__restrict__ dY, int64_t ldyy, float *__restrict__ dW, int64_t ldw,
    float *__restrict__ dbias, float *__restrict__ dgamma, float *__restrict__ dbeta, int mode,
    int relu, bool vecx, bool vecdw) {
    __shared__ float4 sdy[kFcRows];  // dY[row][the block's 4 columns]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * kFcNB;

    {  // phase 1: wave = column, lane = row
        const int64_t n = n0 + wave;
        float dy = 0.f;
        if (n < N) {  // wave-uniform
            const bool in = lane < B;
            const float d = in ? dA[(int64_t)lane * ldd + n] : 0.f;
            const float y = in ? Y[(int64_t)lane * ldy + n] : 0.f;
            if (mode == kFcNoBn) {
                dy = !relu || y > 0.f ? d : 0.f;
            } else {
                const float mu = stats[n], is = stats[N + n], ga = gamma[n], be = beta[n];
                const float xh = fc_xhat(y, mu, is);
                const float dd = !relu || xh * ga + be > 0.f ? d : 0.f;  // dXn
                double s1 = 0.0, s2 = 0.0;
                for (int r = 0; r < B; ++r) {
                    const double dr = (double)fc_lane(dd, r);
                    s1 += dr;
                    s2 += dr * (((double)fc_lane(y, r) - (double)mu) * (double)is);
                }
                if (lane == 0) dbeta[n] = (float)s1, dgamma[n] = (float)s2;
                if (mode == kFcBatch) {
                    const float m1 = (float)(s1 / (double)B), m2 = (float)(s2 / (double)B);
                    dy = ga * is * (dd - m1 - xh * m2);
                } else {
                    dy = ga * is * dd;
                }
            }
            if (in) dY[(int64_t)lane * ldyy + n] = dy;
            double sb = 0.0;
            for (int r = 0; r < B; ++r) sb += (double)fc_lane(dy, r);
            if (lane == 0) dbias[n] = (float)sb;
            if (!in) dy = 0.f;
        }
        reinterpret_cast<float *>(sdy)[lane * kFcNB + wave] = dy;
    }
    __syncthreads();

    // phase 2: dW[n0 + c][k .. k+3] = sum over ascending r of dY[r][c] * X[r][k ..], one fma a step
    for (int64_t k = (int64_t)tid * 4; k < K; k += kFcThreads * 4) {
        float acc[kFcNB][4];
#pragma unroll
        for (int c = 0; c < kFcNB; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][j] = 0.f;
#pragma unroll 4
        for (int r = 0; r < B; ++r) {
            const float4 x = fc_fetch4(X + (int64_t)r * ldx, k, K, vecx);
            const float4 d4 = sdy[r];
            const float xs[4] = {x.x, x.y, x.z, x.w}, ds[kFcNB] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int c = 0; c < kFcNB; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[c][j] = __fmaf_rn(ds[c], xs[j], acc[c][j]);
        }
#pragma unroll
        for (int c = 0; c < kFcNB; ++c) {
            const int64_t n = n0 + c;
            if (n >= N) break;
            float *o = dW + n * ldw + k;
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

// ---- any B: the kernels above over slabs of kFcRows rows (the file comment has the scheme)
constexpr int64_t kFcRowsMaxB = 1ll << 30;  // the slab loop's int row counter stays below 2^31

__global__ __launch_bounds__(kFcThreads) void fc_rows_fwd_kernel(
    const float *__restrict__ X, int64_t ldx, const float *__restrict__ W, int64_t ldw,
    const float *__restrict__ bias, int B, int64_t N, int64_t K, double eps, double momentum,
    float *running_mean, float *running_var, const float *__restrict__ gamma,
    const float *__restrict__ beta, float *__restrict__ Y, int64_t ldy, float *__restrict__ A,
    int64_t lda, float *__restrict__ stats, int mode, int relu, bool vecx, bool vecw) {
    __shared__ float4 sx[kFcRows * kFcLdx];
    __shared__ float4 sw[kFcNB * kFcG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * kFcNB;
    const int64_t n = n0 + wave;
    const bool live = n < N;  // wave-uniform; a wave past N still loads and keeps the barriers

    float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f, bi = 0.f;
    if (live) {
        bi = bias[n];
        if (mode != kFcNoBn) ga = gamma[n], be = beta[n];
        if (mode == kFcFrozen) {
            mu = running_mean[n];
            is = (float)(1.0 / sqrt((double)running_var[n] + eps));
        }
    }
    auto act = [&](float y) {
        float a = y;
        if (mode != kFcNoBn) a = fc_xhat(y, mu, is) * ga + be;
        if (relu) a = a > 0.f ? a : 0.f;
        return a;
    };

    double s = 0.0, q = 0.0;  // the column's float64 sums, carried over the slabs in row order
    for (int r0 = 0; r0 < B; r0 += kFcRows) {
        const int rows = B - r0 < kFcRows ? B - r0 : kFcRows;
        const float *__restrict__ Xs = X + (int64_t)r0 * ldx;
        const int items = rows * kFcG;  // (row, group) pairs of the slab's X chunk

        float4 fx[kFcXI], fw;
        auto fetch = [&](int64_t k0) {
#pragma unroll
            for (int j = 0; j < kFcXI; ++j) {
                const int i = tid + j * kFcThreads;
                if (i < items) fx[j] = fc_fetch4(Xs + (int64_t)(i / kFcG) * ldx, k0 + (i % kFcG) * 4, K, vecx);
            }
            if (tid < kFcNB * kFcG) {
                const int64_t c = n0 + tid / kFcG;
                fw = c < N ? fc_fetch4(W + c * ldw, k0 + (tid % kFcG) * 4, K, vecw) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        fetch(0);

        float acc = 0.f;
        const int rr = lane < rows ? lane : 0;
        for (int64_t k0 = 0; k0 < K; k0 += kFcKC) {
#pragma unroll
            for (int j = 0; j < kFcXI; ++j) {
                const int i = tid + j * kFcThreads;
                if (i < items) sx[(i / kFcG) * kFcLdx + i % kFcG] = fx[j];
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

        if (live) {
            const float y = acc + bi;
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

    if (mode == kFcBatch) {
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
    if (lane == 0) stats[n] = mu, stats[N + n] = is;
    if (mode == kFcBatch) {
        // the column's statistics are known only now: each thread reads back the Y elements it
        // stored itself (same thread, same address: program order) and writes their activation
        for (int64_t r = lane; r < B; r += kFcRows) A[r * lda + n] = act(Y[r * ldy + n]);
    }
}

__global__ __launch_bounds__(kFcThreads) void fc_rows_bwd_kernel(
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
    const bool live = n < N;  // wave-uniform

    float mu = 0.f, is = 0.f, ga = 0.f, be = 0.f, m1 = 0.f, m2 = 0.f;
    // dXn of this lane's row of the slab at r0 (0 in a lane past the slab), and the row's Y
    auto dxn = [&](int r0, int rows, float &y) {
        const bool in = lane < rows;
        const int64_t r = (int64_t)r0 + lane;
        const float d = in ? dA[r * ldd + n] : 0.f;
        y = in ? Y[r * ldy + n] : 0.f;
        if (mode == kFcNoBn) return !relu || y > 0.f ? d : 0.f;
        return !relu || fc_xhat(y, mu, is) * ga + be > 0.f ? d : 0.f;
    };

    if (live && mode != kFcNoBn) {  // sweep 1: dbeta, dgamma
        mu = stats[n], is = stats[N + n], ga = gamma[n], be = beta[n];
        double s1 = 0.0, s2 = 0.0;
        for (int r0 = 0; r0 < B; r0 += kFcRows) {
            const int rows = B - r0 < kFcRows ? B - r0 : kFcRows;
            float y;
            const float dd = dxn(r0, rows, y);
            for (int t = 0; t < rows; ++t) {
                const double dr = (double)fc_lane(dd, t);
                s1 += dr;
                s2 += dr * (((double)fc_lane(y, t) - (double)mu) * (double)is);
            }
        }
        if (lane == 0) dbeta[n] = (float)s1, dgamma[n] = (float)s2;
        if (mode == kFcBatch) m1 = (float)(s1 / (double)B), m2 = (float)(s2 / (double)B);
    }

    // sweep 2, once per 1024 columns of dW: a slab's dY (wave = column, lane = row), then the
    // slab's rows of dW[n0 + c][k .. k+3] += dY[r][c] * X[r][k ..], one fma a step
    double sb = 0.0;
    for (int64_t kb = 0; kb < K; kb += kFcThreads * 4) {
        const int64_t k = kb + (int64_t)tid * 4;
        float acc[kFcNB][4];
#pragma unroll
        for (int c = 0; c < kFcNB; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[c][j] = 0.f;
        for (int r0 = 0; r0 < B; r0 += kFcRows) {
            const int rows = B - r0 < kFcRows ? B - r0 : kFcRows;
            float dy = 0.f;
            if (live) {
                const bool in = lane < rows;
                float y;
                const float dd = dxn(r0, rows, y);
                if (mode == kFcNoBn)
                    dy = dd;
                else if (mode == kFcBatch)
                    dy = ga * is * (dd - m1 - fc_xhat(y, mu, is) * m2);
                else
                    dy = ga * is * dd;
                if (kb == 0) {
                    if (in) dY[((int64_t)r0 + lane) * ldyy + n] = dy;
                    for (int t = 0; t < rows; ++t) sb += (double)fc_lane(dy, t);
                }
                if (!in) dy = 0.f;
            }
            reinterpret_cast<float *>(sdy)[lane * kFcNB + wave] = dy;
            __syncthreads();
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
            __syncthreads();  // the slab's sdy is read before the next one is written
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

// the two forward entries: one validation, the one-slab kernel or the slab loop
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
    hipLaunchKernelGGL(any_rows ? fc_rows_fwd_kernel : fc_fwd_kernel, dim3((unsigned)((N + kFcNB - 1) / kFcNB)),
                       dim3(kFcThreads), 0, as_stream(stream), X, ldx, W, ldw, bias, (int)B, N, K, eps, momentum,
                       running_mean, running_var, gamma, beta, Y, ldy, A, lda, stats, mode,
                       (flags & PN2_LAYER_NO_RELU) ? 0 : 1, fc_vec(X, ldx), fc_vec(W, ldw));
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
    hipLaunchKernelGGL(any_rows ? fc_rows_bwd_kernel : fc_bwd_kernel, dim3((unsigned)((N + kFcNB - 1) / kFcNB)),
                       dim3(kFcThreads), 0, as_stream(stream), dA, ldd, Y, ldy, X, ldx, stats, gamma, beta, (int)B,
                       N, K, dY, ldyy, dW, ldw, dbias, dgamma, dbeta, mode, (flags & PN2_LAYER_NO_RELU) ? 0 : 1,
                       fc_vec(X, ldx), fc_vec(dW, ldw));
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
