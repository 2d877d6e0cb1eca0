// knn.hip -- delet_outlier_statistical of the reference's capture scripts
// (point_collect/collect.py:80-90), for gfx950: Open3D's RemoveStatisticalOutliers with its kd-tree
// replaced by exact brute-force arithmetic.  The rule is stated in include/pn2.h ("statistical
// outlier removal", S1 to S5); the mean distances are float64 values whose every operation is
// fixed, so parity with the numpy restatement is bit for bit.
//
// Three kernels:
//   * knn_pack_kernel: columns 0..2 of the rows, widened to float64, as three arrays in the
//     workspace; a row with a non-finite coordinate becomes three NaNs (it is no candidate and no
//     query).  The selection kernel is then the same for both input types and strides.
//   * knn_mean_kernel<QW>: tiled brute force over (query, candidate) pairs.  A workgroup stages the
//     candidates through LDS as collect_pair_kernel does; each of its four waves owns QW queries.
//     Per step a lane takes one candidate and computes d2 to each of the wave's queries; a ballot
//     finds the lanes below the query's bound (its k-th smallest d2 so far) and only those append
//     to the query's LDS buffer of kPool / (4 * QW) >= 2k doubles.  A buffer that could not take
//     another 64 is bitonic-sorted by its wave and cut to the k smallest, which tightens the
//     bound.  At the end the survivors are sorted, their square roots taken, and the ascending
//     chain added.  No atomics; no wave waits for another outside the tile barriers.
//   * stat_flags_kernel: S4 and S5 in one workgroup.  The two sums are serial float64 chains by
//     definition: all threads stage `mean` (and the squared deviations) through LDS, thread 0 adds.
#include "collect_common.h"

namespace pn2 {

constexpr int kKnnMaxK = 256;
constexpr int kKnnThreads = 256;             // four waves
constexpr int kKnnTile = 1024;               // candidates per LDS tile: 3 x 8 KiB
constexpr int kKnnPool = 4096;               // doubles of selection buffers per workgroup: 32 KiB
constexpr int kStatThreads = 1024;
constexpr int kStatChunk = 2048;             // doubles per staged chunk, two chunks in LDS

// lanes of one wave exchange values through LDS: the hardware keeps a wave's LDS operations in
// order, so only the compiler has to be kept from moving them
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending bitonic sort of buf[0 .. P), P a power of two >= 2, by one wave
__device__ __forceinline__ void wave_sort(double *buf, int P, int lane) {
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const double a = buf[i], b = buf[j];
                if ((a > b) == up) buf[i] = b, buf[j] = a;
            }
            wave_lds_sync();
        }
    }
}

__device__ __forceinline__ void wave_pad(double *buf, int from, int to, int lane) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int t = from + lane; t < to; t += 64) buf[t] = inf;
    wave_lds_sync();
}

__device__ __forceinline__ bool finite3(double x, double y, double z) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    return fabs(x) < inf && fabs(y) < inf && fabs(z) < inf;  // a NaN fails
}

template <typename T>
__global__ void knn_pack_kernel(const T *__restrict__ pts, int64_t ld, int n, double *__restrict__ px,
                                double *__restrict__ py, double *__restrict__ pz) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    load_xyz(pts, ld, i, x, y, z);
    if (!finite3(x, y, z)) x = y = z = __longlong_as_double(0x7ff8000000000000ll);
    px[i] = x, py[i] = y, pz[i] = z;
}

template <int QW>
__global__ __launch_bounds__(kKnnThreads) void knn_mean_kernel(const double *__restrict__ px,
                                                               const double *__restrict__ py,
                                                               const double *__restrict__ pz, int n, int k,
                                                               double *__restrict__ mean) {
    constexpr int CAP = kKnnPool / (4 * QW);  // doubles per query; the host sees to 2k <= CAP, so k + 64 <= CAP
    static_assert(CAP >= 128 && (CAP & (CAP - 1)) == 0, "a power of two that holds k + 64 whenever it holds 2k");
    __shared__ double sx[kKnnTile], sy[kKnnTile], sz[kKnnTile];
    __shared__ double pool[kKnnPool];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int qi[QW], cnt[QW];
    double qx[QW], qy[QW], qz[QW], bound[QW];
    double *buf[QW];
#pragma unroll
    for (int q = 0; q < QW; ++q) {
        qi[q] = (blockIdx.x * 4 + wave) * QW + q;
        buf[q] = pool + (wave * QW + q) * CAP;
        cnt[q] = 0;
        // a NaN bound takes every candidate; 0 takes none (d2 >= 0): a slot past n, a non-finite row
        qx[q] = qy[q] = qz[q] = 0.0, bound[q] = 0.0;
        if (qi[q] < n) {
            const double x = px[qi[q]];
            if (x == x) qx[q] = x, qy[q] = py[qi[q]], qz[q] = pz[qi[q]], bound[q] = nan;
        }
    }
    for (int c0 = 0; c0 < n; c0 += kKnnTile) {
        const int tlen = min(kKnnTile, n - c0);
        for (int i = tid; i < tlen; i += kKnnThreads) sx[i] = px[c0 + i], sy[i] = py[c0 + i], sz[i] = pz[c0 + i];
        __syncthreads();
        for (int s0 = 0; s0 < tlen; s0 += 64) {
            const int ci = s0 + lane;  // < kKnnTile: s0 is a multiple of 64 below tlen
            const double cx = sx[ci], cy = sy[ci], cz = sz[ci];
            const bool ok = ci < tlen && cx == cx;
#pragma unroll
            for (int q = 0; q < QW; ++q) {
                const double d2 = nbr_d2(qx[q], qy[q], qz[q], cx, cy, cz);
                const bool take = ok && !(d2 >= bound[q]);
                const unsigned long long m = __ballot(take);
                if (m) {  // wave-uniform
                    if (take) buf[q][cnt[q] + __popcll(m & ((1ull << lane) - 1ull))] = d2;
                    cnt[q] += __popcll(m);  // <= CAP: it was <= CAP - 64
                    if (cnt[q] + 64 > CAP) {
                        wave_pad(buf[q], cnt[q], CAP, lane);
                        wave_sort(buf[q], CAP, lane);
                        cnt[q] = k;  // CAP - 64 >= k
                        bound[q] = buf[q][k - 1];
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < QW; ++q) {
        if (qi[q] >= n) continue;  // wave-uniform
        if (cnt[q] == 0) {         // a non-finite row (a finite one holds itself)
            if (lane == 0) mean[qi[q]] = -1.0;
            continue;
        }
        int P = 2;
        while (P < cnt[q]) P <<= 1;
        wave_pad(buf[q], cnt[q], P, lane);
        wave_sort(buf[q], P, lane);
        const int m = min(cnt[q], k);  // k_eff
        for (int t = lane; t < m; t += 64) buf[q][t] = __dsqrt_rn(buf[q][t]);
        wave_lds_sync();
        double s = 0.0;
        for (int t = 0; t < m; ++t) s = s + buf[q][t];  // every lane the same chain: a broadcast
        if (lane == 0) mean[qi[q]] = s / (double)m;
    }
}

// stats = {cloud_mean, std, threshold, valid}; flags[i] = mean[i] > 0 && mean[i] < threshold
__global__ __launch_bounds__(kStatThreads) void stat_flags_kernel(const double *__restrict__ mean, int n,
                                                                  double std_ratio, int *__restrict__ flags,
                                                                  double *__restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double stage[2][kStatChunk];
    __shared__ double s_cm, s_thr;
    __shared__ int s_valid[kStatThreads / 64];
    const int tid = threadIdx.x;
    const int nchunks = (n + kStatChunk - 1) / kStatChunk;
    int valid = 0;
    double cm = 0.0, acc = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
        acc = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            double *st = stage[c & 1];
            const int len = min(kStatChunk, n - c * kStatChunk);
            for (int t = tid; t < len; t += kStatThreads) {
                const double m = mean[c * kStatChunk + t];
                if (pass == 0) valid += m >= 0.0 ? 1 : 0;  // a non-finite row carries -1
                const double d = m - cm;
                st[t] = m > 0.0 ? (pass == 0 ? m : d * d) : 0.0;  // + 0.0 leaves a sum >= 0 as it is
            }
            // one barrier per chunk: the others fill the second half while thread 0 adds this one
            __syncthreads();
            if (tid == 0) {
#pragma unroll 8
                for (int t = 0; t < len; ++t) acc = acc + st[t];
            }
        }
        if (pass == 0) {
            int v = valid;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((tid & 63) == 0) s_valid[tid >> 6] = v;
            __syncthreads();
            if (tid == 0) {
                int total = 0;
                for (int w = 0; w < kStatThreads / 64; ++w) total += s_valid[w];
                s_valid[0] = total;
                s_cm = acc / (double)total;
            }
            __syncthreads();
            cm = s_cm;
        }
    }
    if (tid == 0) {
        const double v = (double)s_valid[0];
        const double sd = __dsqrt_rn(acc / (v - 1.0));
        const double thr = cm + std_ratio * sd;
        stats[0] = cm, stats[1] = sd, stats[2] = thr, stats[3] = v;
        s_thr = thr;
    }
    __syncthreads();
    const double thr = s_thr;
    for (int i = tid; i < n; i += kStatThreads) {
        const double m = mean[i];
        flags[i] = (m > 0.0 && m < thr) ? 1 : 0;
    }
}

static int64_t knn_ws_bytes(int64_t N) { return 3 * align16(N * 8); }

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_knn_max_k(void) { return kKnnMaxK; }

extern "C" int64_t pn2_knn_mean_dist_workspace_bytes(int64_t N, int64_t k) {
    if (N < 0 || N > kCollectMaxN || k < 1 || k > kKnnMaxK) return -1;
    return knn_ws_bytes(N);
}

extern "C" int pn2_knn_mean_dist_f64(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, int64_t k,
                                     double *mean, void *workspace, int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && mean, "pn2_knn_mean_dist_f64: null pointer");
    const int rc = check_cloud("pn2_knn_mean_dist_f64", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(k >= 1, "pn2_knn_mean_dist_f64: nb_neighbors = %lld, needs >= 1", (long long)k);
    if (k > kKnnMaxK)
        return set_error(PN2_EUNSUPPORTED, "pn2_knn_mean_dist_f64: nb_neighbors = %lld above pn2_knn_max_k() = %d",
                         (long long)k, kKnnMaxK);
    if (N == 0) return PN2_OK;
    const int64_t need = knn_ws_bytes(N);
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_knn_mean_dist_f64: workspace too small: needs pn2_knn_mean_dist_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    hipStream_t st = as_stream(stream);
    double *px = static_cast<double *>(workspace);
    double *py = px + align16(N * 8) / 8, *pz = py + align16(N * 8) / 8;
    const dim3 pgrid((unsigned)((N + 255) / 256));
    if (dtype == PN2_DTYPE_F64)
        hipLaunchKernelGGL(knn_pack_kernel<double>, pgrid, dim3(256), 0, st, static_cast<const double *>(pts), ld,
                           (int)N, px, py, pz);
    else
        hipLaunchKernelGGL(knn_pack_kernel<float>, pgrid, dim3(256), 0, st, static_cast<const float *>(pts), ld,
                           (int)N, px, py, pz);
    PN2_LAUNCH_CHECK("knn_pack_kernel");
    // the widest query set whose buffers hold 2k: 16 queries per workgroup up to k = 128, else 8
    if (2 * k <= kKnnPool / 16)
        hipLaunchKernelGGL(knn_mean_kernel<4>, dim3((unsigned)((N + 15) / 16)), dim3(kKnnThreads), 0, st, px, py, pz,
                           (int)N, (int)k, mean);
    else
        hipLaunchKernelGGL(knn_mean_kernel<2>, dim3((unsigned)((N + 7) / 8)), dim3(kKnnThreads), 0, st, px, py, pz,
                           (int)N, (int)k, mean);
    PN2_LAUNCH_CHECK("knn_mean_kernel");
    return PN2_OK;
}

extern "C" int pn2_stat_outlier_flags(const double *mean, int64_t N, double std_ratio, int32_t *flags, double *stats,
                                      void *stream) {
    PN2_REQUIRE(mean && flags && stats, "pn2_stat_outlier_flags: null pointer");
    PN2_REQUIRE(N >= 0, "pn2_stat_outlier_flags: bad shape (N=%lld)", (long long)N);
    if (N > kCollectMaxN)
        return set_error(PN2_EUNSUPPORTED, "pn2_stat_outlier_flags: N=%lld above pn2_collect_max_points() = %lld",
                         (long long)N, (long long)kCollectMaxN);
    PN2_REQUIRE(std_ratio > 0.0, "pn2_stat_outlier_flags: std_ratio = %g, needs > 0", std_ratio);
    if (N == 0) return PN2_OK;
    hipLaunchKernelGGL(stat_flags_kernel, dim3(1), dim3(kStatThreads), 0, as_stream(stream), mean, (int)N, std_ratio,
                       flags, stats);
    PN2_LAUNCH_CHECK("stat_flags_kernel");
    return PN2_OK;
}
