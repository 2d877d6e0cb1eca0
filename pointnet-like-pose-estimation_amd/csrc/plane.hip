// plane.hip -- delete_plane of the reference's capture scripts (point_collect/collect.py:6-28),
// for gfx950: Open3D's segment_plane (RANSAC) with the draws made an input.  The rule is stated
// in include/pn2.h ("plane segmentation", P1 to P7); everything after the draws is float64
// arithmetic whose every operation and order is fixed, so parity with the numpy restatement is
// bit for bit.
//
// pn2_plane_segment is four launches:
//   * plane_fit_kernel: thread i < N widens row i to float64 into the workspace (the later
//     kernels are then the same for both input types and strides); thread m < M gathers the n
//     rows of hypothesis m from the input and applies P2 / P3.  A skipped hypothesis (zero plane,
//     index out of range) is stored as a NaN plane: every distance to it is NaN, no point is an
//     inlier, its count and err are 0 without a branch in the score kernel.
//   * plane_score_kernel: the hot path.  A workgroup owns one chunk of PN2_PLANE_CHUNK rows,
//     staged in LDS as separate x, y, z arrays, and kScoreHyps hypotheses, kScoreH per thread in
//     registers.  Every lane reads the same row (a broadcast, no bank conflict) and walks the
//     chunk in index order: each thread's count and err chain is P4's chunk sum as it stands.  No
//     cross-lane float sum, no atomics.
//   * plane_select_kernel: one workgroup.  A thread adds its hypotheses' chunk partials in chunk
//     order and keeps the best of them by P5; the threads' bests meet in a tree reduction on the
//     total key (count desc, err asc, index asc), which does not depend on the order.
//   * plane_flag_kernel: P6 over the N rows under the winning plane, read from device memory.
// pn2_plane_refit (P7) is two rounds -- centroid, then second moments -- of a chunk-partials
// kernel (the products staged in LDS by all threads, one thread per chain) and a one-wave
// finishing kernel that adds the chunk sums in order.
#include "collect_common.h"

namespace pn2 {

constexpr int kPlaneMaxRansacN = 64;
constexpr int kPlaneMaxIterations = 4096;
constexpr int kPlaneChunk = PN2_PLANE_CHUNK;
// Two hypotheses per thread: the three LDS broadcasts of a row feed 2 x 10 float64 VALU
// operations, as in collect_pair_kernel.  128 threads keep the tail of M = 1000 short (four
// blocks of 256 hypotheses, the last 232 wide); a whole 640 x 480 frame, N = 307200, is then
// 300 x 4 workgroups.
constexpr int kScoreThreads = 128;
constexpr int kScoreH = 2;
constexpr int kScoreHyps = kScoreThreads * kScoreH;
constexpr int kSelectThreads = 1024;
constexpr int kRefitThreads = 256;
constexpr int kRefitChains = 7;  // up to six sums and the row count

struct Plane {
    double a, b, c, d;
};

__device__ __forceinline__ double plane_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the norm, the zero test and the normalisation of P2 / P3; (qx, qy, qz) is the point d is taken at
__device__ __forceinline__ Plane plane_normalise(double a, double b, double c, double qx, double qy, double qz,
                                                 bool &zero) {
#pragma clang fp contract(off)
    const double norm = __dsqrt_rn((a * a + b * b) + c * c);
    zero = norm == 0.0;
    if (zero) return {0.0, 0.0, 0.0, 0.0};
    a = a / norm, b = b / norm, c = c / norm;
    return {a, b, c, -((a * qx + b * qy) + c * qz)};
}

// P2 from the six second moments and the centroid
__device__ __forceinline__ Plane plane_of_moments(double xx, double xy, double xz, double yy, double yz, double zz,
                                                  double cx, double cy, double cz, bool &zero) {
#pragma clang fp contract(off)
    const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
    double a, b, c;
    if (det_x > det_y && det_x > det_z) a = det_x, b = xz * yz - xy * zz, c = xy * yz - xz * yy;
    else if (det_y > det_z) a = xz * yz - xy * zz, b = det_y, c = xy * xz - yz * xx;
    else a = xy * yz - xz * yy, b = xy * xz - yz * xx, c = det_z;
    return plane_normalise(a, b, c, cx, cy, cz, zero);
}

// P4's distance
__device__ __forceinline__ double plane_dist(double a, double b, double c, double d, double x, double y, double z) {
#pragma clang fp contract(off)
    return fabs(((a * x + b * y) + c * z) + d);
}

template <typename T>
__global__ __launch_bounds__(256) void plane_fit_kernel(const T *__restrict__ pts, int64_t ld, int N,
                                                        const int *__restrict__ samples, int M, int n,
                                                        double *__restrict__ px, double *__restrict__ py,
                                                        double *__restrict__ pz, double *__restrict__ hyp,
                                                        double *__restrict__ out_planes, unsigned *__restrict__ err) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) load_xyz(pts, ld, i, px[i], py[i], pz[i]);
    if (i >= M) return;
    const int *row = samples + (int64_t)i * n;
    bool bad = false;
    for (int j = 0; j < n; ++j) bad |= row[j] < 0 || row[j] >= N;
    bool zero = false;
    Plane p = {0.0, 0.0, 0.0, 0.0};
    double x, y, z;
    if (bad) {
        atomicOr(err, (unsigned)PN2_DEVERR_INDEX);
    } else if (n == 3) {
        double x0, y0, z0;
        load_xyz(pts, ld, row[0], x0, y0, z0);
        load_xyz(pts, ld, row[1], x, y, z);
        const double e0x = x - x0, e0y = y - y0, e0z = z - z0;
        load_xyz(pts, ld, row[2], x, y, z);
        const double e1x = x - x0, e1y = y - y0, e1z = z - z0;
        p = plane_normalise(e0y * e1z - e0z * e1y, e0z * e1x - e0x * e1z, e0x * e1y - e0y * e1x, x0, y0, z0, zero);
    } else {
        double cx = 0.0, cy = 0.0, cz = 0.0;
        for (int j = 0; j < n; ++j) {
            load_xyz(pts, ld, row[j], x, y, z);
            cx = cx + x, cy = cy + y, cz = cz + z;
        }
        cx = cx / (double)n, cy = cy / (double)n, cz = cz / (double)n;
        double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
        for (int j = 0; j < n; ++j) {
            load_xyz(pts, ld, row[j], x, y, z);
            const double rx = x - cx, ry = y - cy, rz = z - cz;
            xx = xx + rx * rx, xy = xy + rx * ry, xz = xz + rx * rz;
            yy = yy + ry * ry, yz = yz + ry * rz, zz = zz + rz * rz;
        }
        p = plane_of_moments(xx, xy, xz, yy, yz, zz, cx, cy, cz, zero);
    }
    const bool skip = bad || zero;
    const double nan = plane_nan();
    double *h = hyp + (int64_t)i * 4;
    h[0] = skip ? nan : p.a, h[1] = skip ? nan : p.b, h[2] = skip ? nan : p.c, h[3] = skip ? nan : p.d;
    if (out_planes) {
        double *o = out_planes + (int64_t)i * 4;
        o[0] = skip ? 0.0 : p.a, o[1] = skip ? 0.0 : p.b, o[2] = skip ? 0.0 : p.c, o[3] = skip ? 0.0 : p.d;
    }
}

// pcnt / perr [nchunks][M]: chunk blockIdx.x under hypothesis m
__global__ __launch_bounds__(kScoreThreads) void plane_score_kernel(const double *__restrict__ px,
                                                                    const double *__restrict__ py,
                                                                    const double *__restrict__ pz, int N,
                                                                    const double *__restrict__ hyp, int M, double thr,
                                                                    int *__restrict__ pcnt,
                                                                    double *__restrict__ perr) {
#pragma clang fp contract(off)
    __shared__ double sx[kPlaneChunk], sy[kPlaneChunk], sz[kPlaneChunk];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kPlaneChunk;
    const int tlen = min(kPlaneChunk, N - c0);  // >= 1: the grid is ceil(N / chunk)
    for (int k = tid; k < tlen; k += kScoreThreads) sx[k] = px[c0 + k], sy[k] = py[c0 + k], sz[k] = pz[c0 + k];
    int m[kScoreH], cnt[kScoreH];
    double a[kScoreH], b[kScoreH], c[kScoreH], d[kScoreH], e[kScoreH];
#pragma unroll
    for (int h = 0; h < kScoreH; ++h) {
        m[h] = blockIdx.y * kScoreHyps + h * kScoreThreads + tid;
        a[h] = b[h] = c[h] = d[h] = plane_nan();  // a slot past M counts nothing
        if (m[h] < M) {
            const double *p = hyp + (int64_t)m[h] * 4;
            a[h] = p[0], b[h] = p[1], c[h] = p[2], d[h] = p[3];
        }
        cnt[h] = 0, e[h] = 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < tlen; ++k) {
        const double x = sx[k], y = sy[k], z = sz[k];
#pragma unroll
        for (int h = 0; h < kScoreH; ++h) {
            const double dist = plane_dist(a[h], b[h], c[h], d[h], x, y, z);
            const bool in = dist < thr;  // a NaN fails
            cnt[h] += in ? 1 : 0;
            e[h] = in ? e[h] + dist : e[h];
        }
    }
#pragma unroll
    for (int h = 0; h < kScoreH; ++h) {
        if (m[h] < M) {
            const int64_t at = (int64_t)blockIdx.x * M + m[h];
            pcnt[at] = cnt[h], perr[at] = e[h];
        }
    }
}

// P5's order as a total one: more inliers, then the smaller err, then the lower index
__device__ __forceinline__ bool plane_better(int ca, double ea, int ia, int cb, double eb, int ib) {
    return ca > cb || (ca == cb && (ea < eb || (ea == eb && ia < ib)));
}

__global__ __launch_bounds__(kSelectThreads) void plane_select_kernel(const int *__restrict__ pcnt,
                                                                      const double *__restrict__ perr, int nchunks,
                                                                      int M, const double *__restrict__ hyp,
                                                                      double *__restrict__ result,
                                                                      int *__restrict__ out_count,
                                                                      double *__restrict__ out_err) {
#pragma clang fp contract(off)
    __shared__ int s_cnt[kSelectThreads], s_idx[kSelectThreads];
    __shared__ double s_err[kSelectThreads];
    const int tid = threadIdx.x;
    int bc = 0, bi = -1;
    double be = 0.0;
    for (int m = tid; m < M; m += kSelectThreads) {  // ascending m: P5's walk as it stands
        int cn = 0;
        double e = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            cn += pcnt[(int64_t)c * M + m];
            e = e + perr[(int64_t)c * M + m];
        }
        if (out_count) out_count[m] = cn;
        if (out_err) out_err[m] = e;
        if (cn > bc || (cn == bc && e < be)) bc = cn, be = e, bi = m;
    }
    // a thread without a winner carries (0, 0.0, -1); every winner has count > 0 and beats it
    s_cnt[tid] = bc, s_err[tid] = be, s_idx[tid] = bi < 0 ? 0x7fffffff : bi;
    __syncthreads();
    for (int o = kSelectThreads / 2; o > 0; o >>= 1) {
        if (tid < o && plane_better(s_cnt[tid + o], s_err[tid + o], s_idx[tid + o], s_cnt[tid], s_err[tid], s_idx[tid]))
            s_cnt[tid] = s_cnt[tid + o], s_err[tid] = s_err[tid + o], s_idx[tid] = s_idx[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const bool none = s_cnt[0] == 0;
        const double *p = hyp + (int64_t)(none ? 0 : s_idx[0]) * 4;
        for (int k = 0; k < 4; ++k) result[k] = none ? 0.0 : p[k];
        result[4] = none ? -1.0 : (double)s_idx[0];
        result[5] = (double)s_cnt[0], result[6] = s_err[0], result[7] = 0.0;
    }
}

__global__ __launch_bounds__(256) void plane_flag_kernel(const double *__restrict__ px, const double *__restrict__ py,
                                                         const double *__restrict__ pz, int N,
                                                         const double *__restrict__ result, double thr,
                                                         int *__restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const bool none = result[4] < 0.0;  // P5's -1: nothing is an inlier
    const double dist = plane_dist(result[0], result[1], result[2], result[3], px[i], py[i], pz[i]);
    flags[i] = (!none && dist < thr) ? 1 : 0;
}

// ------------------------------------------------------------------------------------- refit
// Round 0 adds x, y, z and the row count of the flagged rows of one chunk; round 1 the six
// products of r = p - centroid.  A row that is not flagged adds +0.0: a chain from +0.0 is never
// -0.0, so it stays as it is.  The count is a chain of 1.0s, exact far past 2^20 rows.
// partial [nchunks][kRefitChains]; centre = {cx, cy, cz, (double)count} of round 0.
template <typename T>
__global__ __launch_bounds__(kRefitThreads) void plane_refit_partial_kernel(const T *__restrict__ pts, int64_t ld,
                                                                            int N, const int *__restrict__ flags,
                                                                            int round,
                                                                            const double *__restrict__ centre,
                                                                            double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double v[kPlaneChunk * kRefitChains];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kPlaneChunk;
    const int tlen = min(kPlaneChunk, N - c0);
    const double cx = round ? centre[0] : 0.0, cy = round ? centre[1] : 0.0, cz = round ? centre[2] : 0.0;
    for (int k = tid; k < tlen; k += kRefitThreads) {
        double x, y, z;
        load_xyz(pts, ld, c0 + k, x, y, z);
        const bool f = flags[c0 + k] != 0;
        double *s = v + k * kRefitChains;
        if (round == 0) {
            s[0] = f ? x : 0.0, s[1] = f ? y : 0.0, s[2] = f ? z : 0.0, s[3] = f ? 1.0 : 0.0;
        } else {
            const double rx = x - cx, ry = y - cy, rz = z - cz;
            s[0] = f ? rx * rx : 0.0, s[1] = f ? rx * ry : 0.0, s[2] = f ? rx * rz : 0.0;
            s[3] = f ? ry * ry : 0.0, s[4] = f ? ry * rz : 0.0, s[5] = f ? rz * rz : 0.0;
        }
    }
    __syncthreads();
    const int chains = round == 0 ? 4 : 6;
    if (tid < chains) {
        double acc = 0.0;
#pragma unroll 8
        for (int k = 0; k < tlen; ++k) acc = acc + v[k * kRefitChains + tid];
        partial[(int64_t)blockIdx.x * kRefitChains + tid] = acc;
    }
}

// one wave: lane q adds chain q's chunk sums in chunk order; lane 0 finishes the round
__global__ __launch_bounds__(64) void plane_refit_finish_kernel(const double *__restrict__ partial, int nchunks,
                                                                int round, double *__restrict__ centre,
                                                                double *__restrict__ plane) {
#pragma clang fp contract(off)
    __shared__ double total[kRefitChains];
    const int tid = threadIdx.x;
    const int chains = round == 0 ? 4 : 6;
    if (tid < chains) {
        double acc = 0.0;
        for (int c = 0; c < nchunks; ++c) acc = acc + partial[(int64_t)c * kRefitChains + tid];
        total[tid] = acc;
    }
    __syncthreads();
    if (tid != 0) return;
    if (round == 0) {
        const double n = total[3];
        const bool none = n == 0.0;
        centre[0] = none ? 0.0 : total[0] / n, centre[1] = none ? 0.0 : total[1] / n;
        centre[2] = none ? 0.0 : total[2] / n, centre[3] = n;
    } else {
        bool zero = false;
        Plane p = {0.0, 0.0, 0.0, 0.0};
        if (centre[3] != 0.0)
            p = plane_of_moments(total[0], total[1], total[2], total[3], total[4], total[5], centre[0], centre[1],
                                 centre[2], zero);
        plane[0] = p.a, plane[1] = p.b, plane[2] = p.c, plane[3] = p.d;
    }
}

static int64_t plane_chunks(int64_t N) { return (N + kPlaneChunk - 1) / kPlaneChunk; }

// the arrays of pn2_plane_segment's workspace, each padded to 16 bytes
struct PlaneWs {
    double *px, *py, *pz, *hyp, *perr;
    int *pcnt;
};
static int64_t plane_ws_bytes(int64_t N, int64_t M) {
    return 3 * align16(N * 8) + align16(M * 32) + align16(plane_chunks(N) * M * 8) + align16(plane_chunks(N) * M * 4);
}
static PlaneWs plane_ws(void *ws, int64_t N, int64_t M) {
    char *p = static_cast<char *>(ws);
    PlaneWs w;
    double **coords[3] = {&w.px, &w.py, &w.pz};
    for (int k = 0; k < 3; ++k) *coords[k] = reinterpret_cast<double *>(p), p += align16(N * 8);
    w.hyp = reinterpret_cast<double *>(p), p += align16(M * 32);
    w.perr = reinterpret_cast<double *>(p), p += align16(plane_chunks(N) * M * 8);
    w.pcnt = reinterpret_cast<int *>(p);
    return w;
}
static void score_launch(const PlaneWs &w, int64_t N, int64_t M, double thr, hipStream_t st) {
    hipLaunchKernelGGL(plane_score_kernel,
                       dim3((unsigned)plane_chunks(N), (unsigned)((M + kScoreHyps - 1) / kScoreHyps)),
                       dim3(kScoreThreads), 0, st, w.px, w.py, w.pz, (int)N, w.hyp, (int)M, thr, w.pcnt, w.perr);
}
static int64_t refit_ws_bytes(int64_t N) { return align16(plane_chunks(N) * kRefitChains * 8) + 32; }

static bool threshold_ok(double t) { return t > 0.0 && t < __builtin_inf(); }  // a NaN fails

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_plane_max_ransac_n(void) { return kPlaneMaxRansacN; }
extern "C" int64_t pn2_plane_max_iterations(void) { return kPlaneMaxIterations; }

extern "C" int64_t pn2_plane_segment_workspace_bytes(int64_t N, int64_t M) {
    if (N < 0 || N > kCollectMaxN || M < 1 || M > kPlaneMaxIterations) return -1;
    return plane_ws_bytes(N, M);
}

extern "C" int pn2_plane_segment(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, const int32_t *samples,
                                 int64_t M, int64_t n, double distance_threshold, int32_t *flags, double *result,
                                 double *out_planes, int32_t *out_count, double *out_err, void *workspace,
                                 int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && samples && flags && result, "pn2_plane_segment: null pointer");
    const int rc = check_cloud("pn2_plane_segment", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(n >= 3, "pn2_plane_segment: ransac_n = %lld, needs >= 3", (long long)n);
    PN2_REQUIRE(M >= 1, "pn2_plane_segment: num_iterations = %lld, needs >= 1", (long long)M);
    if (n > kPlaneMaxRansacN)
        return set_error(PN2_EUNSUPPORTED, "pn2_plane_segment: ransac_n = %lld above pn2_plane_max_ransac_n() = %d",
                         (long long)n, kPlaneMaxRansacN);
    if (M > kPlaneMaxIterations)
        return set_error(PN2_EUNSUPPORTED,
                         "pn2_plane_segment: num_iterations = %lld above pn2_plane_max_iterations() = %d",
                         (long long)M, kPlaneMaxIterations);
    PN2_REQUIRE(threshold_ok(distance_threshold), "pn2_plane_segment: distance_threshold = %g, needs finite and > 0",
                distance_threshold);
    if (N == 0) return PN2_OK;
    const int64_t need = plane_ws_bytes(N, M);
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_plane_segment: workspace too small: needs pn2_plane_segment_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    hipStream_t st = as_stream(stream);
    unsigned *err = error_word(st);
    PN2_REQUIRE(err, "pn2_plane_segment: no device error slot");
    const PlaneWs w = plane_ws(workspace, N, M);
    const int64_t nchunks = plane_chunks(N);
    const dim3 fgrid((unsigned)(((N > M ? N : M) + 255) / 256));
    if (dtype == PN2_DTYPE_F64)
        hipLaunchKernelGGL(plane_fit_kernel<double>, fgrid, dim3(256), 0, st, static_cast<const double *>(pts), ld,
                           (int)N, samples, (int)M, (int)n, w.px, w.py, w.pz, w.hyp, out_planes, err);
    else
        hipLaunchKernelGGL(plane_fit_kernel<float>, fgrid, dim3(256), 0, st, static_cast<const float *>(pts), ld,
                           (int)N, samples, (int)M, (int)n, w.px, w.py, w.pz, w.hyp, out_planes, err);
    PN2_LAUNCH_CHECK("plane_fit_kernel");
    score_launch(w, N, M, distance_threshold, st);
    PN2_LAUNCH_CHECK("plane_score_kernel");
    hipLaunchKernelGGL(plane_select_kernel, dim3(1), dim3(kSelectThreads), 0, st, w.pcnt, w.perr, (int)nchunks, (int)M,
                       w.hyp, result, out_count, out_err);
    PN2_LAUNCH_CHECK("plane_select_kernel");
    hipLaunchKernelGGL(plane_flag_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, w.px, w.py, w.pz, (int)N,
                       result, distance_threshold, flags);
    PN2_LAUNCH_CHECK("plane_flag_kernel");
    return PN2_OK;
}

extern "C" int pn2_plane_score(int64_t N, int64_t M, double distance_threshold, void *workspace,
                               int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(N >= 0 && M >= 1, "pn2_plane_score: bad shape (N=%lld M=%lld)", (long long)N, (long long)M);
    if (N > kCollectMaxN)
        return set_error(PN2_EUNSUPPORTED, "pn2_plane_score: N=%lld above pn2_collect_max_points() = %lld",
                         (long long)N, (long long)kCollectMaxN);
    if (M > kPlaneMaxIterations)
        return set_error(PN2_EUNSUPPORTED, "pn2_plane_score: num_iterations = %lld above pn2_plane_max_iterations() = %d",
                         (long long)M, kPlaneMaxIterations);
    PN2_REQUIRE(threshold_ok(distance_threshold), "pn2_plane_score: distance_threshold = %g, needs finite and > 0",
                distance_threshold);
    if (N == 0) return PN2_OK;
    const int64_t need = plane_ws_bytes(N, M);
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_plane_score: workspace too small: needs pn2_plane_segment_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    score_launch(plane_ws(workspace, N, M), N, M, distance_threshold, as_stream(stream));
    PN2_LAUNCH_CHECK("plane_score_kernel");
    return PN2_OK;
}

extern "C" int64_t pn2_plane_refit_workspace_bytes(int64_t N) {
    if (N < 0 || N > kCollectMaxN) return -1;
    return refit_ws_bytes(N);
}

template <typename T>
static int refit_run(const void *pts, int64_t N, int64_t ld, const int *flags, double *plane, void *ws,
                     hipStream_t st) {
    const int64_t nchunks = plane_chunks(N);
    double *partial = static_cast<double *>(ws);
    double *centre = partial + align16(nchunks * kRefitChains * 8) / 8;
    for (int round = 0; round < 2; ++round) {
        hipLaunchKernelGGL(plane_refit_partial_kernel<T>, dim3((unsigned)nchunks), dim3(kRefitThreads), 0, st,
                           static_cast<const T *>(pts), ld, (int)N, flags, round, centre, partial);
        PN2_LAUNCH_CHECK("plane_refit_partial_kernel");
        hipLaunchKernelGGL(plane_refit_finish_kernel, dim3(1), dim3(64), 0, st, partial, (int)nchunks, round, centre,
                           plane);
        PN2_LAUNCH_CHECK("plane_refit_finish_kernel");
    }
    return PN2_OK;
}

extern "C" int pn2_plane_refit(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, const int32_t *flags,
                               double *plane, void *workspace, int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && flags && plane, "pn2_plane_refit: null pointer");
    const int rc = check_cloud("pn2_plane_refit", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    if (N == 0) return PN2_OK;
    const int64_t need = refit_ws_bytes(N);
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_plane_refit: workspace too small: needs pn2_plane_refit_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    hipStream_t st = as_stream(stream);
    if (dtype == PN2_DTYPE_F64) return refit_run<double>(pts, N, ld, flags, plane, workspace, st);
    return refit_run<float>(pts, N, ld, flags, plane, workspace, st);
}
