// fps_points.hip -- farthest-point downsampling of raw clouds by the reference's NUMPY rule, for
// gfx950.
//
// Replaces the host function farthest_point_sample(point_cloud, number) that every route into
// the reference's models passes through (provider.py:183-204 and its textually identical copies
// data_utils/ModelDataLoader.py:10-31, data_utils/ModelNetDataLoader.py:25-46,
// point_collect/transformer.py:120-141, colledt_data_structure/transformer.py:120-141,
// data_build/*.py e.g. Cube.py:102-123):
//
//     xyz = point_cloud[:, :3]
//     distance = np.ones((N,)) * 1e10
//     farthest = np.random.randint(0, N)
//     for i in range(number):
//         centroids[i] = farthest
//         dist = np.sum((xyz - xyz[farthest, :]) ** 2, -1)
//         mask = dist < distance;  distance[mask] = dist[mask]
//         farthest = np.argmax(distance, -1)
//     return point_cloud[centroids.astype(np.int32)]
//
// A different computation from fps.hip (the SA layers' torch rule): the arithmetic is the input's
// own precision (float64 rows from np.loadtxt, float32 in the ModelNet loader), only the first
// three columns are measured whatever C is, the initial distance is a finite 1e10 that is
// COMPARED (a point farther than that from every centroid is never updated), the iteration count
// is `number` even past N, and the result is the gathered rows with all C columns.
//
// In numpy's order, every operation rounded on its own (the unit is built with -ffp-contract=off
// and the helpers below switch contraction off themselves):
//     d_k = x_k - c_k (k = 0, 1, 2);  s_k = d_k * d_k;  dist = (s_0 + s_1) + s_2
// (np.sum over a 3-element last axis adds in order).  np.argmax returns the FIRST index of the
// maximum.  Distances are never negative and never NaN for finite input (an overflowing square
// is +inf, which `<` leaves alone), so their IEEE bit patterns order as unsigned integers.
//
// One workgroup of kPtsThreads threads per cloud; the launch is a ragged batch (row offsets per
// cloud), one workgroup never waits for another.  Nothing of a cloud is register-resident: each
// iteration thread t walks the points t, t + kPtsThreads, ..., re-reading x, y, z (L2 hits after
// the first iteration), and keeps the running distance -- in LDS when the launch's largest cloud
// fits (DL), else in the caller's workspace, one element per input row -- and its best
// (distance bits, index) pair, which wg_argmax (below) merges across the workgroup by
// np.argmax's rule.  A point's distance element is only ever touched by its own thread.  The
// indices go straight to out_idx; the gather pass after the loop reads them back.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kPtsThreads = 1024;
constexpr int kPtsWaves = kPtsThreads / 64;
constexpr size_t kPtsLds = (size_t)160 * 1024;
// wg_argmax slots: [2][waves] distance bits (room for 64-bit ones), then [2][waves] int indices
constexpr size_t kPtsLdsHead = (size_t)2 * kPtsWaves * (8 + 4);

template <typename T> struct PtsBits;
template <> struct PtsBits<float> {
    typedef unsigned type;
    static __device__ __forceinline__ type of(float v) { return __float_as_uint(v); }
};
template <> struct PtsBits<double> {
    typedef unsigned long long type;
    static __device__ __forceinline__ type of(double v) { return (unsigned long long)__double_as_longlong(v); }
};

template <typename T>
__device__ __forceinline__ T pts_sub(T a, T b) {
#pragma clang fp contract(off)
    return a - b;
}
template <typename T>
__device__ __forceinline__ T pts_mul(T a, T b) {
#pragma clang fp contract(off)
    return a * b;
}
template <typename T>
__device__ __forceinline__ T pts_add(T a, T b) {
#pragma clang fp contract(off)
    return a + b;
}

// ---- workgroup argmax, "the first index of the maximum" (np.argmax), on (bits,
// index) pairs, bits the unsigned pattern of a non-negative distance: greater bits win, on equal
// bits the smaller index.  A thread without a point holds (0, INT32_MAX), which loses to every
// real pair.
template <typename U>
__device__ __forceinline__ void argmax_take(U &bits, int &idx, U ob, int oi) {
    static_assert(sizeof(U) == 4 || sizeof(U) == 8, "unsigned or unsigned long long bits");
    const bool take = (ob > bits) | ((ob == bits) & (oi < idx));  // two selects, no branch
    bits = take ? ob : bits, idx = take ? oi : idx;
}
// Every thread of a workgroup of NW waves brings its pair and leaves with the workgroup's best:
// wave merge by shuffles, one LDS slot per wave (sbits / sidx: [2][NW]), ONE barrier, every
// thread merges the NW slots.  The slots are double-buffered by the caller's iteration parity
// `par`, which is why one barrier suffices: a thread writing parity p in iteration i + 2 has
// passed the barrier of iteration i + 1, which no thread reaches before it has finished reading
// iteration i's slots of parity p.
template <int NW, typename U>
__device__ __forceinline__ void wg_argmax(U &bits, int &idx, U *sbits, int *sidx, int par) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) argmax_take(bits, idx, __shfl_xor(bits, o), __shfl_xor(idx, o));
    sbits += par * NW, sidx += par * NW;
    if ((threadIdx.x & 63) == 0) sbits[threadIdx.x >> 6] = bits, sidx[threadIdx.x >> 6] = idx;
    __syncthreads();
    bits = sbits[0], idx = sidx[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) argmax_take(bits, idx, sbits[w], sidx[w]);
}

template <typename T, bool DL>
__global__ __launch_bounds__(kPtsThreads) void fps_points_kernel(
    const T *__restrict__ pts, int64_t ld, int C, const int64_t *__restrict__ offsets,
    const int64_t *__restrict__ starts, int S, int64_t max_n, int64_t total_rows,
    int64_t *__restrict__ out_idx, T *__restrict__ out_pts, T *__restrict__ dist_ws,
    unsigned *__restrict__ err) {
    typedef typename PtsBits<T>::type U;
    constexpr int NT = kPtsThreads, NW = kPtsWaves;
    extern __shared__ __attribute__((aligned(16))) unsigned long long psm[];
    U *sbits = reinterpret_cast<U *>(psm);                    // [2][NW]
    int *sidx = reinterpret_cast<int *>(psm + 2 * NW);        // [2][NW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int64_t row0 = offsets[b], N64 = offsets[b + 1] - row0;
    int64_t *oi = out_idx + b * S;
    int far = (int)starts[b];
    // a table the host did not build as documented: stay in bounds, mark the cloud, raise the bit
    if (row0 < 0 || N64 < 1 || N64 > max_n || row0 + N64 > total_rows || starts[b] < 0 || starts[b] >= N64) {
        for (int i = tid; i < S; i += NT) oi[i] = -1;
        if (tid == 0) atomicOr(err, (unsigned)PN2_DEVERR_INDEX);
        return;
    }
    const int N = (int)N64;
    const T *P = pts + row0 * ld;
    T *dist = DL ? reinterpret_cast<T *>(reinterpret_cast<char *>(psm) + kPtsLdsHead) : dist_ws + row0;
    for (int n = tid; n < N; n += NT) dist[n] = (T)1e10;
    T c0 = P[(int64_t)far * ld], c1 = P[(int64_t)far * ld + 1], c2 = P[(int64_t)far * ld + 2];
    for (int i = 0;; ++i) {
        if (tid == 0) oi[i] = far;
        if (i == S - 1) break;  // the last iteration's update feeds no further argmax
        U best = 0;
        far = tid < N ? tid : INT32_MAX;  // the thread's first point holds any tie at 0
        for (int n = tid; n < N; n += NT) {
            const T *q = P + (int64_t)n * ld;
            const T d0 = pts_sub(q[0], c0), d1 = pts_sub(q[1], c1), d2 = pts_sub(q[2], c2);
            const T dd = pts_add(pts_add(pts_mul(d0, d0), pts_mul(d1, d1)), pts_mul(d2, d2));
            T cur = dist[n];
            if (dd < cur) {  // strict: the reference's mask
                cur = dd;
                dist[n] = dd;
            }
            const U bits = PtsBits<T>::of(cur);
            if (bits > best) best = bits, far = n;  // n ascends: the first index of the thread's maximum
        }
        wg_argmax<NW>(best, far, sbits, sidx, i & 1);
        c0 = P[(int64_t)far * ld], c1 = P[(int64_t)far * ld + 1], c2 = P[(int64_t)far * ld + 2];
    }
    __syncthreads();
    // point_cloud[idx]: all C columns of the chosen rows (indices written by thread 0 above)
    // one 64-lane wave per row, its lanes over the columns: no division, coalesced rows
    T *o = out_pts + b * S * C;
    for (int i = wave; i < S; i += NW) {
        const int64_t n = __hip_atomic_load(oi + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int k = lane; k < C; k += 64) o[(int64_t)i * C + k] = P[n * ld + k];
    }
}

static int64_t elem_bytes(int dtype) { return dtype == PN2_DTYPE_F64 ? 8 : dtype == PN2_DTYPE_F32 ? 4 : 0; }
// largest cloud whose running distances the LDS holds beside the wave slots
static int64_t lds_max_n(int dtype) { return (int64_t)((kPtsLds - kPtsLdsHead) / (size_t)elem_bytes(dtype)); }

template <typename T>
static int launch_fps_points(const void *pts, int64_t B, const int64_t *offsets, const int64_t *starts,
                             int64_t total_rows, int64_t max_n, int64_t C, int64_t ld, int64_t S,
                             int64_t *out_idx, void *out_pts, void *ws, bool dl, unsigned *err, hipStream_t st) {
    const T *p = static_cast<const T *>(pts);
    T *o = static_cast<T *>(out_pts);
    if (dl) {
        // per device, so set on every call (a host-side table update), not once per process
        const hipError_t attr = hipFuncSetAttribute(
            reinterpret_cast<const void *>(&fps_points_kernel<T, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPtsLds);
        PN2_REQUIRE(attr == hipSuccess, "pn2_fps_points: LDS attribute: %s", hipGetErrorString(attr));
        hipLaunchKernelGGL((fps_points_kernel<T, true>), dim3((unsigned)B), dim3(kPtsThreads),
                           kPtsLdsHead + (size_t)max_n * sizeof(T), st, p, ld, (int)C, offsets, starts, (int)S,
                           max_n, total_rows, out_idx, o, nullptr, err);
    } else {
        hipLaunchKernelGGL((fps_points_kernel<T, false>), dim3((unsigned)B), dim3(kPtsThreads), kPtsLdsHead, st,
                           p, ld, (int)C, offsets, starts, (int)S, max_n, total_rows, out_idx, o,
                           static_cast<T *>(ws), err);
    }
    PN2_LAUNCH_CHECK("fps_points_kernel");
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_fps_points_workspace_bytes(int dtype, int64_t total_rows, int64_t max_n) {
    if (elem_bytes(dtype) == 0 || total_rows < 0 || max_n < 0 || max_n > total_rows) return -1;
    return max_n <= lds_max_n(dtype) ? 0 : total_rows * elem_bytes(dtype);
}

extern "C" int pn2_fps_points(const void *pts, int dtype, int64_t B, const int64_t *offsets,
                              const int64_t *starts, int64_t total_rows, int64_t max_n, int64_t C, int64_t ld,
                              int64_t S, int64_t *out_idx, void *out_pts, void *workspace,
                              int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && offsets && starts && out_idx && out_pts, "pn2_fps_points: null pointer");
    PN2_REQUIRE(elem_bytes(dtype) != 0, "pn2_fps_points: unknown dtype %d", dtype);
    PN2_REQUIRE(B >= 0 && B < INT32_MAX && C >= 3 && C < INT32_MAX && ld >= C && S >= 0 && S < INT32_MAX &&
                    max_n >= 1 && max_n < INT32_MAX && total_rows >= max_n,
                "pn2_fps_points: bad shape (B=%lld rows=%lld max_n=%lld C=%lld ld=%lld S=%lld)", (long long)B,
                (long long)total_rows, (long long)max_n, (long long)C, (long long)ld, (long long)S);
    const int64_t need = pn2_fps_points_workspace_bytes(dtype, total_rows, max_n);
    PN2_REQUIRE(need == 0 || (workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need),
                "pn2_fps_points: workspace too small: max_n=%lld needs pn2_fps_points_workspace_bytes = %lld "
                "bytes, 8-byte aligned", (long long)max_n, (long long)need);
    if (B == 0 || S == 0) return PN2_OK;
    hipStream_t st = as_stream(stream);
    unsigned *err = error_word(st);
    PN2_REQUIRE(err, "pn2_fps_points: no device error slot");
    if (dtype == PN2_DTYPE_F64)
        return launch_fps_points<double>(pts, B, offsets, starts, total_rows, max_n, C, ld, S, out_idx, out_pts,
                                         workspace, need == 0, err, st);
    return launch_fps_points<float>(pts, B, offsets, starts, total_rows, max_n, C, ld, S, out_idx, out_pts,
                                    workspace, need == 0, err, st);
}
