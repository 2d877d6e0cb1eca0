// collect.hip -- the camera-cloud front end of the reference's capture scripts, for gfx950:
// clip_distance, delet_outlier_radius and cluster_point (point_collect/collect.py:30-102 and its
// copy colledt_data_structure/collect.py; camera_test/camera.py:131), which there are numpy masks
// and Open3D kd-tree calls on the host over a 640 x 480 frame.  The rules are stated in
// include/pn2.h ("camera-cloud front end"); every result is a selection of input rows or an
// integer, so parity is bit for bit.
//
// Three kernel families:
//   * collect_pair_kernel: tiled brute force over (query, candidate) pairs.  A workgroup owns a
//     slab of kPairSlab queries in registers (kPairQ per thread) and streams the candidates
//     through LDS as separate x, y, z arrays: every lane reads the same candidate (a broadcast,
//     no bank conflict) and feeds kPairQ chains.  Three modes share the tiling: COUNT (neighbours
//     per point), UNION (core-core pairs into a union-find), BORDER (min core label per non-core
//     point).  No workgroup waits on another.
//   * the compaction (compact_count / compact_scan / compact_scatter): an order-preserving
//     bucket sort of rows by a per-row key, one wave per chunk of kChunk consecutive rows.  With
//     one bucket it is the stream compaction of the clip and the radius filter; with L buckets
//     the stable counting sort of rows by cluster label, whose scan also is the `offsets` table
//     pn2_fps_points takes.
//   * small maps (flags, union-find init / flatten / label).
#include "collect_common.h"

namespace pn2 {

constexpr int kPairThreads = 256;
// Queries per thread.  float64 adds and multiplies issue at a quarter of the float32 rate, so the
// three LDS broadcasts per candidate are already hidden behind 2 x 10 VALU operations; a larger
// slab only leaves fewer waves (a 307200-point frame is 2400 waves of 128 queries: 2.3 per SIMD).
constexpr int kPairQ = 2;
constexpr int kPairSlab = kPairThreads * kPairQ;
constexpr int kPairTile = 1024;  // candidates per LDS tile: 3 x 8 KiB (+ 4 KiB of labels)
constexpr int kChunk = 256;      // rows per compaction chunk: one wave, kChunkSteps steps of 64
constexpr int kChunkSteps = kChunk / 64;
constexpr int64_t kCompactMaxEntries = (int64_t)1 << 26;  // chunks x buckets of one compaction

// ------------------------------------------------------------------------ the neighbour rule
// (nbr_d2: collect_common.h)
// j is a neighbour of i iff d2 < r*r.  The strict `<` is a reading of nanoflann's radius result
// set behind Open3D's SearchRadius that nobody has checked against Open3D: a
// correction is this one line.
__device__ __forceinline__ bool nbr_within(double d2, double r2) { return d2 < r2; }

__device__ __forceinline__ int n_of(const int64_t *n_dev, int n_host) {
    if (!n_dev) return n_host;
    const int64_t n = *n_dev;
    return n < 0 ? 0 : n > n_host ? n_host : (int)n;  // never past what the host sized
}

// ------------------------------------------------------------------------------- union-find
// 32-bit parents over the compacted core points.  A root is linked under a SMALLER root only, by
// compare-and-swap on its own slot, so a parent only ever decreases: every retry loop terminates
// and no thread waits for another's progress.  After the flatten pass every root is its
// component's smallest index whatever the order of execution.
__device__ __forceinline__ int uf_load(int *parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int *parent, int x) {
    for (;;) {
        const int p = uf_load(parent, x);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ int uf_unite(int *parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        if (atomicCAS(parent + a, a, b) == a) return b;  // else a was linked meanwhile: again
    }
}

enum { PAIR_COUNT = 0, PAIR_UNION = 1, PAIR_BORDER = 2 };

// queries qi in [0, nq): point qsel[qi] (or qi); candidates cj in [0, nc): point csel[cj] (or cj).
//   COUNT   out[point of qi] = number of candidates within r
//   UNION   qsel == csel (the core points): unite(qi, cj) for every cj < qi within r
//   BORDER  out[point of qi] = min clabel[cj] over candidates within r, -1 if none
template <typename T, int MODE>
__global__ __launch_bounds__(kPairThreads) void collect_pair_kernel(
    const T *__restrict__ pts, int64_t ld, const int *__restrict__ qsel, const int64_t *nq_dev, int nq_host,
    const int *__restrict__ csel, const int64_t *nc_dev, int nc_host, double r2, int *__restrict__ out,
    int *parent, const int *__restrict__ clabel) {
    __shared__ double sx[kPairTile], sy[kPairTile], sz[kPairTile];
    __shared__ int sl[MODE == PAIR_BORDER ? kPairTile : 1];
    const int tid = threadIdx.x;
    const int nq = n_of(nq_dev, nq_host), nc = n_of(nc_dev, nc_host);
    const int base = blockIdx.x * kPairSlab;
    if (base >= nq) return;  // the whole workgroup: before any barrier
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int qi[kPairQ], qp[kPairQ], root[kPairQ];
    unsigned acc[kPairQ];
    double qx[kPairQ], qy[kPairQ], qz[kPairQ];
#pragma unroll
    for (int s = 0; s < kPairQ; ++s) {
        qi[s] = base + s * kPairThreads + tid;
        qx[s] = qy[s] = qz[s] = nan;  // a slot past nq is nobody's neighbour
        qp[s] = -1;
        if (qi[s] < nq) {
            qp[s] = qsel ? qsel[qi[s]] : qi[s];
            load_xyz(pts, ld, qp[s], qx[s], qy[s], qz[s]);
        }
        acc[s] = MODE == PAIR_BORDER ? 0xffffffffu : 0u;
        root[s] = qi[s];
    }
    // UNION takes the pairs cj < qi only: the relation is symmetric
    const int cend = MODE == PAIR_UNION ? min(nc, base + kPairSlab) : nc;
    for (int c0 = 0; c0 < cend; c0 += kPairTile) {
        const int tlen = min(kPairTile, cend - c0);
        for (int k = tid; k < tlen; k += kPairThreads) {
            const int cp = csel ? csel[c0 + k] : c0 + k;
            load_xyz(pts, ld, cp, sx[k], sy[k], sz[k]);
            if (MODE == PAIR_BORDER) sl[k] = clabel[c0 + k];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < tlen; ++k) {
            const double cx = sx[k], cy = sy[k], cz = sz[k];
#pragma unroll
            for (int s = 0; s < kPairQ; ++s) {
                const bool in = nbr_within(nbr_d2(qx[s], qy[s], qz[s], cx, cy, cz), r2);
                if (MODE == PAIR_COUNT) acc[s] += in ? 1u : 0u;
                if (MODE == PAIR_BORDER) acc[s] = in ? min(acc[s], (unsigned)sl[k]) : acc[s];
                if (MODE == PAIR_UNION) {
                    const int cj = c0 + k;
                    // one read settles a candidate already under the root this query last saw
                    if (in && cj < qi[s] && uf_load(parent, cj) != root[s]) root[s] = uf_unite(parent, qi[s], cj);
                }
            }
        }
        __syncthreads();
    }
    if (MODE != PAIR_UNION) {
#pragma unroll
        for (int s = 0; s < kPairQ; ++s)
            if (qp[s] >= 0) out[qp[s]] = (int)acc[s];
    }
}

// ---------------------------------------------------------------------------------- small maps
template <typename T>
__global__ void clip_flags_kernel(const T *__restrict__ pts, int64_t ld, int n, int axis, double lo, double hi,
                                  int *__restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = (double)pts[(int64_t)i * ld + axis];
    flags[i] = (v >= lo && v <= hi) ? 1 : 0;  // a NaN fails both
}

__global__ void uf_init_kernel(int *parent, int n_host) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_host) parent[i] = i;
}
// root[k] = the component's smallest core index; isroot[k] for the ranking compaction
__global__ void uf_flatten_kernel(int *parent, const int64_t *m_dev, int n_host, int *__restrict__ root,
                                  int *__restrict__ isroot) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_of(m_dev, n_host)) return;
    const int r = uf_find(parent, k);
    root[k] = r;
    isroot[k] = r == k ? 1 : 0;
}
// clusters numbered in ascending order of their smallest core index: rank[] is the exclusive
// prefix sum over "is root" in index order (the compaction's out_pos)
__global__ void core_label_kernel(const int *__restrict__ root, const int *__restrict__ rank,
                                  const int *__restrict__ core_idx, const int64_t *m_dev, int n_host,
                                  const int64_t *nroots, int *__restrict__ clabel, int *__restrict__ labels,
                                  int64_t *__restrict__ nclusters) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *nclusters = *nroots;
    if (k >= n_of(m_dev, n_host)) return;
    const int l = rank[root[k]];
    clabel[k] = l;
    labels[core_idx[k]] = l;
}

// ---------------------------------------------------------------------------------- compaction
// bucket of row i: FLAG_GT key > thresh -> 0, FLAG_LE key <= thresh -> 0, LABEL key in [0, L);
// everything else is dropped (-1).  A LABEL key >= L raises PN2_DEVERR_INDEX.
__device__ __forceinline__ int bucket_of(const int *keys, int i, int n, int mode, int thresh, int L, bool &bad) {
    if (i >= n) return -1;
    const int k = keys[i];
    if (mode == PN2_COMPACT_FLAG_GT) return k > thresh ? 0 : -1;
    if (mode == PN2_COMPACT_FLAG_LE) return k <= thresh ? 0 : -1;
    if (k >= L) bad = true;
    return (k < 0 || k >= L) ? -1 : k;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// table[b * nchunks + c] = rows of chunk c in bucket b (zeroed by the host before the launch:
// a (bucket, chunk) pair without rows is never written)
__global__ __launch_bounds__(256) void compact_count_kernel(const int *__restrict__ keys, const int64_t *n_dev,
                                                            int n_host, int mode, int thresh, int L,
                                                            int64_t nchunks, int *__restrict__ table,
                                                            unsigned *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = n_of(n_dev, n_host);
    if (c >= nchunks || c * kChunk >= n) return;  // wave-uniform
    int b[kChunkSteps];
    unsigned long long todo[kChunkSteps];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < kChunkSteps; ++s) {
        b[s] = bucket_of(keys, (int)(c * kChunk) + s * 64 + lane, n, mode, thresh, L, bad);
        todo[s] = __ballot(b[s] >= 0);
    }
    if (bad) atomicOr(err, (unsigned)PN2_DEVERR_INDEX);
#pragma unroll
    for (int s = 0; s < kChunkSteps; ++s) {
        while (todo[s]) {  // one round per distinct bucket of the chunk
            const int cur = __shfl(b[s], __ffsll((long long)todo[s]) - 1);
            int total = 0;
#pragma unroll
            for (int t = s; t < kChunkSteps; ++t) {
                const unsigned long long m = __ballot(b[t] == cur);
                total += __popcll(m);
                todo[t] &= ~m;
            }
            if (lane == 0) table[(int64_t)cur * nchunks + c] = total;
        }
    }
}

// exclusive scan of the table in bucket-major order, in place; offsets[b] = first output row of
// bucket b, offsets[L] = rows kept.  One workgroup: the table is chunks x buckets ints.
__global__ __launch_bounds__(1024) void compact_scan_kernel(int *__restrict__ table, int64_t entries,
                                                            int64_t nchunks, int64_t L,
                                                            int64_t *__restrict__ offsets) {
    __shared__ int swave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int64_t e0 = 0; e0 < entries; e0 += 1024) {
        const int64_t e = e0 + tid;
        const int v = e < entries ? table[e] : 0;
        int x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) swave[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = swave[w];
            before += w < wave ? t : 0;
            total += t;
        }
        const int excl = carry + before + x - v;
        if (e < entries) {
            table[e] = excl;
            if (e % nchunks == 0) offsets[e / nchunks] = excl;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[L] = carry;
}

// U: the unit rows are moved in (uint4 where every row of both sides is 16-byte aligned, else
// the element); upr units per output row, ldu units between input rows
template <typename U>
__global__ __launch_bounds__(256) void compact_scatter_kernel(
    const U *__restrict__ in, int64_t ldu, int upr, const int *__restrict__ keys, const int64_t *n_dev, int n_host,
    int mode, int thresh, int L, int64_t nchunks, const int *__restrict__ table, U *__restrict__ out,
    int *__restrict__ out_src, int *__restrict__ out_pos) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = n_of(n_dev, n_host);
    if (c >= nchunks || c * kChunk >= n) return;
    const int row0 = (int)(c * kChunk);
    int b[kChunkSteps], pos[kChunkSteps];
    unsigned long long todo[kChunkSteps];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < kChunkSteps; ++s) {
        b[s] = bucket_of(keys, row0 + s * 64 + lane, n, mode, thresh, L, bad);
        todo[s] = __ballot(b[s] >= 0);
        pos[s] = -1;
    }
#pragma unroll
    for (int s = 0; s < kChunkSteps; ++s) {
        while (todo[s]) {
            const int cur = __shfl(b[s], __ffsll((long long)todo[s]) - 1);
            int running = table[(int64_t)cur * nchunks + c];  // first output row of (cur, c)
#pragma unroll
            for (int t = s; t < kChunkSteps; ++t) {
                const unsigned long long m = __ballot(b[t] == cur);
                if (b[t] == cur) pos[t] = running + __popcll(m & lanes_below(lane));
                running += __popcll(m);
                todo[t] &= ~m;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kChunkSteps; ++s) {
        const int i = row0 + s * 64 + lane;
        if (i < n) {
            if (out_pos) out_pos[i] = pos[s];
            if (out_src && pos[s] >= 0) out_src[pos[s]] = i;
        }
        if (in) {  // the step's 64 rows as one flat run of units over the lanes
            for (int u = lane; u < 64 * upr; u += 64) {
                const int r = u / upr, piece = u - r * upr;
                const int dst = __shfl(pos[s], r);
                if (dst >= 0) out[(int64_t)dst * upr + piece] = in[(int64_t)(row0 + s * 64 + r) * ldu + piece];
            }
        }
    }
}

static int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

struct CompactJob {
    const void *pts;  // null: indices only
    int dtype;
    int64_t n_host;
    const int64_t *n_dev;
    int64_t C, ld;
    const int *keys;
    int mode;
    int64_t thresh, L;
    void *out_rows;
    int *out_src, *out_pos;
    int64_t *offsets;
    int *table;
};

template <typename U>
static void scatter_launch(const CompactJob &j, int64_t nchunks, int64_t es, hipStream_t st) {
    const int64_t per = (int64_t)sizeof(U) / es;  // elements per unit
    hipLaunchKernelGGL((compact_scatter_kernel<U>), dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, st,
                       static_cast<const U *>(j.pts), j.ld / per, (int)(j.C / per), j.keys, j.n_dev, (int)j.n_host,
                       j.mode, (int)j.thresh, (int)j.L, nchunks, j.table, static_cast<U *>(j.out_rows), j.out_src,
                       j.out_pos);
}

static int compact_run(const CompactJob &j, unsigned *err, hipStream_t st) {
    const int64_t nchunks = chunks_of(j.n_host), entries = nchunks * j.L;
    const hipError_t e = hipMemsetAsync(j.table, 0, (size_t)entries * 4, st);
    if (e != hipSuccess) return set_error(PN2_EHIP, "pn2_compact_rows: memset: %s", hipGetErrorString(e));
    const unsigned grid = (unsigned)((nchunks + 3) / 4);
    hipLaunchKernelGGL(compact_count_kernel, dim3(grid), dim3(256), 0, st, j.keys, j.n_dev, (int)j.n_host, j.mode,
                       (int)j.thresh, (int)j.L, nchunks, j.table, err);
    PN2_LAUNCH_CHECK("compact_count_kernel");
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, st, j.table, entries, nchunks, j.L, j.offsets);
    PN2_LAUNCH_CHECK("compact_scan_kernel");
    const int64_t es = j.pts ? elem_size(j.dtype) : 4;
    const bool v16 = j.pts && (j.C * es) % 16 == 0 && (j.ld * es) % 16 == 0 && ((uintptr_t)j.pts & 15) == 0 &&
                     ((uintptr_t)j.out_rows & 15) == 0;
    if (v16) scatter_launch<uint4>(j, nchunks, es, st);
    else if (es == 8) scatter_launch<unsigned long long>(j, nchunks, es, st);
    else scatter_launch<unsigned>(j, nchunks, es, st);
    PN2_LAUNCH_CHECK("compact_scatter_kernel");
    return PN2_OK;
}

template <typename T, int MODE>
static void pair_launch(const void *pts, int64_t ld, const int *qsel, const int64_t *nq_dev, int64_t nq_host,
                        const int *csel, const int64_t *nc_dev, int64_t nc_host, double r2, int *out, int *parent,
                        const int *clabel, hipStream_t st) {
    hipLaunchKernelGGL((collect_pair_kernel<T, MODE>), dim3((unsigned)((nq_host + kPairSlab - 1) / kPairSlab)),
                       dim3(kPairThreads), 0, st, static_cast<const T *>(pts), ld, qsel, nq_dev, (int)nq_host, csel,
                       nc_dev, (int)nc_host, r2, out, parent, clabel);
}

// the int32 arrays of pn2_dbscan_labels' workspace, each padded to 16 bytes
struct DbscanWs {
    int *core_idx, *border_idx, *parent, *root, *isroot, *rank, *clabel, *table;
    int64_t *off_core, *off_border, *off_root;  // [2] each: {0, count}
};
static int64_t dbscan_ws_bytes(int64_t N) { return 7 * align16(N * 4) + align16(chunks_of(N) * 4) + 3 * 16; }
static DbscanWs dbscan_ws(void *ws, int64_t N) {
    char *p = static_cast<char *>(ws);
    DbscanWs w;
    int **arrays[7] = {&w.core_idx, &w.border_idx, &w.parent, &w.root, &w.isroot, &w.rank, &w.clabel};
    for (int k = 0; k < 7; ++k) *arrays[k] = reinterpret_cast<int *>(p), p += align16(N * 4);
    w.table = reinterpret_cast<int *>(p), p += align16(chunks_of(N) * 4);
    w.off_core = reinterpret_cast<int64_t *>(p), p += 16;
    w.off_border = reinterpret_cast<int64_t *>(p), p += 16;
    w.off_root = reinterpret_cast<int64_t *>(p);
    return w;
}

template <typename T>
static int dbscan_run(const void *pts, int64_t N, int64_t ld, double r2, int64_t min_points, const int *counts,
                      int *labels, int64_t *nclusters, void *ws, unsigned *err, hipStream_t st) {
    const DbscanWs w = dbscan_ws(ws, N);
    const unsigned grid = (unsigned)((N + 255) / 256);
    // core points (count >= min_points) and the others, as ascending index lists
    CompactJob core = {nullptr, 0, N, nullptr, 0, 0, counts, PN2_COMPACT_FLAG_GT, min_points - 1, 1,
                       nullptr, w.core_idx, nullptr, w.off_core, w.table};
    int rc = compact_run(core, err, st);
    if (rc != PN2_OK) return rc;
    CompactJob border = core;
    border.mode = PN2_COMPACT_FLAG_LE, border.out_src = w.border_idx, border.offsets = w.off_border;
    if ((rc = compact_run(border, err, st)) != PN2_OK) return rc;
    const int64_t *m_dev = w.off_core + 1;
    hipLaunchKernelGGL(uf_init_kernel, dim3(grid), dim3(256), 0, st, w.parent, (int)N);
    PN2_LAUNCH_CHECK("uf_init_kernel");
    pair_launch<T, PAIR_UNION>(pts, ld, w.core_idx, m_dev, N, w.core_idx, m_dev, N, r2, nullptr, w.parent, nullptr, st);
    PN2_LAUNCH_CHECK("collect_pair_kernel<UNION>");
    hipLaunchKernelGGL(uf_flatten_kernel, dim3(grid), dim3(256), 0, st, w.parent, m_dev, (int)N, w.root, w.isroot);
    PN2_LAUNCH_CHECK("uf_flatten_kernel");
    CompactJob roots = {nullptr, 0, N, m_dev, 0, 0, w.isroot, PN2_COMPACT_FLAG_GT, 0, 1,
                        nullptr, nullptr, w.rank, w.off_root, w.table};
    if ((rc = compact_run(roots, err, st)) != PN2_OK) return rc;
    hipLaunchKernelGGL(core_label_kernel, dim3(grid), dim3(256), 0, st, w.root, w.rank, w.core_idx, m_dev, (int)N,
                       w.off_root + 1, w.clabel, labels, nclusters);
    PN2_LAUNCH_CHECK("core_label_kernel");
    pair_launch<T, PAIR_BORDER>(pts, ld, w.border_idx, w.off_border + 1, N, w.core_idx, m_dev, N, r2, labels, nullptr,
                                w.clabel, st);
    PN2_LAUNCH_CHECK("collect_pair_kernel<BORDER>");
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_collect_max_points(void) { return kCollectMaxN; }

extern "C" int pn2_clip_flags(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, int64_t axis, double lo,
                              double hi, int32_t *flags, void *stream) {
    PN2_REQUIRE(pts && flags, "pn2_clip_flags: null pointer");
    const int rc = check_cloud("pn2_clip_flags", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(axis >= 0 && axis < C, "pn2_clip_flags: axis %lld outside [0, C=%lld)", (long long)axis, (long long)C);
    if (N == 0) return PN2_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((N + 255) / 256));
    if (dtype == PN2_DTYPE_F64)
        hipLaunchKernelGGL(clip_flags_kernel<double>, grid, dim3(256), 0, st, static_cast<const double *>(pts), ld,
                           (int)N, (int)axis, lo, hi, flags);
    else
        hipLaunchKernelGGL(clip_flags_kernel<float>, grid, dim3(256), 0, st, static_cast<const float *>(pts), ld,
                           (int)N, (int)axis, lo, hi, flags);
    PN2_LAUNCH_CHECK("clip_flags_kernel");
    return PN2_OK;
}

extern "C" int pn2_radius_count_f64(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, double radius,
                                    int32_t *counts, void *stream) {
    PN2_REQUIRE(pts && counts, "pn2_radius_count_f64: null pointer");
    const int rc = check_cloud("pn2_radius_count_f64", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    if (N == 0) return PN2_OK;
    const double r2 = radius * radius;  // one float64 product
    hipStream_t st = as_stream(stream);
    if (dtype == PN2_DTYPE_F64)
        pair_launch<double, PAIR_COUNT>(pts, ld, nullptr, nullptr, N, nullptr, nullptr, N, r2, counts, nullptr, nullptr, st);
    else
        pair_launch<float, PAIR_COUNT>(pts, ld, nullptr, nullptr, N, nullptr, nullptr, N, r2, counts, nullptr, nullptr, st);
    PN2_LAUNCH_CHECK("collect_pair_kernel<COUNT>");
    return PN2_OK;
}

extern "C" int64_t pn2_compact_rows_workspace_bytes(int64_t N, int64_t L) {
    if (N < 0 || N > kCollectMaxN || L < 1 || chunks_of(N) * L > kCompactMaxEntries) return -1;
    return align16(chunks_of(N) * L * 4);
}

extern "C" int pn2_compact_rows(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, const int32_t *keys,
                                int mode, int64_t thresh, int64_t L, void *out_rows, int32_t *out_src,
                                int64_t *offsets, void *workspace, int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && keys && out_rows && offsets, "pn2_compact_rows: null pointer");
    const int rc = check_cloud("pn2_compact_rows", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(mode == PN2_COMPACT_FLAG_GT || mode == PN2_COMPACT_LABEL || mode == PN2_COMPACT_FLAG_LE,
                "pn2_compact_rows: unknown mode %d", mode);
    PN2_REQUIRE(L >= 1 && (mode == PN2_COMPACT_LABEL || L == 1) && thresh >= INT32_MIN && thresh <= INT32_MAX,
                "pn2_compact_rows: bad buckets (mode=%d L=%lld thresh=%lld)", mode, (long long)L, (long long)thresh);
    const int64_t need = pn2_compact_rows_workspace_bytes(N, L);
    if (need < 0)
        return set_error(PN2_EUNSUPPORTED, "pn2_compact_rows: %lld chunks x %lld buckets above %lld table entries",
                         (long long)chunks_of(N), (long long)L, (long long)kCompactMaxEntries);
    if (N == 0) return PN2_OK;
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_compact_rows: workspace too small: needs pn2_compact_rows_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    hipStream_t st = as_stream(stream);
    unsigned *err = error_word(st);
    PN2_REQUIRE(err, "pn2_compact_rows: no device error slot");
    const CompactJob j = {pts, dtype, N, nullptr, C, ld, keys, mode, thresh, L,
                          out_rows, out_src, nullptr, offsets, static_cast<int *>(workspace)};
    return compact_run(j, err, st);
}

extern "C" int64_t pn2_dbscan_labels_workspace_bytes(int64_t N) {
    if (N < 0 || N > kCollectMaxN) return -1;
    return dbscan_ws_bytes(N);
}

extern "C" int pn2_dbscan_labels(const void *pts, int dtype, int64_t N, int64_t C, int64_t ld, double eps,
                                 int64_t min_points, const int32_t *counts, int32_t *labels, int64_t *nclusters,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(pts && counts && labels && nclusters, "pn2_dbscan_labels: null pointer");
    const int rc = check_cloud("pn2_dbscan_labels", pts, dtype, N, C, ld);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(min_points > INT32_MIN && min_points <= INT32_MAX, "pn2_dbscan_labels: bad min_points %lld",
                (long long)min_points);
    if (N == 0) return PN2_OK;
    const int64_t need = dbscan_ws_bytes(N);
    PN2_REQUIRE(ws_fits(workspace, workspace_bytes, need),
                "pn2_dbscan_labels: workspace too small: needs pn2_dbscan_labels_workspace_bytes = %lld bytes, "
                "16-byte aligned", (long long)need);
    hipStream_t st = as_stream(stream);
    unsigned *err = error_word(st);
    PN2_REQUIRE(err, "pn2_dbscan_labels: no device error slot");
    const double r2 = eps * eps;
    if (dtype == PN2_DTYPE_F64)
        return dbscan_run<double>(pts, N, ld, r2, min_points, counts, labels, nclusters, workspace, err, st);
    return dbscan_run<float>(pts, N, ld, r2, min_points, counts, labels, nclusters, workspace, err, st);
}
