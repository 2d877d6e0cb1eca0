// v1_transform.hip -- the per-cloud transforms of the PointNet-v1 networks and their
// orthogonality regulariser under autograd (include/pn2.h states the contracts and the order
// rules):
//   pn2_transform_points_f32            y[b,n,:] = T[b] x[b,n,:]            torch.bmm(trans, x)
//   pn2_transform_points_backward_f32   dx = T[b]^T dy, dT[b] = sum_n dy x^T  (its backward)
//   pn2_orthogonality_forward_f32       mean_b || T[b] T[b]^T - I ||_F
//   pn2_orthogonality_backward_f32      its gradient
//
// Reference: model/pointnet_utils.py:102-113, 120-123 (the 3x3 input transform and the 64x64
// feature transform), :140-147 (feature_transform_reguliarzer), pose.py:50-69.
//
// Shapes: k is 3 or 64 in the reference (1 .. 64 here), N 1024 .. 10240 points, B a few to a
// few dozen clouds.  All of it is bandwidth or latency, none of it matrix-core work: plain
// float32 / float64 VALU arithmetic, one operation per rounding.
//   transform (forward and dx): a workgroup takes 64 rows of one cloud.  The tile and T[b] (for
//     dx: its transpose) go to LDS; lane = row, wave = a quarter of the outputs, so T is a
//     wave-uniform broadcast read and the tile a conflict-free one (odd row pitch).  An output
//     is ONE fma chain inside one lane: row independence and the order hold by construction.
//     The results leave through an LDS tile so that either layout stores coalesced.
//   dT: a workgroup takes one slab of kSlabRows rows of one cloud, 64 rows at a time through
//     LDS, and a thread owns up to 16 (i,j) pairs, each ONE float64 chain over the slab's rows.
//     The partials go to the workspace; a second launch adds them in slab order.
//   regulariser: a workgroup per cloud; G in LDS; thread 0 walks the one float64 chain of the
//     norm.  The mean over the clouds is a second, single-thread launch (no workgroup reads
//     another's result inside a launch).
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile): an fma is only where
// __fmaf_rn / __fma_rn says so, everything else rounds on its own.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kTfThreads = 256;
constexpr int kTfMaxK = 64;
constexpr int kTfTile = 64;               // rows of a tile: a lane per row
constexpr int kTfPitchMax = kTfMaxK + 1;  // LDS row pitch is k + 1 (odd at k = 64)
constexpr int kSlabRows = 128;            // R of the dT rule
constexpr int64_t kTfMaxDim = 1ll << 30;  // B, N: tiles and slabs are counted in an int32

// how a [rows, k] tile of a strided tensor is walked (chosen on the host from base and strides)
enum TileMode {
    kScalarC = 0,  // dword accesses, the channel index fastest (sc == 1, or nothing contiguous)
    kScalarN = 1,  // dword accesses, the row index fastest (sn == 1: channel-first)
    kVecC = 2,     // 16-byte accesses along the channels (sc == 1, k % 4 == 0, all aligned)
    kVecN = 3      // 16-byte accesses along the rows (sn == 1, all aligned; a short tail by dwords)
};

struct Strided {
    const float *p;
    int64_t sb, sn, sc;
    int mode;
};

// global [rows, k] at g (row stride sn, channel stride sc) -> LDS tile t (row pitch k + 1)
__device__ __forceinline__ void load_tile(float *__restrict__ t, const float *__restrict__ g, int64_t sn, int64_t sc,
                                          int rows, int k, int mode) {
    const int tid = threadIdx.x, pitch = k + 1;
    if (mode == kVecC) {
        const int kq = k >> 2;
        for (int e = tid; e < rows * kq; e += kTfThreads) {
            const int r = e / kq, c = (e - r * kq) << 2;
            const float4 v = *reinterpret_cast<const float4 *>(g + r * sn + c);
            float *d = t + r * pitch + c;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
    } else if (mode == kVecN) {
        const int rq = (rows + 3) >> 2;
        for (int e = tid; e < rq * k; e += kTfThreads) {
            const int c = e / rq, r = (e - c * rq) << 2;
            const float *s = g + c * sc + r;
            if (r + 3 < rows) {
                const float4 v = *reinterpret_cast<const float4 *>(s);
                t[r * pitch + c] = v.x, t[(r + 1) * pitch + c] = v.y;
                t[(r + 2) * pitch + c] = v.z, t[(r + 3) * pitch + c] = v.w;
            } else {
                for (int q = 0; r + q < rows; ++q) t[(r + q) * pitch + c] = s[q];
            }
        }
    } else if (mode == kScalarN) {
        for (int e = tid; e < rows * k; e += kTfThreads) {
            const int c = e / rows, r = e - c * rows;
            t[r * pitch + c] = g[r * sn + c * sc];
        }
    } else {
        for (int e = tid; e < rows * k; e += kTfThreads) {
            const int r = e / k, c = e - r * k;
            t[r * pitch + c] = g[r * sn + c * sc];
        }
    }
}

__device__ __forceinline__ void store_tile(const float *__restrict__ t, float *__restrict__ g, int64_t sn, int64_t sc,
                                           int rows, int k, int mode) {
    const int tid = threadIdx.x, pitch = k + 1;
    if (mode == kVecC) {
        const int kq = k >> 2;
        for (int e = tid; e < rows * kq; e += kTfThreads) {
            const int r = e / kq, c = (e - r * kq) << 2;
            const float *s = t + r * pitch + c;
            *reinterpret_cast<float4 *>(g + r * sn + c) = make_float4(s[0], s[1], s[2], s[3]);
        }
    } else if (mode == kVecN) {
        const int rq = (rows + 3) >> 2;
        for (int e = tid; e < rq * k; e += kTfThreads) {
            const int c = e / rq, r = (e - c * rq) << 2;
            float *d = g + c * sc + r;
            if (r + 3 < rows) {
                *reinterpret_cast<float4 *>(d) = make_float4(t[r * pitch + c], t[(r + 1) * pitch + c],
                                                             t[(r + 2) * pitch + c], t[(r + 3) * pitch + c]);
            } else {
                for (int q = 0; r + q < rows; ++q) d[q] = t[(r + q) * pitch + c];
            }
        }
    } else if (mode == kScalarN) {
        for (int e = tid; e < rows * k; e += kTfThreads) {
            const int c = e / rows, r = e - c * rows;
            g[r * sn + c * sc] = t[r * pitch + c];
        }
    } else {
        for (int e = tid; e < rows * k; e += kTfThreads) {
            const int r = e / k, c = e - r * k;
            g[r * sn + c * sc] = t[r * pitch + c];
        }
    }
}

// ------------------------------------------------------------------------------ y = T x, dx = T^T dy
// out[n][o] = sum_r M[o][r] * in[n][r], r ascending from +0.0f, M = T[b] (transposed: T[b]^T).
// NACC: outputs per lane, ceil(k / 4) rounded up to 1, 4 or 16 (the accumulators stay in VGPRs).
template <int NACC>
__global__ __launch_bounds__(kTfThreads) void transform_kernel(Strided in, const float *__restrict__ T, int64_t ldt,
                                                               int transposed, float *__restrict__ out, int64_t osb,
                                                               int64_t osn, int64_t osc, int omode, int N, int k,
                                                               int tiles) {
    __shared__ float Ms[kTfMaxK * kTfMaxK];     // [o][r], pitch k
    __shared__ float xs[kTfTile * kTfPitchMax];
    __shared__ float ys[kTfTile * kTfPitchMax];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int n0 = tile * kTfTile;
    const int rows = N - n0 < kTfTile ? N - n0 : kTfTile;
    const int tid = threadIdx.x, pitch = k + 1;
    const float *Tb = T + (int64_t)b * k * ldt;
    for (int e = tid; e < k * k; e += kTfThreads) {
        const int i = e / k, j = e - i * k;
        const float v = Tb[i * ldt + j];
        Ms[transposed ? j * k + i : e] = v;
    }
    load_tile(xs, in.p + (int64_t)b * in.sb + (int64_t)n0 * in.sn, in.sn, in.sc, rows, k, in.mode);
    __syncthreads();
    const int lane = tid & 63, g = tid >> 6;  // lane = row, wave g: outputs g, g + 4, ...
    if (lane < rows) {
        float acc[NACC];
#pragma unroll
        for (int q = 0; q < NACC; ++q) acc[q] = 0.f;
        const float *xr = xs + lane * pitch;
        for (int r = 0; r < k; ++r) {
            const float xv = xr[r];
#pragma unroll
            for (int q = 0; q < NACC; ++q) {
                const int o = g + 4 * q;
                if (o < k) acc[q] = __fmaf_rn(Ms[o * k + r], xv, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int o = g + 4 * q;
            if (o < k) ys[lane * pitch + o] = acc[q];
        }
    }
    __syncthreads();
    store_tile(ys, out + (int64_t)b * osb + (int64_t)n0 * osn, osn, osc, rows, k, omode);
}

// ------------------------------------------------------------------------------ dT
// slab partials: P[b][s][i][j] = sum_n double(dy[n][i]) * double(x[n][j]) over the slab's rows in
// ascending n from +0.0 (the product is exact in float64, so the fma rounds what the add would).
// NACC: (i,j) pairs per thread, ceil(k*k / 256) rounded up to 1, 4 or 16.
template <int NACC>
__global__ __launch_bounds__(kTfThreads) void transform_dT_slab_kernel(Strided dy, Strided x, double *__restrict__ P,
                                                                       int N, int k, int slabs) {
    __shared__ float ds[kTfTile * kTfPitchMax];
    __shared__ float xs[kTfTile * kTfPitchMax];
    const int b = blockIdx.x / slabs, s = blockIdx.x - b * slabs;
    const int lo = s * kSlabRows;
    const int hi = N - lo < kSlabRows ? N : lo + kSlabRows;
    const int tid = threadIdx.x, pitch = k + 1, kk = k * k;
    int pi[NACC], pj[NACC];
    double acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        const int p = tid + kTfThreads * q;
        const int pp = p < kk ? p : 0;
        pi[q] = pp / k;
        pj[q] = pp - pi[q] * k;
        acc[q] = 0.0;
    }
    for (int n0 = lo; n0 < hi; n0 += kTfTile) {
        const int rows = hi - n0 < kTfTile ? hi - n0 : kTfTile;
        load_tile(ds, dy.p + (int64_t)b * dy.sb + (int64_t)n0 * dy.sn, dy.sn, dy.sc, rows, k, dy.mode);
        load_tile(xs, x.p + (int64_t)b * x.sb + (int64_t)n0 * x.sn, x.sn, x.sc, rows, k, x.mode);
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
#pragma unroll
            for (int q = 0; q < NACC; ++q)
                acc[q] = __fma_rn((double)ds[r * pitch + pi[q]], (double)xs[r * pitch + pj[q]], acc[q]);
        }
        __syncthreads();
    }
    double *Pb = P + ((int64_t)b * slabs + s) * kk;
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        const int p = tid + kTfThreads * q;
        if (p < kk) Pb[p] = acc[q];
    }
}

// dT[b][i][j] = float32(sum_s P[b][s][i][j]) in ascending s from +0.0
__global__ __launch_bounds__(kTfThreads) void transform_dT_reduce_kernel(const double *__restrict__ P,
                                                                         float *__restrict__ dT, int64_t total, int kk,
                                                                         int slabs) {
    const int64_t e = (int64_t)blockIdx.x * kTfThreads + threadIdx.x;
    if (e >= total) return;
    const int64_t b = e / kk, p = e - b * kk;
    const double *src = P + b * slabs * kk + p;
    double acc = 0.0;
    for (int s = 0; s < slabs; ++s) acc = acc + src[(int64_t)s * kk];
    dT[e] = (float)acc;
}

// ------------------------------------------------------------------------------ regulariser
// T[b] -> Ts (pitch k + 1), G[b] = T T^T - I -> Gs (pitch k)
__device__ __forceinline__ void gram_minus_identity(const float *__restrict__ Tb, int64_t ldt, int k, float *Ts,
                                                    float *Gs) {
    const int tid = threadIdx.x, pitch = k + 1;
    for (int e = tid; e < k * k; e += kTfThreads) {
        const int i = e / k, j = e - i * k;
        Ts[i * pitch + j] = Tb[i * ldt + j];
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += kTfThreads) {
        const int i = e / k, j = e - i * k;
        float acc = 0.f;
        for (int l = 0; l < k; ++l) acc = __fmaf_rn(Ts[i * pitch + l], Ts[j * pitch + l], acc);
        Gs[e] = i == j ? acc - 1.0f : acc;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kTfThreads) void ortho_fwd_kernel(const float *__restrict__ T, int64_t ldt, int k,
                                                               float *__restrict__ G, float *__restrict__ norm) {
    __shared__ float Ts[kTfMaxK * kTfPitchMax];
    __shared__ float Gs[kTfMaxK * kTfMaxK];
    const int b = blockIdx.x, tid = threadIdx.x, kk = k * k;
    gram_minus_identity(T + (int64_t)b * k * ldt, ldt, k, Ts, Gs);
    if (G)
        for (int e = tid; e < kk; e += kTfThreads) G[(int64_t)b * kk + e] = Gs[e];
    if (tid == 0) {
        double acc = 0.0;  // THE chain of this cloud's norm: row-major (i, j)
        for (int e = 0; e < kk; ++e) {
            const double g = (double)Gs[e];
            acc = acc + g * g;  // the square of a float32 is exact in float64
        }
        norm[b] = (float)__dsqrt_rn(acc);
    }
}

__global__ void ortho_mean_kernel(const float *__restrict__ norm, int B, float *__restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (int b = 0; b < B; ++b) acc = acc + (double)norm[b];
    *loss = (float)(acc / (double)B);
}

__global__ __launch_bounds__(kTfThreads) void ortho_bwd_kernel(const float *__restrict__ T, int64_t ldt,
                                                               const float *__restrict__ norm,
                                                               const float *__restrict__ dloss, int B, int k,
                                                               float *__restrict__ dT) {
    __shared__ float Ts[kTfMaxK * kTfPitchMax];
    __shared__ float Gs[kTfMaxK * kTfMaxK];
    const int b = blockIdx.x, tid = threadIdx.x, kk = k * k, pitch = k + 1;
    gram_minus_identity(T + (int64_t)b * k * ldt, ldt, k, Ts, Gs);
    const float nb = norm[b];
    // a zero norm: torch's backward of the norm fills the gradient with zeros there
    const float c = nb == 0.f ? 0.f : (float)((2.0 * (double)dloss[0]) / ((double)B * (double)nb));
    for (int e = tid; e < kk; e += kTfThreads) {
        const int i = e / k, j = e - i * k;
        float acc = 0.f;
        for (int l = 0; l < k; ++l) acc = __fmaf_rn(Gs[i * k + l], Ts[l * pitch + j], acc);
        dT[(int64_t)b * kk + e] = acc * c;
    }
}

// ------------------------------------------------------------------------------ host
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int tile_mode(const float *p, int64_t sb, int64_t sn, int64_t sc, int64_t k) {
    if (sc == 1) return (k % 4 == 0 && sn % 4 == 0 && sb % 4 == 0 && aligned16(p)) ? kVecC : kScalarC;
    if (sn == 1) return (sc % 4 == 0 && sb % 4 == 0 && aligned16(p)) ? kVecN : kScalarN;
    return kScalarC;
}

static int transform_shape(const char *what, int64_t B, int64_t N, int64_t k) {
    if (B < 1 || N < 1 || k < 1)
        return set_error(PN2_EINVAL, "%s: bad shape B=%lld N=%lld k=%lld", what, (long long)B, (long long)N,
                         (long long)k);
    if (k > kTfMaxK) return set_error(PN2_EUNSUPPORTED, "%s: k=%lld above %d", what, (long long)k, kTfMaxK);
    if (B > kTfMaxDim || N > kTfMaxDim || B * ((N + kTfTile - 1) / kTfTile) > 0x7fffffffll)
        return set_error(PN2_EUNSUPPORTED, "%s: B=%lld N=%lld above 2^30, or more than 2^31 - 1 row tiles", what,
                         (long long)B, (long long)N);
    return PN2_OK;
}

static int launch_transform(const char *what, const float *in, int64_t isb, int64_t isn, int64_t isc, const float *T,
                            int64_t ldt, int transposed, float *out, int64_t osb, int64_t osn, int64_t osc, int64_t B,
                            int64_t N, int64_t k, hipStream_t st) {
    const Strided src{in, isb, isn, isc, tile_mode(in, isb, isn, isc, k)};
    const int omode = tile_mode(out, osb, osn, osc, k);
    const int tiles = (int)((N + kTfTile - 1) / kTfTile);
    const dim3 grid((unsigned)(B * tiles)), block(kTfThreads);
    if (k <= 4)
        hipLaunchKernelGGL(transform_kernel<1>, grid, block, 0, st, src, T, ldt, transposed, out, osb, osn, osc, omode,
                           (int)N, (int)k, tiles);
    else if (k <= 16)
        hipLaunchKernelGGL(transform_kernel<4>, grid, block, 0, st, src, T, ldt, transposed, out, osb, osn, osc, omode,
                           (int)N, (int)k, tiles);
    else
        hipLaunchKernelGGL(transform_kernel<16>, grid, block, 0, st, src, T, ldt, transposed, out, osb, osn, osc,
                           omode, (int)N, (int)k, tiles);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_transform_slab_rows(void) { return kSlabRows; }

extern "C" int64_t pn2_transform_workspace_bytes(int64_t B, int64_t N, int64_t k) {
    if (B < 1 || N < 1 || k < 1 || k > kTfMaxK || B > kTfMaxDim || N > kTfMaxDim) return -1;
    return B * ((N + kSlabRows - 1) / kSlabRows) * k * k * (int64_t)sizeof(double);
}

extern "C" int pn2_transform_points_f32(const float *x, int64_t xsb, int64_t xsn, int64_t xsc, const float *T,
                                        int64_t ldt, float *y, int64_t ysb, int64_t ysn, int64_t ysc, int64_t B,
                                        int64_t N, int64_t k, void *stream) {
    const char *what = "pn2_transform_points_f32";
    PN2_REQUIRE(x && T && y, "%s: null pointer", what);
    const int rc = transform_shape(what, B, N, k);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(xsb >= 0 && xsn >= 0 && xsc >= 0 && ysb >= 0 && ysn >= 0 && ysc >= 0, "%s: negative stride", what);
    PN2_REQUIRE(ldt >= k, "%s: T's row stride is below k", what);
    return launch_transform(what, x, xsb, xsn, xsc, T, ldt, 0, y, ysb, ysn, ysc, B, N, k, as_stream(stream));
}

extern "C" int pn2_transform_points_backward_f32(const float *dy, int64_t dsb, int64_t dsn, int64_t dsc,
                                                 const float *x, int64_t xsb, int64_t xsn, int64_t xsc,
                                                 const float *T, int64_t ldt, float *dx, int64_t gsb, int64_t gsn,
                                                 int64_t gsc, float *dT, int64_t B, int64_t N, int64_t k,
                                                 void *workspace, int64_t workspace_bytes, void *stream) {
    const char *what = "pn2_transform_points_backward_f32";
    PN2_REQUIRE(dy && (dx || dT), "%s: null pointer", what);
    PN2_REQUIRE(!dx || T, "%s: null pointer (dx needs T)", what);
    PN2_REQUIRE(!dT || (x && workspace), "%s: null pointer (dT needs x and the workspace)", what);
    const int rc = transform_shape(what, B, N, k);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(dsb >= 0 && dsn >= 0 && dsc >= 0, "%s: negative stride", what);
    const hipStream_t st = as_stream(stream);
    if (dT) {
        PN2_REQUIRE(xsb >= 0 && xsn >= 0 && xsc >= 0, "%s: negative stride", what);
        PN2_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: the workspace is not 8-byte aligned", what);
        PN2_REQUIRE(workspace_bytes >= pn2_transform_workspace_bytes(B, N, k),
                    "%s: workspace of %lld bytes, %lld needed", what, (long long)workspace_bytes,
                    (long long)pn2_transform_workspace_bytes(B, N, k));
    }
    if (dx) {
        PN2_REQUIRE(gsb >= 0 && gsn >= 0 && gsc >= 0, "%s: negative stride", what);
        PN2_REQUIRE(ldt >= k, "%s: T's row stride is below k", what);
        const int rd = launch_transform(what, dy, dsb, dsn, dsc, T, ldt, 1, dx, gsb, gsn, gsc, B, N, k, st);
        if (rd != PN2_OK) return rd;
    }
    if (dT) {
        const Strided d{dy, dsb, dsn, dsc, tile_mode(dy, dsb, dsn, dsc, k)};
        const Strided xx{x, xsb, xsn, xsc, tile_mode(x, xsb, xsn, xsc, k)};
        const int slabs = (int)((N + kSlabRows - 1) / kSlabRows);
        double *P = static_cast<double *>(workspace);
        const dim3 grid((unsigned)(B * slabs)), block(kTfThreads);
        if (k * k <= kTfThreads)
            hipLaunchKernelGGL(transform_dT_slab_kernel<1>, grid, block, 0, st, d, xx, P, (int)N, (int)k, slabs);
        else if (k * k <= 4 * kTfThreads)
            hipLaunchKernelGGL(transform_dT_slab_kernel<4>, grid, block, 0, st, d, xx, P, (int)N, (int)k, slabs);
        else
            hipLaunchKernelGGL(transform_dT_slab_kernel<16>, grid, block, 0, st, d, xx, P, (int)N, (int)k, slabs);
        PN2_LAUNCH_CHECK(what);
        const int64_t total = B * k * k;
        hipLaunchKernelGGL(transform_dT_reduce_kernel, dim3((unsigned)((total + kTfThreads - 1) / kTfThreads)), block,
                           0, st, P, dT, total, (int)(k * k), slabs);
        PN2_LAUNCH_CHECK(what);
    }
    return PN2_OK;
}

static int ortho_shape(const char *what, int64_t B, int64_t k, int64_t ldt) {
    if (B < 1 || k < 1) return set_error(PN2_EINVAL, "%s: bad shape B=%lld k=%lld", what, (long long)B, (long long)k);
    if (k > kTfMaxK) return set_error(PN2_EUNSUPPORTED, "%s: k=%lld above %d", what, (long long)k, kTfMaxK);
    if (B > kTfMaxDim) return set_error(PN2_EUNSUPPORTED, "%s: B=%lld above 2^30", what, (long long)B);
    PN2_REQUIRE(ldt >= k, "%s: T's row stride is below k", what);
    return PN2_OK;
}

extern "C" int pn2_orthogonality_forward_f32(const float *T, int64_t ldt, int64_t B, int64_t k, float *G, float *norm,
                                             float *loss, void *stream) {
    const char *what = "pn2_orthogonality_forward_f32";
    PN2_REQUIRE(T && norm && loss, "%s: null pointer", what);
    const int rc = ortho_shape(what, B, k, ldt);
    if (rc != PN2_OK) return rc;
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(ortho_fwd_kernel, dim3((unsigned)B), dim3(kTfThreads), 0, st, T, ldt, (int)k, G, norm);
    PN2_LAUNCH_CHECK(what);
    hipLaunchKernelGGL(ortho_mean_kernel, dim3(1), dim3(64), 0, st, norm, (int)B, loss);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

extern "C" int pn2_orthogonality_backward_f32(const float *T, int64_t ldt, const float *norm, const float *dloss,
                                              int64_t B, int64_t k, float *dT, void *stream) {
    const char *what = "pn2_orthogonality_backward_f32";
    PN2_REQUIRE(T && norm && dloss && dT, "%s: null pointer", what);
    const int rc = ortho_shape(what, B, k, ldt);
    if (rc != PN2_OK) return rc;
    hipLaunchKernelGGL(ortho_bwd_kernel, dim3((unsigned)B), dim3(kTfThreads), 0, as_stream(stream), T, ldt, norm,
                       dloss, (int)B, (int)k, dT);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}
