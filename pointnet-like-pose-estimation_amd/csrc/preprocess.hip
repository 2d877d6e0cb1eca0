// preprocess.hip -- the input preparation the reference's scripts run on the host before every
// forward, as one kernel writing the model's input in HBM.
//
// Reference sequence (test_translation.py:72-79, test_rotation.py:71-77, train_*.py:113-118
// without the augmentations; /root/reference/provider.py):
//   points = points.data.numpy()                 float64 [B,N,C] (np.loadtxt rows)
//   mean   = np.mean(points[:, :3, :], axis=1)   translation heads only: the first 3 POINTS
//   points[:, :, 0:3] = provider.normalization(points[:, :, 0:3])        provider.py:5-21
//   points = torch.Tensor(points)                float32 (round to nearest even)
//   points = provider.splice_torch(points, label)                        provider.py:166-180
//   points = points.transpose(2, 1)              [B, C+K, N] view of [B, N, C+K] storage
//
// normalization() per cloud, in float64 with numpy's operation order (measured here,
// tests/test_preprocess.py): centroid = np.mean(pc, axis=0) -- an axis-0 reduction adds the
// rows sequentially, starting from row 0, then divides by N; pc - centroid; pc ** 2 is x*x;
// np.sum(axis=1) over 3 columns is ((x2 + y2) + z2); sqrt is correctly rounded; the max is
// exact (NaN propagates); pc / m is a correctly rounded division.  The unit is built without
// FMA contraction (Makefile GEOFLAGS), so every op rounds separately as numpy's do.
//
// The training loops run the same sequence after augmenting the batch (train_translation.py:
// 109-119); prepare_train_kernel is the same body reading the augmented values (prep_at below).
//
// One workgroup per cloud.  The two sequential sums (centroid over N points, mean over the
// first 3) are inherently serial in numpy's rounding order: a few lanes of wave 0 run them
// (the centroid from LDS chunks the other waves stage ahead); everything else is per point.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kPrepThreads = 256;
constexpr int kPrepChunk = 1024;  // points per LDS chunk of the centroid sum (2 x 24 KB)

__device__ __forceinline__ double nan_max(double a, double b) {
    return (a > b || a != a) ? a : b;  // np.max: NaN wins
}

// The training scripts' augmentations (train_translation.py:110-112; provider.py:157-164,
// 144-155, 131-142) are folded into the loads: every pass of the body reads point n, channel c
// as at(row(n), c), which restates, per element, what the reference leaves in `points` before
// the mean:
//   random_point_dropout     row n is row 0's (all C channels) where drop[n]
//   random_scale_point_cloud xyz *= scale[b]      one rounded multiply
//   shift_point_cloud        xyz += shift[b][c]   one rounded add
// A null drop / scale / shift skips that stage (x + 0.0 would turn -0.0 into +0.0).  AUG = false
// is the plain read of the eval scripts' entry.
//
// One cloud's draws.  Three scalars for the shift, not an array (a runtime channel index would
// put it on the stack), and handed to prep_at by value: written as members of the body's own
// closures, the select between them compiled to a select of stack addresses.
struct PrepAug {
    const uint8_t *drop;  // this cloud's [N], or null
    bool has_scale, has_shift;
    double scale, sh0, sh1, sh2;
};

template <bool AUG>
__device__ __forceinline__ int64_t prep_row(const PrepAug a, int64_t n) {
    if constexpr (AUG) return (a.drop && a.drop[n]) ? 0 : n;
    return n;
}

template <bool AUG>
__device__ __forceinline__ double prep_at(const PrepAug a, const double *P, int64_t sn, int64_t sc,
                                          int64_t r, int c) {
    double v = P[r * sn + (int64_t)c * sc];
    if constexpr (AUG) {
        if (a.has_scale && c < 3) v = __dmul_rn(v, a.scale);
        if (a.has_shift && c < 3) v = __dadd_rn(v, c == 0 ? a.sh0 : c == 1 ? a.sh1 : a.sh2);
    }
    return v;
}

template <bool AUG>
__device__ __forceinline__ void prepare_body(
    const double *__restrict__ pts, int64_t N, int C, int64_t sb, int64_t sn, int64_t sc,
    const int64_t *__restrict__ labels, int K, int normalize, float *__restrict__ out,
    float *__restrict__ mean_out, const uint8_t *__restrict__ drop,
    const double *__restrict__ scale, const double *__restrict__ shift) {
    __shared__ double cen[3];
    __shared__ double chunk[2][kPrepChunk * 3];
    __shared__ double wmax[kPrepThreads / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const double *P = pts + b * sb;
    PrepAug aug = {nullptr, false, false, 1.0, 0.0, 0.0, 0.0};
    if constexpr (AUG) {
        aug.drop = drop ? drop + b * N : nullptr;
        aug.has_scale = scale != nullptr, aug.has_shift = shift != nullptr;
        if (scale) aug.scale = scale[b];
        if (shift) aug.sh0 = shift[b * 3], aug.sh1 = shift[b * 3 + 1], aug.sh2 = shift[b * 3 + 2];
    }
    auto row = [aug](int64_t n) __attribute__((always_inline)) { return prep_row<AUG>(aug, n); };
    auto at = [aug, P, sn, sc](int64_t r, int c) __attribute__((always_inline)) {
        return prep_at<AUG>(aug, P, sn, sc, r, c);
    };

    // mean of the first min(3, N) points, every channel (before normalising)
    if (mean_out && tid < C) {
        const int64_t cnt = N < 3 ? N : 3;
        double s = at(0, tid);
        for (int64_t n = 1; n < cnt; ++n) s = __dadd_rn(s, at(row(n), tid));
        mean_out[b * C + tid] = (float)__ddiv_rn(s, (double)cnt);
    }
    if (!normalize) {
        for (int64_t n = tid; n < N; n += kPrepThreads) {
            float *o = out + (b * N + n) * (C + K);
            const int64_t r = row(n);
            for (int c = 0; c < C; ++c) o[c] = (float)at(r, c);
            for (int k = 0; k < K; ++k) o[C + k] = (labels[b] == k) ? 1.f : 0.f;
        }
        return;
    }
    // centroid: sequential sum from row 0 by lanes 0..2 of wave 0, reading the cloud from LDS
    // in chunks that waves 1..3 stage one chunk ahead (double-buffered): the dependent add
    // chain, not global-load latency, sets the time
    {
        const int64_t nch = (N + kPrepChunk - 1) / kPrepChunk;
        auto stage = [&](int64_t k) __attribute__((always_inline)) {
            double *dst = chunk[k & 1];
            const int64_t n0 = k * kPrepChunk;
            const int64_t cnt = (N - n0 < kPrepChunk ? N - n0 : kPrepChunk) * 3;
            for (int64_t e = tid - 64; e < cnt; e += kPrepThreads - 64) {
                const int64_t n = n0 + e / 3;
                dst[e] = at(row(n), (int)(e % 3));
            }
        };
        if (tid >= 64) stage(0);
        __syncthreads();
        double s = 0.0;
        for (int64_t k = 0; k < nch; ++k) {
            if (tid >= 64) {
                if (k + 1 < nch) stage(k + 1);
            } else if (tid < 3) {
                const double *src = chunk[k & 1] + tid;
                const int cnt = (int)(N - k * kPrepChunk < kPrepChunk ? N - k * kPrepChunk : kPrepChunk);
                int j = 0;
                if (k == 0) s = src[0], j = 1;  // numpy starts from row 0
                for (; j + 8 <= cnt; j += 8) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = src[3 * (j + u)];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s = __dadd_rn(s, v[u]);
                }
                for (; j < cnt; ++j) s = __dadd_rn(s, src[3 * j]);
            }
            __syncthreads();
        }
        if (tid < 3) cen[tid] = __ddiv_rn(s, (double)N);
    }
    __syncthreads();
    const double c0 = cen[0], c1 = cen[1], c2 = cen[2];
    // m = max_n sqrt((x^2 + y^2) + z^2) of the centred points
    double m = -__builtin_inf();
    for (int64_t n = tid; n < N; n += kPrepThreads) {
        const int64_t r = row(n);
        const double x = __dsub_rn(at(r, 0), c0), y = __dsub_rn(at(r, 1), c1),
                     z = __dsub_rn(at(r, 2), c2);
        const double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
        m = nan_max(m, d);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = nan_max(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kPrepThreads / 64; ++w) m = nan_max(m, wmax[w]);
    // out row: normalised xyz, other channels as they are, one-hot of the label
    for (int64_t n = tid; n < N; n += kPrepThreads) {
        const int64_t r = row(n);
        float *o = out + (b * N + n) * (C + K);
        o[0] = (float)__ddiv_rn(__dsub_rn(at(r, 0), c0), m);
        o[1] = (float)__ddiv_rn(__dsub_rn(at(r, 1), c1), m);
        o[2] = (float)__ddiv_rn(__dsub_rn(at(r, 2), c2), m);
        for (int c = 3; c < C; ++c) o[c] = (float)at(r, c);
        for (int k = 0; k < K; ++k) o[C + k] = (labels[b] == k) ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(kPrepThreads) void prepare_kernel(
    const double *__restrict__ pts, int64_t N, int C, int64_t sb, int64_t sn, int64_t sc,
    const int64_t *__restrict__ labels, int K, int normalize, float *__restrict__ out,
    float *__restrict__ mean_out) {
    prepare_body<false>(pts, N, C, sb, sn, sc, labels, K, normalize, out, mean_out, nullptr,
                        nullptr, nullptr);
}

__global__ __launch_bounds__(kPrepThreads) void prepare_train_kernel(
    const double *__restrict__ pts, int64_t N, int C, int64_t sb, int64_t sn, int64_t sc,
    const int64_t *__restrict__ labels, int K, int normalize, float *__restrict__ out,
    float *__restrict__ mean_out, const uint8_t *__restrict__ drop,
    const double *__restrict__ scale, const double *__restrict__ shift) {
    prepare_body<true>(pts, N, C, sb, sn, sc, labels, K, normalize, out, mean_out, drop, scale,
                       shift);
}

}  // namespace pn2

using namespace pn2;

extern "C" int pn2_prepare_points_f64(const double *pts, int64_t B, int64_t N, int64_t C,
                                      int64_t sb, int64_t sn, int64_t sc, int normalize,
                                      const int64_t *labels, int64_t num_category, float *out,
                                      float *mean_out, void *stream) {
    PN2_REQUIRE(pts && out, "pn2_prepare_points_f64: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= (normalize ? 3 : 1) && C <= 64,
                "pn2_prepare_points_f64: bad shape (B=%lld N=%lld C=%lld)", (long long)B,
                (long long)N, (long long)C);
    PN2_REQUIRE(num_category >= 0 && num_category <= 1024 && (num_category == 0 || labels),
                "pn2_prepare_points_f64: bad num_category / labels");
    if (B == 0) return PN2_OK;
    hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)B), dim3(kPrepThreads), 0,
                       as_stream(stream), pts, N, (int)C, sb, sn, sc, labels, (int)num_category,
                       normalize ? 1 : 0, out, mean_out);
    PN2_LAUNCH_CHECK("prepare_kernel");
    return PN2_OK;
}

extern "C" int pn2_prepare_train_points_f64(const double *pts, int64_t B, int64_t N, int64_t C,
                                            int64_t sb, int64_t sn, int64_t sc, int normalize,
                                            const int64_t *labels, int64_t num_category,
                                            const uint8_t *drop, const double *scale,
                                            const double *shift, float *out, float *mean_out,
                                            void *stream) {
    PN2_REQUIRE(pts && out, "pn2_prepare_train_points_f64: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= (normalize ? 3 : 1) && C <= 64,
                "pn2_prepare_train_points_f64: bad shape (B=%lld N=%lld C=%lld)", (long long)B,
                (long long)N, (long long)C);
    PN2_REQUIRE(num_category >= 0 && num_category <= 1024 && (num_category == 0 || labels),
                "pn2_prepare_train_points_f64: bad num_category / labels");
    if (B == 0) return PN2_OK;
    hipLaunchKernelGGL(prepare_train_kernel, dim3((unsigned)B), dim3(kPrepThreads), 0,
                       as_stream(stream), pts, N, (int)C, sb, sn, sc, labels, (int)num_category,
                       normalize ? 1 : 0, out, mean_out, drop, scale, shift);
    PN2_LAUNCH_CHECK("prepare_train_kernel");
    return PN2_OK;
}
