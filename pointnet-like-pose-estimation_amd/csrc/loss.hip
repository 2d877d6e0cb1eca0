// loss.hip -- the reductions of a train step that sit after the heads' last layer, and the
// reference loops' per-batch metrics (include/pn2.h states the contracts and the order rules):
//   pn2_log_softmax_rows_f32 / _backward_f32   the classifiers' F.log_softmax under autograd
//   pn2_criterion_forward_f32 / _backward_f32  nll_loss, MSELoss, L1Loss, BCELoss (mean or sum)
//   pn2_meter_update                           the test loops' per-class bookkeeping, on the device
//
// Reference: the get_loss classes of model/pointnet2_cls_ssg.py:40-47, rotation_ssg.py:40-50,
// sign_ssg.py:38-45; F.log_softmax at pointnet2_cls_ssg.py:36; the loops of
// train_classification.py:121-122, 144-150, train_rotation.py:126-127, 157-163 and
// train_sign.py:148-153 (pn2/losses.py, pn2/metrics.py).
//
// Every shape these serve is a few thousand elements at most ([B,7], [B,3], [B,1]), so a launch
// is latency, not bandwidth: the kernels are written for a fixed order first.
//   log_softmax: a thread per row walks its K columns three times (max, the float64 sum of
//     exponentials in ascending j, the outputs).  A row never leaves its thread: row
//     independence and the order hold by construction.
//   criterion forward: ONE workgroup.  Its 256 threads compute 1024 float64 element terms at a
//     time into LDS (coalesced reads), thread 0 then continues the one float64 chain over them
//     in row-major order.  No partial sums exist anywhere, so there is nothing to combine.
//   criterion backward: elementwise, a grid-stride loop.
//   meter: ONE workgroup; a thread per (category, column) of the accumulator, per record column
//     and one for the invalid count walks the B rows in row order.
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile): every operation rounds on its
// own, so each expression in pn2.h is what the hardware evaluates.  exp and log are the device
// library's float64 functions -- the only operations here that are not correctly rounded.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kLsThreads = 64;          // log_softmax: rows per workgroup (a row per lane)
constexpr int kLsMaxK = 1024;           // widest log_softmax row
constexpr int64_t kLossMaxB = 1ll << 30;  // rows are counted in an int32
constexpr int kCrThreads = 256;
constexpr int kCrChunk = 1024;          // element terms per LDS round of the criterion forward
constexpr int kCrMaxBlocks = 4096;      // criterion backward: grid-stride above this
constexpr int kMeterThreads = 256;
constexpr int kMeterMaxCat = 4096;
constexpr int kMeterMaxD = 16;

// ------------------------------------------------------------------------------ log_softmax
__global__ __launch_bounds__(kLsThreads) void log_softmax_fwd_kernel(const float *__restrict__ X, int64_t ldx,
                                                                     float *__restrict__ Y, int64_t ldy, int B,
                                                                     int K) {
    const int64_t r = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (r >= B) return;
    const float *x = X + r * ldx;
    float *y = Y + r * ldy;
    float m = x[0];
    for (int j = 1; j < K; ++j) {
        const float v = x[j];
        m = v > m ? v : m;
    }
    const double dm = (double)m;
    double s = 0.0;
    for (int j = 0; j < K; ++j) s = s + exp((double)x[j] - dm);
    const double ls = log(s);
    for (int j = 0; j < K; ++j) y[j] = (float)(((double)x[j] - dm) - ls);
}

__global__ __launch_bounds__(kLsThreads) void log_softmax_bwd_kernel(const float *__restrict__ dY, int64_t ldd,
                                                                     const float *__restrict__ Y, int64_t ldy,
                                                                     float *__restrict__ dX, int64_t ldx, int B,
                                                                     int K) {
    const int64_t r = (int64_t)blockIdx.x * kLsThreads + threadIdx.x;
    if (r >= B) return;
    const float *dy = dY + r * ldd;
    const float *y = Y + r * ldy;
    float *dx = dX + r * ldx;
    double g = 0.0;
    for (int j = 0; j < K; ++j) g = g + (double)dy[j];
    for (int j = 0; j < K; ++j) dx[j] = (float)((double)dy[j] - exp((double)y[j]) * g);
}

// ------------------------------------------------------------------------------ criteria
__device__ __forceinline__ double clamp_log(double v) {
    const double l = log(v);
    return l < -100.0 ? -100.0 : l;  // torch's clamp of BCELoss; a NaN stays a NaN
}

// element term i (row-major) in float64; NLL: i is the row
__device__ __forceinline__ double criterion_term(int kind, const float *__restrict__ P, int64_t ldp,
                                                 const void *__restrict__ T, int64_t ldt, int64_t i, int64_t K) {
    if (kind == PN2_LOSS_NLL) {
        const int64_t t = static_cast<const int64_t *>(T)[i];
        if (t < 0 || t >= K) return __longlong_as_double(0x7ff8000000000000ll);  // nothing is indexed with it
        return -(double)P[i * ldp + t];
    }
    const int64_t b = i / K, j = i - b * K;
    const double p = (double)P[b * ldp + j];
    const double t = (double)static_cast<const float *>(T)[b * ldt + j];
    if (kind == PN2_LOSS_BCE) return -(t * clamp_log(p) + (1.0 - t) * clamp_log(1.0 - p));
    const double d = p - t;
    return kind == PN2_LOSS_MSE ? d * d : fabs(d);
}

__global__ __launch_bounds__(kCrThreads) void criterion_fwd_kernel(int kind, int mean, const float *__restrict__ P,
                                                                   int64_t ldp, const void *__restrict__ T,
                                                                   int64_t ldt, int64_t B, int64_t K,
                                                                   float *__restrict__ loss) {
    __shared__ double terms[kCrChunk];
    const int64_t n = kind == PN2_LOSS_NLL ? B : B * K;
    const int tid = threadIdx.x;
    double acc = 0.0;  // thread 0's: THE chain
    for (int64_t base = 0; base < n; base += kCrChunk) {
#pragma unroll
        for (int q = 0; q < kCrChunk / kCrThreads; ++q) {
            const int s = q * kCrThreads + tid;
            if (base + s < n) terms[s] = criterion_term(kind, P, ldp, T, ldt, base + s, K);
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = (int)(n - base < kCrChunk ? n - base : kCrChunk);
            for (int s = 0; s < cnt; ++s) acc = acc + terms[s];
        }
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(mean ? acc / (double)n : acc);
}

__global__ __launch_bounds__(kCrThreads) void criterion_bwd_kernel(int kind, int mean, const float *__restrict__ P,
                                                                   int64_t ldp, const void *__restrict__ T,
                                                                   int64_t ldt, const float *__restrict__ g,
                                                                   int64_t B, int64_t K, float *__restrict__ dP,
                                                                   int64_t ldd) {
    const int64_t n = B * K;
    const double c = mean ? 1.0 / (double)(kind == PN2_LOSS_NLL ? B : n) : 1.0;
    const double gc = (double)g[0] * c;
    for (int64_t i = (int64_t)blockIdx.x * kCrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCrThreads) {
        const int64_t b = i / K, j = i - b * K;
        float out;
        if (kind == PN2_LOSS_NLL) {
            const int64_t t = static_cast<const int64_t *>(T)[b];
            out = (t < 0 || t >= K) ? 0.f : (float)(gc * (j == t ? -1.0 : 0.0));
        } else {
            const double p = (double)P[b * ldp + j];
            const double t = (double)static_cast<const float *>(T)[b * ldt + j];
            const double d = p - t;
            double term;
            if (kind == PN2_LOSS_MSE) {
                term = 2.0 * d;
            } else if (kind == PN2_LOSS_L1) {
                term = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d == 0.0 ? 0.0 : d;  // a NaN stays a NaN
            } else {
                const double q = (1.0 - p) * p;
                term = d / (q > 1e-12 ? q : 1e-12);
            }
            out = (float)(gc * term);
        }
        dP[b * ldd + j] = out;
    }
}

// ------------------------------------------------------------------------------ meters
// the category of row r: the target itself for CLS, the label else
__device__ __forceinline__ int64_t meter_label(int kind, const void *target, const int64_t *label, int r) {
    return kind == PN2_METER_CLS ? static_cast<const int64_t *>(target)[r] : label[r];
}

// whether row r counts as correct (CLS: int64 equality; SIGN: float equality)
__device__ __forceinline__ bool meter_hit(int kind, const void *pred, int64_t ldp, const void *target, int64_t ldt,
                                          int r) {
    if (kind == PN2_METER_CLS)
        return static_cast<const int64_t *>(pred)[r] == static_cast<const int64_t *>(target)[r];
    return static_cast<const float *>(pred)[r * ldp] == static_cast<const float *>(target)[r * ldt];
}

__device__ __forceinline__ double meter_abs(const void *pred, int64_t ldp, const void *target, int64_t ldt, int r,
                                            int axis) {
    const float a = static_cast<const float *>(pred)[r * ldp + axis] - static_cast<const float *>(target)[r * ldt + axis];
    return (double)fabsf(a);
}

__global__ __launch_bounds__(kMeterThreads) void meter_kernel(int kind, const void *__restrict__ pred, int64_t ldp,
                                                              const void *__restrict__ target, int64_t ldt,
                                                              const int64_t *__restrict__ label, int B, int D,
                                                              int nc, double *__restrict__ acc,
                                                              double *__restrict__ invalid,
                                                              double *__restrict__ record) {
    const int W = kind == PN2_METER_POSE ? 1 + D : 2;
    const int RW = kind == PN2_METER_POSE ? D : 1;
    const int jobs = nc * W + RW + 1;
    for (int job = threadIdx.x; job < jobs; job += kMeterThreads) {
        if (job < nc * W) {
            const int c = job / W, col = job - c * W;
            int count = 0, hits = 0;
            double s = 0.0;
            for (int r = 0; r < B; ++r) {
                if (meter_label(kind, target, label, r) != c) continue;
                ++count;
                if (kind != PN2_METER_POSE) hits += meter_hit(kind, pred, ldp, target, ldt, r) ? 1 : 0;
                else if (col > 0) s = s + meter_abs(pred, ldp, target, ldt, r, col - 1);
            }
            if (count == 0) continue;  // a category absent from the batch: its row keeps its bits
            double add;
            if (kind == PN2_METER_CLS) add = col == 0 ? (double)hits / (double)count : 1.0;
            else if (kind == PN2_METER_SIGN) add = col == 0 ? (double)hits : (double)count;
            else add = col == 0 ? 1.0 : (double)(float)(s / (double)count);
            acc[job] = acc[job] + add;
        } else if (job < nc * W + RW) {
            const int k = job - nc * W;
            if (kind == PN2_METER_POSE) {
                double s = 0.0;
                for (int r = 0; r < B; ++r) s = s + meter_abs(pred, ldp, target, ldt, r, k);
                record[k] = (double)(float)(s / (double)B);
            } else {
                int hits = 0;
                for (int r = 0; r < B; ++r) hits += meter_hit(kind, pred, ldp, target, ldt, r) ? 1 : 0;
                record[0] = (double)hits / (double)B;
            }
        } else {
            int bad = 0;
            for (int r = 0; r < B; ++r) {
                const int64_t l = meter_label(kind, target, label, r);
                bad += (l < 0 || l >= nc) ? 1 : 0;
            }
            if (bad) invalid[0] = invalid[0] + (double)bad;
        }
    }
}

// ------------------------------------------------------------------------------ host
static int loss_rows(const char *what, int64_t B, int64_t K) {
    if (B < 1 || K < 1) return set_error(PN2_EINVAL, "%s: bad shape B=%lld K=%lld", what, (long long)B, (long long)K);
    if (B > kLossMaxB)
        return set_error(PN2_EUNSUPPORTED, "%s: B=%lld above 2^30 rows", what, (long long)B);
    return PN2_OK;
}

static int criterion_check(const char *what, int kind, int reduction, const float *P, int64_t ldp, const void *T,
                           int64_t ldt, int64_t B, int64_t K) {
    PN2_REQUIRE(kind == PN2_LOSS_NLL || kind == PN2_LOSS_MSE || kind == PN2_LOSS_L1 || kind == PN2_LOSS_BCE,
                "%s: unknown kind %d", what, kind);
    PN2_REQUIRE(reduction == PN2_REDUCE_MEAN || reduction == PN2_REDUCE_SUM, "%s: unknown reduction %d", what,
                reduction);
    PN2_REQUIRE(P && T, "%s: null pointer", what);
    const int rc = loss_rows(what, B, K);
    if (rc != PN2_OK) return rc;
    if (K > kLossMaxB) return set_error(PN2_EUNSUPPORTED, "%s: K=%lld above 2^30 columns", what, (long long)K);
    PN2_REQUIRE(ldp >= K && (kind == PN2_LOSS_NLL || ldt >= K), "%s: a leading dimension is below its matrix width",
                what);
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int pn2_log_softmax_rows_f32(const float *X, int64_t ldx, float *Y, int64_t ldy, int64_t B, int64_t K,
                                        void *stream) {
    const char *what = "pn2_log_softmax_rows_f32";
    PN2_REQUIRE(X && Y, "%s: null pointer", what);
    const int rc = loss_rows(what, B, K);
    if (rc != PN2_OK) return rc;
    if (K > kLsMaxK) return set_error(PN2_EUNSUPPORTED, "%s: K=%lld above %d columns", what, (long long)K, kLsMaxK);
    PN2_REQUIRE(ldx >= K && ldy >= K, "%s: a leading dimension is below its matrix width", what);
    hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3((unsigned)((B + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads),
                       0, as_stream(stream), X, ldx, Y, ldy, (int)B, (int)K);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

extern "C" int pn2_log_softmax_rows_backward_f32(const float *dY, int64_t ldd, const float *Y, int64_t ldy,
                                                 float *dX, int64_t ldx, int64_t B, int64_t K, void *stream) {
    const char *what = "pn2_log_softmax_rows_backward_f32";
    PN2_REQUIRE(dY && Y && dX, "%s: null pointer", what);
    const int rc = loss_rows(what, B, K);
    if (rc != PN2_OK) return rc;
    if (K > kLsMaxK) return set_error(PN2_EUNSUPPORTED, "%s: K=%lld above %d columns", what, (long long)K, kLsMaxK);
    PN2_REQUIRE(ldd >= K && ldy >= K && ldx >= K, "%s: a leading dimension is below its matrix width", what);
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3((unsigned)((B + kLsThreads - 1) / kLsThreads)), dim3(kLsThreads),
                       0, as_stream(stream), dY, ldd, Y, ldy, dX, ldx, (int)B, (int)K);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

extern "C" int pn2_criterion_forward_f32(int kind, int reduction, const float *P, int64_t ldp, const void *target,
                                         int64_t ldt, int64_t B, int64_t K, float *loss, void *stream) {
    const char *what = "pn2_criterion_forward_f32";
    const int rc = criterion_check(what, kind, reduction, P, ldp, target, ldt, B, K);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(loss, "%s: null pointer", what);
    hipLaunchKernelGGL(criterion_fwd_kernel, dim3(1), dim3(kCrThreads), 0, as_stream(stream), kind,
                       reduction == PN2_REDUCE_MEAN ? 1 : 0, P, ldp, target, ldt, B, K, loss);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

extern "C" int pn2_criterion_backward_f32(int kind, int reduction, const float *P, int64_t ldp, const void *target,
                                          int64_t ldt, const float *g, int64_t B, int64_t K, float *dP, int64_t ldd,
                                          void *stream) {
    const char *what = "pn2_criterion_backward_f32";
    const int rc = criterion_check(what, kind, reduction, P, ldp, target, ldt, B, K);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(g && dP, "%s: null pointer", what);
    PN2_REQUIRE(ldd >= K, "%s: a leading dimension is below its matrix width", what);
    const int64_t blocks = (B * K + kCrThreads - 1) / kCrThreads;
    hipLaunchKernelGGL(criterion_bwd_kernel, dim3((unsigned)(blocks < kCrMaxBlocks ? blocks : kCrMaxBlocks)),
                       dim3(kCrThreads), 0, as_stream(stream), kind, reduction == PN2_REDUCE_MEAN ? 1 : 0, P, ldp,
                       target, ldt, g, B, K, dP, ldd);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}

extern "C" int pn2_meter_update(int kind, const void *pred, int64_t ldp, const void *target, int64_t ldt,
                                const int64_t *label, int64_t B, int64_t D, int64_t num_category, double *acc,
                                double *invalid, double *records, int64_t slot, int64_t slots, void *stream) {
    const char *what = "pn2_meter_update";
    PN2_REQUIRE(kind == PN2_METER_CLS || kind == PN2_METER_SIGN || kind == PN2_METER_POSE, "%s: unknown kind %d", what,
                kind);
    PN2_REQUIRE(pred && target && acc && invalid && records && (kind == PN2_METER_CLS || label),
                "%s: null pointer", what);
    if (B < 1 || D < 1 || num_category < 1)
        return set_error(PN2_EINVAL, "%s: bad shape B=%lld D=%lld num_category=%lld", what, (long long)B,
                         (long long)D, (long long)num_category);
    PN2_REQUIRE(kind == PN2_METER_POSE || D == 1, "%s: bad shape D=%lld (1 for this kind)", what, (long long)D);
    if (B > kLossMaxB) return set_error(PN2_EUNSUPPORTED, "%s: B=%lld above 2^30 rows", what, (long long)B);
    if (D > kMeterMaxD || num_category > kMeterMaxCat)
        return set_error(PN2_EUNSUPPORTED, "%s: D=%lld above %d or num_category=%lld above %d", what, (long long)D,
                         kMeterMaxD, (long long)num_category, kMeterMaxCat);
    PN2_REQUIRE(kind == PN2_METER_CLS || (ldp >= D && ldt >= D), "%s: a leading dimension is below its matrix width",
                what);
    PN2_REQUIRE(slot >= 0 && slot < slots, "%s: record slot %lld outside [0, %lld)", what, (long long)slot,
                (long long)slots);
    const int64_t rw = kind == PN2_METER_POSE ? D : 1;
    hipLaunchKernelGGL(meter_kernel, dim3(1), dim3(kMeterThreads), 0, as_stream(stream), kind, pred, ldp, target, ldt,
                       label, (int)B, (int)D, (int)num_category, acc, invalid, records + slot * rw);
    PN2_LAUNCH_CHECK(what);
    return PN2_OK;
}
