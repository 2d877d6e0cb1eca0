// group.hip -- index_points and the neighbourhood grouping, for the public op API.
//
// index_points:        /root/reference/model/pointnet2_utils.py:28-45
// sample_and_group:    pointnet2_utils.py:107-116  ([xyz - centroid, feature], xyz first)
// SA-MSG grouping:     pointnet2_utils.py:204-209  ([feature, xyz - centroid], feature first)
// The fused SA path (sa_mlp.hip) gathers straight into LDS and never materialises these
// tensors; these kernels serve the standalone functions of the drop-in module.
// One thread per output element (contiguous output => coalesced stores); the subtraction is a
// single correctly rounded float32 op, bit-identical to the reference.
//
// Indices follow torch's advanced indexing: -N <= n < 0 counts from the end.  Outside [-N, N)
// the reference raises IndexError; a kernel cannot, so the element is NaN (never an
// out-of-bounds read) and PN2_DEVERR_INDEX is raised in the launching thread's device error slot
// (pn2_error_slot_set / pn2_device_errors; pn2.check_device_errors() raises IndexError).
#include <atomic>

#include "pn2_internal.h"

namespace pn2 {

// the process-wide default error slot (pn2_internal.h): [0] bits, [1] the take's snapshot
__device__ unsigned g_default_errors[2];

static std::atomic<unsigned *> g_default_cache[kMaxDevices];

// device d's copy of g_default_errors (the symbol's address is per device: resolved with d
// current, once)
unsigned *default_error_slot(int d) {
    if (d < 0 || d >= kMaxDevices) return nullptr;
    unsigned *p = g_default_cache[d].load(std::memory_order_acquire);
    if (!p) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) return nullptr;
        if (cur != d && hipSetDevice(d) != hipSuccess) return nullptr;
        void *a = nullptr;
        const hipError_t e = hipGetSymbolAddress(&a, HIP_SYMBOL(g_default_errors));
        if (cur != d) (void)hipSetDevice(cur);
        if (e != hipSuccess) return nullptr;
        p = static_cast<unsigned *>(a);
        g_default_cache[d].store(p, std::memory_order_release);
    }
    return p;
}

bool is_default_error_slot(const unsigned *slot) {
    for (int d = 0; d < kMaxDevices; ++d)
        if (slot && g_default_cache[d].load(std::memory_order_acquire) == slot) return true;
    return false;
}

// the slot's value (and, with clear, its reset) in ONE device atomic: a bit that a kernel ORs in
// between cannot be lost (a read followed by a separate clear could drop it)
__global__ void errors_take_kernel(unsigned *slot, int clear) {
    slot[1] = clear ? atomicExch(&slot[0], 0u) : atomicOr(&slot[0], 0u);
}

hipError_t take_errors(unsigned *slot, int clear, unsigned *bits, hipStream_t st) {
    hipLaunchKernelGGL(errors_take_kernel, dim3(1), dim3(1), 0, st, slot, clear);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    unsigned v = 0;
    if ((e = hipMemcpyAsync(&v, slot + 1, sizeof(v), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    *bits = v;
    return hipSuccess;
}

// torch's index rule; -1 when out of range (and the error bit raised in the launch's slot)
__device__ __forceinline__ int64_t torch_index(int64_t n, int64_t N, unsigned *err) {
    if (n < 0) n += N;
    if (n < 0 || n >= N) {
        atomicOr(err, (unsigned)PN2_DEVERR_INDEX);
        return -1;
    }
    return n;
}

__global__ __launch_bounds__(256) void index_points_kernel(const float *__restrict__ pts,
                                                           int64_t B, int64_t N, int64_t C,
                                                           int64_t sb, int64_t sn, int64_t sc,
                                                           const int64_t *__restrict__ idx,
                                                           int64_t M, float *__restrict__ out,
                                                           unsigned *err) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * M * C) return;
    const int64_t c = e % C;
    const int64_t bm = e / C;
    const int64_t b = bm / M;
    const int64_t n = torch_index(idx[bm], N, err);
    out[e] = n < 0 ? __builtin_nanf("") : pts[b * sb + n * sn + c * sc];
}

__global__ __launch_bounds__(256) void group_kernel(const float *__restrict__ pts, int64_t N,
                                                    int64_t C, int64_t sb, int64_t sn, int64_t sc,
                                                    const float *__restrict__ feat, int64_t D,
                                                    int64_t fb, int64_t fn, int64_t fd,
                                                    const float *__restrict__ ctr, int64_t S,
                                                    const int64_t *__restrict__ idx, int64_t K,
                                                    int feature_first, int64_t total,
                                                    float *__restrict__ out, unsigned *err) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t W = C + D;
    const int64_t ch = e % W;
    const int64_t row = e / W;  // (b*S + s)*K + k
    const int64_t g = row / K;
    const int64_t b = g / S;
    const int64_t n = torch_index(idx[row], N, err);
    const int64_t xc = feature_first ? ch - D : ch;  // xyz channel, if any
    float v;
    if (n < 0)
        v = __builtin_nanf("");
    else if (xc >= 0 && xc < C)
        v = __fsub_rn(pts[b * sb + n * sn + xc * sc], ctr[g * C + xc]);
    else {
        const int64_t d = feature_first ? ch : ch - C;
        v = feat[b * fb + n * fn + d * fd];
    }
    out[e] = v;
}

// ------------------------------------------------------------------ grouping backward
// dfeat[b,n,:] = the float32 sum of the grouped rows' feature gradients over the positions
// (s,k) with idx[b,s,k] == n, taken in ascending (s,k) order from +0.0f, one rounding per add:
// np.add.at / torch's CPU index_add_, bit for bit, and the same bits on every run (no float
// atomics anywhere).  Three launches over a workspace [cnt B*N | start B*N | pos B*S*K] (int32):
//   gb_count   one thread per position: cnt[b,n] += 1 (integer atomics: the result has no order);
//              an index outside [-N, N) raises PN2_DEVERR_INDEX and is counted nowhere
//   gb_fill    one wave per 64 destination points of a cloud: start = the exclusive prefix of the
//              cloud's counts, then the cloud's S*K indices in order, 64 per load; the lanes whose
//              index falls in the wave's range are served one distinct destination per step (a
//              padded list repeats one index: its lanes share a step), each lane's slot = the
//              destination's cursor + the number of lower lanes with the same destination
//              => pos lists every destination's positions ascending
//   gb_sum     one wave per destination point: lanes span the channels (16-byte loads when width,
//              offset, stride and bases allow; else dwords), the wave walks the point's list in
//              order, 8 rows in flight.  Every point is written (zeros for an empty list).
// The positions of cloud b live in pos[b*S*K ...]: a cloud never holds more than S*K of them.
template <typename IT>
__device__ __forceinline__ int64_t gb_index(const IT *__restrict__ idx, int64_t b, int p, int K,
                                            int64_t ib, int64_t is, int64_t ik) {
    const int s = p / K;
    return (int64_t)idx[b * ib + s * is + (p - s * K) * ik];
}

template <typename IT>
__global__ __launch_bounds__(256) void gb_count_kernel(const IT *__restrict__ idx, int64_t ib,
                                                       int64_t is, int64_t ik, int64_t B, int N,
                                                       int SK, int K, int *__restrict__ cnt,
                                                       unsigned *err) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * SK) return;
    const int64_t b = e / SK;
    const int64_t n = torch_index(gb_index(idx, b, (int)(e - b * SK), K, ib, is, ik), N, err);
    if (n >= 0) atomicAdd(&cnt[b * N + n], 1);
}

template <typename IT>
__global__ __launch_bounds__(256) void gb_fill_kernel(const IT *__restrict__ idx, int64_t ib,
                                                      int64_t is, int64_t ik, int64_t B, int N,
                                                      int SK, int K, const int *__restrict__ cnt,
                                                      int *__restrict__ start,
                                                      int *__restrict__ pos) {
    const int lane = threadIdx.x & 63;
    const int wpc = (N + 63) >> 6;  // waves per cloud
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= B * wpc) return;  // whole waves
    const int64_t b = gw / wpc;
    const int n0 = (int)(gw - b * wpc) * 64;
    const int *c = cnt + b * N;
    // positions of the cloud's points before n0, then of the wave's points before the lane's
    int before = 0;
    for (int i = lane; i < n0; i += 64) before += c[i];
#pragma unroll
    for (int o = 32; o; o >>= 1) before += __shfl_xor(before, o);
    const bool mine = n0 + lane < N;
    const int own = mine ? c[n0 + lane] : 0;
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    int cur = before + incl - own;
    if (mine) start[b * N + n0 + lane] = cur;
    int *out = pos + b * SK;
    for (int p0 = 0; p0 < SK; p0 += 64) {
        const int p = p0 + lane;
        int d = -1;
        if (p < SK) {
            int64_t n = gb_index(idx, b, p, K, ib, is, ik);
            if (n < 0) n += N;
            if (n >= n0 && n < N && n < (int64_t)n0 + 64) d = (int)n - n0;
        }
        unsigned long long todo = __ballot(d >= 0);
        while (todo) {  // wave-uniform: one distinct destination per step
            const int dd = __builtin_amdgcn_readlane(d, __ffsll(todo) - 1);
            const unsigned long long m = __ballot(d == dd);
            const int slot = __builtin_amdgcn_readlane(cur, dd) + __popcll(m & ((1ull << lane) - 1));
            if (d == dd && slot < SK) out[slot] = p;
            if (lane == dd) cur += __popcll(m);
            todo &= ~m;
        }
    }
}

// VEC: float4 per lane (dg + off, rs, out and D all multiples of 4 floats); a pass covers
// 64 * NJ * (VEC ? 4 : 1) channels, NJ accumulators per lane
template <bool VEC>
__global__ __launch_bounds__(256) void gb_sum_kernel(const float *__restrict__ dg, int64_t rs,
                                                     int64_t B, int N, int SK, int D,
                                                     const int *__restrict__ cnt,
                                                     const int *__restrict__ start,
                                                     const int *__restrict__ pos,
                                                     float *__restrict__ out) {
    constexpr int NJ = VEC ? 1 : 4;
    constexpr int W = VEC ? 4 : 1;
    constexpr int R = 8;  // rows in flight
    typedef float vec_t __attribute__((ext_vector_type(W)));
    const int lane = threadIdx.x & 63;
    const int64_t dst = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // b*N + n
    if (dst >= B * N) return;  // whole waves
    const int64_t b = dst / N;
    const int len = min(max(cnt[dst], 0), SK);
    const int first = min(max(start[dst], 0), SK - len);
    const int *list = pos + b * SK + first;
    const float *rows = dg + b * SK * rs;
    float *o = out + dst * D;
    for (int c0 = 0; c0 < D; c0 += 64 * NJ * W) {
        vec_t acc[NJ];
        bool on[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            acc[j] = vec_t(0.f);
            on[j] = c0 + (j * 64 + lane) * W < D;
        }
        const float *col = rows + c0 + lane * W;
        for (int i0 = 0; i0 < len; i0 += 64) {
            const int nb = min(64, len - i0);
            // 64 positions per load, clamped: a row read never leaves dgrouped
            const int mine = lane < nb ? min(max(list[i0 + lane], 0), SK - 1) : 0;
            int i = 0;
            for (; i + R <= nb; i += R) {
                vec_t v[R][NJ];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float *q = col + (int64_t)__builtin_amdgcn_readlane(mine, i + r) * rs;
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        v[r][j] = on[j] ? *reinterpret_cast<const vec_t *>(q + j * 64 * W) : vec_t(0.f);
                }
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[j] += v[r][j];
            }
            for (; i < nb; ++i) {
                const float *q = col + (int64_t)__builtin_amdgcn_readlane(mine, i) * rs;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (on[j]) acc[j] += *reinterpret_cast<const vec_t *>(q + j * 64 * W);
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (on[j]) *reinterpret_cast<vec_t *>(o + c0 + (j * 64 + lane) * W) = acc[j];
    }
}

static int64_t gb_workspace_bytes(int64_t B, int64_t N, int64_t S, int64_t K) {
    return ((2 * B * N + B * S * K) * 4 + 15) & ~(int64_t)15;
}

template <typename IT>
static int gb_launch(const float *dg, int64_t rs, const IT *idx, int64_t ib, int64_t is, int64_t ik,
                     int64_t B, int N, int SK, int K, int D, bool vec, float *dfeat, int *ws,
                     unsigned *err, hipStream_t st) {
    int *cnt = ws, *start = ws + B * N, *pos = ws + 2 * B * N;
    const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)B * N * 4, st);
    if (e != hipSuccess)
        return set_error(PN2_EHIP, "pn2_group_backward_f32: memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(gb_count_kernel<IT>, dim3((unsigned)((B * SK + 255) / 256)), dim3(256), 0, st,
                       idx, ib, is, ik, B, N, SK, K, cnt, err);
    PN2_LAUNCH_CHECK("gb_count_kernel");
    const int64_t fill_waves = B * ((N + 63) / 64);
    hipLaunchKernelGGL(gb_fill_kernel<IT>, dim3((unsigned)((fill_waves + 3) / 4)), dim3(256), 0, st,
                       idx, ib, is, ik, B, N, SK, K, cnt, start, pos);
    PN2_LAUNCH_CHECK("gb_fill_kernel");
    const dim3 grid((unsigned)((B * N + 3) / 4));
    if (vec)
        hipLaunchKernelGGL(gb_sum_kernel<true>, grid, dim3(256), 0, st, dg, rs, B, N, SK, D, cnt,
                           start, pos, dfeat);
    else
        hipLaunchKernelGGL(gb_sum_kernel<false>, grid, dim3(256), 0, st, dg, rs, B, N, SK, D, cnt,
                           start, pos, dfeat);
    PN2_LAUNCH_CHECK("gb_sum_kernel");
    return PN2_OK;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_group_backward_workspace_bytes(int64_t B, int64_t N, int64_t S, int64_t K) {
    if (B < 0 || N < 1 || S < 0 || K < 1) return -1;
    return gb_workspace_bytes(B, N, S, K);
}

extern "C" int pn2_group_backward_f32(const float *dgrouped, int64_t row_stride, int64_t offset,
                                      const void *idx, int idx_dtype, int64_t ib, int64_t is,
                                      int64_t ik, int64_t B, int64_t N, int64_t S, int64_t K,
                                      int64_t D, float *dfeat, void *workspace,
                                      int64_t workspace_bytes, void *stream) {
    PN2_REQUIRE(dgrouped && idx && dfeat && workspace, "pn2_group_backward_f32: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && S >= 0 && K >= 1 && D >= 0 && offset >= 0 &&
                    row_stride >= offset + D,
                "pn2_group_backward_f32: bad shape");
    PN2_REQUIRE(D != 0, "pn2_group_backward_f32: D == 0 (no feature columns to sum)");
    PN2_REQUIRE(idx_dtype == PN2_INDEX_I64 || idx_dtype == PN2_INDEX_I32,
                "pn2_group_backward_f32: unknown index dtype %d", idx_dtype);
    // positions, counts and point numbers are 32-bit in the table
    PN2_REQUIRE(N < (1ll << 31) && D < (1ll << 31) && S * K < (1ll << 31) && B * N < (1ll << 31),
                "pn2_group_backward_f32: shape too large");
    PN2_REQUIRE(((uintptr_t)workspace & 3) == 0 && workspace_bytes >= gb_workspace_bytes(B, N, S, K),
                "pn2_group_backward_f32: workspace too small (%lld bytes, need %lld)",
                (long long)workspace_bytes, (long long)gb_workspace_bytes(B, N, S, K));
    if (B == 0) return PN2_OK;
    hipStream_t st = as_stream(stream);
    if (S == 0) {  // no rows: every sum is empty
        const hipError_t e = hipMemsetAsync(dfeat, 0, (size_t)B * N * D * 4, st);
        return e == hipSuccess ? PN2_OK
                               : set_error(PN2_EHIP, "pn2_group_backward_f32: memset: %s", hipGetErrorString(e));
    }
    unsigned *err = error_word(st);
    PN2_REQUIRE(err, "pn2_group_backward_f32: no device error slot");
    const float *dg = dgrouped + offset;
    const bool vec = rows_16b(dg, D, row_stride, 0, false) && ((uintptr_t)dfeat & 15) == 0;
    int *ws = static_cast<int *>(workspace);
    if (idx_dtype == PN2_INDEX_I32)
        return gb_launch(dg, row_stride, static_cast<const int32_t *>(idx), ib, is, ik, B, (int)N,
                         (int)(S * K), (int)K, (int)D, vec, dfeat, ws, err, st);
    return gb_launch(dg, row_stride, static_cast<const int64_t *>(idx), ib, is, ik, B, (int)N,
                     (int)(S * K), (int)K, (int)D, vec, dfeat, ws, err, st);
}

extern "C" int pn2_index_points_f32(const float *pts, int64_t B, int64_t N, int64_t C,
                                    int64_t sb, int64_t sn, int64_t sc, const int64_t *idx,
                                    int64_t M, float *out, void *stream) {
    PN2_REQUIRE(pts && idx && out, "pn2_index_points_f32: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= 1 && M >= 0, "pn2_index_points_f32: bad shape");
    const int64_t tot = B * M * C;
    if (tot == 0) return PN2_OK;
    unsigned *err = error_word(as_stream(stream));
    PN2_REQUIRE(err, "pn2_index_points_f32: no device error slot");
    hipLaunchKernelGGL(index_points_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       as_stream(stream), pts, B, N, C, sb, sn, sc, idx, M, out, err);
    PN2_LAUNCH_CHECK("index_points_kernel");
    return PN2_OK;
}

extern "C" int pn2_group_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                             int64_t sn, int64_t sc, const float *feat, int64_t D, int64_t fb,
                             int64_t fn, int64_t fd, const float *ctr, int64_t S,
                             const int64_t *idx, int64_t K, int feature_first, float *out,
                             void *stream) {
    PN2_REQUIRE(pts && ctr && idx && out, "pn2_group_f32: null pointer");
    PN2_REQUIRE(D == 0 || feat, "pn2_group_f32: D > 0 but feat is null");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= 1 && D >= 0 && S >= 0 && K >= 1,
                "pn2_group_f32: bad shape");
    const int64_t tot = B * S * K * (C + D);
    if (tot == 0) return PN2_OK;
    unsigned *err = error_word(as_stream(stream));
    PN2_REQUIRE(err, "pn2_group_f32: no device error slot");
    hipLaunchKernelGGL(group_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       as_stream(stream), pts, N, C, sb, sn, sc, feat, D, fb, fn, fd, ctr, S, idx,
                       K, feature_first, tot, out, err);
    PN2_LAUNCH_CHECK("group_kernel");
    return PN2_OK;
}
