// fps.hip -- farthest point sampling for gfx950.
//
// Replaces farthest_point_sample (/root/reference/model/pointnet2_utils.py:47-68) and the
// index_points(points, fps_idx) that follows it (pointnet2_utils.py:106, 201).
//
// One workgroup per cloud.  Lane t of the block owns the CONTIGUOUS points t*PPT .. t*PPT+PPT-1
// and keeps them in registers for the whole run, together with their running min-distance (the
// uint bits of a non-negative float, so compares/maxima are integer ops).  Because ownership is
// contiguous and in lane/wave order, "the first index among the maxima" (torch.max's tie rule)
// is simply the first lane -- then the first wave -- that holds the maximum: one DPP max per
// level plus a ballot, no second (index) reduction.  One iteration:
//   branchless distance of every owned point to the centroid in the reference's exact float32
//   order (differences, exact squares, layout-dependent channel sum, no FMA contraction) ->
//   strict-< min update -> per-lane max -> wave max by DPP + ballot/ctz for the owner lane -> the
//   owner's first point at the max by one ballot per point (wave-uniform index, SALU scan) and its
//   coordinates by one indexed register move each -> [NW > 1] the owner writes {max, index,
//   coordinates} to its wave's LDS slot (double-buffered by iteration parity), ONE barrier,
//   every wave reads all NW
//   slots (one lane each), DPP max over a 16-lane row + ballot picks the winning wave and
//   v_readlane broadcasts its index/coordinates.  No second barrier, no global memory in the loop.
// The sampled indices are kept in LDS and written, with the gathered centroids and the packed
// (coords, ssq) records the ball query reads, after the serial loop.
#include "fps_body.h"

#include <stdlib.h>

#include <algorithm>

namespace pn2 {

template <int NT, int PPT, int CM, bool FIXED, bool LDSC, int CR = CM>
__global__ __launch_bounds__(NT) void fps_kernel(const FpsArgs F) {
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    fps_block<NT, PPT, CM, FIXED, LDSC, CR>(F, (int)blockIdx.x, fsm);
}

// both sampling levels of a cloud by one workgroup (fps_body.h fps2_block)
template <int NT>
__global__ __launch_bounds__(NT) void fps2_kernel(const Fps2Args G) {
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    fps2_block<NT>(G, (int)blockIdx.x, fsm);
}

// ------------------------------------------------------------------------- streamed FPS
// Any N and S: nothing of the cloud is register-resident.  Each iteration every thread walks
// the points n = tid, tid + NT, ... (coalesced reads of the input for either layout), computes
// the distance in the reference's order, updates the running minimum -- held in LDS when the
// cloud's N words fit (DL), else in the caller's workspace (one word per point) -- and keeps
// the 64-bit key (distance bits : ~index), whose maximum is torch.max's first index among the
// maxima.  Wave max by shuffles, one LDS slot per wave (double-buffered by parity), ONE
// barrier, every thread reduces the NW slots (the exchange of fps_points.hip's wg_argmax, kept
// in this packed form: as pairs the workspace variant measured 0.5 % slower).
// The centroid's coordinates are re-read from
// the input (one broadcast load).  Indices go straight to out_idx; the output pass reads them
// back with sc1 loads (stores of other waves of this workgroup).
// Point dimensions past the register-resident kMaxC (16 < C <= kMaxCWide) always take this
// kernel, with 256 threads: a point's channels, squares and the centroid are register arrays
// of kMaxCWide entries (predicated on C), too many for 1024-thread workgroups.
constexpr int kFpsStreamT = 1024;
template <int CM>
constexpr int fps_stream_threads() { return CM > kMaxC ? 256 : kFpsStreamT; }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

template <int CM, bool FIXED, bool DL>
__global__ __launch_bounds__(fps_stream_threads<CM>()) void fps_stream_kernel(const FpsArgs F,
                                                                              unsigned *__restrict__ dist_ws) {
    constexpr int NT = fps_stream_threads<CM>(), NW = NT / 64;
    // always raised: the tuning key fps_prio (F.prio) governs only the resident kernels
    __builtin_amdgcn_s_setprio(PN2_FPS_PRIO);
    const int N = F.N, C = FIXED ? CM : F.C, kind = F.kind, S = F.S, cp = F.cp;
    const int64_t sn = F.sn, sc = F.sc;
    float *__restrict__ out_pts = F.out_pts;
    float *__restrict__ out_packed = F.out_packed;
    float *__restrict__ pts_packed = F.pts_packed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float *__restrict__ P = F.pts + (int64_t)b * F.sb;
    extern __shared__ __attribute__((aligned(16))) unsigned long long ssm[];
    unsigned long long *slots = ssm;                               // [2][NW]
    unsigned *dist = DL ? reinterpret_cast<unsigned *>(ssm + 2 * NW)  // [N]
                        : dist_ws + (int64_t)b * N;
    auto point = [&](int64_t n, float (&q)[CM]) {
#pragma unroll
        for (int k = 0; k < CM; ++k) q[k] = (k < C) ? P[n * sn + (int64_t)k * sc] : 0.f;
    };
    for (int n = tid; n < N; n += NT) {
        dist[n] = __float_as_uint(1e10f);
        if (pts_packed) {
            float q[CM], sq[CM];
            point(n, q);
#pragma unroll
            for (int k = 0; k < CM; ++k) sq[k] = __fmul_rn(q[k], q[k]);
            float *dst = pts_packed + ((int64_t)b * N + n) * cp;
#pragma unroll
            for (int k = 0; k < CM; ++k)
                if (k < C) dst[k] = q[k];
            dst[C] = layout_sum<CM>(sq, C, point_rule(kind, n, N));
            for (int k = C + 1; k < cp; ++k) dst[k] = 0.f;
        }
    }
    int far = fps_start(F.start, b);
    float c[CM];
    point(far, c);
    __syncthreads();
    int64_t *__restrict__ oi = F.out_idx + (int64_t)b * S;
    for (int i = 0;; ++i) {
        if (tid == 0) oi[i] = far;
        if (i == S - 1) break;
        unsigned long long best = 0ull;
        for (int n = tid; n < N; n += NT) {
            float q[CM], sq[CM];
            point(n, q);
#pragma unroll
            for (int k = 0; k < CM; ++k) {
                const float d = q[k] - c[k];
                sq[k] = __fmul_rn(d, d);
            }
            float dd;
            if constexpr (FIXED && CM == 3) dd = seq_sum<CM>(sq, C);  // every rule agrees for C=3
            else dd = layout_sum<CM>(sq, C, point_rule(kind, n, N));
            const unsigned v = min(dist[n], __float_as_uint(dd));  // strict '<' update
            dist[n] = v;
            const unsigned long long key = ((unsigned long long)v << 32) | (0xFFFFFFFFu - (unsigned)n);
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        const int par = i & 1;
        if (lane == 0) slots[par * NW + wave] = best;
        __syncthreads();  // the other parity's slots were last read before this barrier
        unsigned long long g = slots[par * NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const unsigned long long v = slots[par * NW + w];
            g = v > g ? v : g;
        }
        far = (int)(0xFFFFFFFFu - (unsigned)g);
        point(far, c);
    }
    __syncthreads();
    for (int i = tid; i < S; i += NT) {
        const int64_t n = __hip_atomic_load(oi + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (out_pts || out_packed) {
            float q[CM], sq[CM];
            point(n, q);
#pragma unroll
            for (int k = 0; k < CM; ++k) sq[k] = __fmul_rn(q[k], q[k]);
            if (out_pts) {
                float *o = out_pts + ((int64_t)b * S + i) * C;
#pragma unroll
                for (int k = 0; k < CM; ++k)
                    if (k < C) o[k] = q[k];
            }
            if (out_packed) {
                float *o = out_packed + ((int64_t)b * S + i) * cp;
#pragma unroll
                for (int k = 0; k < CM; ++k)
                    if (k < C) o[k] = q[k];
                o[C] = contig_sum<CM>(sq, C);
                for (int k = C + 1; k < cp; ++k) o[k] = 0.f;
            }
        }
    }
}

// ------------------------------------------------------------------------- pack kernel
template <int CM>
__global__ __launch_bounds__(256) void pack_points_kernel(const float *__restrict__ pts, int64_t B,
                                                          int N, int C, int64_t sb, int64_t sn,
                                                          int64_t sc, int kind,
                                                          float *__restrict__ packed, int cp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * N) return;
    const int64_t b = e / N;
    const int n = (int)(e - b * N);
    const float *q = pts + b * sb + (int64_t)n * sn;
    float a[CM], sq[CM];
#pragma unroll
    for (int k = 0; k < CM; ++k) {
        a[k] = (k < C) ? q[(int64_t)k * sc] : 0.f;
        sq[k] = __fmul_rn(a[k], a[k]);
    }
    float *o = packed + e * cp;
#pragma unroll
    for (int k = 0; k < CM; ++k)
        if (k < C) o[k] = a[k];
    o[C] = layout_sum<CM>(sq, C, point_rule(kind, n, N));
    for (int k = C + 1; k < cp; ++k) o[k] = 0.f;
}

}  // namespace pn2

using namespace pn2;

extern "C" int64_t pn2_packed_stride(int64_t C) { return ((C + 1 + 3) / 4) * 4; }

// the FpsArgs of a launch (or side job) over points pts[b*sb + n*sn + c*sc], starts from the
// device array start_dev (null: carried in the arguments, fps_host_starts)
static FpsArgs fps_args(const float *pts, int64_t N, int64_t C, int64_t sb, int64_t sn, int64_t sc,
                        const int64_t *start_dev, int64_t S, int64_t *out_idx, float *out_pts,
                        float *out_packed, float *pts_packed) {
    FpsArgs F;
    F.pts = pts;
    F.N = (int)N;
    F.C = (int)C;
    F.sb = sb;
    F.sn = sn;
    F.sc = sc;
    F.kind = layout_kind(sn, sc);
    F.S = (int)S;
    F.out_idx = out_idx;
    F.out_pts = out_pts;
    F.out_packed = out_packed;
    F.pts_packed = pts_packed;
    F.cp = (int)pn2_packed_stride(C);
    F.prio = tuning().fps_prio ? 1 : 0;
    F.start.dev = start_dev;
    return F;
}

// One FPS call, built once by its entry point: the kernels' argument block for clouds 0 .. B-1
// and the streamed kernel's workspace (one word per point; null where none is needed)
struct FpsCall {
    FpsArgs F;
    int64_t B;
    unsigned *ws;
};

// start[0 .. B) of a host array inside [0, N), else who's error; then into the argument block
static int fps_host_starts_check(const char *who, const int64_t *start, int64_t B, int64_t N) {
    for (int64_t b = 0; b < B; ++b)
        PN2_REQUIRE(start[b] >= 0 && start[b] < N, "%s: start[%lld] = %lld outside [0, %lld)", who,
                    (long long)b, (long long)start[b], (long long)N);
    return PN2_OK;
}
static void fps_host_starts(FpsStart &fs, const int64_t *start, int64_t B) {
    fs.dev = nullptr;
    for (int64_t b = 0; b < B; ++b) fs.v[b] = (int)start[b];
}

// the call over its clouds b0 .. B-1; an optional output or workspace that is absent stays absent
static FpsCall fps_advance(FpsCall c, int64_t b0) {
    const auto off = [](auto *p, int64_t n) { return p ? p + n : nullptr; };
    FpsArgs &F = c.F;
    F.pts += b0 * F.sb;
    F.out_idx += b0 * F.S;
    F.out_pts = off(F.out_pts, b0 * F.S * F.C);
    F.out_packed = off(F.out_packed, b0 * F.S * F.cp);
    F.pts_packed = off(F.pts_packed, b0 * F.N * F.cp);
    c.ws = off(c.ws, b0 * F.N);
    c.B -= b0;
    return c;
}

template <int NT, int PPT, int CM, bool FIXED, int CR = CM>
static int launch_fps(const FpsCall &c, hipStream_t st) {
    const FpsArgs &F = c.F;
    const int64_t B = c.B, N = F.N, S = F.S;
    const size_t head = fps_block_lds(NT, CM, true, 0, S);
    const size_t cloud = fps_block_lds(NT, CM, true, N, S) - head;
    const bool ldsc = CR == CM && cloud <= (size_t)kFpsLdsCloud && head + cloud <= (size_t)160 * 1024;
    const size_t lds = fps_block_lds(NT, CM, ldsc, N, S);
    if constexpr (CR != CM) {
        hipLaunchKernelGGL((fps_kernel<NT, PPT, CM, FIXED, false, CR>), dim3((unsigned)B), dim3(NT), lds, st, F);
    } else if (ldsc) {
        static const hipError_t attr = hipFuncSetAttribute(
            reinterpret_cast<const void *>(&fps_kernel<NT, PPT, CM, FIXED, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)attr;
        hipLaunchKernelGGL((fps_kernel<NT, PPT, CM, FIXED, true>), dim3((unsigned)B), dim3(NT), lds, st, F);
    } else {
        hipLaunchKernelGGL((fps_kernel<NT, PPT, CM, FIXED, false>), dim3((unsigned)B), dim3(NT), lds, st, F);
    }
    PN2_LAUNCH_CHECK("fps_kernel");
    return PN2_OK;
}

// Block shape per cloud size.  Tuning fps_threads / fps_ppt force one of the compiled shapes
// (tuning experiments only).
template <int CM, bool FIXED, int CAP>
static int dispatch_fps(const FpsCall &c, hipStream_t st) {
    const int64_t N = c.F.N;
    const int64_t fnt = tuning().fps_threads, fppt = tuning().fps_ppt;
#define PN2_FPS_TRY(nt, ppt) \
    if (fnt == nt && fppt == ppt && N <= (int64_t)nt * ppt) return launch_fps<nt, ppt, CM, FIXED>(c, st);
    PN2_FPS_TRY(64, 8) PN2_FPS_TRY(64, 16) PN2_FPS_TRY(128, 4) PN2_FPS_TRY(128, 8) PN2_FPS_TRY(256, 2)
    PN2_FPS_TRY(256, 4) PN2_FPS_TRY(512, 2) PN2_FPS_TRY(1024, 1) PN2_FPS_TRY(512, 4) PN2_FPS_TRY(1024, 2)
    if constexpr (CM == 3) {
        PN2_FPS_TRY(512, 16) PN2_FPS_TRY(512, 32) PN2_FPS_TRY(256, 32) PN2_FPS_TRY(1024, 8)
    }
#undef PN2_FPS_TRY
    if (N <= 256) return launch_fps<64, 4, CM, FIXED>(c, st);
    // measured on MI355X (tools/bench_fps.py): two points per lane and 4-16 waves win until
    // the per-wave register set grows; past 2048 points the block is capped at 1024 threads.
    // Up to 1024 points (tuning fps_mid): alone on the chip 8 waves of 2 points are fastest
    // (r04, interleaved x3: SSG sa1 154 vs 178 us at 256 x 4, sa2 43.0 vs 49.4; the eager
    // forward +6.5 %); in the pipelines, beside the chains on the same SIMDs, 4 waves of 4
    // points read ~2 % better (K = 100, tools/gpu_r04ab.sh), so pn2/pipeline.py selects that
    // for its geometry
    if (N <= 1024) {
        if (tuning().fps_mid == 256) return launch_fps<256, 4, CM, FIXED>(c, st);
        return launch_fps<512, 2, CM, FIXED>(c, st);
    }
    if (N <= 2048) return launch_fps<1024, 2, CM, FIXED>(c, st);
    if (N <= 4096) return launch_fps<1024, 4, CM, FIXED>(c, st);
    if constexpr (CAP >= 8192)
        if (N <= 8192) return launch_fps<1024, 8, CM, FIXED>(c, st);
    if constexpr (CAP >= 16384)
        if (N <= 16384) return launch_fps<1024, 16, CM, FIXED>(c, st);
    // past the register-resident caps: xyz in registers, the other channels re-read from the
    // input each iteration when they are not constant (the pose heads' one-hot clouds -- e.g.
    // the 10000-point camera scans -- never read them)
    if constexpr (CM > 3)
        if (N <= 16384) return launch_fps<1024, 16, CM, FIXED, 3>(c, st);
    return set_error(PN2_EUNSUPPORTED, "pn2_fps_f32: N=%lld: no register-resident shape", (long long)N);
}

// the register-resident kernels' limits (dispatch_fps); past them the streamed kernel
static bool fps_resident(int64_t N, int64_t S) { return N <= 16384 && S <= kFpsMaxS; }
static size_t fps_stream_lds(int64_t N, int nt = kFpsStreamT) { return (size_t)2 * (nt / 64) * 8 + (size_t)N * 4; }
static bool fps_stream_dl(int64_t N, int nt = kFpsStreamT) { return fps_stream_lds(N, nt) <= (size_t)160 * 1024; }

template <int CM, bool FIXED>
static int launch_fps_stream(const FpsCall &c, hipStream_t st) {
    constexpr int NT = fps_stream_threads<CM>();
    const int64_t N = c.F.N;
    if (fps_stream_dl(N, NT)) {
        static const hipError_t attr = hipFuncSetAttribute(
            reinterpret_cast<const void *>(&fps_stream_kernel<CM, FIXED, true>),
            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        PN2_REQUIRE(attr == hipSuccess, "pn2_fps_f32: LDS attribute: %s", hipGetErrorString(attr));
        hipLaunchKernelGGL((fps_stream_kernel<CM, FIXED, true>), dim3((unsigned)c.B), dim3(NT),
                           fps_stream_lds(N, NT), st, c.F, nullptr);
    } else {
        hipLaunchKernelGGL((fps_stream_kernel<CM, FIXED, false>), dim3((unsigned)c.B), dim3(NT),
                           fps_stream_lds(0, NT), st, c.F, c.ws);
    }
    PN2_LAUNCH_CHECK("fps_stream_kernel");
    return PN2_OK;
}

extern "C" int64_t pn2_fps_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t S) {
    if (B < 0 || N < 1 || C < 1 || S < 1) return -1;
    if (C > kMaxC) return fps_stream_dl(N, fps_stream_threads<kMaxCWide>()) ? 0 : B * N * 4;
    return (fps_resident(N, S) || fps_stream_dl(N)) ? 0 : B * N * 4;
}

static int fps_check(const float *pts, const int64_t *start, int64_t *out_idx, int64_t B, int64_t N,
                     int64_t C, int64_t S, void *workspace, int64_t workspace_bytes) {
    PN2_REQUIRE(pts && start && out_idx, "pn2_fps_f32: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= 1 && S >= 1 && N < INT32_MAX && S < INT32_MAX,
                "pn2_fps_f32: bad shape B=%lld N=%lld C=%lld S=%lld", (long long)B, (long long)N, (long long)C,
                (long long)S);
    if (C > kMaxCWide)
        return set_error(PN2_EUNSUPPORTED, "pn2_fps_f32: unsupported C=%lld (max %d)", (long long)C, kMaxCWide);
    const int64_t need = pn2_fps_workspace_bytes(B, N, C, S);
    PN2_REQUIRE(workspace_bytes >= need && (need == 0 || workspace),
                "pn2_fps_f32: N=%lld needs pn2_fps_workspace_bytes = %lld bytes of workspace", (long long)N,
                (long long)need);
    return PN2_OK;
}

static int fps_run(const FpsCall &c, hipStream_t st) {
    const int C = c.F.C;
    if (C > kMaxC) return launch_fps_stream<kMaxCWide, false>(c, st);
    if (!fps_resident(c.F.N, c.F.S)) {
        if (C == 3) return launch_fps_stream<3, true>(c, st);
        if (C == 10) return launch_fps_stream<10, true>(c, st);
        return launch_fps_stream<kMaxC, false>(c, st);
    }
    if (C == 3) return dispatch_fps<3, true, 16384>(c, st);
    if (C == 10) return dispatch_fps<10, true, 8192>(c, st);
    return dispatch_fps<kMaxC, false, 4096>(c, st);
}

extern "C" int pn2_fps_ws_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                              int64_t sc, const int64_t *start, int64_t S, int64_t *out_idx, float *out_pts,
                              float *out_packed, float *pts_packed, void *workspace, int64_t workspace_bytes,
                              void *stream) {
    const int rc = fps_check(pts, start, out_idx, B, N, C, S, workspace, workspace_bytes);
    if (rc != PN2_OK || B == 0) return rc;
    const FpsCall c = {fps_args(pts, N, C, sb, sn, sc, start, S, out_idx, out_pts, out_packed, pts_packed), B,
                       static_cast<unsigned *>(workspace)};
    return fps_run(c, as_stream(stream));
}

// start in host memory, read during the call (the caller may reuse it on return): carried in
// the kernel arguments, kFpsArgStarts clouds per launch (a launch of that many clouds already
// covers the chip's 256 CUs, so the split costs no concurrency)
extern "C" int pn2_fps_host_ws_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                                   int64_t sc, const int64_t *start_host, int64_t S, int64_t *out_idx,
                                   float *out_pts, float *out_packed, float *pts_packed, void *workspace,
                                   int64_t workspace_bytes, void *stream) {
    int rc = fps_check(pts, start_host, out_idx, B, N, C, S, workspace, workspace_bytes);
    if (rc != PN2_OK || B == 0) return rc;
    if ((rc = fps_host_starts_check("pn2_fps_f32", start_host, B, N)) != PN2_OK) return rc;
    const FpsCall c = {fps_args(pts, N, C, sb, sn, sc, nullptr, S, out_idx, out_pts, out_packed, pts_packed), B,
                       static_cast<unsigned *>(workspace)};
    for (int64_t b0 = 0; b0 < B; b0 += kFpsArgStarts) {
        FpsCall k = fps_advance(c, b0);
        k.B = std::min<int64_t>(kFpsArgStarts, k.B);
        fps_host_starts(k.F.start, start_host + b0, k.B);
        if ((rc = fps_run(k, as_stream(stream))) != PN2_OK) return rc;
    }
    return PN2_OK;
}

extern "C" int pn2_fps_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                           int64_t sn, int64_t sc, const int64_t *start, int64_t S,
                           int64_t *out_idx, float *out_pts, float *out_packed, float *pts_packed,
                           void *stream) {
    return pn2_fps_ws_f32(pts, B, N, C, sb, sn, sc, start, S, out_idx, out_pts, out_packed, pts_packed, nullptr, 0,
                          stream);
}

// ------------------------------------------------------------------------- two-level FPS
// The shapes fps2_kernel takes: xyz clouds of up to kFps2MaxN points, S1 <= kFps2MaxS1, under the
// automatic 512 x 2 / 256 x 2 block choice (a forced block shape, or the fused pipelines' 256 x 4
// profile, keeps the two launches those were measured with).
extern "C" int pn2_fps2_eligible(int64_t N, int64_t C, int64_t S1, int64_t S2) {
    const Tuning T = tuning();
    return C == 3 && N >= 1 && N <= kFps2MaxN && S1 >= 1 && S1 <= kFps2MaxS1 && S2 >= 1 && S2 <= kFpsMaxS &&
           T.fps_threads == 0 && T.fps_ppt == 0 && T.fps_mid == 512;
}

extern "C" int pn2_fps2_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn,
                            int64_t sc, const int64_t *start1, int64_t S1, const int64_t *start2,
                            int64_t S2, int64_t *out_idx1, float *out_pts1, float *out_packed1,
                            float *pts_packed1, int64_t *out_idx2, float *out_pts2, float *out_packed2,
                            float *pts_packed2, void *stream) {
    PN2_REQUIRE(pts && start1 && start2 && out_idx1 && out_idx2, "pn2_fps2_f32: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= 1 && S1 >= 1 && S2 >= 1,
                "pn2_fps2_f32: bad shape B=%lld N=%lld C=%lld S1=%lld S2=%lld", (long long)B, (long long)N,
                (long long)C, (long long)S1, (long long)S2);
    if (!pn2_fps2_eligible(N, C, S1, S2))
        return set_error(PN2_EUNSUPPORTED,
                         "pn2_fps2_f32: N=%lld C=%lld S1=%lld S2=%lld is not a two-level shape "
                         "(pn2_fps2_eligible): run two pn2_fps_f32 launches",
                         (long long)N, (long long)C, (long long)S1, (long long)S2);
    if (B == 0) return PN2_OK;
    Fps2Args G;
    G.l1 = fps_args(pts, N, C, sb, sn, sc, start1, S1, out_idx1, out_pts1, out_packed1, pts_packed1);
    G.start2 = start2;
    G.S2 = (int)S2;
    G.out_idx2 = out_idx2;
    G.out_pts2 = out_pts2;
    G.out_packed2 = out_packed2;
    G.pts_packed2 = pts_packed2;
    hipStream_t st = as_stream(stream);
    if (N <= 512) {
        const size_t lds = fps2_block_lds(256, N, S1, S2);
        hipLaunchKernelGGL(fps2_kernel<256>, dim3((unsigned)B), dim3(256), lds, st, G);
    } else {
        const size_t lds = fps2_block_lds(512, N, S1, S2);  // <= 59 KB at the caps
        hipLaunchKernelGGL(fps2_kernel<512>, dim3((unsigned)B), dim3(512), lds, st, G);
    }
    PN2_LAUNCH_CHECK("fps2_kernel");
    return PN2_OK;
}

#ifdef PN2_FPS_STAMPS
extern "C" int pn2_debug_fps_stamps(unsigned long long *out) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fps_stamps), sizeof(g_fps_stamps)) == hipSuccess ? 0 : -1;
}
#endif

// ------------------------------------------------------------------------- FPS side jobs
int pn2::fps_side_check(const pn2_fps_side &f) {
    PN2_REQUIRE(f.start_host, "pn2_fps_side: null start_host");
    const int rc = fps_check(f.pts, f.start_host, f.out_idx, f.B, f.N, f.C, f.S, nullptr, 0);
    return rc != PN2_OK ? rc : fps_host_starts_check("pn2_fps_side", f.start_host, f.B, f.N);
}

int pn2::fps_side_launch(const pn2_fps_side &f, hipStream_t st) {
    return pn2_fps_host_ws_f32(f.pts, f.B, f.N, f.C, f.sb, f.sn, f.sc, f.start_host, f.S, f.out_idx, f.out_pts,
                               f.out_packed, f.pts_packed, nullptr, 0, st);
}

// The side job as workgroups of a chain launch (sa_chain_kernel<., ., 1, ., .>: fps_block<256, 2,
// C, true, true>, one workgroup per cloud): false when its shape does not fit that instance or
// its LDS exceeds the chain's
bool pn2::fps_side_block_args(const pn2_fps_side &f, size_t lds_avail, FpsArgs &F) {
    if (f.B < 1 || f.B > kFpsArgStarts || f.N > 512 || f.S > kFpsMaxS || (f.C != 3 && f.C != 10)) return false;
    if (fps_block_lds(256, (int)f.C, true, f.N, f.S) > lds_avail) return false;
    F = fps_args(f.pts, f.N, f.C, f.sb, f.sn, f.sc, nullptr, f.S, f.out_idx, f.out_pts, f.out_packed, f.pts_packed);
    fps_host_starts(F.start, f.start_host, f.B);
    return true;
}

extern "C" int pn2_pack_points_f32(const float *pts, int64_t B, int64_t N, int64_t C, int64_t sb,
                                   int64_t sn, int64_t sc, float *packed, void *stream) {
    PN2_REQUIRE(pts && packed, "pn2_pack_points_f32: null pointer");
    PN2_REQUIRE(B >= 0 && N >= 1 && C >= 1, "pn2_pack_points_f32: bad shape");
    if (C > kMaxCWide)
        return set_error(PN2_EUNSUPPORTED, "pn2_pack_points_f32: unsupported C=%lld (max %d)", (long long)C, kMaxCWide);
    if (B == 0) return PN2_OK;
    const int kind = layout_kind(sn, sc);
    const int64_t tot = B * N;
    const dim3 grid((unsigned)((tot + 255) / 256));
    const int cp = (int)pn2_packed_stride(C);
    if (C == 3)
        hipLaunchKernelGGL(pack_points_kernel<3>, grid, dim3(256), 0, as_stream(stream), pts, B,
                           (int)N, 3, sb, sn, sc, kind, packed, cp);
    else if (C <= kMaxC)
        hipLaunchKernelGGL(pack_points_kernel<kMaxC>, grid, dim3(256), 0, as_stream(stream), pts,
                           B, (int)N, (int)C, sb, sn, sc, kind, packed, cp);
    else
        hipLaunchKernelGGL(pack_points_kernel<kMaxCWide>, grid, dim3(256), 0, as_stream(stream), pts,
                           B, (int)N, (int)C, sb, sn, sc, kind, packed, cp);
    PN2_LAUNCH_CHECK("pack_points_kernel");
    return PN2_OK;
}
