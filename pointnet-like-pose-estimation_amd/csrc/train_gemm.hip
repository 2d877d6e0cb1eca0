// train_gemm.hip -- the three matrix products of a shared-MLP layer's training step, with a
// fixed summation order (include/pn2.h states the contracts):
//   pn2_gemm_nt_f32   Y  = X W^T + b      C[M,N] = A[M,K] B[N,K]^T (+ bias)
//   pn2_gemm_nn_f32   dX = dY W           C[M,N] = A[M,K] B[K,N]
//   pn2_gemm_tn_f32   dW = dY^T X         C[N,K] = A[M,N]^T B[M,K]   (the sum over rows)
//
// Reference: the Conv2d 1x1 / Conv1d 1x1 of the shared MLPs under autograd,
// /root/reference/model/pointnet2_utils.py:167-172, 211-218 (pn2/train.py _MlpMaxTrain).
//
// One kernel template serves the three: out[i][j] = sum_l a(i,l) * b(j,l) over a range of l,
// where an operand is either stored with l contiguous ("rows": a(i,l) = A[i*ld + l]) or with
// its own index contiguous ("columns": a(i,l) = A[l*ld + i]).  nt = rows x rows, nn = rows x
// columns, tn = columns x columns.  Arithmetic is split_bf16.h's: every operand value goes
// into three bf16 planes (split8), a product step is six v_mfma_f32_32x32x16_bf16 (mma6_wb).
//
// A workgroup of 4 waves owns a 128 x 64 output tile (wave w the rows 32w .. 32w+31, two 32x32
// accumulators) and walks l in blocks of 32, i.e. two ascending 16-wide MFMA steps:
//   - every thread fetches, for its share of the tile's (row, 8 consecutive l) groups, the 8
//     float32 values into registers: a "rows" operand by two 16-byte loads when the base and
//     the leading dimension allow, else by dword loads; a "columns" operand by 8 dword loads
//     that are coalesced across the lanes (consecutive i).  Anything past the operand's edge or
//     the l range is a zero in the register: no load is issued for it;
//   - splits them and stores the planes as 16-byte fragments in LDS, [plane][l group][row]
//     with the l-group stride padded by two fragments (the stores of a "rows" operand -- 8
//     consecutive lanes hold 2 rows x 4 l groups -- then fall on 8 distinct 16-byte slots of the
//     128-byte bank row; the fragment reads take 16 consecutive rows: conflict-free);
//   - the next block's global loads are issued before the MFMAs of the current one.
// The order of an output element's sum is fixed by the l range alone: +0, then ascending
// 16-wide steps, each in mma6_wb's plane order; a step that lies wholly past the range is
// skipped (it would add exact zeros).  Nothing depends on the grid, the row count of a "rows"
// operand or the element's position in a tile.
//
// tn cuts the rows into slabs of kTgSlab; slab j's workgroups (blockIdx.z = j) sum the rows
// [j*kTgSlab, min((j+1)*kTgSlab, M)) and store their partial in the workspace; a second launch
// adds the partials in ascending j in float64 and rounds once.  No atomics, no inter-workgroup
// wait.
#include "pn2_internal.h"
#include "split_bf16.h"

namespace pn2 {

constexpr int kTgTI = 128;      // output rows per workgroup
constexpr int kTgTJ = 64;       // output columns per workgroup
constexpr int kTgBL = 32;       // reduction elements per block (two MFMA steps)
constexpr int kTgLG = kTgBL / 8;  // 8-element groups per block
constexpr int kTgThreads = 256;
constexpr int kTgSlab = 2048;   // tn: rows per slab (pn2_gemm_tn_slab_rows)
constexpr int kTgMax = 4096;    // largest N, K
static_assert(kTgSlab % kTgBL == 0, "a slab is whole reduction blocks");

struct TgFrag {
    float v[8];
};

// the 8 values (row r0 + row, l .. l+7) of an operand; zeros outside [0, rows) x [.., lend)
template <bool COLS>
__device__ __forceinline__ TgFrag tg_fetch(const float *__restrict__ X, int64_t ld, int64_t r0,
                                           int row, int64_t rows, int64_t l, int64_t lend, bool vec) {
    TgFrag f;
    const int64_t r = r0 + row;
    if constexpr (COLS) {
        const float *p = X + l * ld + r;
#pragma unroll
        for (int j = 0; j < 8; ++j) f.v[j] = (r < rows && l + j < lend) ? p[j * ld] : 0.f;
    } else {
        const float *p = X + r * ld + l;
        if (vec && r < rows && l + 8 <= lend) {
            const float4 a = *reinterpret_cast<const float4 *>(p);
            const float4 b = *reinterpret_cast<const float4 *>(p + 4);
            f.v[0] = a.x, f.v[1] = a.y, f.v[2] = a.z, f.v[3] = a.w;
            f.v[4] = b.x, f.v[5] = b.y, f.v[6] = b.z, f.v[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) f.v[j] = (r < rows && l + j < lend) ? p[j] : 0.f;
        }
    }
    return f;
}

// group g of a TR-row operand tile -> (row, l group).  "rows": the 4 l groups of a row on 4
// consecutive lanes (32 contiguous floats per row); "columns": consecutive lanes on
// consecutive rows (coalesced dwords)
template <int TR, bool COLS>
__device__ __forceinline__ void tg_where(int g, int &row, int &lg) {
    if constexpr (COLS) {
        row = g % TR;
        lg = g / TR;
    } else {
        row = g / kTgLG;
        lg = g % kTgLG;
    }
}

template <int TR>
__device__ __forceinline__ void tg_store(bf16x8 *lds, int row, int lg, const TgFrag &f) {
    const Split s = split8(f.v);
    bf16x8 *q = lds + lg * (TR + 2) + row;
    q[0] = s.h;
    q[kTgLG * (TR + 2)] = s.m;
    q[2 * kTgLG * (TR + 2)] = s.l;
}

template <int TR>
__device__ __forceinline__ Split tg_load(const bf16x8 *lds, int row, int lg) {
    const bf16x8 *q = lds + lg * (TR + 2) + row;
    Split s;
    s.h = q[0];
    s.m = q[kTgLG * (TR + 2)];
    s.l = q[2 * kTgLG * (TR + 2)];
    return s;
}

// out[i][j] = sum_{l in [l0, l1)} a(i,l) b(j,l) (+ bias[j]), i < I, j < J; blockIdx.z = slab:
// l0 = z * slab, l1 = min(l0 + slab, L), out += z * out_slab
template <bool ACOLS, bool BCOLS>
__global__ __launch_bounds__(kTgThreads) void tg_kernel(const float *__restrict__ A, int64_t lda,
                                                        const float *__restrict__ B, int64_t ldb,
                                                        const float *__restrict__ bias,
                                                        float *__restrict__ out, int64_t ldo,
                                                        int64_t out_slab, int64_t I, int J, int64_t L,
                                                        int64_t slab, bool veca, bool vecb) {
    constexpr int NA = kTgTI * kTgLG / kTgThreads;  // 2 groups per thread
    constexpr int NB = kTgTJ * kTgLG / kTgThreads;  // 1
    __shared__ bf16x8 lds_a[3 * kTgLG * (kTgTI + 2)];
    __shared__ bf16x8 lds_b[3 * kTgLG * (kTgTJ + 2)];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * kTgTI;
    const int64_t j0 = (int64_t)blockIdx.y * kTgTJ;
    const int64_t l0 = (int64_t)blockIdx.z * slab;
    const int64_t l1 = l0 + slab < L ? l0 + slab : L;
    out += (int64_t)blockIdx.z * out_slab;

    int arow[NA], alg[NA], brow[NB], blg[NB];
#pragma unroll
    for (int q = 0; q < NA; ++q) tg_where<kTgTI, ACOLS>(tid + q * kTgThreads, arow[q], alg[q]);
#pragma unroll
    for (int q = 0; q < NB; ++q) tg_where<kTgTJ, BCOLS>(tid + q * kTgThreads, brow[q], blg[q]);

    TgFrag fa[NA], fb[NB];
#pragma unroll
    for (int q = 0; q < NA; ++q) fa[q] = tg_fetch<ACOLS>(A, lda, i0, arow[q], I, l0 + alg[q] * 8, l1, veca);
#pragma unroll
    for (int q = 0; q < NB; ++q) fb[q] = tg_fetch<BCOLS>(B, ldb, j0, brow[q], J, l0 + blg[q] * 8, l1, vecb);

    cfloatx16 acc0 = {0.f}, acc1 = {0.f};
#pragma unroll
    for (int e = 0; e < 16; ++e) acc0[e] = 0.f, acc1[e] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    for (int64_t l = l0; l < l1; l += kTgBL) {
#pragma unroll
        for (int q = 0; q < NA; ++q) tg_store<kTgTI>(lds_a, arow[q], alg[q], fa[q]);
#pragma unroll
        for (int q = 0; q < NB; ++q) tg_store<kTgTJ>(lds_b, brow[q], blg[q], fb[q]);
        __syncthreads();
        const int64_t ln = l + kTgBL;
        if (ln < l1) {  // the next block's loads fly during this block's MFMAs
#pragma unroll
            for (int q = 0; q < NA; ++q)
                fa[q] = tg_fetch<ACOLS>(A, lda, i0, arow[q], I, ln + alg[q] * 8, l1, veca);
#pragma unroll
            for (int q = 0; q < NB; ++q)
                fb[q] = tg_fetch<BCOLS>(B, ldb, j0, brow[q], J, ln + blg[q] * 8, l1, vecb);
        }
#pragma unroll
        for (int s = 0; s < kTgBL / 16; ++s) {
            if (l + 16 * s < l1) {  // workgroup-uniform: a step wholly past the range adds zeros
                const Split a = tg_load<kTgTI>(lds_a, wave * 32 + fr, 2 * s + fh);
                const Split b0 = tg_load<kTgTJ>(lds_b, fr, 2 * s + fh);
                const Split b1 = tg_load<kTgTJ>(lds_b, 32 + fr, 2 * s + fh);
                acc0 = mma6_wb(a, b0, acc0);
                acc1 = mma6_wb(a, b1, acc1);
            }
        }
        __syncthreads();
    }

    // accumulator element e of lane (fr, fh): row (e&3) + 8*(e>>2) + 4*fh, column fr
    const int64_t ja = j0 + fr, jb = j0 + 32 + fr;
    const float ba = (bias && ja < J) ? bias[ja] : 0.f;
    const float bb = (bias && jb < J) ? bias[jb] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t i = i0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (i < I) {
            float *o = out + i * ldo;
            if (ja < J) o[ja] = bias ? acc0[e] + ba : acc0[e];
            if (jb < J) o[jb] = bias ? acc1[e] + bb : acc1[e];
        }
    }
}

// C[e] = float32(sum_j double(P_j[e])), ascending j from +0.0
__global__ __launch_bounds__(256) void tg_reduce_kernel(const float *__restrict__ part, int64_t slabs,
                                                        int64_t NK, int K, float *__restrict__ C,
                                                        int64_t ldc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= NK) return;
    double s = 0.0;
    for (int64_t j = 0; j < slabs; ++j) s += (double)part[j * NK + e];
    C[(e / K) * ldc + e % K] = (float)s;
}

static inline bool tg_vec(const float *p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

static int tg_check(const char *what, const void *A, const void *B, const void *C, int64_t M,
                    int64_t N, int64_t K, bool lds_ok) {
    if (!A || !B || !C) return set_error(PN2_EINVAL, "%s: null pointer", what);
    if (M < 0 || N < 1 || K < 1)
        return set_error(PN2_EINVAL, "%s: bad shape M=%lld N=%lld K=%lld", what, (long long)M,
                         (long long)N, (long long)K);
    if (N > kTgMax || K > kTgMax)
        return set_error(PN2_EUNSUPPORTED, "%s: N=%lld K=%lld above %d", what, (long long)N, (long long)K,
                         kTgMax);
    if (!lds_ok) return set_error(PN2_EINVAL, "%s: a leading dimension is below its matrix width", what);
    return PN2_OK;
}

static inline int64_t tg_slabs(int64_t M) { return (M + kTgSlab - 1) / kTgSlab; }

}  // namespace pn2

using namespace pn2;

extern "C" int pn2_gemm_nt_f32(const float *A, int64_t lda, const float *B, int64_t ldb,
                               const float *bias, float *C, int64_t ldc, int64_t M, int64_t N,
                               int64_t K, void *stream) {
    const int rc = tg_check("pn2_gemm_nt_f32", A, B, C, M, N, K, lda >= K && ldb >= K && ldc >= N);
    if (rc != PN2_OK) return rc;
    if (M == 0) return PN2_OK;
    const int64_t gx = (M + kTgTI - 1) / kTgTI;
    if (gx >= (1ll << 31))
        return set_error(PN2_EUNSUPPORTED, "pn2_gemm_nt_f32: M=%lld too large", (long long)M);
    hipLaunchKernelGGL((tg_kernel<false, false>), dim3((unsigned)gx, (unsigned)((N + kTgTJ - 1) / kTgTJ)),
                       dim3(kTgThreads), 0, as_stream(stream), A, lda, B, ldb, bias, C, ldc, (int64_t)0,
                       M, (int)N, K, K, tg_vec(A, lda), tg_vec(B, ldb));
    PN2_LAUNCH_CHECK("pn2_gemm_nt_f32");
    return PN2_OK;
}

extern "C" int pn2_gemm_nn_f32(const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                               int64_t ldc, int64_t M, int64_t N, int64_t K, void *stream) {
    const int rc = tg_check("pn2_gemm_nn_f32", A, B, C, M, N, K, lda >= K && ldb >= N && ldc >= N);
    if (rc != PN2_OK) return rc;
    if (M == 0) return PN2_OK;
    const int64_t gx = (M + kTgTI - 1) / kTgTI;
    if (gx >= (1ll << 31))
        return set_error(PN2_EUNSUPPORTED, "pn2_gemm_nn_f32: M=%lld too large", (long long)M);
    hipLaunchKernelGGL((tg_kernel<false, true>), dim3((unsigned)gx, (unsigned)((N + kTgTJ - 1) / kTgTJ)),
                       dim3(kTgThreads), 0, as_stream(stream), A, lda, B, ldb, (const float *)nullptr, C,
                       ldc, (int64_t)0, M, (int)N, K, K, tg_vec(A, lda), false);
    PN2_LAUNCH_CHECK("pn2_gemm_nn_f32");
    return PN2_OK;
}

extern "C" int64_t pn2_gemm_tn_slab_rows(void) { return kTgSlab; }

extern "C" int64_t pn2_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    if (M < 0 || N < 1 || K < 1 || N > kTgMax || K > kTgMax) return -1;
    return tg_slabs(M) * N * K * 4;
}

extern "C" int pn2_gemm_tn_f32(const float *A, int64_t lda, const float *B, int64_t ldb, float *C,
                               int64_t ldc, int64_t M, int64_t N, int64_t K, void *ws,
                               int64_t ws_bytes, void *stream) {
    const int rc = tg_check("pn2_gemm_tn_f32", A, B, C, M, N, K, lda >= N && ldb >= K && ldc >= K);
    if (rc != PN2_OK) return rc;
    const int64_t slabs = tg_slabs(M), need = slabs * N * K * 4;
    PN2_REQUIRE(need == 0 || (ws && ((uintptr_t)ws & 3) == 0 && ws_bytes >= need),
                "pn2_gemm_tn_f32: workspace too small (%lld bytes, need %lld)", (long long)ws_bytes,
                (long long)need);
    if (M == 0) return PN2_OK;
    if (slabs > 65535)
        return set_error(PN2_EUNSUPPORTED, "pn2_gemm_tn_f32: M=%lld too large", (long long)M);
    hipStream_t st = as_stream(stream);
    float *part = static_cast<float *>(ws);
    hipLaunchKernelGGL((tg_kernel<true, true>),
                       dim3((unsigned)((N + kTgTI - 1) / kTgTI), (unsigned)((K + kTgTJ - 1) / kTgTJ),
                            (unsigned)slabs),
                       dim3(kTgThreads), 0, st, A, lda, B, ldb, (const float *)nullptr, part, K, N * K, N,
                       (int)K, M, (int64_t)kTgSlab, false, false);
    PN2_LAUNCH_CHECK("pn2_gemm_tn_f32");
    hipLaunchKernelGGL(tg_reduce_kernel, dim3((unsigned)((N * K + 255) / 256)), dim3(256), 0, st, part,
                       slabs, N * K, (int)K, C, ldc);
    PN2_LAUNCH_CHECK("pn2_gemm_tn_f32 (reduce)");
    return PN2_OK;
}
