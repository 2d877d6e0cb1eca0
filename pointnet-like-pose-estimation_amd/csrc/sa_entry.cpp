// sa_entry.cpp -- the SA MLP entry points (pn2_sa_mlp_max_f32 / _bf16 and their size queries):
// validation, the order in which the kernel families are tried, the callers' side jobs, and
// the report of what ran.  Host code only; the kernels and their planners are in sa_chain.hip
// (fused 3-layer chains), sa_dense.hip (layer by layer) and sa_mlp.hip (fp32 MFMA segments).
//
// A call is planned, fitted, launched and reported:
//   plan    each family's planner decides everything it can from the shapes and one Tuning
//           snapshot (MlpCall); the size query returns the largest of the plans' byte needs
//   fit     the launch runs the same plan against the caller's workspace: a chain without room
//           drops its pre-pass / compact table, a dense chain without room is not eligible
//   launch  the first eligible family, in the order of mlp_max below
//   report  the family fills an MlpReport; a successful call's becomes the thread's last
#include "pn2_internal.h"

#include <algorithm>

using namespace pn2;

namespace {

constexpr int kMaxLayers = 4;

// (every text names the fp32 entry: the checks are shared and callers match on them)
int validate(const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers, int64_t &M, int64_t &K) {
    PN2_REQUIRE(src && layers, "pn2_sa_mlp_max_f32: null pointer");
    PN2_REQUIRE(nlayers >= 1 && nlayers <= kMaxLayers, "pn2_sa_mlp_max_f32: nlayers=%d", nlayers);
    const pn2_sa_src &s = *src;
    int64_t cin0 = 0;
    switch (s.mode) {
    case PN2_SRC_GROUP_XYZ_FIRST:
    case PN2_SRC_GROUP_FEAT_FIRST:
        PN2_REQUIRE(s.pts && s.ctr && (s.idx || s.idx32) && (s.D == 0 || s.feat), "pn2_sa_mlp_max_f32: group source");
        PN2_REQUIRE(s.B >= 0 && s.N >= 1 && s.S >= 1 && s.K >= 1 && s.C >= 1 && s.D >= 0,
                    "pn2_sa_mlp_max_f32: bad group shape");
        M = s.B * s.S * s.K; cin0 = s.C + s.D; K = s.K;
        break;
    case PN2_SRC_GROUP_ALL:
        PN2_REQUIRE(s.pts && (s.D == 0 || s.feat), "pn2_sa_mlp_max_f32: group_all source");
        PN2_REQUIRE(s.B >= 0 && s.N >= 1 && s.C >= 1 && s.D >= 0, "pn2_sa_mlp_max_f32: bad group_all shape");
        M = s.B * s.N; cin0 = s.C + s.D; K = s.N;
        break;
    case PN2_SRC_ROWS:
        PN2_REQUIRE(s.rows && s.rs >= layers[0].cin, "pn2_sa_mlp_max_f32: rows source");
        PN2_REQUIRE(s.B >= 0 && s.S >= 1 && s.K >= 1, "pn2_sa_mlp_max_f32: bad rows shape");
        M = s.B * s.S * s.K; cin0 = layers[0].cin; K = s.K;
        break;
    default:
        return set_error(PN2_EINVAL, "pn2_sa_mlp_max_f32: mode %d", s.mode);
    }
    PN2_REQUIRE(M < (int64_t(1) << 31), "pn2_sa_mlp_max_f32: %lld rows exceed 2^31", (long long)M);
    PN2_REQUIRE(layers[0].cin == cin0, "pn2_sa_mlp_max_f32: layer0 cin %lld != source width %lld",
                (long long)layers[0].cin, (long long)cin0);
    for (int l = 0; l < nlayers; ++l) {
        const pn2_mlp_layer &q = layers[l];
        PN2_REQUIRE(q.wt && q.alpha && q.beta, "pn2_sa_mlp_max_f32: layer %d null", l);
        PN2_REQUIRE(q.cout % 32 == 0 && q.cout >= 32,
                    "pn2_sa_mlp_max_f32: layer %d cout=%lld not a multiple of 32", l, (long long)q.cout);
        if (l > 0)
            PN2_REQUIRE(q.cin == layers[l - 1].cout, "pn2_sa_mlp_max_f32: layer %d cin mismatch", l);
    }
    return PN2_OK;
}

// the src's zero side job on the paths whose kernels do not take it (the dense-layer path's
// last layer does)
int zero_side_job(const pn2_sa_src &s, hipStream_t st) {
    if (!s.zero_out || s.zero_count <= 0) return PN2_OK;
    const hipError_t e = hipMemsetAsync(s.zero_out, 0, (size_t)s.zero_count * 4, st);
    return e == hipSuccess ? PN2_OK : set_error(PN2_EHIP, "pn2_sa_mlp_max: zero_out: %s", hipGetErrorString(e));
}

thread_local MlpReport g_last;

// np = 3: fp32-accurate (split chain, split dense layers, else the fp32 MFMA kernels).
// np = 1: bf16 arithmetic (BASELINE config 5, the large-N stress run) -- the same chain / dense
// kernels with one bf16 plane per operand: activations rounded to bf16 (round-to-nearest-even)
// where a layer reads them, weights = the hi plane of the split image, products exact, fp32
// accumulation, BN / ReLU / max in fp32, fp32 output.  No fp32 fallback.
int mlp_max(const char *name, int np, const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers,
            int pool, float *out, int64_t ostride, float *workspace, int64_t workspace_bytes,
            void *stream) {
    const pn2_fps_side *side = src ? src->fps_side : nullptr;
    if (side) {
        const int rc = fps_side_check(*side);
        if (rc != PN2_OK) return rc;
    }
    int64_t M = 0, K = 1;
    int rc = validate(src, layers, nlayers, M, K);
    if (rc != PN2_OK) return rc;
    PN2_REQUIRE(out, "%s: null out", name);
    PN2_REQUIRE(ostride >= layers[nlayers - 1].cout, "%s: ostride", name);
    if (np == 1)
        for (int l = 0; l < nlayers; ++l)
            PN2_REQUIRE(layers[l].wt_split && ((uintptr_t)layers[l].wt_split & 15) == 0,
                        "%s: layer %d needs its 16-byte aligned split weight image", name, l);
    const MlpCall c{*src, layers, nlayers, pool, M, K, np, name, tuning(),
                    out, ostride, workspace, workspace_bytes, as_stream(stream)};
    MlpReport r = g_last;  // (a call over no rows launches nothing: path and planes stay)
    r.fps_side = side ? 0 : -1;
    if (M > 0) {
        if (pool) PN2_REQUIRE(M % K == 0, "%s: rows not a multiple of the group size", name);
        // 1. the fused chain kernel (takes the FPS side job when it can; not the zero side job)
        rc = try_launch_chain(c, r);
        if (rc > 0 && (rc = zero_side_job(*src, c.st)) == PN2_OK) rc = 1;
        // 2. split dense layers, one launch each (the last one runs the zero side job)
        if (rc == 0) rc = try_launch_dense(c, r);
        // 3. fp32 MFMA segments, after the zero side job
        if (rc == 0 && np == 3) {
            if ((rc = zero_side_job(*src, c.st)) != PN2_OK) return rc;
            rc = try_launch_f32(c, r);
        }
        if (rc < 0) return rc;
        if (rc == 0)
            return set_error(PN2_EUNSUPPORTED, "%s: no bf16 kernel for this chain (%d layers, mode %d) "
                             "or workspace too small", name, nlayers, src->mode);
        if (np == 1) r.path = PN2_PATH_BF16, r.planes = 1;
    }
    g_last = r;
    // the FPS side job as its own launch, after the MLP's, when the chain launch did not run it
    return side && r.fps_side == 0 ? fps_side_launch(*side, c.st) : PN2_OK;
}

int64_t workspace_bytes(int np, const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers) {
    int64_t M = 0, K = 1;
    if (validate(src, layers, nlayers, M, K) != PN2_OK) return -1;
    const MlpCall c{*src, layers, nlayers, 1, M, K, np, "", tuning(), nullptr, 0, nullptr, 0, nullptr};
    return std::max({chain_ws_bytes(c), dense_ws_bytes(c), np == 3 ? f32_ws_bytes(c) : 0});
}

}  // namespace

extern "C" int pn2_sa_mlp_last_path(void) { return g_last.path; }
extern "C" int pn2_sa_mlp_last_planes(void) { return g_last.planes; }
extern "C" int pn2_sa_mlp_last_fps_side(void) { return g_last.fps_side; }

extern "C" int pn2_sa_mlp_max_f32(const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers,
                                  int pool, float *out, int64_t ostride, float *workspace,
                                  int64_t workspace_bytes, void *stream) {
    return mlp_max("pn2_sa_mlp_max_f32", 3, src, layers, nlayers, pool, out, ostride, workspace,
                   workspace_bytes, stream);
}

extern "C" int pn2_sa_mlp_max_bf16(const pn2_sa_src *src, const pn2_mlp_layer *layers, int nlayers,
                                   int pool, float *out, int64_t ostride, float *workspace,
                                   int64_t workspace_bytes, void *stream) {
    return mlp_max("pn2_sa_mlp_max_bf16", 1, src, layers, nlayers, pool, out, ostride, workspace,
                   workspace_bytes, stream);
}

extern "C" int64_t pn2_sa_mlp_workspace_bytes(const pn2_sa_src *src, const pn2_mlp_layer *layers,
                                              int nlayers) {
    return workspace_bytes(3, src, layers, nlayers);
}

extern "C" int64_t pn2_sa_mlp_workspace_bytes_bf16(const pn2_sa_src *src, const pn2_mlp_layer *layers,
                                                   int nlayers) {
    return workspace_bytes(1, src, layers, nlayers);
}
