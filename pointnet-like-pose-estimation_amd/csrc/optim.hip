// optim.hip -- the optimizer phase of a train step as ONE launch over every tensor of the step
// (include/pn2.h states the contract and the arithmetic rule):
//   pn2_adam_step_f32   torch.optim.Adam's update (no amsgrad, no maximize)
//   pn2_sgd_step_f32    torch.optim.SGD's update (momentum, dampening, weight decay; no nesterov)
//
// Reference: every train script builds torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-08,
// weight_decay=args.decay_rate) or SGD(lr=0.01, momentum=0.9) and steps it after every batch
// (train_classification.py:88-101, 128; train_rotation.py, train_translation.py, train_sign.py
// alike); pn2/optim.py is the host side.
//
// A PointNet++ head has ~46 parameter tensors from 64 elements (a BatchNorm vector) to 512 K (an
// FC or sa3 weight), 1.5 M elements in all: ~40 MB of traffic, microseconds of device time, so
// what counts is that it is one launch and that a captured launch replays correctly.
//   - a device table of descriptors (pn2_optim_tensor) says where each tensor's p, g, m, v are;
//   - a device job table maps workgroup -> (tensor, chunk of kOptimChunk elements);
//   - the step's scalars (step size, bias correction, betas, eps, weight decay) are read from
//     device memory -- never kernel arguments -- so a replay sees the values the host wrote for
//     THAT step.
// No LDS, no atomics, no cross-lane traffic: an element depends on its own p, g, m, v only, and
// computes the same bits on the 16-byte path and on the dword path.
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile) and every operation of the rule
// goes through add_rn / mul_rn / div_rn / sqrt_rn: one correctly rounded IEEE float32 operation
// each.  div_rn and sqrt_rn are the plain operator and sqrtf, which hipcc expands to the
// correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 plus the
// one-ulp correction by residuals) -- NOT __fsqrt_rn, which the HIP headers map to the native
// square root (1 ulp).  The only fused multiply-adds in the device code are those inside these
// two expansions.
#include "pn2_internal.h"

namespace pn2 {

constexpr int kOptimThreads = 256;
constexpr int kOptimChunk = 2048;  // elements per workgroup: two 16-byte pieces per thread and array
constexpr int kOptimScalars = 8;   // floats per scalar block
constexpr int64_t kOptimMaxJobs = 1ll << 30;
static_assert(kOptimChunk == kOptimThreads * 8, "two float4 per thread");

typedef float pn2_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return sqrtf(a); }

struct AdamScalars {
    float ss, bc2_sqrt, omb1, b2, omb2, eps, wd;
};
struct SgdScalars {
    float lr, mu, omd, wd, first;
};

__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamScalars &s) {
#pragma clang fp contract(off)
    if (s.wd != 0.f) g = add_rn(g, mul_rn(s.wd, p));
    m = add_rn(m, mul_rn(s.omb1, add_rn(g, -m)));
    v = mul_rn(v, s.b2);
    v = add_rn(v, mul_rn(mul_rn(s.omb2, g), g));
    const float den = add_rn(div_rn(sqrt_rn(v), s.bc2_sqrt), s.eps);
    p = add_rn(p, mul_rn(s.ss, div_rn(m, den)));
}

// has_buf: the tensor has a momentum buffer (uniform per workgroup)
__device__ __forceinline__ void sgd_elem(float &p, float g, float &buf, bool has_buf, const SgdScalars &s) {
#pragma clang fp contract(off)
    if (s.wd != 0.f) g = add_rn(g, mul_rn(s.wd, p));
    if (has_buf) {
        buf = s.first != 0.f ? g : add_rn(mul_rn(buf, s.mu), mul_rn(s.omd, g));
        g = buf;
    }
    p = add_rn(p, -mul_rn(s.lr, g));
}

// the (tensor, first element, element count) of this workgroup; false: nothing to do.  Every
// index read from the tables is checked against the launch's own bounds before it is used.
__device__ __forceinline__ bool optim_job(const pn2_optim_tensor *__restrict__ T, int ntensors,
                                          const int2 *__restrict__ jobs, int nblocks, pn2_optim_tensor &t,
                                          int64_t &base, int &cnt) {
    const int2 job = jobs[blockIdx.x];
    if ((unsigned)job.x >= (unsigned)ntensors || job.y < 0) return false;
    t = T[job.x];
    if (t.scalars < 0 || t.scalars >= nblocks) return false;
    base = (int64_t)job.y * kOptimChunk;
    if (base >= t.n) return false;
    const int64_t left = t.n - base;
    cnt = left < kOptimChunk ? (int)left : kOptimChunk;
    return true;
}

__device__ __forceinline__ bool aligned16(const void *a, const void *b, const void *c, const void *d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

__global__ __launch_bounds__(kOptimThreads) void adam_step_kernel(const pn2_optim_tensor *__restrict__ T, int ntensors,
                                                                  const int2 *__restrict__ jobs,
                                                                  const float *__restrict__ S, int nblocks) {
    pn2_optim_tensor t;
    int64_t base;
    int cnt;
    if (!optim_job(T, ntensors, jobs, nblocks, t, base, cnt)) return;
    const float *sb = S + t.scalars * kOptimScalars;
    const AdamScalars s = {sb[0], sb[1], sb[2], sb[3], sb[4], sb[5], sb[6]};
    float *p = t.p + base, *m = t.m + base, *v = t.v + base;
    const float *g = t.g + base;
    if (cnt == kOptimChunk && aligned16(t.p, t.g, t.m, t.v)) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = r * kOptimThreads + threadIdx.x;
            pn2_f4 p4 = ((pn2_f4 *)p)[i], m4 = ((pn2_f4 *)m)[i], v4 = ((pn2_f4 *)v)[i];
            const pn2_f4 g4 = ((const pn2_f4 *)g)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p4[k], mk = m4[k], vk = v4[k];
                adam_elem(pk, g4[k], mk, vk, s);
                p4[k] = pk, m4[k] = mk, v4[k] = vk;
            }
            ((pn2_f4 *)p)[i] = p4, ((pn2_f4 *)m)[i] = m4, ((pn2_f4 *)v)[i] = v4;
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += kOptimThreads) {
            float pk = p[i], mk = m[i], vk = v[i];
            adam_elem(pk, g[i], mk, vk, s);
            p[i] = pk, m[i] = mk, v[i] = vk;
        }
    }
}

__global__ __launch_bounds__(kOptimThreads) void sgd_step_kernel(const pn2_optim_tensor *__restrict__ T, int ntensors,
                                                                 const int2 *__restrict__ jobs,
                                                                 const float *__restrict__ S, int nblocks) {
    pn2_optim_tensor t;
    int64_t base;
    int cnt;
    if (!optim_job(T, ntensors, jobs, nblocks, t, base, cnt)) return;
    const float *sb = S + t.scalars * kOptimScalars;
    const SgdScalars s = {sb[0], sb[1], sb[2], sb[3], sb[4]};
    const bool has_buf = t.m != nullptr;
    float *p = t.p + base, *m = has_buf ? t.m + base : nullptr;
    const float *g = t.g + base;
    if (cnt == kOptimChunk && aligned16(t.p, t.g, t.m, nullptr)) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = r * kOptimThreads + threadIdx.x;
            pn2_f4 p4 = ((pn2_f4 *)p)[i], m4 = {0.f, 0.f, 0.f, 0.f};
            // the first step writes the buffer without reading it
            if (has_buf && s.first == 0.f) m4 = ((pn2_f4 *)m)[i];
            const pn2_f4 g4 = ((const pn2_f4 *)g)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p4[k], mk = m4[k];
                sgd_elem(pk, g4[k], mk, has_buf, s);
                p4[k] = pk, m4[k] = mk;
            }
            ((pn2_f4 *)p)[i] = p4;
            if (has_buf) ((pn2_f4 *)m)[i] = m4;
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += kOptimThreads) {
            float pk = p[i], mk = (has_buf && s.first == 0.f) ? m[i] : 0.f;
            sgd_elem(pk, g[i], mk, has_buf, s);
            p[i] = pk;
            if (has_buf) m[i] = mk;
        }
    }
}

// everything the host can know: the mirror of the descriptor table, and both tables' lengths
static int optim_check(const char *name, bool adam, const pn2_optim_tensor *host, const pn2_optim_tensor *tensors,
                       int64_t ntensors, const int32_t *jobs, int64_t njobs, const float *scalars, int64_t nblocks) {
    PN2_REQUIRE(host && tensors && jobs && scalars, "%s: null pointer", name);
    PN2_REQUIRE(ntensors >= 1 && ntensors < (1ll << 31) && nblocks >= 1 && nblocks < (1ll << 31),
                "%s: bad table length (ntensors=%lld nblocks=%lld)", name, (long long)ntensors, (long long)nblocks);
    int64_t need = 0;
    for (int64_t i = 0; i < ntensors; ++i) {
        const pn2_optim_tensor &t = host[i];
        PN2_REQUIRE(t.p && t.g && (!adam || (t.m && t.v)), "%s: null pointer in tensor %lld", name, (long long)i);
        PN2_REQUIRE(t.n >= 1 && t.n < (1ll << 31), "%s: bad count n=%lld of tensor %lld (1 <= n < 2^31)", name,
                    (long long)t.n, (long long)i);
        PN2_REQUIRE(t.scalars >= 0 && t.scalars < nblocks, "%s: scalar index %lld of tensor %lld outside [0, %lld)",
                    name, (long long)t.scalars, (long long)i, (long long)nblocks);
        need += (t.n + kOptimChunk - 1) / kOptimChunk;
    }
    PN2_REQUIRE(njobs == need, "%s: job table length %lld does not match the tensors' %lld chunks", name,
                (long long)njobs, (long long)need);
    if (njobs > kOptimMaxJobs)
        return set_error(PN2_EUNSUPPORTED, "%s: %lld chunks > 2^30", name, (long long)njobs);
    return PN2_OK;
}

}  // namespace pn2

extern "C" int64_t pn2_optim_chunk(void) { return pn2::kOptimChunk; }
extern "C" int64_t pn2_optim_scalars(void) { return pn2::kOptimScalars; }

extern "C" int pn2_adam_step_f32(const pn2_optim_tensor *tensors_host, const pn2_optim_tensor *tensors,
                                 int64_t ntensors, const int32_t *jobs, int64_t njobs, const float *scalars,
                                 int64_t nblocks, void *stream) {
    if (const int rc = pn2::optim_check("pn2_adam_step_f32", true, tensors_host, tensors, ntensors, jobs, njobs,
                                        scalars, nblocks))
        return rc;
    pn2::adam_step_kernel<<<dim3((unsigned)njobs), dim3(pn2::kOptimThreads), 0, pn2::as_stream(stream)>>>(
        tensors, (int)ntensors, (const int2 *)jobs, scalars, (int)nblocks);
    PN2_LAUNCH_CHECK("pn2_adam_step_f32");
    return PN2_OK;
}

extern "C" int pn2_sgd_step_f32(const pn2_optim_tensor *tensors_host, const pn2_optim_tensor *tensors,
                                int64_t ntensors, const int32_t *jobs, int64_t njobs, const float *scalars,
                                int64_t nblocks, void *stream) {
    if (const int rc = pn2::optim_check("pn2_sgd_step_f32", false, tensors_host, tensors, ntensors, jobs, njobs,
                                        scalars, nblocks))
        return rc;
    pn2::sgd_step_kernel<<<dim3((unsigned)njobs), dim3(pn2::kOptimThreads), 0, pn2::as_stream(stream)>>>(
        tensors, (int)ntensors, (const int2 *)jobs, scalars, (int)nblocks);
    PN2_LAUNCH_CHECK("pn2_sgd_step_f32");
    return PN2_OK;
}
