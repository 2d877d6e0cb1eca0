// bn_elem.h -- the per-element BatchNorm (+ ReLU) expressions of the training kernels, written
// once for train.hip (the SA layers' BN / ReLU / max sweeps) and fc_train.hip (the heads' FC
// layers).  Both units are compiled with -ffp-contract=off: every operation below rounds on its
// own, and the bits of A, dXn and the dgamma sum are the same in both files by construction.
// bn_act and bn_dxn spell their ReLU out instead of calling bn_relu / bn_gate (the forms for a
// layer without BN): nested, the compiler unswitched three of train.hip's sweeps on `relu`
// differently (other code sizes and register counts), and their code is meant to stay as measured.
#pragma once

namespace pn2 {

__device__ __forceinline__ float bn_xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }

// xhat for the dgamma sum.  The float32 one is off by up to 2 ulp per row, which the sum over M
// rows does not average below S2's own size: S2 is a sum of signed terms, about sqrt(M) of them
// in magnitude, so S2/M in dY lost digits on columns where it came out small (caught by
// tests/test_gpu_train_kernels.py at C = 2048, M = 8197: 7x the float32 bound of dY).
__device__ __forceinline__ double bn_xhat64(float y, float mean, float invstd) {
    return ((double)y - (double)mean) * (double)invstd;
}

__device__ __forceinline__ float bn_relu(float x, int relu) { return relu ? (x > 0.f ? x : 0.f) : x; }

// A = act(bn(y)); relu is uniform: no divergence
__device__ __forceinline__ float bn_act(float y, float mean, float invstd, float gamma, float beta, int relu) {
    const float x = bn_xhat(y, mean, invstd) * gamma + beta;
    return relu ? (x > 0.f ? x : 0.f) : x;
}

// the incoming gradient d behind the mask of a ReLU whose input was pre
__device__ __forceinline__ float bn_gate(float pre, float d, int relu) { return !relu || pre > 0.f ? d : 0.f; }

// dXn of one element
__device__ __forceinline__ float bn_dxn(float xhat, float gamma, float beta, float d, int relu) {
    return !relu || xhat * gamma + beta > 0.f ? d : 0.f;
}

}  // namespace pn2
