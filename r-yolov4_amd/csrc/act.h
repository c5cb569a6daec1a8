// The activations of the conv stack (Mish | LeakyReLU(.1) | SiLU) and their derivatives, stated once for every kernel that applies them: the
// BatchNorm + activation passes (elementwise.hip), the inference epilogues of the GEMM-shaped kernels and the first-layer kernels (stem.hip).
// The recompute stem, the fused stem backward and the inference epilogues must give the bits of the unfused training passes; they do because
// all of them call the arms below.  The codes are the ones engine/structs.py passes (tests/test_act_codes_cpu.py holds the two together).
#pragma once
#include "common.h"

enum { ACT_LINEAR = 0, ACT_MISH = 1, ACT_LEAKY = 2, ACT_SILU = 3 };

// Every arm costs ONE v_exp_f32 and one/two v_rcp_f32 per element (no IEEE division, no libm): the elementwise kernels move 4-6 bytes per
// element, so a libm tanhf/log1pf or a correctly-rounded divide per element makes them VALU-bound instead of HBM-bound.
// Mish uses tanh(softplus(u)) = (n^2 + 2n) / (n^2 + 2n + 2) with n = e^u; its arms are the expressions below the `u > 20` cut-off, which the
// callers apply (as an early return in the scalar chains, as a select in the vector forms).
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }

__device__ __forceinline__ float silu_f(float u) { return u * rcp(1.f + __expf(-u)); }
__device__ __forceinline__ float silu_d(float u) { const float s = rcp(1.f + __expf(-u)); return s * (1.f + u * (1.f - s)); }
__device__ __forceinline__ float leaky_f(float u) { return u > 0.f ? u : 0.1f * u; }
__device__ __forceinline__ float leaky_d(float u) { return u > 0.f ? 1.f : 0.1f; }
__device__ __forceinline__ float mish_f(float u)
{
    const float n = __expf(u), w = n * (n + 2.f);
    return u * w * rcp(w + 2.f);
}
__device__ __forceinline__ float mish_d(float u)
{
    const float n = __expf(u), w = n * (n + 2.f);
    const float t = w * rcp(w + 2.f);                 // tanh(softplus(u))
    const float sg = n * rcp(1.f + n);                // sigmoid(u)
    return t + u * (1.f - t * t) * sg;
}

// act(u) and d act / du of one value
__device__ __forceinline__ float act_fwd(float u, int act)
{
    if (act == ACT_SILU) return silu_f(u);
    if (act == ACT_LEAKY) return leaky_f(u);
    if (act == ACT_MISH) {
        if (u > 20.f) return u;
        return mish_f(u);
    }
    return u;
}
__device__ __forceinline__ float act_bwd(float u, int act)
{
    if (act == ACT_SILU) return silu_d(u);
    if (act == ACT_LEAKY) return leaky_d(u);
    if (act == ACT_MISH) {
        if (u > 20.f) return 1.f;
        return mish_d(u);
    }
    return 1.f;
}

// Folded BatchNorm + activation of N accumulator values (inference epilogues, EPI_AFFINE_ACT): v[q] = act(v[q] * sc[q] + sf[q]).  `act` is
// wave-uniform; called per element through act_fwd every value paid the whole `if` chain (three scalar compare + branch pairs, and Mish's
// `u > 20` early return as a DIVERGENT branch: 1 008 s_cbranch in the affine instantiation of the persistent pointwise kernel, r06 ISA count).  Here
// the chain is walked once per N values and every arm is branch-free (the Mish cut-off as a select).
template <int N> __device__ __forceinline__ void act_affine_vec(float (&v)[N], const float (&sc)[N], const float (&sf)[N], int act)
{
    if (act == ACT_SILU) {
#pragma unroll
        for (int q = 0; q < N; q++) v[q] = silu_f(v[q] * sc[q] + sf[q]);
    } else if (act == ACT_MISH) {
#pragma unroll
        for (int q = 0; q < N; q++) {
            const float u = v[q] * sc[q] + sf[q];
            const float r = mish_f(u);
            v[q] = u > 20.f ? u : r;
        }
    } else if (act == ACT_LEAKY) {
#pragma unroll
        for (int q = 0; q < N; q++) v[q] = leaky_f(v[q] * sc[q] + sf[q]);
    } else {
#pragma unroll
        for (int q = 0; q < N; q++) v[q] = v[q] * sc[q] + sf[q];
    }
}
__device__ __forceinline__ void act_affine_quad(float (&v)[4], const float (&sc)[4], const float (&sf)[4], int act) { act_affine_vec<4>(v, sc, sf, act); }

// d act / du of N values with ONE walk of the (wave-uniform) activation chain and branch-free arms.  The fused first-layer backward (stem.hip)
// is instruction-rate bound: per element the chain was three scalar compare + branch pairs plus a divergent early return.
template <int N> __device__ __forceinline__ void act_bwd_vec(const float (&u)[N], float (&d)[N], int act)
{
    if (act == ACT_SILU) {
#pragma unroll
        for (int q = 0; q < N; q++) d[q] = silu_d(u[q]);
    } else if (act == ACT_MISH) {
#pragma unroll
        for (int q = 0; q < N; q++) {
            const float r = mish_d(u[q]);
            d[q] = u[q] > 20.f ? 1.f : r;
        }
    } else if (act == ACT_LEAKY) {
#pragma unroll
        for (int q = 0; q < N; q++) d[q] = leaky_d(u[q]);
    } else {
#pragma unroll
        for (int q = 0; q < N; q++) d[q] = 1.f;
    }
}
