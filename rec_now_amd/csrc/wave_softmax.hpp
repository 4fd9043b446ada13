// Wave-level pieces of a softmax held in registers, shared by csrc/autoint.hip and csrc/afm.hip: the DPP / crossbar reductions of four
// values at once and the compensated exponential.  Included after common.hpp.
#pragma once

// Wave reductions of four values at once (the four queries of a block: four independent chains hide each other's latency).  Every step
// exchanges between lane PAIRS (l <-> l ^ 1, l ^ 2, 7 - l and 15 - l inside a row of 16 lanes by DPP, l ^ 16 and l ^ 32 through the LDS
// crossbar), so both partners form the same sum and all lanes end with the same bits.  n2 is a power of two >= F; lanes >= F hold the
// neutral element, and the steps across rows are skipped when F fits 16 or 32 lanes.
template <int CTRL>
__device__ __forceinline__ float ai_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
#define AI_DPP_XOR1 0xB1                        // quad_perm [1, 0, 3, 2]
#define AI_DPP_XOR2 0x4E                        // quad_perm [2, 3, 0, 1]
#define AI_DPP_HALF_MIRROR 0x141                // lane l of a row <- lane 7 - l of its half
#define AI_DPP_MIRROR 0x140                     // lane l of a row <- lane 15 - l
template <bool MAX>
__device__ __forceinline__ float ai_comb(float a, float b) { return MAX ? (b > a ? b : a) : a + b; }
template <bool MAX>
__device__ __forceinline__ rn_f4 ai_wave_red4(rn_f4 v, int n2) {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], ai_dpp<AI_DPP_XOR1>(v[u]));
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], ai_dpp<AI_DPP_XOR2>(v[u]));
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], ai_dpp<AI_DPP_HALF_MIRROR>(v[u]));
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], ai_dpp<AI_DPP_MIRROR>(v[u]));
    if (n2 > 16) {
        rn_f4 t;
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = __shfl_xor(v[u], 16, 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], t[u]);
    }
    if (n2 > 32) {
        rn_f4 t;
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = __shfl_xor(v[u], 32, 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ai_comb<MAX>(v[u], t[u]);
    }
    return v;
}
// exp(x), x <= 0, through the hardware exp2.  y = fl(x log2 e) alone carries half an ulp of y, a RELATIVE error of |x| 2^-24 in the result --
// 1e-6 for a key 14 below the row maximum; the rounding residual r of the product (exact by FMA, plus the low word of log2 e) is put back to
// first order: 2^(y + r) = 2^y (1 + r ln 2).
__device__ __forceinline__ float ai_exp(float x) {
    const float L2E = 1.44269502f, L2E_LO = 1.92596299e-8f;
    const float y = x * L2E;
    const float r = fmaf(x, L2E_LO, fmaf(x, L2E, -y));
    const float p = __builtin_amdgcn_exp2f(y);
    return fmaf(p, r * 0.693147181f, p);
}
