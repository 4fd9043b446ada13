// AFMLayer (Xiao et al. 2017, arXiv 1708.04617, section 3): FM's pair products pooled by a learned softmax over the pairs -- C ABI 27.
//   p_k = x_i * x_j  (pair k = (i, j), i < j, i-major);   z_k = W^T p_k + b  (A);   e_k = <relu(z_k), h>;
//   a = softmax of e over the P pairs (maximum subtracted);   v = sum_k a_k p_k  (D);   out = <v, p>  or  v.
// `fields` is a DEVICE array of F device pointers; field f of sample b starts at fields[f] + b * xstride (one row stride for all fields).
// fp32 FMA on exact fp32 operands, no float atomics, every reduction in a fixed order.  Neither (P, D) nor (P, A) exists anywhere.
//
// One wave per sample, a workgroup of ONE wave over a contiguous chunk of samples: everything below is wave-private and no barrier is used.
// LDS of a wave, in floats (DS = the row stride of a field, 4 ceil(D / 4) or that plus 4 so that DS / 4 is odd; PP = 4 ceil(P / 4)):
//   forward:   xt (F DS)  st (PP: e, then exp, then a)
//   backward:  xt (F DS)  dxt (F DS)  dt (PP: da, then de)  qt (4 PP: dz of FOUR hidden units for every pair; its first PP floats are st
//              until the attention has been consumed)
// Two lane mappings:
//   lane = pair (k = lane, lane + 64, ..): the Gram phase.  For a block of four hidden units a lane reads x_i and x_j 16 bytes at a time,
//     forms p once and runs 16 FMAs per 4 columns against W rows, which every lane reads at the same address: scalar loads through the constant address space.
//   lane = (field i, column quad q): the mixing phase  M_i = sum_{j != i} s_ij x_j  with s the symmetric F x F matrix of a per-pair value.
//     v = 1/2 sum_i x_i * (a X)_i;  dX_i = dv * (a X)_i + sum_a W[:, a] * (dz_a X)_i;  dW[:, a] = 1/2 sum_i x_i * (dz_a X)_i.
//     Lanes of one quad are lane, lane + DQP, ..; sums over the fields are butterflies of __shfl_xor over those lanes.
// Backward of a sample: scores and da in one walk over the pairs, the softmax and de = a (da - sum a da) (da shifted by the da of the top pair,
// as csrc/autoint.hip does), dxt = dv * (a X), then per block of four hidden units: recompute z, write dz to qt, add (dz X) W^T to dxt.
//
// Weight gradient: the wave adds its samples' contributions, in sample order, into its own slab of the workspace (every element is owned by
// one lane; the first sample stores, the others add); rn_part_reduce (partials.hpp) adds the slabs of the G waves in fp64 in a fixed tree.  A slab is
// [dW (D A) | db (A) | dh (A) | dp (D)] padded to n = 4 ceil((D A + 2 A + D) / 4) floats.
// Workspace (recnow_afm_workspace_bytes): G n floats rounded up to 256 bytes, G = rn_part_groups(B, AFM_DW_ROWS, AFM_MAXG, n) = max(1, min(ceil(B / AFM_DW_ROWS), AFM_MAXG, RN_PART_BYTES / (4 n))).
#include "common.hpp"
#include "wave_softmax.hpp"                     // ai_wave_red4, ai_exp
#include "partials.hpp"
#include <math.h>

#define AFM_MAX_F 64
#define AFM_MAX_D 64
#define AFM_MAX_A 64
#define AFM_LDS_BYTES (160 * 1024)
#define AFM_MAXG 4096                           // waves (and weight-gradient partials) of a launch at the most
#define AFM_DW_ROWS 4                           // samples of one wave at the least

struct AfmDesc {
    int F, D, A, P, PP, DQ, DS, DQP, qsh, proj, nS;
    int64_t B, xs, dxs, rows;                   // xs / dxs: row strides of the fields / their gradients; rows: samples per wave
};

// rn_ld4 for an address that is the same in every lane of the wave and whose memory no kernel of the launch writes (weights, the upstream
// gradient): read through the constant address space, the load goes to the scalar unit and its cache and costs no vector or LDS cycle
typedef const float __attribute__((address_space(4)))* afm_ccf;
typedef const rn_f4 __attribute__((address_space(4)))* afm_ccf4;
__device__ __forceinline__ rn_f4 afm_ldu4(const float* p, int n, bool vec) {
    if (vec) return *reinterpret_cast<afm_ccf4>((afm_ccf)p);
    rn_f4 v = {0.f, 0.f, 0.f, 0.f};
    afm_ccf g = (afm_ccf)p;
    if (n > 0) v.x = g[0];
    if (n > 1) v.y = g[1];
    if (n > 2) v.z = g[2];
    if (n > 3) v.w = g[3];
    return v;
}
__device__ __forceinline__ float afm_red_sum(float v) { return ai_wave_red4<false>(rn_f4{v, 0.f, 0.f, 0.f}, 64).x; }
__device__ __forceinline__ float afm_red_max(float v) { return ai_wave_red4<true>(rn_f4{v, v, v, v}, 64).x; }
// sum over the lanes lane, lane ^ DQP, lane ^ 2 DQP, ..: the fields of one column quad
__device__ __forceinline__ rn_f4 afm_red_fields(rn_f4 v, int DQP) {
    for (int off = DQP; off < 64; off <<= 1) {
        rn_f4 t;
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = __shfl_xor(v[u], off, 64);
        v += t;
    }
    return v;
}
// index of pair (i, i + 1): the pairs (i, .) are consecutive from there
__device__ __forceinline__ int afm_start(int i, int F) { return i * (2 * F - i - 1) / 2; }
__device__ __forceinline__ void afm_pair(int k, int F, int& i, int& j) {
    const float t = (float)(2 * F - 1);
    int ii = (int)((t - sqrtf(t * t - 8.f * (float)k)) * 0.5f);         // exact up to one either way; t^2 - 8 k >= 9
    ii = max(0, min(ii, F - 2));
    if (ii < F - 2 && afm_start(ii + 1, F) <= k) ++ii;
    if (afm_start(ii, F) > k) --ii;
    i = ii;
    j = k - afm_start(ii, F) + ii + 1;
}
struct AfmW {
    const float *W, *b, *h, *p;
    bool vw, vb, vh, vp;
};
// z[a0 .. a0 + 3] of one pair: b + sum_c W[c][a] x_i[c] x_j[c]; hidden units >= A come out 0
template <bool FAST>
__device__ __forceinline__ rn_f4 afm_z4(const AfmDesc& c, const AfmW& w, const rn_f4* xi, const rn_f4* xj, int a0) {
    rn_f4 z = afm_ldu4(w.b + a0, c.A - a0, w.vb);
    for (int cq = 0; cq < c.DQ; ++cq) {
        const rn_f4 p = xi[cq] * xj[cq];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cc = 4 * cq + u;
            const rn_f4 wr = FAST || cc < c.D ? afm_ldu4(w.W + cc * c.A + a0, c.A - a0, w.vw) : rn_f4{0.f, 0.f, 0.f, 0.f};
            z += p[u] * wr;
        }
    }
    return z;
}
// dv[4 q .. 4 q + 3]: g * p with the projection, else the row of dout.  UNI: q is the same in every lane
template <bool UNI>
__device__ __forceinline__ rn_f4 afm_dv4(const AfmDesc& c, const AfmW& w, const float* dout, int64_t b, float gb, int q, bool vg) {
    const float* src = c.proj ? w.p + 4 * q : dout + b * c.D + 4 * q;
    const bool vec = c.proj ? w.vp : vg;
    const rn_f4 v = UNI ? afm_ldu4(src, c.D - 4 * q, vec) : rn_ld4(src, c.D - 4 * q, vec);
    return c.proj ? gb * v : v;
}
// the fields of sample b -> xt
__device__ __forceinline__ void afm_load(const AfmDesc& c, const float* const* fields, float* xt, int64_t b, int lane) {
    for (int e = lane; e < c.F * c.DQ; e += 64) {
        const int f = e / c.DQ, q = e - f * c.DQ;
        const float* xf = fields[f];
        *reinterpret_cast<rn_f4*>(xt + f * c.DS + 4 * q) = rn_ld4(xf + b * c.xs + 4 * q, c.D - 4 * q, rn_vec4_ok(xf, c.D, c.xs));
    }
    RN_LDS_WAVE_SYNC();
}
// st <- the attention a of the sample in xt; BWD: dt <- de = a (da - sum a da), da_k = <dv, p_k>
template <bool BWD, bool FAST>
__device__ __forceinline__ void afm_attention(const AfmDesc& c, const AfmW& w, const float* xt, float* st, float* dt, const float* dout, int64_t b,
                                              float gb, bool vg, int lane) {
    float m = -INFINITY;
    for (int k = lane; k < c.P; k += 64) {
        int i, j;
        afm_pair(k, c.F, i, j);
        const rn_f4* xi = reinterpret_cast<const rn_f4*>(xt + i * c.DS);
        const rn_f4* xj = reinterpret_cast<const rn_f4*>(xt + j * c.DS);
        if (BWD) {
            float da = 0.f;
            for (int cq = 0; cq < c.DQ; ++cq) da += rn_dot4(afm_dv4<true>(c, w, dout, b, gb, cq, vg), xi[cq] * xj[cq]);
            dt[k] = da;
        }
        float e = 0.f;
        for (int a0 = 0; a0 < c.A; a0 += 4) {
            rn_f4 z = afm_z4<FAST>(c, w, xi, xj, a0);
#pragma unroll
            for (int u = 0; u < 4; ++u) z[u] = z[u] > 0.f ? z[u] : 0.f;
            e += rn_dot4(z, afm_ldu4(w.h + a0, c.A - a0, w.vh));
        }
        st[k] = e;
        m = e > m ? e : m;
    }
    m = afm_red_max(m);
    // de = a (da - sum a da) does not change when da is shifted; shifted by the da of the top pair, a near one-hot sample (a_top ~ 1,
    // da_top - sum a da cancelling) keeps its small de_top to full precision
    float l = 0.f, sh = -INFINITY;
    for (int k = lane; k < c.P; k += 64) {
        const float e = st[k], ex = ai_exp(e - m);
        st[k] = ex;
        l += ex;
        if (BWD && e == m) sh = dt[k] > sh ? dt[k] : sh;
    }
    l = afm_red_sum(l);
    if (BWD) sh = afm_red_max(sh);
    float s2 = 0.f;
    for (int k = lane; k < c.P; k += 64) {
        const float a = st[k] / l;
        st[k] = a;
        if (BWD) {
            const float d = dt[k] - sh;
            dt[k] = d;
            s2 += a * d;
        }
    }
    if (BWD) {
        s2 = afm_red_sum(s2);
        for (int k = lane; k < c.P; k += 64) dt[k] = st[k] * (dt[k] - s2);
    }
    RN_LDS_WAVE_SYNC();
}
// sum over j != i of s[pair(i, j)] * x_j[4 q .. 4 q + 3]
__device__ __forceinline__ rn_f4 afm_mix1(const AfmDesc& c, const float* xt, const float* s, int i, int q) {
    const float* xq = xt + 4 * q;
    rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = i - 1;                                                      // pair (0, i); pair (j + 1, i) is F - j - 2 further on
    for (int j = 0; j < i; ++j) {
        acc += s[k] * *reinterpret_cast<const rn_f4*>(xq + j * c.DS);
        k += c.F - j - 2;
    }
    k = afm_start(i, c.F);
    for (int j = i + 1; j < c.F; ++j, ++k) acc += s[k] * *reinterpret_cast<const rn_f4*>(xq + j * c.DS);
    return acc;
}
// the same with four values per pair: r[u] = sum over j != i of q4[pair(i, j)][u] * x_j[4 q .. 4 q + 3]
__device__ __forceinline__ void afm_mix4(const AfmDesc& c, const float* xt, const float* qt, int i, int q, rn_f4 (&r)[4]) {
    const float* xq = xt + 4 * q;
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = rn_f4{0.f, 0.f, 0.f, 0.f};
    int k = i - 1;
    for (int j = 0; j < i; ++j) {
        const rn_f4 s = *reinterpret_cast<const rn_f4*>(qt + 4 * k), x = *reinterpret_cast<const rn_f4*>(xq + j * c.DS);
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] += s[u] * x;
        k += c.F - j - 2;
    }
    k = afm_start(i, c.F);
    for (int j = i + 1; j < c.F; ++j, ++k) {
        const rn_f4 s = *reinterpret_cast<const rn_f4*>(qt + 4 * k), x = *reinterpret_cast<const rn_f4*>(xq + j * c.DS);
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] += s[u] * x;
    }
}
template <bool FAST>
__device__ __forceinline__ AfmW afm_weights(const AfmDesc& c, const float* W, const float* bias, const float* h, const float* p) {
    AfmW w;
    w.W = W; w.b = bias; w.h = h; w.p = p;
    w.vw = FAST || rn_vec4_ok(W, c.A, 0); w.vb = FAST || rn_vec4_ok(bias, c.A, 0); w.vh = FAST || rn_vec4_ok(h, c.A, 0); w.vp = c.proj && rn_vec4_ok(p, c.D, 0);
    return w;
}

// FAST (chosen by the host): D and A are multiples of 4 and W, b, h are 16-byte aligned, so the Gram loop has no guard and its four row loads
// issue back to back; the arithmetic and its order are the same either way.
template <bool FAST>
__global__ void __launch_bounds__(64)
k_afm_fwd(const float* const* __restrict__ fields, float* __restrict__ out, const float* __restrict__ W, const float* __restrict__ bias,
          const float* __restrict__ h, const float* __restrict__ p, AfmDesc c) {
    extern __shared__ __attribute__((aligned(16))) float afm_lds[];
    const int lane = threadIdx.x, slot = lane >> c.qsh, q = lane & (c.DQP - 1), ipw = 64 >> c.qsh;
    float* xt = afm_lds;
    float* st = xt + c.F * c.DS;
    const AfmW w = afm_weights<FAST>(c, W, bias, h, p);
    const bool vo = rn_vec4_ok(out, c.D, 0);
    const int64_t r0 = (int64_t)blockIdx.x * c.rows, r1 = min(c.B, r0 + c.rows);
    for (int64_t b = r0; b < r1; ++b) {
        afm_load(c, fields, xt, b, lane);
        afm_attention<false, FAST>(c, w, xt, st, nullptr, nullptr, b, 0.f, false, lane);
        rn_f4 v = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < c.F; i0 += ipw) {
            const int i = i0 + slot;
            if (i < c.F && q < c.DQ) v += *reinterpret_cast<const rn_f4*>(xt + i * c.DS + 4 * q) * afm_mix1(c, xt, st, i, q);
        }
        v = 0.5f * afm_red_fields(v, c.DQP);
        const bool owner = slot == 0 && q < c.DQ;
        if (c.proj) {
            const float o = afm_red_sum(owner ? rn_dot4(v, rn_ld4(p + 4 * q, c.D - 4 * q, w.vp)) : 0.f);
            if (lane == 0) out[b] = o;
        } else if (owner) {
            rn_st4(out + b * c.D + 4 * q, v, c.D - 4 * q, vo);
        }
        RN_LDS_WAVE_SYNC();                                     // tiles read before the next sample overwrites them
    }
}

// part: this launch's partials, slab g = blockIdx.x of c.nS floats (NULL: no weight gradient).
template <bool FAST>
__global__ void __launch_bounds__(64)
k_afm_bwd(const float* const* __restrict__ fields, float* const* __restrict__ dfields, const float* __restrict__ dout, float* __restrict__ part,
          const float* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ h, const float* __restrict__ p, AfmDesc c) {
    extern __shared__ __attribute__((aligned(16))) float afm_lds[];
    const int lane = threadIdx.x, slot = lane >> c.qsh, q = lane & (c.DQP - 1), ipw = 64 >> c.qsh;
    const int F = c.F, D = c.D, A = c.A, DS = c.DS;
    float* xt = afm_lds;
    float* dxt = xt + F * DS;
    float* dt = dxt + F * DS;
    float* qt = dt + c.PP;
    float* st = qt;                                         // dead before qt is first written
    const AfmW w = afm_weights<FAST>(c, W, bias, h, p);
    const bool vg = !c.proj && rn_vec4_ok(dout, D, 0);
    const bool owner = slot == 0 && q < c.DQ;
    float* slab = part ? part + (int64_t)blockIdx.x * c.nS : nullptr;
    float* sb = slab + D * A;                               // db, then dh, then dp
    const bool vsa = (A & 3) == 0, vsp = vsa && (D & 3) == 0;
    const rn_f4 zero = {0.f, 0.f, 0.f, 0.f};
    const int64_t r0 = (int64_t)blockIdx.x * c.rows, r1 = min(c.B, r0 + c.rows);
    for (int64_t b = r0; b < r1; ++b) {
        const bool first = b == r0;
        const float gb = c.proj ? dout[b] : 0.f;
        afm_load(c, fields, xt, b, lane);
        afm_attention<true, FAST>(c, w, xt, st, dt, dout, b, gb, vg, lane);
        // dxt = dv * (a X);  v for dp
        rn_f4 v = zero;
        for (int i0 = 0; i0 < F; i0 += ipw) {
            const int i = i0 + slot;
            if (i < F && q < c.DQ) {
                const rn_f4 mx = afm_mix1(c, xt, st, i, q);
                v += *reinterpret_cast<const rn_f4*>(xt + i * DS + 4 * q) * mx;
                *reinterpret_cast<rn_f4*>(dxt + i * DS + 4 * q) = afm_dv4<false>(c, w, dout, b, gb, q, vg) * mx;
            }
        }
        if (slab && c.proj) {
            v = 0.5f * afm_red_fields(v, c.DQP);
            if (owner) {
                float* s = sb + 2 * A + 4 * q;
                rn_st4(s, (first ? zero : rn_ld4(s, D - 4 * q, vsp)) + gb * v, D - 4 * q, vsp);
            }
        }
        RN_LDS_WAVE_SYNC();                                     // st consumed: qt may be written
        for (int a0 = 0; a0 < A; a0 += 4) {
            const rn_f4 h4 = afm_ldu4(h + a0, A - a0, w.vh);
            rn_f4 dh4 = zero, db4 = zero;
            for (int k = lane; k < c.P; k += 64) {
                int i, j;
                afm_pair(k, F, i, j);
                const rn_f4 z = afm_z4<FAST>(c, w, reinterpret_cast<const rn_f4*>(xt + i * DS), reinterpret_cast<const rn_f4*>(xt + j * DS), a0);
                const float de = dt[k];
                rn_f4 dz;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    dh4[u] += z[u] > 0.f ? de * z[u] : 0.f;
                    dz[u] = z[u] > 0.f ? de * h4[u] : 0.f;
                }
                db4 += dz;
                *reinterpret_cast<rn_f4*>(qt + 4 * k) = dz;
            }
            if (slab) {
                dh4 = ai_wave_red4<false>(dh4, 64);
                db4 = ai_wave_red4<false>(db4, 64);
                if (lane == 0) {
                    float* s = sb + a0;
                    rn_st4(s, (first ? zero : rn_ld4(s, A - a0, vsa)) + db4, A - a0, vsa);
                    s += A;
                    rn_st4(s, (first ? zero : rn_ld4(s, A - a0, vsa)) + dh4, A - a0, vsa);
                }
            }
            RN_LDS_WAVE_SYNC();
            // dxt_i += W[:, a] * (dz_a X)_i;  dW[:, a] += 1/2 x_i * (dz_a X)_i
            rn_f4 wr[4], dw[4];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                wr[cc] = q < c.DQ && 4 * q + cc < D ? rn_ld4(W + (4 * q + cc) * A + a0, A - a0, w.vw) : zero;
                dw[cc] = zero;
            }
            for (int i0 = 0; i0 < F; i0 += ipw) {
                const int i = i0 + slot;
                if (i < F && q < c.DQ) {
                    rn_f4 r[4];
                    afm_mix4(c, xt, qt, i, q, r);
                    const rn_f4 xi = *reinterpret_cast<const rn_f4*>(xt + i * DS + 4 * q);
                    rn_f4 dx = *reinterpret_cast<const rn_f4*>(dxt + i * DS + 4 * q);
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            dx[cc] = fmaf(wr[cc][u], r[u][cc], dx[cc]);
                            dw[cc][u] = fmaf(xi[cc], r[u][cc], dw[cc][u]);
                        }
                    }
                    *reinterpret_cast<rn_f4*>(dxt + i * DS + 4 * q) = dx;
                }
            }
            if (slab) {
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    dw[cc] = 0.5f * afm_red_fields(dw[cc], c.DQP);
                    if (owner && 4 * q + cc < D) {
                        float* s = slab + (4 * q + cc) * A + a0;
                        rn_st4(s, (first ? zero : rn_ld4(s, A - a0, vsa)) + dw[cc], A - a0, vsa);
                    }
                }
            }
            RN_LDS_WAVE_SYNC();                                 // qt read before the next block overwrites it
        }
        for (int e = lane; e < F * c.DQ; e += 64) {
            const int f = e / c.DQ, qq = e - f * c.DQ;
            float* df = dfields[f];
            rn_st4(df + b * c.dxs + 4 * qq, *reinterpret_cast<const rn_f4*>(dxt + f * DS + 4 * qq), D - 4 * qq, rn_vec4_ok(df, D, c.dxs));
        }
        RN_LDS_WAVE_SYNC();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
static inline bool afm_shape_ok(int F, int D, int A) {
    return F >= 2 && F <= AFM_MAX_F && D >= 1 && D <= AFM_MAX_D && A >= 1 && A <= AFM_MAX_A;
}
static inline bool afm_fast(int D, int A, const float* W, const float* b, const float* h) {
    return ((D | A) & 3) == 0 && ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(h)) & 15) == 0;
}
static inline int afm_slab(int D, int A) { return (D * A + 2 * A + D + 3) & ~3; }
static int afm_groups(int64_t B, int D, int A) { return rn_part_groups(B, AFM_DW_ROWS, AFM_MAXG, afm_slab(D, A)); }
static AfmDesc afm_desc(int F, int64_t B, int D, int A, int proj, int bwd, int64_t xs, int64_t dxs, size_t* lds, int* grid) {
    AfmDesc c;
    c.F = F; c.D = D; c.A = A; c.P = F * (F - 1) / 2; c.PP = (c.P + 3) & ~3;
    c.DQ = (D + 3) / 4;
    c.DS = 4 * (c.DQ | 1);                                  // DS / 4 odd: rows of 16-byte reads start on different bank groups
    c.DQP = 1; c.qsh = 0;
    while (c.DQP < c.DQ) { c.DQP <<= 1; ++c.qsh; }
    c.proj = proj; c.nS = afm_slab(D, A);
    c.B = B; c.xs = xs; c.dxs = dxs;
    *lds = sizeof(float) * (bwd ? (size_t)2 * F * c.DS + 5 * c.PP : (size_t)F * c.DS + c.PP);     // at most 75 136 bytes
    int G = afm_groups(B, D, A);
    if (!bwd) {                                             // no partials: twice the waves hide the latency of the row loads
        const int64_t g = (B + AFM_DW_ROWS - 1) / AFM_DW_ROWS;
        G = g > 2 * AFM_MAXG ? 2 * AFM_MAXG : (int)g;
    }
    c.rows = (B + G - 1) / G;
    *grid = (int)((B + c.rows - 1) / c.rows);               // <= G (<= afm_groups in the backward), every wave has a sample
    return c;
}
extern "C" int recnow_afm_supported(int F, int D, int A) { return afm_shape_ok(F, D, A) ? 1 : 0; }

extern "C" int recnow_afm_route(int F, int D, int A, int bwd) {
    (void)bwd;
    return afm_shape_ok(F, D, A) ? 0 : RECNOW_EUNSUPPORTED;
}

extern "C" size_t recnow_afm_workspace_bytes(int64_t B, int F, int D, int A) {
    if (!afm_shape_ok(F, D, A) || B <= 0) return 0;
    return rn_align((size_t)afm_groups(B, D, A) * afm_slab(D, A) * sizeof(float));
}

extern "C" int recnow_afm_fwd(const float* const* fields, int64_t xstride, int F, int64_t B, int D, int A, const float* W, const float* b,
                              const float* h, const float* p, float* out, void* stream) {
    if (F < 1 || B < 0 || D < 1 || A < 1) return RECNOW_EINVAL;
    if (!afm_shape_ok(F, D, A)) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!fields || !W || !b || !h || !out || xstride < D) return RECNOW_EINVAL;
    int grid;
    size_t lds;
    const AfmDesc c = afm_desc(F, B, D, A, p ? 1 : 0, 0, xstride, 0, &lds, &grid);
    if (afm_fast(D, A, W, b, h)) hipLaunchKernelGGL(k_afm_fwd<true>, grid, 64, lds, (hipStream_t)stream, fields, out, W, b, h, p, c);
    else hipLaunchKernelGGL(k_afm_fwd<false>, grid, 64, lds, (hipStream_t)stream, fields, out, W, b, h, p, c);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_afm_bwd(const float* const* fields, int64_t xstride, float* const* dfields, int64_t dxstride, int F, int64_t B, int D,
                              int A, const float* W, const float* b, const float* h, const float* p, const float* dout, float* dW, float* db,
                              float* dh, float* dp, void* ws, size_t ws_bytes, void* stream) {
    if (F < 1 || B < 0 || D < 1 || A < 1) return RECNOW_EINVAL;
    if (!afm_shape_ok(F, D, A)) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!fields || !dfields || !W || !b || !h || !dout || xstride < D || dxstride < D) return RECNOW_EINVAL;
    const bool want_dw = dW || db || dh || dp;
    if (want_dw && (!dW || !db || !dh || (p && !dp))) return RECNOW_EINVAL;                 // all of them or none
    float* part = nullptr;
    if (want_dw) {
        if (!ws || ws_bytes < recnow_afm_workspace_bytes(B, F, D, A)) return RECNOW_EWORKSPACE;
        part = (float*)ws;
    }
    int grid;
    size_t lds;
    const AfmDesc c = afm_desc(F, B, D, A, p ? 1 : 0, 1, xstride, dxstride, &lds, &grid);
    hipStream_t st = (hipStream_t)stream;
    const bool fast = afm_fast(D, A, W, b, h);
    // F = D = 64: two F x DS tiles and five PP rows are 75 136 bytes
    if (lds > 64 * 1024) RN_HIP(rn_lds_grant(fast ? (const void*)k_afm_bwd<true> : (const void*)k_afm_bwd<false>, AFM_LDS_BYTES));
    if (fast) hipLaunchKernelGGL(k_afm_bwd<true>, grid, 64, lds, st, fields, dfields, dout, part, W, b, h, p, c);
    else hipLaunchKernelGGL(k_afm_bwd<false>, grid, 64, lds, st, fields, dfields, dout, part, W, b, h, p, c);
    RN_LAUNCH_CHECK();
    if (!part) return RECNOW_OK;
    const int DA = D * A;
    const RnPartDst dst = {{dW, db, dh, dp}, {DA, DA + A, DA + 2 * A, DA + 2 * A + (p ? D : 0)}};
    return rn_part_reduce(part, dst.end[3], 1, grid, c.nS, 0, dst, st);
}
