// attention_by_softmax: masked multi-head softmax target attention of a padded (B, L, D) history against H queries per sample (C ABI 34).
// An addition (the reference has no softmax attention).  K(b) = { l : l < lengths[b] and mask[b][l] != 0 }:
//   s_hl = scale <q[b,h], x[b,l]>  (l in K(b));   a_hl = exp(s_hl - m_h) / sum_h;   out[b,h] = sum_l a_hl x[b,l]
//   stat[b,h] = (m_h, log2 of the sum rescaled by m_h);   lse = m_h + ln 2 * stat[b,h][1]
// backward (scores recomputed from x, q and stat), dc = d out, g_hl = <dc_h, x_l>, gbar_h = <dc_h, out_h>:
//   ds_hl = a_hl (g_hl - gbar_h);   dx_l = sum_h (a_hl dc_h + scale ds_hl q_h);   dq_h = scale sum_l ds_hl x_l
// Pure streams: x is read once per direction, dx written once; everything per (b, h) lives in registers.  No LDS, no atomics, every row
// written once by one lane group in a fixed order.  Positions outside K(b) are kept out by selects (never by arithmetic): their loads are
// replaced by zeros before any product is formed, so NaN / inf there do not reach a bit of anything, and positions at or beyond the
// length are not even read.
//
// Two routes (as_route, queryable through recnow_attention_softmax_route):
//   vector   D = 4 CPL, CPL in {1, 2, 4, 8, 16}, every base 16-byte aligned: k_as_v4_fwd / _bwd<CPL, HB>.  AS_LANES = 16 lanes serve one
//            sample (AS_SPW = 4 samples per wave) and walk its L * CPL float4 pieces, piece k = lane + 16 i <-> position k / CPL, columns
//            4 (k % CPL) .. + 3; k % CPL is the same for every piece of a lane, so the lane keeps columns 4c .. 4c + 3 of all H queries.
//            The lanes of a sample hold DIFFERENT positions at the same time: each lane carries the (m, s, acc) of its own subset of
//            positions (AS_V4 pieces per loop trip: one maximum and one rescale per trip) and the 16 / CPL subsets are merged once at the end.
//   guarded  every other D <= 256, and misaligned bases: k_as_fwd / _bwd<GS, HB>, GS = 16 / 32 / 64 lanes per sample for D <= 16 / <= 32 /
//            <= 256, lane <-> column (4 chunks of 64 for GS = 64), 4-byte accesses, one position at a time: the classic online softmax,
//            one exponential per position and head.  Its summation order differs from the vector route's (columns, then positions one by
//            one): the two routes agree within rounding, not bit for bit.
// HB in {1, 2, 4, 8} is H rounded up to a power of two: the head loops are unrolled HB times and guarded by h < H (wave-uniform).
#include "common.hpp"
#include "wave_softmax.hpp"
#include <math.h>

#define AS_LANES 16     // lanes per sample on the vector route
#define AS_SPW 4        // samples per wave on the vector route
#define AS_V4 4         // float4 pieces per lane and loop trip on the vector route
#define AS_NCH 4        // 64-wide column chunks a lane keeps on the guarded route with GS = 64
#define AS_MAX_D 256
#define AS_MAX_H 8
#define AS_NEG_INF (-__builtin_inff())

template <int GS>
__device__ __forceinline__ float as_group_sum(float v) {
#pragma unroll
    for (int o = GS / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int as_wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int as_len(const int32_t* lengths, int64_t b, bool ok, int L) {
    if (!ok) return 0;
    if (!lengths) return L;
    const int n = lengths[b];
    return n < 0 ? 0 : (n > L ? L : n);
}
// exp(x - m) for a running maximum m that may still be -inf (nothing seen yet: the weight of what was accumulated so far, zeros, is 0)
__device__ __forceinline__ float as_rescale(float m, float mn) { return m > AS_NEG_INF ? ai_exp(m - mn) : 0.f; }
__device__ __forceinline__ float as_dot4(rn_f4 a, rn_f4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// ---------------------------------------------------------------------------------------------------------------------
// vector route
// ---------------------------------------------------------------------------------------------------------------------
template <int CPL, int HB>
__global__ void __launch_bounds__(256)
k_as_v4_fwd(const float* __restrict__ user, const float* __restrict__ query, const int32_t* __restrict__ lengths,
            const uint8_t* __restrict__ mask, int64_t B, int L, int H, float scale, float* __restrict__ out, float* __restrict__ stat) {
    constexpr int D = 4 * CPL;
    const int lane = threadIdx.x & 63, gl = lane & (AS_LANES - 1), gr = lane / AS_LANES;
    const int c = gl % CPL;
    const int64_t nrg = (B + AS_SPW - 1) / AS_SPW;
    const rn_f4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t rg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); rg < nrg; rg += (int64_t)gridDim.x * 4) {
        const int64_t b = rg * AS_SPW + gr;
        const bool ok = b < B;
        const int64_t bb = ok ? b : 0;
        const rn_f4* u4 = reinterpret_cast<const rn_f4*>(user + bb * (int64_t)L * D);
        const uint8_t* mk = mask ? mask + bb * (int64_t)L : nullptr;
        const int nvl = as_len(lengths, b, ok, L) * CPL;        // pieces inside the length; the rest of the row is not read
        const int nvw = as_wave_max_int(nvl);                   // every lane of the wave runs the same trip count
        rn_f4 q[HB], acc[HB];
        float m[HB], s[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            q[h] = (ok && h < H) ? *reinterpret_cast<const rn_f4*>(query + (bb * H + h) * D + 4 * c) : zero;
            acc[h] = zero;
            m[h] = AS_NEG_INF;
            s[h] = 0.f;
        }
        for (int k0 = 0; k0 < nvw; k0 += AS_LANES * AS_V4) {
            rn_f4 uv[AS_V4];
            bool key[AS_V4];
#pragma unroll
            for (int i = 0; i < AS_V4; ++i) {
                const int k = k0 + AS_LANES * i + gl;
                const bool in = k < nvl;
                const rn_f4 v = in ? RN_LD_STREAM(u4 + k) : zero;
                key[i] = in && (!mk || mk[k / CPL] != 0);
                uv[i] = key[i] ? v : zero;                      // the select that keeps a masked position out
            }
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
                    float sc[AS_V4], mt = m[h];
#pragma unroll
                    for (int i = 0; i < AS_V4; ++i) {
                        float p = as_dot4(uv[i], q[h]);
#pragma unroll
                        for (int o = CPL / 2; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
                        sc[i] = key[i] ? scale * p : AS_NEG_INF;
                        mt = sc[i] > mt ? sc[i] : mt;
                    }
                    const float r = as_rescale(m[h], mt);
                    float es = 0.f;
                    rn_f4 ea = zero;
#pragma unroll
                    for (int i = 0; i < AS_V4; ++i) {
                        const float e = key[i] ? ai_exp(sc[i] - mt) : 0.f;
                        es += e;
                        ea += uv[i] * e;
                    }
                    s[h] = s[h] * r + es;
                    acc[h] = acc[h] * r + ea;
                    m[h] = mt;
                }
            }
        }
        // merge the 16 / CPL subsets (lanes c, c + CPL, ..): both partners of an exchange form the SAME expression (a = the lower lane's
        // triple, b = the upper lane's), so all lanes end with the same bits
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            if (h < H) {
#pragma unroll
                for (int o = CPL; o < AS_LANES; o <<= 1) {
                    const bool lo = (gl & o) == 0;
                    const float mo = __shfl_xor(m[h], o, 64), so = __shfl_xor(s[h], o, 64);
                    rn_f4 ao;
                    ao.x = __shfl_xor(acc[h].x, o, 64); ao.y = __shfl_xor(acc[h].y, o, 64);
                    ao.z = __shfl_xor(acc[h].z, o, 64); ao.w = __shfl_xor(acc[h].w, o, 64);
                    const float ma = lo ? m[h] : mo, mb = lo ? mo : m[h];
                    const float sa = lo ? s[h] : so, sb = lo ? so : s[h];
                    const rn_f4 aa = lo ? acc[h] : ao, ab = lo ? ao : acc[h];
                    const float mn = mb > ma ? mb : ma;
                    const float ra = as_rescale(ma, mn), rb = as_rescale(mb, mn);
                    s[h] = sa * ra + sb * rb;
                    acc[h] = aa * ra + ab * rb;
                    m[h] = mn;
                }
                const bool any = s[h] > 0.f || s[h] != s[h];    // a NaN inside the keys stays visible in its own sample
                if (ok && gl < CPL) *reinterpret_cast<rn_f4*>(out + (b * H + h) * D + 4 * c) = any ? acc[h] / s[h] : zero;
                if (ok && gl == 0) {
                    stat[(b * H + h) * 2] = m[h];
                    stat[(b * H + h) * 2 + 1] = any ? log2f(s[h]) : AS_NEG_INF;
                }
            }
        }
    }
}

template <int CPL, int HB>
__global__ void __launch_bounds__(256)
k_as_v4_bwd(const float* __restrict__ user, const float* __restrict__ query, const int32_t* __restrict__ lengths,
            const uint8_t* __restrict__ mask, const float* __restrict__ out, const float* __restrict__ stat,
            const float* __restrict__ dout, int64_t B, int L, int H, float scale, float* __restrict__ duser, float* __restrict__ dquery) {
    constexpr int D = 4 * CPL;
    constexpr int BV = HB == 8 ? 2 : AS_V4;                    // pieces per lane and trip: two at 8 heads, whose q, dc and dq fill the registers
    const int lane = threadIdx.x & 63, gl = lane & (AS_LANES - 1), gr = lane / AS_LANES;
    const int c = gl % CPL;
    const int64_t nrg = (B + AS_SPW - 1) / AS_SPW;
    const int nv = L * CPL;
    const rn_f4 zero = {0.f, 0.f, 0.f, 0.f};
    const bool want_dx = duser != nullptr, want_dq = dquery != nullptr;
    for (int64_t rg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); rg < nrg; rg += (int64_t)gridDim.x * 4) {
        const int64_t b = rg * AS_SPW + gr;
        const bool ok = b < B;
        const int64_t bb = ok ? b : 0;
        const rn_f4* u4 = reinterpret_cast<const rn_f4*>(user + bb * (int64_t)L * D);
        rn_f4* du4 = want_dx ? reinterpret_cast<rn_f4*>(duser + bb * (int64_t)L * D) : nullptr;
        const uint8_t* mk = mask ? mask + bb * (int64_t)L : nullptr;
        const int nvl = as_len(lengths, b, ok, L) * CPL;
        const int nvw = want_dx ? nv : as_wave_max_int(nvl);    // dx rows beyond the length are written (zeros), never read
        rn_f4 q[HB], dc[HB], dq[HB];
        float m[HB], invs[HB], gbar[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            const bool on = ok && h < H;
            const int64_t row = (bb * H + (on ? h : 0)) * D + 4 * c;
            q[h] = on ? *reinterpret_cast<const rn_f4*>(query + row) : zero;
            dc[h] = on ? *reinterpret_cast<const rn_f4*>(dout + row) : zero;
            const rn_f4 o4 = on ? *reinterpret_cast<const rn_f4*>(out + row) : zero;
            float g = as_dot4(dc[h], o4);
#pragma unroll
            for (int o = CPL / 2; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
            gbar[h] = g;
            m[h] = on ? stat[(bb * H + h) * 2] : 0.f;
            invs[h] = on ? exp2f(-stat[(bb * H + h) * 2 + 1]) : 0.f;
            dq[h] = zero;
        }
        for (int k0 = 0; k0 < nvw; k0 += AS_LANES * BV) {
            rn_f4 uv[BV];
            bool key[BV];
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int k = k0 + AS_LANES * i + gl;
                const bool in = k < nvl;
                const rn_f4 v = in ? RN_LD_STREAM(u4 + k) : zero;
                key[i] = in && (!mk || mk[k / CPL] != 0);
                uv[i] = key[i] ? v : zero;
            }
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int k = k0 + AS_LANES * i + gl;
                rn_f4 dx = zero;
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    if (h < H) {
                        float p = as_dot4(uv[i], q[h]), g = as_dot4(uv[i], dc[h]);
#pragma unroll
                        for (int o = CPL / 2; o > 0; o >>= 1) {
                            p += __shfl_xor(p, o, 64);
                            g += __shfl_xor(g, o, 64);
                        }
                        const float a = key[i] ? ai_exp(scale * p - m[h]) * invs[h] : 0.f;
                        const float ds = key[i] ? a * (g - gbar[h]) : 0.f;
                        if (want_dx) dx += dc[h] * a + q[h] * (scale * ds);
                        if (want_dq) dq[h] += uv[i] * ds;
                    }
                }
                if (want_dx && ok && k < nv) RN_ST_STREAM(du4 + k, key[i] ? dx : zero);
            }
        }
        if (want_dq) {
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
#pragma unroll
                    for (int o = CPL; o < AS_LANES; o <<= 1) {
                        dq[h].x += __shfl_xor(dq[h].x, o, 64); dq[h].y += __shfl_xor(dq[h].y, o, 64);
                        dq[h].z += __shfl_xor(dq[h].z, o, 64); dq[h].w += __shfl_xor(dq[h].w, o, 64);
                    }
                    if (ok && gl < CPL) *reinterpret_cast<rn_f4*>(dquery + (b * H + h) * D + 4 * c) = dq[h] * scale;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// guarded route
// ---------------------------------------------------------------------------------------------------------------------
template <int GS, int HB>
__global__ void __launch_bounds__(256)
k_as_fwd(const float* __restrict__ user, const float* __restrict__ query, const int32_t* __restrict__ lengths,
         const uint8_t* __restrict__ mask, int64_t B, int L, int D, int H, float scale, float* __restrict__ out, float* __restrict__ stat) {
    constexpr int RPW = 64 / GS, NCH = GS == 64 ? AS_NCH : 1;
    const int lane = threadIdx.x & 63, gl = lane % GS, gr = lane / GS;
    const int64_t nrg = (B + RPW - 1) / RPW;
    for (int64_t rg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); rg < nrg; rg += (int64_t)gridDim.x * 4) {
        const int64_t b = rg * RPW + gr;
        const bool ok = b < B;
        const int64_t bb = ok ? b : 0;
        const float* u = user + bb * (int64_t)L * D;
        const uint8_t* mk = mask ? mask + bb * (int64_t)L : nullptr;
        const int len = as_len(lengths, b, ok, L);
        const int lenw = as_wave_max_int(len);
        float q[HB][NCH], acc[HB][NCH], m[HB], s[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int d = j * 64 + gl;
                q[h][j] = (ok && h < H && d < D) ? query[(bb * H + h) * D + d] : 0.f;
                acc[h][j] = 0.f;
            }
            m[h] = AS_NEG_INF;
            s[h] = 0.f;
        }
        for (int l = 0; l < lenw; ++l) {
            const bool key = l < len && (!mk || mk[l] != 0);
            float uv[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int d = j * 64 + gl;
                const float v = (l < len && d < D) ? RN_LD_STREAM(u + (int64_t)l * D + d) : 0.f;
                uv[j] = key ? v : 0.f;
            }
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) p += uv[j] * q[h][j];
                    const float sc = scale * as_group_sum<GS>(p);
                    // one exponential: either the accumulated part is rescaled (the maximum moves) or the new term is
                    const bool up = sc > m[h];
                    const float t = as_rescale(up ? m[h] : sc, up ? sc : m[h]);
                    const float r = key ? (up ? t : 1.f) : 1.f, e = key ? (up ? 1.f : t) : 0.f;
                    s[h] = s[h] * r + e;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) acc[h][j] = acc[h][j] * r + e * uv[j];
                    m[h] = (key && up) ? sc : m[h];
                }
            }
        }
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            if (h < H) {
                const bool any = s[h] > 0.f || s[h] != s[h];
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    const int d = j * 64 + gl;
                    if (ok && d < D) out[(b * H + h) * D + d] = any ? acc[h][j] / s[h] : 0.f;
                }
                if (ok && gl == 0) {
                    stat[(b * H + h) * 2] = m[h];
                    stat[(b * H + h) * 2 + 1] = any ? log2f(s[h]) : AS_NEG_INF;
                }
            }
        }
    }
}

template <int GS, int HB>
__global__ void __launch_bounds__(256)
k_as_bwd(const float* __restrict__ user, const float* __restrict__ query, const int32_t* __restrict__ lengths,
         const uint8_t* __restrict__ mask, const float* __restrict__ out, const float* __restrict__ stat, const float* __restrict__ dout,
         int64_t B, int L, int D, int H, float scale, float* __restrict__ duser, float* __restrict__ dquery) {
    constexpr int RPW = 64 / GS, NCH = GS == 64 ? AS_NCH : 1;
    const int lane = threadIdx.x & 63, gl = lane % GS, gr = lane / GS;
    const int64_t nrg = (B + RPW - 1) / RPW;
    const bool want_dx = duser != nullptr, want_dq = dquery != nullptr;
    for (int64_t rg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); rg < nrg; rg += (int64_t)gridDim.x * 4) {
        const int64_t b = rg * RPW + gr;
        const bool ok = b < B;
        const int64_t bb = ok ? b : 0;
        const float* u = user + bb * (int64_t)L * D;
        float* du = want_dx ? duser + bb * (int64_t)L * D : nullptr;
        const uint8_t* mk = mask ? mask + bb * (int64_t)L : nullptr;
        const int len = as_len(lengths, b, ok, L);
        const int lenw = want_dx ? L : as_wave_max_int(len);
        float q[HB][NCH], dc[HB][NCH], dq[HB][NCH], m[HB], invs[HB], gbar[HB];
#pragma unroll
        for (int h = 0; h < HB; ++h) {
            const bool on = ok && h < H;
            float g = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int d = j * 64 + gl;
                const bool in = on && d < D;
                const int64_t at = (bb * H + (on ? h : 0)) * D + (in ? d : 0);
                q[h][j] = in ? query[at] : 0.f;
                dc[h][j] = in ? dout[at] : 0.f;
                g += dc[h][j] * (in ? out[at] : 0.f);
                dq[h][j] = 0.f;
            }
            gbar[h] = as_group_sum<GS>(g);
            m[h] = on ? stat[(bb * H + h) * 2] : 0.f;
            invs[h] = on ? exp2f(-stat[(bb * H + h) * 2 + 1]) : 0.f;
        }
        for (int l = 0; l < lenw; ++l) {
            const bool key = l < len && (!mk || mk[l] != 0);
            float uv[NCH], dx[NCH];
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int d = j * 64 + gl;
                const float v = (l < len && d < D) ? RN_LD_STREAM(u + (int64_t)l * D + d) : 0.f;
                uv[j] = key ? v : 0.f;
                dx[j] = 0.f;
            }
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
                    float p = 0.f, g = 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        p += uv[j] * q[h][j];
                        g += uv[j] * dc[h][j];
                    }
                    p = as_group_sum<GS>(p);
                    g = as_group_sum<GS>(g);
                    const float a = key ? ai_exp(scale * p - m[h]) * invs[h] : 0.f;
                    const float ds = key ? a * (g - gbar[h]) : 0.f;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        if (want_dx) dx[j] += dc[h][j] * a + q[h][j] * (scale * ds);
                        if (want_dq) dq[h][j] += uv[j] * ds;
                    }
                }
            }
            if (want_dx) {
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    const int d = j * 64 + gl;
                    if (ok && d < D) du[(int64_t)l * D + d] = key ? dx[j] : 0.f;
                }
            }
        }
        if (want_dq) {
#pragma unroll
            for (int h = 0; h < HB; ++h) {
                if (h < H) {
#pragma unroll
                    for (int j = 0; j < NCH; ++j) {
                        const int d = j * 64 + gl;
                        if (ok && d < D) dquery[(b * H + h) * D + d] = dq[h][j] * scale;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: the route choice stated once (the launchers launch what as_route returns, recnow_attention_softmax_route answers the same
// question without a launch).  mis: one bit per tensor that starts OFF a 16-byte boundary (NULL is aligned).
// ---------------------------------------------------------------------------------------------------------------------
#define AS_MIS_USER 1
#define AS_MIS_QUERY 2
#define AS_MIS_OUT 4
#define AS_MIS_DOUT 8       /* backward */
#define AS_MIS_DUSER 16     /* backward */
#define AS_MIS_DQUERY 32    /* backward */
struct AsRoute {
    int cpl;    // > 0: k_as_v4_fwd / _bwd<cpl, hb>
    int gs;     // cpl == 0: k_as_fwd / _bwd<gs, hb>
    int hb;
};
static AsRoute as_route(int D, int H, int mis) {
    AsRoute r = {0, D <= 16 ? 16 : D <= 32 ? 32 : 64, H <= 1 ? 1 : H <= 2 ? 2 : H <= 4 ? 4 : 8};
    const int cpl = D / 4;
    if (D % 4 == 0 && !mis && (cpl == 1 || cpl == 2 || cpl == 4 || cpl == 8 || cpl == 16)) r.cpl = cpl;
    return r;
}
static inline int as_mis(const void* user, const void* query, const void* out, const void* dout, const void* duser, const void* dquery) {
    auto off = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    return (off(user) ? AS_MIS_USER : 0) | (off(query) ? AS_MIS_QUERY : 0) | (off(out) ? AS_MIS_OUT : 0) | (off(dout) ? AS_MIS_DOUT : 0) |
           (off(duser) ? AS_MIS_DUSER : 0) | (off(dquery) ? AS_MIS_DQUERY : 0);
}
static inline int as_grid(int64_t B, int rows_per_wave) {
    const int64_t nrg = (B + rows_per_wave - 1) / rows_per_wave;
    int64_t g = (nrg + 3) / 4;
    if (g > 8192) g = 8192;
    return (int)(g > 0 ? g : 1);
}
static inline int as_shape_check(int64_t B, int L, int D, int H) {
    if (B < 0 || L < 0 || D < 1 || H < 1) return RECNOW_EINVAL;
    if (D > AS_MAX_D || H > AS_MAX_H) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}
extern "C" int recnow_attention_softmax_supported(int L, int D, int H) {
    return L >= 0 && D >= 1 && D <= AS_MAX_D && H >= 1 && H <= AS_MAX_H;
}
extern "C" int recnow_attention_softmax_tile(int which) {
    switch (which) {
        case 0: return AS_SPW;
        case 1: return AS_LANES * AS_V4;
        case 2: return AS_LANES;
        default: return RECNOW_EINVAL;
    }
}
extern "C" int recnow_attention_softmax_route(int which, int64_t B, int L, int D, int H, int align_mask) {
    if ((which != 0 && which != 1) || align_mask < 0 || align_mask > (which ? 63 : 7)) return RECNOW_EINVAL;
    const int rc = as_shape_check(B, L, D, H);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return 0;
    const AsRoute r = as_route(D, H, align_mask);
    return (r.cpl ? 200000 + 100 * r.cpl : 100000 + 100 * r.gs) + r.hb;
}

#define AS_HB_SWITCH(KERNEL, P, RPW, ...)                                                                                    \
    switch (route.hb) {                                                                                                      \
        case 1: hipLaunchKernelGGL((KERNEL<P, 1>), as_grid(B, RPW), 256, 0, st, __VA_ARGS__); break;                         \
        case 2: hipLaunchKernelGGL((KERNEL<P, 2>), as_grid(B, RPW), 256, 0, st, __VA_ARGS__); break;                         \
        case 4: hipLaunchKernelGGL((KERNEL<P, 4>), as_grid(B, RPW), 256, 0, st, __VA_ARGS__); break;                         \
        default: hipLaunchKernelGGL((KERNEL<P, 8>), as_grid(B, RPW), 256, 0, st, __VA_ARGS__); break;                        \
    }
#define AS_V4_LAUNCH(KERNEL, ...)                                                                                            \
    switch (route.cpl) {                                                                                                     \
        case 1: AS_HB_SWITCH(KERNEL, 1, AS_SPW, __VA_ARGS__) break;                                                          \
        case 2: AS_HB_SWITCH(KERNEL, 2, AS_SPW, __VA_ARGS__) break;                                                          \
        case 4: AS_HB_SWITCH(KERNEL, 4, AS_SPW, __VA_ARGS__) break;                                                          \
        case 8: AS_HB_SWITCH(KERNEL, 8, AS_SPW, __VA_ARGS__) break;                                                          \
        default: AS_HB_SWITCH(KERNEL, 16, AS_SPW, __VA_ARGS__) break;                                                        \
    }
#define AS_GS_LAUNCH(KERNEL, ...)                                                                                            \
    switch (route.gs) {                                                                                                      \
        case 16: AS_HB_SWITCH(KERNEL, 16, 4, __VA_ARGS__) break;                                                             \
        case 32: AS_HB_SWITCH(KERNEL, 32, 2, __VA_ARGS__) break;                                                             \
        default: AS_HB_SWITCH(KERNEL, 64, 1, __VA_ARGS__) break;                                                             \
    }

extern "C" int recnow_attention_softmax_fwd(const float* user, const float* query, const int32_t* lengths, const uint8_t* mask, int64_t B,
                                            int L, int D, int H, float scale, float* out, float* stat, void* stream) {
    const int rc = as_shape_check(B, L, D, H);
    if (rc != RECNOW_OK) return rc;
    if (!(scale > 0.f) || !(scale < __builtin_inff())) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    if ((L > 0 && !user) || !query || !out || !stat) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const AsRoute route = as_route(D, H, as_mis(user, query, out, nullptr, nullptr, nullptr));
    if (route.cpl) {
        AS_V4_LAUNCH(k_as_v4_fwd, user, query, lengths, mask, B, L, H, scale, out, stat)
    } else {
        AS_GS_LAUNCH(k_as_fwd, user, query, lengths, mask, B, L, D, H, scale, out, stat)
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
extern "C" int recnow_attention_softmax_bwd(const float* user, const float* query, const int32_t* lengths, const uint8_t* mask,
                                            const float* out, const float* stat, const float* dout, int64_t B, int L, int D, int H,
                                            float scale, float* duser, float* dquery, void* stream) {
    const int rc = as_shape_check(B, L, D, H);
    if (rc != RECNOW_OK) return rc;
    if (!(scale > 0.f) || !(scale < __builtin_inff())) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    if ((L > 0 && !user) || !query || !out || !stat || !dout) return RECNOW_EINVAL;
    if (!duser && !dquery) return RECNOW_OK;
    if (L == 0 && !dquery) return RECNOW_OK;
    hipStream_t st = (hipStream_t)stream;
    const AsRoute route = as_route(D, H, as_mis(user, query, out, dout, duser, dquery));
    if (route.cpl) {
        AS_V4_LAUNCH(k_as_v4_bwd, user, query, lengths, mask, out, stat, dout, B, L, H, scale, duser, dquery)
    } else {
        AS_GS_LAUNCH(k_as_bwd, user, query, lengths, mask, out, stat, dout, B, L, D, H, scale, duser, dquery)
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
