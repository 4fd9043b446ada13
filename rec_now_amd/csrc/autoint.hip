// InteractingLayer (AutoInt, Song et al. 2019, arXiv 1810.11921, section 4.3): multi-head self-attention over the fields -- C ABI 26.
//   Q = X Wq, K = X Wk, V = X Wv  (F, E), E = H * d, head h = columns [h d, (h+1) d);   S_h = Q_h K_h^T (* 1/sqrt(d));
//   A_h = softmax over the keys of S_h (row maximum subtracted);   pre = concat_h A_h V_h (+ X Wr);   out = relu(pre) or pre.
// `fields` is a DEVICE array of F device pointers; field f of sample b starts at fields[f] + b * xstride (one row stride for all fields, so a
// (B, F, D) tensor and column views of a (B, F*D) tensor pass as they are).  fp32 FMA on exact fp32 operands, no float atomics, every
// reduction in a fixed order.  Q, K, V, S, A and pre live in LDS and registers only; the backward recomputes them from X.
//
// One wave per sample, a workgroup of 1, 2 or 4 waves over a contiguous chunk of samples.  Every wave-private LDS tile is TRANSPOSED,
// [feature][field] with the row stride FS = 4 ceil(F / 4) + 4: the lanes of a wave differ in the field (the key, for the scores), so they
// touch consecutive words, and the 4 extra words keep rows of 16-byte reads off each other's banks.  Pad columns and pad rows are zeroed once
// and never written.  Tiles of one wave, in order:
//   forward:   xt (DP rows)  qt kt vt pt (EP rows each)  at (4 rows: the attention of a block of 4 queries)
//   backward:  xt  qt kt vt  dqt dkt dvt  pt  st (4 rows: dS of a block of 4 queries)           DP = 4 ceil(D / 4), EP = 4 ceil(E / 4)
// pt holds X Wr, then pre, then (backward) dpre.  Scores: lane j is key j and takes 4 queries at a time; the row maximum and the row sum
// are wave reductions (pairwise exchanges by DPP inside a row of 16 lanes, through the LDS crossbar across rows).
//
// Routes (recnow_autoint_route): AI_ROUTE_LDS keeps the 3 or 4 weight matrices (row stride EP + 4) and, in the backward, the workgroup's
// weight-gradient accumulators resident in LDS for the whole launch; AI_ROUTE_GLOBAL reads the weights through L2 and accumulates into the
// workgroup's slab of the workspace (every element is owned by one thread: a fixed order either way).
//
// Weight gradient: after every batch of `waves` samples the whole workgroup adds  X^T dQ, X^T dK, X^T dV, X^T dpre  of those samples, in
// sample then field order, to its fp32 partial; rn_part_reduce (partials.hpp) adds the partials of the G workgroups in fp64 in a fixed tree.
// Workspace (recnow_autoint_workspace_bytes): G * nW * D * E floats rounded up to 256 bytes, nW = 3 + use_res,
//   G = rn_part_groups(B, AI_DW_ROWS, AI_MAXG, nW D E) = max(1, min(ceil(B / AI_DW_ROWS), AI_MAXG, RN_PART_BYTES / (4 nW D E))).
#include "common.hpp"
#include "wave_softmax.hpp"                     // ai_wave_red4, ai_exp
#include "partials.hpp"
#include <math.h>

#define AI_ROUTE_LDS 0
#define AI_ROUTE_GLOBAL 1
#define AI_MAX_F 64
#define AI_MAX_D 64
#define AI_MAX_E 64
#define AI_MAX_H 8
#define AI_LDS_BYTES (160 * 1024)
#define AI_MAXG 1024                            // workgroups (and weight-gradient partials) of a launch at the most
#define AI_DW_ROWS 8                            // samples of one workgroup at the least

struct AiDesc {
    int F, D, E, H, d, DQ, EQ, DP, EP, ES, FS, fp2, nW, wres, relu, bwd, wavefl;
    float scale;
    int64_t B, xs, dxs, rows;                   // xs / dxs: row strides of the fields / their gradients; rows: samples per workgroup
    const float *Wq, *Wk, *Wv, *Wr;
};
struct AiTiles {
    float *xt, *qt, *kt, *vt, *gt, *pt, *at;    // gt: dqt, dkt, dvt (backward only); at: the 4-row tile
};

__device__ __forceinline__ const float* ai_wptr(const AiDesc& c, int m) { return m == 0 ? c.Wq : m == 1 ? c.Wk : m == 2 ? c.Wv : c.Wr; }
// W_m[k][e .. e+3], zeros past E
__device__ __forceinline__ rn_f4 ai_w4(const AiDesc& c, const float* wl, int m, int k, int e, bool vw) {
    if (c.wres) return *reinterpret_cast<const rn_f4*>(wl + (m * c.D + k) * c.ES + e);
    return rn_ld4(ai_wptr(c, m) + k * c.E + e, c.E - e, vw);
}
__device__ __forceinline__ bool ai_w_vec(const AiDesc& c) {
    return rn_vec4_ok(c.Wq, c.E, 0) && rn_vec4_ok(c.Wk, c.E, 0) && rn_vec4_ok(c.Wv, c.E, 0) && (c.nW < 4 || rn_vec4_ok(c.Wr, c.E, 0));
}
__device__ __forceinline__ AiTiles ai_tiles(const AiDesc& c, float* base) {
    const int T = c.EP * c.FS;
    AiTiles t;
    t.xt = base;
    t.qt = base + c.DP * c.FS;
    t.kt = t.qt + T;
    t.vt = t.kt + T;
    t.gt = t.vt + T;
    t.pt = t.vt + (c.bwd ? 4 : 1) * T;
    t.at = t.pt + T;
    return t;
}
// Whole workgroup: the resident weights (zero padded), zeroed accumulators and zeroed wave tiles.  Returns with a barrier.
__device__ __forceinline__ void ai_prologue(const AiDesc& c, float* lds, int nwaves) {
    int wfl = 0;
    if (c.wres) {
        wfl = c.nW * c.D * c.ES;
        const bool vw = ai_w_vec(c);
        const int SQ = c.ES >> 2;
        for (int e = threadIdx.x; e < c.nW * c.D * SQ; e += blockDim.x) {
            const int row = e / SQ, q = e - row * SQ, m = row / c.D, k = row - m * c.D;
            rn_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < c.EQ) v = rn_ld4(ai_wptr(c, m) + k * c.E + 4 * q, c.E - 4 * q, vw);
            *reinterpret_cast<rn_f4*>(lds + row * c.ES + 4 * q) = v;
        }
        if (c.bwd) wfl += c.nW * c.D * c.EP;
    }
    const int total = (c.wres ? wfl : 0) + nwaves * c.wavefl;
    for (int e = (c.wres ? c.nW * c.D * c.ES : 0) + threadIdx.x; e < total; e += blockDim.x) lds[e] = 0.f;
    __syncthreads();
}
// the attention weights of queries 4 ib .. 4 ib + 3 of head h for key `lane` (0 for lanes >= F and queries >= F); top: 1 where the key holds
// its row's maximum
__device__ __forceinline__ rn_f4 ai_attn(const AiDesc& c, const AiTiles& t, int h, int ib, int jj, bool valid, rn_f4& top) {
    const int FS = c.FS;
    const float* qr = t.qt + h * c.d * FS + 4 * ib;
    const float* kr = t.kt + h * c.d * FS + jj;
    rn_f4 s = {0.f, 0.f, 0.f, 0.f};
    for (int cc = 0; cc < c.d; ++cc) s += *reinterpret_cast<const rn_f4*>(qr + cc * FS) * kr[cc * FS];
    rn_f4 a, p;
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = valid ? s[u] : -INFINITY;
    const rn_f4 mx = ai_wave_red4<true>(s, c.fp2);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        p[u] = valid ? ai_exp(s[u] - mx[u]) : 0.f;
        top[u] = valid && s[u] == mx[u] ? 1.f : 0.f;
    }
    const rn_f4 l = ai_wave_red4<false>(p, c.fp2);
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = valid && 4 * ib + u < c.F ? p[u] / l[u] : 0.f;
    return a;
}
// item (u, cc) of a block of 4 queries: sum_j row_u[j] * tile[h d + cc][j]
__device__ __forceinline__ float ai_rowdot(const AiDesc& c, const float* row, const float* tr) {
    rn_f4 s4 = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < c.FS - 4; j += 4) s4 += *reinterpret_cast<const rn_f4*>(row + j) * *reinterpret_cast<const rn_f4*>(tr + j);
    return (s4.x + s4.y) + (s4.z + s4.w);
}

// X -> xt, the projections -> qt (scaled), kt, vt, pt (= X Wr), then head by head pt = pre.  One wave.
__device__ __forceinline__ void ai_sample_fwd(const AiDesc& c, const float* const* fields, const float* wl, bool vw, const AiTiles& t, int64_t b,
                                              int lane) {
    const int FS = c.FS;
    for (int e = lane; e < c.F * c.DQ; e += 64) {
        const int f = e / c.DQ, q = e - f * c.DQ;
        const float* xf = fields[f];
        const rn_f4 v = rn_ld4(xf + b * c.xs + 4 * q, c.D - 4 * q, rn_vec4_ok(xf, c.D, c.xs));
        float* o = t.xt + 4 * q * FS + f;
        o[0] = v.x; o[FS] = v.y; o[2 * FS] = v.z; o[3 * FS] = v.w;
    }
    RN_LDS_WAVE_SYNC();
    const int per = c.F * c.EQ;
    for (int e = lane; e < c.nW * per; e += 64) {
        const int m = e / per, r = e - m * per, f = r / c.EQ, q = r - f * c.EQ;
        rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < c.D; ++k) acc += t.xt[k * FS + f] * ai_w4(c, wl, m, k, 4 * q, vw);
        if (m == 0) acc *= c.scale;
        float* o = (m == 3 ? t.pt : t.qt + m * c.EP * FS) + 4 * q * FS + f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * q + u < c.E) o[u * FS] = acc[u];
    }
    RN_LDS_WAVE_SYNC();
    const int jj = min(lane, FS - 1);
    const bool valid = lane < c.F;
    for (int h = 0; h < c.H; ++h) {
        for (int ib = 0; 4 * ib < c.F; ++ib) {
            rn_f4 top;
            const rn_f4 a = ai_attn(c, t, h, ib, jj, valid, top);
            if (lane < FS) {
#pragma unroll
                for (int u = 0; u < 4; ++u) t.at[u * FS + lane] = a[u];
            }
            RN_LDS_WAVE_SYNC();
            for (int e = lane; e < 4 * c.d; e += 64) {
                const int u = e / c.d, cc = e - u * c.d, i = 4 * ib + u;
                const float o = ai_rowdot(c, t.at + u * FS, t.vt + (h * c.d + cc) * FS);
                if (i < c.F) {
                    float* p = t.pt + (h * c.d + cc) * FS + i;
                    *p = (c.nW == 4 ? *p : 0.f) + o;
                }
            }
            RN_LDS_WAVE_SYNC();                                 // `at` read before the next block overwrites it
        }
    }
}

__global__ void __launch_bounds__(256)
k_ai_fwd(const float* const* __restrict__ fields, float* __restrict__ out, AiDesc c) {
    extern __shared__ __attribute__((aligned(16))) float ai_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    ai_prologue(c, ai_lds, nw);
    const float* wl = ai_lds;
    const AiTiles t = ai_tiles(c, ai_lds + (c.wres ? c.nW * c.D * c.ES : 0) + w * c.wavefl);
    const bool vw = ai_w_vec(c), vo = rn_vec4_ok(out, c.E, 0);
    const int64_t r0 = (int64_t)blockIdx.x * c.rows, r1 = min(c.B, r0 + c.rows);
    for (int64_t b = r0 + w; b < r1; b += nw) {
        ai_sample_fwd(c, fields, wl, vw, t, b, lane);
        for (int e = lane; e < c.F * c.EQ; e += 64) {
            const int f = e / c.EQ, q = e - f * c.EQ;
            const float* p = t.pt + 4 * q * c.FS + f;
            rn_f4 v = {p[0], p[c.FS], p[2 * c.FS], p[3 * c.FS]};
            if (c.relu) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (v[u] > 0.f || v[u] != v[u]) ? v[u] : 0.f;       // a NaN stays a NaN
            }
            rn_st4_stream(out + (b * c.F + f) * c.E + 4 * q, v, c.E - 4 * q, vo);
        }
        RN_LDS_WAVE_SYNC();                                     // tiles read before the next sample overwrites them
    }
}

// part: this launch's partials, slab g = blockIdx.x of nW * D * E floats (NULL: no weight gradient).
__global__ void __launch_bounds__(256)
k_ai_bwd(const float* const* __restrict__ fields, float* const* __restrict__ dfields, const float* __restrict__ dout, float* __restrict__ part,
         AiDesc c) {
    extern __shared__ __attribute__((aligned(16))) float ai_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int FS = c.FS, F = c.F, D = c.D, E = c.E, EP = c.EP, T = EP * FS;
    ai_prologue(c, ai_lds, nw);
    const float* wl = ai_lds;
    float* dwl = ai_lds + c.nW * D * c.ES;                  // LDS route only
    float* tiles0 = ai_lds + (c.wres ? c.nW * D * (c.ES + EP) : 0);
    const AiTiles t = ai_tiles(c, tiles0 + w * c.wavefl);
    float* dqt = t.gt;
    float* dkt = dqt + T;
    float* dvt = dkt + T;
    const bool vw = ai_w_vec(c), vg = rn_vec4_ok(dout, E, 0), vs = (E & 3) == 0;
    float* slab = part ? part + (int64_t)blockIdx.x * c.nW * D * E : nullptr;
    const int nitem = c.nW * D * c.EQ;                      // (m, k, e quad) items of the weight gradient, one owner thread each
    if (slab && !c.wres)
        for (int it = threadIdx.x; it < nitem; it += blockDim.x) {
            const int row = it / c.EQ, q = it - row * c.EQ;
            rn_st4(slab + row * E + 4 * q, rn_f4{0.f, 0.f, 0.f, 0.f}, E - 4 * q, vs);
        }
    const int jj = min(lane, FS - 1);
    const bool valid = lane < F;
    const int64_t r0 = (int64_t)blockIdx.x * c.rows, r1 = min(c.B, r0 + c.rows);
    for (int64_t b0 = r0; b0 < r1; b0 += nw) {              // uniform over the workgroup
        const int64_t b = b0 + w;
        if (b < r1) {
            ai_sample_fwd(c, fields, wl, vw, t, b, lane);
            // pt: pre -> dpre;  dkt, dvt: cleared (dqt is written whole)
            for (int e = lane; e < F * c.EQ; e += 64) {
                const int f = e / c.EQ, q = e - f * c.EQ;
                const rn_f4 g = rn_ld4(dout + (b * F + f) * E + 4 * q, E - 4 * q, vg);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (4 * q + u < E) {
                        float* p = t.pt + (4 * q + u) * FS + f;
                        const float pre = *p;
                        *p = c.relu ? (pre > 0.f ? g[u] : (pre != pre ? pre : 0.f)) : g[u];
                    }
            }
            for (int e = lane; e < 2 * T; e += 64) dkt[e] = 0.f;
            RN_LDS_WAVE_SYNC();
            for (int h = 0; h < c.H; ++h) {
                const int hd = h * c.d;
                for (int ib = 0; 4 * ib < F; ++ib) {
                    rn_f4 top;
                    const rn_f4 a = ai_attn(c, t, h, ib, jj, valid, top);
                    // dA[i][j] = <dO_i, V_j>;  dV_j += sum_i A[i][j] dO_i        (dO = the head's columns of dpre)
                    rn_f4 dA = {0.f, 0.f, 0.f, 0.f};
                    for (int cc = 0; cc < c.d; ++cc) {
                        const rn_f4 g4 = *reinterpret_cast<const rn_f4*>(t.pt + (hd + cc) * FS + 4 * ib);
                        dA += g4 * t.vt[(hd + cc) * FS + jj];
                        if (valid) dvt[(hd + cc) * FS + lane] += rn_dot4(a, g4);
                    }
                    // dS = a (dA - sum a dA) does not change when dA is shifted; shifted by the dA of the row's top key, a near one-hot
                    // row (a_top ~ 1, dA_top - sum a dA cancelling) keeps its small dS_top to full precision
                    rn_f4 dS, sh, ad;
#pragma unroll
                    for (int u = 0; u < 4; ++u) sh[u] = top[u] != 0.f ? dA[u] : -INFINITY;
                    sh = ai_wave_red4<true>(sh, c.fp2);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        dA[u] -= sh[u];
                        ad[u] = valid ? a[u] * dA[u] : 0.f;
                    }
                    const rn_f4 rd = ai_wave_red4<false>(ad, c.fp2);                        // every lane takes part in the reduction
#pragma unroll
                    for (int u = 0; u < 4; ++u) dS[u] = valid ? a[u] * (dA[u] - rd[u]) : 0.f;
                    // dK_j += sum_i dS[i][j] Q_i (Q carries the scale);  dQ_i = scale * sum_j dS[i][j] K_j
                    for (int cc = 0; cc < c.d; ++cc)
                        if (valid) dkt[(hd + cc) * FS + lane] += rn_dot4(dS, *reinterpret_cast<const rn_f4*>(t.qt + (hd + cc) * FS + 4 * ib));
                    if (lane < FS) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) t.at[u * FS + lane] = dS[u];
                    }
                    RN_LDS_WAVE_SYNC();
                    for (int e = lane; e < 4 * c.d; e += 64) {
                        const int u = e / c.d, cc = e - u * c.d, i = 4 * ib + u;
                        const float o = ai_rowdot(c, t.at + u * FS, t.kt + (hd + cc) * FS);
                        if (i < F) dqt[(hd + cc) * FS + i] = o * c.scale;
                    }
                    RN_LDS_WAVE_SYNC();
                }
            }
            // dX_f = dQ_f Wq^T + dK_f Wk^T + dV_f Wv^T (+ dpre_f Wr^T)
            for (int e = lane; e < F * c.DQ; e += 64) {
                const int f = e / c.DQ, kq = e - f * c.DQ;
                int kk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) kk[u] = min(4 * kq + u, D - 1);      // components >= D repeat row D-1: never stored
                rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int m = 0; m < c.nW; ++m) {
                    const float* tl = dqt + m * T + f;
                    for (int e2 = 0; e2 < EP; e2 += 4) {
                        const rn_f4 p = {tl[e2 * FS], tl[(e2 + 1) * FS], tl[(e2 + 2) * FS], tl[(e2 + 3) * FS]};
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u] += rn_dot4(ai_w4(c, wl, m, kk[u], e2, vw), p);
                    }
                }
                float* df = dfields[f];
                rn_st4(df + b * c.dxs + 4 * kq, acc, D - 4 * kq, rn_vec4_ok(df, D, c.dxs));
            }
            RN_LDS_WAVE_SYNC();
        }
        if (slab) {
            __syncthreads();                                // every wave's tiles are complete
            const int nvalid = (int)min((int64_t)nw, r1 - b0);
            for (int it = threadIdx.x; it < nitem; it += blockDim.x) {
                const int row = it / c.EQ, q = it - row * c.EQ, m = row / D, k = row - m * D;
                rn_f4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int w2 = 0; w2 < nvalid; ++w2) {
                    const float* xr = tiles0 + w2 * c.wavefl + k * FS;
                    const float* tl = tiles0 + w2 * c.wavefl + (c.DP * FS + 3 * T) + (m * EP + 4 * q) * FS;
                    for (int f = 0; f < FS - 4; f += 4) {
                        const rn_f4 x4 = *reinterpret_cast<const rn_f4*>(xr + f);
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u] += rn_dot4(x4, *reinterpret_cast<const rn_f4*>(tl + u * FS + f));
                    }
                }
                if (c.wres) {
                    *reinterpret_cast<rn_f4*>(dwl + row * EP + 4 * q) += acc;
                } else {
                    float* s = slab + row * E + 4 * q;
                    rn_st4(s, rn_ld4(s, E - 4 * q, vs) + acc, E - 4 * q, vs);
                }
            }
            __syncthreads();                                // tiles consumed
        }
    }
    if (slab && c.wres)
        for (int it = threadIdx.x; it < nitem; it += blockDim.x) {
            const int row = it / c.EQ, q = it - row * c.EQ;
            rn_st4(slab + row * E + 4 * q, *reinterpret_cast<const rn_f4*>(dwl + row * EP + 4 * q), E - 4 * q, vs);
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
static inline bool ai_shape_ok(int F, int D, int H, int d) {
    return F >= 1 && F <= AI_MAX_F && D >= 1 && D <= AI_MAX_D && H >= 1 && H <= AI_MAX_H && d >= 1 && (int64_t)H * d <= AI_MAX_E;
}
// waves per workgroup, weight residency, LDS bytes and floats of one wave's tiles
static void ai_cfg(int F, int D, int E, int nW, int bwd, int* waves, int* wres, size_t* lds, int* wavefl) {
    const int DP = (D + 3) & ~3, EP = (E + 3) & ~3, FS = ((F + 3) & ~3) + 4;
    *wavefl = (DP + (bwd ? 7 : 4) * EP + 4) * FS;
    const size_t wfl = (size_t)nW * D * (EP + 4) + (bwd ? (size_t)nW * D * EP : 0);
    static const int order[6][2] = {{4, 1}, {2, 1}, {4, 0}, {2, 0}, {1, 1}, {1, 0}};
    for (int t = 0; t < 6; ++t) {
        const size_t bytes = 4 * ((order[t][1] ? wfl : 0) + (size_t)order[t][0] * *wavefl);
        if (bytes <= AI_LDS_BYTES || t == 5) {               // the last entry always fits: (64 + 7 * 64 + 4) * 68 floats
            *waves = order[t][0];
            *wres = order[t][1];
            *lds = bytes;
            return;
        }
    }
}
static int ai_groups(int64_t B, int nW, int D, int E) { return rn_part_groups(B, AI_DW_ROWS, AI_MAXG, (int64_t)nW * D * E); }
static AiDesc ai_desc(int F, int64_t B, int D, int H, int d, const float* Wq, const float* Wk, const float* Wv, const float* Wr, int scaling,
                      int relu, int bwd, int64_t xs, int64_t dxs, int* waves, size_t* lds, int* grid) {
    AiDesc c;
    c.F = F; c.D = D; c.E = H * d; c.H = H; c.d = d;
    c.DQ = (D + 3) / 4; c.EQ = (c.E + 3) / 4; c.DP = 4 * c.DQ; c.EP = 4 * c.EQ; c.ES = c.EP + 4; c.FS = ((F + 3) & ~3) + 4;
    c.fp2 = 1;
    while (c.fp2 < F) c.fp2 <<= 1;
    c.nW = Wr ? 4 : 3; c.relu = relu; c.bwd = bwd;
    c.scale = scaling ? (float)(1.0 / sqrt((double)d)) : 1.f;
    c.B = B; c.xs = xs; c.dxs = dxs;
    c.Wq = Wq; c.Wk = Wk; c.Wv = Wv; c.Wr = Wr;
    ai_cfg(F, D, c.E, c.nW, bwd, waves, &c.wres, lds, &c.wavefl);
    const int G = ai_groups(B, c.nW, D, c.E);
    int64_t rows = (B + G - 1) / G;
    rows = (rows + *waves - 1) / *waves * *waves;
    c.rows = rows;
    *grid = (int)((B + rows - 1) / rows);                   // <= G, every workgroup has a sample
    return c;
}
extern "C" int recnow_autoint_supported(int F, int D, int H, int d) { return ai_shape_ok(F, D, H, d) ? 1 : 0; }

extern "C" int recnow_autoint_route(int F, int D, int H, int d, int use_res, int bwd) {
    if (!ai_shape_ok(F, D, H, d)) return RECNOW_EUNSUPPORTED;
    int waves, wres, wavefl;
    size_t lds;
    ai_cfg(F, D, H * d, use_res ? 4 : 3, bwd ? 1 : 0, &waves, &wres, &lds, &wavefl);
    return wres ? AI_ROUTE_LDS : AI_ROUTE_GLOBAL;
}

extern "C" size_t recnow_autoint_workspace_bytes(int64_t B, int F, int D, int H, int d, int use_res) {
    if (!ai_shape_ok(F, D, H, d) || B <= 0) return 0;
    const int nW = use_res ? 4 : 3;
    return rn_align((size_t)ai_groups(B, nW, D, H * d) * nW * D * H * d * sizeof(float));
}

extern "C" int recnow_autoint_fwd(const float* const* fields, int64_t xstride, int F, int64_t B, int D, int H, int d, const float* Wq,
                                  const float* Wk, const float* Wv, const float* Wr, int scaling, int relu, float* out, void* stream) {
    if (F < 1 || B < 0 || D < 1 || H < 1 || d < 1) return RECNOW_EINVAL;
    if (!ai_shape_ok(F, D, H, d)) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!fields || !Wq || !Wk || !Wv || !out || xstride < D) return RECNOW_EINVAL;
    int waves, grid;
    size_t lds;
    const AiDesc c = ai_desc(F, B, D, H, d, Wq, Wk, Wv, Wr, scaling, relu, 0, xstride, 0, &waves, &lds, &grid);
    if (lds > 64 * 1024) RN_HIP(rn_lds_grant((const void*)k_ai_fwd, AI_LDS_BYTES));       // resident weights beside up to four waves' tiles
    hipLaunchKernelGGL(k_ai_fwd, grid, waves * 64, lds, (hipStream_t)stream, fields, out, c);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_autoint_bwd(const float* const* fields, int64_t xstride, float* const* dfields, int64_t dxstride, int F, int64_t B, int D,
                                  int H, int d, const float* Wq, const float* Wk, const float* Wv, const float* Wr, int scaling, int relu,
                                  const float* dout, float* dWq, float* dWk, float* dWv, float* dWr, void* ws, size_t ws_bytes, void* stream) {
    if (F < 1 || B < 0 || D < 1 || H < 1 || d < 1) return RECNOW_EINVAL;
    if (!ai_shape_ok(F, D, H, d)) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!fields || !dfields || !Wq || !Wk || !Wv || !dout || xstride < D || dxstride < D) return RECNOW_EINVAL;
    const bool want_dw = dWq || dWk || dWv || dWr;
    if (want_dw && (!dWq || !dWk || !dWv || (Wr && !dWr))) return RECNOW_EINVAL;       // all of them or none
    float* part = nullptr;
    if (want_dw) {
        if (!ws || ws_bytes < recnow_autoint_workspace_bytes(B, F, D, H, d, Wr ? 1 : 0)) return RECNOW_EWORKSPACE;
        part = (float*)ws;
    }
    int waves, grid;
    size_t lds;
    const AiDesc c = ai_desc(F, B, D, H, d, Wq, Wk, Wv, Wr, scaling, relu, 1, xstride, dxstride, &waves, &lds, &grid);
    if (lds > 64 * 1024) RN_HIP(rn_lds_grant((const void*)k_ai_bwd, AI_LDS_BYTES));       // the same, and the weight-gradient accumulators
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ai_bwd, grid, waves * 64, lds, st, fields, dfields, dout, part, c);
    RN_LAUNCH_CHECK();
    if (!part) return RECNOW_OK;
    const int64_t DE = (int64_t)D * c.E;
    const RnPartDst dst = {{dWq, dWk, dWv, dWr}, {DE, 2 * DE, 3 * DE, c.nW * DE}};
    return rn_part_reduce(part, c.nW * DE, 1, grid, c.nW * DE, 0, dst, st);
}
