// StarDenseLayer / StackedDenseLayer: a Dense layer whose kernel and bias are personalised per row by K parameter rows,
// reference rec_now/layers/star_dense_layer.py:118-163 and stacked_dense_layer.py:116-155:
//   P_k[b] = [ kernel part (D x U, row-major [d][u]) | bias part (U) ],   R = D*U + U floats per row
//   MUL (star):    Weff[b] = W * prod_k P_k[b][:DU]          beff[b] = sum_k P_k[b][DU:] + bias - K
//   ADD (stacked): Weff[b] = W + w * sum_k P_k[b][:DU]       beff[b] = bias + w * sum_k P_k[b][DU:]
//   y[b] = act(x[b] . Weff[b] + beff[b])
// The reference materialises Weff as a (B, D, U) tensor.  Here Weff exists only in registers: every P_k element is read once
// (non-temporal), W (D x U, shared by all rows) is re-read from L2, so both directions are bound by streaming the P_k (and,
// backward, writing the dP_k) through HBM.
//
// Thread geometry (one 256-thread workgroup): TU = 2^tu_bits <= 64 lanes across u, TD = 256 / TU across d, lane t = td*TU + tu.
// Lane tu owns VEC consecutive columns of each chunk of TU*VEC columns (nj chunks cover U), so for U = 1 or 5 the lanes span d,
// and the TU lanes of one d are a contiguous, aligned group inside one wave: the reduction over u (dx) is a shuffle.
//   forward:  one row per workgroup (grid-stride); the reduction over d goes through LDS in a fixed order.
//   backward: workgroup (tile, chunk) owns the TD rows d of its tile and a chunk of batch rows; its lanes keep the dW / dbias partials
//             of their fixed (d, u) over the chunk in registers and write them once to part[chunk]; k_sd_reduce sums the chunks in
//             order.  No float atomics: the gradients are bit-identical from run to run.
#include "common.hpp"

#define SD_MAXK 4
#define SD_THREADS 256
#define SD_TARGET_WG 2048       // backward grid: 8 workgroups of 256 per CU
#define SD_MIN_ROWS 8           // fewest batch rows per backward chunk
#define SD_RB 4                 // batch rows whose loads the backward issues together

struct SdPtrs {
    const float* p[SD_MAXK];
    float* dp[SD_MAXK];
};

template <int VEC>
__device__ __forceinline__ void sd_ld(const float* base, int64_t i, float* v, bool stream) {
    if constexpr (VEC == 4) {
        const rn_gcf4 q = (rn_gcf4)(base + i);
        const rn_f4 t = stream ? RN_LD_STREAM(q) : *q;
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        const rn_gcf q = (rn_gcf)(base + i);
        v[0] = stream ? RN_LD_STREAM(q) : *q;
    }
}
template <int VEC>
__device__ __forceinline__ void sd_st(float* base, int64_t i, const float* v) {
    if constexpr (VEC == 4) {
        const rn_f4 t = {v[0], v[1], v[2], v[3]};
        RN_ST_STREAM((rn_gf4)(base + i), t);
    } else {
        RN_ST_STREAM((rn_gf)(base + i), v[0]);
    }
}

template <int K, int VEC, bool STAR>
__global__ void __launch_bounds__(SD_THREADS)
k_sd_fwd(const float* __restrict__ x, SdPtrs P, float w, const float* __restrict__ W, const float* __restrict__ bias, int64_t B, int D,
         int U, int tu_bits, int nj, int act, float* __restrict__ y) {
    __shared__ float red[SD_THREADS * VEC];
    const int TU = 1 << tu_bits, TD = SD_THREADS >> tu_bits, CW = TU * VEC;
    const int tu = threadIdx.x & (TU - 1), td = threadIdx.x >> tu_bits;
    const int64_t DU = (int64_t)D * U, R = DU + U;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const float* xb = x + b * D;
        for (int j = 0; j < nj; ++j) {
            const int u0 = j * CW + tu * VEC;
            float acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
            if (u0 < U) {          // VEC = 4 only when U % 4 == 0: a vector is wholly in or out
#pragma unroll 4
                for (int d = td; d < D; d += TD) {
                    const int64_t e = (int64_t)d * U + u0;
                    float wv[VEC], pv[K][VEC];
                    sd_ld<VEC>(W, e, wv, false);
#pragma unroll
                    for (int k = 0; k < K; ++k) sd_ld<VEC>(P.p[k], b * R + e, pv[k], true);
                    const float xd = xb[d];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        float m = pv[0][v];
#pragma unroll
                        for (int k = 1; k < K; ++k) m = STAR ? m * pv[k][v] : m + pv[k][v];
                        const float weff = STAR ? wv[v] * m : wv[v] + w * m;
                        acc[v] = fmaf(xd, weff, acc[v]);
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) red[td * CW + tu * VEC + v] = acc[v];
            __syncthreads();
            const int t = threadIdx.x, u = j * CW + t;
            if (t < CW && u < U) {
                float s = 0.f;
                for (int i = 0; i < TD; ++i) s += red[i * CW + t];
                float pb = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) pb += P.p[k][b * R + DU + u];
                // star: kernel and bias share one ones-initialised table, so each of the K bias parts carries +1 (star_dense_layer.py:152-155)
                float be = STAR ? pb : w * pb;
                if (bias) be += bias[u];
                if (STAR) be -= (float)K;
                y[b * U + u] = rn_act(s + be, act);
            }
            __syncthreads();
        }
    }
}

// dz = dy * act'(y);  for each k with dP_k:  dP_k[b][d][u] = MUL: dz x_d W_du prod_{j != k} P_j[b][d][u]   ADD: w x_d dz
//                                             dP_k[b][DU + u] = MUL: dz   ADD: w dz
// dx[b][d] = sum_u Weff[b][d][u] dz[b][u];  part[chunk][d][u] = sum_{b in chunk} x_d dz_u (MUL: * prod_k P_k);  part[chunk][DU + u] = sum dz_u
template <int K, int VEC, bool STAR>
__global__ void __launch_bounds__(SD_THREADS)
k_sd_bwd(const float* __restrict__ x, SdPtrs P, float w, const float* __restrict__ W, const float* __restrict__ y,
         const float* __restrict__ dy, int64_t B, int D, int U, int tu_bits, int nj, int act, int64_t rows, float* __restrict__ dx,
         float* __restrict__ part) {
    const int TU = 1 << tu_bits, TD = SD_THREADS >> tu_bits, CW = TU * VEC;
    const int tu = threadIdx.x & (TU - 1), td = threadIdx.x >> tu_bits;
    const int d = blockIdx.x * TD + td;
    const bool dok = d < D;
    const bool bias_lane = blockIdx.x == 0 && td == 0;     // owns the bias part of its columns (d = 0 exists in tile 0)
    const int64_t DU = (int64_t)D * U, R = DU + U;
    const int64_t b0 = (int64_t)blockIdx.y * rows, b1 = b0 + rows < B ? b0 + rows : B;
    bool any_dp = false;
#pragma unroll
    for (int k = 0; k < K; ++k) any_dp |= P.dp[k] != nullptr;
    const bool need_p = STAR || dx != nullptr;
    for (int j = 0; j < nj; ++j) {
        const int u0 = j * CW + tu * VEC;
        const bool uok = u0 < U, ok = dok && uok;
        const int64_t e = ok ? (int64_t)d * U + u0 : 0;
        float wv[VEC], gw[VEC], gb[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) wv[v] = gw[v] = gb[v] = 0.f;
        if (ok) sd_ld<VEC>(W, e, wv, false);
        for (int64_t bb = b0; bb < b1; bb += SD_RB) {
            float xd[SD_RB], dz[SD_RB][VEC], pv[SD_RB][K][VEC];
            // load phase: SD_RB rows of everything before any store (the dP_k stores could alias the P_k for the compiler)
#pragma unroll
            for (int r = 0; r < SD_RB; ++r) {
                const int64_t b = bb + r;
                const bool rok = b < b1;
                xd[r] = ok && rok ? x[b * D + d] : 0.f;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const int64_t i = b * U + u0 + v;
                    dz[r][v] = uok && rok ? dy[i] * rn_act_grad_from_out(y[i], act) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) pv[r][k][v] = 0.f;
                    if (need_p && ok && rok) sd_ld<VEC>(P.p[k], b * R + e, pv[r][k], true);
                }
            }
#pragma unroll
            for (int r = 0; r < SD_RB; ++r) {
                const int64_t b = bb + r;
                const bool rok = b < b1;
                float gx = 0.f;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    float m = pv[r][0][v];
#pragma unroll
                    for (int k = 1; k < K; ++k) m = STAR ? m * pv[r][k][v] : m + pv[r][k][v];
                    const float weff = STAR ? wv[v] * m : wv[v] + w * m;
                    gx = fmaf(weff, dz[r][v], gx);
                    const float xz = xd[r] * dz[r][v];
                    gw[v] = fmaf(xz, STAR ? m : 1.f, gw[v]);
                    gb[v] += dz[r][v];
                }
                if (any_dp && ok && rok) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        if (!P.dp[k]) continue;
                        float g[VEC];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) {
                            float o = xd[r] * dz[r][v];
                            if (STAR) {
                                o *= wv[v];
#pragma unroll
                                for (int i = 0; i < K; ++i)
                                    if (i != k) o *= pv[r][i][v];
                            } else {
                                o *= w;
                            }
                            g[v] = o;
                        }
                        sd_st<VEC>(P.dp[k], b * R + e, g);
                    }
                }
                if (any_dp && bias_lane && uok && rok) {
                    float g[VEC];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) g[v] = STAR ? dz[r][v] : w * dz[r][v];
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (P.dp[k]) sd_st<VEC>(P.dp[k], b * R + DU + u0, g);
                }
                if (dx) {                   // uniform branch: every lane of the TU group takes part in the shuffles
                    for (int o = TU >> 1; o > 0; o >>= 1) gx += __shfl_xor(gx, o, 64);
                    if (tu == 0 && dok && rok) {
                        float* p = dx + b * D + d;
                        *p = j == 0 ? gx : *p + gx;       // later column chunks: the same lane re-reads what it wrote
                    }
                }
            }
        }
        if (part) {
            float* pc = part + (int64_t)blockIdx.y * R;
            if (ok) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) pc[e + v] = gw[v];
            }
            if (bias_lane && uok) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) pc[DU + u0 + v] = gb[v];
            }
        }
    }
}

// dW[i] (i < DU) and dbias[i - DU] = sum over the chunks of part[c][i], in chunk order.
__global__ void __launch_bounds__(SD_THREADS)
k_sd_reduce(const float* __restrict__ part, int nchunk, int64_t DU, int U, float* __restrict__ dW, float* __restrict__ db) {
    const int64_t R = DU + U;
    for (int64_t i = (int64_t)blockIdx.x * SD_THREADS + threadIdx.x; i < R; i += (int64_t)gridDim.x * SD_THREADS) {
        float s = 0.f;
        for (int c = 0; c < nchunk; ++c) s += part[c * R + i];
        if (i < DU) {
            if (dW) dW[i] = s;
        } else if (db) {
            db[i - DU] = s;
        }
    }
}

namespace {
struct SdGeo {
    int vec, tu_bits, td, nj, ndt;
};

SdGeo sd_geo(int D, int U, int vec) {
    SdGeo g;
    g.vec = vec;
    const int cols = (U + vec - 1) / vec;
    g.tu_bits = 0;
    while ((1 << g.tu_bits) < cols && g.tu_bits < 6) ++g.tu_bits;
    g.td = SD_THREADS >> g.tu_bits;
    g.nj = (cols + (1 << g.tu_bits) - 1) >> g.tu_bits;
    g.ndt = (D + g.td - 1) / g.td;
    return g;
}

// backward batch chunks: a function of the shape alone, so the workspace query needs no pointers
void sd_chunks(int64_t B, int D, int U, int* nchunk, int64_t* rows) {
    const SdGeo g = sd_geo(D, U, U % 4 == 0 ? 4 : 1);
    int64_t n = SD_TARGET_WG / g.ndt;
    const int64_t most = (B + SD_MIN_ROWS - 1) / SD_MIN_ROWS;
    if (n > most) n = most;
    if (n < 1) n = 1;
    int64_t r = (B + n - 1) / n;
    r = (r + SD_RB - 1) / SD_RB * SD_RB;
    *rows = r;
    *nchunk = (int)((B + r - 1) / r);
}

bool sd_aligned(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

template <template <int, int, bool> class F, typename... A>
int sd_dispatch(int K, int vec, bool star, A... a) {
#define SD_CASE(KK)                                                  \
    case KK:                                                         \
        if (vec == 4) return star ? F<KK, 4, true>::run(a...) : F<KK, 4, false>::run(a...); \
        return star ? F<KK, 1, true>::run(a...) : F<KK, 1, false>::run(a...);
    switch (K) {
        SD_CASE(1)
        SD_CASE(2)
        SD_CASE(3)
        SD_CASE(4)
    }
#undef SD_CASE
    return RECNOW_EUNSUPPORTED;
}

template <int K, int VEC, bool STAR>
struct SdFwd {
    static int run(dim3 grid, hipStream_t st, const float* x, SdPtrs P, float w, const float* W, const float* bias, int64_t B, int D, int U,
                   int tu_bits, int nj, int act, float* y) {
        hipLaunchKernelGGL((k_sd_fwd<K, VEC, STAR>), grid, SD_THREADS, 0, st, x, P, w, W, bias, B, D, U, tu_bits, nj, act, y);
        return 0;
    }
};
template <int K, int VEC, bool STAR>
struct SdBwd {
    static int run(dim3 grid, hipStream_t st, const float* x, SdPtrs P, float w, const float* W, const float* y, const float* dy, int64_t B,
                   int D, int U, int tu_bits, int nj, int act, int64_t rows, float* dx, float* part) {
        hipLaunchKernelGGL((k_sd_bwd<K, VEC, STAR>), grid, SD_THREADS, 0, st, x, P, w, W, y, dy, B, D, U, tu_bits, nj, act, rows, dx, part);
        return 0;
    }
};

int sd_check(const float* x, const float* const* params_host, int K, int mode, const float* kernel, int64_t B, int D, int U, int act) {
    if (K < 1 || B < 0 || D < 1 || U < 1 || act < RECNOW_ACT_LINEAR || act > RECNOW_ACT_SIGMOID) return RECNOW_EINVAL;
    if (mode != RECNOW_STAR_MUL && mode != RECNOW_STAR_ADD) return RECNOW_EINVAL;
    if (K > SD_MAXK) return RECNOW_EUNSUPPORTED;
    if (!x || !params_host || !kernel) return RECNOW_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!params_host[k]) return RECNOW_EINVAL;
    return RECNOW_OK;
}
}  // namespace

extern "C" size_t recnow_star_dense_workspace_bytes(int64_t B, int D, int U) {
    if (B < 1 || D < 1 || U < 1) return 0;
    int nchunk;
    int64_t rows;
    sd_chunks(B, D, U, &nchunk, &rows);
    return rn_align((size_t)nchunk * ((size_t)D * U + U) * sizeof(float));
}

extern "C" int recnow_star_dense_fwd(const float* x, const float* const* params_host, int K, int mode, float weight, const float* kernel,
                                     const float* bias, int64_t B, int D, int U, int act, float* y, void* stream) {
    int rc = sd_check(x, params_host, K, mode, kernel, B, D, U, act);
    if (rc) return rc;
    if (!y) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    SdPtrs P = {};
    bool al = sd_aligned(kernel);
    for (int k = 0; k < K; ++k) P.p[k] = params_host[k], al &= sd_aligned(params_host[k]);
    const SdGeo g = sd_geo(D, U, U % 4 == 0 && al ? 4 : 1);
    const dim3 grid((unsigned)(B < 16384 ? B : 16384));
    rc = sd_dispatch<SdFwd>(K, g.vec, mode == RECNOW_STAR_MUL, grid, (hipStream_t)stream, x, P, weight, kernel, bias, B, D, U, g.tu_bits, g.nj,
                            act, y);
    if (rc) return rc;
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_star_dense_bwd(const float* x, const float* const* params_host, int K, int mode, float weight, const float* kernel,
                                     const float* y, const float* dy, int64_t B, int D, int U, int act, float* dx,
                                     float* const* dparams_host, float* dkernel, float* dbias, void* ws, size_t ws_bytes, void* stream) {
    int rc = sd_check(x, params_host, K, mode, kernel, B, D, U, act);
    if (rc) return rc;
    if (!y || !dy) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t R = (size_t)D * U + U;
    if (B == 0) {            // empty batch: the parameter gradients are sums over no rows
        if (dkernel) RN_HIP(hipMemsetAsync(dkernel, 0, (size_t)D * U * sizeof(float), st));
        if (dbias) RN_HIP(hipMemsetAsync(dbias, 0, (size_t)U * sizeof(float), st));
        return RECNOW_OK;
    }
    const bool need_part = dkernel || dbias;
    if (need_part && (!ws || ws_bytes < recnow_star_dense_workspace_bytes(B, D, U))) return RECNOW_EWORKSPACE;
    SdPtrs P = {};
    bool al = sd_aligned(kernel), any = dx || need_part;
    for (int k = 0; k < K; ++k) {
        P.p[k] = params_host[k];
        P.dp[k] = dparams_host ? dparams_host[k] : nullptr;
        al &= sd_aligned(P.p[k]) && sd_aligned(P.dp[k]);
        any |= P.dp[k] != nullptr;
    }
    if (!any) return RECNOW_OK;
    const SdGeo g = sd_geo(D, U, U % 4 == 0 && al ? 4 : 1);
    int nchunk;
    int64_t rows;
    sd_chunks(B, D, U, &nchunk, &rows);
    float* part = need_part ? (float*)ws : nullptr;
    rc = sd_dispatch<SdBwd>(K, g.vec, mode == RECNOW_STAR_MUL, dim3((unsigned)g.ndt, (unsigned)nchunk), st, x, P, weight, kernel, y, dy, B, D,
                            U, g.tu_bits, g.nj, act, rows, dx, part);
    if (rc) return rc;
    RN_LAUNCH_CHECK();
    if (need_part) {
        const int64_t blocks = ((int64_t)R + SD_THREADS - 1) / SD_THREADS;
        hipLaunchKernelGGL(k_sd_reduce, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), SD_THREADS, 0, st, part, nchunk, (int64_t)D * U, U,
                           dkernel, dbias);
        RN_LAUNCH_CHECK();
    }
    return RECNOW_OK;
}
