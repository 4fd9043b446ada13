// attention_by_dnn (DIN attention unit), reference rec_now/rec_block/attention.py:41-82:
//   x[b,l] = [user[b,l] | doc[b]],  logit = Dense_n(...act(Dense_1(x))),  s = sigmoid(logit)
//   mat[b] = sum_l s[b,l] user[b,l],  score_sum[b] = sum_l s[b,l]
// The reference tiles doc to (B, L, D), concatenates a (B, L, 2D) input and keeps every (B, L, H_i) activation in HBM.  Here:
//   * layer 1 is split: q[b] = doc[b] . W1[D:2D] + b1 is formed once per batch row (a "group" of G <= 32 rows at a time), the
//     positions only contract user[b,l] . W1[0:D];
//   * a workgroup (4 waves) walks the G*L flattened positions of its group in tiles of 32 (a tile may end inside a row, a row with
//     L > 32 spans several tiles); every Dense of the tile runs on v_mfma_f32_32x32x2_f32 (exact fp32) with the activations in LDS;
//   * the last Dense(1) is a row dot, the sigmoid and the sums over l follow in the tile epilogue.  Nothing of size B*L*H is stored.
// Weights stay in global memory (L2-resident, a few hundred KiB at most) and are read as MFMA B fragments; LDS holds the tile's
// activations only (sum over layers of 32 x width floats, <= 129 KiB at D = 256 with three hidden layers of 256).
// Backward recomputes the tile's forward, then walks the layers back with dZ_i written over H_i in place.  Per-b quantities (q, the
// sum over l of dz1) and the weight-gradient partials live in the workgroup's own slab of the workspace; k_din_reduce sums the slabs
// in workgroup order.  No float atomics: the gradients are bit-identical from run to run.  Design notes and numbers: DESIGN.md 8e.
#include "common.hpp"

typedef float dn_f16v __attribute__((ext_vector_type(16)));

#define DN_THREADS 256
#define DN_WAVES 4
#define DN_TM 32             // positions per tile = rows of one MFMA block
#define DN_MAXL 4            // Dense layers (at most 3 hidden + the final Dense(1))
#define DN_MAXW 256          // D and every Dense width
#define DN_GROUPS_FWD 2048   // G shrinks (32 -> 1) until B / G reaches this many groups (forward: ~18 KiB of LDS, 8 workgroups per CU)
#define DN_GROUPS_BWD 1024   // backward: fewer, longer groups (each ends with the doc-side products)
#define DN_MAX_WG_FWD 2048   // workgroups: 8 per CU
#define DN_MAX_WG_BWD 768    // 3 per CU (the backward's registers)
#define DN_WS_BUDGET (256ll << 20)   // backward slabs are capped near this many bytes in total (bounded, independent of B and L)

struct DnArgs {
    const float* user;
    const float* doc;
    const float* W[DN_MAXL];       // W[0]: (2D, w1) [user rows | doc rows], W[i]: (w[i], w[i+1]), row-major (Keras (in, out))
    const float* bias[DN_MAXL];
    int w[DN_MAXL + 1];            // w[0] = D, w[i] = dims[i-1]; w[nl] = 1
    int act, L, D, G;
    int64_t B, ngroups;
    float* mat;
    float* ssum;
    const float* dmat;
    const float* dsum;
    float* duser;
    float* ddoc;
    float* ws;
    int64_t slab;                  // floats per workgroup: Q (32 w1) | S (32 w1, backward) | parameter-gradient partials
    int64_t koff[DN_MAXL], boff[DN_MAXL];   // offsets of kernel i / bias i inside the partials
};

// C[M][N] = sum_k A[m][k] B[k][n] over 32 x 32 output blocks, dealt round-robin to the 4 waves; A(m, k) = A[m*am + k*ak],
// B(k, n) = B[k*bk + n*bn].  Out-of-range m / n / k contribute exact zeros (the index is clamped, the value selected away), so
// odd K and widths that are not multiples of 32 need no padding.  epi(m, n, value) for every in-range output element.
template <class Epi>
__device__ __forceinline__ void dn_mm(const float* A, int am, int ak, const float* Bm, int bk, int bn, int M, int N, int K, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int nb = (N + 31) >> 5, nblk = ((M + 31) >> 5) * nb;
    for (int blk = wave; blk < nblk; blk += DN_WAVES) {
        const int m0 = blk / nb * 32, n0 = blk % nb * 32;
        const bool mok = m0 + li < M, nok = n0 + li < N;
        const float* ap = A + (mok ? m0 + li : 0) * am;
        const float* bp = Bm + (nok ? n0 + li : 0) * bn;
        dn_f16v acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < K; k0 += 8) {
            float av[4], bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = k0 + 2 * s + lh;
                const bool kok = k < K;
                const int kc = kok ? k : 0;
                const float x = ap[kc * ak], y = bp[kc * bk];
                av[s] = mok && kok ? x : 0.f;
                bv[s] = nok && kok ? y : 0.f;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
        }
        // accumulator register r of lane (li, lh): row 8 (r / 4) + 4 lh + r % 4, column li
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 8 * (r >> 2) + 4 * lh + (r & 3), n = n0 + li;
            if (m < M && n < N) epi(m, n, acc[r]);
        }
    }
}

__device__ __forceinline__ int dn_ld(int w) { return w | 1; }     // odd row strides: the per-row A-fragment reads spread over the banks

// One launch per direction.  NH = number of hidden layers (Dense layers - 1).
template <int NH, bool BWD>
__global__ void __launch_bounds__(DN_THREADS) k_din(DnArgs a) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, D = a.D, L = a.L, w1 = a.w[1], act = a.act;
    float* H[NH + 1];              // H[0] = the user tile, H[i] = the tile's output of hidden layer i (dZ_i in the backward)
    int ld[NH + 1];
    float* p = sm;
#pragma unroll
    for (int i = 0; i <= NH; ++i) ld[i] = dn_ld(a.w[i]), H[i] = p, p += DN_TM * ld[i];
    float* s_s = p;
    float* s_gz = p + DN_TM;
    int* s_rb = (int*)(p + 2 * DN_TM);      // batch row of tile row r, relative to the group (0 for rows past the end)
    int* s_rl = s_rb + DN_TM;               // position l of tile row r inside its batch row
    int* s_ok = s_rl + DN_TM;
    float* slab = a.ws + (int64_t)blockIdx.x * a.slab;
    float* Q = slab;                        // (G, w1): doc[b] . W1[D:2D] + b1
    float* S = slab + DN_TM * w1;           // (G, w1): sum over l of dz1 (backward)
    float* part = S + DN_TM * w1;
    const float* W1d = a.W[0] + (int64_t)D * w1;
    const float* wl = a.W[NH];              // final Dense(1): a column (stride 1); W1[0:D] when NH = 0
    if (BWD)
        for (int64_t i = tid; i < a.slab - 2 * DN_TM * w1; i += DN_THREADS) part[i] = 0.f;

    for (int64_t grp = blockIdx.x; grp < a.ngroups; grp += gridDim.x) {
        const int64_t g0 = grp * a.G;
        const int gn = (int)(a.B - g0 < a.G ? a.B - g0 : a.G);
        // ---- group prologue: Q = doc . W1[D:2D] + b1 (the doc rows staged in the user tile's LDS)
        for (int i = tid; i < DN_TM * D; i += DN_THREADS) {
            const int g = i / D, c = i - g * D;
            H[0][g * ld[0] + c] = g < gn ? a.doc[(g0 + g) * D + c] : 0.f;
        }
        if (BWD)
            for (int i = tid; i < DN_TM * w1; i += DN_THREADS) S[i] = 0.f;
        __syncthreads();
        {
            const float* b1 = a.bias[0];
            dn_mm(H[0], ld[0], 1, W1d, w1, 1, gn, w1, D, [&](int m, int n, float v) { Q[m * w1 + n] = v + b1[n]; });
        }
        __syncthreads();
        const int64_t pbeg = g0 * L, pend = (g0 + gn) * L;
        for (int64_t t0 = pbeg; t0 < pend; t0 += DN_TM) {
            // ---- forward of the tile (recomputed in the backward)
            if (tid < DN_TM) {
                const int64_t f = t0 + tid;
                const bool ok = f < pend;
                const int64_t b = ok ? f / L : g0;
                s_rb[tid] = (int)(b - g0);
                s_rl[tid] = (int)(f - b * L);
                s_ok[tid] = ok;
            }
            {
                const int64_t nvalid = (pend - t0 < DN_TM ? pend - t0 : DN_TM) * D;
                const float* ub = a.user + t0 * D;          // the tile's rows are one contiguous range of user
                for (int i = tid; i < DN_TM * D; i += DN_THREADS) {
                    const int r = i / D, c = i - r * D;
                    H[0][r * ld[0] + c] = i < nvalid ? ub[i] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 1; i <= NH; ++i) {
                float* out = H[i];
                const int ldo = ld[i], wi = a.w[i];
                const float* bi = a.bias[i - 1];
                const float* Wi = a.W[i - 1];          // W[0]: its first D rows (the user part)
                if (i == 1)
                    dn_mm(H[0], ld[0], 1, Wi, wi, 1, DN_TM, wi, D, [&](int m, int n, float v) {
                        out[m * ldo + n] = rn_act(v + Q[s_rb[m] * w1 + n], act);
                    });
                else
                    dn_mm(H[i - 1], ld[i - 1], 1, Wi, wi, 1, DN_TM, wi, a.w[i - 1], [&](int m, int n, float v) {
                        out[m * ldo + n] = rn_act(v + bi[n], act);
                    });
                __syncthreads();
            }
            {   // final Dense(1) as a row dot: 8 lanes per row, fixed reduction order
                const int r = tid >> 3, j = tid & 7, wx = a.w[NH];
                const float* x = H[NH] + r * ld[NH];
                float z = 0.f, gd = 0.f;
                for (int k = j; k < wx; k += 8) z = fmaf(x[k], wl[k], z);
                const bool ok = s_ok[r];
                const int64_t b = g0 + s_rb[r];
                if (BWD && a.dmat)
                    for (int k = j; k < D; k += 8) gd = fmaf(a.dmat[b * D + k], H[0][r * ld[0] + k], gd);
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) {
                    z += __shfl_xor(z, o, 64);
                    if (BWD) gd += __shfl_xor(gd, o, 64);
                }
                const float logit = z + (NH == 0 ? Q[s_rb[r]] : a.bias[NH][0]);
                const float s = ok ? rn_sigmoid(logit) : 0.f;
                if (j == 0) {
                    s_s[r] = s;
                    if (BWD) s_gz[r] = ok ? (gd + (a.dsum ? a.dsum[b] : 0.f)) * s * (1.f - s) : 0.f;
                }
            }
            __syncthreads();
            if (!BWD) {
                // mat[b] += sum over the tile's rows of b of s * user;  column D carries score_sum.  A row's first tile stores.
                for (int c = tid; c <= D; c += DN_THREADS) {
                    float acc = 0.f;
                    int cur = -1;
                    bool first = false;
                    auto flush = [&]() {
                        const int64_t b = g0 + cur;
                        float* dst = c < D ? a.mat + b * D + c : a.ssum + b;
                        *dst = first ? acc : *dst + acc;
                    };
                    for (int r = 0; r < DN_TM && s_ok[r]; ++r) {
                        if (s_rb[r] != cur) {
                            if (cur >= 0) flush();
                            cur = s_rb[r], first = s_rl[r] == 0, acc = 0.f;
                        }
                        acc = fmaf(s_s[r], c < D ? H[0][r * ld[0] + c] : 1.f, acc);
                    }
                    if (cur >= 0) flush();
                }
                __syncthreads();
                continue;
            }
            // ---- backward of the tile.  Final layer: dW_last += X^T gz, db_last += sum gz (NH = 0: into S, the bias is b1)
            {
                const int wx = a.w[NH];
                float* X = H[NH];
                for (int k = tid; k < wx; k += DN_THREADS) {
                    float acc = 0.f;
                    for (int r = 0; r < DN_TM; ++r) acc = fmaf(X[r * ld[NH] + k], s_gz[r], acc);
                    part[a.koff[NH] + k] += acc;
                }
                if (NH > 0 && tid == DN_THREADS - 1) {
                    float acc = 0.f;
                    for (int r = 0; r < DN_TM; ++r) acc += s_gz[r];
                    part[a.boff[NH]] += acc;
                }
                if (NH == 0) {
                    if (tid == 0) {            // S[b] += sum over the tile's rows of b of gz
                        float acc = 0.f;
                        int cur = -1;
                        for (int r = 0; r < DN_TM && s_ok[r]; ++r) {
                            if (s_rb[r] != cur) {
                                if (cur >= 0) S[cur] += acc;
                                cur = s_rb[r], acc = 0.f;
                            }
                            acc += s_gz[r];
                        }
                        if (cur >= 0) S[cur] += acc;
                    }
                    for (int i = tid; i < DN_TM * D; i += DN_THREADS) {
                        const int r = i / D, c = i - r * D;
                        if (!s_ok[r]) continue;
                        const int64_t b = g0 + s_rb[r];
                        a.duser[(t0 + r) * D + c] = (a.dmat ? s_s[r] * a.dmat[b * D + c] : 0.f) + s_gz[r] * wl[c];
                    }
                }
                __syncthreads();
                if (NH > 0) {                  // dZ_NH = gz wl^T * act'(H_NH), in place
                    for (int i = tid; i < DN_TM * wx; i += DN_THREADS) {
                        const int r = i / wx, k = i - r * wx;
                        float* h = X + r * ld[NH] + k;
                        *h = s_gz[r] * wl[k] * rn_act_grad_from_out(*h, act);
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int i = NH; i >= 1; --i) {
                const int wi = a.w[i], wp = a.w[i - 1];
                const float* dZ = H[i];
                const int ldz = ld[i];
                float* pk = part + a.koff[i - 1];     // i = 1: rows 0..D-1 of W1 (the user part)
                // dW_i += H_{i-1}^T dZ_i  (contraction over the 32 positions; rows past the end have dZ = 0)
                dn_mm(H[i - 1], 1, ld[i - 1], dZ, ldz, 1, wp, wi, DN_TM, [&](int m, int n, float v) { pk[m * wi + n] += v; });
                if (i > 1) {
                    float* pb = part + a.boff[i - 1];
                    for (int n = tid; n < wi; n += DN_THREADS) {
                        float acc = 0.f;
                        for (int r = 0; r < DN_TM; ++r) acc += dZ[r * ldz + n];
                        pb[n] += acc;
                    }
                    __syncthreads();
                    // dZ_{i-1} = (dZ_i W_i^T) * act'(H_{i-1}), over H_{i-1} in place
                    float* hp = H[i - 1];
                    const int ldp = ld[i - 1];
                    dn_mm(dZ, ldz, 1, a.W[i - 1], 1, wi, DN_TM, wp, wi, [&](int m, int n, float v) {
                        float* h = hp + m * ldp + n;
                        *h = v * rn_act_grad_from_out(*h, act);
                    });
                    __syncthreads();
                } else {
                    // S[b] += sum over the tile's rows of b of dz1 (per column, rows in order)
                    for (int n = tid; n < w1; n += DN_THREADS) {
                        float acc = 0.f;
                        int cur = -1;
                        for (int r = 0; r < DN_TM && s_ok[r]; ++r) {
                            if (s_rb[r] != cur) {
                                if (cur >= 0) S[cur * w1 + n] += acc;
                                cur = s_rb[r], acc = 0.f;
                            }
                            acc += dZ[r * ldz + n];
                        }
                        if (cur >= 0) S[cur * w1 + n] += acc;
                    }
                    // duser = s dmat[b] + dz1 W1[0:D]^T, written once
                    dn_mm(dZ, ldz, 1, a.W[0], 1, w1, DN_TM, D, w1, [&](int m, int n, float v) {
                        if (s_ok[m]) {
                            const int64_t b = g0 + s_rb[m];
                            a.duser[(t0 + m) * D + n] = v + (a.dmat ? s_s[m] * a.dmat[b * D + n] : 0.f);
                        }
                    });
                    __syncthreads();
                }
            }
        }
        if (!BWD) continue;
        // ---- group epilogue: db1 += sum_b S[b];  dW1[D:2D] += doc^T S;  ddoc = S W1[D:2D]^T
        for (int n = tid; n < w1; n += DN_THREADS) {
            float acc = 0.f;
            for (int g = 0; g < gn; ++g) acc += S[g * w1 + n];
            part[a.boff[0] + n] += acc;
        }
        for (int i = tid; i < DN_TM * D; i += DN_THREADS) {
            const int g = i / D, c = i - g * D;
            H[0][g * ld[0] + c] = g < gn ? a.doc[(g0 + g) * D + c] : 0.f;
        }
        __syncthreads();
        {
            float* pk = part + a.koff[0] + (int64_t)D * w1;
            dn_mm(H[0], 1, ld[0], S, w1, 1, D, w1, gn, [&](int m, int n, float v) { pk[m * w1 + n] += v; });
            if (a.ddoc) dn_mm(S, w1, 1, W1d, 1, w1, gn, D, w1, [&](int m, int n, float v) { a.ddoc[(g0 + m) * D + n] = v; });
        }
        __syncthreads();
    }
}

// Parameter gradients: dst segment j (kernel i = j / 2, bias i when j is odd) = sum over the workgroup slabs, in workgroup order.
struct DnRed {
    float* dst[2 * DN_MAXL];
    int64_t off[2 * DN_MAXL + 1];
};

__global__ void __launch_bounds__(DN_THREADS)
k_din_reduce(const float* __restrict__ ws, int64_t slab, int64_t pbase, int nwg, DnRed r) {
    const int64_t n = r.off[2 * DN_MAXL];
    for (int64_t i = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * DN_THREADS) {
        float s = 0.f;
        for (int w = 0; w < nwg; ++w) s += ws[w * slab + pbase + i];
        float* d = nullptr;
        int64_t o = 0;
#pragma unroll
        for (int j = 0; j < 2 * DN_MAXL; ++j)
            if (i >= r.off[j] && i < r.off[j + 1]) d = r.dst[j], o = r.off[j];
        if (d) d[i - o] = s;
    }
}

namespace {
struct DnPlan {
    int G, grid;
    int64_t ngroups, slab_fwd, slab_bwd, nparam;
    int64_t koff[DN_MAXL], boff[DN_MAXL];
    size_t lds;
};

int dn_check(int64_t B, int L, int D, int nl, const int* dims, int act) {
    if (B < 0 || L < 0 || D < 1 || nl < 1 || !dims || act < RECNOW_ACT_LINEAR || act > RECNOW_ACT_SIGMOID) return RECNOW_EINVAL;
    if (dims[nl - 1] != 1) return RECNOW_EINVAL;
    for (int i = 0; i < nl; ++i)
        if (dims[i] < 1) return RECNOW_EINVAL;
    if (nl > DN_MAXL || D > DN_MAXW) return RECNOW_EUNSUPPORTED;
    for (int i = 0; i < nl; ++i)
        if (dims[i] > DN_MAXW) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}

// A function of the shape alone, so the workspace query needs no pointers.
DnPlan dn_plan(int64_t B, int L, int D, int nl, const int* dims, bool bwd) {
    DnPlan p = {};
    p.G = DN_TM;
    while (p.G > 1 && (B + p.G - 1) / p.G < (bwd ? DN_GROUPS_BWD : DN_GROUPS_FWD)) p.G >>= 1;
    p.ngroups = (B + p.G - 1) / p.G;
    int64_t o = 0, in = 2 * (int64_t)D;
    for (int i = 0; i < nl; ++i) {
        p.koff[i] = o, o += in * dims[i];
        p.boff[i] = o, o += dims[i];
        in = dims[i];
    }
    p.nparam = o;
    p.slab_fwd = DN_TM * (int64_t)dims[0];
    p.slab_bwd = (int64_t)rn_align((size_t)(2 * p.slab_fwd + p.nparam), 64);
    int64_t cap = bwd ? DN_WS_BUDGET / (p.slab_bwd * 4) : DN_MAX_WG_FWD;
    if (cap > (bwd ? DN_MAX_WG_BWD : DN_MAX_WG_FWD)) cap = bwd ? DN_MAX_WG_BWD : DN_MAX_WG_FWD;
    if (cap < 64) cap = 64;
    p.grid = (int)(p.ngroups < cap ? p.ngroups : cap);
    p.lds = 5 * DN_TM * sizeof(float);
    int w = D;
    for (int i = 0; i < nl; ++i) {
        p.lds += (size_t)DN_TM * (w | 1) * sizeof(float);
        w = dims[i];
    }
    return p;
}

template <int NH, bool BWD>
int dn_launch(const DnArgs& a, const DnPlan& p, hipStream_t st) {
    RN_HIP(rn_lds_grant((const void*)k_din<NH, BWD>, 160 * 1024));        // the input tile of every layer stays in LDS: above 64 KiB from D = 256 on
    hipLaunchKernelGGL((k_din<NH, BWD>), dim3((unsigned)p.grid), DN_THREADS, p.lds, st, a);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

template <bool BWD>
int dn_dispatch(const DnArgs& a, const DnPlan& p, int nl, hipStream_t st) {
    switch (nl) {
        case 1: return dn_launch<0, BWD>(a, p, st);
        case 2: return dn_launch<1, BWD>(a, p, st);
        case 3: return dn_launch<2, BWD>(a, p, st);
        case 4: return dn_launch<3, BWD>(a, p, st);
    }
    return RECNOW_EUNSUPPORTED;
}

int dn_args(DnArgs* a, const DnPlan& p, const float* user, const float* doc, int64_t B, int L, int D, int nl, const int* dims,
            const float* const* kernels_host, const float* const* biases_host, int act, void* ws) {
    if (!user || !doc || !kernels_host || !biases_host) return RECNOW_EINVAL;
    *a = DnArgs{};
    a->user = user, a->doc = doc;
    a->w[0] = D;
    for (int i = 0; i < nl; ++i) {
        if (!kernels_host[i] || !biases_host[i]) return RECNOW_EINVAL;
        a->W[i] = kernels_host[i], a->bias[i] = biases_host[i], a->w[i + 1] = dims[i];
        a->koff[i] = p.koff[i], a->boff[i] = p.boff[i];
    }
    a->act = act, a->L = L, a->D = D, a->G = p.G, a->B = B, a->ngroups = p.ngroups;
    a->ws = (float*)ws;
    return RECNOW_OK;
}
}  // namespace

extern "C" size_t recnow_attention_dnn_workspace_bytes(int64_t B, int L, int D, int nl, const int* dims_host, int backward) {
    if (dn_check(B, L, D, nl, dims_host, RECNOW_ACT_LINEAR) || B == 0 || L == 0) return 0;
    const DnPlan p = dn_plan(B, L, D, nl, dims_host, backward != 0);
    return rn_align((size_t)p.grid * (backward ? p.slab_bwd : p.slab_fwd) * sizeof(float));
}

extern "C" int recnow_attention_dnn_fwd(const float* user, const float* doc, int64_t B, int L, int D, int nl, const int* dims_host,
                                        const float* const* kernels_host, const float* const* biases_host, int act, float* mat,
                                        float* score_sum, void* ws, size_t ws_bytes, void* stream) {
    int rc = dn_check(B, L, D, nl, dims_host, act);
    if (rc) return rc;
    if (B == 0) return RECNOW_OK;
    if (!mat || !score_sum) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (L == 0) {                      // sums over no positions
        RN_HIP(hipMemsetAsync(mat, 0, (size_t)B * D * sizeof(float), st));
        RN_HIP(hipMemsetAsync(score_sum, 0, (size_t)B * sizeof(float), st));
        return RECNOW_OK;
    }
    if (!ws || ws_bytes < recnow_attention_dnn_workspace_bytes(B, L, D, nl, dims_host, 0)) return RECNOW_EWORKSPACE;
    const DnPlan p = dn_plan(B, L, D, nl, dims_host, false);
    DnArgs a;
    rc = dn_args(&a, p, user, doc, B, L, D, nl, dims_host, kernels_host, biases_host, act, ws);
    if (rc) return rc;
    a.mat = mat, a.ssum = score_sum, a.slab = p.slab_fwd;
    return dn_dispatch<false>(a, p, nl, st);
}

extern "C" int recnow_attention_dnn_bwd(const float* user, const float* doc, int64_t B, int L, int D, int nl, const int* dims_host,
                                        const float* const* kernels_host, const float* const* biases_host, int act, const float* dmat,
                                        const float* dsum, float* duser, float* ddoc, float* const* dkernels_host,
                                        float* const* dbiases_host, void* ws, size_t ws_bytes, void* stream) {
    int rc = dn_check(B, L, D, nl, dims_host, act);
    if (rc) return rc;
    if ((B > 0 && L > 0 && !duser) || (B > 0 && !ddoc)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const DnPlan p = dn_plan(B, L, D, nl, dims_host, true);
    if (B == 0 || L == 0) {            // sums over no positions: every gradient but the (empty) duser is zero
        if (B > 0) RN_HIP(hipMemsetAsync(ddoc, 0, (size_t)B * D * sizeof(float), st));
        int in = 2 * D;
        for (int i = 0; i < nl; ++i) {
            if (dkernels_host && dkernels_host[i]) RN_HIP(hipMemsetAsync(dkernels_host[i], 0, (size_t)in * dims_host[i] * sizeof(float), st));
            if (dbiases_host && dbiases_host[i]) RN_HIP(hipMemsetAsync(dbiases_host[i], 0, (size_t)dims_host[i] * sizeof(float), st));
            in = dims_host[i];
        }
        return RECNOW_OK;
    }
    if (!ws || ws_bytes < recnow_attention_dnn_workspace_bytes(B, L, D, nl, dims_host, 1)) return RECNOW_EWORKSPACE;
    DnArgs a;
    rc = dn_args(&a, p, user, doc, B, L, D, nl, dims_host, kernels_host, biases_host, act, ws);
    if (rc) return rc;
    a.dmat = dmat, a.dsum = dsum, a.duser = duser, a.ddoc = ddoc, a.slab = p.slab_bwd;
    rc = dn_dispatch<true>(a, p, nl, st);
    if (rc) return rc;
    DnRed r = {};
    for (int i = 0; i < nl; ++i) {
        r.dst[2 * i] = dkernels_host ? dkernels_host[i] : nullptr;
        r.dst[2 * i + 1] = dbiases_host ? dbiases_host[i] : nullptr;
        r.off[2 * i] = p.koff[i], r.off[2 * i + 1] = p.boff[i];
    }
    for (int j = 2 * nl; j <= 2 * DN_MAXL; ++j) r.off[j] = p.nparam;
    const int64_t blocks = (p.nparam + DN_THREADS - 1) / DN_THREADS;
    hipLaunchKernelGGL(k_din_reduce, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), DN_THREADS, 0, st, (const float*)ws, p.slab_bwd,
                       2 * p.slab_fwd, p.grid, r);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
