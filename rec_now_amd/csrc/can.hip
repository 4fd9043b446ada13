// CANLayer (co-action network), reference rec_now/layers/can_layer.py:228-275: every sample b applies its OWN small MLP, whose kernels
// and biases are the sample's row of params (B, P), to each of its L input rows x[b][l] (D0), masks the rows that are all zero and
// (optionally) combines the L results.  The reference runs one broadcast batched matmul per layer on a (B, 1, din, dout) view and keeps
// a (B, L, 1, D_k) activation per layer; here one workgroup owns one sample: its P floats are copied into LDS once, its positions walk
// the whole layer chain on-chip, and y is written once.  Both directions are meant to be bound by reading x and params once.
//
// Geometry (one 256-thread workgroup = 4 waves): a position is worked by a group of G = 16, 32 or 64 consecutive lanes (the smallest
// that covers the widest layer, D0 included), lane j of the group forming column j of every layer; a wave holds 64 / G positions,
// the workgroup C = 256 / G positions per pass: slot s = thread / G takes position pass * C + s.  Each slot has a row in LDS
// that holds the layer inputs h_0 .. h_{n-1} (and, backward, dz_1 .. dz_n), so a lane reads the other columns of its position from
// there.  The arithmetic of a position depends on nothing but its input row and the sample's parameters: not on l, not on the slot.
//   forward:  the combiner runs inside the launch in a fixed order: every slot over its positions, then the slots of a wave in slot
//             order, then the waves in wave order (through LDS).
//   backward: RECOMPUTES the chain of every position (act(z) itself, also under res_net), then walks it back.  The C positions of a pass
//             are the backward's chunk: their h_{k-1} and dz_k rows stay in LDS, and thread t, which owns the entries t, t + 256, ... of
//             the sample's dparams row in registers, adds h_{k-1}[l][r] dz_k[l][c] over the chunk in position order.  max / min
//             take a counting pass first (positions whose output equals y), then share g / count among them.
// No atomics, no workspace: every element of y, dx and dparams is written once, and the same input gives the same bits on every run.
// Every thread reaches every barrier: the pass and layer loops have workgroup-uniform trip counts.
#include "common.hpp"
#include <limits.h>
#include <math.h>

#define CAN_THREADS 256
#define CAN_WAVES (CAN_THREADS / RN_WAVE)
#define CAN_MIN_GROUP 16        // lanes per position at widths <= 16: CAN_THREADS / CAN_MIN_GROUP positions per pass and per backward chunk
#define CAN_MAX_DIM 64          // = the widest lane group, one wave
#define CAN_MAX_LAYERS 8
#define CAN_LDS_BYTES 65536     // most LDS one workgroup asks for: two workgroups fit a CU's 160 KiB

struct CanPlan {
    int n, P, ldsW;                         // layers; floats of one parameter row; its LDS image (P rounded up to 4)
    int gbits, C, SS;                       // log2 G; positions per pass; floats of one slot row
    int act, use_bias, res, last_act, mask, comb;
    int dims[CAN_MAX_LAYERS + 1];           // D0, D1 .. Dn
    int woff[CAN_MAX_LAYERS];               // kernel k in the parameter row
    int boff[CAN_MAX_LAYERS];               // bias k in the parameter row
    int hoff[CAN_MAX_LAYERS];               // h_k (the input of layer k) in the slot row
    int zoff[CAN_MAX_LAYERS];               // dz of layer k in the slot row (backward only)
};

__device__ __forceinline__ float can_comb_init(int comb) {
    return comb == RECNOW_REDUCE_MAX ? -INFINITY : comb == RECNOW_REDUCE_MIN ? INFINITY : 0.f;
}
__device__ __forceinline__ float can_comb(float a, float v, int comb) {
    if (comb == RECNOW_REDUCE_MAX) return v > a ? v : a;
    if (comb == RECNOW_REDUCE_MIN) return v < a ? v : a;
    return a + v;
}

// the sample's parameter row -> LDS, every float read once
__device__ __forceinline__ void can_load_params(const float* __restrict__ src, float* Wl, int P, int vec4) {
    if (vec4) {
        for (int e = threadIdx.x * 4; e < P; e += CAN_THREADS * 4) *(rn_f4*)(Wl + e) = RN_LD_STREAM((rn_gcf4)(src + e));
    } else {
        for (int e = threadIdx.x; e < P; e += CAN_THREADS) Wl[e] = RN_LD_STREAM((rn_gcf)(src + e));
    }
}

// x[b][l] -> h_0 of the slot row (zeros for a position past L); returns whether the row has a non-zero (-0.0 counts as zero)
__device__ __forceinline__ bool can_load_x(const CanPlan& p, const float* __restrict__ xrow, bool valid, float* row, int j) {
    const int D0 = p.dims[0];
    float xv = 0.f;
    if (valid && j < D0) xv = RN_LD_STREAM((rn_gcf)(xrow + j));
    if (j < D0) row[j] = xv;
    const unsigned long long bal = __ballot(xv != 0.f);
    const int lane = threadIdx.x & (RN_WAVE - 1), G = 1 << p.gbits;
    const unsigned long long gm = G == RN_WAVE ? ~0ull : (1ull << G) - 1ull;
    return ((bal >> (lane & ~(G - 1))) & gm) != 0ull;
}

// The layer chain of one position; lane j returns column j of h_n (lanes past D_n: a clamped copy).  h_0 must be in the slot row behind a
// barrier.  BWD: also leaves act'(z_k)[j] (1 on a layer without activation) where dz_k[j] will go.  Ends behind a barrier.
template <bool BWD>
__device__ __forceinline__ float can_chain(const CanPlan& p, const float* Wl, float* row, int j) {
    float a = 0.f;
    for (int k = 0; k < p.n; ++k) {
        const int din = p.dims[k], dout = p.dims[k + 1];
        const int jc = j < dout ? j : dout - 1;
        const float* W = Wl + p.woff[k] + jc;
        const float* hin = row + p.hoff[k];
        float z = p.use_bias ? Wl[p.boff[k] + jc] : 0.f;
        for (int i = 0; i < din; ++i) z = fmaf(hin[i], W[i * dout], z);
        const bool has_act = k + 1 < p.n || p.last_act;
        a = has_act ? rn_act(z, p.act) : z;
        const float ag = has_act ? rn_act_grad_from_out(a, p.act) : 1.f;
        if (p.res) a += hin[jc];                          // din == dout
        if (j < dout) {
            if (k + 1 < p.n) row[p.hoff[k + 1] + j] = a;
            if (BWD) row[p.zoff[k] + j] = ag;
        }
        __syncthreads();
    }
    return a;
}

// LDS: [ parameter row: ldsW ][ slot rows: C x SS ][ red: C x 64 ][ cnt: 64 ]
__global__ void __launch_bounds__(CAN_THREADS)
k_can_fwd(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ y, int64_t B, int L, CanPlan p, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float can_lds[];
    float* Wl = can_lds;
    float* rows = can_lds + p.ldsW;
    float* red = rows + p.C * p.SS;
    const int t = threadIdx.x, G = 1 << p.gbits, j = t & (G - 1), s = t >> p.gbits;
    float* row = rows + s * p.SS;
    const int D0 = p.dims[0], Dn = p.dims[p.n];
    const int npass = (L + p.C - 1) / p.C;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        can_load_params(params + b * p.P, Wl, p.P, vec4);
        float acc = can_comb_init(p.comb);
        for (int pass = 0; pass < npass; ++pass) {
            const int l = pass * p.C + s;
            const bool valid = l < L;
            const int64_t pos = b * L + (valid ? l : 0);
            const bool nz = can_load_x(p, x + pos * D0, valid, row, j);
            __syncthreads();
            float o = can_chain<false>(p, Wl, row, j);
            if (p.mask && !nz) o = 0.f;
            if (valid && j < Dn) {
                if (p.comb < 0)
                    RN_ST_STREAM((rn_gf)(y + pos * Dn + j), o);
                else
                    acc = can_comb(acc, o, p.comb);
            }
        }
        if (p.comb >= 0) {
            red[s * CAN_MAX_DIM + j] = acc;
            __syncthreads();
            if (t < Dn) {
                const int ng = RN_WAVE >> p.gbits;
                float r = can_comb_init(p.comb);
                for (int w = 0; w < CAN_WAVES; ++w) {
                    float pw = can_comb_init(p.comb);
                    for (int g = 0; g < ng; ++g) pw = can_comb(pw, red[(w * ng + g) * CAN_MAX_DIM + t], p.comb);
                    r = can_comb(r, pw, p.comb);
                }
                if (p.comb == RECNOW_REDUCE_MEAN) r /= (float)L;
                y[b * Dn + t] = r;
            }
        }
        __syncthreads();               // the next sample overwrites the parameter row and red
    }
}

// NE: dparams entries per thread (entry e = t + i * 256)
template <int NE>
__global__ void __launch_bounds__(CAN_THREADS)
k_can_bwd(const float* __restrict__ x, const float* __restrict__ params, const float* __restrict__ g, const float* __restrict__ y, int64_t B,
          int L, CanPlan p, int vec4, float* __restrict__ dx, float* __restrict__ dparams) {
    extern __shared__ __attribute__((aligned(16))) float can_lds[];
    float* Wl = can_lds;
    float* rows = can_lds + p.ldsW;
    float* red = rows + p.C * p.SS;
    float* cnt = red + p.C * CAN_MAX_DIM;
    const int t = threadIdx.x, G = 1 << p.gbits, j = t & (G - 1), s = t >> p.gbits;
    float* row = rows + s * p.SS;
    const int D0 = p.dims[0], Dn = p.dims[p.n];
    const int npass = (L + p.C - 1) / p.C;
    const bool extremum = p.comb == RECNOW_REDUCE_MAX || p.comb == RECNOW_REDUCE_MIN;

    // where entry e of the parameter row finds its two factors in a slot row: h_{k-1}[r] | dz_k[c] << 16; a bias entry has no h (0xffff)
    int ofs[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int e = t + i * CAN_THREADS;
        ofs[i] = -1;
        if (dparams && e < p.P) {
            for (int k = 0; k < p.n; ++k) {
                const int dout = p.dims[k + 1], w = e - p.woff[k], nw = p.dims[k] * dout;
                if (w >= 0 && w < nw) ofs[i] = (p.hoff[k] + w / dout) | (p.zoff[k] + w % dout) << 16;
                if (p.use_bias && w >= nw && w < nw + dout) ofs[i] = 0xffff | (p.zoff[k] + w - nw) << 16;
            }
        }
    }

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        can_load_params(params + b * p.P, Wl, p.P, vec4);
        float gs = 0.f, yv = 0.f;                                       // the sample's combined gradient and output, column j
        if (p.comb >= 0 && j < Dn) {
            gs = g[b * Dn + j];
            if (p.comb == RECNOW_REDUCE_MEAN) gs /= (float)L;
            if (extremum) yv = y[b * Dn + j];
        }
        if (extremum) {                                                   // counting pass: how many positions attain y[b][j]
            float c = 0.f;
            for (int pass = 0; pass < npass; ++pass) {
                const int l = pass * p.C + s;
                const bool valid = l < L;
                const bool nz = can_load_x(p, x + (b * L + (valid ? l : 0)) * D0, valid, row, j);
                __syncthreads();
                float o = can_chain<true>(p, Wl, row, j);
                if (p.mask && !nz) o = 0.f;
                if (valid && j < Dn && o == yv) c += 1.f;
            }
            red[s * CAN_MAX_DIM + j] = c;
            __syncthreads();
            if (t < Dn) {
                float r = 0.f;
                for (int q = 0; q < p.C; ++q) r += red[q * CAN_MAX_DIM + t];       // small integers: exact in any order
                cnt[t] = r;
            }
            __syncthreads();
            if (j < Dn) gs /= cnt[j] > 0.f ? cnt[j] : 1.f;
        }

        float acc[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) acc[i] = 0.f;
        for (int pass = 0; pass < npass; ++pass) {
            const int l = pass * p.C + s;
            const bool valid = l < L;
            const int64_t pos = b * L + (valid ? l : 0);
            const bool nz = can_load_x(p, x + pos * D0, valid, row, j);
            __syncthreads();
            float o = can_chain<true>(p, Wl, row, j);
            if (p.mask && !nz) o = 0.f;
            float dh = 0.f;                                               // d loss / d h_n [j]
            if (valid && j < Dn && (nz || !p.mask)) {
                if (p.comb < 0)
                    dh = RN_LD_STREAM((rn_gcf)(g + pos * Dn + j));
                else if (extremum)
                    dh = o == yv ? gs : 0.f;
                else
                    dh = gs;
            }
            for (int k = p.n - 1; k >= 0; --k) {
                const int din = p.dims[k], dout = p.dims[k + 1];
                float* zr = row + p.zoff[k];
                if (j < dout) zr[j] = dh * zr[j];                         // dz_k = dh_k act'(z_k)
                __syncthreads();
                // dh_{k-1}[i] = sum_c dz_k[c] W_k[i][c] (+ dh_k[i] under res_net); lane i starts at column i % dout, so that the lanes of a
                // group, whose kernel rows lie dout floats apart, read different banks
                const int ic = j < din ? j : din - 1;
                const float* W = Wl + p.woff[k] + ic * dout;
                float nd = p.res ? dh : 0.f;
                int c = ic % dout;
                for (int q = 0; q < dout; ++q) {
                    nd = fmaf(zr[c], W[c], nd);
                    if (++c == dout) c = 0;
                }
                dh = j < din ? nd : 0.f;
            }
            if (dx && valid && j < D0) RN_ST_STREAM((rn_gf)(dx + pos * D0 + j), dh);
            if (dparams) {                                                // uniform; the rows of the chunk are complete behind the last barrier
#pragma unroll
                for (int i = 0; i < NE; ++i) {
                    if (ofs[i] >= 0) {
                        const int ho = ofs[i] & 0xffff, zo = ofs[i] >> 16;
                        float a = acc[i];
                        for (int q = 0; q < p.C; ++q) {
                            const float* r = rows + q * p.SS;
                            a = fmaf(ho == 0xffff ? 1.f : r[ho], r[zo], a);
                        }
                        acc[i] = a;
                    }
                }
            }
            __syncthreads();                                              // the next pass overwrites the slot rows
        }
        if (dparams) {
            float* dp = dparams + b * p.P;
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int e = t + i * CAN_THREADS;
                if (e < p.P) RN_ST_STREAM((rn_gf)(dp + e), acc[i]);
            }
        }
        __syncthreads();               // the next sample overwrites the parameter row
    }
}

namespace {
size_t can_lds_bytes(const CanPlan& p) {
    return ((size_t)p.ldsW + (size_t)p.C * p.SS + (size_t)p.C * CAN_MAX_DIM + CAN_MAX_DIM) * sizeof(float);
}

// Fills *p for (D0, dims, use_bias); returns whether the kernels take the shape: the backward's LDS request, the larger one, decides.
bool can_plan(int D0, const int* dims, int n, int use_bias, bool bwd, CanPlan* p) {
    if (!dims || n < 1 || n > CAN_MAX_LAYERS || D0 < 1 || D0 > CAN_MAX_DIM) return false;
    for (int k = 0; k < n; ++k)
        if (dims[k] < 1 || dims[k] > CAN_MAX_DIM) return false;
    *p = CanPlan{};
    p->n = n;
    p->use_bias = use_bias != 0;
    p->dims[0] = D0;
    int widest = D0, off = 0, sh = 0;
    for (int k = 0; k < n; ++k) {
        const int din = p->dims[k], dout = dims[k];
        p->dims[k + 1] = dout;
        widest = dout > widest ? dout : widest;
        p->woff[k] = off;
        off += din * dout;
        p->boff[k] = off;
        if (use_bias) off += dout;
        p->hoff[k] = sh;
        sh += din;
    }
    int sz = 0;
    for (int k = 0; k < n; ++k) {
        p->zoff[k] = sh + sz;
        sz += p->dims[k + 1];
    }
    p->P = off;
    p->ldsW = (off + 3) & ~3;
    p->gbits = widest <= CAN_MIN_GROUP ? 4 : widest <= 32 ? 5 : 6;
    p->C = CAN_THREADS >> p->gbits;
    p->SS = (sh + sz) | 1;                              // odd: the rows of neighbouring slots start in different banks
    if (can_lds_bytes(*p) > CAN_LDS_BYTES) return false;
    if (!bwd) p->SS = sh | 1;                           // the forward keeps no dz rows
    return true;
}

// argument checks shared by both directions; on RECNOW_OK *p is complete and *lds holds the launch's LDS bytes
int can_check(const float* x, const float* params, int64_t B, int64_t L, int D0, const int* dims, int n, int act, int use_bias, int res_net,
              int last_act, int mask, int comb, bool bwd, CanPlan* p, size_t* lds) {
    if (B < 0 || L < 0 || L > INT_MAX || !dims || n < 1 || D0 < 1) return RECNOW_EINVAL;
    if (act < RECNOW_ACT_LINEAR || act > RECNOW_ACT_SIGMOID || comb < -1 || comb > RECNOW_REDUCE_MIN) return RECNOW_EINVAL;
    for (int k = 0; k < n && k < CAN_MAX_LAYERS; ++k)
        if (dims[k] < 1 || (res_net && dims[k] != D0)) return RECNOW_EINVAL;
    if (comb >= 0 && L == 0) return RECNOW_EINVAL;
    if (!can_plan(D0, dims, n, use_bias, bwd, p)) return RECNOW_EUNSUPPORTED;
    if (B > 0 && (!params || (L > 0 && !x))) return RECNOW_EINVAL;
    p->act = act, p->res = res_net != 0, p->last_act = last_act != 0, p->mask = mask != 0, p->comb = comb;
    *lds = can_lds_bytes(*p);
    int dev = 0, most = 0;
    RN_HIP(hipGetDevice(&dev));
    RN_HIP(hipDeviceGetAttribute(&most, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (*lds > (size_t)most) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}

bool can_vec4(const CanPlan& p, const float* params) { return p.P % 4 == 0 && ((uintptr_t)params & 15) == 0; }
dim3 can_grid(int64_t B) { return dim3((unsigned)(B < (1 << 20) ? B : (1 << 20))); }
}  // namespace

extern "C" int recnow_can_supported(int D0, const int* dims, int n_layers, int use_bias) {
    CanPlan p;
    return can_plan(D0, dims, n_layers, use_bias, true, &p) ? 1 : 0;
}

extern "C" int recnow_can_fwd(const float* x, const float* params, float* y, int64_t B, int64_t L, int D0, const int* dims, int n_layers,
                              int act, int use_bias, int res_net, int last_act, int mask, int combiner, void* stream) {
    CanPlan p;
    size_t lds = 0;
    const int rc = can_check(x, params, B, L, D0, dims, n_layers, act, use_bias, res_net, last_act, mask, combiner, false, &p, &lds);
    if (rc) return rc;
    if (B == 0 || (combiner < 0 && L == 0)) return RECNOW_OK;
    if (!y) return RECNOW_EINVAL;
    hipLaunchKernelGGL(k_can_fwd, can_grid(B), CAN_THREADS, lds, (hipStream_t)stream, x, params, y, B, (int)L, p, (int)can_vec4(p, params));
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_can_bwd(const float* x, const float* params, const float* g, const float* y, int64_t B, int64_t L, int D0,
                              const int* dims, int n_layers, int act, int use_bias, int res_net, int last_act, int mask, int combiner,
                              float* dx, float* dparams, void* stream) {
    CanPlan p;
    size_t lds = 0;
    const int rc = can_check(x, params, B, L, D0, dims, n_layers, act, use_bias, res_net, last_act, mask, combiner, true, &p, &lds);
    if (rc) return rc;
    if (B == 0 || (!dx && !dparams)) return RECNOW_OK;
    if (L > 0 && !g) return RECNOW_EINVAL;
    if (combiner >= RECNOW_REDUCE_MAX && !y) return RECNOW_EINVAL;
    const dim3 grid = can_grid(B);
    hipStream_t st = (hipStream_t)stream;
    const int L32 = (int)L, v4 = (int)can_vec4(p, params);
    if (p.P <= 4 * CAN_THREADS)
        hipLaunchKernelGGL(k_can_bwd<4>, grid, CAN_THREADS, lds, st, x, params, g, y, B, L32, p, v4, dx, dparams);
    else if (p.P <= 16 * CAN_THREADS)
        hipLaunchKernelGGL(k_can_bwd<16>, grid, CAN_THREADS, lds, st, x, params, g, y, B, L32, p, v4, dx, dparams);
    else            // P <= CAN_LDS_BYTES / 4 = 64 * CAN_THREADS
        hipLaunchKernelGGL(k_can_bwd<64>, grid, CAN_THREADS, lds, st, x, params, g, y, B, L32, p, v4, dx, dparams);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
