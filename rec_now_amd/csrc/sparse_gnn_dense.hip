// SparseGNNLayer, the DENSE route: the graph as an (F, F) matrix on the matrix cores, for up to 128 fields.  csrc/sparse_gnn.hip (the edge route)
// spends about five vector instructions and an LDS wait per edge; here a layer over a tile of (row, channel) pairs is one small exact-fp32 product
//   Z[dst][pair] = sum_src M[src][dst] V[src][pair],   M = I + W,   W[src_e][dst_e] = w[set][e],   v <- act(z)
// on v_mfma_f32_32x32x2_f32, whatever the number of edges.
//
// Layout.  FP = F rounded up to 32 (NB = FP / 32 blocks), P = FP + 1 the odd LDS pitch: a pair's vector sits at pair * P + f (sg_load / sg_store of
// sparse_gnn.hpp, shared with the edge route: BFD / BDF / LIST inputs, 16-byte and 4-byte paths, D > 64 channel tiles, 64-bit offsets).
//   k_sd_densify  one small launch per call: M (n_sets, 2, FP, FP) from w (n_sets, E); plane 0 is M[src][dst], plane 1 its transpose; padding rows
//                 and columns are zero, the identity sits on the first F diagonal entries.  One thread per entry finds its edge by bisection of
//                 the SORTED edge list, so there is no memset, no second launch and no two writers of one entry (a self loop gives 1 + w).
//   product       per 32-pair block: the B operand of step k0 is buf[pair * P + k0 + (lane >> 5)], one ds_read_b32, conflict-free with the odd pitch;
//                 the A operand is M[(k0 + (lane >> 5)) * FP + 32 blk + (lane & 31)], a coalesced 128-byte global read per half wave.  M is read from
//                 L1 / L2 at every F (4 KB per set at F = 32, 64 KB at F = 128): no LDS or registers are spent on it, the reads are independent of
//                 the accumulator chain and the other waves of the CU cover them.  The accumulators of all NB destination blocks are complete
//                 before the first one is written, so a layer runs IN PLACE: the forward needs one buffer.
//   forward       one launch, all L layers: x tile (<= 64 pairs, two pair blocks) -> LDS, L products with the activation on the accumulators, every
//                 requested layer output written once.
//   backward      one launch + k_sd_gather: x tile (<= 32 pairs) -> LDS, the chain RECOMPUTED into a ring of S + 1 buffers (as the edge route; with
//                 L > S once per segment), dz = dv * act'(v_out) element-wise, dv_prev = the same product with plane 1 in place, and
//                   dM[src][dst] = sum_pairs v_in[pair][src] dz[pair][dst]
//                 as an MFMA product over the PAIRS (A = vbuf[pair * P + src], B = dzbuf[pair * P + dst], both conflict-free), NB x NB blocks of 16
//                 registers, added to the workgroup's own row of the workspace (plain load + store: every address has one owner lane for the whole
//                 launch).  k_sd_gather sums the rows in row order at the E edge positions into dw.  No float atomics: dx and dw are bit-identical
//                 from run to run.  Shared weights add their layers in layer order (L - 1 down to 0) in the row itself.
// Every buffer is zeroed once per workgroup: pairs past the tile, fields past F and the pitch column then hold finite values for ever (act(0)
// in the chain, exact zeros in the gradient buffers), so the padding adds exact zeros to dM and never a NaN to a product.
#include "sparse_gnn.hpp"

#define SD_MAXF 128
#define SD_FWD_WG 4096            // forward grid cap: 16 one-wave workgroups per CU
#define SD_BWD_WG 1024            // backward grid cap = most rows of the dM workspace
#define SD_MIN_ROWS 16
#define SD_ROWS_BYTES ((size_t)32 << 20)      // the dM rows take at most this much (or SD_MIN_ROWS rows): fewer workgroups at F = 128 with many sets

typedef float sd_f16 __attribute__((ext_vector_type(16)));

struct SdArgs {
    const float* x;
    const float* const* xl;
    int in_layout, x_v4;
    float* y_last;
    float* const* y_all;
    const float* dy_last;
    const float* const* dy_all;
    int out_layout, y_v4;
    float* dx;
    int dx_v4;
    float* rows;                  // backward: gridDim.x rows of n_sets * FP * FP floats, or NULL (no dw)
    const float* M;               // (n_sets, 2, FP, FP)
    int64_t B;
    int F, D, L, n_sets, act, S;
    SgGeo g;
};

__global__ void __launch_bounds__(256) k_sd_densify(const float* __restrict__ w, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                    float* __restrict__ M, int F, int FP, int E, int n_sets) {
    const int idx = blockIdx.x * 256 + threadIdx.x, per = FP * FP;
    if (idx >= n_sets * per) return;
    const int set = idx / per, ij = idx - set * per, i = ij / FP, j = ij - i * FP;
    float v = i == j && i < F ? 1.f : 0.f;
    int lo = 0, hi = E;                          // first edge not below (i, j)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int s = src[mid], d = dst[mid];
        if (s < i || (s == i && d < j)) lo = mid + 1;
        else hi = mid;
    }
    if (lo < E && src[lo] == i && dst[lo] == j) v += w[(int64_t)set * E + lo];
    float* m = M + (int64_t)set * 2 * per;
    m[i * FP + j] = v;
    m[per + j * FP + i] = v;
}

// out[pair][row] = epi(sum_k Mx[k][row] in[pair][k]) for the npb 32-pair blocks of a buffer; out may be in.  k runs over the fields (rounded up to 2:
// row F of Mx is zero, entry F of a vector is finite).
template <int NB, bool ACT>
__device__ __forceinline__ void sd_prod(const float* Mx, const float* in, float* out, int npb, int F, int act) {
    constexpr int FP = NB * 32, P = FP + 1;
    const int li = threadIdx.x & 31, lh = threadIdx.x >> 5, kend = (F + 1) & ~1;
    const rn_gcf ap = (rn_gcf)Mx + lh * FP + li;
    for (int pb = 0; pb < npb; ++pb) {
        sd_f16 acc[NB];
#pragma unroll
        for (int db = 0; db < NB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
        const float* bp = in + (pb * 32 + li) * P + lh;
        auto step = [&](int k0) {
            const float b = bp[k0];
#pragma unroll
            for (int db = 0; db < NB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k0 * FP + db * 32], b, acc[db], 0, 0, 0);
        };
        int k0 = 0;
        for (; k0 + 8 <= kend; k0 += 8) {        // four steps' operands in flight
#pragma unroll
            for (int u = 0; u < 8; u += 2) step(k0 + u);
        }
        for (; k0 < kend; k0 += 2) step(k0);
        // accumulator register r of lane (li, lh): row 8 (r / 4) + 4 lh + r % 4, column li
        float* op = out + (pb * 32 + li) * P + 4 * lh;
#pragma unroll
        for (int db = 0; db < NB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) op[db * 32 + 8 * (r >> 2) + (r & 3)] = ACT ? rn_act(acc[db][r], act) : acc[db][r];
    }
}

// row[src][dst] (+)= sum over the 32 pairs of vin[pair][src] dz[pair][dst]
template <int NB>
__device__ __forceinline__ void sd_dm(const float* vin, const float* dz, float* row, bool first) {
    constexpr int FP = NB * 32, P = FP + 1;
    const int li = threadIdx.x & 31, lh = threadIdx.x >> 5;
#pragma unroll 1
    for (int sb = 0; sb < NB; ++sb)
#pragma unroll 1
        for (int db = 0; db < NB; ++db) {
            const rn_gf q = (rn_gf)row + (sb * 32 + 4 * lh) * FP + db * 32 + li;
            sd_f16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = first ? 0.f : q[(8 * (r >> 2) + (r & 3)) * FP];       // in flight while the products run
            const float* ap = vin + lh * P + sb * 32 + li;
            const float* bp = dz + lh * P + db * 32 + li;
#pragma unroll
            for (int k0 = 0; k0 < 32; k0 += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k0 * P], bp[k0 * P], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) q[(8 * (r >> 2) + (r & 3)) * FP] = acc[r];
        }
}

__device__ __forceinline__ void sd_zero(float* lds, int n) {
    for (int i = threadIdx.x; i < n; i += SG_LANES) lds[i] = 0.f;
    __syncthreads();
}

template <int NB>
__global__ void __launch_bounds__(SG_LANES) k_sd_fwd(SdArgs a) {
    extern __shared__ float sd_lds[];
    constexpr int FP = NB * 32, P = FP + 1;
    const int F = a.F, npb = (a.g.np + 31) >> 5;
    float* const buf = sd_lds;
    sd_zero(buf, npb * 32 * P);
    for (int64_t tile = blockIdx.x; tile < a.g.ntiles; tile += gridDim.x) {
        int64_t b0;
        int d0;
        sg_tile_origin(tile, a.g, b0, d0);
        sg_load(buf, a.x, a.xl, a.in_layout, a.x_v4, b0, d0, a.B, F, a.D, P, a.g);
        __syncthreads();
        for (int l = 0; l < a.L; ++l) {
            sd_prod<NB, true>(a.M + (int64_t)(l % a.n_sets) * 2 * FP * FP, buf, buf, npb, F, a.act);
            float* y = a.y_all ? a.y_all[l] : nullptr;
            __syncthreads();                // the layer's writes before the stores below read them
            if (y) sg_store(buf, y, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, P, a.g);
            if (l == a.L - 1 && a.y_last) sg_store(buf, a.y_last, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, P, a.g);
            __syncthreads();                // the stores' reads before the next layer (or the next tile) overwrites the buffer
        }
    }
}

template <int NB>
__global__ void __launch_bounds__(SG_LANES) k_sd_bwd(SdArgs a) {
    extern __shared__ float sd_lds[];
    constexpr int FP = NB * 32, P = FP + 1, bufsz = 32 * P, MM = FP * FP;
    const int F = a.F, L = a.L, S = a.S, act = a.act;
    float* const X = sd_lds;                    // v_0
    float* const ring = X + bufsz;              // v_j, j >= 1, at slot j % (S + 1)
    float* const G = ring + (S + 1) * bufsz;    // the gradient that walks down the chain
    float* const T = G + bufsz;                 // a layer's own output gradient (only with dy_all)
    sd_zero(sd_lds, (S + 3 + (a.dy_all ? 1 : 0)) * bufsz);
    float* const wsrow = a.rows ? a.rows + (int64_t)blockIdx.x * a.n_sets * MM : nullptr;
    bool first_tile = true;
    for (int64_t tile = blockIdx.x; tile < a.g.ntiles; tile += gridDim.x) {
        int64_t b0;
        int d0;
        sg_tile_origin(tile, a.g, b0, d0);
        sg_load(X, a.x, a.xl, a.in_layout, a.x_v4, b0, d0, a.B, F, a.D, P, a.g);
        sg_load(G, a.dy_last, nullptr, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, P, a.g);     // zeros when only per-layer gradients come in
        __syncthreads();
        for (int hi = L; hi > 0;) {
            const int lo = hi > S ? hi - S : 0;
            for (int j = 0; j < hi; ++j) {           // v_1 .. v_hi; v_lo .. v_hi survive in the ring (hi - lo <= S)
                const float* in = j == 0 ? X : ring + (j % (S + 1)) * bufsz;
                sd_prod<NB, true>(a.M + (int64_t)(j % a.n_sets) * 2 * MM, in, ring + ((j + 1) % (S + 1)) * bufsz, 1, F, act);
                __syncthreads();
            }
            for (int l = hi - 1; l >= lo; --l) {
                const float* vout = ring + ((l + 1) % (S + 1)) * bufsz;
                const float* vin = l == 0 ? X : ring + (l % (S + 1)) * bufsz;
                const float* dyl = a.dy_all ? a.dy_all[l] : nullptr;
                if (dyl) {                           // this layer's own output gradient joins the one that came down the chain
                    sg_load(T, dyl, nullptr, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, P, a.g);
                    __syncthreads();
                    for (int i = threadIdx.x; i < bufsz; i += SG_LANES) G[i] = (G[i] + T[i]) * rn_act_grad_from_out(vout[i], act);
                } else {
                    for (int i = threadIdx.x; i < bufsz; i += SG_LANES) G[i] *= rn_act_grad_from_out(vout[i], act);      // dz
                }
                __syncthreads();
                const int s = l % a.n_sets;
                if (wsrow) sd_dm<NB>(vin, G, wsrow + (int64_t)s * MM, first_tile && l >= L - a.n_sets);     // a set's first contribution: store, do not add
                if (l > 0 || a.dx) {                 // dv_prev = dz M^T, in place
                    sd_prod<NB, false>(a.M + ((int64_t)s * 2 + 1) * MM, G, G, 1, F, act);
                    __syncthreads();
                }
            }
            hi = lo;
        }
        if (a.dx) sg_store(G, a.dx, a.in_layout, a.dx_v4, b0, d0, a.B, F, a.D, P, a.g);
        __syncthreads();
        first_tile = false;
    }
}

// dw[set][e] = sum over the workspace rows of rows[row][set][src_e][dst_e], in row order
__global__ void __launch_bounds__(256) k_sd_gather(const float* __restrict__ rows, int nrows, const int32_t* __restrict__ src,
                                                   const int32_t* __restrict__ dst, int FP, int E, int n_sets, float* __restrict__ dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sets * E) return;
    const int set = i / E, e = i - set * E;
    const int64_t stride = (int64_t)n_sets * FP * FP;
    const float* p = rows + (int64_t)set * FP * FP + src[e] * FP + dst[e];
    float s = 0.f;
    int r = 0;
    for (; r + 8 <= nrows; r += 8) {         // eight loads in flight, added in row order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(r + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < nrows; ++r) s += p[r * stride];
    dw[i] = s;
}

namespace {
int sd_fp(int F) { return (F + 31) / 32 * 32; }
size_t sd_m_bytes(int F, int n_sets) { return rn_align((size_t)n_sets * 2 * sd_fp(F) * sd_fp(F) * sizeof(float)); }
int sd_rows(int F, int n_sets) {
    const size_t row = (size_t)n_sets * sd_fp(F) * sd_fp(F) * sizeof(float);
    const size_t fit = SD_ROWS_BYTES / row;
    return (int)(fit > SD_BWD_WG ? SD_BWD_WG : fit < SD_MIN_ROWS ? SD_MIN_ROWS : fit);
}

int sd_check(const float* x, const float* const* x_fields, int in_layout, int out_layout, const int32_t* src, const int32_t* dst, const float* w,
             int64_t B, int F, int D, int E, int L, int n_sets, int act) {
    if (B < 0 || F < 1 || D < 1 || E < 0 || L < 1 || n_sets < 1 || n_sets > L) return RECNOW_EINVAL;
    if (act < RECNOW_ACT_LINEAR || act > RECNOW_ACT_SIGMOID) return RECNOW_EINVAL;
    if (in_layout < RECNOW_GNN_BFD || in_layout > RECNOW_GNN_LIST) return RECNOW_EINVAL;
    if (out_layout != RECNOW_GNN_BFD && out_layout != RECNOW_GNN_BDF) return RECNOW_EINVAL;
    if (F > SD_MAXF || (int64_t)E > (int64_t)F * F) return RECNOW_EUNSUPPORTED;
    if (B > 0 && (in_layout == RECNOW_GNN_LIST ? x_fields == nullptr : x == nullptr)) return RECNOW_EINVAL;
    if (E > 0 && (!src || !dst || !w)) return RECNOW_EINVAL;
    return RECNOW_OK;
}

void sd_fill(SdArgs& a, const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const float* M, int64_t B,
             int F, int D, int L, int n_sets, int act) {
    a.x = in_layout == RECNOW_GNN_LIST ? nullptr : x;
    a.xl = in_layout == RECNOW_GNN_LIST ? x_fields : nullptr;
    a.in_layout = in_layout, a.out_layout = out_layout;
    const int in_run = in_layout == RECNOW_GNN_BDF ? F : D;       // the axis a 16-byte access runs along
    a.x_v4 = in_run % 4 == 0 && (in_layout == RECNOW_GNN_LIST ? x_aligned != 0 : sg_aligned(x));
    a.M = M;
    a.B = B, a.F = F, a.D = D, a.L = L, a.n_sets = n_sets, a.act = act;
}

int sd_densify(const float* w, const int32_t* src, const int32_t* dst, float* M, int F, int E, int n_sets, hipStream_t st) {
    const int FP = sd_fp(F), n = n_sets * FP * FP;
    hipLaunchKernelGGL(k_sd_densify, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, src, dst, M, F, FP, E, n_sets);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// Dynamic LDS a workgroup of the backward may own on this device: raising the kernel's limit IS the query (the device attribute only reports
// the 64 KB default); rn_lds_grant remembers either answer.
template <int NB>
size_t sd_bwd_lds_cap() {
    return rn_lds_grant((const void*)k_sd_bwd<NB>, 160 * 1024) == hipSuccess ? 160 * 1024 : 64 * 1024;
}

// Ring slots of the backward: as many as L needs inside 40 KB (four workgroups per CU); else inside 64 KB; else inside what the device allows.
template <int NB>
int sd_bwd_slots(int L, int extra, size_t* lds) {
    const size_t buf = (size_t)32 * (NB * 32 + 1) * sizeof(float);
    const int want = L < 2 ? L : 2;
    int S = (int)(40 * 1024 / buf) - 3 - extra;
    if (S < want) S = (int)(64 * 1024 / buf) - 3 - extra;
    if (S < want) S = (int)(sd_bwd_lds_cap<NB>() / buf) - 3 - extra;
    if (S > L) S = L;
    *lds = (size_t)(S + 3 + extra) * buf;
    return S;
}

template <int NB>
int sd_launch_bwd(SdArgs& a, int grid, hipStream_t st) {
    size_t lds = 0;
    a.S = sd_bwd_slots<NB>(a.L, a.dy_all ? 1 : 0, &lds);
    if (a.S < 1) return RECNOW_EUNSUPPORTED;
    hipLaunchKernelGGL(k_sd_bwd<NB>, dim3((unsigned)grid), dim3(SG_LANES), lds, st, a);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
}  // namespace

extern "C" size_t recnow_sparse_gnn_dense_workspace_bytes(int F, int E, int n_sets, int backward) {
    if (F < 1 || F > SD_MAXF || E < 0 || n_sets < 1) return 0;
    size_t n = sd_m_bytes(F, n_sets);
    if (backward && E > 0) n += rn_align((size_t)sd_rows(F, n_sets) * n_sets * sd_fp(F) * sd_fp(F) * sizeof(float));
    return n;
}

extern "C" int recnow_sparse_gnn_dense_fwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout,
                                           const int32_t* src, const int32_t* dst, const float* w, int64_t B, int F, int D, int E, int L,
                                           int n_sets, int act, float* y_last, float* const* y_all, int y_aligned, void* ws, size_t ws_bytes,
                                           void* stream) {
    int rc = sd_check(x, x_fields, in_layout, out_layout, src, dst, w, B, F, D, E, L, n_sets, act);
    if (rc) return rc;
    if (!y_last && !y_all) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    if (!ws || !sg_aligned(ws) || ws_bytes < recnow_sparse_gnn_dense_workspace_bytes(F, E, n_sets, 0)) return RECNOW_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    rc = sd_densify(w, src, dst, (float*)ws, F, E, n_sets, st);
    if (rc) return rc;
    SdArgs a = {};
    sd_fill(a, x, x_fields, in_layout, x_aligned, out_layout, (const float*)ws, B, F, D, L, n_sets, act);
    a.y_last = y_last, a.y_all = y_all;
    a.y_v4 = (out_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(y_last) && (y_all == nullptr || y_aligned != 0);
    a.g = sg_geo(B, D, SG_LANES);
    const int NB = sd_fp(F) / 32;
    const size_t lds = (size_t)((a.g.np + 31) / 32) * 32 * (NB * 32 + 1) * sizeof(float);
    const dim3 grid((unsigned)(a.g.ntiles < SD_FWD_WG ? a.g.ntiles : SD_FWD_WG));
    if (NB == 1) hipLaunchKernelGGL(k_sd_fwd<1>, grid, dim3(SG_LANES), lds, st, a);
    else if (NB == 2) hipLaunchKernelGGL(k_sd_fwd<2>, grid, dim3(SG_LANES), lds, st, a);
    else if (NB == 3) hipLaunchKernelGGL(k_sd_fwd<3>, grid, dim3(SG_LANES), lds, st, a);
    else hipLaunchKernelGGL(k_sd_fwd<4>, grid, dim3(SG_LANES), lds, st, a);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_sparse_gnn_dense_bwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout,
                                           const int32_t* src, const int32_t* dst, const float* w, int64_t B, int F, int D, int E, int L,
                                           int n_sets, int act, const float* dy_last, const float* const* dy_all, int dy_aligned, float* dx,
                                           float* dw, void* ws, size_t ws_bytes, void* stream) {
    int rc = sd_check(x, x_fields, in_layout, out_layout, src, dst, w, B, F, D, E, L, n_sets, act);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (E == 0) dw = nullptr;
    if (B == 0) {                 // empty batch: the weight gradients are sums over no rows
        if (dw) RN_HIP(hipMemsetAsync(dw, 0, (size_t)n_sets * E * sizeof(float), st));
        return RECNOW_OK;
    }
    if (!dy_last && !dy_all) return RECNOW_EINVAL;
    if (!dx && !dw) return RECNOW_OK;
    if (!ws || !sg_aligned(ws) || ws_bytes < recnow_sparse_gnn_dense_workspace_bytes(F, E, n_sets, dw != nullptr)) return RECNOW_EWORKSPACE;
    rc = sd_densify(w, src, dst, (float*)ws, F, E, n_sets, st);
    if (rc) return rc;
    SdArgs a = {};
    sd_fill(a, x, x_fields, in_layout, x_aligned, out_layout, (const float*)ws, B, F, D, L, n_sets, act);
    a.dy_last = dy_last, a.dy_all = dy_all;
    a.y_v4 = (out_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(dy_last) && (dy_all == nullptr || dy_aligned != 0);
    a.dx = dx;
    a.dx_v4 = (in_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(dx);
    a.rows = dw ? (float*)((char*)ws + sd_m_bytes(F, n_sets)) : nullptr;
    a.g = sg_geo(B, D, 32);
    const int cap = dw ? sd_rows(F, n_sets) : SD_BWD_WG;
    const int grid = (int)(a.g.ntiles < cap ? a.g.ntiles : cap);
    const int NB = sd_fp(F) / 32;
    rc = NB == 1 ? sd_launch_bwd<1>(a, grid, st) : NB == 2 ? sd_launch_bwd<2>(a, grid, st) : NB == 3 ? sd_launch_bwd<3>(a, grid, st)
                                                                                                     : sd_launch_bwd<4>(a, grid, st);
    if (rc) return rc;
    if (dw) {
        const int n = n_sets * E;
        hipLaunchKernelGGL(k_sd_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)a.rows, grid, src, dst, NB * 32, E, n_sets, dw);
        RN_LAUNCH_CHECK();
    }
    return RECNOW_OK;
}
