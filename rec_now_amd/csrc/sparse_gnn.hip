// SparseGNNLayer: L graph-convolution layers over the F field embeddings of a row, reference rec_now/layers/sparse_gnn_layer.py:227-236:
//   x (B, D, F);  per layer  x = act(x + x @ to_dense(W_l)),  W_l an (F, F) matrix with E non-zeros  W_l[src_e][dst_e] = w[l % n_sets][e].
// The layer is pointwise over the B*D (row, channel) PAIRS: a pair owns an F-vector v and every layer maps it to
//   z[i] = v[i] + sum_{e: dst_e = i} w[e] v[src_e],   v <- act(z).
// One lane owns one pair.  Its F-vectors (one per live layer) sit in LDS at pair * FP + f with FP = F | 1: the pitch is odd, so the lanes of a
// ds_read_b32 group (32 consecutive pairs, one field) fall in 32 different banks, and the edge loop reads v[src_e] with a wave-uniform src_e from the
// edge tables (loaded 64 chunks of four edges at a time, one chunk per lane, and broadcast with v_readlane).  Nothing but the staging loops ever reads another lane's LDS.
//
// A TILE is np <= 64 pairs: RT = np / D whole rows when D <= np (a contiguous block of RT*F*D floats in the (B,F,D) and (B,D,F) layouts, moved with
// 16-byte accesses when the addresses allow it), else DT channels of one row.  Workgroups are one wave and walk the tiles with a grid stride.
//   forward:  x tile -> LDS, L layers ping-pong between two buffers, every requested layer output is written once.
//   backward: x tile -> LDS, the layer chain is RECOMPUTED (nothing but x is read from HBM); v_lo .. v_hi of a segment of S layers stay in a ring
//             of S + 1 buffers, S as large as 64 KB of LDS allows; with L > S the chain is recomputed once per segment.
//             dz = dv * act'(v_{l+1}); dw[e] += v_l[src_e] dz[dst_e]; dv[i] = dz[i] + sum_{e: src_e = i} w[e] dz[dst_e].
//             dw: the 64 per-lane products of 32 edges are summed by a butterfly (one shuffle per edge), the owning lane adds the sum to the
//             workgroup's own row of the workspace (plain load + store: only that lane ever touches the address), k_sg_reduce adds the rows in
//             order.  No float atomics: dw is bit-identical from run to run.
#include "sparse_gnn.hpp"

#define SG_MAXF 64
#define SG_MAXE (SG_MAXF * SG_MAXF)
#define SG_LDS_BYTES 65536
#define SG_FWD_WG 2304          // forward grid cap: 9 one-wave workgroups per CU (what 17 KB of LDS each allows at F = 32)
#define SG_BWD_WG 1024          // backward grid cap = rows of the dw workspace

// Read-only for the whole launch: the constant address space makes a wave-uniform read a scalar load.
typedef const int32_t __attribute__((address_space(4)))* sg_ci;

// Edge tables (int32, built once per layer object).  A pass over the graph is a stream of CHUNKS of four edges of one node, in node order: a node
// with no edge still has one chunk, a short chunk is padded with edges of weight index -1 (weight 0) that read the node itself.  The stream is
// walked front to back, 64 chunks per vector load (sg_pass).
//   tab = Cd | Cs | 0 | 0 | dS (Cd x 8) | dG (Cd x 4) | sS (Cs x 8) | sG (Cs x 4) | ssrc (E) | sdst (E) | swid (E)
//   S: o0 o1 o2 o3 node flags 0 0   (flags: 1 = first chunk of the node, 2 = last);   G: the weight index of each of the four edges
//   d*: by destination (o = source; the forward).  s*: by source (o = destination; the input gradient).  ssrc / sdst / swid: the edges in by-source
//   order with their weight index, for the weight-gradient pass.
#define SG_CHUNK 4
struct SgTab {
    int Cd, Cs;
    const int32_t *dS, *dG, *sS, *sG, *ssrc, *sdst, *swid;
};

struct SgArgs {
    const float* x;               // BFD / BDF input, or NULL
    const float* const* xl;       // LIST input: device array of F pointers to (B, D)
    int in_layout, x_v4;
    float* y_last;                // forward: last layer's output or NULL
    float* const* y_all;          // forward: device array of L pointers (entries may be 0) or NULL
    const float* dy_last;         // backward
    const float* const* dy_all;   // backward: device array of L pointers (entries may be 0) or NULL
    int out_layout, y_v4;
    float* dx;                    // backward: BFD / BDF as the input, (F, B, D) block for LIST; or NULL
    int dx_v4;
    float* ws;                    // backward: gridDim.x rows of n_sets * E floats, or NULL (no dw)
    const int32_t* tab;
    const float* w;               // (n_sets, E)
    int64_t B;
    int F, D, E, L, n_sets, act, S;
    SgGeo g;
};

__device__ __forceinline__ SgTab sg_tab(const int32_t* tab, int E) {
    SgTab t;
    t.Cd = ((sg_ci)tab)[0], t.Cs = ((sg_ci)tab)[1];
    t.dS = tab + 4;
    t.dG = t.dS + t.Cd * 8;
    t.sS = t.dG + t.Cd * 4;
    t.sG = t.sS + t.Cs * 8;
    t.ssrc = t.sG + t.Cs * 4;
    t.sdst = t.ssrc + E;
    t.swid = t.sdst + E;
    return t;
}

typedef int sg_i4 __attribute__((ext_vector_type(4)));
typedef int sg_i2 __attribute__((ext_vector_type(2)));
typedef const sg_i4 __attribute__((address_space(1)))* sg_gci4;
typedef const sg_i2 __attribute__((address_space(1)))* sg_gci2;
typedef const int32_t __attribute__((address_space(1)))* sg_gci;

__device__ __forceinline__ int sg_bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float sg_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// One pass over a chunk stream for the lane's pair at `in` / `out`: out[node] = in[node] + sum over the node's edges of wl[g] in[o], then the
// activation when ACT.  Forward: the by-destination stream.  Input gradient: the by-source stream.
// The stream is taken 64 chunks at a time: lane c loads the record, the weight indices and the four weights of chunk c with vector loads (two
// memory round trips per 64 chunks), and the chunk loop broadcasts them from lane c with v_readlane -- there is no memory access in it but the
// LDS reads of the pair's values.  EVERY lane of the wave must call this (lanes without a pair pass live = false and a valid `in`).
template <bool ACT>
__device__ __forceinline__ void sg_pass(const float* in, float* out, bool live, const int32_t* S, const int32_t* G, int C, const float* wl, int act) {
    const int lane = threadIdx.x;
    float z = 0.f;
    for (int cb = 0; cb < C; cb += SG_LANES) {
        const int c = cb + lane < C ? cb + lane : C - 1;
        const sg_i4 o = *(sg_gci4)(S + c * 8);
        const sg_i2 nf = *(sg_gci2)(S + c * 8 + 4);
        const sg_i4 g = *(sg_gci4)(G + c * 4);
        const rn_gcf wg = (rn_gcf)wl;
        const float w0 = g.x < 0 ? 0.f : wg[g.x < 0 ? 0 : g.x], w1 = g.y < 0 ? 0.f : wg[g.y < 0 ? 0 : g.y];     // index -1: a padding edge, weight 0
        const float w2 = g.z < 0 ? 0.f : wg[g.z < 0 ? 0 : g.z], w3 = g.w < 0 ? 0.f : wg[g.w < 0 ? 0 : g.w];
        const int n = C - cb < SG_LANES ? C - cb : SG_LANES;
        for (int j = 0; j < n; ++j) {
            const int node = sg_bcast(nf.x, j), flags = sg_bcast(nf.y, j);
            const float self = in[node], v0 = in[sg_bcast(o.x, j)], v1 = in[sg_bcast(o.y, j)], v2 = in[sg_bcast(o.z, j)], v3 = in[sg_bcast(o.w, j)];
            z = flags & 1 ? self : z;
            z = fmaf(sg_bcast(w0, j), v0, z), z = fmaf(sg_bcast(w1, j), v1, z), z = fmaf(sg_bcast(w2, j), v2, z), z = fmaf(sg_bcast(w3, j), v3, z);
            if ((flags & 2) && live) out[node] = ACT ? rn_act(z, act) : z;
        }
    }
}

__global__ void __launch_bounds__(SG_LANES) k_sg_fwd(SgArgs a) {
    extern __shared__ float sg_lds[];
    const int lane = threadIdx.x, F = a.F, FP = F | 1, bufsz = a.g.np * FP;
    const bool live = lane < a.g.np;
    const int my = (live ? lane : 0) * FP;      // lanes without a pair never write; what they read is discarded
    const SgTab t = sg_tab(a.tab, a.E);
    const float* w = a.w;
    for (int64_t tile = blockIdx.x; tile < a.g.ntiles; tile += gridDim.x) {
        int64_t b0;
        int d0;
        sg_tile_origin(tile, a.g, b0, d0);
        float *cur = sg_lds, *nxt = sg_lds + bufsz;
        sg_load(cur, a.x, a.xl, a.in_layout, a.x_v4, b0, d0, a.B, F, a.D, FP, a.g);
        __syncthreads();
        for (int l = 0; l < a.L; ++l) {
            sg_pass<true>(cur + my, nxt + my, live, t.dS, t.dG, t.Cd, w + (int64_t)(l % a.n_sets) * a.E, a.act);
            float* s = cur;
            cur = nxt, nxt = s;
            float* y = a.y_all ? a.y_all[l] : nullptr;
            __syncthreads();                // the layer's writes before the stores below read them; the stores of layer l - 1 before `nxt` is rewritten
            if (y) sg_store(cur, y, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, FP, a.g);
            if (l == a.L - 1 && a.y_last) sg_store(cur, a.y_last, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, FP, a.g);
        }
        __syncthreads();
    }
}

// a[0] <- sum over the 64 lanes of a[j], j = the lane's bits 5..1 read as a number (both lanes of a pair end with the same sum)
__device__ __forceinline__ float sg_butterfly(float (&a)[32], int lane) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int h = 16 >> s, o = 32 >> s;
        const unsigned up = lane & o ? ~0u : 0u;      // bit selects (v_bfi): a ?: on two array elements becomes a dynamically indexed array
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const unsigned lo = __float_as_uint(a[j]), hi = __float_as_uint(a[j + h]);
            const float keep = __uint_as_float((hi & up) | (lo & ~up)), send = __uint_as_float((lo & up) | (hi & ~up));
            a[j] = keep + __shfl_xor(send, o, 64);
        }
    }
    return a[0] + __shfl_xor(a[0], 1, 64);
}

__global__ void __launch_bounds__(SG_LANES) k_sg_bwd(SgArgs a) {
    extern __shared__ float sg_lds[];
    const int lane = threadIdx.x, F = a.F, FP = F | 1, bufsz = a.g.np * FP, E = a.E, L = a.L, S = a.S, act = a.act;
    const bool live = lane < a.g.np;
    const SgTab t = sg_tab(a.tab, E);
    const float* w = a.w;
    float* const X = sg_lds;                    // v_0
    float* const ring = X + bufsz;              // v_j, j >= 1, at slot j % (S + 1)
    float* const G0 = ring + (S + 1) * bufsz;   // the two gradient buffers
    float* const G1 = G0 + bufsz;
    const int my = (live ? lane : 0) * FP;      // lanes without a pair never write; what they read is discarded
    const int edge_of_lane = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    float* const wsrow = a.ws ? a.ws + (int64_t)blockIdx.x * a.n_sets * E : nullptr;
    bool first_tile = true;
    for (int64_t tile = blockIdx.x; tile < a.g.ntiles; tile += gridDim.x) {
        int64_t b0;
        int d0;
        sg_tile_origin(tile, a.g, b0, d0);
        sg_load(X, a.x, a.xl, a.in_layout, a.x_v4, b0, d0, a.B, F, a.D, FP, a.g);
        float *cur = G0, *oth = G1;
        sg_load(cur, a.dy_last, nullptr, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, FP, a.g);     // zeros when only per-layer gradients come in
        __syncthreads();
        for (int hi = L; hi > 0;) {
            const int lo = hi > S ? hi - S : 0;
            for (int j = 0; j < hi; ++j) {           // v_1 .. v_hi; v_lo .. v_hi survive in the ring (hi - lo <= S)
                const float* in = j == 0 ? X : ring + (j % (S + 1)) * bufsz;
                sg_pass<true>(in + my, ring + ((j + 1) % (S + 1)) * bufsz + my, live, t.dS, t.dG, t.Cd, w + (int64_t)(j % a.n_sets) * E, act);
            }
            for (int l = hi - 1; l >= lo; --l) {
                const float* vout = ring + ((l + 1) % (S + 1)) * bufsz + my;
                const float* vin = (l == 0 ? X : ring + (l % (S + 1)) * bufsz) + my;
                const float* dyl = a.dy_all ? a.dy_all[l] : nullptr;
                if (dyl) {                           // this layer's own output gradient joins the one that came down the chain
                    __syncthreads();
                    sg_load(oth, dyl, nullptr, a.out_layout, a.y_v4, b0, d0, a.B, F, a.D, FP, a.g);
                    __syncthreads();
                    if (live)
                        for (int i = 0; i < F; ++i) cur[my + i] += oth[my + i];
                }
                if (live)
                    for (int i = 0; i < F; ++i) cur[my + i] *= rn_act_grad_from_out(vout[i], act);     // dz
                const int s = l % a.n_sets;
                if (wsrow) {
                    float* wsl = wsrow + (int64_t)s * E;
                    const bool first = first_tile && l >= L - a.n_sets;      // the first contribution to this set's row: store, do not add
                    for (int kb = 0; kb < E; kb += 32) {
                        const int kl = kb + (lane & 31) < E ? kb + (lane & 31) : E - 1;      // lane j (and j + 32) loads edge kb + j
                        const int es = ((sg_gci)t.ssrc)[kl], ed = ((sg_gci)t.sdst)[kl], ew = ((sg_gci)t.swid)[kl];
                        const bool mine = !(lane & 1) && kb + edge_of_lane < E;
                        float* q = wsl + __shfl(ew, edge_of_lane, 64);
                        const float old = mine && !first ? *q : 0.f;       // in flight while the products are formed and summed
                        float p[32];
#pragma unroll
                        for (int j = 0; j < 32; ++j) {
                            const float prod = vin[sg_bcast(es, j)] * cur[my + sg_bcast(ed, j)];
                            p[j] = live ? prod : 0.f;
                        }
                        const float sum = sg_butterfly(p, lane);
                        if (mine) *q = old + sum;
                    }
                }
                if (l > 0 || a.dx) {                 // dv[i] = dz[i] + sum over the by-source segment i of w[wid] dz[dst]
                    sg_pass<false>(cur + my, oth + my, live, t.sS, t.sG, t.Cs, w + (int64_t)s * E, act);
                    float* sw = cur;
                    cur = oth, oth = sw;
                }
            }
            hi = lo;
        }
        __syncthreads();
        if (a.dx) sg_store(cur, a.dx, a.in_layout, a.dx_v4, b0, d0, a.B, F, a.D, FP, a.g);
        __syncthreads();
        first_tile = false;
    }
}

// dw[i] = sum over the workspace rows of ws[row][i], in row order
__global__ void __launch_bounds__(256) k_sg_reduce(const float* __restrict__ ws, int rows, int n, float* __restrict__ dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    int r = 0;
    for (; r + 8 <= rows; r += 8) {          // eight loads in flight, added in row order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ws[(int64_t)(r + u) * n + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < rows; ++r) s += ws[(int64_t)r * n + i];
    dw[i] = s;
}

namespace {
// backward tile: the most pairs (64, 32, 16) whose x, two gradient buffers and a ring of two fit in LDS; then as many ring slots as fit, at most L + 1
int sg_bwd_npmax(int F) {
    int np = SG_LANES;
    while (np > 16 && (size_t)5 * np * (F | 1) * sizeof(float) > SG_LDS_BYTES) np >>= 1;
    return np;
}
int sg_bwd_slots(const SgGeo& g, int F, int L) {
    const int fit = (int)(SG_LDS_BYTES / ((size_t)g.np * (F | 1) * sizeof(float))) - 4;
    return fit < L ? fit : L;
}
int sg_bwd_wgs(const SgGeo& g) { return (int)(g.ntiles < SG_BWD_WG ? g.ntiles : SG_BWD_WG); }

int sg_check(const float* x, const float* const* x_fields, int in_layout, int out_layout, const int32_t* tab, const float* w, int64_t B, int F,
             int D, int E, int L, int n_sets, int act) {
    if (B < 0 || F < 1 || D < 1 || E < 0 || L < 1 || n_sets < 1 || n_sets > L) return RECNOW_EINVAL;
    if (act < RECNOW_ACT_LINEAR || act > RECNOW_ACT_SIGMOID) return RECNOW_EINVAL;
    if (in_layout < RECNOW_GNN_BFD || in_layout > RECNOW_GNN_LIST) return RECNOW_EINVAL;
    if (out_layout != RECNOW_GNN_BFD && out_layout != RECNOW_GNN_BDF) return RECNOW_EINVAL;
    if (F > SG_MAXF || E > SG_MAXE) return RECNOW_EUNSUPPORTED;
    if (B > 0 && (in_layout == RECNOW_GNN_LIST ? x_fields == nullptr : x == nullptr)) return RECNOW_EINVAL;
    if (!tab || !sg_aligned(tab) || (E > 0 && !w)) return RECNOW_EINVAL;       // the chunk records are read 16 bytes at a time
    return RECNOW_OK;
}

void sg_fill(SgArgs& a, const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout, const int32_t* tab,
             const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act) {
    a.x = in_layout == RECNOW_GNN_LIST ? nullptr : x;
    a.xl = in_layout == RECNOW_GNN_LIST ? x_fields : nullptr;
    a.in_layout = in_layout, a.out_layout = out_layout;
    const int in_run = in_layout == RECNOW_GNN_BDF ? F : D;       // the axis a 16-byte access runs along
    a.x_v4 = in_run % 4 == 0 && (in_layout == RECNOW_GNN_LIST ? x_aligned != 0 : sg_aligned(x));
    a.tab = tab, a.w = w;
    a.B = B, a.F = F, a.D = D, a.E = E, a.L = L, a.n_sets = n_sets, a.act = act;
}
}  // namespace

extern "C" size_t recnow_sparse_gnn_workspace_bytes(int64_t B, int F, int D, int E, int n_sets) {
    if (B < 1 || F < 1 || F > SG_MAXF || D < 1 || E < 1 || n_sets < 1) return 0;
    const SgGeo g = sg_geo(B, D, sg_bwd_npmax(F));
    return rn_align((size_t)sg_bwd_wgs(g) * n_sets * E * sizeof(float));
}

extern "C" int recnow_sparse_gnn_fwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout,
                                     const int32_t* tab, const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act,
                                     float* y_last, float* const* y_all, int y_aligned, void* stream) {
    int rc = sg_check(x, x_fields, in_layout, out_layout, tab, w, B, F, D, E, L, n_sets, act);
    if (rc) return rc;
    if (!y_last && !y_all) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    SgArgs a = {};
    sg_fill(a, x, x_fields, in_layout, x_aligned, out_layout, tab, w, B, F, D, E, L, n_sets, act);
    a.y_last = y_last, a.y_all = y_all;
    a.y_v4 = (out_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(y_last) && (y_all == nullptr || y_aligned != 0);
    a.g = sg_geo(B, D, SG_LANES);
    const size_t lds = (size_t)2 * a.g.np * (F | 1) * sizeof(float);
    const unsigned grid = (unsigned)(a.g.ntiles < SG_FWD_WG ? a.g.ntiles : SG_FWD_WG);
    hipLaunchKernelGGL(k_sg_fwd, dim3(grid), dim3(SG_LANES), lds, (hipStream_t)stream, a);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_sparse_gnn_bwd(const float* x, const float* const* x_fields, int in_layout, int x_aligned, int out_layout,
                                     const int32_t* tab, const float* w, int64_t B, int F, int D, int E, int L, int n_sets, int act,
                                     const float* dy_last, const float* const* dy_all, int dy_aligned, float* dx, float* dw, void* ws,
                                     size_t ws_bytes, void* stream) {
    int rc = sg_check(x, x_fields, in_layout, out_layout, tab, w, B, F, D, E, L, n_sets, act);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int n = n_sets * E;
    if (E == 0) dw = nullptr;
    if (B == 0) {                 // empty batch: the weight gradients are sums over no rows
        if (dw) RN_HIP(hipMemsetAsync(dw, 0, (size_t)n * sizeof(float), st));
        return RECNOW_OK;
    }
    if (!dy_last && !dy_all) return RECNOW_EINVAL;
    if (!dx && !dw) return RECNOW_OK;
    if (dw && (!ws || ws_bytes < recnow_sparse_gnn_workspace_bytes(B, F, D, E, n_sets))) return RECNOW_EWORKSPACE;
    SgArgs a = {};
    sg_fill(a, x, x_fields, in_layout, x_aligned, out_layout, tab, w, B, F, D, E, L, n_sets, act);
    a.dy_last = dy_last, a.dy_all = dy_all;
    a.y_v4 = (out_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(dy_last) && (dy_all == nullptr || dy_aligned != 0);
    a.dx = dx;
    a.dx_v4 = (in_layout == RECNOW_GNN_BDF ? F : D) % 4 == 0 && sg_aligned(dx);
    a.ws = dw ? (float*)ws : nullptr;
    a.g = sg_geo(B, D, sg_bwd_npmax(F));
    a.S = sg_bwd_slots(a.g, F, L);
    if (a.S < 1) return RECNOW_EUNSUPPORTED;
    const size_t lds = (size_t)(a.S + 4) * a.g.np * (F | 1) * sizeof(float);
    const int grid = sg_bwd_wgs(a.g);
    hipLaunchKernelGGL(k_sg_bwd, dim3((unsigned)grid), dim3(SG_LANES), lds, st, a);
    RN_LAUNCH_CHECK();
    if (dw) {
        hipLaunchKernelGGL(k_sg_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)ws, grid, n, dw);
        RN_LAUNCH_CHECK();
    }
    return RECNOW_OK;
}
