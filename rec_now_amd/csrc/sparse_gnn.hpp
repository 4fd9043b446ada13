// Tile geometry and the global <-> LDS staging of the SparseGNNLayer kernels (csrc/sparse_gnn.hip, the edge route; csrc/sparse_gnn_dense.hip,
// the dense MFMA route).  A TILE is np <= 64 pairs of one-wave workgroups: RT = np / D whole rows when D <= np, else DT channels of one row; a
// pair's F-vector sits in LDS at pair * FP + f, FP an odd pitch >= F that the caller chooses.
#pragma once
#include "common.hpp"

#define SG_LANES 64

struct SgGeo {
    int np, rt, dt, ndt;   // pairs per tile = rt * dt; ndt channel tiles per row (1 when rt rows are whole)
    int64_t ntiles;
};

__device__ __forceinline__ int sg_div(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }   // exact for x < 2^16 (x + 0.5 is 0.5/n away from an integer)

// element (b, f, d) of a tensor in `layout`; RECNOW_GNN_LIST here is the (F, B, D) block of the list gradient
__device__ __forceinline__ int64_t sg_off(int layout, int64_t b, int f, int d, int64_t B, int F, int D) {
    if (layout == RECNOW_GNN_BFD) return (b * F + f) * D + d;
    if (layout == RECNOW_GNN_BDF) return (b * D + d) * F + f;
    return ((int64_t)f * B + b) * D + d;
}

// The tile's elements in the memory order of `layout`, V at a time: idx -> (row r, channel dd, field f) of the tile.  BDF runs along f, the others along d.
struct SgWalk {
    int n0, n1, layout;
    float i0, i1;
    __device__ SgWalk(int layout_, int F, const SgGeo& g) : layout(layout_) {
        if (layout == RECNOW_GNN_BDF) n0 = F, n1 = g.dt;          // (r, dd, f)
        else if (layout == RECNOW_GNN_BFD) n0 = g.dt, n1 = F;     // (r, f, dd)
        else n0 = g.dt, n1 = g.rt;                                // (f, r, dd)
        i0 = 1.0f / (float)n0, i1 = 1.0f / (float)n1;
    }
    __device__ __forceinline__ void at(int idx, int& r, int& dd, int& f) const {
        const int q = sg_div(idx, i0), lo = idx - q * n0, a = sg_div(q, i1), m = q - a * n1;
        const bool bdf = layout == RECNOW_GNN_BDF, bfd = layout == RECNOW_GNN_BFD;       // selects, not stores through the references
        r = bdf || bfd ? a : m;
        dd = bdf ? m : lo;
        f = bdf ? lo : (bfd ? m : a);
    }
};

// global -> LDS: buf[pl * FP + f] = tensor element, 0 for rows >= B and channels >= D (and everywhere when there is no tensor)
__device__ __forceinline__ void sg_load(float* buf, const float* g, const float* const* gl, int layout, bool v4, int64_t b0, int d0, int64_t B,
                                        int F, int D, int FP, const SgGeo& geo) {
    const int lane = threadIdx.x, total = geo.np * F;
    const SgWalk wk(layout, F, geo);
    const bool along_f = layout == RECNOW_GNN_BDF, none = g == nullptr && gl == nullptr;
    if (v4 && !none) {
#pragma unroll 8
        for (int idx = lane * 4; idx < total; idx += SG_LANES * 4) {
            int r, dd, f;
            wk.at(idx, r, dd, f);
            const int64_t b = b0 + r;
            const int d = d0 + dd;
            rn_f4 v = {0.f, 0.f, 0.f, 0.f};
            if (b < B && d < D) {
                const float* p = gl ? gl[f] + b * D + d : g + sg_off(layout, b, f, d, B, F, D);
                v = RN_LD_STREAM((rn_gcf4)p);
            }
            float* o = buf + (r * geo.dt + dd) * FP + f;
            const int st = along_f ? 1 : FP;
            o[0] = v.x, o[st] = v.y, o[2 * st] = v.z, o[3 * st] = v.w;
        }
    } else {
#pragma unroll 8
        for (int idx = lane; idx < total; idx += SG_LANES) {
            int r, dd, f;
            wk.at(idx, r, dd, f);
            const int64_t b = b0 + r;
            const int d = d0 + dd;
            float v = 0.f;
            if (!none && b < B && d < D) {
                const float* p = gl ? gl[f] + b * D + d : g + sg_off(layout, b, f, d, B, F, D);
                v = RN_LD_STREAM((rn_gcf)p);
            }
            buf[(r * geo.dt + dd) * FP + f] = v;
        }
    }
}

// LDS -> global
__device__ __forceinline__ void sg_store(const float* buf, float* g, int layout, bool v4, int64_t b0, int d0, int64_t B, int F, int D, int FP,
                                         const SgGeo& geo) {
    const int lane = threadIdx.x, total = geo.np * F;
    const SgWalk wk(layout, F, geo);
    const bool along_f = layout == RECNOW_GNN_BDF;
    if (v4) {
#pragma unroll 8
        for (int idx = lane * 4; idx < total; idx += SG_LANES * 4) {
            int r, dd, f;
            wk.at(idx, r, dd, f);
            const int64_t b = b0 + r;
            const int d = d0 + dd;
            if (b < B && d < D) {
                const float* o = buf + (r * geo.dt + dd) * FP + f;
                const int st = along_f ? 1 : FP;
                const rn_f4 v = {o[0], o[st], o[2 * st], o[3 * st]};
                RN_ST_STREAM((rn_gf4)(g + sg_off(layout, b, f, d, B, F, D)), v);
            }
        }
    } else {
#pragma unroll 8
        for (int idx = lane; idx < total; idx += SG_LANES) {
            int r, dd, f;
            wk.at(idx, r, dd, f);
            const int64_t b = b0 + r;
            const int d = d0 + dd;
            if (b < B && d < D) RN_ST_STREAM((rn_gf)(g + sg_off(layout, b, f, d, B, F, D)), buf[(r * geo.dt + dd) * FP + f]);
        }
    }
}

__device__ __forceinline__ void sg_tile_origin(int64_t tile, const SgGeo& g, int64_t& b0, int& d0) {
    if (g.ndt == 1) {
        b0 = tile * g.rt, d0 = 0;
    } else {
        b0 = tile / g.ndt, d0 = (int)(tile - b0 * g.ndt) * g.dt;
    }
}

static inline bool sg_aligned(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

static inline SgGeo sg_geo(int64_t B, int D, int npmax) {
    SgGeo g;
    if (D <= npmax) {
        g.dt = D, g.rt = npmax / D, g.ndt = 1;
        g.ntiles = (B + g.rt - 1) / g.rt;
    } else {
        g.rt = 1, g.dt = npmax & ~3, g.ndt = (D + g.dt - 1) / g.dt;
        g.ntiles = B * g.ndt;
    }
    g.np = g.rt * g.dt;
    return g;
}
