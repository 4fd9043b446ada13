// The two device buffers of the DCN-v2 layer (dcnmix.hip), each laid out in ONE place.  Host only.
//   MixSaved   what a forward pass keeps for its backward pass (`saved`): one walk over the regions; the same walk over a null base is the size
//   MixWs      the workspace, in the two orders its routes carve it (mix_ws, mix_ws_exact); recnow_dcn_mix_workspace_bytes covers both
// rn_gemm decides by the NUMBER of workspace bytes it is handed whether a product may take the split-precision kernels (gemm.hip), so the size
// behind a GEMM workspace decides bits of the result just as its address does: tests/test_abi.py holds every size to tests/golden/dcn_mix_sizes.npz.
#pragma once
#include <algorithm>
#include <type_traits>
#include "gemm.hpp"
#include "dcnmix_mid.hpp"
#include "dcnmix_tile.hpp"

static inline int ldt_of(int S, int N) {
    const int kc = N * S + N;
    if (kc <= 32) return 32;
    if (kc <= 64) return 64;
    if (kc <= 128) return 128;
    if (kc <= 160) return 160;
    return (kc + 127) / 128 * 128;
}
static inline int kp_of(int S, int N) {            // padded depth of the K = N*S+N products
    const int kc = N * S + N;
    return kc <= 256 ? (kc + 15) / 16 * 16 : (kc + 31) / 32 * 32;
}

struct MixDims {
    int64_t B;
    int D, S, N, L, NS, KC, LDT, KP;   // KC = NS + N; LDT/KP = padded width / depth
    bool exact;                        // exact-128 formulation (side products + rank-N epilogue updates)
};
// Exact formulation: every D-sized product has exactly NS MFMA columns / NS-deep K; the N gate columns and the N
// gate-weighted bias rows are VALU side products / rank-N epilogue updates of the lean 128x128 GEMM kernels.
static inline bool mix_exact(int64_t B, int D, int S, int N) {
    return (N * S) % 128 == 0 && D % 128 == 0 && B % 256 == 0 && N <= 4 && kp_of(S, N) <= 512;     // second outputs: K <= 512
}
static inline MixDims mix_dims(int64_t B, int D, int S, int N, int L) {
    MixDims m;
    m.B = B; m.D = D; m.S = S; m.N = N; m.L = L; m.NS = N * S; m.KC = N * S + N; m.LDT = ldt_of(S, N); m.KP = kp_of(S, N);
    m.exact = mix_exact(B, D, S, N);
    if (m.exact) m.LDT = m.KP;      // [NS main | N gate | zero pad to a multiple of 16]: N = NS products + side product, K = KP products
    return m;
}
static inline size_t act_block(const MixDims& m) { return rn_align((size_t)m.B * m.LDT * sizeof(float)); }      // one (B, LDT) activation
static inline size_t xbuf(const MixDims& m) { return rn_align((size_t)m.B * m.D * sizeof(float)); }             // one (B, D) block

// exact path, L <= MIX_PACK_MAX_L: the packed weights of every layer live in `saved`: the forward packs them ONCE per step (one launch) and the
// backward reads them there instead of packing again.
#define MIX_PACK_MAX_L 8
// shapes the row-block persistent kernels run (dcnmix_tile.hip): `saved` then holds their fragment-ordered packs as well
static inline bool mix_tile_shape(const MixDims& m) {
    return m.exact && m.L <= MIX_PACK_MAX_L && m.L <= RN_TILE_MAX_L && rn_mix_tile_supported(m.B, m.D, m.S, m.N, m.L, m.LDT);
}
// shapes whose packed weights get split-precision piece planes in `saved` (written ONCE per step by the forward -- rn_split_planes_multi behind
// k_pack_all -- instead of by a split launch in front of each of the 12 products that read them)
static inline bool mix_planes_shape(const MixDims& m) { return m.exact && m.L <= MIX_PACK_MAX_L && 4 * m.L <= RN_SPLIT_MAX_JOBS && m.NS == 128 && m.KP == 144; }

// `saved`, in this order (a region a shape does not have is empty):
//   per layer T1 | T2 | T2g                (B, LDT) each
//   x_1 .. x_{L-1}                         (B, D) layer outputs between the layers.  A forward that does not materialise them (mix_xless) leaves the region
//                                          unused; the head-Q forward (dcnmix.hip: mix_head_q) keeps Q = x Wh^T (B, LDT) at its start, see Q()
//   O_0 .. O_{L-1}                         (B, D), exact path: O_l = T2g_l [W; b] is kept next to x_{l+1} = x * O_l (second output of GEMM3), so the
//                                          backward forms dx = sum_l g_l * O_l inside kernels that stream g_l anyway instead of recomputing the products.
//                                          Head-Q forward: O_{L-1} is NOT written (its slot stays free: a backward that needs it recomputes it there)
//   Wc1_0 .. Wc1_{L-1}                     [U_l | K_l | 0] (D x LDT), exact path and L <= MIX_PACK_MAX_L, as are the next two
//   Wc2_0 .. Wc2_{L-1}                     [W_l; b_l; 0] (LDT x D)
//   Wh                                     (LDT x D) the fused head's pre-scaled top-layer weights [W; b]_{L-1} * w_head
//   tile packs                             mix_tile_shape: fragment-ordered weights of the row-block kernels (rn_mix_tile_pack_bytes)
//   per layer P1 | P2 | P3 | P4            mix_planes_shape: piece planes of [U | K] as the B operand of GEMM1, of [W; b] of the product that leaves
//                                          the layer, of W^T -- or the fused head's W * w_head -- of the dT2g product, of [U | K]^T of the product that
//                                          forms g_{l-1}.  Head-Q forward: the top layer has no product that leaves it, its P2 holds the (KP x D) planes
//                                          of Wh instead (the second half of the K = 288 input-gradient product)
//   tile split planes                      mix_tile_shape: piece planes of the split-precision row-block forward (dcnmix_tile_split.hip)
// F = float: the forward's view; F = const float: the backward's (where it packs for itself what its forward left out, the const_cast says so).
template <typename F>
struct MixSavedT {
    typedef typename std::conditional<std::is_const<F>::value, const char, char>::type Byte;
    typedef typename std::conditional<std::is_const<F>::value, const void, void>::type Void;
    Byte* base;
    size_t act, xb, pack, plane_long, plane_short;      // bytes of one activation, one (B, D) block, one packed weight, one long-K / short-K plane set
    size_t x_off, o_off, pack_off, tile_off, plane_off, tile_split_off, total;
    int L;
    MixSavedT(const MixDims& m, Void* p) : base((Byte*)p), act(act_block(m)), xb(xbuf(m)), pack(rn_align((size_t)m.D * m.LDT * sizeof(float))),
          plane_long(rn_gemm_split_planes_bytes(m.D, 128)), plane_short(rn_gemm_split_planes_bytes(m.KP, m.D)), L(m.L) {
        const bool packs = m.exact && m.L <= MIX_PACK_MAX_L, tile = mix_tile_shape(m);
        size_t off = 0;
        auto region = [&off](size_t bytes) { const size_t at = off; off += bytes; return at; };
        region((size_t)L * 3 * act);
        x_off = region((size_t)(L - 1) * xb);
        o_off = region(m.exact ? (size_t)L * xb : 0);
        pack_off = region(packs ? (size_t)(2 * L + 1) * pack : 0);      // (exact path: D % 128 == 0, so the packs are contiguous as k_pack_all writes them)
        tile_off = region(tile ? rn_mix_tile_pack_bytes(m.D, m.S, m.N, m.L, m.LDT) : 0);
        plane_off = region(mix_planes_shape(m) ? (size_t)L * 2 * (plane_long + plane_short) : 0);
        tile_split_off = region(tile ? rn_mix_tile_split_pack_bytes(m.D, m.S, m.N, m.L, m.LDT) : 0);
        total = off;
    }
    F* T1(int l) const { return (F*)(base + (size_t)(3 * l) * act); }
    F* T2(int l) const { return (F*)(base + (size_t)(3 * l + 1) * act); }
    F* T2g(int l) const { return (F*)(base + (size_t)(3 * l + 2) * act); }
    F* x_next(int l) const { return (F*)(base + x_off + (size_t)l * xb); }      // x_{l+1}, l < L - 1
    F* Q() const { return x_next(0); }      // head-Q: (B, LDT), aliases x_1 -- only under mix_xless, L > 1 and LDT <= D (mix_head_q_shape)
    F* O(int l) const { return (F*)(base + o_off + (size_t)l * xb); }
    F* Wc1(int l) const { return (F*)(base + pack_off + (size_t)l * pack); }
    F* Wc2(int l) const { return (F*)(base + pack_off + (size_t)(L + l) * pack); }
    F* Wh() const { return (F*)(base + pack_off + (size_t)2 * L * pack); }
    F* tile_packs() const { return (F*)(base + tile_off); }
    Byte* plane(int l, int which) const {      // which: 0 = P1, 1 = P2, 2 = P3, 3 = P4, stored as long | short | long | short
        return base + plane_off + (size_t)l * 2 * (plane_long + plane_short) + (size_t)((which + 1) / 2) * plane_long + (size_t)(which / 2) * plane_short;
    }
    Byte* tile_split_planes() const { return base + tile_split_off; }
};
// shapes whose fused-head forward may take the score from Q = x Wh^T (dcnmix.hip: mix_head_q): the planes, and room for Q in the x_1 slot
static inline bool mix_head_q_shape(const MixDims& m) { return mix_planes_shape(m) && m.L > 1 && act_block(m) <= xbuf(m); }
typedef MixSavedT<float> MixSaved;
typedef MixSavedT<const float> MixSavedC;

// the largest GEMM workspace any product of the layer asks for
static size_t mix_gemm_ws(const MixDims& m) {
    size_t best = 0;
    recnow_gemm_desc d = rn_gemm_desc_zero();
    const int shapes[6][3] = {{(int)m.B, m.LDT, m.D}, {(int)m.B, m.D, m.KP}, {m.LDT, m.D, (int)m.B}, {m.D, m.LDT, (int)m.B},
                              {m.S, m.S, (int)m.B}, {(int)m.B, m.S, m.S}};
    for (int i = 0; i < 6; ++i) {
        d.M = shapes[i][0]; d.N = shapes[i][1]; d.K = shapes[i][2]; d.batch = (i >= 4) ? m.N : 1;
        const size_t s = rn_gemm_ws_bytes(&d);
        if (s > best) best = s;
    }
    if (m.exact) {           // exact-path split-K products carry 4 side columns per slab row
        d.M = m.D; d.N = m.NS; d.K = (int)m.B; d.batch = 1; d.sp_r = m.N; d.a_trans = 1;
        size_t s = rn_gemm_ws_bytes(&d);
        if (s > best) best = s;
        d.M = (int)m.B; d.N = m.NS; d.K = m.D; d.a_trans = 0;       // x_l U / (x*g) W^T: room for the split-precision planes of the weights
        s = rn_gemm_ws_bytes(&d);
        if (s > best) best = s;
    }
    return best;
}

// The workspace, carved in one of two orders.  A route that does not use a region does not read that member; a member its order does not carve is null.
//   mix_ws        forward and general (not exact) backward:  Wc1, Wc2, dWc1, dWc2, dT2g, dC, dT1, g0, g1, [backward: mid_ws,] gws = the REST of the buffer
//   mix_ws_exact  exact and row-block backward:  Wc1_all, dWc1, dT2g, dC, dT1, g0, g1, slab[0 .. 2], mid_ws, cs_ws, [row-block: dT1_all, dvpart, slab[3 .. 2 L - 1]]
struct MixWs {
    float *Wc1, *Wc2, *dWc1, *dWc2;      // one layer's packed weights [U | K | 0] (D x LDT), [W; b; 0] (LDT x D; rows >= KC are zero) and their gradients
    float* Wc1_all;                      // [U | K | 0] of every layer (L > MIX_PACK_MAX_L only: otherwise the forward's, in `saved`)
    float *dT2g, *dC, *dT1;              // (B, LDT) each.  Forward: free -> the three hold the scoring head's row-dot partials (B x 2D/128), from dT2g on
    float *g0, *g1;                      // (B, D) inter-layer gradient ping-pong
    void *mid_ws, *cs_ws, *gws;          // dV partials per workgroup of the fused sub-space backward; fused head: d bias = sum of dscores; GEMM workspace
    size_t mid_ws_bytes, cs_ws_bytes, gws_bytes;
    // split-K slabs, slab_bytes = mix_gemm_ws each.  Exact backward: [0] the chain stream, [1] the dU product, [2] the dW product (kept until the
    // layer-end reduction).  Row-block backward: [2 l] dW_l, [2 l + 1] dU_l -- one per weight-gradient product: behind the chain launch all 2 L
    // products are independent, and sharing slab buffers made each wait for an earlier layer's reduction (round 5, kernel trace at 8192 rows)
    void* slab[2 * RN_TILE_MAX_L];
    float *dT1_all, *dvpart;             // row-block backward: dT1 of every layer (B, LDT); dV partials [layer][workgroup][N S S]
    int grid;                            // ... and the workgroups of its chain launch
    size_t slab_bytes, pack, act, dv_layer, total;      // (pack, act, dv_layer: floats of one packed weight, one activation, one layer's dV partials; total: bytes carved)
    bool ok;
    float* Wc1_of(int l) const { return Wc1_all + (size_t)l * pack; }
    float* dT1_of(int l) const { return dT1_all + (size_t)l * act; }
    float* dvpart_of(int l) const { return dvpart + (size_t)l * dv_layer; }
};
static inline void mix_ws_grads(const MixDims& m, RnCarver& c, MixWs& w) {      // the run both orders share
    w.dT2g = c.take<float>(w.act); w.dC = c.take<float>(w.act); w.dT1 = c.take<float>(w.act);
    w.g0 = c.take<float>(xbuf(m) / sizeof(float)); w.g1 = c.take<float>(xbuf(m) / sizeof(float));
}
static inline MixWs mix_ws(const MixDims& m, void* ws, size_t ws_bytes, bool backward) {
    MixWs w;
    memset(&w, 0, sizeof(w));
    RnCarver c(ws, ws_bytes);
    w.pack = (size_t)m.D * m.LDT; w.act = act_block(m) / sizeof(float);
    w.Wc1 = c.take<float>(w.pack); w.Wc2 = c.take<float>(w.pack); w.dWc1 = c.take<float>(w.pack); w.dWc2 = c.take<float>(w.pack);
    mix_ws_grads(m, c, w);
    if (backward) { w.mid_ws_bytes = rn_mix_mid_bwd_ws_bytes(m.B, m.S, m.N); w.mid_ws = c.take<char>(w.mid_ws_bytes); }
    w.total = c.off; w.ok = c.ok();
    w.gws = c.base + c.off; w.gws_bytes = w.ok ? ws_bytes - c.off : 0;
    return w;
}
static inline MixWs mix_ws_exact(const MixDims& m, void* ws, size_t ws_bytes, bool tile) {      // tile: the row-block backward's regions too (mix_tile_shape only)
    MixWs w;
    memset(&w, 0, sizeof(w));
    RnCarver c(ws, ws_bytes);
    w.pack = (size_t)m.D * m.LDT; w.act = act_block(m) / sizeof(float);
    w.Wc1_all = c.take<float>((size_t)m.L * w.pack); w.dWc1 = c.take<float>(w.pack);
    mix_ws_grads(m, c, w);
    w.slab_bytes = mix_gemm_ws(m);
    for (int i = 0; i < 3; ++i) w.slab[i] = c.take<char>(w.slab_bytes);
    w.mid_ws_bytes = rn_mix_mid_bwd_ws_bytes(m.B, m.S, m.N); w.mid_ws = c.take<char>(w.mid_ws_bytes);
    w.cs_ws_bytes = rn_colsum_ws_bytes(m.B, 1); w.cs_ws = c.take<char>(w.cs_ws_bytes);
    if (tile) {
        w.grid = rn_mix_tile_bwd_grid(m.B); w.dv_layer = (size_t)w.grid * m.N * m.S * m.S;
        w.dT1_all = c.take<float>((size_t)m.L * w.act); w.dvpart = c.take<float>((size_t)m.L * w.dv_layer);
        for (int i = 3; i < 2 * m.L && i < 2 * RN_TILE_MAX_L; ++i) w.slab[i] = c.take<char>(w.slab_bytes);
    }
    w.total = c.off; w.ok = c.ok() && !(tile && m.L > RN_TILE_MAX_L);
    return w;
}

extern "C" size_t recnow_dcn_mix_workspace_bytes(int64_t B, int D, int S, int N, int L) {
    if (B <= 0 || D <= 0 || S <= 0 || N <= 0 || L <= 0) return 256;
    const MixDims m = mix_dims(B, D, S, N, L);
    const size_t gemm_ws = mix_gemm_ws(m);
    size_t s = 0;
    s += rn_align((size_t)D * m.LDT * sizeof(float));        // Wc1
    s += rn_align((size_t)m.LDT * D * sizeof(float));        // Wc2 (rows >= KC are zero)
    s += rn_align((size_t)D * m.LDT * sizeof(float));        // dWc1
    s += rn_align((size_t)m.LDT * D * sizeof(float));        // dWc2
    s += 3 * act_block(m);                                   // dT2g, dC, dT1
    s += 2 * xbuf(m);                                        // inter-layer gradient ping-pong
    s += 3 * rn_align(gemm_ws);                              // split-K slabs: chain stream, dU and dW (the last two are reduced together at the layer's end)
    s += rn_mix_mid_bwd_ws_bytes(B, S, N);                   // per-workgroup dV partials of the fused sub-space backward
    s += (size_t)L * (rn_align((size_t)D * m.LDT * sizeof(float)) + rn_align((size_t)m.LDT * D * sizeof(float)));   // per-layer packs
    s += rn_align(rn_colsum_ws_bytes(B, 1));                 // fused scoring head: d bias = sum of dscores
    if (mix_tile_shape(m)) {                                 // row-block backward: dT1 of every layer, dV partials per layer and workgroup
        s += (size_t)L * act_block(m);
        s += rn_align((size_t)L * rn_mix_tile_bwd_grid(B) * N * S * S * sizeof(float));
        if (2 * L > 3) s += (size_t)(2 * L - 3) * rn_align(gemm_ws);      // ... and one split-K slab buffer per weight-gradient product (three are above)
    }
    // large enough for every route by construction: the sum above has been an upper bound of both carves for every shape (the golden size sweep)
    return std::max(s + 4096, std::max(mix_ws(m, nullptr, 0, true).total + gemm_ws, mix_ws_exact(m, nullptr, 0, mix_tile_shape(m)).total));
}
