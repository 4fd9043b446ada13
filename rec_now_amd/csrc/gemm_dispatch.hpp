// Host-only dispatch logic of the exact-fp32 MFMA GEMM (gemm.hip): rn_gemm_plan turns a descriptor into the ONE route its launch takes -- return
// code, tile family, K split and slabs, kernel family and template arguments (checked against the instantiation lists of gemm_inst_lists.hpp),
// piece planes, grid, remap, slab reduction and profiling tag -- and rnd_ws_bytes is the workspace query on the same helpers.  rn_gemm_impl launches what
// the plan names; recnow_gemm_route returns it without a launch.  No HIP in here and no pointer is dereferenced (addresses are read for their
// alignment only): gemm.hip includes it, and tools/san/dispatch_san.cpp compiles it with plain g++ under -fsanitize=address,undefined to sweep
// descriptors on the CPU box (sanitizer build).  Every run-time switch that feeds the rule comes in through `RnDispatchEnv` so
// that the driver can set it.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/recnow.h"
#include "gemm_inst_lists.hpp"
#include "prof_tags.hpp"

static inline int rnd_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

struct GemmCfg {
    int BM, BN;
};
struct RnDispatchEnv {
    int bm64_max_tiles;      // RECNOW_GEMM_BM64 (default 256; 0 = 64-row tiles off)
    int bm64_kb_mode;        // RECNOW_GEMM_BM64_KB (-1 default, 0 = only to fill the chip, 1 = always)
    int precision;           // rn_gemm_precision(): 0 fp32, 1 bf16x3 (128-row kernels only)
    int staging = 0;         // recnow_set_gemm_staging / RECNOW_GEMM_GLDS: 1 = LDS-DMA operand staging (XF | 32)
    int split_longk = 1;     // RECNOW_SPLIT_LONGK: 0 = no split-precision long-K products (A/B switch; diagnostics: which family an error comes from)
    int split_shortk = 1;    // RECNOW_SPLIT_SHORTK: 0 = no split-precision short-K products (A/B switch)
    int split_lean = 1;      // RECNOW_SPLIT_LEAN: 0 = k_gemm_split of rounds 2-5 only, 1 = k_gemm_s3, 2 = k_gemm_s3 also for the K = B products (A/B switch)
    int s3_pair = 1;         // RECNOW_S3_PAIR: 0 = no paired A loads in k_gemm_s3 (A/B switch)
};
// What a caller of rn_gemm / rn_gemm_deferred states about ONE launch beside its descriptor.
struct RnGemmOpts {
    int slots = 0;                          // workgroup slots the K split aims at (0 = 512); products launched as concurrent pairs ask for 256 (pick_split)
    const void* planes_ready = nullptr;     // the piece planes of this product's B operand (the layout and size its own split would write): that split is skipped
};

static inline GemmCfg pick_cfg(int N) {
    if (N <= 32) return {256, 32};
    if (N <= 64) return {256, 64};
    if (N > 128 && N <= 160) return {128, 160};
    return {128, 128};
}
// Small-M dispatch (round 4): the 128-column products with the two-wide side product -- every long-K product of the DCN-v2 step -- run on
// 64 x 128 tiles when 128-row tiles would leave at most `bm64_max_tiles` output tiles.  Default 256 = the 32 768-, 16 384- and 8192-row shards of the metric's
// 2-, 4- and 8-GPU rows (32 768 rows: 512 tiles in one round without a K split, 1.89 against 1.92 ms per step): at 16 384 rows 256 tiles x 2 K-slices (16 k-tiles each, half the slab traffic) instead of 128 x 4, measured 1.17 against 1.22 ms
// per step; at 8192 rows 128 x 4 fill all 512 workgroup slots where 64 x 4 filled half (the split is capped at 8 k-tiles per slice): 0.78 against
// 0.79 ms (tools/ab_bm64.sh, profiles/r04_small_m.md).  RECNOW_GEMM_BM64 = 0 switches it off, = N sets the tile bound (A/B).
static inline bool wants_bm64(const recnow_gemm_desc* d, const RnDispatchEnv& env) {
    if (d->N != 128 || d->sp_r < 1 || d->sp_r > 2 || d->eu_r > 0 || d->as_out || d->c2_mode || d->mid_V || d->batch != 1 || d->K < 512) return false;
    if (d->M % 64 || env.precision != 0) return false;      // (the opt-in split-precision kernels are 128-row kernels)
    const long long tiles128 = rnd_cdiv(d->M, 128);
    if (tiles128 > env.bm64_max_tiles) return false;
    // few row tiles and a long K (the K = B weight-gradient products, M = D): 64-row tiles where 128-row tiles cannot fill the 512 workgroup slots
    // under the split's cap of 8 k-tiles per slice (B = 8192: 8 tiles x 32 slices) and up to K = 32 768 (the shards: 1.114 against 1.128 ms per step at
    // 16 384 rows, 1.805 against 1.812 at 32 768); at the metric's own K = 65 536 the 128-row tiles are the faster ones (145 against 148 us per launch)
    if (tiles128 < 64 && env.bm64_kb_mode != 1) {
        long long s = (512 + tiles128 - 1) / tiles128;
        const long long maxs = d->K / (8 * 32);
        if (s > maxs) s = maxs;
        return tiles128 * (s > 0 ? s : 1) < 512 || (env.bm64_kb_mode != 0 && d->K <= 32768);
    }
    return true;
}
static inline GemmCfg pick_cfg(const recnow_gemm_desc* d, const RnDispatchEnv& env) {
    GemmCfg c = pick_cfg(d->N);
    if (c.BM == 128 && c.BN == 128 && wants_bm64(d, env)) c.BM = 64;
    return c;
}

// slots = workgroup slots the K split aims to fill: 512 (256 CUs x 2 resident workgroups) for a product that runs alone; 256 for the K = B
// weight-gradient products that dcnmix_bwd_tile launches as concurrent PAIRS on two streams (together they fill the chip with half the slices:
// 16 k-tiles per workgroup instead of 8 and half the slab traffic; 8192 rows 0.705 -> 0.680 ms per step, 16 384 rows 1.125 -> 1.098)
static inline void pick_split(const recnow_gemm_desc* d, const GemmCfg& c, int* splitk, int* kchunk, int slots = 512) {
    const long long tiles = (long long)rnd_cdiv(d->M, c.BM) * rnd_cdiv(d->N, c.BN) * d->batch;
    int s = 1;
    // fused side / second outputs and the rank-R update need the whole K in one workgroup (the slab reduce applies neither)
    const bool whole_k = d->as_out || d->c2_mode || d->mid_V || d->eu_r > 0;
    if (tiles < slots && !whole_k) {
        s = (int)((slots + tiles - 1) / tiles);          // 256 CUs x 2 resident workgroups (256..511 tiles left half the slots empty until round 2)
        const int maxs = d->K / (8 * 32);      // at least 8 k-tiles per slice
        if (s > maxs) s = maxs;
        if (s < 1) s = 1;
    }
    // accuracy, not occupancy: an fp32 accumulator that walks K >= 16384 terms in sequence carries ~sqrt(K) roundings (the K = 32768
    // weight gradients of PLE sat at 0.95 of the 1e-5 parity bound); slabs of <= 8192 terms, summed in fp64 by the reduce, halve that
    if (s == 1 && d->K >= 16384 && !whole_k && d->c_perm_s == 0) s = d->K / 8192;
    int kc = rnd_cdiv(rnd_cdiv(d->K, s), 32) * 32;
    if (kc < 32) kc = 32;
    s = rnd_cdiv(d->K, kc);
    if (s < 1) s = 1;
    *splitk = s;
    *kchunk = kc;
}

// bytes of split-K slabs of a product (0: not split); `align` = the workspace carve granule
static inline size_t rnd_slab_bytes(const recnow_gemm_desc* d, int splitk, size_t align) {
    if (splitk <= 1) return 0;
    const size_t b = (size_t)splitk * d->batch * d->M * (d->N + (d->sp_r > 0 ? 4 : 0)) * sizeof(float);
    return (b + align - 1) / align * align;
}
// what a workspace query reserves: the larger of the two slot targets a launch may run with (fewer slots usually means fewer slices, but a product
// that is not split for occupancy any more may still be split for accuracy: tools/san found M 1000, N 4096, K 32 768 with 4 slices against 2)
static inline size_t rnd_slab_bytes_any(const recnow_gemm_desc* d, const GemmCfg& c, size_t align) {
    int s = 1, kc = 0;
    pick_split(d, c, &s, &kc, 512);
    size_t b = rnd_slab_bytes(d, s, align);
    pick_split(d, c, &s, &kc, 256);
    const size_t b2 = rnd_slab_bytes(d, s, align);
    return b2 > b ? b2 : b;
}

// ---- piece planes of the split-precision (bf16x3) products ------------------------------------------------------------------------------
// three piece planes of (K / 8) x N units of 16 bytes (gemm_split.hip, gemm_shortk.hip: the same layout)
static inline size_t rnd_planes_bytes(int K, int N) { return ((size_t)(K / 8) * N * 16 * 3 + 255) / 256 * 256; }
// products whose B operand the split-precision kernel splits once per launch into global planes (weights: small, L2-resident)
// (round 6: also the (K, 128) activation operand of the K = B weight-gradient products, [k][n] rows of ldb floats -- each of the eight row-tile
// workgroups that read a k-tile of it split it again before)
static inline bool split_planes_shape(const recnow_gemm_desc* d, const RnDispatchEnv& env) {
    return d->sp_r > 0 && d->N == 128 && d->K % 16 == 0 && d->batch == 1 && ((!d->a_trans && d->K <= 4096) || (env.split_lean == 2 && d->a_trans && !d->b_trans));
}
// short-K products whose packed weights the split-precision short-K kernel splits into planes (K = 144: the ring schedule)
static inline bool shortk_planes_shape(const recnow_gemm_desc* d) {
    return d->K == 144 && d->N % 128 == 0 && d->M % 128 == 0 && d->batch == 1 && !d->a_trans && d->sp_r == 0 && d->eu_r == 0;
}
// The workspace query: slabs for either slot target, behind them the planes of a long-K split product (whatever the precision mode is when the product
// runs); the short-K planes start at the workspace's base (a short-K product is never split over K).
static inline size_t rnd_ws_bytes(const recnow_gemm_desc* d, const RnDispatchEnv& env) {
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch <= 0) return 0;
    size_t b = rnd_slab_bytes_any(d, pick_cfg(d, env), 256);
    if (split_planes_shape(d, env)) b += rnd_planes_bytes(d->K, d->N);
    if (shortk_planes_shape(d) && b < rnd_planes_bytes(d->K, d->N)) b = rnd_planes_bytes(d->K, d->N);
    return b;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------
// family: what is launched.  RN_GF_GEMM: k_gemm<BM, BN, WM, WN, BK, A_KC, B_KC, EDGE, A2K, B2K, XF> (gemm_inst_*.hip; WM, WN follow the tile);
// RN_GF_SHORTK / _SHORTK_SPLIT: k_gemm_shortk in fp32 / on piece planes (K = 144), gemm_shortk.hip picks the schedule from K, b_kc, ep, c2_mode;
// RN_GF_SPLIT: k_gemm_split<A_KC, A2K, BP>; RN_GF_S3: k_gemm_s3<A_KC, A2K, PAIR>; RN_GF_NONE: an empty product, nothing to launch
enum RnGemmFamily { RN_GF_NONE = 0, RN_GF_GEMM = 1, RN_GF_SHORTK = 2, RN_GF_SHORTK_SPLIT = 3, RN_GF_SPLIT = 4, RN_GF_S3 = 5 };
struct RnGemmPlan {
    int family, BM, BN, BK, a_kc, b_kc, edge, a2k, b2k, xf;
    int bp, pair;               // the split kernels' BP (RN_GEMM_SPLIT_LIST) and PAIR (paired A loads)
    int ep, c2_mode;            // short-K: ep = (emul ? 1 : 0) | (accumulate ? 2 : 0)
    int planes;                 // 0 none; 1 B is split into the workspace at planes_off first (k_split_planes); 2 the caller's ready planes
    size_t planes_off, slab_bytes;      // the slabs lie at the workspace's base (0 bytes: not split)
    int splitk, kchunk, grid_x, grid_y, grid_z, xcd_remap, tail_pairs;
    int reduce_variant, reduce_blocks;      // k_gemm_splitk_reduce<VEC, QUAD>: 0 <false, false>, 1 <true, false>, 2 <true, true> (splitk > 1)
    int tag;                    // RN_TAG_GEMM_*: names the kernel that runs
};

// "is instantiated": the lists the launchers are expanded from, read as predicates
#define RND_ROW4(AKC, BKC, A2, B2) || (a_kc == AKC && b_kc == BKC && a2k == A2 && b2k == B2)
#define RND_ROW5(AKC, BKC, A2, B2, XFV) || (a_kc == AKC && b_kc == BKC && a2k == A2 && b2k == B2 && xf == XFV)
#define RND_ROW3(AKC, A2, BP) || (a_kc == AKC && a2k == A2 && bp == BP)
static inline bool rnd_has_lean(bool a_kc, bool b_kc, int a2k, int b2k) { return false RN_GEMM_LEAN_LIST(RND_ROW4); }
static inline bool rnd_has_lean64(bool a_kc, bool b_kc, int a2k, int b2k) { return false RN_GEMM_LEAN64_LIST(RND_ROW4); }
static inline bool rnd_has_lean128x(bool a_kc, bool b_kc, int a2k, int b2k, int xf) { return false RN_GEMM_LEAN128X_LIST(RND_ROW5); }
static inline bool rnd_has_lean64x(bool a_kc, bool b_kc, int a2k, int b2k, int xf) { return false RN_GEMM_LEAN64X_LIST(RND_ROW5); }
static inline bool rnd_has_split(bool a_kc, int a2k, int bp) { return false RN_GEMM_SPLIT_LIST(RND_ROW3); }
// is k_gemm<BM, BN, .., BK, A_KC, B_KC, EDGE, A2K, B2K, XF> instantiated? (the edge kernels: gemm_inst_edge.hip, all four families and layouts at BK 32)
static inline bool rnd_has_kgemm(const RnGemmPlan& p) {
    const bool bk_any = p.BK == 16 || p.BK == 32;
    if (p.edge) return p.BK == 32 && p.a2k == -1 && p.b2k == -1 && p.xf == 0 && ((p.BM == 256 && (p.BN == 32 || p.BN == 64)) || (p.BM == 128 && (p.BN == 128 || p.BN == 160)));
    if (p.BM == 64 && p.BN == 128) return p.BK == 32 && rnd_has_lean64x(p.a_kc, p.b_kc, p.a2k, p.b2k, p.xf);
    if (p.BM == 256 && p.BN == 64) return p.BK == 32 && p.xf == 0 && rnd_has_lean64(p.a_kc, p.b_kc, p.a2k, p.b2k);
    if (p.BM == 128 && p.BN == 128 && p.xf) return bk_any && rnd_has_lean128x(p.a_kc, p.b_kc, p.a2k, p.b2k, p.xf);
    if (p.BM == 128 && (p.BN == 128 || p.BN == 160)) return bk_any && rnd_has_lean(p.a_kc, p.b_kc, p.a2k, p.b2k);
    return false;
}
// the persistent short-K kernel's forms (gemm_shortk.hip rn_gemm_launch_shortk): K = 144 runs the ring schedule with second outputs 5 / 6 as well
static inline bool rnd_has_shortk(int K, bool b_kc, int ep, int c2) {
    if (!b_kc && ep == 1) return c2 == 0 || c2 == 1 || c2 == 3;
    if (c2 == 2 || c2 == 4) return b_kc && ep == 0;
    if (c2 == 5 || c2 == 6) return K == 144 && b_kc && ep == 0;
    return c2 == 0 && ep >= 0 && ep <= 3;
}
// ... and on piece planes (rn_gemm_launch_shortk_split, K = 144)
static inline bool rnd_has_shortk_split(bool b_kc, int ep, int c2) {
    if (!b_kc) return (ep == 1 && (c2 == 0 || c2 == 1 || c2 == 3)) || (ep == 0 && c2 == 0);
    return (ep == 2 && c2 == 0) || (ep == 0 && (c2 == 0 || c2 == 2 || c2 == 4 || c2 == 5 || c2 == 6));
}

static inline bool rnd_aligned(const void* p, int64_t ld, int64_t sb) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0) && (sb % 4 == 0); }
// the lean (EDGE = false) kernel needs every tile in bounds and every float4 aligned
static inline bool gemm_interior(const recnow_gemm_desc* d, const GemmCfg& c, int bk, int kchunk, bool split) {
    if (d->M % c.BM || d->N % c.BN || d->K % bk || kchunk % bk) return false;
    if ((int64_t)256 * d->lda >= (1ll << 30) || (int64_t)256 * d->ldb >= (1ll << 30)) return false;      // 32-bit byte offsets inside a tile
    if (!rnd_aligned(d->A, d->lda, d->a_batch_stride) || !rnd_aligned(d->B, d->ldb, d->b_batch_stride)) return false;
    if (d->a_mode == RECNOW_OPMODE_OUTER) { if (d->a_hq % 4) return false; }
    else if (d->a_mode != RECNOW_OPMODE_NONE && !rnd_aligned(d->A2, d->lda, d->a_batch_stride)) return false;
    if (d->b_mode == RECNOW_OPMODE_OUTER) { if (d->b_hq % 4) return false; }
    else if (d->b_mode != RECNOW_OPMODE_NONE && !rnd_aligned(d->B2, d->ldb, d->b_batch_stride)) return false;
    // the lean epilogue is float4 along the columns of C (the split-K slabs always qualify: N is a tile multiple)
    if (!split) {
        if (!d->c_trans && !rnd_aligned(d->C, d->ldc, d->c_batch_stride)) return false;
        if (d->emul && !rnd_aligned(d->emul, d->lde, d->e_batch_stride)) return false;
        if (d->bias && !rnd_aligned(d->bias, 4, d->bias_batch_stride)) return false;
    }
    return true;
}

// The slab reduction of a split product.  Four lanes per output (each a quarter of the slabs) only where one lane per output would leave the chip
// idle: with eight slabs in flight per lane the one-lane form reads faster from 96 workgroups on (c3 layer-end reduction: 19.3 vs 24.1 us).
static inline void rnd_reduce(const recnow_gemm_desc* d, int splitk, int* variant, int* blocks) {
    const int64_t total = (int64_t)d->M * (d->N + (d->sp_r > 0 ? 4 : 0)) * d->batch;
    const int g = rnd_cdiv(total, 256);
    *variant = 0;
    *blocks = g > 2048 ? 2048 : g;
    if (d->N % 4 == 0 && splitk >= 16 && (total / 4) % 64 == 0 && rnd_cdiv(total / 4, 256) < 96) {      // whole quads per wave: the shuffles need all four lanes in the loop
        *variant = 2;
        *blocks = g > 4096 ? 4096 : g;
    } else if (d->N % 4 == 0) {
        *variant = 1;
        *blocks = rnd_cdiv(total / 4, 256) > 2048 ? 2048 : rnd_cdiv(total / 4, 256);
    }
}

// The split-precision long-K kernels (gemm_split.hip): N = 128 (one column tile: the side product belongs to it), k-tiles of 16.
#define RND_SPL_BK 16
#define RND_S3_MAXK 2048      // k_gemm_s3 stages the side weights of a whole k-chunk in LDS: 2 floats per k
// k_gemm_s3 (round 6): N = 128, at most two side columns, whole k-chunks of an even number of k-tiles
static inline bool s3_shape(const recnow_gemm_desc* d, int kchunk) {
    return d->batch == 1 && d->N == 128 && d->sp_r >= 1 && d->sp_r <= 2 && kchunk % (2 * RND_SPL_BK) == 0 && d->K % kchunk == 0 && kchunk <= RND_S3_MAXK &&
           (d->a_mode == RECNOW_OPMODE_NONE || d->a_mode == RECNOW_OPMODE_MUL) && !d->as_out;
}
// Fills the plan with the split-precision kernel of a long-K product that passed split_ok; false: none takes it, the fp32 kernel runs.
static inline bool rnd_plan_split(const recnow_gemm_desc* d, const RnGemmOpts& o, bool has_ws, size_t ws_bytes, const RnDispatchEnv& env, RnGemmPlan* p) {
    if (p->grid_y != 1 || d->K % RND_SPL_BK || p->kchunk % RND_SPL_BK || d->sp_r <= 0) return false;
    if ((int64_t)128 * d->lda >= (1ll << 31) || (int64_t)128 * d->ldb >= (1ll << 31)) return false;      // element offsets inside a tile are 32-bit
    const bool a_kc = p->a_kc != 0, b_kc = p->b_kc != 0;
    // room for the planes of B behind the slabs (rnd_ws_bytes reserves it for these shapes)
    const bool room = split_planes_shape(d, env) && has_ws && ws_bytes >= p->slab_bytes + rnd_planes_bytes(d->K, d->N);
    const bool s3 = env.split_lean != 0 && s3_shape(d, p->kchunk);
    // [k][row] operands (the K = B weight-gradient products) with a pre-split activation operand: built and measured in the step -- 103 / 130 us
    // (A / A * A2) + 18 us for the split of the (B, 128) operand against 111 / 126 us for k_gemm_split, which splits B in every workgroup: the
    // pre-pass costs what the leaner loop gains, so these products stay on k_gemm_split (RECNOW_SPLIT_LEAN=2 routes them to k_gemm_s3: A/B switch)
    if (o.planes_ready && s3 && a_kc) {      // the caller holds the planes of this product's B already (the packed weights of a step are split once, dcnmix.hip)
        p->family = RN_GF_S3;
        p->planes = 2;
    } else if (room && s3 && (a_kc || (!b_kc && env.split_lean == 2))) {
        p->family = RN_GF_S3;
        p->planes = 1;
    } else if (room && d->batch == 1 && a_kc && d->K <= 4096 && rnd_has_split(true, p->a2k, 2)) {
        p->family = RN_GF_SPLIT;
        p->planes = 1;
        p->bp = 2;
    } else if (rnd_has_split(a_kc, p->a2k, b_kc ? 1 : 0)) {
        p->family = RN_GF_SPLIT;
        p->bp = b_kc ? 1 : 0;
    } else {
        return false;
    }
    if (p->planes == 1) p->planes_off = p->slab_bytes;
    // paired A loads of k_gemm_s3: k-contiguous operands, whole groups of four k-tiles, rows that start on a 128-byte line
    p->pair = p->family == RN_GF_S3 && a_kc && env.s3_pair != 0 && p->kchunk % (4 * RND_SPL_BK) == 0 && d->lda % 32 == 0 && ((uintptr_t)d->A & 127) == 0 &&
              (p->a2k == RECNOW_OPMODE_NONE || ((uintptr_t)d->A2 & 127) == 0);
    p->BK = RND_SPL_BK;
    p->tag = RN_TAG_GEMM_SPLIT;
    return true;
}

// The route of recnow_gemm(d, ws, ws_bytes) with the options `o`: the return code the call gives before its first launch and, on RECNOW_OK, what it
// launches.  The checks keep the order they have always had, so that every descriptor gets the code it always got.
static inline int rn_gemm_plan(const recnow_gemm_desc* d, const RnGemmOpts& o, bool has_ws, size_t ws_bytes, const RnDispatchEnv& env, RnGemmPlan* p) {
    memset(p, 0, sizeof(*p));
    if (!d || d->M < 0 || d->N < 0 || d->K < 0 || d->batch < 0) return RECNOW_EINVAL;
    if (d->M == 0 || d->N == 0 || d->batch == 0) return RECNOW_OK;
    if (!d->A || !d->B || !d->C) return RECNOW_EINVAL;
    if ((d->a_mode != RECNOW_OPMODE_NONE && !d->A2) || (d->b_mode != RECNOW_OPMODE_NONE && !d->B2)) return RECNOW_EINVAL;
    if (d->K == 0) return RECNOW_EUNSUPPORTED;
    const GemmCfg c = pick_cfg(d, env);
    if (d->sp_r < 0 || d->sp_r > 4 || d->eu_r < 0 || d->eu_r > 4 || (d->sp_r > 0 && d->eu_r > 0)) return RECNOW_EINVAL;
    if (d->sp_r > 0 && (!d->sp_bx || !d->sp_cx || d->batch != 1)) return RECNOW_EINVAL;
    if (d->eu_r > 0 && (!d->eu_p || !d->eu_q || d->batch != 1)) return RECNOW_EINVAL;
    pick_split(d, c, &p->splitk, &p->kchunk, o.slots > 0 ? o.slots : 512);
    if (d->c_perm_s > 0 && p->splitk <= 1) return RECNOW_EUNSUPPORTED;       // the permuted store lives in the split-K reduce
    if (d->c_perm_s < 0 || (d->c_perm_s > 0 && (d->N % d->c_perm_s || d->batch != 1 || d->c_trans || d->accumulate))) return RECNOW_EINVAL;
    if (d->k_valid < 0 || d->k_valid > d->K) return RECNOW_EINVAL;
    p->tail_pairs = 8;
    if (d->k_valid > 0 && d->K % 16 == 0 && d->k_valid > d->K - 16) p->tail_pairs = (d->k_valid - (d->K - 16) + 1) / 2;      // pairs of the last 16-deep tile
    if ((d->as_in != nullptr) != (d->as_out != nullptr)) return RECNOW_EINVAL;
    if (d->c2_mode < 0 || d->c2_mode > 6 || (d->c2_mode && d->c2_mode != 3 && d->c2_mode < 5 && !d->C2) || ((d->c2_mode == 2 || d->c2_mode >= 4) && !d->E2))
        return RECNOW_EINVAL;
    if (d->c2_mode >= 5) {      // the input gradient in one go: C = acc + E2 * E3 [+ E4 * E5] + rv (x) cv * E6
        if (!d->E3 || !d->E6 || !d->rv || !d->cv || ((uintptr_t)d->cv & 15) || d->lde2 != d->lde3 || d->emul || d->accumulate || (d->c2_mode == 5 && (!d->E4 || !d->E5)))
            return RECNOW_EINVAL;
        if (!rnd_aligned(d->E2, d->lde2, 0) || !rnd_aligned(d->E3, d->lde2, 0) || !rnd_aligned(d->E6, d->lde2, 0) ||
            (d->c2_mode == 5 && (!rnd_aligned(d->E4, d->lde2, 0) || !rnd_aligned(d->E5, d->lde2, 0))))
            return RECNOW_EUNSUPPORTED;
    }
    if (d->c2_mode == 3 && (!d->hv || !d->hp || !d->emul || d->hp_ld < d->N / 64 || ((uintptr_t)d->hv & 15))) return RECNOW_EINVAL;
    if (d->c2_mode == 4 && (!d->E3 || !d->rv || !d->cv || ((uintptr_t)d->cv & 15) || !rnd_aligned(d->E3, d->lde3, 0))) return RECNOW_EINVAL;
    if (d->mid_V) {      // fused sub-space forward: the transposed GEMM1 of DCNMixLayer with two experts of 64 (see recnow_gemm_desc)
        if (!d->mid_T1 || !d->mid_T2 || !d->mid_T2g || d->M != 128 || d->N % 128 || d->sp_r != 2 || !d->a_trans || !d->b_trans || d->a_mode ||
            (d->b_mode != RECNOW_OPMODE_NONE && d->b_mode != RECNOW_OPMODE_MUL) ||
            d->batch != 1 || d->bias || d->emul || d->accumulate || d->c_trans || d->mid_ld % 4 || d->mid_ld < 144 ||
            (((uintptr_t)d->mid_T1 | (uintptr_t)d->mid_T2 | (uintptr_t)d->mid_T2g) & 15))
            return RECNOW_EUNSUPPORTED;
    }
    if (d->c2_mode && (d->K > 512 || d->K % 16 || d->batch != 1)) return RECNOW_EUNSUPPORTED;      // short-K kernel only
    p->slab_bytes = rnd_slab_bytes(d, p->splitk, 256);
    if (p->splitk > 1 && (!has_ws || ws_bytes < p->slab_bytes)) return RECNOW_EWORKSPACE;
    const long long gz = (long long)d->batch * p->splitk;
    if (gz > 65535) return RECNOW_EUNSUPPORTED;
    p->grid_x = rnd_cdiv(d->M, c.BM); p->grid_y = rnd_cdiv(d->N, c.BN); p->grid_z = (int)gz;
    p->xcd_remap = (p->splitk > 1 && d->batch == 1 && p->grid_y == 1 && gz % 8 == 0 && p->grid_x > 1) ? 1 : 0;
    if (!p->xcd_remap && p->grid_y > 1 && p->grid_x % 8 == 0 && d->sp_r == 0 && !d->as_out) p->xcd_remap = 2;
    if (p->splitk > 1) rnd_reduce(d, p->splitk, &p->reduce_variant, &p->reduce_blocks);
    const bool a_kc = d->a_trans == 0, b_kc = d->b_trans != 0;
    p->BM = c.BM; p->BN = c.BN; p->a_kc = a_kc; p->b_kc = b_kc; p->a2k = d->a_mode; p->b2k = d->b_mode;
    p->tag = (c.BM == 256 && c.BN == 32) ? RN_TAG_GEMM_256x32 : (c.BM == 256) ? RN_TAG_GEMM_256x64
           : (c.BN == 160) ? RN_TAG_GEMM_128x160 : (c.BM == 64) ? RN_TAG_GEMM_64x128 : RN_TAG_GEMM_128x128;
    // short-K products (K <= 256, e.g. the K = N*S+N = 130 contractions of DCN-v2) are prologue/epilogue dominated:
    // BK = 16 halves the LDS footprint so 4 workgroups per CU overlap each other's load/store phases.
    const bool short_k = d->K <= 256 || (d->c2_mode && d->K <= 512);
    const bool bk16 = short_k && c.BM == 128;
    p->BK = bk16 ? 16 : 32;
    const bool edge = !gemm_interior(d, c, p->BK, p->kchunk, p->splitk > 1);
    int xf = (d->sp_r > 0 ? 1 : 0) | (d->eu_r > 0 ? 2 : 0);
    if (d->mid_V && (edge || p->splitk != 1 || c.BM != 128 || c.BN != 128 || short_k)) return RECNOW_EUNSUPPORTED;
    // the persistent short-K kernel takes the plain products
    const bool use_shortk = !xf && !d->as_out && !edge && bk16 && c.BN == 128 && a_kc && p->splitk == 1 && d->batch == 1 && d->a_mode == 0 &&
                            d->b_mode == 0 && !d->bias && d->act == RECNOW_ACT_LINEAR && !d->c_trans &&
                            (!d->emul || d->e_mode == RECNOW_OPMODE_MUL);
    // opt-in split precision: the long-K products with a side product (every k_gemm launch of the DCN-v2 step)
    const bool split_ok = env.precision == 1 && env.split_longk != 0 && xf == 1 && !d->as_out && !edge && !bk16 && c.BM == 128 && c.BN == 128 && d->b_mode == 0 &&
                          (d->a_mode == RECNOW_OPMODE_NONE || d->a_mode == RECNOW_OPMODE_MUL) &&
                          ((a_kc && !b_kc && (d->a_mode == 0 || o.planes_ready != nullptr)) || (a_kc && b_kc) || (!a_kc && !b_kc));      // (x0 * O_{l-1}) U: the lean kernel on the caller's planes only
    if (d->as_out) {      // A-stream side output: instantiated with the side product of dT2g; written by the first column tile
        if (xf != 1 || d->a_trans || d->a_mode != RECNOW_OPMODE_MUL || d->batch != 1 || p->splitk != 1 ||
            !rnd_aligned(d->as_in, d->lda, 0) || !rnd_aligned(d->as_out, d->lda, 0))
            return RECNOW_EUNSUPPORTED;
        xf |= 4;
    }
    p->family = RN_GF_GEMM;
    if (xf) {        // side product / rank-R update exist only in the lean 128x128 (and 64x128) kernels: the caller guarantees the shape
        if (edge || (c.BM != 128 && c.BM != 64) || c.BN != 128 || d->c2_mode) return RECNOW_EUNSUPPORTED;
        if (c.BM == 64) {        // small-M dispatch (pick_cfg): 64 x 128 tiles, two-wide side product, fp32 kernels only
            if (xf != 1 || bk16) return RECNOW_EUNSUPPORTED;
            p->xf = 9;
        } else if (split_ok && rnd_plan_split(d, o, has_ws, ws_bytes, env, p)) {
            return RECNOW_OK;
        } else if (d->mid_V) {      // XF 16 | 8 | 1: a kernel of its own, the product's flops + the whole sub-space forward in one launch
            p->a2k = 0; p->xf = 25;
            p->tag = RN_TAG_GEMM_MIDF;
        } else {
            p->xf = xf;
            if (xf == 1 && d->sp_r <= 2 && !bk16) {      // the two-wide side product; LDS-DMA operand staging (XF | 32) where it is switched on and built
                if (env.staging == 1 && !a_kc && !b_kc && d->a_mode == 0 && d->b_mode == 0 && rnd_has_lean128x(a_kc, b_kc, 0, 0, 41)) p->xf = 41;
                else if (rnd_has_lean128x(a_kc, b_kc, d->a_mode, d->b_mode, 9)) p->xf = 9;
            }
        }
        return rnd_has_kgemm(*p) ? RECNOW_OK : RECNOW_EUNSUPPORTED;
    }
    if (use_shortk) {
        // C = (A B) [* emul] [+ C] with a short K: persistent kernel, no per-tile prologue, pipelined epilogue (gemm_shortk.hip)
        if (d->c2_mode && d->c2_mode < 5 && ((d->C2 && !rnd_aligned(d->C2, d->ldc2, 0)) || ((d->c2_mode == 2 || d->c2_mode == 4) && !rnd_aligned(d->E2, d->lde2, 0)))) return RECNOW_EUNSUPPORTED;
        p->ep = (d->emul ? 1 : 0) | (d->accumulate ? 2 : 0);
        p->c2_mode = d->c2_mode;
        p->tag = RN_TAG_GEMM_SHORTK;
        p->BM = p->BN = 128; p->BK = 16;
        if (env.precision == 1 && env.split_shortk != 0 && shortk_planes_shape(d) && (o.planes_ready || (has_ws && ws_bytes >= rnd_planes_bytes(d->K, d->N))) &&
            (int64_t)128 * d->lda < (1ll << 29) && rnd_has_shortk_split(b_kc, p->ep, d->c2_mode)) {
            p->family = RN_GF_SHORTK_SPLIT;
            p->planes = o.planes_ready ? 2 : 1;      // (1: at the workspace's base)
            return RECNOW_OK;
        }
        p->family = RN_GF_SHORTK;
        return rnd_has_shortk(d->K, b_kc, p->ep, d->c2_mode) ? RECNOW_OK : RECNOW_EUNSUPPORTED;
    }
    if (d->c2_mode) return RECNOW_EUNSUPPORTED;          // the second output exists only in the short-K kernel
    // lean kernels exist for the (layout, operand-kind) combos the layers use; anything else (and every edge shape) runs the general kernel of the
    // same tile family
    if (!edge && rnd_has_kgemm(*p)) return RECNOW_OK;
    p->BK = 32; p->edge = 1; p->a2k = p->b2k = -1;
    return RECNOW_OK;
}
