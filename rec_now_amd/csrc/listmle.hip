// In-batch ListMLE (rec_block/listmle.py; recnow_listmle_fwdbwd): the negative log-likelihood of the label-sorted permutation of every list under
// the Plackett-Luce model, on the caller's sorted segments.  No (G, Lmax) matrix, no host synchronisation, lists of any length.
//
// Definitions.  A row takes part when its mask byte is non-zero (or there is no mask) and its label is not NaN.  The permutation of a list is its
//   taking-part rows by label descending (-0.0 == +0.0), ties by ascending row index; n their number, s_1 .. s_n their logits in that order,
//   K = n, or min(topn, n).  A list is valid when n >= 2 and its taking-part rows hold at least two label values.
//     lse_p  = log sum_{q >= p} exp(s_q)                                  (suffix scan)
//     l      = sum_{p <= K} (lse_p - s_p)                                  (times 1 / K with list_mean, times the list's weight)
//     logA_q = log sum_{p <= min(q, K)} exp(-lse_p)                        (prefix scan)
//     dl/ds_q = exp(s_q + logA_q) - [q <= K]
//   A non-finite logit of a taking-part row makes l non-finite (a place behind K adds NaN instead of 0), and every taking-part row of a list whose
//   l is non-finite gets a NaN gradient.  Nothing crosses a list boundary: the scan operators below SELECT on the segment flag.
//
//  1. k_ml_keys      a thread per position k of the CALLER's order: key word 0 = seg_id[k], word 1 = ~rn_float_key(label) (descending), the one largest
//                    key for a row that does not take part (it sorts behind its list's members); the logit and the taking-part byte by position.
//  2. recnow_group_segments(words, 2, 1): stable, and the caller's order is ascending by row inside a list: that is the tie rule.  List g occupies
//                    [seg_first[g], seg_first[g + 1]) in the inner order as in the caller's, so seg_id[p] is the list of inner position p too.
//  3. k_ml_suffix    a workgroup per tile of ML_T positions, thread t at position tile_end - 1 - t: inclusive segmented scan of logaddexp from the
//                    tile's end, the tile's aggregate {a list ends in the tile, value at its first position}.  The heads of lists also write the
//                    list's validity (the members' count from the run of non-members, two label runs among the members) at its first row.
//  4. k_ml_tilescan<MlLse, reverse>  one wave: the carry into every tile.     5. rn_scan of the validity by first row: the valid rank of k_lw_rank.
//  6. k_ml_prefix    a workgroup per tile: applies the suffix carry (lse_p, kept), then the inclusive segmented scan from the tile's start of
//                    {logaddexp of -lse_p, plain fp64 sum of lse_p - s_p} over the places below K.      7. k_ml_tilescan<MlPre, forward>.
//  8. k_ml_rows      a thread per position: applies the prefix carry, writes the gradient base, the row's valid rank and the terms at the row's
//                    original index, and at the list's last position the list's loss (by valid rank, and by segment).
//  9. k_ml_finish    block 0: the mean of the valid lists' losses (fp64, fixed order) and n_valid; all blocks: the gradient divided by n_valid when
//                    `reduce`; where either grouping reported a grid-barrier time-out (n_seg[0] < 0): loss, gradient and per-list losses NaN,
//                    n_valid = -1.
// Bounds.  Every index read from the caller's arrays or from the sort's is clamped, so the identity order of a time-out stays inside the buffers.
// fp64 throughout; no atomics; bitwise reproducible; nothing sized by anything but B.
#include <cmath>
#include "common.hpp"
#include "float_key.hpp"
#include "scan.hpp"

#define ML_T RECNOW_LISTMLE_TILE
static_assert(ML_T == 1024, "k_ml_suffix / k_ml_prefix give every position of a tile one of their 1024 threads");
#define ML_NINF (-__builtin_inf())

namespace {
// ---- the scan operators --------------------------------------------------------------------------------------------------------------------
// log(exp(a) + exp(b)).  -inf is the identity and is SELECTED, so (-inf) - (-inf) is never formed; a NaN on either side comes out as NaN.
__device__ __forceinline__ double ml_lae(double a, double b) {
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo == ML_NINF) return hi;
    return hi + log1p(exp(lo - hi));
}

// state of the suffix scan: f = a list boundary lies at or before this element in scan direction
struct MlLse {
    int f;
    double v;
    static __device__ __forceinline__ MlLse identity() { return {0, ML_NINF}; }
    // `a` comes first in scan direction
    static __device__ __forceinline__ MlLse combine(const MlLse& a, const MlLse& b) { return {a.f | b.f, b.f ? b.v : ml_lae(a.v, b.v)}; }
    static __device__ __forceinline__ MlLse shfl_up(const MlLse& x, int o) { return {__shfl_up(x.f, o, 64), __shfl_up(x.v, o, 64)}; }
    static __device__ __forceinline__ MlLse lane(const MlLse& x, int l) { return {__shfl(x.f, l, 64), __shfl(x.v, l, 64)}; }
};
// state of the prefix scan: a = log sum exp(-lse_p), s = sum (lse_p - s_p), both over the places below K
struct MlPre {
    int f;
    double a, s;
    static __device__ __forceinline__ MlPre identity() { return {0, ML_NINF, 0.0}; }
    static __device__ __forceinline__ MlPre combine(const MlPre& x, const MlPre& y) {
        return {x.f | y.f, y.f ? y.a : ml_lae(x.a, y.a), y.f ? y.s : x.s + y.s};
    }
    static __device__ __forceinline__ MlPre shfl_up(const MlPre& x, int o) {
        return {__shfl_up(x.f, o, 64), __shfl_up(x.a, o, 64), __shfl_up(x.s, o, 64)};
    }
    static __device__ __forceinline__ MlPre lane(const MlPre& x, int l) { return {__shfl(x.f, l, 64), __shfl(x.a, l, 64), __shfl(x.s, l, 64)}; }
};

template <typename S>
__device__ __forceinline__ S ml_wave_scan(S x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const S t = S::shfl_up(x, o);
        if (lane >= o) x = S::combine(t, x);
    }
    return x;
}

// inclusive scan over the ML_T threads of the workgroup in thread order; *total = the last thread's.  lds: ML_T / 64 elements.
template <typename S>
__device__ __forceinline__ S ml_block_scan(S x, S* lds, S* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    x = ml_wave_scan(x);
    if (lane == 63) lds[w] = x;
    __syncthreads();
    if (w == 0) {
        S t = lane < ML_T / 64 ? lds[lane] : S::identity();
        t = ml_wave_scan(t);
        if (lane < ML_T / 64) lds[lane] = t;
    }
    __syncthreads();
    if (w > 0) x = S::combine(lds[w - 1], x);
    *total = lds[ML_T / 64 - 1];
    return x;
}

__device__ __forceinline__ int ml_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the number of taking-part rows of the list at [a, e) of the inner order: they sort in front of the one run of rows that do not
__device__ __forceinline__ int ml_members(int a, int e, const int32_t* __restrict__ order2, const int32_t* __restrict__ run_id,
                                          const int32_t* __restrict__ run_first, const uint8_t* __restrict__ part, int64_t B) {
    if (e <= a) return 0;
    if (part[ml_clamp(order2[e - 1], (int)(B - 1))]) return e - a;
    const int n = ml_clamp(run_first[ml_clamp(run_id[e - 1], (int)(B - 1))], (int)B) - a;
    return n < 0 ? 0 : (n > e - a ? e - a : n);
}

struct MlWs {
    uint32_t* words;                                            // [2][B] key words of the inner sort
    uint8_t *solo, *part;                                       // [B] zeros; takes part, by caller position
    float* sk;                                                  // [B] logit by caller position
    int32_t *order2, *run_id, *run_first, *super2, *nseg2;      // the inner sort's outputs
    int32_t *seg_valid, *valid_at_row, *vscan;                  // [B] by segment; [B + 1] by first row; its exclusive scan, [B] = n_valid
    double *lse, *pa, *ps, *gloss;                              // [B] by inner position (lse: local, then final); [B] loss by valid rank
    MlLse *agg_s, *carry_s;                                     // [tiles]
    MlPre *agg_p, *carry_p;                                     // [tiles]
    void* scan; size_t scan_bytes;
    void* grp; size_t grp_bytes;                                // workspace of the inner sort
    size_t total;
};
MlWs ml_ws(void* ws, int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1), nt = (size_t)rn_cdiv(n, ML_T);
    RnCarver c(ws, 0);
    MlWs w;
    w.words = c.take<uint32_t>(2 * n);
    w.solo = c.take<uint8_t>(n);
    w.part = c.take<uint8_t>(n);
    w.sk = c.take<float>(n);
    w.order2 = c.take<int32_t>(n);
    w.run_id = c.take<int32_t>(n);
    w.run_first = c.take<int32_t>(n + 1);
    w.super2 = c.take<int32_t>(n);
    w.nseg2 = c.take<int32_t>(2);
    w.seg_valid = c.take<int32_t>(n);
    w.valid_at_row = c.take<int32_t>(n + 1);
    w.vscan = c.take<int32_t>(n + 1);
    w.lse = c.take<double>(n);
    w.pa = c.take<double>(n);
    w.ps = c.take<double>(n);
    w.gloss = c.take<double>(n);
    w.agg_s = c.take<MlLse>(nt);
    w.carry_s = c.take<MlLse>(nt);
    w.agg_p = c.take<MlPre>(nt);
    w.carry_p = c.take<MlPre>(nt);
    w.scan_bytes = rn_scan_ws_bytes(B);
    w.scan = c.take<char>(w.scan_bytes);
    w.grp_bytes = recnow_group_segments_workspace_bytes(B, 2);
    w.grp = c.take<char>(w.grp_bytes);
    w.total = c.off;
    return w;
}
}  // namespace

// ---- 1. keys ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ml_keys(const float* __restrict__ labels, const float* __restrict__ logits, const uint8_t* __restrict__ mask, const int32_t* __restrict__ order,
          const int32_t* __restrict__ seg_id, int64_t B, uint32_t* __restrict__ words, float* __restrict__ sk, uint8_t* __restrict__ part) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= B) return;
    const int32_t row = ml_clamp(order[k], (int)(B - 1));
    const float y = labels[row];
    const bool p = (mask ? mask[row] != 0 : true) && y == y;
    words[k] = (uint32_t)seg_id[k];
    words[B + k] = p ? ~rn_float_key(y) : RN_FLOAT_KEY_NAN;      // (the key of +inf is 0xff800000: no member's complement is all ones)
    sk[k] = logits[row];
    part[k] = p ? 1 : 0;
}

// ---- 3. suffix scan inside the tiles, and the lists' validity --------------------------------------------------------------------------------
__global__ void __launch_bounds__(ML_T)
k_ml_suffix(const int32_t* __restrict__ order, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
            const int32_t* __restrict__ order2, const int32_t* __restrict__ run_id, const int32_t* __restrict__ run_first,
            const float* __restrict__ sk, const uint8_t* __restrict__ part, int64_t B, double* __restrict__ lse, MlLse* __restrict__ agg,
            int32_t* __restrict__ seg_valid, int32_t* __restrict__ valid_at_row) {
    __shared__ MlLse lds[ML_T / 64];
    const int64_t p = (int64_t)blockIdx.x * ML_T + (ML_T - 1 - (int)threadIdx.x);      // thread order = from the tile's end to its start
    MlLse x = MlLse::identity();
    if (p < B) {
        const int g = ml_clamp(seg_id[p], (int)(B - 1));
        const int a = ml_clamp(seg_first[g], (int)B), e = ml_clamp(seg_first[g + 1], (int)B);
        const int k = ml_clamp(order2[p], (int)(B - 1));
        x.f = p == e - 1 ? 1 : 0;
        x.v = part[k] ? (double)sk[k] : ML_NINF;
        if (p == a) {
            const int n = ml_members(a, e, order2, run_id, run_first, part, B);
            const int valid = (n >= 2 && run_id[a] != run_id[a + n - 1]) ? 1 : 0;
            seg_valid[g] = valid;
            valid_at_row[ml_clamp(order[a], (int)(B - 1))] = valid;      // order[a]: the list's smallest row (the caller's order is ascending in a list)
        }
    }
    MlLse total;
    x = ml_block_scan(x, lds, &total);
    if (p < B) lse[p] = x.v;
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// ---- 4. / 7. the carry into every tile: exclusive scan over the tiles' aggregates, one wave ---------------------------------------------------
template <typename S, int REVERSE>
__global__ void __launch_bounds__(64)
k_ml_tilescan(const S* __restrict__ agg, int nt, S* __restrict__ carry) {
    const int lane = threadIdx.x;
    S run = S::identity();
    for (int base = 0; base < nt; base += 64) {
        const int i = base + lane;
        const int t = REVERSE ? nt - 1 - i : i;
        const S inc = ml_wave_scan(i < nt ? agg[t] : S::identity());
        S exc = S::shfl_up(inc, 1);
        exc = lane == 0 ? run : S::combine(run, exc);
        if (i < nt) carry[t] = exc;
        run = S::combine(run, S::lane(inc, 63));
    }
}

// ---- 6. lse_p with its carry, and the prefix scan inside the tiles --------------------------------------------------------------------------
__global__ void __launch_bounds__(ML_T)
k_ml_prefix(const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, const int32_t* __restrict__ order2,
            const float* __restrict__ sk, const uint8_t* __restrict__ part, const MlLse* __restrict__ carry_s, int64_t B, int topn,
            double* __restrict__ lse, double* __restrict__ pa, double* __restrict__ ps, MlPre* __restrict__ agg) {
    __shared__ MlPre lds[ML_T / 64];
    const int64_t p = (int64_t)blockIdx.x * ML_T + threadIdx.x;
    MlPre x = MlPre::identity();
    if (p < B) {
        const int g = ml_clamp(seg_id[p], (int)(B - 1));
        const int a = ml_clamp(seg_first[g], (int)B), e = ml_clamp(seg_first[g + 1], (int)B);
        const int k = ml_clamp(order2[p], (int)(B - 1));
        double l = lse[p];
        if ((int64_t)e > ((int64_t)blockIdx.x + 1) * ML_T) l = ml_lae(carry_s[blockIdx.x].v, l);      // the list goes on behind the tile
        lse[p] = l;
        const bool member = part[k] != 0;
        const double s = (double)sk[k];
        const bool in = member && (topn <= 0 || p - a < topn);
        x.f = p == a ? 1 : 0;
        x.a = in ? -l : ML_NINF;
        x.s = in ? l - s : ((member && !isfinite(s)) ? (double)NAN : 0.0);
    }
    MlPre total;
    x = ml_block_scan(x, lds, &total);
    if (p < B) {
        pa[p] = x.a;
        ps[p] = x.s;
    }
    if (threadIdx.x == ML_T - 1) agg[blockIdx.x] = total;
}

// ---- 8. the rows ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ml_rows(const int32_t* __restrict__ order, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
          const int32_t* __restrict__ order2, const int32_t* __restrict__ run_id, const int32_t* __restrict__ run_first,
          const float* __restrict__ sk, const uint8_t* __restrict__ part, const int32_t* __restrict__ seg_valid, const int32_t* __restrict__ vscan,
          const double* __restrict__ lse, const double* __restrict__ pa, const double* __restrict__ ps, const MlPre* __restrict__ carry_p,
          const float* __restrict__ weights, int64_t B, int topn, int list_mean, float* __restrict__ dbase, int32_t* __restrict__ row_rank,
          double* __restrict__ gloss, float* __restrict__ group_loss, int32_t* __restrict__ position, double* __restrict__ row_lse,
          double* __restrict__ list_loss, int32_t* __restrict__ list_valid) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    const int g = ml_clamp(seg_id[p], (int)(B - 1));
    const int a = ml_clamp(seg_first[g], (int)B), e = ml_clamp(seg_first[g + 1], (int)B);
    const int k = ml_clamp(order2[p], (int)(B - 1));
    const int row = ml_clamp(order[k], (int)(B - 1));
    const bool member = part[k] != 0;
    const int n = ml_members(a, e, order2, run_id, run_first, part, B);
    const int K = topn > 0 && topn < n ? topn : n;
    const int valid = seg_valid[g];
    const int vr = valid ? vscan[ml_clamp(order[a], (int)(B - 1))] : -1;
    const double scale = (weights && vr >= 0 ? (double)weights[vr] : 1.0) * (list_mean && K > 0 ? 1.0 / (double)K : 1.0);
    // the list's loss: the sum at its last position (its carry applies when the list began in front of that position's tile)
    const int last = ml_clamp(e > a ? e - 1 : a, (int)(B - 1));
    const int lt = last / ML_T;
    double tot = ps[last];
    if (a < lt * ML_T) tot = carry_p[lt].s + tot;
    const int pos = (int)(p - a);
    if (dbase) {
        double d = 0.0;
        if (valid && member) {
            const int t = (int)(p / ML_T);
            double la = pa[p];
            if (a < t * ML_T) la = ml_lae(carry_p[t].a, la);
            d = isfinite(tot) ? scale * (exp((double)sk[k] + la) - (pos < K ? 1.0 : 0.0)) : (double)NAN;
        }
        dbase[row] = (float)d;
    }
    if (row_rank) row_rank[row] = vr;
    if (position) position[row] = member ? pos : -1;
    if (row_lse) row_lse[row] = member ? lse[p] : (double)NAN;
    if (p == last) {
        if (vr >= 0) {
            gloss[vr] = scale * tot;
            if (group_loss) group_loss[vr] = (float)(scale * tot);
        }
        if (list_loss) list_loss[g] = tot;
        if (list_valid) list_valid[g] = valid;
    }
}

// ---- 9. the mean, the division by n_valid, the poison -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_ml_finish(const double* __restrict__ gloss, const int32_t* __restrict__ vscan, const int32_t* __restrict__ n_seg, const int32_t* __restrict__ nseg2,
            int64_t B, int reduce, float* __restrict__ loss, int32_t* __restrict__ n_valid, float* __restrict__ dbase,
            float* __restrict__ group_loss) {
    __shared__ double red[16];
    const bool bad = n_seg[0] < 0 || nseg2[0] < 0;
    const int nv = vscan[B];
    if (blockIdx.x == 0) {
        double s = 0.0;
        if (loss && !bad)
            for (int i = threadIdx.x; i < nv; i += 256) s += gloss[i];
        s = block_sum<double>(s, red);
        if (threadIdx.x == 0) {
            if (loss) *loss = bad ? NAN : (nv > 0 ? (float)(s / (double)nv) : 0.f);
            if (n_valid) *n_valid = bad ? -1 : nv;
        }
    }
    if (!bad && !(reduce && dbase)) return;
    const float sc = nv > 0 ? 1.f / (float)nv : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) {
        if (bad) {
            if (dbase) dbase[i] = NAN;
            if (group_loss) group_loss[i] = NAN;
        } else {
            dbase[i] *= sc;
        }
    }
}

extern "C" size_t recnow_listmle_workspace_bytes(int64_t B) {
    if (B < 0) return 0;
    return ml_ws(nullptr, B).total;
}

extern "C" int recnow_listmle_fwdbwd(const float* labels, const float* logits, const uint8_t* mask, const float* weights, const int32_t* order,
                                     const int32_t* seg_id, const int32_t* seg_first, const int32_t* n_seg, int64_t B, int topn, int list_mean,
                                     int reduce, float* loss, int32_t* n_valid, float* dbase, int32_t* row_rank, float* group_loss,
                                     int32_t* position, double* row_lse, double* list_loss, int32_t* list_valid, void* ws, size_t ws_bytes,
                                     void* stream) {
    if (B < 0 || topn < 0) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (loss) RN_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
        if (n_valid) RN_HIP(hipMemsetAsync(n_valid, 0, sizeof(int32_t), st));
        return RECNOW_OK;
    }
    if (!order || !seg_id || !seg_first || !n_seg || !ws) return RECNOW_EINVAL;
    if (ws_bytes < recnow_listmle_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    if (!labels || !logits) return RECNOW_EINVAL;
    const MlWs w = ml_ws(ws, B);
    const int nt = rn_cdiv(B, ML_T);
    RN_HIP(hipMemsetAsync(w.solo, 0, (size_t)B, st));
    RN_HIP(hipMemsetAsync(w.valid_at_row, 0, (size_t)(B + 1) * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_ml_keys, rn_cdiv(B, 256), 256, 0, st, labels, logits, mask, order, seg_id, B, w.words, w.sk, w.part);
    RN_LAUNCH_CHECK();
    int rc = recnow_group_segments(w.words, w.solo, B, 2, 1, w.order2, w.run_id, w.run_first, w.super2, w.nseg2, w.grp, w.grp_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ml_suffix, nt, ML_T, 0, st, order, seg_id, seg_first, (const int32_t*)w.order2, (const int32_t*)w.run_id,
                       (const int32_t*)w.run_first, (const float*)w.sk, (const uint8_t*)w.part, B, w.lse, w.agg_s, w.seg_valid, w.valid_at_row);
    hipLaunchKernelGGL((k_ml_tilescan<MlLse, 1>), 1, 64, 0, st, (const MlLse*)w.agg_s, nt, w.carry_s);
    RN_LAUNCH_CHECK();
    if ((rc = rn_scan<int32_t, int32_t, 0>(w.valid_at_row, w.vscan, B, 1, w.scan, w.scan_bytes, st))) return rc;
    hipLaunchKernelGGL(k_ml_prefix, nt, ML_T, 0, st, seg_id, seg_first, (const int32_t*)w.order2, (const float*)w.sk, (const uint8_t*)w.part,
                       (const MlLse*)w.carry_s, B, topn, w.lse, w.pa, w.ps, w.agg_p);
    hipLaunchKernelGGL((k_ml_tilescan<MlPre, 0>), 1, 64, 0, st, (const MlPre*)w.agg_p, nt, w.carry_p);
    hipLaunchKernelGGL(k_ml_rows, rn_cdiv(B, 256), 256, 0, st, order, seg_id, seg_first, (const int32_t*)w.order2, (const int32_t*)w.run_id,
                       (const int32_t*)w.run_first, (const float*)w.sk, (const uint8_t*)w.part, (const int32_t*)w.seg_valid,
                       (const int32_t*)w.vscan, (const double*)w.lse, (const double*)w.pa, (const double*)w.ps, (const MlPre*)w.carry_p, weights, B,
                       topn, list_mean, dbase, row_rank, w.gloss, group_loss, position, row_lse, list_loss, list_valid);
    const int GF = rn_cdiv(B, 256) < 1024 ? rn_cdiv(B, 256) : 1024;
    hipLaunchKernelGGL(k_ml_finish, GF, 256, 0, st, (const double*)w.gloss, (const int32_t*)w.vscan, n_seg, (const int32_t*)w.nseg2, B, reduce, loss,
                       n_valid, dbase, group_loss);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
