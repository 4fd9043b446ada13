// In-batch GAUC, the sort route (rec_block/auc.py, route='sort'; recnow_pair_auc_sorted_terms): the same integers as the walk of pairwise_auc.hip -- the
// definitions at the top of that file hold word for word -- in O(B log B) instead of the sum of squared list lengths.  No pair is looked at: the rows of every
// list are sorted by score and the counts of row i are differences of per-class prefix counts at the ends of its list and of its run of tied scores.
//
// Classes.  Binary rule: class 1 where label > th, else class 0 (a NaN label: 0).  Graded rule: the rank of the label among the distinct non-NaN label values of
//   the taking-part rows of the BATCH (-0.0 and +0.0 are one value), found on the device in a table of 16 values; a NaN label has no class.  A row that does
//   not take part has no class.  More than 16 values: the call is poisoned (below).
// With G(x)[c'] = the number of class-c' rows at positions below x of the (list, score) order, and L(x)[c] = sum over c' < c of G(x)[c'], a row of class c
//   in list [a, e) and tie run [rs, re) has
//     n_i = L(e)[c] - L(a)[c],   c_i = L(rs)[c] - L(a)[c],   t_i = L(re)[c] - L(rs)[c],   and c_i = t_i = 0 where its score is NaN.
//   NaN scores carry the one largest key: they sort last in their list, behind +inf, so no other row counts them as lower or tied.
//
//  1. k_as_keys   a thread per position k of the CALLER's sorted order: key word 0 = seg_id[k], word 1 = the order-preserving image of the score; the row's class
//                 input (binary: the class; graded: the label's key) and whether it takes part; graded: the label's key goes into the value table (a 17-slot
//                 set in LDS per workgroup, then the batch's in global memory; integer compare-and-swap: the SET does not depend on the order of arrival).
//  2. recnow_group_segments(words, n_words = 2, n_words_first = 1): the existing stable radix sort.  Its order is the (list, score) order, its segments are the
//                 runs of equal (list, score).  Word 0 is the caller's seg_id, so list g occupies [seg_first[g], seg_first[g + 1]) here as there.
//  3. k_as_tilecount   a workgroup per tile of RECNOW_AUC_SORT_TILE positions: the class of every position (the rank of its label key in the table), the tile's
//                 count per class (wave ballots, one LDS row per wave).   4. k_as_tilescan (one workgroup, a wave per class): exclusive scan over the tiles.
//  5. k_as_heads  a workgroup per tile: L(x) for every x that heads a run, and L(B), into [run][class].   6. k_as_rows: a thread per position: the four reads
//                 above, the record {n, c, t, takes part} at the row's position k of the caller's order, the three counts by original row.
//  7. k_pa_segsum, k_pa_metric (pairwise_auc.hpp): the walk's own.   8. k_as_poison: where the table overflowed, or the sort of step 2 reported a grid-barrier
//                 time-out (n_seg[0] < 0; it leaves the identity order behind), every output asked for is overwritten: auc, weighted_sum, weight_sum = NaN,
//                 n_lists = -1, every per-row and per-list count = -1 (all B entries).
// Bounds.  Every index read from the caller's arrays or from the sort's is used as the walk's consumers use theirs (order[k] in [0, B), seg_id[k] in [0, B),
//   seg_first[g] in [0, B]); what the sort returns is clamped besides, so the kernels stay inside their buffers on the identity order of a time-out too.
// Integer ballots, counts and compare-and-swaps only; no float atomics; prefix counts are int32 (B < 2**31), list sums int64; bitwise reproducible.
#include <cmath>
#include "common.hpp"
#include "float_key.hpp"
#include "pairwise_auc.hpp"

#define AS_T RECNOW_AUC_SORT_TILE
#define AS_MAXC 16                 // classes under the graded rule (the cap of LabelPairWeightTable)
#define AS_NONE 255u               // no class: the row does not take part, or its label is NaN under the graded rule
#define AS_EMPTY 0xffffffffu       // empty slot of the value table; the key of a NaN
static_assert(AS_T == 1024, "k_as_tilecount / k_as_heads give every position of a tile one of their 1024 threads");

namespace {
struct SortAucWs {
    uint32_t* words;                // [2][B] key words of the inner sort
    uint8_t* solo;                  // [B] zeros
    uint32_t* lab;                  // [B] class input by caller position
    uint8_t* part;                  // [B] takes part, by caller position
    int32_t *order2, *run_id, *run_first, *super2, *nseg2;      // the inner sort's outputs
    uint8_t* cls;                   // [B] class by (list, score) position
    uint32_t* tab;                  // [32] the label values' keys (17 slots used: slot 16 filled = more than 16 values)
    int32_t *tilecnt, *tileoff;     // [tiles][16]
    int32_t* L;                     // [B + 1][16] by run
    int4* nct;                      // [B] {n, c, t, takes part} per caller position
    long long *ln, *lc, *lt, *lr;   // [B] per segment
    void* grp; size_t grp_bytes;    // workspace of the inner sort
    size_t total;
};
SortAucWs as_ws(void* ws, int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1), nt = (size_t)rn_cdiv(n, AS_T);
    RnCarver c(ws, 0);
    SortAucWs a;
    a.words = c.take<uint32_t>(2 * n);
    a.solo = c.take<uint8_t>(n);
    a.lab = c.take<uint32_t>(n);
    a.part = c.take<uint8_t>(n);
    a.order2 = c.take<int32_t>(n);
    a.run_id = c.take<int32_t>(n);
    a.run_first = c.take<int32_t>(n + 1);
    a.super2 = c.take<int32_t>(n);
    a.nseg2 = c.take<int32_t>(2);
    a.cls = c.take<uint8_t>(n);
    a.tab = c.take<uint32_t>(32);
    a.tilecnt = c.take<int32_t>(nt * AS_MAXC);
    a.tileoff = c.take<int32_t>(nt * AS_MAXC);
    a.L = c.take<int32_t>((n + 1) * AS_MAXC);
    a.nct = c.take<int4>(n);
    a.ln = c.take<long long>(n);
    a.lc = c.take<long long>(n);
    a.lt = c.take<long long>(n);
    a.lr = c.take<long long>(n);
    a.grp_bytes = recnow_group_segments_workspace_bytes(B, 2);
    a.grp = c.take<char>(a.grp_bytes);
    a.total = c.off;
    return a;
}

// order-preserving uint32 image of a float (float_key.hpp): a < b <=> key(a) < key(b), -0.0 and +0.0 share a key, every NaN has the one largest key
static_assert(AS_EMPTY == RN_FLOAT_KEY_NAN, "the key of a NaN is the empty slot of the value table");
__device__ __forceinline__ uint32_t as_key(float v) { return rn_float_key(v); }

// `key` into a 17-slot set: the first free slot, unless the key is there already.  A full set drops the key: slot 16 is then filled, which is the overflow flag.
__device__ __forceinline__ void as_insert(uint32_t* tab, uint32_t key) {
    for (int s = 0; s <= AS_MAXC; ++s) {
        const uint32_t cur = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return;
        if (cur == AS_EMPTY) {
            const uint32_t old = atomicCAS(&tab[s], AS_EMPTY, key);
            if (old == AS_EMPTY || old == key) return;
        }
    }
}

__device__ __forceinline__ int as_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
}  // namespace

// ---- 1. keys ------------------------------------------------------------------------------------------------------------------------------
template <int BINARY>
__global__ void __launch_bounds__(256)
k_as_keys(const float* __restrict__ scores, const float* __restrict__ labels, const uint8_t* __restrict__ mask, const int32_t* __restrict__ order,
          const int32_t* __restrict__ seg_id, int64_t B, float th, uint32_t* __restrict__ words, uint32_t* __restrict__ lab, uint8_t* __restrict__ part,
          uint32_t* __restrict__ tab) {
    __shared__ uint32_t s_tab[AS_MAXC + 1];
    if (!BINARY) {
        if (threadIdx.x <= AS_MAXC) s_tab[threadIdx.x] = AS_EMPTY;
        __syncthreads();
    }
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < B) {
        const int32_t row = order[k];
        const float y = labels[row];
        const bool p = mask ? mask[row] != 0 : true;
        words[k] = (uint32_t)seg_id[k];
        words[B + k] = as_key(scores[row]);
        part[k] = p ? 1 : 0;
        if (BINARY) {
            lab[k] = p ? (y > th ? 1u : 0u) : AS_NONE;
        } else {
            const uint32_t key = p ? as_key(y) : AS_EMPTY;
            lab[k] = key;
            if (key != AS_EMPTY) as_insert(s_tab, key);
        }
    }
    if (!BINARY) {
        __syncthreads();
        if (threadIdx.x <= AS_MAXC && s_tab[threadIdx.x] != AS_EMPTY) as_insert(tab, s_tab[threadIdx.x]);
    }
}

// ---- 3. classes and the tiles' counts --------------------------------------------------------------------------------------------------------
// the 16 waves' counts of class c, one LDS row per wave: every thread of the workgroup calls it
template <int NC>
__device__ __forceinline__ void as_wave_counts(unsigned cls, int (*wtot)[AS_MAXC]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const unsigned long long m = __ballot(cls == (unsigned)c);
        if (lane == 0) wtot[w][c] = __popcll(m);
    }
}

template <int NC>
__global__ void __launch_bounds__(AS_T)
k_as_tilecount(const int32_t* __restrict__ order2, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ tab, int64_t B,
               uint8_t* __restrict__ cls_out, int32_t* __restrict__ tilecnt) {
    __shared__ uint32_t s_tab[AS_MAXC];
    __shared__ int wtot[AS_T / 64][AS_MAXC];
    if (NC > 2) {
        if (threadIdx.x < AS_MAXC) s_tab[threadIdx.x] = tab[threadIdx.x];
        __syncthreads();
    }
    const int64_t p = (int64_t)blockIdx.x * AS_T + threadIdx.x;
    unsigned cls = AS_NONE;
    if (p < B) {
        const uint32_t v = lab[as_clamp(order2[p], (int)(B - 1))];
        if (NC == 2) {
            cls = v;
        } else if (v != AS_EMPTY) {
            unsigned r = 0;
#pragma unroll
            for (int j = 0; j < AS_MAXC; ++j) r += s_tab[j] < v ? 1u : 0u;      // (an empty slot holds the largest key: never below v)
            cls = r < AS_MAXC ? r : AS_NONE;                                      // (only an overflowing table, whose call is poisoned, ranks a value 16th)
        }
        cls_out[p] = (uint8_t)cls;
    }
    as_wave_counts<NC>(cls, wtot);
    __syncthreads();
    if (threadIdx.x < NC) {
        int s = 0;
        for (int w = 0; w < AS_T / 64; ++w) s += wtot[w][threadIdx.x];
        tilecnt[(int64_t)blockIdx.x * NC + threadIdx.x] = s;
    }
}

// ---- 4. exclusive scan over the tiles, a wave per class ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_as_tilescan(const int32_t* __restrict__ tilecnt, int nt, int nc, int32_t* __restrict__ tileoff) {
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (c >= nc) return;
    int carry = 0;
    for (int base = 0; base < nt; base += 64) {
        const int i = base + lane;
        const int v = i < nt ? tilecnt[(int64_t)i * nc + c] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (i < nt) tileoff[(int64_t)i * nc + c] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
}

// ---- 5. L(x) at the head of every run, and L(B) --------------------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(AS_T)
k_as_heads(const uint8_t* __restrict__ cls_in, const int32_t* __restrict__ run_id, const int32_t* __restrict__ tileoff, int64_t B,
           int32_t* __restrict__ L) {
    __shared__ int wtot[AS_T / 64][AS_MAXC];
    __shared__ int wbase[AS_T / 64][AS_MAXC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * AS_T + threadIdx.x;
    const bool ok = p < B;
    const unsigned cls = ok ? cls_in[p] : AS_NONE;
    const int r = ok ? as_clamp(run_id[p], (int)(B - 1)) : 0;
    const bool head = ok && (p == 0 || run_id[p - 1] != run_id[p]);
    const bool last = p == B - 1;
    as_wave_counts<NC>(cls, wtot);
    __syncthreads();
    if (threadIdx.x < (AS_T / 64) * NC) {
        const int ww = threadIdx.x / NC, c = threadIdx.x % NC;
        int s = 0;
        for (int j = 0; j < ww; ++j) s += wtot[j][c];
        wbase[ww][c] = s;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    int acc = 0, acc_end = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const unsigned long long m = __ballot(cls == (unsigned)c);
        const int g = tileoff[(int64_t)blockIdx.x * NC + c] + wbase[w][c] + __popcll(m & below);      // G(p)[c]
        if (head) L[(int64_t)r * NC + c] = acc;
        if (last) L[(int64_t)(r + 1) * NC + c] = acc_end;
        acc += g;
        acc_end += g + (cls == (unsigned)c ? 1 : 0);
    }
}

// ---- 6. the rows ---------------------------------------------------------------------------------------------------------------------------------
// the run that begins at position x of the (list, score) order (x heads one wherever the grouping is one), or the slot behind the last run for x = B
__device__ __forceinline__ int64_t as_run_at(const int32_t* __restrict__ run_id, int x, int64_t B) {
    return x < B ? as_clamp(run_id[x], (int)(B - 1)) : (int64_t)as_clamp(run_id[B - 1], (int)(B - 1)) + 1;
}

template <int NC>
__global__ void __launch_bounds__(256)
k_as_rows(const int32_t* __restrict__ order, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
          const int32_t* __restrict__ order2, const int32_t* __restrict__ run_id, const uint8_t* __restrict__ cls_in,
          const uint32_t* __restrict__ words, const uint8_t* __restrict__ part, const int32_t* __restrict__ L, int64_t B, int4* __restrict__ nct,
          int32_t* __restrict__ row_n, int32_t* __restrict__ row_c, int32_t* __restrict__ row_t) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    const int k = as_clamp(order2[p], (int)(B - 1));
    const unsigned c = cls_in[p];
    int n = 0, cc = 0, t = 0;
    if (c != AS_NONE && c > 0) {                                   // class 0 has nothing below it
        const int g = seg_id[k];
        const int a = as_clamp(seg_first[g], (int)B), e = as_clamp(seg_first[g + 1], (int)B);
        const int64_t r = as_clamp(run_id[p], (int)(B - 1));
        const int la = L[as_run_at(run_id, a, B) * NC + c], le = L[as_run_at(run_id, e, B) * NC + c];
        n = le - la;
        if (words[B + k] != AS_EMPTY) {                            // a NaN score is above nobody and ties with nobody
            const int lrs = L[r * NC + c], lre = L[(r + 1) * NC + c];
            cc = lrs - la;
            t = lre - lrs;
        }
    }
    nct[k] = make_int4(n, cc, t, part[k]);
    const int32_t row = order[k];
    if (row_n) row_n[row] = n;
    if (row_c) row_c[row] = cc;
    if (row_t) row_t[row] = t;
}

// ---- 8. poison -----------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_as_poison(const uint32_t* __restrict__ tab, const int32_t* __restrict__ nseg2, int64_t B, int32_t* __restrict__ row_n, int32_t* __restrict__ row_c,
            int32_t* __restrict__ row_t, long long* __restrict__ list_n, long long* __restrict__ list_c, long long* __restrict__ list_t,
            long long* __restrict__ list_rows, float* __restrict__ auc, double* __restrict__ weighted_sum, double* __restrict__ weight_sum,
            long long* __restrict__ n_lists) {
    if (tab[AS_MAXC] == AS_EMPTY && nseg2[0] >= 0) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) {
        if (row_n) row_n[i] = -1;
        if (row_c) row_c[i] = -1;
        if (row_t) row_t[i] = -1;
        if (list_n) list_n[i] = -1;
        if (list_c) list_c[i] = -1;
        if (list_t) list_t[i] = -1;
        if (list_rows) list_rows[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (auc) *auc = NAN;
        if (weighted_sum) *weighted_sum = (double)NAN;
        if (weight_sum) *weight_sum = (double)NAN;
        if (n_lists) *n_lists = -1;
    }
}

extern "C" size_t recnow_pair_auc_sorted_workspace_bytes(int64_t B) {
    if (B < 0) return 0;
    return as_ws(nullptr, B).total;
}

template <int NC>
static void as_launch_counts(const SortAucWs& w, const int32_t* order, const int32_t* seg_id, const int32_t* seg_first, int64_t B, int32_t* row_n,
                             int32_t* row_c, int32_t* row_t, hipStream_t st) {
    const int nt = rn_cdiv(B, AS_T);
    hipLaunchKernelGGL(k_as_tilecount<NC>, nt, AS_T, 0, st, (const int32_t*)w.order2, (const uint32_t*)w.lab, (const uint32_t*)w.tab, B, w.cls, w.tilecnt);
    hipLaunchKernelGGL(k_as_tilescan, 1, 1024, 0, st, (const int32_t*)w.tilecnt, nt, NC, w.tileoff);
    hipLaunchKernelGGL(k_as_heads<NC>, nt, AS_T, 0, st, (const uint8_t*)w.cls, (const int32_t*)w.run_id, (const int32_t*)w.tileoff, B, w.L);
    hipLaunchKernelGGL(k_as_rows<NC>, rn_cdiv(B, 256), 256, 0, st, order, seg_id, seg_first, (const int32_t*)w.order2, (const int32_t*)w.run_id,
                       (const uint8_t*)w.cls, (const uint32_t*)w.words, (const uint8_t*)w.part, (const int32_t*)w.L, B, w.nct, row_n, row_c, row_t);
}

extern "C" int recnow_pair_auc_sorted_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                                            const int32_t* seg_first, int64_t B, int flags, int binary, float pos_neg_th, int weight_kind,
                                            int32_t* row_n, int32_t* row_c, int32_t* row_t, int64_t* list_n, int64_t* list_c, int64_t* list_t,
                                            int64_t* list_rows, float* auc, double* weighted_sum, double* weight_sum, int64_t* n_lists, void* ws,
                                            size_t ws_bytes, void* stream) {
    // RECNOW_PAIR_MEMBERS_PACKED is refused: this route reads no member records, so there is nothing of a count call's to reuse
    if (B < 0 || flags != 0) return RECNOW_EINVAL;
    if (weight_kind != RECNOW_AUC_WEIGHT_ROWS && weight_kind != RECNOW_AUC_WEIGHT_PAIRS && weight_kind != RECNOW_AUC_WEIGHT_UNIFORM)
        return RECNOW_EINVAL;
    if (binary && !std::isfinite(pos_neg_th)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (auc) RN_HIP(hipMemsetAsync(auc, 0, sizeof(float), st));
        if (weighted_sum) RN_HIP(hipMemsetAsync(weighted_sum, 0, sizeof(double), st));
        if (weight_sum) RN_HIP(hipMemsetAsync(weight_sum, 0, sizeof(double), st));
        if (n_lists) RN_HIP(hipMemsetAsync(n_lists, 0, sizeof(int64_t), st));
        return RECNOW_OK;
    }
    if (!seg_id || !seg_first || !ws) return RECNOW_EINVAL;
    if (ws_bytes < recnow_pair_auc_sorted_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    if (!scores || !labels || !order) return RECNOW_EINVAL;
    const SortAucWs w = as_ws(ws, B);
    RN_HIP(hipMemsetAsync(w.solo, 0, (size_t)B, st));
    RN_HIP(hipMemsetAsync(w.tab, 0xff, 32 * sizeof(uint32_t), st));
    const float th = binary ? pos_neg_th : 0.f;
    if (binary)
        hipLaunchKernelGGL(k_as_keys<1>, rn_cdiv(B, 256), 256, 0, st, scores, labels, mask, order, seg_id, B, th, w.words, w.lab, w.part, w.tab);
    else
        hipLaunchKernelGGL(k_as_keys<0>, rn_cdiv(B, 256), 256, 0, st, scores, labels, mask, order, seg_id, B, th, w.words, w.lab, w.part, w.tab);
    RN_LAUNCH_CHECK();
    const int rc = recnow_group_segments(w.words, w.solo, B, 2, 1, w.order2, w.run_id, w.run_first, w.super2, w.nseg2, w.grp, w.grp_bytes, stream);
    if (rc) return rc;
    if (binary) as_launch_counts<2>(w, order, seg_id, seg_first, B, row_n, row_c, row_t, st);
    else as_launch_counts<AS_MAXC>(w, order, seg_id, seg_first, B, row_n, row_c, row_t, st);
    long long* ln = list_n ? (long long*)list_n : w.ln;
    long long* lc = list_c ? (long long*)list_c : w.lc;
    long long* lt = list_t ? (long long*)list_t : w.lt;
    long long* lr = list_rows ? (long long*)list_rows : w.lr;
    pa_launch_sums(seg_id, seg_first, B, (const int4*)w.nct, ln, lc, lt, lr, weight_kind, auc, weighted_sum, weight_sum, n_lists, st);
    const int GP = rn_cdiv(B, 256) < 1024 ? rn_cdiv(B, 256) : 1024;
    hipLaunchKernelGGL(k_as_poison, GP, 256, 0, st, (const uint32_t*)w.tab, (const int32_t*)w.nseg2, B, row_n, row_c, row_t, (long long*)list_n,
                       (long long*)list_c, (long long*)list_t, (long long*)list_rows, auc, weighted_sum, weight_sum, (long long*)n_lists);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
