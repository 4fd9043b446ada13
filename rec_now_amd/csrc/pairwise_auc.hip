// In-batch GAUC: the AUC of every list, averaged over the lists (rec_block/auc.py, in_batch_gauc / auc_terms).  Exact integer pair counts from one
// compare-only traversal of every segment on the two route skeletons of pairwise_walk.hpp; no pair list, no host synchronisation.
//
// Lists and rows.  A list is one segment of build_segments(groups).  Only rows that take part are looked at.  A row takes part when mask is true, or
//   when no mask is given.
// Pairs.  For two distinct taking-part rows i, j of one list, (i, j) is a pair
//   - under the graded rule, when label_i > label_j (the default, pos_neg_th=None: the concordance index for graded labels; for 0/1 labels the AUC);
//   - under the binary rule, when label_i > th and not (label_j > th) (pos_neg_th=th, a finite float).
//   Comparisons are float32 and IEEE: a NaN label is in no pair under the graded rule and is a negative under the binary rule.
// Per-row counts, kept by row i as the higher side of the pair, int32:
//   n_i = number of j for which (i, j) is a pair,  c_i = number of pairs with s_i > s_j,  t_i = number of pairs with s_i == s_j.
//   A NaN score makes both comparisons false, so that pair counts as discordant.  A row that does not take part holds 0, 0, 0.
// Per-list counts.  N, C, T are the int64 sums of n_i, c_i, t_i over the list, R is the number of taking-part rows.  The list's AUC is
//   (2C + T) / (2N), formed in fp64 from the integers, for lists with N > 0.  Lists with N = 0 have no AUC and are left out of every batch mean.
// Batch metric.  sum_L w_L AUC_L / sum_L w_L over the lists with N > 0;  w_L = R (RECNOW_AUC_WEIGHT_ROWS, impressions-weighted GAUC), N
//   (RECNOW_AUC_WEIGHT_PAIRS, the pooled share of correctly ordered pairs) or 1 (RECNOW_AUC_WEIGHT_UNIFORM).  0 when no list has N > 0.  The sums
//   are fp64 in a fixed order.
//
//  1. walk (k_pa_long, k_pa_rows<BINARY>: PaAuc on the two route skeletons): a thread per row from the workgroup's LDS stage, a wave per row for
//     segments over PW_LONG, global reads for ranges over PW_STAGE.  Per candidate the label compare(s), two score compares and three integer adds.
//     The counts go by sorted position into the workspace ({n, c, t, takes part}: one 16-byte record) and by original row into the optional outputs.
//  2. per-segment sums (k_pa_segsum): a workgroup per segment (grid-stride over the segments), 256 threads striding the segment, int64 block sums of
//     n, c, t and the row count; no atomics.  k_pa_metric (one workgroup): the fp64 weighted sum and weight sum in fixed order, their float32 ratio
//     and the int64 number of lists counted.
// Bitwise reproducible: integer counts written by their row, integer sums per segment, fixed-order fp64 sums over the segments.
#include <cmath>
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_auc.hpp"

namespace {
// workspace: the pairwise workspace (members, ...: what a count call packs) | the records of this file
struct AucWs {
    int4* long_nct;                 // [B] counts of the rows of long segments (k_pa_long), by sorted position
    int4* nct;                      // [B] {n, c, t, takes part} per sorted row
    long long *ln, *lc, *lt, *lr;   // [B] per segment
};
size_t auc_off(int64_t B) { return rn_align(recnow_pairwise_workspace_bytes(B)); }
size_t auc_bytes(int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1);
    return 2 * rn_align(n * sizeof(int4)) + 4 * rn_align(n * sizeof(long long));
}
AucWs auc_ws(void* ws, size_t ws_bytes, int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1);
    RnCarver c((char*)ws + auc_off(B), ws_bytes - auc_off(B));
    AucWs a;
    a.long_nct = c.take<int4>(n);
    a.nct = c.take<int4>(n);
    a.ln = c.take<long long>(n);
    a.lc = c.take<long long>(n);
    a.lt = c.take<long long>(n);
    a.lr = c.take<long long>(n);
    return a;
}
}  // namespace

// ---- 1. the walk ------------------------------------------------------------------------------------------------------------------------
struct PaRow {
    int n, c, t;
};

template <int BINARY>
struct PaAuc : PwPlain {
    typedef PaRow Row;
    typedef int Out;           // (nothing to sum over the workgroup)
    float th;                  // BINARY: label > th is a positive
    int4* long_nct;            // k_pa_long parks the counts here
    const int4* parked;        // k_pa_rows reads them
    int4* nct;
    int32_t *row_n, *row_c, *row_t;
    __device__ __forceinline__ Row begin(const Member&, int64_t, bool) const { return Row{0, 0, 0}; }
    // Exact: float32 compares and integer adds.  `me` is the higher side of the pair.
    __device__ __forceinline__ void candidate(Row& r, const Member& me, const Member& o, bool other, bool, int, int) const {
        const bool both = other && ((me.valid & o.valid & 1) != 0);
        const bool pair = both && (BINARY ? (me.label > th && !(o.label > th)) : (me.label > o.label));
        r.n += pair ? 1 : 0;
        r.c += (pair && me.score > o.score) ? 1 : 0;
        r.t += (pair && me.score == o.score) ? 1 : 0;
    }
    __device__ __forceinline__ void park(Row& r, int64_t k, int lane) const {
        const int n = wave_sum(r.n), c = wave_sum(r.c), t = wave_sum(r.t);
        if (lane == 0) long_nct[k] = make_int4(n, c, t, 0);
    }
    __device__ __forceinline__ Out finish(Row& r, const Member& me, int64_t k, bool is_long) const {
        if (is_long) {
            const int4 p = parked[k];
            r = Row{p.x, p.y, p.z};
        }
        nct[k] = make_int4(r.n, r.c, r.t, me.valid & 1);
        if (row_n) row_n[me.row] = r.n;
        if (row_c) row_c[me.row] = r.c;
        if (row_t) row_t[me.row] = r.t;
        return 0;
    }
};

// one kernel for both rules (a block-uniform branch around the skeleton): batches without long segments pay one empty launch either way
__global__ void __launch_bounds__(256)
k_pa_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, int binary, float th,
          int4* __restrict__ long_nct) {
    __shared__ Member staged[PW_STAGE];
    if (binary) {
        const PaAuc<1> p = {{}, th, long_nct};
        pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
    } else {
        const PaAuc<0> p = {{}, th, long_nct};
        pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
    }
}

template <int BINARY>
__global__ void __launch_bounds__(256)
k_pa_rows(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, float th,
          const int4* __restrict__ long_nct, int4* __restrict__ nct, int32_t* __restrict__ row_n, int32_t* __restrict__ row_c,
          int32_t* __restrict__ row_t) {
    __shared__ Member staged[PW_STAGE];
    const PaAuc<BINARY> p = {{}, th, nullptr, long_nct, nct, row_n, row_c, row_t};
    pw_thread_rows(mem, seg_id, seg_first, B, staged, p);
}

// ---- 2. per-segment sums and the metric: k_pa_segsum, k_pa_metric (pairwise_auc.hpp, shared with the sort route) -------------------------------

extern "C" size_t recnow_pair_auc_workspace_bytes(int64_t B) {
    if (B < 0) return 0;
    return auc_off(B) + auc_bytes(B);
}

extern "C" int recnow_pair_auc_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, const int32_t* seg_id,
                                     const int32_t* seg_first, int64_t B, int flags, int binary, float pos_neg_th, int weight_kind,
                                     int32_t* row_n, int32_t* row_c, int32_t* row_t, int64_t* list_n, int64_t* list_c, int64_t* list_t,
                                     int64_t* list_rows, float* auc, double* weighted_sum, double* weight_sum, int64_t* n_lists, void* ws,
                                     size_t ws_bytes, void* stream) {
    if (B < 0 || (flags & ~RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
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
    if (ws_bytes < recnow_pair_auc_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    const AucWs aw = auc_ws(ws, ws_bytes, B);
    const int G = rn_cdiv(B, RN_PW_T), GL = rn_cdiv(B, 64);
    // RECNOW_PAIR_MEMBERS_PACKED: `ws` holds the members of a count call on these inputs (recnow_pair_count or recnow_pair_table_count: bit 0 of
    // Member.valid says whether the row takes part either way)
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) {
        if (!scores || !labels || !order) return RECNOW_EINVAL;
        const int rc = rn_pack_members(scores, labels, mask, order, B, pw.mem, st);
        if (rc) return rc;
    }
    const float th = binary ? pos_neg_th : 0.f;
    hipLaunchKernelGGL(k_pa_long, GL, 256, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, binary ? 1 : 0, th, aw.long_nct);
    if (binary)
        hipLaunchKernelGGL(k_pa_rows<1>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, th, (const int4*)aw.long_nct, aw.nct, row_n,
                           row_c, row_t);
    else
        hipLaunchKernelGGL(k_pa_rows<0>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, th, (const int4*)aw.long_nct, aw.nct, row_n,
                           row_c, row_t);
    long long* ln = list_n ? (long long*)list_n : aw.ln;
    long long* lc = list_c ? (long long*)list_c : aw.lc;
    long long* lt = list_t ? (long long*)list_t : aw.lt;
    long long* lr = list_rows ? (long long*)list_rows : aw.lr;
    pa_launch_sums(seg_id, seg_first, B, (const int4*)aw.nct, ln, lc, lt, lr, weight_kind, auc, weighted_sum, weight_sum, n_lists, st);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
