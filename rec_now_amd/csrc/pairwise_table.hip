// In-batch pairwise loss with per-label-pair weights from a K x K table (LabelPairWeightTable of rec_block/pairwise_loss_from_batch.py):
// the label_pair_to_weight_func of the reference (rec_now/rec_block/pairwise_loss_from_batch.py:175-194) for labels that take at most 16
// distinct values.  An element-wise weight function is then fully described by W[a][b] = func(values[a], values[b]), and the segment walks
// of pairwise.hip can look the weight of a candidate up instead of materialising the pairs.
//
//  * class id: found once per row where the members are packed (a linear compare against the <= 16 values) and kept in the spare bits of
//    Member.valid -- bit 0: the row takes part (mask) AND its label is one of the values; bits 1..4: class id; bit 8: the row takes part but
//    its label is NOT among the values (the loss and every gradient entry then come out NaN, never a silent number).
//  * table: 1 KB at most; every workgroup keeps it in LDS as 16 x 16 floats plus its transpose, already reduced to the reference's rule
//    "a pair survives where its weight is > 0" (:193): zero, negative and NaN entries are stored as 0, +inf stays.  A walk reads row
//    class(me) of both copies, indexed by the candidate's class: the weight of (me, o) and of (o, me).
//  * both directions: the walks of pairwise.hip rest on "at most one of (i, j) / (j, i) is a pair".  Here W[a][b] and W[b][a] may both be
//    positive and a positive diagonal pairs tied labels both ways, so every candidate contributes its forward term (me positive: loss and
//    gradient) AND its backward term (me negative: gradient only; the loss term is the other row's forward term).  Both come from ONE
//    exp(-|d|), d = factor (s_me - s_o): log(1 + e) serves softplus(-d) = max(-d, 0) + log(1 + e) and softplus(d) = max(d, 0) + log(1 + e)
//    (= softplus(-d) + d), e / (1 + e) and 1 / (1 + e) are the two sigmoids.
//  * bounds of a walk: those of pairwise_walk.hpp; class ids are < 16 by construction (4 bits), the LDS tables hold 16 x 16 entries whatever
//    n_values is.
// This file holds the packing and flag kernels, the counting kernels (PtCount on the two route skeletons of pairwise_walk.hpp) and the entry points;
// the forward+backward walks are k_pf_long / k_pf_walk<PF_TERM_BPR, 1, WRONG, 0> of pairwise_table.hpp, pt_term there is the term above.
// No float atomics: per-row terms are written by their row, loss partials per workgroup are summed in fixed order (bitwise reproducible).
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_table.hpp"      // PT_* macros, pt_load_table, pt_dirs, pt_bad_flag, the forward+backward kernel pair

// members with class ids; clears the counters the counting kernel adds into (zero_b: B entries, zero_1: one) and the unknown-label flag
__global__ void k_pt_pack(const float* __restrict__ scores, const float* __restrict__ labels, const uint8_t* __restrict__ mask,
                          const int32_t* __restrict__ order, int64_t B, const float* __restrict__ values, int nv, Member* __restrict__ out,
                          unsigned long long* __restrict__ zero_b, unsigned long long* __restrict__ zero_1, unsigned* __restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < B) {
        Member m = load_member(scores, labels, mask, order, k);
        int cls = -1;
        for (int c = 0; c < nv; ++c) cls = (m.label == values[c]) ? c : cls;      // float compare: -0.0 == 0.0; NaN matches nothing
        const int takes = m.valid;
        m.valid = ((takes && cls >= 0) ? 1 : 0) | ((cls < 0 ? 0 : cls) << 1) | ((takes && cls < 0) ? PT_BAD : 0);
        out[k] = m;
        if (zero_b) zero_b[k] = 0ull;
    }
    if (k == 0) {
        if (zero_1) *zero_1 = 0ull;
        *bad = 0u;
    }
}

// raises the unknown-label flag (integer atomic: order-independent); the counting kernel does the same for its own rows
__global__ void k_pt_flag(const Member* __restrict__ mem, int64_t B, unsigned* __restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < B && (mem[k].valid & PT_BAD)) atomicOr(bad, 1u);
}

// ---- count: the table's direction weights, a pair where the forward weight is > 0 (PairCount of pairwise.hip with the table) -----------------
template <int WRONG>
struct PtCount : PwPlain {
    struct Row {
        const float *trow, *tcol;
        int cc;
    };
    typedef long long Out;
    const float* W;
    int nv;
    float* tw;
    int32_t* long_cnt;
    PwCountOut out;
    unsigned* bad;
    __device__ __forceinline__ void once() const { pt_load_table(W, nv, tw); }
    __device__ __forceinline__ Row begin(const Member& me, int64_t, bool) const {
        const float* trow = tw + (PT_CLS(me.valid) << 4);
        return Row{trow, trow + PT_MAXV * PT_MAXV, 0};
    }
    __device__ __forceinline__ void candidate(Row& r, const Member& me, const Member& o, bool other, bool, int, int) const {
        float wf, wb;
        pt_dirs<WRONG>(me, o, other, r.trow, r.tcol, wf, wb);
        r.cc += wf > 0.f ? 1 : 0;
    }
    __device__ __forceinline__ void park(Row& r, int64_t k, int lane) const { pw_park_count(r.cc, k, lane, long_cnt); }
    __device__ __forceinline__ Out finish(Row& r, const Member& me, int64_t k, bool is_long) const {
        if (me.valid & PT_BAD) atomicOr(bad, 1u);
        return out.finish(r.cc, me, k, is_long);
    }
};

template <int WRONG>
__global__ void __launch_bounds__(256)
k_pt_count_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
                const float* __restrict__ W, int nv, int32_t* __restrict__ long_cnt) {
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[2 * PT_MAXV * PT_MAXV];
    const PtCount<WRONG> p = {{}, W, nv, tw, long_cnt, {}, nullptr};
    pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
}

template <int WRONG>
__global__ void __launch_bounds__(256)
k_pt_count(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
           const int32_t* __restrict__ super_id, int64_t B, const float* __restrict__ W, int nv, const int32_t* __restrict__ long_cnt,
           int32_t* __restrict__ cnt_row, unsigned long long* __restrict__ cnt_super, unsigned long long* __restrict__ n_pair,
           unsigned* __restrict__ bad) {
    __shared__ long long red[16];
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[2 * PT_MAXV * PT_MAXV];
    const PtCount<WRONG> p = {{}, W, nv, tw, nullptr, {long_cnt, cnt_row, super_id, cnt_super}, bad};
    pw_add_pairs(pw_thread_rows(mem, seg_id, seg_first, B, staged, p), red, n_pair);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
#define PT_FLAGS_OK(flags) (((flags) & ~(RECNOW_PAIR_WRONG_ORDER | RECNOW_PAIR_MEMBERS_PACKED)) == 0)

extern "C" int recnow_pair_table_count(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                       const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, int64_t B, int flags,
                                       const float* label_values, int n_values, const float* table, int32_t* cnt_row, int64_t* cnt_super,
                                       int64_t* n_pair, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || !n_pair || n_values < 1 || n_values > PT_MAXV || (flags & ~RECNOW_PAIR_WRONG_ORDER)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        RN_HIP(hipMemsetAsync(n_pair, 0, sizeof(int64_t), st));
        return RECNOW_OK;
    }
    if (!scores || !labels || !order || !seg_id || !seg_first || !super_id || !label_values || !table || !cnt_row || !cnt_super || !ws)
        return RECNOW_EINVAL;
    if (ws_bytes < recnow_pairwise_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    unsigned* bad = pt_bad_flag(pw, B);
    const int G = rn_cdiv(B, RN_PW_T), GL = rn_cdiv(B, 64);
    hipLaunchKernelGGL(k_pt_pack, G, RN_PW_T, 0, st, scores, labels, mask, order, B, label_values, n_values, pw.mem,
                       (unsigned long long*)cnt_super, (unsigned long long*)n_pair, bad);
    if (flags & RECNOW_PAIR_WRONG_ORDER) {
        hipLaunchKernelGGL(k_pt_count_long<1>, GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, pw.long_cnt);
        hipLaunchKernelGGL(k_pt_count<1>, G, RN_PW_T, 0, st, pw.mem, seg_id, seg_first, super_id, B, table, n_values, pw.long_cnt, cnt_row,
                           (unsigned long long*)cnt_super, (unsigned long long*)n_pair, bad);
    } else {
        hipLaunchKernelGGL(k_pt_count_long<0>, GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, pw.long_cnt);
        hipLaunchKernelGGL(k_pt_count<0>, G, RN_PW_T, 0, st, pw.mem, seg_id, seg_first, super_id, B, table, n_values, pw.long_cnt, cnt_row,
                           (unsigned long long*)cnt_super, (unsigned long long*)n_pair, bad);
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_pair_table_bpr_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                            const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id,
                                            const int64_t* cnt_super, const int64_t* n_pair, int64_t B, int flags,
                                            const float* label_values, int n_values, const float* table, float factor, float power,
                                            int reduce_mean, float* loss, float* dscores, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || !loss || n_values < 1 || n_values > PT_MAXV || !PT_FLAGS_OK(flags)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        RN_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
        return RECNOW_OK;
    }
    if (!scores || !labels || !order || !seg_id || !seg_first || !super_id || !label_values || !table || !n_pair || !dscores || !ws)
        return RECNOW_EINVAL;
    if (power != 0.f && !cnt_super) return RECNOW_EINVAL;
    if (ws_bytes < recnow_pairwise_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    // RECNOW_PAIR_MEMBERS_PACKED: `ws` still holds the members (class ids, unknown-label flag) recnow_pair_table_count packed from these inputs
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) {
        const int rc = rn_pt_pack_members(scores, labels, mask, order, B, label_values, n_values, pw, st);
        if (rc) return rc;
    }
    const PfArgs a = {pw.mem, nullptr, nullptr, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super, (const unsigned long long*)n_pair, B,
                      table, n_values, factor, 0.f, power, reduce_mean, pw.long_la, pw.long_ga, pt_bad_flag(pw, B), pw.part, dscores};
    if (flags & RECNOW_PAIR_WRONG_ORDER) pf_launch<PF_TERM_BPR, 1, 1, 0>(a, st);
    else pf_launch<PF_TERM_BPR, 1, 0, 0>(a, st);
    RN_LAUNCH_CHECK();
    return rn_loss_finalize(pw.part, rn_cdiv(B, RN_PW_T), n_pair, reduce_mean, loss, st);
}

// ---- the packing kernels above for recnow_pair_table_bpr_fwdbwd and, from another translation unit, pairwise_kind.hip -------------------------------
int rn_pt_pack_members(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, int64_t B, const float* label_values,
                       int n_values, const PairWs& pw, hipStream_t st) {
    unsigned* bad = pt_bad_flag(pw, B);
    const int G = rn_cdiv(B, RN_PW_T);
    hipLaunchKernelGGL(k_pt_pack, G, RN_PW_T, 0, st, scores, labels, mask, order, B, label_values, n_values, pw.mem,
                       (unsigned long long*)nullptr, (unsigned long long*)nullptr, bad);
    hipLaunchKernelGGL(k_pt_flag, G, RN_PW_T, 0, st, pw.mem, B, bad);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
