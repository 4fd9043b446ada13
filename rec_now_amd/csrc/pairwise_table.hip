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
//  * bounds of a walk: as in pairwise.hip -- a row walks [seg_first[g], seg_first[g + 1]) of its own segment, read from the workgroup's LDS
//    stage (<= PW_STAGE members) or from the member array (B records); class ids are < 16 by construction (4 bits), the LDS tables hold
//    16 x 16 entries whatever n_values is.
// No float atomics: per-row terms are written by their row, loss partials per workgroup are summed in fixed order (bitwise reproducible).
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_table.hpp"      // PT_* macros, pt_load_table, pt_dirs, pt_bad_flag

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

// One candidate, both directions from one exp(-|d|); hardware exp2 / log2 / rcp and selects instead of per-lane branches, as bpr_term.
__device__ __forceinline__ void pt_term(const Member& me, const Member& o, float wf, float wb, float factor, float& la, float& ga) {
    const float d = factor * (me.score - o.score);
    const float ex = __builtin_amdgcn_exp2f(-1.44269504f * fabsf(d));
    const float inv = __builtin_amdgcn_rcpf(1.f + ex);
    const float lg = 0.69314718f * __builtin_amdgcn_logf(1.f + ex);
    const float lo = ex * inv;
    const float sgn = d >= 0.f ? lo : inv;                                         // sigma(-d)
    const float sgp = d >= 0.f ? inv : lo;                                         // sigma(d)
    la += wf > 0.f ? wf * (fmaxf(-d, 0.f) + lg) : 0.f;                             // w(me, o) softplus(-d)
    ga += (wb > 0.f ? wb * sgp : 0.f) - (wf > 0.f ? wf * sgn : 0.f);
}

// ---- long segments: a wave per row (k_pair_long with the table) -----------------------------------------------------------------
template <int WRONG, int MODE>                     // MODE 0: pair counts;  1: BPR loss and gradient terms
__global__ void __launch_bounds__(256)
k_pt_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
          const float* __restrict__ W, int nv, float factor, int32_t* __restrict__ long_cnt, float* __restrict__ long_la,
          float* __restrict__ long_ga) {
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[2 * PT_MAXV * PT_MAXV];
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    if (k0 >= B) return;
    const int64_t kl = min(B, k0 + 64) - 1;
    const int g0 = seg_id[k0], g1 = seg_id[kl];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool tab = false;
    for (int phase = 0; phase < 2; ++phase) {                       // only the first and the last row's segment can be long (block-uniform)
        if (phase == 1 && g1 == g0) break;
        const int g = phase == 0 ? g0 : g1;
        const int s = seg_first[g], e = seg_first[g + 1];
        if (e - s <= PW_LONG) continue;
        const bool in_lds = e - s <= PW_STAGE;
        __syncthreads();                                            // every wave is done with the previous segment's stage
        if (!tab) pt_load_table(W, nv, tw);
        tab = true;
        if (in_lds)
            for (int i = threadIdx.x; i < e - s; i += 256) staged[i] = mem[s + i];
        __syncthreads();
        const int64_t ka = k0 > s ? k0 : (int64_t)s, kb = kl < (int64_t)e - 1 ? kl : (int64_t)e - 1;
        for (int64_t k = ka + w; k <= kb; k += 4) {                 // waves take the segment's rows of this block in turn
            const Member me = mem[k];
            const float* trow = tw + (PT_CLS(me.valid) << 4);
            const float* tcol = trow + PT_MAXV * PT_MAXV;
            int cc = 0;
            float la = 0.f, ga = 0.f;
            PW_WALK_STRIDED(in_lds, staged, s, mem, s + lane, e, j, o, {
                float wf;
                float wb;
                pt_dirs<WRONG>(me, o, j != (int)k, trow, tcol, wf, wb);
                if (MODE == 0) cc += wf > 0.f ? 1 : 0;
                if (MODE == 1) pt_term(me, o, wf, wb, factor, la, ga);
            });
            if (MODE == 0) {
                cc = wave_sum(cc);
                if (lane == 0) long_cnt[k] = cc;
            } else {
                la = wave_sum(la);
                ga = wave_sum(ga);
                if (lane == 0) {
                    long_la[k] = la;
                    long_ga[k] = ga;
                }
            }
        }
    }
}

// ---- count (k_pair_count with the table) ---------------------------------------------------------------------------------------------
template <int WRONG>
__global__ void __launch_bounds__(256)
k_pt_count(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
           const int32_t* __restrict__ super_id, int64_t B, const float* __restrict__ W, int nv, const int32_t* __restrict__ long_cnt,
           int32_t* __restrict__ cnt_row, unsigned long long* __restrict__ cnt_super, unsigned long long* __restrict__ n_pair,
           unsigned* __restrict__ bad) {
    __shared__ long long red[16];
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[2 * PT_MAXV * PT_MAXV];
    pt_load_table(W, nv, tw);
    int sbase;
    const bool in_lds = stage_members(mem, seg_id, seg_first, B, staged, &sbase);
    if (!in_lds) __syncthreads();                   // (stage_members synchronises only when it stages)
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    long long c = 0;
    if (k < B) {
        const Member me = mem[k];
        const int g = seg_id[k];
        const int s = seg_first[g], e = seg_first[g + 1];
        const bool is_long = e - s > PW_LONG;       // walked by k_pt_long
        const float* trow = tw + (PT_CLS(me.valid) << 4);
        const float* tcol = trow + PT_MAXV * PT_MAXV;
        int cc = 0;
        PW_WALK(in_lds, staged, sbase, mem, (is_long ? e : s), e, j, o, {
            float wf;
            float wb;
            pt_dirs<WRONG>(me, o, j != (int)k, trow, tcol, wf, wb);
            cc += wf > 0.f ? 1 : 0;
        });
        if (is_long) cc = long_cnt[k];
        cnt_row[me.row] = cc;
        if (cc) atomicAdd(&cnt_super[super_id[k]], (unsigned long long)cc);   // integer atomics: order-independent
        if (me.valid & PT_BAD) atomicOr(bad, 1u);
        c = cc;
    }
    c = block_sum<long long>(c, red);
    if (threadIdx.x == 0 && c) atomicAdd(n_pair, (unsigned long long)c);
}

// ---- BPR forward + backward (k_pair_bpr with the table) -------------------------------------------------------------------------------
// The occurrence weight cnt_super[super] ** power is uniform within a segment (a segment lies inside one main group), so it multiplies
// the row's sums of both directions.  *bad != 0 (a taking-part row with a label outside the values): NaN everywhere.
template <int WRONG>
__global__ void __launch_bounds__(256)
k_pt_bpr(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
         const int32_t* __restrict__ super_id, const unsigned long long* __restrict__ cnt_super,
         const unsigned long long* __restrict__ n_pair, int64_t B, const float* __restrict__ W, int nv, float factor, float power,
         int reduce_mean, const float* __restrict__ long_la, const float* __restrict__ long_ga, const unsigned* __restrict__ bad,
         double* __restrict__ block_loss, float* __restrict__ dscores) {
    __shared__ double red[16];
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[2 * PT_MAXV * PT_MAXV];
    pt_load_table(W, nv, tw);
    int sbase;
    const bool in_lds = stage_members(mem, seg_id, seg_first, B, staged, &sbase);
    if (!in_lds) __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool poisoned = *bad != 0u;
    const float qnan = __int_as_float(0x7fc00000);
    double lsum = 0.0;
    if (k < B) {
        const Member me = mem[k];
        const int g = seg_id[k];
        const int s = seg_first[g], e = seg_first[g + 1];
        float w = 1.f;
        if (power != 0.f) {
            const float cnt = (float)cnt_super[super_id[k]];
            // cnt == 0: no pair of this main group survived, the weight is never used (avoid 0**negative = inf -> inf*0)
            w = (cnt == 0.f) ? 1.f : ((power == 1.f) ? cnt : powf(cnt, power));
        }
        const bool is_long = e - s > PW_LONG;       // walked by k_pt_long
        const float* trow = tw + (PT_CLS(me.valid) << 4);
        const float* tcol = trow + PT_MAXV * PT_MAXV;
        float la = 0.f, ga = 0.f;
        PW_WALK(in_lds, staged, sbase, mem, (is_long ? e : s), e, j, o, {
            float wf;
            float wb;
            pt_dirs<WRONG>(me, o, j != (int)k, trow, tcol, wf, wb);
            pt_term(me, o, wf, wb, factor, la, ga);
        });
        if (is_long) {
            la = long_la[k];
            ga = long_ga[k];
        }
        const float denom = reduce_mean ? ((float)(*n_pair) + 1.0e-10f) : 1.f;
        dscores[me.row] = poisoned ? qnan : w * factor * ga / denom;
        lsum = poisoned ? (double)qnan : (double)(w * la);
    }
    lsum = block_sum<double>(lsum, red);
    if (threadIdx.x == 0) block_loss[blockIdx.x] = lsum;
}

__global__ void __launch_bounds__(1024)
k_pt_finalize(const double* __restrict__ part, int n, const unsigned long long* __restrict__ n_pair, int reduce_mean, float* __restrict__ loss) {
    __shared__ double red[16];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[i];     // fixed order per thread, fixed tree
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) {
        float v = (float)s;
        if (reduce_mean) v = v / ((float)(*n_pair) + 1.0e-10f);
        *loss = v;
    }
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
        hipLaunchKernelGGL((k_pt_long<1, 0>), GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, 1.f, pw.long_cnt, pw.long_la, pw.long_ga);
        hipLaunchKernelGGL(k_pt_count<1>, G, RN_PW_T, 0, st, pw.mem, seg_id, seg_first, super_id, B, table, n_values, pw.long_cnt, cnt_row,
                           (unsigned long long*)cnt_super, (unsigned long long*)n_pair, bad);
    } else {
        hipLaunchKernelGGL((k_pt_long<0, 0>), GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, 1.f, pw.long_cnt, pw.long_la, pw.long_ga);
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
    unsigned* bad = pt_bad_flag(pw, B);
    const int G = rn_cdiv(B, RN_PW_T), GL = rn_cdiv(B, 64);
    // RECNOW_PAIR_MEMBERS_PACKED: `ws` still holds the members (class ids, unknown-label flag) recnow_pair_table_count packed from these inputs
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) {
        hipLaunchKernelGGL(k_pt_pack, G, RN_PW_T, 0, st, scores, labels, mask, order, B, label_values, n_values, pw.mem,
                           (unsigned long long*)nullptr, (unsigned long long*)nullptr, bad);
        hipLaunchKernelGGL(k_pt_flag, G, RN_PW_T, 0, st, pw.mem, B, bad);
    }
    if (flags & RECNOW_PAIR_WRONG_ORDER) {
        hipLaunchKernelGGL((k_pt_long<1, 1>), GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, factor, pw.long_cnt, pw.long_la, pw.long_ga);
        hipLaunchKernelGGL(k_pt_bpr<1>, G, RN_PW_T, 0, st, pw.mem, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super,
                           (const unsigned long long*)n_pair, B, table, n_values, factor, power, reduce_mean, pw.long_la, pw.long_ga, bad, pw.part, dscores);
    } else {
        hipLaunchKernelGGL((k_pt_long<0, 1>), GL, 256, 0, st, pw.mem, seg_id, seg_first, B, table, n_values, factor, pw.long_cnt, pw.long_la, pw.long_ga);
        hipLaunchKernelGGL(k_pt_bpr<0>, G, RN_PW_T, 0, st, pw.mem, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super,
                           (const unsigned long long*)n_pair, B, table, n_values, factor, power, reduce_mean, pw.long_la, pw.long_ga, bad, pw.part, dscores);
    }
    hipLaunchKernelGGL(k_pt_finalize, 1, 1024, 0, st, pw.part, G, (const unsigned long long*)n_pair, reduce_mean, loss);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// ---- for pairwise_kind.hip: the packing and finalize kernels above, launched from another translation unit -------------------------------
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

int rn_pt_finalize(const double* part, int n, const int64_t* n_pair, int reduce_mean, float* loss, hipStream_t st) {
    hipLaunchKernelGGL(k_pt_finalize, 1, 1024, 0, st, part, n, (const unsigned long long*)n_pair, reduce_mean, loss);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
