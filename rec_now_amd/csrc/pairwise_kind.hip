// In-batch pairwise loss whose pair term is not softplus(-d): hinge, squared hinge and margin-logistic pairs (hinge_loss_func,
// squared_hinge_loss_func, margin_bpr_loss_func of rec_block/pairwise_loss_from_batch.py) on the sorted segments, as the `pairloss_func` of the
// reference's pairwise_loss (rec_now/rec_block/pairwise_loss_from_batch.py:228-279).  The walks are those of pairwise_table.hip (k_pt_long<WRONG, 1>,
// k_pt_bpr<WRONG>) over two more template parameters:
//
//  * KIND: with d = factor (s_me - s_o) a candidate has u_f = margin - d for the pair (me, o) and u_b = margin + d for the pair (o, me), and
//        hinge            f(u) = max(u, 0)          f'(u) = u > 0 ? 1 : 0       (subgradient 0 at the kink, as torch.relu)
//        squared hinge    f(u) = max(u, 0)^2        f'(u) = 2 max(u, 0)
//        margin-logistic  f(u) = softplus(u)        f'(u) = sigma(u)
//    la += wf f(u_f);  ga += wb f'(u_b) - wf f'(u_f);  dscores[row] = w_occ factor ga / denom.  With a margin the two directions no longer share
//    |d| (|margin - d| != |margin + d|), so the margin-logistic kind pays two exponentials per candidate: exp2, rcp and log2 for the forward
//    direction (loss and gradient), exp2 and rcp for the backward direction (gradient only).
//  * TABLE = 1: direction weights from the K x K table in LDS and the class ids in Member.valid (members as recnow_pair_table_count packs them);
//    TABLE = 0: the default rule -- wf = 1 where label_me > label_o, wb = 1 where label_o > label_me, both ANDed with valid, the wrong-order
//    rule per direction (members as recnow_pair_count packs them: valid is 0 / 1).
//
// Every candidate goes through the selects `w > 0 ? w * term : 0`: a direction that is no pair (masked row, other group rule, the row itself)
// contributes an exact 0 whatever its scores hold; no per-lane branch surrounds the transcendentals.
// Bounds of a walk: as pairwise_table.hip -- a row walks [seg_first[g], seg_first[g + 1]) of its own segment, from the workgroup's LDS stage
// (<= PW_STAGE members) or from the member array (B records); class ids are < 16 by construction, the LDS tables hold 16 x 16 entries.
// No float atomics: per-row terms are written by their row, loss partials per workgroup are summed in fixed order (bitwise reproducible).
#include <cmath>
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_table.hpp"

// pk_f, pk_term (one candidate, both directions) and pk_dirs (the default rule's direction weights) live in pairwise_walk.hpp: the walks of
// pairwise_lambda.hip use them as well.
#define PK_TW (TABLE ? 2 * PT_MAXV * PT_MAXV : 1)

// ---- long segments: a wave per row (k_pt_long<WRONG, 1> over KIND and TABLE) ------------------------------------------------------------
template <int KIND, int TABLE, int WRONG>
__global__ void __launch_bounds__(256)
k_pk_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
          const float* __restrict__ W, int nv, float factor, float margin, float* __restrict__ long_la, float* __restrict__ long_ga) {
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[PK_TW];
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
        if (TABLE && !tab) pt_load_table(W, nv, tw);
        tab = true;
        if (in_lds)
            for (int i = threadIdx.x; i < e - s; i += 256) staged[i] = mem[s + i];
        __syncthreads();
        const int64_t ka = k0 > s ? k0 : (int64_t)s, kb = kl < (int64_t)e - 1 ? kl : (int64_t)e - 1;
        for (int64_t k = ka + w; k <= kb; k += 4) {                 // waves take the segment's rows of this block in turn
            const Member me = mem[k];
            const float* trow = tw + (TABLE ? (PT_CLS(me.valid) << 4) : 0);
            const float* tcol = trow + (TABLE ? PT_MAXV * PT_MAXV : 0);
            float la = 0.f, ga = 0.f;
            PW_WALK_STRIDED(in_lds, staged, s, mem, s + lane, e, j, o, {
                float wf;
                float wb;
                if (TABLE) pt_dirs<WRONG>(me, o, j != (int)k, trow, tcol, wf, wb);
                else pk_dirs<WRONG>(me, o, j != (int)k, wf, wb);
                pk_term<KIND>(me, o, wf, wb, factor, margin, la, ga);
            });
            la = wave_sum(la);
            ga = wave_sum(ga);
            if (lane == 0) {
                long_la[k] = la;
                long_ga[k] = ga;
            }
        }
    }
}

// ---- forward + backward (k_pt_bpr<WRONG> over KIND and TABLE) --------------------------------------------------------------------------
// The occurrence weight cnt_super[super] ** power is uniform within a segment (a segment lies inside one main group), so it multiplies
// the row's sums of both directions.  TABLE and *bad != 0 (a taking-part row with a label outside the values): NaN everywhere.
template <int KIND, int TABLE, int WRONG>
__global__ void __launch_bounds__(256)
k_pk_walk(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
          const int32_t* __restrict__ super_id, const unsigned long long* __restrict__ cnt_super,
          const unsigned long long* __restrict__ n_pair, int64_t B, const float* __restrict__ W, int nv, float factor, float margin, float power,
          int reduce_mean, const float* __restrict__ long_la, const float* __restrict__ long_ga, const unsigned* __restrict__ bad,
          double* __restrict__ block_loss, float* __restrict__ dscores) {
    __shared__ double red[16];
    __shared__ Member staged[PW_STAGE];
    __shared__ float tw[PK_TW];
    if (TABLE) pt_load_table(W, nv, tw);
    int sbase;
    const bool in_lds = stage_members(mem, seg_id, seg_first, B, staged, &sbase);
    if (TABLE && !in_lds) __syncthreads();          // (stage_members synchronises only when it stages)
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool poisoned = TABLE && *bad != 0u;
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
        const bool is_long = e - s > PW_LONG;       // walked by k_pk_long
        const float* trow = tw + (TABLE ? (PT_CLS(me.valid) << 4) : 0);
        const float* tcol = trow + (TABLE ? PT_MAXV * PT_MAXV : 0);
        float la = 0.f, ga = 0.f;
        PW_WALK(in_lds, staged, sbase, mem, (is_long ? e : s), e, j, o, {
            float wf;
            float wb;
            if (TABLE) pt_dirs<WRONG>(me, o, j != (int)k, trow, tcol, wf, wb);
            else pk_dirs<WRONG>(me, o, j != (int)k, wf, wb);
            pk_term<KIND>(me, o, wf, wb, factor, margin, la, ga);
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

// members of the default rule when the caller's workspace does not hold them yet (k_pack_members of pairwise.hip without the counters)
__global__ void k_pk_pack(const float* __restrict__ scores, const float* __restrict__ labels, const uint8_t* __restrict__ mask,
                          const int32_t* __restrict__ order, int64_t B, Member* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < B) out[k] = load_member(scores, labels, mask, order, k);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
namespace {
struct PkArgs {
    const Member* mem;
    const int32_t *seg_id, *seg_first, *super_id;
    const unsigned long long *cnt_super, *n_pair;
    int64_t B;
    const float* table;
    int nv;
    float factor, margin, power;
    int reduce_mean;
    float *long_la, *long_ga;
    const unsigned* bad;
    double* part;
    float* dscores;
};

template <int KIND, int TABLE, int WRONG>
void pk_launch(const PkArgs& a, hipStream_t st) {
    const int G = rn_cdiv(a.B, RN_PW_T), GL = rn_cdiv(a.B, 64);
    hipLaunchKernelGGL((k_pk_long<KIND, TABLE, WRONG>), GL, 256, 0, st, a.mem, a.seg_id, a.seg_first, a.B, a.table, a.nv, a.factor, a.margin,
                       a.long_la, a.long_ga);
    hipLaunchKernelGGL((k_pk_walk<KIND, TABLE, WRONG>), G, RN_PW_T, 0, st, a.mem, a.seg_id, a.seg_first, a.super_id, a.cnt_super, a.n_pair, a.B,
                       a.table, a.nv, a.factor, a.margin, a.power, a.reduce_mean, (const float*)a.long_la, (const float*)a.long_ga, a.bad, a.part,
                       a.dscores);
}

template <int KIND>
void pk_launch_kind(const PkArgs& a, bool table, bool wrong, hipStream_t st) {
    if (table) {
        if (wrong) pk_launch<KIND, 1, 1>(a, st);
        else pk_launch<KIND, 1, 0>(a, st);
    } else {
        if (wrong) pk_launch<KIND, 0, 1>(a, st);
        else pk_launch<KIND, 0, 0>(a, st);
    }
}
}  // namespace

extern "C" int recnow_pair_kind_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                       const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, const int64_t* cnt_super,
                                       const int64_t* n_pair, int64_t B, int flags, int kind, float margin, const float* label_values,
                                       int n_values, const float* table, float factor, float power, int reduce_mean, float* loss,
                                       float* dscores, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || !loss) return RECNOW_EINVAL;
    if (kind != RECNOW_PAIR_KIND_HINGE && kind != RECNOW_PAIR_KIND_SQUARED_HINGE && kind != RECNOW_PAIR_KIND_MARGIN_LOGISTIC) return RECNOW_EINVAL;
    if (!std::isfinite(margin) || !std::isfinite(factor)) return RECNOW_EINVAL;
    if (table) {
        if (n_values < 1 || n_values > PT_MAXV) return RECNOW_EINVAL;
        if (flags & ~(RECNOW_PAIR_WRONG_ORDER | RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
    } else {
        if (!(flags & RECNOW_PAIR_LABEL_GT)) return RECNOW_EINVAL;
        if (flags & ~(RECNOW_PAIR_LABEL_GT | RECNOW_PAIR_WRONG_ORDER | RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        RN_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
        return RECNOW_OK;
    }
    if (!scores || !labels || !order || !seg_id || !seg_first || !super_id || !n_pair || !dscores || !ws) return RECNOW_EINVAL;
    if (table && !label_values) return RECNOW_EINVAL;
    if (power != 0.f && !cnt_super) return RECNOW_EINVAL;
    if (ws_bytes < recnow_pairwise_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    // RECNOW_PAIR_MEMBERS_PACKED: `ws` still holds the members of the matching count call on these inputs -- recnow_pair_table_count (class ids,
    // unknown-label flag) with a table, recnow_pair_count with RECNOW_PAIR_LABEL_GT without one
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) {
        if (table) {
            const int rc = rn_pt_pack_members(scores, labels, mask, order, B, label_values, n_values, pw, st);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_pk_pack, rn_cdiv(B, RN_PW_T), RN_PW_T, 0, st, scores, labels, mask, order, B, pw.mem);
        }
    }
    const PkArgs a = {pw.mem, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super, (const unsigned long long*)n_pair, B, table,
                      table ? n_values : 0, factor, margin, power, reduce_mean, pw.long_la, pw.long_ga, pt_bad_flag(pw, B), pw.part, dscores};
    const bool wrong = (flags & RECNOW_PAIR_WRONG_ORDER) != 0;
    switch (kind) {
        case RECNOW_PAIR_KIND_HINGE: pk_launch_kind<RECNOW_PAIR_KIND_HINGE>(a, table != nullptr, wrong, st); break;
        case RECNOW_PAIR_KIND_SQUARED_HINGE: pk_launch_kind<RECNOW_PAIR_KIND_SQUARED_HINGE>(a, table != nullptr, wrong, st); break;
        default: pk_launch_kind<RECNOW_PAIR_KIND_MARGIN_LOGISTIC>(a, table != nullptr, wrong, st); break;
    }
    RN_LAUNCH_CHECK();
    return rn_pt_finalize(pw.part, rn_cdiv(B, RN_PW_T), n_pair, reduce_mean, loss, st);
}
