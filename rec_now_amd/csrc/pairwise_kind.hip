// In-batch pairwise loss whose pair term is not softplus(-d): hinge, squared hinge and margin-logistic pairs (hinge_loss_func,
// squared_hinge_loss_func, margin_bpr_loss_func of rec_block/pairwise_loss_from_batch.py) on the sorted segments, as the `pairloss_func` of the
// reference's pairwise_loss (rec_now/rec_block/pairwise_loss_from_batch.py:228-279).  This file holds the entry point; the walks are k_pf_long /
// k_pf_walk<TERM, TABLE, WRONG, 0> of pairwise_table.hpp (the kernel pair the table route of BPR and the NDCG walks share) with:
//
//  * TERM, the kind: with d = factor (s_me - s_o) a candidate has u_f = margin - d for the pair (me, o) and u_b = margin + d for the pair (o, me), and
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
// Bounds of a walk: those of pairwise_walk.hpp; class ids are < 16 by construction, the LDS tables hold 16 x 16 entries.
// No float atomics: per-row terms are written by their row, loss partials per workgroup are summed in fixed order (bitwise reproducible).
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_table.hpp"

extern "C" int recnow_pair_kind_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                       const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, const int64_t* cnt_super,
                                       const int64_t* n_pair, int64_t B, int flags, int kind, float margin, const float* label_values,
                                       int n_values, const float* table, float factor, float power, int reduce_mean, float* loss,
                                       float* dscores, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || !loss) return RECNOW_EINVAL;
    if (int rc = pf_check_kind(kind, margin, factor, flags, table, n_values)) return rc;
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
        const int rc = table ? rn_pt_pack_members(scores, labels, mask, order, B, label_values, n_values, pw, st)
                             : rn_pack_members(scores, labels, mask, order, B, pw.mem, st);
        if (rc) return rc;
    }
    const PfArgs a = {pw.mem, nullptr, nullptr, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super, (const unsigned long long*)n_pair, B,
                      table, table ? n_values : 0, factor, margin, power, reduce_mean, pw.long_la, pw.long_ga, pt_bad_flag(pw, B), pw.part, dscores};
    return pf_run_kind<0>(a, kind, (flags & RECNOW_PAIR_WRONG_ORDER) != 0, n_pair, loss, st);
}
