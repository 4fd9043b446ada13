// Shared by pairwise_table.hip (BPR with a table), pairwise_kind.hip (hinge, squared hinge, margin-logistic) and pairwise_lambda.hip (NDCG pair weights): the
// class id kept in Member.valid, the K x K weight table in LDS, the direction weights of one candidate, and the ONE forward+backward kernel pair of the three
// families, k_pf_long / k_pf_walk over <TERM, TABLE, WRONG, LAMBDA>, with its host-side arguments, dispatch and argument checks.  Each file instantiates only
// what it launches.  The packing, flag and counting kernels stay in pairwise_table.hip; the other two reach the first two through rn_pt_pack_members.
#pragma once
#include <cmath>
#include "common.hpp"
#include "pairwise_walk.hpp"

#define PT_MAXV 16
#define PT_BAD 256
#define PT_CLS(v) (((v) >> 1) & 15)

// tw[0..256): W reduced to "> 0 else 0", row-major with a stride of 16; tw[256..512): its transpose.  The caller synchronises.
__device__ __forceinline__ void pt_load_table(const float* __restrict__ W, int nv, float* tw) {
    for (int i = threadIdx.x; i < PT_MAXV * PT_MAXV; i += blockDim.x) {
        const int a = i >> 4, b = i & 15;
        float w = (a < nv && b < nv) ? W[a * nv + b] : 0.f;
        w = w > 0.f ? w : 0.f;                                                     // zero, negative and NaN drop the pair; +inf keeps it
        tw[i] = w;
        tw[PT_MAXV * PT_MAXV + ((b << 4) | a)] = w;
    }
}

// Weights of the two directions of one candidate: wf of (me, o), wb of (o, me); 0 where that direction is no pair.  trow / tcol: row
// class(me) of the table and of its transpose.  The wrong-order rule ANDs in per direction (reference :197-203).
template <int WRONG>
__device__ __forceinline__ void pt_dirs(const Member& me, const Member& o, bool other, const float* trow, const float* tcol, float& wf, float& wb) {
    const int oc = PT_CLS(o.valid);
    const bool both = other && ((me.valid & o.valid & 1) != 0);
    bool okf = both, okb = both;
    if (WRONG) {
        okf = okf && (me.score < o.score);
        okb = okb && (o.score < me.score);
    }
    const float f = trow[oc], b = tcol[oc];
    wf = okf ? f : 0.f;
    wb = okb ? b : 0.f;
}

// One BPR candidate, both directions from one exp(-|d|); hardware exp2 / log2 / rcp and selects instead of per-lane branches, as bpr_term.
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

// the unknown-label flag lives in the spare member record mem[B] of the pairwise workspace
static inline unsigned* pt_bad_flag(const PairWs& pw, int64_t B) { return reinterpret_cast<unsigned*>(pw.mem + B); }

// k_pt_pack + k_pt_flag (pairwise_table.hip): members with class ids into pw.mem, the unknown-label flag raised or cleared (no counter is touched)
int rn_pt_pack_members(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, int64_t B, const float* label_values,
                       int n_values, const PairWs& pw, hipStream_t st);

// ---- forward + backward of the table, kind and NDCG families ---------------------------------------------------------------------------------
//  * TERM: a RECNOW_PAIR_KIND_* value -- pk_term<TERM>, two directions with a margin (two exponentials for the margin-logistic kind) -- or PF_TERM_BPR:
//    pt_term, BPR with both directions from one exponential (the table route of BPR; BPR with NDCG weights is the margin-logistic kind at margin 0).
//  * TABLE = 1: direction weights from the K x K table in LDS and the class ids in Member.valid (members as recnow_pair_table_count packs them);
//    TABLE = 0: the default rule of pk_dirs (members as recnow_pair_count packs them: valid is 0 / 1); no table is loaded, tw holds one float.
//  * LAMBDA = 1: both weights times |dG| |dD| from the {discount, gain} records, staged beside the members (16 KB); inv multiplies the row's sums once.
// Every candidate goes through the selects `w > 0 ? w * term : 0`: a direction that is no pair (masked row, other group rule, the row itself; weight
// 0, or NaN from 0 * inf) contributes an exact 0 whatever its scores and records hold; no per-lane branch surrounds the transcendentals (lanes of a
// wave walk segments of different membership: both sides would be serialised).  Class ids are < 16 by construction (4 bits), the LDS tables hold
// 16 x 16 entries whatever n_values is.  TABLE and *bad != 0 (a taking-part row with a label outside the values): NaN everywhere.
#define PF_TERM_BPR 0
template <int TERM, int TABLE, int WRONG, int LAMBDA>
struct PfWalk {
    struct Row {
        const float *trow, *tcol;
        PairAux ma;
        float w, la, ga;
        bool poisoned;
    };
    typedef double Out;
    const PairAux* aux;
    const float* W;
    int nv;
    float factor, margin;
    float* tw;
    PairAux* saux;
    float *long_la, *long_ga;
    PwRowEnd<TABLE != 0, LAMBDA != 0> end;
    __device__ __forceinline__ void once() const {
        if (TABLE) pt_load_table(W, nv, tw);
    }
    __device__ __forceinline__ void stage(int i, int k) const {
        if (LAMBDA) saux[i] = aux[k];
    }
    __device__ __forceinline__ Row begin(const Member& me, int64_t k, bool wave) const {
        Row r = {};
        if (LAMBDA) r.ma = aux[k];
        r.w = wave ? 1.f : end.weight(k);
        r.poisoned = !wave && end.poison();
        r.trow = tw + (TABLE ? (PT_CLS(me.valid) << 4) : 0);
        r.tcol = r.trow + (TABLE ? PT_MAXV * PT_MAXV : 0);
        return r;
    }
    __device__ __forceinline__ void candidate(Row& r, const Member& me, const Member& o, bool other, bool in_lds, int i, int j) const {
        float wf, wb;
        if (TABLE) pt_dirs<WRONG>(me, o, other, r.trow, r.tcol, wf, wb);
        else pk_dirs<WRONG>(me, o, other, wf, wb);
        if (LAMBDA) {
            const PairAux oa = in_lds ? saux[i] : aux[j];
            const float lam = fabsf(r.ma.gain - oa.gain) * fabsf(r.ma.discount - oa.discount);
            wf *= lam;
            wb *= lam;
        }
        if (TERM == PF_TERM_BPR) pt_term(me, o, wf, wb, factor, r.la, r.ga);
        else pk_term<TERM>(me, o, wf, wb, factor, margin, r.la, r.ga);
    }
    __device__ __forceinline__ void park(Row& r, int64_t k, int lane) const { pw_park_sums(r.la, r.ga, k, lane, long_la, long_ga); }
    __device__ __forceinline__ Out finish(Row& r, const Member& me, int64_t k, bool is_long) const { return end.finish(me, k, is_long, r.w, r.la, r.ga, r.poisoned); }
};
#define PF_LDS                                             \
    __shared__ Member staged[PW_STAGE];                    \
    __shared__ PairAux saux[LAMBDA ? PW_STAGE : 1];        \
    __shared__ float tw[TABLE ? 2 * PT_MAXV * PT_MAXV : 1]

template <int TERM, int TABLE, int WRONG, int LAMBDA>
__global__ void __launch_bounds__(256)
k_pf_long(const Member* __restrict__ mem, const PairAux* __restrict__ aux, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
          int64_t B, const float* __restrict__ W, int nv, float factor, float margin, float* __restrict__ long_la, float* __restrict__ long_ga) {
    PF_LDS;
    const PfWalk<TERM, TABLE, WRONG, LAMBDA> p = {aux, W, nv, factor, margin, tw, saux, long_la, long_ga, {}};
    pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
}

template <int TERM, int TABLE, int WRONG, int LAMBDA>
__global__ void __launch_bounds__(256)
k_pf_walk(const Member* __restrict__ mem, const PairAux* __restrict__ aux, const float* __restrict__ inv, const int32_t* __restrict__ seg_id,
          const int32_t* __restrict__ seg_first, const int32_t* __restrict__ super_id, const unsigned long long* __restrict__ cnt_super,
          const unsigned long long* __restrict__ n_pair, int64_t B, const float* __restrict__ W, int nv, float factor, float margin, float power,
          int reduce_mean, const float* __restrict__ long_la, const float* __restrict__ long_ga, const unsigned* __restrict__ bad,
          double* __restrict__ block_loss, float* __restrict__ dscores) {
    __shared__ double red[16];
    PF_LDS;
    const PfWalk<TERM, TABLE, WRONG, LAMBDA> p = {aux, W, nv, factor, margin, tw, saux, nullptr, nullptr,
        {super_id, cnt_super, n_pair, inv, factor, power, reduce_mean, bad, long_la, long_ga, dscores}};
    pw_store_block_loss(pw_thread_rows(mem, seg_id, seg_first, B, staged, p), red, block_loss);
}

// ---- host side of the pair ----------------------------------------------------------------------------------------------------------------------
struct PfArgs {
    const Member* mem;
    const PairAux* aux;      // LAMBDA: the records and 1 / IDCG per sorted row (recnow_pair_lambda_terms); else NULL
    const float* inv;
    const int32_t *seg_id, *seg_first, *super_id;
    const unsigned long long *cnt_super, *n_pair;
    int64_t B;
    const float* table;      // NULL: the default rule
    int nv;
    float factor, margin, power;
    int reduce_mean;
    float *long_la, *long_ga;
    const unsigned* bad;
    double* part;
    float* dscores;
};

template <int TERM, int TABLE, int WRONG, int LAMBDA>
static void pf_launch(const PfArgs& a, hipStream_t st) {
    const int G = rn_cdiv(a.B, RN_PW_T), GL = rn_cdiv(a.B, 64);
    hipLaunchKernelGGL((k_pf_long<TERM, TABLE, WRONG, LAMBDA>), GL, 256, 0, st, a.mem, a.aux, a.seg_id, a.seg_first, a.B, a.table, a.nv, a.factor,
                       a.margin, a.long_la, a.long_ga);
    hipLaunchKernelGGL((k_pf_walk<TERM, TABLE, WRONG, LAMBDA>), G, RN_PW_T, 0, st, a.mem, a.aux, a.inv, a.seg_id, a.seg_first, a.super_id, a.cnt_super,
                       a.n_pair, a.B, a.table, a.nv, a.factor, a.margin, a.power, a.reduce_mean, (const float*)a.long_la, (const float*)a.long_ga,
                       a.bad, a.part, a.dscores);
}

// the long and the thread-per-row launch of <kind, a.table != NULL, wrong, LAMBDA>, then the fixed-order sum of the loss partials into *loss
template <int LAMBDA>
static int pf_run_kind(const PfArgs& a, int kind, bool wrong, const int64_t* n_pair, float* loss, hipStream_t st) {
#define PF_KIND(K)                                                       \
    do {                                                                 \
        if (a.table) {                                                   \
            if (wrong) pf_launch<K, 1, 1, LAMBDA>(a, st);                \
            else pf_launch<K, 1, 0, LAMBDA>(a, st);                      \
        } else {                                                         \
            if (wrong) pf_launch<K, 0, 1, LAMBDA>(a, st);                \
            else pf_launch<K, 0, 0, LAMBDA>(a, st);                      \
        }                                                                \
    } while (0)
    switch (kind) {
        case RECNOW_PAIR_KIND_HINGE: PF_KIND(RECNOW_PAIR_KIND_HINGE); break;
        case RECNOW_PAIR_KIND_SQUARED_HINGE: PF_KIND(RECNOW_PAIR_KIND_SQUARED_HINGE); break;
        default: PF_KIND(RECNOW_PAIR_KIND_MARGIN_LOGISTIC); break;
    }
#undef PF_KIND
    RN_LAUNCH_CHECK();
    return rn_loss_finalize(a.part, rn_cdiv(a.B, RN_PW_T), n_pair, a.reduce_mean, loss, st);
}

// what recnow_pair_kind_fwdbwd and recnow_pair_lambda_fwdbwd check of kind / margin / factor / flags before anything else
static inline int pf_check_kind(int kind, float margin, float factor, int flags, const float* table, int n_values) {
    if (kind != RECNOW_PAIR_KIND_HINGE && kind != RECNOW_PAIR_KIND_SQUARED_HINGE && kind != RECNOW_PAIR_KIND_MARGIN_LOGISTIC) return RECNOW_EINVAL;
    if (!std::isfinite(margin) || !std::isfinite(factor)) return RECNOW_EINVAL;
    if (table) {
        if (n_values < 1 || n_values > PT_MAXV) return RECNOW_EINVAL;
        if (flags & ~(RECNOW_PAIR_WRONG_ORDER | RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
    } else {
        if (!(flags & RECNOW_PAIR_LABEL_GT)) return RECNOW_EINVAL;
        if (flags & ~(RECNOW_PAIR_LABEL_GT | RECNOW_PAIR_WRONG_ORDER | RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
    }
    return RECNOW_OK;
}
