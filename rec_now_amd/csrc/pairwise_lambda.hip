// In-batch pairwise loss with the LambdaRank pair weight |delta NDCG|, and the in-batch NDCG that falls out of the same pre-pass
// (rec_block/ndcg.py, NDCGLambdaWeight / ndcg_rank_terms / in_batch_ndcg; `lambda_weight=` of pairwise_loss).  A list is one segment.
//
//   position   r_i = #{ j in the list, taking part, j != i : s_j > s_i or (s_j == s_i and row_j < row_i) }   (q_i: the same count on the labels)
//   discount   D(r) = 1 / log2(2 + r), 0 for r >= topn;   gain G(y) = 2**y - 1 or y
//   list sums  DCG = sum G(y_i) D(r_i),  IDCG = sum G(y_i) D(q_i),  inv = 1 / IDCG where IDCG > 0 else 0
//   weight     lambda_ij = |G(y_i) - G(y_j)| |D(r_i) - D(r_j)| inv(list): one more factor of a pair's weight, a constant in the backward pass.
//              It never changes which pairs exist: n_pair, cnt_super and the wrong-order rule come from the count call as they are.
//
//  1. rank pre-pass (k_pl_rank_long, k_pl_rank): the two-route shape and the bounds of the walks of pairwise_kind.hip -- a thread per row from the
//     workgroup's LDS stage, a wave per row for segments over PW_LONG, global reads for ranges over PW_STAGE.  Per candidate two compares on the
//     scores, two on the labels and two integer adds; per ROW one fp64 log2 each for D(r) and D(q); D(r) rounded to float32 (B evaluations: the
//     difference D(r_i) - D(r_j) a walk forms is then good to half an ulp of D) goes into the {discount, gain} record beside the member, the
//     unrounded values into the row's fp64 terms G D(r), G D(q); the position.
//  2. per-segment sums (k_pl_segsum): a workgroup per segment (grid-stride over the segments), 256 threads striding the segment, fp64, fixed
//     order, no atomics; it writes inv per sorted row.  k_pl_metric (one workgroup): mean of DCG / IDCG over the lists with IDCG > 0 and their
//     number, in fixed order.  Nothing here synchronises with the host.
//  3. walks (k_pl_long, k_pl_walk over <KIND, TABLE, WRONG>): those of pairwise_kind.hip with the auxiliary records staged beside the members
//     (PW_WALK_AUX of pairwise_walk.hpp) -- 32 KB members + 16 KB records + 2 KB table, about 50 KB of LDS per workgroup.  Direction weights are
//     w |dG| |dD| and go through the same selects `w > 0 ? w * term : 0` (pk_term), so a direction that is no pair contributes an exact 0 whatever
//     its records hold; inv multiplies the row's two sums once.  BPR is the margin-logistic kind at margin 0.
// Bitwise reproducible: integer counts, per-row terms written by their row, fixed-order fp64 sums.
#include <cmath>
#include "common.hpp"
#include "pairwise_walk.hpp"
#include "pairwise_table.hpp"

namespace {
// workspace: the pairwise workspace (members, loss partials, long-row terms: what the count call packs) | the records of this file
struct LamWs {
    PairAux* aux;        // [B] sorted order
    float* inv;          // [B] sorted order, uniform within a segment
    int2* long_rq;       // [B] positions of the rows of long segments (k_pl_rank_long)
    double *td, *tq;     // [B] G D(r), G D(q) per sorted row
    double *dcg, *idcg;  // [B] per segment
};
size_t lam_off(int64_t B) { return rn_align(recnow_pairwise_workspace_bytes(B)); }
size_t lam_bytes(int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1);
    return rn_align(n * sizeof(PairAux)) + rn_align(n * sizeof(float)) + rn_align(n * sizeof(int2)) + 4 * rn_align(n * sizeof(double));
}
LamWs lam_ws(void* ws, size_t ws_bytes, int64_t B) {
    const size_t n = (size_t)(B > 0 ? B : 1);
    RnCarver c((char*)ws + lam_off(B), ws_bytes - lam_off(B));
    LamWs l;
    l.aux = c.take<PairAux>(n);
    l.inv = c.take<float>(n);
    l.long_rq = c.take<int2>(n);
    l.td = c.take<double>(n);
    l.tq = c.take<double>(n);
    l.dcg = c.take<double>(n);
    l.idcg = c.take<double>(n);
    return l;
}
}  // namespace

// ---- 1. rank pre-pass ----------------------------------------------------------------------------------------------------------------
// One candidate: does it stand before `me` by score (r) / by label (q)?  Ties go to the smaller original row index, so the positions of a list
// form a permutation.  Exact: float32 compares and integer adds.
__device__ __forceinline__ void pl_before(const Member& me, const Member& o, bool other, int& r, int& q) {
    const bool ok = other && ((o.valid & 1) != 0);
    const bool first = o.row < me.row;
    r += (ok && (o.score > me.score || (o.score == me.score && first))) ? 1 : 0;
    q += (ok && (o.label > me.label || (o.label == me.label && first))) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
k_pl_rank_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
               int2* __restrict__ long_rq) {
    __shared__ Member staged[PW_STAGE];
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    if (k0 >= B) return;
    const int64_t kl = min(B, k0 + 64) - 1;
    const int g0 = seg_id[k0], g1 = seg_id[kl];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int phase = 0; phase < 2; ++phase) {                       // only the first and the last row's segment can be long (block-uniform)
        if (phase == 1 && g1 == g0) break;
        const int g = phase == 0 ? g0 : g1;
        const int s = seg_first[g], e = seg_first[g + 1];
        if (e - s <= PW_LONG) continue;
        const bool in_lds = e - s <= PW_STAGE;
        __syncthreads();                                            // every wave is done with the previous segment's stage
        if (in_lds)
            for (int i = threadIdx.x; i < e - s; i += 256) staged[i] = mem[s + i];
        __syncthreads();
        const int64_t ka = k0 > s ? k0 : (int64_t)s, kb = kl < (int64_t)e - 1 ? kl : (int64_t)e - 1;
        for (int64_t k = ka + w; k <= kb; k += 4) {                 // waves take the segment's rows of this block in turn
            const Member me = mem[k];
            int r = 0, q = 0;
            PW_WALK_STRIDED(in_lds, staged, s, mem, s + lane, e, j, o, { pl_before(me, o, j != (int)k, r, q); });
            r = wave_sum(r);
            q = wave_sum(q);
            if (lane == 0) long_rq[k] = make_int2(r, q);
        }
    }
}

// D(r) in fp64: the list sums take it as it is, the record beside the member holds it rounded once
__device__ __forceinline__ double pl_discount(int r, int topn) {
    if (topn > 0 && r >= topn) return 0.0;
    return 1.0 / log2(2.0 + (double)r);
}

template <int GAIN>
__global__ void __launch_bounds__(256)
k_pl_rank(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, int topn,
          const int2* __restrict__ long_rq, PairAux* __restrict__ aux, double* __restrict__ td, double* __restrict__ tq,
          int32_t* __restrict__ rank, float* __restrict__ disc_out, float* __restrict__ gain_out) {
    __shared__ Member staged[PW_STAGE];
    int sbase;
    const bool in_lds = stage_members(mem, seg_id, seg_first, B, staged, &sbase);
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    const Member me = mem[k];
    const int g = seg_id[k];
    const int s = seg_first[g], e = seg_first[g + 1];
    const bool is_long = e - s > PW_LONG;           // walked by k_pl_rank_long
    int r = 0, q = 0;
    PW_WALK(in_lds, staged, sbase, mem, (is_long ? e : s), e, j, o, { pl_before(me, o, j != (int)k, r, q); });
    if (is_long) {
        const int2 rq = long_rq[k];
        r = rq.x;
        q = rq.y;
    }
    const bool takes = (me.valid & 1) != 0;
    double dr = 0.0, dq = 0.0, gn = 0.0;
    if (takes) {
        dr = pl_discount(r, topn);
        dq = pl_discount(q, topn);
        gn = GAIN == RECNOW_NDCG_GAIN_LINEAR ? (double)me.label : exp2((double)me.label) - 1.0;
    }
    PairAux a;
    a.discount = (float)dr;
    a.gain = (float)gn;
    aux[k] = a;
    td[k] = gn * dr;                                // DCG and IDCG are fp64 sums of fp64 terms: not of the float32 records
    tq[k] = gn * dq;
    if (rank) rank[me.row] = takes ? r : -1;
    if (disc_out) disc_out[me.row] = a.discount;
    if (gain_out) gain_out[me.row] = a.gain;
}

// ---- 2. per-segment sums and the metric ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pl_segsum(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
            const double* __restrict__ td, const double* __restrict__ tq, double* __restrict__ dcg, double* __restrict__ idcg,
            float* __restrict__ inv_sorted, float* __restrict__ inv_out) {
    __shared__ double red[16];
    const int nseg = seg_id[B - 1] + 1;
    for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
        const int s = seg_first[g], e = seg_first[g + 1];
        double a = 0.0, b = 0.0;
        for (int i = s + threadIdx.x; i < e; i += 256) {            // fixed order per thread, fixed tree
            a += td[i];
            b += tq[i];
        }
        a = block_sum<double>(a, red);
        b = block_sum<double>(b, red);
        if (threadIdx.x == 0) {
            dcg[g] = a;
            idcg[g] = b;
        }
        const float inv = b > 0.0 ? (float)(1.0 / b) : 0.f;
        for (int i = s + threadIdx.x; i < e; i += 256) {
            inv_sorted[i] = inv;
            if (inv_out) inv_out[mem[i].row] = inv;
        }
    }
}

__global__ void __launch_bounds__(1024)
k_pl_metric(const int32_t* __restrict__ seg_id, int64_t B, const double* __restrict__ dcg, const double* __restrict__ idcg,
            float* __restrict__ ndcg_mean, long long* __restrict__ n_lists) {
    __shared__ double red[16];
    __shared__ long long redc[16];
    const int nseg = seg_id[B - 1] + 1;
    double sum = 0.0;
    long long c = 0;
    for (int g = threadIdx.x; g < nseg; g += 1024) {
        const double d = idcg[g];
        if (d > 0.0) {
            sum += dcg[g] / d;
            c += 1;
        }
    }
    sum = block_sum<double>(sum, red);
    c = block_sum<long long>(c, redc);
    if (threadIdx.x == 0) {
        if (ndcg_mean) *ndcg_mean = c > 0 ? (float)(sum / (double)c) : 0.f;
        if (n_lists) *n_lists = c;
    }
}

// ---- 3. walks --------------------------------------------------------------------------------------------------------------------------
#define PL_TW (TABLE ? 2 * PT_MAXV * PT_MAXV : 1)

// Direction weights of one candidate times |dG| |dD| (inv is applied per row).  A direction that is no pair keeps w == 0 or turns NaN
// (0 * inf); neither passes the select `w > 0` of pk_term.
template <int TABLE, int WRONG>
__device__ __forceinline__ void pl_dirs(const Member& me, const PairAux& ma, const Member& o, const PairAux& oa, bool other, const float* trow,
                                        const float* tcol, float& wf, float& wb) {
    if (TABLE) pt_dirs<WRONG>(me, o, other, trow, tcol, wf, wb);
    else pk_dirs<WRONG>(me, o, other, wf, wb);
    const float lam = fabsf(ma.gain - oa.gain) * fabsf(ma.discount - oa.discount);
    wf *= lam;
    wb *= lam;
}

template <int KIND, int TABLE, int WRONG>
__global__ void __launch_bounds__(256)
k_pl_long(const Member* __restrict__ mem, const PairAux* __restrict__ aux, const int32_t* __restrict__ seg_id,
          const int32_t* __restrict__ seg_first, int64_t B, const float* __restrict__ W, int nv, float factor, float margin,
          float* __restrict__ long_la, float* __restrict__ long_ga) {
    __shared__ Member staged[PW_STAGE];
    __shared__ PairAux saux[PW_STAGE];
    __shared__ float tw[PL_TW];
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
            for (int i = threadIdx.x; i < e - s; i += 256) {
                staged[i] = mem[s + i];
                saux[i] = aux[s + i];
            }
        __syncthreads();
        const int64_t ka = k0 > s ? k0 : (int64_t)s, kb = kl < (int64_t)e - 1 ? kl : (int64_t)e - 1;
        for (int64_t k = ka + w; k <= kb; k += 4) {                 // waves take the segment's rows of this block in turn
            const Member me = mem[k];
            const PairAux ma = aux[k];
            const float* trow = tw + (TABLE ? (PT_CLS(me.valid) << 4) : 0);
            const float* tcol = trow + (TABLE ? PT_MAXV * PT_MAXV : 0);
            float la = 0.f, ga = 0.f;
            PW_WALK_AUX(in_lds, staged, saux, s, mem, aux, s + lane, e, 64, j, o, oa, {
                float wf;
                float wb;
                (pl_dirs<TABLE, WRONG>)(me, ma, o, oa, j != (int)k, trow, tcol, wf, wb);
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

// The occurrence weight cnt_super[super] ** power and inv are uniform within a segment, so they multiply the row's sums of both directions.
// TABLE and *bad != 0 (a taking-part row with a label outside the values): NaN everywhere.
template <int KIND, int TABLE, int WRONG>
__global__ void __launch_bounds__(256)
k_pl_walk(const Member* __restrict__ mem, const PairAux* __restrict__ aux, const float* __restrict__ inv, const int32_t* __restrict__ seg_id,
          const int32_t* __restrict__ seg_first, const int32_t* __restrict__ super_id, const unsigned long long* __restrict__ cnt_super,
          const unsigned long long* __restrict__ n_pair, int64_t B, const float* __restrict__ W, int nv, float factor, float margin, float power,
          int reduce_mean, const float* __restrict__ long_la, const float* __restrict__ long_ga, const unsigned* __restrict__ bad,
          double* __restrict__ block_loss, float* __restrict__ dscores) {
    __shared__ double red[16];
    __shared__ Member staged[PW_STAGE];
    __shared__ PairAux saux[PW_STAGE];
    __shared__ float tw[PL_TW];
    if (TABLE) pt_load_table(W, nv, tw);
    int sbase;
    const bool in_lds = stage_members(mem, seg_id, seg_first, B, staged, &sbase);
    if (in_lds) stage_beside(aux, seg_id, seg_first, B, saux);
    __syncthreads();                                // the records, and the table when stage_members did not synchronise
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool poisoned = TABLE && *bad != 0u;
    const float qnan = __int_as_float(0x7fc00000);
    double lsum = 0.0;
    if (k < B) {
        const Member me = mem[k];
        const PairAux ma = aux[k];
        const int g = seg_id[k];
        const int s = seg_first[g], e = seg_first[g + 1];
        float w = 1.f;
        if (power != 0.f) {
            const float cnt = (float)cnt_super[super_id[k]];
            // cnt == 0: no pair of this main group survived, the weight is never used (avoid 0**negative = inf -> inf*0)
            w = (cnt == 0.f) ? 1.f : ((power == 1.f) ? cnt : powf(cnt, power));
        }
        w *= inv[k];
        const bool is_long = e - s > PW_LONG;       // walked by k_pl_long
        const float* trow = tw + (TABLE ? (PT_CLS(me.valid) << 4) : 0);
        const float* tcol = trow + (TABLE ? PT_MAXV * PT_MAXV : 0);
        float la = 0.f, ga = 0.f;
        PW_WALK_AUX(in_lds, staged, saux, sbase, mem, aux, (is_long ? e : s), e, 1, j, o, oa, {
            float wf;
            float wb;
            (pl_dirs<TABLE, WRONG>)(me, ma, o, oa, j != (int)k, trow, tcol, wf, wb);
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

// members of the default rule when the caller's workspace does not hold them yet
__global__ void k_pl_pack(const float* __restrict__ scores, const float* __restrict__ labels, const uint8_t* __restrict__ mask,
                          const int32_t* __restrict__ order, int64_t B, Member* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < B) out[k] = load_member(scores, labels, mask, order, k);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
namespace {
struct PlArgs {
    const Member* mem;
    const PairAux* aux;
    const float* inv;
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
void pl_launch(const PlArgs& a, hipStream_t st) {
    const int G = rn_cdiv(a.B, RN_PW_T), GL = rn_cdiv(a.B, 64);
    hipLaunchKernelGGL((k_pl_long<KIND, TABLE, WRONG>), GL, 256, 0, st, a.mem, a.aux, a.seg_id, a.seg_first, a.B, a.table, a.nv, a.factor,
                       a.margin, a.long_la, a.long_ga);
    hipLaunchKernelGGL((k_pl_walk<KIND, TABLE, WRONG>), G, RN_PW_T, 0, st, a.mem, a.aux, a.inv, a.seg_id, a.seg_first, a.super_id, a.cnt_super,
                       a.n_pair, a.B, a.table, a.nv, a.factor, a.margin, a.power, a.reduce_mean, (const float*)a.long_la,
                       (const float*)a.long_ga, a.bad, a.part, a.dscores);
}

template <int KIND>
void pl_launch_kind(const PlArgs& a, bool table, bool wrong, hipStream_t st) {
    if (table) {
        if (wrong) pl_launch<KIND, 1, 1>(a, st);
        else pl_launch<KIND, 1, 0>(a, st);
    } else {
        if (wrong) pl_launch<KIND, 0, 1>(a, st);
        else pl_launch<KIND, 0, 0>(a, st);
    }
}
}  // namespace

extern "C" size_t recnow_pair_lambda_workspace_bytes(int64_t B) {
    if (B < 0) return 0;
    return lam_off(B) + lam_bytes(B);
}

extern "C" int recnow_pair_lambda_terms(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                        const int32_t* seg_id, const int32_t* seg_first, int64_t B, int flags, int gain, int topn,
                                        int32_t* rank, float* discount, float* gain_out, float* inv_idcg, double* list_dcg, double* list_idcg,
                                        float* ndcg_mean, int64_t* n_lists, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || (flags & ~RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;
    if (gain != RECNOW_NDCG_GAIN_EXP2 && gain != RECNOW_NDCG_GAIN_LINEAR) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (ndcg_mean) RN_HIP(hipMemsetAsync(ndcg_mean, 0, sizeof(float), st));
        if (n_lists) RN_HIP(hipMemsetAsync(n_lists, 0, sizeof(int64_t), st));
        return RECNOW_OK;
    }
    if (!seg_id || !seg_first || !ws) return RECNOW_EINVAL;
    if (ws_bytes < recnow_pair_lambda_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    const LamWs lw = lam_ws(ws, ws_bytes, B);
    const int G = rn_cdiv(B, RN_PW_T), GL = rn_cdiv(B, 64);
    // RECNOW_PAIR_MEMBERS_PACKED: `ws` holds the members of a count call on these inputs (recnow_pair_count or recnow_pair_table_count: bit 0 of
    // Member.valid says whether the row takes part either way)
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) {
        if (!scores || !labels || !order) return RECNOW_EINVAL;
        hipLaunchKernelGGL(k_pl_pack, G, RN_PW_T, 0, st, scores, labels, mask, order, B, pw.mem);
    }
    hipLaunchKernelGGL(k_pl_rank_long, GL, 256, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, lw.long_rq);
    if (gain == RECNOW_NDCG_GAIN_LINEAR)
        hipLaunchKernelGGL(k_pl_rank<RECNOW_NDCG_GAIN_LINEAR>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, topn,
                           (const int2*)lw.long_rq, lw.aux, lw.td, lw.tq, rank, discount, gain_out);
    else
        hipLaunchKernelGGL(k_pl_rank<RECNOW_NDCG_GAIN_EXP2>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, topn,
                           (const int2*)lw.long_rq, lw.aux, lw.td, lw.tq, rank, discount, gain_out);
    double* dcg = list_dcg ? list_dcg : lw.dcg;
    double* idcg = list_idcg ? list_idcg : lw.idcg;
    const int GS = B < 4096 ? (int)B : 4096;                        // a workgroup per segment, grid-stride: there are at most B segments
    hipLaunchKernelGGL(k_pl_segsum, GS, 256, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, (const double*)lw.td, (const double*)lw.tq, dcg,
                       idcg, lw.inv, inv_idcg);
    if (ndcg_mean || n_lists)
        hipLaunchKernelGGL(k_pl_metric, 1, 1024, 0, st, seg_id, B, (const double*)dcg, (const double*)idcg, ndcg_mean, (long long*)n_lists);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_pair_lambda_fwdbwd(const int32_t* seg_id, const int32_t* seg_first, const int32_t* super_id, const int64_t* cnt_super,
                                         const int64_t* n_pair, int64_t B, int flags, int kind, float margin, int n_values, const float* table,
                                         float factor, float power, int reduce_mean, float* loss, float* dscores, void* ws, size_t ws_bytes,
                                         void* stream) {
    if (B < 0 || !loss) return RECNOW_EINVAL;
    if (kind != RECNOW_PAIR_KIND_HINGE && kind != RECNOW_PAIR_KIND_SQUARED_HINGE && kind != RECNOW_PAIR_KIND_MARGIN_LOGISTIC) return RECNOW_EINVAL;
    if (!std::isfinite(margin) || !std::isfinite(factor)) return RECNOW_EINVAL;
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;      // the members and the records are those already in `ws`
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
    if (!seg_id || !seg_first || !super_id || !n_pair || !dscores || !ws) return RECNOW_EINVAL;
    if (power != 0.f && !cnt_super) return RECNOW_EINVAL;
    if (ws_bytes < recnow_pair_lambda_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    const LamWs lw = lam_ws(ws, ws_bytes, B);
    const PlArgs a = {pw.mem, lw.aux, lw.inv, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super,
                      (const unsigned long long*)n_pair, B, table, table ? n_values : 0, factor, margin, power, reduce_mean, pw.long_la,
                      pw.long_ga, pt_bad_flag(pw, B), pw.part, dscores};
    const bool wrong = (flags & RECNOW_PAIR_WRONG_ORDER) != 0;
    switch (kind) {
        case RECNOW_PAIR_KIND_HINGE: pl_launch_kind<RECNOW_PAIR_KIND_HINGE>(a, table != nullptr, wrong, st); break;
        case RECNOW_PAIR_KIND_SQUARED_HINGE: pl_launch_kind<RECNOW_PAIR_KIND_SQUARED_HINGE>(a, table != nullptr, wrong, st); break;
        default: pl_launch_kind<RECNOW_PAIR_KIND_MARGIN_LOGISTIC>(a, table != nullptr, wrong, st); break;
    }
    RN_LAUNCH_CHECK();
    return rn_pt_finalize(pw.part, rn_cdiv(B, RN_PW_T), n_pair, reduce_mean, loss, st);
}
