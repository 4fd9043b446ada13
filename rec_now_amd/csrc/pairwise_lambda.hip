// In-batch pairwise loss with the LambdaRank pair weight |delta NDCG|, and the in-batch NDCG that falls out of the same pre-pass
// (rec_block/ndcg.py, NDCGLambdaWeight / ndcg_rank_terms / in_batch_ndcg; `lambda_weight=` of pairwise_loss).  A list is one segment.
//
//   position   r_i = #{ j in the list, taking part, j != i : s_j > s_i or (s_j == s_i and row_j < row_i) }   (q_i: the same count on the labels)
//   discount   D(r) = 1 / log2(2 + r), 0 for r >= topn;   gain G(y) = 2**y - 1 or y
//   list sums  DCG = sum G(y_i) D(r_i),  IDCG = sum G(y_i) D(q_i),  inv = 1 / IDCG where IDCG > 0 else 0
//   weight     lambda_ij = |G(y_i) - G(y_j)| |D(r_i) - D(r_j)| inv(list): one more factor of a pair's weight, a constant in the backward pass.
//              It never changes which pairs exist: n_pair, cnt_super and the wrong-order rule come from the count call as they are.
//
//  1. rank pre-pass (k_pl_rank_long, k_pl_rank: PlRank on the two route skeletons of pairwise_walk.hpp): a thread per row from the workgroup's LDS
//     stage, a wave per row for segments over PW_LONG, global reads for ranges over PW_STAGE.  Per candidate two compares on the scores, two on
//     the labels and two integer adds; per ROW one fp64 log2 each for D(r) and D(q); D(r) rounded to float32 (B evaluations: the difference
//     D(r_i) - D(r_j) a walk forms is then good to half an ulp of D) goes into the {discount, gain} record beside the member, the unrounded
//     values into the row's fp64 terms G D(r), G D(q); the position.
//  2. per-segment sums (k_pl_segsum): a workgroup per segment (grid-stride over the segments), 256 threads striding the segment, fp64, fixed
//     order, no atomics; it writes inv per sorted row.  k_pl_metric (one workgroup): mean of DCG / IDCG over the lists with IDCG > 0 and their
//     number, in fixed order.  Nothing here synchronises with the host.
//  3. walks: k_pf_long / k_pf_walk<KIND, TABLE, WRONG, 1> of pairwise_table.hpp, the kernel pair of pairwise_kind.hip with the auxiliary records staged
//     beside the members -- 32 KB members + 16 KB records + 2 KB table, about 50 KB of LDS per workgroup.  Direction weights are w |dG| |dD| and go
//     through the same selects `w > 0 ? w * term : 0` (pk_term), so a direction that is no pair contributes an exact 0 whatever its records hold; inv
//     multiplies the row's two sums once.  BPR is the margin-logistic kind at margin 0.
// This file holds the workspace of the records, the pre-pass kernels and the two entry points.
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

// D(r) in fp64: the list sums take it as it is, the record beside the member holds it rounded once
__device__ __forceinline__ double pl_discount(int r, int topn) {
    if (topn > 0 && r >= topn) return 0.0;
    return 1.0 / log2(2.0 + (double)r);
}

template <int GAIN>
struct PlRank : PwPlain {
    typedef int2 Row;      // {r, q}
    typedef int Out;       // (nothing to sum over the workgroup)
    int2* long_rq;             // k_pl_rank_long parks the positions here
    const int2* parked;        // k_pl_rank reads them
    int topn;
    PairAux* aux;
    double *td, *tq;
    int32_t* rank;
    float *disc_out, *gain_out;
    __device__ __forceinline__ Row begin(const Member&, int64_t, bool) const { return make_int2(0, 0); }
    __device__ __forceinline__ void candidate(Row& rq, const Member& me, const Member& o, bool other, bool, int, int) const {
        pl_before(me, o, other, rq.x, rq.y);
    }
    __device__ __forceinline__ void park(Row& rq, int64_t k, int lane) const {
        const int r = wave_sum(rq.x), q = wave_sum(rq.y);
        if (lane == 0) long_rq[k] = make_int2(r, q);
    }
    __device__ __forceinline__ Out finish(Row& rq, const Member& me, int64_t k, bool is_long) const {
        if (is_long) rq = parked[k];
        const bool takes = (me.valid & 1) != 0;
        double dr = 0.0, dq = 0.0, gn = 0.0;
        if (takes) {
            dr = pl_discount(rq.x, topn);
            dq = pl_discount(rq.y, topn);
            gn = GAIN == RECNOW_NDCG_GAIN_LINEAR ? (double)me.label : exp2((double)me.label) - 1.0;
        }
        PairAux a;
        a.discount = (float)dr;
        a.gain = (float)gn;
        aux[k] = a;
        td[k] = gn * dr;                                // DCG and IDCG are fp64 sums of fp64 terms: not of the float32 records
        tq[k] = gn * dq;
        if (rank) rank[me.row] = takes ? rq.x : -1;
        if (disc_out) disc_out[me.row] = a.discount;
        if (gain_out) gain_out[me.row] = a.gain;
        return 0;
    }
};

__global__ void __launch_bounds__(256)
k_pl_rank_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B,
               int2* __restrict__ long_rq) {
    __shared__ Member staged[PW_STAGE];
    const PlRank<0> p = {{}, long_rq};
    pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
}

template <int GAIN>
__global__ void __launch_bounds__(256)
k_pl_rank(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, int topn,
          const int2* __restrict__ long_rq, PairAux* __restrict__ aux, double* __restrict__ td, double* __restrict__ tq,
          int32_t* __restrict__ rank, float* __restrict__ disc_out, float* __restrict__ gain_out) {
    __shared__ Member staged[PW_STAGE];
    const PlRank<GAIN> p = {{}, nullptr, long_rq, topn, aux, td, tq, rank, disc_out, gain_out};
    pw_thread_rows(mem, seg_id, seg_first, B, staged, p);
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
        const int rc = rn_pack_members(scores, labels, mask, order, B, pw.mem, st);
        if (rc) return rc;
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
    if (int rc = pf_check_kind(kind, margin, factor, flags, table, n_values)) return rc;
    if (!(flags & RECNOW_PAIR_MEMBERS_PACKED)) return RECNOW_EINVAL;      // the members and the records are those already in `ws`
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
    const PfArgs a = {pw.mem, lw.aux, lw.inv, seg_id, seg_first, super_id, (const unsigned long long*)cnt_super,
                      (const unsigned long long*)n_pair, B, table, table ? n_values : 0, factor, margin, power, reduce_mean, pw.long_la,
                      pw.long_ga, pt_bad_flag(pw, B), pw.part, dscores};
    return pf_run_kind<1>(a, kind, (flags & RECNOW_PAIR_WRONG_ORDER) != 0, n_pair, loss, st);
}
