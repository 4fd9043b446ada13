// In-batch ApproxNDCG (rec_block/approx_ndcg.py; recnow_approx_ndcg_fwdbwd; Qin, Liu and Li 2010): a differentiable NDCG loss, forward and
// backward, on the two route skeletons of pairwise_walk.hpp.  No pair list, no host synchronisation, no float atomics.
//
// Definitions.
//   Lists and rows.  A list is one segment of build_segments(groups): the lists of in_batch_ndcg.  A row takes part when mask is true there, or
//     when there is no mask.  Rows that do not take part influence nothing and get gradient exactly 0.
//   Temperature.  tau is a finite float greater than 0.
//   Soft position of a taking-part row.  R_i = sum_{j in the list, taking part, j != i} sigma((s_j - s_i) / tau).  0-based, so it matches
//     D(r) = 1 / log2(2 + r).  For distinct scores R_i tends to the hard position r_i as tau -> 0.
//   Gain.  G(y) = 2**y - 1 or y.
//   Ideal DCG.  IDCG = sum G(y_i) D(q_i), q_i the label position of pairwise_lambda.hip (ties go to the smaller original row index).  No topn.
//   Valid list.  IDCG > 0.  A NaN label of a taking-part row makes that comparison false, so the list is invalid.
//   Loss of a valid list.  l = -ADCG / IDCG, ADCG = sum_i G(y_i) / log2(2 + R_i).  The batch loss is the mean of l over the valid lists, 0
//     when there is none.
//   Gradient.  c_i = G(y_i) ln 2 / ((2 + R_i) ln^2(2 + R_i));  sigma'_kj = sigma(x) (1 - sigma(x)), x = (s_j - s_k) / tau, symmetric in k, j;
//     dl/ds_k = (1 / (tau IDCG)) sum_{j != k, taking part} sigma'_kj (c_j - c_k).  The gradient of a list sums to zero.  Rows of an invalid
//     list get exactly 0, by a select.
//   NaN scores.  A NaN score of a taking-part row makes its own list's loss NaN (its R is NaN by definition, also in a list of one), and the
//     batch mean with it; that list's taking-part rows get NaN gradients; every other list's gradient bits stay as they were.  A row that does
//     not take part may hold any score and any label: every candidate goes through a select on `other && valid`, as pk_term's do.
//
//  1. rn_pack_members (pairwise.hip): the 16-byte member records by sorted position.
//  2. walk 1 (k_px_rank_long, k_px_rank<GAIN>: PxRank on pw_wave_rows / pw_thread_rows).  Per candidate the label compare of pl_before for q and
//     one float32 sigmoid from the hardware exp2 / rcp in the exp(-|x|) form of pk_f -- x of (k, j) is the exact negative of x of (j, k), so both
//     rows of a pair see the same exp and rcp bits --, added to an fp64 accumulator of R.  Per ROW, in fp64: G, G D(q), G / log2(2 + R) and c;
//     c rounded to float32 goes by sorted position beside the members, R by original row into approx_rank.
//  3. k_px_segsum: a workgroup per segment (grid-stride), fp64, fixed order: IDCG, ADCG, the list's loss, validity and 1 / IDCG by segment.
//     k_px_mean (one workgroup): the fixed-order fp64 sum of the valid lists' losses, their int64 number, the float32 mean; the NaN / -1 poison
//     where the grouping reported a grid-barrier time-out (n_seg[0] < 0).
//  4. walk 2 (k_px_grad_long, k_px_grad: PxGrad on the same skeletons), the c records staged beside the members through P::stage.  Per candidate
//     one sigma' = ex / (1 + ex)^2 (bit-symmetric in the pair) and sigma' (c_j - c_k), a float32 product that is the exact negative of the other
//     row's, added to an fp64 accumulator: a list's gradient sums to zero up to the float32 rounding of each stored entry.  finish multiplies by
//     1 / IDCG / tau / n_lists and writes dscores[me.row].
// Bounds.  Walks stay inside their segment (pairwise_walk.hpp); per-segment arrays are indexed by seg_id[k] < B; every array is sized by B.
// Bitwise reproducible: fixed butterflies, fixed-order sums, every value written by its row or its segment.
#include <cmath>
#include "common.hpp"
#include "pairwise_walk.hpp"

namespace {
// workspace: the pairwise workspace (members: what rn_pack_members fills) | the records of this file
struct PxWs {
    float* c;                              // [B] sorted order: c_i, 0 for a row that does not take part
    double *tq, *ta;                       // [B] sorted order: G D(q), G / log2(2 + R)
    double *park_r, *park_g;               // [B] sorted order: what the long-row kernels park (R; the gradient sum)
    int32_t* park_q;                       // [B]
    double *adcg, *idcg, *lloss, *linv;    // [B] per segment
    int32_t* lvalid;                       // [B] per segment
    long long* nl;                         // [1] number of valid lists, -1 after a grouping time-out
};
size_t px_off(int64_t B) { return rn_align(recnow_pairwise_workspace_bytes(B)); }
PxWs px_ws(void* ws, int64_t B, size_t* bytes) {
    const size_t n = (size_t)(B > 0 ? B : 1);
    RnCarver c((char*)ws + px_off(B), 0);
    PxWs w;
    w.c = c.take<float>(n);
    w.tq = c.take<double>(n);
    w.ta = c.take<double>(n);
    w.park_r = c.take<double>(n);
    w.park_g = c.take<double>(n);
    w.park_q = c.take<int32_t>(n);
    w.adcg = c.take<double>(n);
    w.idcg = c.take<double>(n);
    w.lloss = c.take<double>(n);
    w.linv = c.take<double>(n);
    w.lvalid = c.take<int32_t>(n);
    w.nl = c.take<long long>(1);
    if (bytes) *bytes = px_off(B) + c.off;
    return w;
}
}  // namespace

// sigma(x) and sigma'(x) = sigma(x) (1 - sigma(x)) from one exp(-|x|): ex in (0, 1], 1 + ex never denormal.  sigma' depends on |x| alone.
__device__ __forceinline__ void px_sigmoid(float x, float& sg, float& dsg) {
    const float ex = __builtin_amdgcn_exp2f(-1.44269504f * fabsf(x));
    const float inv = __builtin_amdgcn_rcpf(1.f + ex);
    const float lo = ex * inv;
    sg = x >= 0.f ? inv : lo;
    dsg = lo * inv;
}

// ---- 2. walk 1: soft positions, label positions, the per-row terms ---------------------------------------------------------------------------
template <int GAIN>
struct PxRank : PwPlain {
    struct Row {
        double r;
        int q;
    };
    typedef int Out;           // (nothing to sum over the workgroup)
    float inv_tau;
    double* park_r;            // k_px_rank_long parks here
    int32_t* park_q;
    const double* parked_r;    // k_px_rank reads them
    const int32_t* parked_q;
    float* c;
    double *tq, *ta, *approx_rank;
    __device__ __forceinline__ Row begin(const Member&, int64_t, bool) const { return {0.0, 0}; }
    __device__ __forceinline__ void candidate(Row& a, const Member& me, const Member& o, bool other, bool, int, int) const {
        const bool ok = other && ((o.valid & 1) != 0);
        a.q += (ok && (o.label > me.label || (o.label == me.label && o.row < me.row))) ? 1 : 0;
        float sg, dsg;
        px_sigmoid((o.score - me.score) * inv_tau, sg, dsg);
        a.r += (double)(ok ? sg : 0.f);
    }
    __device__ __forceinline__ void park(Row& a, int64_t k, int lane) const {
        const double r = wave_sum(a.r);
        const int q = wave_sum(a.q);
        if (lane == 0) {
            park_r[k] = r;
            park_q[k] = q;
        }
    }
    __device__ __forceinline__ Out finish(Row& a, const Member& me, int64_t k, bool is_long) const {
        if (is_long) {
            a.r = parked_r[k];
            a.q = parked_q[k];
        }
        const bool takes = (me.valid & 1) != 0;
        const double R = me.score != me.score ? (double)NAN : a.r;
        double gq = 0.0, ga = 0.0, cc = 0.0;
        if (takes) {
            const double gn = GAIN == RECNOW_NDCG_GAIN_LINEAR ? (double)me.label : exp2((double)me.label) - 1.0;
            const double t = 2.0 + R, L = log(t);
            gq = gn / log2(2.0 + (double)a.q);
            ga = gn * 0.69314718055994530942 / L;
            cc = ga / (t * L);
        }
        c[k] = (float)cc;
        tq[k] = gq;
        ta[k] = ga;
        if (approx_rank) approx_rank[me.row] = takes ? R : (double)NAN;
        return 0;
    }
};

__global__ void __launch_bounds__(256)
k_px_rank_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, float inv_tau,
               double* __restrict__ park_r, int32_t* __restrict__ park_q) {
    __shared__ Member staged[PW_STAGE];
    const PxRank<0> p = {{}, inv_tau, park_r, park_q};
    pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
}

template <int GAIN>
__global__ void __launch_bounds__(256)
k_px_rank(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, float inv_tau,
          const double* __restrict__ park_r, const int32_t* __restrict__ park_q, float* __restrict__ c, double* __restrict__ tq,
          double* __restrict__ ta, double* __restrict__ approx_rank) {
    __shared__ Member staged[PW_STAGE];
    const PxRank<GAIN> p = {{}, inv_tau, nullptr, nullptr, park_r, park_q, c, tq, ta, approx_rank};
    pw_thread_rows(mem, seg_id, seg_first, B, staged, p);
}

// ---- 3. per-segment sums, the mean --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_px_segsum(const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, const double* __restrict__ ta,
            const double* __restrict__ tq, double* __restrict__ adcg, double* __restrict__ idcg, double* __restrict__ lloss,
            double* __restrict__ linv, int32_t* __restrict__ lvalid) {
    __shared__ double red[16];
    const int nseg = seg_id[B - 1] + 1;
    for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
        const int s = seg_first[g], e = seg_first[g + 1];
        double a = 0.0, b = 0.0;
        for (int i = s + threadIdx.x; i < e; i += 256) {            // fixed order per thread, fixed tree
            a += ta[i];
            b += tq[i];
        }
        a = block_sum<double>(a, red);
        b = block_sum<double>(b, red);
        if (threadIdx.x == 0) {
            const bool valid = b > 0.0;                             // false for a NaN IDCG
            adcg[g] = a;
            idcg[g] = b;
            lvalid[g] = valid ? 1 : 0;
            lloss[g] = valid ? -a / b : 0.0;
            linv[g] = valid ? (a == a ? 1.0 / b : (double)NAN) : 0.0;      // a NaN ADCG (a NaN score): every taking-part row's gradient NaN
        }
    }
}

__global__ void __launch_bounds__(1024)
k_px_mean(const int32_t* __restrict__ seg_id, const int32_t* __restrict__ n_seg, int64_t B, const double* __restrict__ lloss,
          const int32_t* __restrict__ lvalid, float* __restrict__ loss, double* __restrict__ loss_sum, long long* __restrict__ n_lists,
          long long* __restrict__ nl_ws) {
    __shared__ double red[16];
    __shared__ long long redc[16];
    const int nseg = seg_id[B - 1] + 1;
    const bool bad = n_seg[0] < 0;
    double sum = 0.0;
    long long c = 0;
    for (int g = threadIdx.x; g < nseg; g += 1024)
        if (lvalid[g]) {
            sum += lloss[g];
            c += 1;
        }
    sum = block_sum<double>(sum, red);
    c = block_sum<long long>(c, redc);
    if (threadIdx.x == 0) {
        if (loss) *loss = bad ? NAN : (c > 0 ? (float)(sum / (double)c) : 0.f);
        if (loss_sum) *loss_sum = bad ? (double)NAN : sum;
        if (n_lists) *n_lists = bad ? -1 : c;
        *nl_ws = bad ? -1 : c;
    }
}

// ---- 4. walk 2: the gradient -------------------------------------------------------------------------------------------------------------------
struct PxGrad {
    struct Row {
        double acc, scale;
        float ck;
        bool live, bad;
    };
    typedef int Out;
    float inv_tau;
    const float* c;
    float* sc;                 // the c records of the staged members
    double* park_g;            // k_px_grad_long parks here
    const double* parked_g;    // k_px_grad reads them
    const int32_t *seg_id, *lvalid;
    const double* linv;
    const long long* nl;
    float* dscores;
    __device__ __forceinline__ void once() const {}
    __device__ __forceinline__ void stage(int i, int k) const { sc[i] = c[k]; }
    __device__ __forceinline__ Row begin(const Member& me, int64_t k, bool wave) const {
        Row r = {};
        r.ck = c[k];
        if (!wave) {           // in front of the walk, so that the dependent loads wait under it
            const int g = seg_id[k];
            const long long n = *nl;
            r.bad = n < 0;
            r.live = lvalid[g] != 0 && (me.valid & 1) != 0;
            r.scale = linv[g] * (double)inv_tau / (double)n;
        }
        return r;
    }
    __device__ __forceinline__ void candidate(Row& r, const Member& me, const Member& o, bool other, bool in_lds, int i, int j) const {
        const bool ok = other && ((o.valid & 1) != 0);
        const float oc = in_lds ? sc[i] : c[j];
        float sg, dsg;
        px_sigmoid((o.score - me.score) * inv_tau, sg, dsg);
        const float t = dsg * (oc - r.ck);
        r.acc += (double)(ok ? t : 0.f);
    }
    __device__ __forceinline__ void park(Row& r, int64_t k, int lane) const {
        const double a = wave_sum(r.acc);
        if (lane == 0) park_g[k] = a;
    }
    __device__ __forceinline__ Out finish(Row& r, const Member& me, int64_t k, bool is_long) const {
        if (is_long) r.acc = parked_g[k];
        const float qnan = __int_as_float(0x7fc00000);
        dscores[me.row] = r.bad ? qnan : (r.live ? (float)(r.acc * r.scale) : 0.f);
        return 0;
    }
};

__global__ void __launch_bounds__(256)
k_px_grad_long(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, float inv_tau,
               const float* __restrict__ c, double* __restrict__ park_g) {
    __shared__ Member staged[PW_STAGE];
    __shared__ float sc[PW_STAGE];
    const PxGrad p = {inv_tau, c, sc, park_g};
    pw_wave_rows(mem, seg_id, seg_first, B, staged, p);
}

__global__ void __launch_bounds__(256)
k_px_grad(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, float inv_tau,
          const float* __restrict__ c, const double* __restrict__ park_g, const int32_t* __restrict__ lvalid, const double* __restrict__ linv,
          const long long* __restrict__ nl, float* __restrict__ dscores) {
    __shared__ Member staged[PW_STAGE];
    __shared__ float sc[PW_STAGE];
    const PxGrad p = {inv_tau, c, sc, nullptr, park_g, seg_id, lvalid, linv, nl, dscores};
    pw_thread_rows(mem, seg_id, seg_first, B, staged, p);
}

extern "C" size_t recnow_approx_ndcg_workspace_bytes(int64_t B) {
    if (B < 0) return 0;
    size_t bytes = 0;
    px_ws(nullptr, B, &bytes);
    return bytes;
}

extern "C" int recnow_approx_ndcg_fwdbwd(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order,
                                         const int32_t* seg_id, const int32_t* seg_first, const int32_t* n_seg, int64_t B, int gain,
                                         float temperature, float* loss, double* loss_sum, int64_t* n_lists, float* dscores,
                                         double* approx_rank, double* list_adcg, double* list_idcg, void* ws, size_t ws_bytes, void* stream) {
    if (B < 0) return RECNOW_EINVAL;
    if (gain != RECNOW_NDCG_GAIN_EXP2 && gain != RECNOW_NDCG_GAIN_LINEAR) return RECNOW_EINVAL;
    if (!std::isfinite(temperature) || !(temperature > 0.f)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        if (loss) RN_HIP(hipMemsetAsync(loss, 0, sizeof(float), st));
        if (loss_sum) RN_HIP(hipMemsetAsync(loss_sum, 0, sizeof(double), st));
        if (n_lists) RN_HIP(hipMemsetAsync(n_lists, 0, sizeof(int64_t), st));
        return RECNOW_OK;
    }
    if (!scores || !labels || !order || !seg_id || !seg_first || !n_seg || !ws) return RECNOW_EINVAL;
    if (ws_bytes < recnow_approx_ndcg_workspace_bytes(B)) return RECNOW_EWORKSPACE;
    const PairWs pw = pair_ws(ws, ws_bytes, B);
    const PxWs w = px_ws(ws, B, nullptr);
    const float inv_tau = (float)(1.0 / (double)temperature);
    const int G = rn_cdiv(B, RN_PW_T), GL = rn_cdiv(B, 64);
    if (int rc = rn_pack_members(scores, labels, mask, order, B, pw.mem, st)) return rc;
    hipLaunchKernelGGL(k_px_rank_long, GL, 256, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, inv_tau, w.park_r, w.park_q);
    if (gain == RECNOW_NDCG_GAIN_LINEAR)
        hipLaunchKernelGGL(k_px_rank<RECNOW_NDCG_GAIN_LINEAR>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, inv_tau,
                           (const double*)w.park_r, (const int32_t*)w.park_q, w.c, w.tq, w.ta, approx_rank);
    else
        hipLaunchKernelGGL(k_px_rank<RECNOW_NDCG_GAIN_EXP2>, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, inv_tau,
                           (const double*)w.park_r, (const int32_t*)w.park_q, w.c, w.tq, w.ta, approx_rank);
    double* adcg = list_adcg ? list_adcg : w.adcg;
    double* idcg = list_idcg ? list_idcg : w.idcg;
    const int GS = B < 4096 ? (int)B : 4096;                        // a workgroup per segment, grid-stride: there are at most B segments
    hipLaunchKernelGGL(k_px_segsum, GS, 256, 0, st, seg_id, seg_first, B, (const double*)w.ta, (const double*)w.tq, adcg, idcg, w.lloss, w.linv,
                       w.lvalid);
    hipLaunchKernelGGL(k_px_mean, 1, 1024, 0, st, seg_id, n_seg, B, (const double*)w.lloss, (const int32_t*)w.lvalid, loss, loss_sum,
                       (long long*)n_lists, w.nl);
    if (dscores) {
        hipLaunchKernelGGL(k_px_grad_long, GL, 256, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, inv_tau, (const float*)w.c, w.park_g);
        hipLaunchKernelGGL(k_px_grad, G, RN_PW_T, 0, st, (const Member*)pw.mem, seg_id, seg_first, B, inv_tau, (const float*)w.c,
                           (const double*)w.park_g, (const int32_t*)w.lvalid, (const double*)w.linv, (const long long*)w.nl, dscores);
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
