// In-batch sampled softmax (recnow_ibs_*, include/recnow.h): the retrieval loss of a two-tower model over in-batch negatives, with the logQ
// correction, the removal of accidental hits and a temperature.  Two-sided flash attention with one "value" per row, in exact fp32, and never
// a (B, B) tensor.  DESIGN.md section 8z.
//
// One kernel template, three uses.  A workgroup of two waves OWNS 64 rows of one side (a wave 32 of them, as B-operand fragments in
// registers for the whole launch) and STREAMS the other side through LDS in tiles of 32 rows.  The logit tile is formed TRANSPOSED on
// v_mfma_f32_32x32x2_f32 -- streamed rows are the MFMA rows, owner rows the MFMA columns -- so that lane (n, h) = (lane & 31, lane >> 5)
// holds, for owner row n, the 16 streamed rows  m_e = 8 (e / 4) + 4 h + e % 4:  a row reduction is 16 register steps and ONE exchange
// with lane ^ 32.
//   MODE 0, forward:  owner = queries, streamed = items.  Running (maximum, rescaled sum) per lane, merged across the half-waves at the end.
//   MODE 1, dq:       owner = queries, streamed = items.  p from the owner's saved statistic.
//   MODE 2, dv:       owner = items,   streamed = queries.  p from the streamed rows' saved statistic (staged in LDS with the tile).
// In the backward modes the 16 weights  w_e = p - [diagonal]  of a lane are fed STRAIGHT BACK as the B operand of the second product
// out^T (d, n) += Y^T (d, m) w (m, n):  step e of it contracts over the two streamed rows m_e(h = 0), m_e(h = 1), and the A operand is read
// from the LDS tile at exactly those rows (a permuted k index; no shuffle, no LDS round trip of the weights).
//
// Selects, never arithmetic, keep rows that do not take part out: they are staged as zeros (a NaN there would otherwise reach the second
// product as 0 * NaN), their weights are selected to 0 and their outputs are written as 0.
#include "common.hpp"
#include "wave_softmax.hpp"

#define IB_ROWS 64                              // owner rows of a workgroup (two waves of 32)
#define IB_TN 32                                // streamed rows of a tile
#define IB_DG 32                                // D is padded to a multiple of this on chip (one 32-row block of the second product)
#define IB_THREADS 128
typedef float ib_f16v __attribute__((ext_vector_type(16)));

struct IbArgs {
    const float* own; int64_t ldo;              // owner-side rows
    const float* str; int64_t lds;              // streamed-side rows
    const int64_t* ids; const float* log_q; const uint8_t* mask;
    int64_t B; int D; float inv_tau; int remove_hits;
    float* row_max; float* row_logsum; float* row_pos; float* row_loss; double* part;                    // MODE 0
    const float* st_max; const float* st_logsum; const float* n_rows; const float* gout; float* dout; int64_t ldd;   // MODE 1, 2
};

template <int NC, int MODE>
__global__ void __launch_bounds__(IB_THREADS) k_ibs(IbArgs a) {
    constexpr int DP = NC * 32, LD = DP + 4;    // + 4: the 16 lanes of a ds_read_b128 phase fall on 64 distinct banks, rows stay 16-byte aligned
    __shared__ __attribute__((aligned(16))) float sY[IB_TN * LD];
    __shared__ __attribute__((aligned(16))) float sLq[IB_TN];
    __shared__ __attribute__((aligned(16))) float sMax[IB_TN];
    __shared__ __attribute__((aligned(16))) float sLs[IB_TN];
    __shared__ __attribute__((aligned(16))) int sOn[IB_TN];
    __shared__ __attribute__((aligned(16))) int64_t sId[IB_TN];
    __shared__ float sRedL[IB_ROWS];
    __shared__ int sRedN[IB_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int64_t B = a.B;
    const int D = a.D;
    const int64_t og = (int64_t)blockIdx.x * IB_ROWS + wave * 32 + n;
    const bool o_in = og < B;
    const bool o_on = o_in && (a.mask == nullptr || a.mask[o_in ? og : 0] != 0);
    const bool use_ids = a.ids != nullptr && a.remove_hits != 0;
    const int64_t o_id = (use_ids && o_in) ? a.ids[og] : 0;
    const float inv_tau = a.inv_tau;

    // the owner rows as B-operand fragments: MFMA step 4 j + u contracts over the columns 8 j + u (h = 0) and 8 j + 4 + u (h = 1)
    rn_f4 x[NC * 4];
    {
        const bool ovec = rn_vec4_ok(a.own, D, a.ldo);
#pragma unroll
        for (int j = 0; j < NC * 4; ++j) {
            const int col = 8 * j + 4 * h;
            rn_f4 z = {0.f, 0.f, 0.f, 0.f};
            x[j] = (o_on && col < D) ? rn_ld4(a.own + og * a.ldo + col, D - col, ovec) : z;
        }
    }
    float o_lq = 0.f, o_max = 0.f, o_ls = 0.f;
    if (MODE == 2 && a.log_q != nullptr && o_in) o_lq = a.log_q[og];
    if (MODE == 1 && o_on) { o_max = a.st_max[og]; o_ls = a.st_logsum[og]; }

    const float NEG_INF = -__builtin_inff();
    float run_m = NEG_INF, run_s = 0.f, pos = 0.f;             // MODE 0
    ib_f16v acc[NC];                                           // MODE 1, 2: out^T, 32 columns d per block
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;

    const bool svec = rn_vec4_ok(a.str, D, a.lds);
    for (int64_t s0 = 0; s0 < B; s0 += IB_TN) {
        __syncthreads();                                       // the tile before this one has been read
        if (tid < IB_TN) {
            const int64_t sg = s0 + tid;
            const bool in = sg < B;
            const bool on = in && (a.mask == nullptr || a.mask[in ? sg : 0] != 0);
            sOn[tid] = on ? 1 : 0;
            sId[tid] = (use_ids && in) ? a.ids[sg] : 0;
            if (MODE != 2) sLq[tid] = (a.log_q != nullptr && in) ? a.log_q[sg] : 0.f;
            if (MODE == 2) { sMax[tid] = on ? a.st_max[sg] : 0.f; sLs[tid] = on ? a.st_logsum[sg] : 0.f; }
        }
        for (int idx = tid; idx < IB_TN * (DP / 4); idx += IB_THREADS) {
            const int r = idx / (DP / 4), c = (idx % (DP / 4)) * 4;
            const int64_t sg = s0 + r;
            const bool in = sg < B;
            const bool on = in && (a.mask == nullptr || a.mask[in ? sg : 0] != 0);
            rn_f4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<rn_f4*>(&sY[r * LD + c]) = (on && c < D) ? rn_ld4(a.str + sg * a.lds + c, D - c, svec) : z;
        }
        __syncthreads();

        // the logit tile, transposed: t[e] = <streamed row m_e, owner row n>
        ib_f16v t;
#pragma unroll
        for (int e = 0; e < 16; ++e) t[e] = 0.f;
        {
            const float* yr = &sY[n * LD + 4 * h];
#pragma unroll
            for (int j = 0; j < NC * 4; ++j) {
                const rn_f4 y = *reinterpret_cast<const rn_f4*>(yr + 8 * j);
                t = __builtin_amdgcn_mfma_f32_32x32x2f32(y.x, x[j].x, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x2f32(y.y, x[j].y, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x2f32(y.z, x[j].z, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x2f32(y.w, x[j].w, t, 0, 0, 0);
            }
        }

        // logits, candidates: s_ij = <q_i, v_j> / tau - log_q[j]; the candidate test is symmetric in (owner, streamed)
        float sv[16];
        bool valid[16], diag[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = 8 * (e >> 2) + 4 * h + (e & 3);
            const int64_t sg = s0 + m;
            diag[e] = sg == og;
            const bool same = use_ids && sId[m] == o_id;
            valid[e] = o_on && sOn[m] != 0 && (diag[e] || !same);
            sv[e] = t[e] * inv_tau - (MODE == 2 ? o_lq : sLq[m]);
        }

        if (MODE == 0) {
            float tm = NEG_INF;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                tm = fmaxf(tm, valid[e] ? sv[e] : NEG_INF);
                if (diag[e]) pos = sv[e];
            }
            const float new_m = fmaxf(run_m, tm);
            const float scale = run_m == NEG_INF ? 0.f : ai_exp(run_m - new_m);      // the running sum follows the maximum
            float add = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) add += valid[e] ? ai_exp(sv[e] - new_m) : 0.f;
            run_s = run_s * scale + add;
            run_m = new_m;
        } else {
            float w[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = 8 * (e >> 2) + 4 * h + (e & 3);
                const float mx = MODE == 1 ? o_max : sMax[m], ls = MODE == 1 ? o_ls : sLs[m];
                const float p = ai_exp((sv[e] - mx) - ls);
                w[e] = valid[e] ? p - (diag[e] ? 1.f : 0.f) : 0.f;
            }
            // out^T (d, n) += sum_m Y (m, d) w (m, n): step e contracts over m_e(0) and m_e(1), the rows this lane's pair of half-waves holds
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float* yc = &sY[4 * h * LD + 32 * c + n];
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(yc[(8 * (e >> 2) + (e & 3)) * LD], w[e], acc[c], 0, 0, 0);
            }
        }
    }

    if (MODE == 0) {
        // the two half-waves of a row: one exchange.  A sum of a half that saw no candidate is 0 and its factor 0; NaN survives (NaN * 0).
        const float m2 = __shfl_xor(run_m, 32, 64), s2 = __shfl_xor(run_s, 32, 64), p2 = __shfl_xor(pos, 32, 64);
        const float mm = fmaxf(run_m, m2);
        const float f1 = run_m == NEG_INF ? 0.f : ai_exp(run_m - mm), f2 = m2 == NEG_INF ? 0.f : ai_exp(m2 - mm);
        const float tot = h == 0 ? run_s * f1 + s2 * f2 : s2 * f2 + run_s * f1;   // the same expression in both halves
        const float ls = logf(tot);                                              // a lone candidate: tot = 1, ls = 0, lse = s_ii bit for bit
        const int64_t diag_tile_h = ((og & 31) >> 2) & 1;                         // the half-wave that held the diagonal element
        const float ps = diag_tile_h == h ? pos : p2;
        const float li = (mm - ps) + ls;
        const float QNAN = __builtin_nanf("");
        if (h == 0) {
            if (o_in) {
                a.row_max[og] = o_on ? mm : QNAN;
                a.row_logsum[og] = o_on ? ls : QNAN;
                a.row_pos[og] = o_on ? ps : QNAN;
                a.row_loss[og] = o_on ? li : 0.f;
            }
            sRedL[wave * 32 + n] = o_on ? li : 0.f;
            sRedN[wave * 32 + n] = o_on ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0) {                                                          // the workgroup's partial: fp64, row order
            double sum = 0.0;
            int cnt = 0;
            for (int r = 0; r < IB_ROWS; ++r) { sum += (double)sRedL[r]; cnt += sRedN[r]; }
            a.part[2 * (int64_t)blockIdx.x] = sum;
            a.part[2 * (int64_t)blockIdx.x + 1] = (double)cnt;
        }
    } else {
        const float nr = a.n_rows[0];
        const float scale = nr > 0.f ? a.gout[0] * inv_tau / nr : 0.f;
        const bool dvec = rn_vec4_ok(a.dout, D, a.ldd);
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 32 * c + 8 * g + 4 * h;
                rn_f4 val = {acc[c][4 * g] * scale, acc[c][4 * g + 1] * scale, acc[c][4 * g + 2] * scale, acc[c][4 * g + 3] * scale};
                rn_f4 z = {0.f, 0.f, 0.f, 0.f};
                if (o_in && col < D) rn_st4(a.dout + og * a.ldd + col, o_on ? val : z, D - col, dvec);
            }
    }
}

// loss = (sum of the workgroup partials) / (sum of their counts), fp64, fixed order: thread c adds the partials c, c + 256, .., one thread the 256 sums.
__global__ void __launch_bounds__(256) k_ibs_mean(const double* __restrict__ part, int nblk, float* __restrict__ loss, float* __restrict__ n_rows) {
    __shared__ double rs[256], rn[256];
    double s = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) { s += part[2 * (int64_t)b]; c += part[2 * (int64_t)b + 1]; }
    rs[threadIdx.x] = s;
    rn[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tc = 0.0;
        for (int i = 0; i < 256; ++i) { ts += rs[i]; tc += rn[i]; }
        loss[0] = tc > 0.0 ? (float)(ts / tc) : 0.f;
        n_rows[0] = (float)tc;
    }
}

static int64_t g_ibs_launches[8][2];

template <int MODE>
static int ibs_launch(const IbArgs& a, hipStream_t st) {
    const int nc = (a.D + IB_DG - 1) / IB_DG;
    const int grid = rn_cdiv(a.B, IB_ROWS);
    switch (nc) {
        case 1: hipLaunchKernelGGL((k_ibs<1, MODE>), grid, IB_THREADS, 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_ibs<2, MODE>), grid, IB_THREADS, 0, st, a); break;
        case 3: hipLaunchKernelGGL((k_ibs<3, MODE>), grid, IB_THREADS, 0, st, a); break;
        default: hipLaunchKernelGGL((k_ibs<4, MODE>), grid, IB_THREADS, 0, st, a); break;
    }
    RN_LAUNCH_CHECK();
    const auto vec = [&](const void* p, int64_t ld) { return ((a.D & 3) == 0 && (ld & 3) == 0 && ((uintptr_t)p & 15) == 0) ? 1 : 0; };
    ++g_ibs_launches[MODE][vec(a.own, a.ldo)];
    ++g_ibs_launches[MODE + 4][vec(a.str, a.lds)];
    return RECNOW_OK;
}

extern "C" int recnow_ibs_supported(int64_t B, int D) { return (B >= 0 && D >= 1 && D <= 128) ? 1 : 0; }

extern "C" size_t recnow_ibs_workspace_bytes(int64_t B, int D, int bwd) {
    (void)D;
    if (bwd || B <= 0) return 0;
    return (size_t)16 * (size_t)((B + IB_ROWS - 1) / IB_ROWS);
}

extern "C" int recnow_ibs_tile(int which) {
    switch (which) {
        case 0: return IB_ROWS;
        case 1: return IB_TN;
        case 2: return IB_DG;
        default: return RECNOW_EINVAL;
    }
}

extern "C" int64_t recnow_ibs_launches(int orientation, int vec) {
    if (orientation < 0 || orientation > 6 || orientation == 3 || vec < 0 || vec > 1) return RECNOW_EINVAL;
    return g_ibs_launches[orientation][vec];
}

static int ibs_check(const float* q, int64_t ldq, const float* v, int64_t ldv, int64_t B, int D) {
    if (B < 0 || D < 1) return RECNOW_EINVAL;
    if (!recnow_ibs_supported(B, D)) return RECNOW_EUNSUPPORTED;
    if (B > 0 && (!q || !v || ldq < D || ldv < D)) return RECNOW_EINVAL;
    if (B > ((int64_t)1 << 30)) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}

extern "C" int recnow_ibs_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                              const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, float* row_max, float* row_logsum,
                              float* row_pos, float* row_loss, float* loss, float* n_rows, void* ws, size_t ws_bytes, void* stream) {
    const int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    if (!row_max || !row_logsum || !row_pos || !row_loss || !loss || !n_rows || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    if (!ws || ws_bytes < recnow_ibs_workspace_bytes(B, D, 0) || ((uintptr_t)ws & 7) != 0) return RECNOW_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    IbArgs a = {};
    a.own = q; a.ldo = ldq; a.str = v; a.lds = ldv; a.ids = ids; a.log_q = log_q; a.mask = mask;
    a.B = B; a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits;
    a.row_max = row_max; a.row_logsum = row_logsum; a.row_pos = row_pos; a.row_loss = row_loss; a.part = (double*)ws;
    const int lrc = ibs_launch<0>(a, st);
    if (lrc != RECNOW_OK) return lrc;
    hipLaunchKernelGGL(k_ibs_mean, 1, 256, 0, st, (const double*)ws, rn_cdiv(B, IB_ROWS), loss, n_rows);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_ibs_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                              const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, const float* row_max,
                              const float* row_logsum, const float* n_rows, const float* gout, float* dq, int64_t lddq, float* dv,
                              int64_t lddv, void* ws, size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    const int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    if (!row_max || !row_logsum || !n_rows || !gout || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    if ((dq && lddq < D) || (dv && lddv < D)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    IbArgs a = {};
    a.ids = ids; a.log_q = log_q; a.mask = mask; a.B = B; a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits;
    a.st_max = row_max; a.st_logsum = row_logsum; a.n_rows = n_rows; a.gout = gout;
    if (dq) {
        a.own = q; a.ldo = ldq; a.str = v; a.lds = ldv; a.dout = dq; a.ldd = lddq;
        const int lrc = ibs_launch<1>(a, st);
        if (lrc != RECNOW_OK) return lrc;
    }
    if (dv) {
        a.own = v; a.ldo = ldv; a.str = q; a.lds = ldq; a.dout = dv; a.ldd = lddv;
        const int lrc = ibs_launch<2>(a, st);
        if (lrc != RECNOW_OK) return lrc;
    }
    return RECNOW_OK;
}
