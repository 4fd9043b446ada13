// In-batch sampled softmax (recnow_ibs_*, include/recnow.h): the retrieval loss of a two-tower model over in-batch negatives, with the logQ
// correction, the removal of accidental hits and a temperature.  Two-sided flash attention with one "value" per row, in exact fp32, and never
// a (B, B) tensor.  DESIGN.md section 8z.
//
// One kernel template, five uses.  A workgroup of two waves OWNS 64 rows of one side (a wave 32 of them, as B-operand fragments in
// registers for the whole launch) and STREAMS the other side through LDS in tiles of 32 rows.  The logit tile is formed TRANSPOSED on
// v_mfma_f32_32x32x2_f32 -- streamed rows are the MFMA rows, owner rows the MFMA columns -- so that lane (n, h) = (lane & 31, lane >> 5)
// holds, for owner row n, the 16 streamed rows  m_e = 8 (e / 4) + 4 h + e % 4:  a row reduction is 16 register steps and ONE exchange
// with lane ^ 32.
//   MODE 0, forward:  owner = queries, streamed = items.  Running (maximum, rescaled sum) per lane, merged across the half-waves at the end.
//   MODE 1, dq:       owner = queries, streamed = items.  p from the owner's saved statistic.
//   MODE 2, dv:       owner = items,   streamed = queries.  p from the streamed rows' saved statistic (staged in LDS with the tile).
//   MODE 3, ranks:    owner = queries, streamed = items, then extras.  Three integer counts per lane -- the candidates other than the positive,
//                     those above it, those equal to it -- merged across the half-waves at the end (recnow_ibs_rank).
//                     The positive's logit has to be known before anything is compared with it: two tiles AHEAD of the walk, the two of
//                     the diagonal segment that hold the workgroup's own positives, go through the same loop body and only pick it up.
//   MODE 4, top-K:    owner = queries, streamed = items, then extras.  The walk and the candidates of MODE 3; each owner row keeps the K
//                     candidates that stand first in the total order (NaN, then the greater score, then the smaller index) as a binary
//                     heap in dynamic LDS with the worst kept entry at its root (recnow_ibs_topk).  The positive
//                     is excluded by index, so nothing is read ahead of the walk.
// Extra negatives (recnow_ibs_extra_*): N item-side rows with no query row of their own.  The streamed side is a
// list of segments; the forward and dq stream the items (a segment with a diagonal), then the extras (one without), each segment from a
// fresh tile.  dv is the square launch unchanged.  de is MODE 2 with the extras as owners and the queries streamed without a diagonal.
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

// One side of the product: rows with their per-row id, logQ correction, on-flag and (backward) saved statistic.  The owner side is one of
// these; the streamed side is a short list of them, walked segment by segment, each from a fresh tile to its own ragged tile.  has_diag: the
// segment's row k is the positive of owner row k (the batch against itself); a segment without one (the extra negatives, or the queries
// streamed past extras that own) holds candidates only.
struct IbSide {
    const float* rows; int64_t ld; int64_t count;
    const int64_t* ids; const float* log_q; const uint8_t* mask;
    const float* st_max; const float* st_logsum;
    int has_diag;
};

struct IbArgs {
    IbSide own;                                 // owner-side rows
    IbSide seg[2]; int nseg;                    // streamed-side rows
    int D; float inv_tau; int remove_hits;
    float* row_max; float* row_logsum; float* row_pos; float* row_loss; double* part;                    // MODE 0
    const float* n_rows; const float* gout; float* dout; int64_t ldd;                                    // MODE 1, 2
    int64_t* n_greater; int64_t* n_equal; int64_t* n_cand; int walk_diag;                                // MODE 3 (row_pos too)
    int K; float* top_s; int64_t ld_top_s; int64_t* top_i; int64_t ld_top_i;                             // MODE 4 (n_cand, walk_diag too)
};

#define IB_TOPK_MAX_K 128                       // 64 rows x 128 slots x 8 bytes = 64 KiB of dynamic LDS beside the tile
#define IB_TOPK_LDS(K_) ((size_t)IB_ROWS * (8 * (size_t)(K_) + 4))                 // scores, indices, one length a row
#define IB_STATIC_LDS(NC_) ((size_t)IB_TN * ((NC_) * 32 + 4) * 4 + 1536)            // the tile and (an upper bound of) the per-row vectors beside it

// The total order of the top-K list as one unsigned compare: a stands before b iff ib_key(a) > ib_key(b).  The high word orders the scores
// (-0.0 and 0.0 tie, a NaN of either sign is greatest), the low word breaks ties towards the smaller index.  Indices are distinct, so
// keys are: the K first candidates are a function of the candidate set alone.
__device__ __forceinline__ unsigned long long ib_key(float s, unsigned idx) {
    unsigned u = __float_as_uint(s);
    const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
    u = (u & 0x7fffffffu) == 0u ? 0u : u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    u = nan ? 0xffffffffu : u;
    return ((unsigned long long)u << 32) | (unsigned long long)(~idx);
}

// XT 0: the square loss -- one streamed segment, the batch, with its diagonal (both known at compile time).  XT 1: the segment list is read
// from the arguments: items then extras (MODE 0, 1), or the queries past owning extras (MODE 2, "de").
template <int NC, int MODE, int XT>
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
    extern __shared__ __attribute__((aligned(16))) unsigned char ib_dyn[];      // MODE 4: the lists (no other mode is launched with any)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int D = a.D;
    const int64_t og = (int64_t)blockIdx.x * IB_ROWS + wave * 32 + n;
    const bool o_in = og < a.own.count;
    const bool o_on = o_in && (a.own.mask == nullptr || a.own.mask[o_in ? og : 0] != 0);
    const bool use_ids = a.own.ids != nullptr && a.remove_hits != 0;
    const int64_t o_id = (use_ids && o_in) ? a.own.ids[og] : 0;
    const float inv_tau = a.inv_tau;

    // the owner rows as B-operand fragments: MFMA step 4 j + u contracts over the columns 8 j + u (h = 0) and 8 j + 4 + u (h = 1)
    rn_f4 x[NC * 4];
    {
        const bool ovec = rn_vec4_ok(a.own.rows, D, a.own.ld);
#pragma unroll
        for (int j = 0; j < NC * 4; ++j) {
            const int col = 8 * j + 4 * h;
            rn_f4 z = {0.f, 0.f, 0.f, 0.f};
            x[j] = (o_on && col < D) ? rn_ld4(a.own.rows + og * a.own.ld + col, D - col, ovec) : z;
        }
    }
    float o_lq = 0.f, o_max = 0.f, o_ls = 0.f;
    if (MODE == 2 && a.own.log_q != nullptr && o_in) o_lq = a.own.log_q[og];
    if (MODE == 1 && o_on) { o_max = a.own.st_max[og]; o_ls = a.own.st_logsum[og]; }

    const float NEG_INF = -__builtin_inff();
    float run_m = NEG_INF, run_s = 0.f, pos = 0.f;             // MODE 0; pos: MODE 3 too
    int n_gt = 0, n_eq = 0, n_cd = 0;                          // MODE 3 (n_cd: MODE 4 too): a lane sees half of at most 2^31 streamed rows
    // MODE 4: owner row r keeps slot s of its list at [s * IB_ROWS + r] -- a lane walks its own row's column, whatever the slot, on its own
    // bank.  A min-heap under ib_key: slot 0 is the worst kept entry, the threshold.  Both half-waves of a row hold its length and its
    // threshold's score; they are read again from LDS after every pass that may have changed them
    const int K = MODE == 4 ? a.K : 0;
    float* const lS = reinterpret_cast<float*>(ib_dyn) + (wave * 32 + n);
    unsigned* const lP = reinterpret_cast<unsigned*>(ib_dyn) + (size_t)K * IB_ROWS + (wave * 32 + n);
    int* const lC = reinterpret_cast<int*>(ib_dyn) + (size_t)2 * K * IB_ROWS + (wave * 32 + n);
    int t_cnt = 0;
    float t_s = 0.f;
    if (MODE == 4 && h == 0) lC[0] = 0;
    ib_f16v acc[NC];                                           // MODE 1, 2: out^T, 32 columns d per block
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;

    // One loop over the tiles of all segments (a nest of two would keep a second copy of the accumulators): the batch segment's tiles first,
    // in the order of the square loss, then -- from a fresh tile -- the second segment's.  de streams the queries alone.
    // The walk is over streamed rows: the first segment's span is rounded up to whole tiles where a second one follows it.
    const int64_t span0 = XT ? (a.seg[0].count + IB_TN - 1) / IB_TN * IB_TN : a.seg[0].count;
    const int64_t span = span0 + ((XT && MODE != 2 && a.nseg > 1) ? a.seg[1].count : 0);
    // MODE 3: the walk is preceded by two tiles (sw < 0), the workgroup's own 64 rows of the diagonal segment, and may leave that segment
    // out (a corpus of extras alone: the batch item is a row's positive and nobody's candidate)
    const int64_t first = MODE == 3 ? -2 * IB_TN : 0, skip = ((MODE == 3 || MODE == 4) && a.walk_diag == 0) ? span0 : 0;
    for (int64_t sw = first; sw < span - skip; sw += IB_TN) {
        const bool ahead = MODE == 3 && sw < 0;
        const int64_t at = ahead ? (int64_t)blockIdx.x * IB_ROWS + (sw - first) : sw + skip;     // the tile's place among the streamed rows
        const int si = (XT && !ahead && at >= span0) ? 1 : 0;
        const IbSide& g = a.seg[si];
        const int64_t s0 = si ? at - span0 : at;
        const int64_t og_d = (XT && g.has_diag == 0) ? -1 : og;  // the streamed row that is this owner's positive; none in a segment without a diagonal
        const bool svec = rn_vec4_ok(g.rows, D, g.ld);           // the access width is a segment's own
        __syncthreads();                                       // the tile before this one has been read
        if (tid < IB_TN) {
            const int64_t sg = s0 + tid;
            const bool in = sg < g.count;
            const bool on = in && (g.mask == nullptr || g.mask[in ? sg : 0] != 0);
            sOn[tid] = on ? 1 : 0;
            sId[tid] = (use_ids && in) ? g.ids[sg] : 0;
            if (MODE != 2) sLq[tid] = (g.log_q != nullptr && in) ? g.log_q[sg] : 0.f;
            if (MODE == 2) { sMax[tid] = on ? g.st_max[sg] : 0.f; sLs[tid] = on ? g.st_logsum[sg] : 0.f; }
        }
        for (int idx = tid; idx < IB_TN * (DP / 4); idx += IB_THREADS) {
            const int r = idx / (DP / 4), c = (idx % (DP / 4)) * 4;
            const int64_t sg = s0 + r;
            const bool in = sg < g.count;
            const bool on = in && (g.mask == nullptr || g.mask[in ? sg : 0] != 0);
            rn_f4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<rn_f4*>(&sY[r * LD + c]) = (on && c < D) ? rn_ld4(g.rows + sg * g.ld + c, D - c, svec) : z;
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

        // logits, candidates: s_ij = <q_i, v_j> / tau - log_q[j]; the candidate test is symmetric in (owner, streamed).  A segment without
        // a diagonal has diag[e] false throughout: no positive is picked up there and no "- 1" can be selected into a weight
        float sv[16];
        bool valid[16], diag[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = 8 * (e >> 2) + 4 * h + (e & 3);
            const int64_t sg = s0 + m;
            diag[e] = sg == og_d;
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
        } else if (MODE == 3) {
            if (ahead) {
                // the positive of a row turns up in one of the two tiles (tile  2 blockIdx.x + wave) and in one half-wave, as in the forward;
                // it is left in LDS, where both half-waves of the row find it after the barrier that opens the next tile
                float pk = 0.f;
                bool got = false;
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (diag[e]) { pk = sv[e]; got = true; }
                if (got) sRedL[wave * 32 + n] = pk;
            } else {
                pos = sRedL[wave * 32 + n];
                // a count is a comparison of two results of the one expression above: a copy of the positive is equal wherever it stands.
                // "not <=" and not ">": a NaN on either side counts as greater
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const bool cand = valid[e] && !diag[e];
                    n_cd += cand ? 1 : 0;
                    n_gt += (cand && !(sv[e] <= pos)) ? 1 : 0;
                    n_eq += (cand && sv[e] == pos) ? 1 : 0;
                }
            }
        } else if (MODE == 4) {
            // the common tile: 16 compares against the threshold's score.  "not <": an equal score goes on to the index, a NaN to the key
            const unsigned base = (unsigned)((si ? a.seg[0].count : 0) + s0) + 4u * h;       // of cat(items, extras); below 2^31
            unsigned hit = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bool cand = valid[e] && !diag[e];
                n_cd += cand ? 1 : 0;
                hit |= (cand && (t_cnt < K || !(sv[e] < t_s))) ? (1u << e) : 0u;
            }
            if (__builtin_amdgcn_ballot_w64(hit != 0) != 0) {
                // the two half-waves of a row share its list: h = 0 inserts, then h = 1, each from the state the other left in LDS
                for (int hh = 0; hh < 2; ++hh) {
                    if (h == hh) {
                        while (hit) {
                            const int e = __builtin_ctz(hit);
                            hit &= hit - 1;
                            float cs = sv[0];
#pragma unroll
                            for (int u = 1; u < 16; ++u) cs = e == u ? sv[u] : cs;
                            const unsigned cp = base + 8u * (e >> 2) + (e & 3);
                            const unsigned long long ck = ib_key(cs, cp);
                            if (t_cnt < K) {
                                // not yet full: every candidate is taken, a -inf one included; sift it up from the end
                                int s = t_cnt++;
                                while (s > 0) {
                                    const int par = (s - 1) >> 1;
                                    const float pf = lS[par * IB_ROWS];
                                    const unsigned pp = lP[par * IB_ROWS];
                                    if (ib_key(pf, pp) <= ck) break;
                                    lS[s * IB_ROWS] = pf; lP[s * IB_ROWS] = pp;
                                    s = par;
                                }
                                lS[s * IB_ROWS] = cs; lP[s * IB_ROWS] = cp;
                            } else if (ck > ib_key(lS[0], lP[0])) {
                                // it stands before the worst kept entry: that one leaves, the candidate sifts down from the root
                                int s = 0;
                                for (;;) {
                                    int c = 2 * s + 1;
                                    if (c >= K) break;
                                    float cf = lS[c * IB_ROWS];
                                    unsigned cq = lP[c * IB_ROWS];
                                    unsigned long long kk = ib_key(cf, cq);
                                    if (c + 1 < K) {
                                        const float rf = lS[(c + 1) * IB_ROWS];
                                        const unsigned rq = lP[(c + 1) * IB_ROWS];
                                        const unsigned long long rk = ib_key(rf, rq);
                                        if (rk < kk) { cf = rf; cq = rq; kk = rk; ++c; }
                                    }
                                    if (kk >= ck) break;
                                    lS[s * IB_ROWS] = cf; lP[s * IB_ROWS] = cq;
                                    s = c;
                                }
                                lS[s * IB_ROWS] = cs; lP[s * IB_ROWS] = cp;
                            }
                        }
                        lC[0] = t_cnt;
                    }
                    __builtin_amdgcn_wave_barrier();
                    t_cnt = lC[0];
                    t_s = lS[0];                                 // slot 0 of an empty list is never compared: t_cnt < K comes first
                }
            }
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
    } else if (MODE == 3) {
        // the two half-waves of a row: one exchange; each row is written once, by its h = 0 lane.  Rows that do not take part counted nothing
        n_gt += __shfl_xor(n_gt, 32, 64);
        n_eq += __shfl_xor(n_eq, 32, 64);
        n_cd += __shfl_xor(n_cd, 32, 64);
        __syncthreads();                                                         // a launch that walks nothing comes here from the tiles ahead
        pos = sRedL[wave * 32 + n];
        if (h == 0 && o_in) {
            a.n_greater[og] = n_gt;
            a.n_equal[og] = n_eq;
            a.n_cand[og] = n_cd;
            a.row_pos[og] = o_on ? pos : __builtin_nanf("");
        }
    } else if (MODE == 4) {
        n_cd += __shfl_xor(n_cd, 32, 64);
        __builtin_amdgcn_wave_barrier();
        // order by counting: an entry's place is the number of entries that stand before it; keys are distinct, so places are.  The two
        // half-waves of a row take every other slot; each output element is written once, the fill included
        if (o_in) {
            float* const os = a.top_s + og * a.ld_top_s;
            int64_t* const oi = a.top_i + og * a.ld_top_i;
            for (int j = h; j < t_cnt; j += 2) {
                const float fj = lS[j * IB_ROWS];
                const unsigned pj = lP[j * IB_ROWS];
                const unsigned long long kj = ib_key(fj, pj);
                int place = 0;
                for (int i = 0; i < t_cnt; ++i) place += ib_key(lS[i * IB_ROWS], lP[i * IB_ROWS]) > kj ? 1 : 0;
                os[place] = fj;
                oi[place] = (int64_t)pj;
            }
            for (int j = t_cnt + h; j < K; j += 2) { os[j] = NEG_INF; oi[j] = -1; }
            if (h == 0) a.n_cand[og] = n_cd;
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
static int64_t g_ibsx_launches[4][2];
static int64_t g_ibsr_launches[4][2];
static int64_t g_ibst_launches[4][2];

static IbSide ibs_side(const float* rows, int64_t ld, int64_t count, const int64_t* ids, const float* log_q, const uint8_t* mask,
                       const float* st_max, const float* st_logsum, int has_diag) {
    IbSide s = {rows, ld, count, ids, log_q, mask, st_max, st_logsum, has_diag};
    return s;
}

template <int MODE, int XT>
static int ibs_launch(const IbArgs& a, hipStream_t st) {
    const int nc = (a.D + IB_DG - 1) / IB_DG;
    const int grid = rn_cdiv(a.own.count, IB_ROWS);
    // MODE 4: the lists (K scores and K indices a row) and their lengths, in dynamic LDS.  With the tile that passes 64 KiB from K = 92
    // (D > 96) to K = 116 (D <= 32) on; the limit is raised once per kernel and device, to what K = IB_TOPK_MAX_K needs
    const size_t dyn = MODE == 4 ? IB_TOPK_LDS(a.K) : 0;
    const bool grant = dyn + IB_STATIC_LDS(nc) > 64 * 1024;
    switch (nc) {
#define IB_CASE(NC_)                                                                                                              \
        if (grant) RN_HIP(rn_lds_grant((const void*)k_ibs<NC_, MODE, XT>, IB_TOPK_LDS(IB_TOPK_MAX_K) + IB_STATIC_LDS(NC_)));      \
        hipLaunchKernelGGL((k_ibs<NC_, MODE, XT>), grid, IB_THREADS, dyn, st, a);                                                 \
        break;
        case 1: IB_CASE(1)
        case 2: IB_CASE(2)
        case 3: IB_CASE(3)
        default: IB_CASE(4)
#undef IB_CASE
    }
    RN_LAUNCH_CHECK();
    const auto vec = [&](const IbSide& s) { return ((a.D & 3) == 0 && (s.ld & 3) == 0 && ((uintptr_t)s.rows & 15) == 0) ? 1 : 0; };
    if (MODE == 3 || MODE == 4) {                        // a census of its own each: the loss's counts are read as deltas
        int64_t (*c)[2] = MODE == 3 ? g_ibsr_launches : g_ibst_launches;
        ++c[0][vec(a.own)];
        ++c[1][vec(a.seg[0])];
        if (a.nseg > 1) ++c[2][vec(a.seg[1])];
        ++c[3][a.walk_diag ? 1 : 0];
    } else if (!XT) {
        ++g_ibs_launches[MODE][vec(a.own)];
        ++g_ibs_launches[MODE + 4][vec(a.seg[0])];
    } else if (MODE != 2) {
        ++g_ibsx_launches[MODE][vec(a.seg[1])];          // forward / dq with an extra segment: the extras' width
    } else {
        ++g_ibsx_launches[2][vec(a.own)];                // de: the extras own,
        ++g_ibsx_launches[3][vec(a.seg[0])];             // the queries are streamed
    }
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

extern "C" int64_t recnow_ibs_extra_launches(int which, int vec) {
    if (which < 0 || which > 3 || vec < 0 || vec > 1) return RECNOW_EINVAL;
    return g_ibsx_launches[which][vec];
}

extern "C" int64_t recnow_ibs_rank_launches(int which, int vec) {
    if (which < 0 || which > 3 || vec < 0 || vec > 1) return RECNOW_EINVAL;
    return g_ibsr_launches[which][vec];
}

extern "C" int64_t recnow_ibs_topk_launches(int which, int vec) {
    if (which < 0 || which > 3 || vec < 0 || vec > 1) return RECNOW_EINVAL;
    return g_ibst_launches[which][vec];
}

extern "C" int recnow_ibs_topk_max_k(void) { return IB_TOPK_MAX_K; }

static int ibs_check(const float* q, int64_t ldq, const float* v, int64_t ldv, int64_t B, int D) {
    if (B < 0 || D < 1) return RECNOW_EINVAL;
    if (!recnow_ibs_supported(B, D)) return RECNOW_EUNSUPPORTED;
    if (B > 0 && (!q || !v || ldq < D || ldv < D)) return RECNOW_EINVAL;
    if (B > ((int64_t)1 << 30)) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}

// The extras of the _extra entries.  Ids come in pairs: the hit test compares one side's with the other's.
static int ibs_check_extra(const float* extra, int64_t ld_extra, const int64_t* ids, const int64_t* extra_ids, int64_t N, int D) {
    if (N < 0) return RECNOW_EINVAL;
    if (N > 0 && (!extra || ld_extra < D || (ids == nullptr) != (extra_ids == nullptr))) return RECNOW_EINVAL;
    if (N > ((int64_t)1 << 30)) return RECNOW_EUNSUPPORTED;
    return RECNOW_OK;
}

// The forward of both entries; ex: the extras as a second streamed segment, or NULL (the square loss, today's kernels).
static int ibs_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q, const uint8_t* mask,
                   const IbSide* ex, int64_t B, int D, float inv_tau, int remove_hits, float* row_max, float* row_logsum, float* row_pos,
                   float* row_loss, float* loss, float* n_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!row_max || !row_logsum || !row_pos || !row_loss || !loss || !n_rows || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    if (!ws || ws_bytes < recnow_ibs_workspace_bytes(B, D, 0) || ((uintptr_t)ws & 7) != 0) return RECNOW_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    IbArgs a = {};
    a.own = ibs_side(q, ldq, B, ids, log_q, mask, nullptr, nullptr, 0);
    a.seg[0] = ibs_side(v, ldv, B, ids, log_q, mask, nullptr, nullptr, 1);
    a.nseg = 1;
    a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits;
    a.row_max = row_max; a.row_logsum = row_logsum; a.row_pos = row_pos; a.row_loss = row_loss; a.part = (double*)ws;
    if (ex) { a.seg[1] = *ex; a.nseg = 2; }
    const int lrc = ex ? ibs_launch<0, 1>(a, st) : ibs_launch<0, 0>(a, st);
    if (lrc != RECNOW_OK) return lrc;
    hipLaunchKernelGGL(k_ibs_mean, 1, 256, 0, st, (const double*)ws, rn_cdiv(B, IB_ROWS), loss, n_rows);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// The backward of both entries.  dq streams the items, then the extras (ex, or NULL); dv is the square launch whatever ex is: its owners are
// the items and p reaches it through the queries' saved statistic; de (ex and de given) has the extras own and streams the queries.
static int ibs_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q, const uint8_t* mask,
                   const IbSide* ex, int64_t B, int D, float inv_tau, int remove_hits, const float* row_max, const float* row_logsum,
                   const float* n_rows, const float* gout, float* dq, int64_t lddq, float* dv, int64_t lddv, float* de, int64_t ldde,
                   void* stream) {
    if (!row_max || !row_logsum || !n_rows || !gout || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    if ((dq && lddq < D) || (dv && lddv < D) || (de && ldde < D)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    IbArgs a = {};
    a.nseg = 1;
    a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits; a.n_rows = n_rows; a.gout = gout;
    if (dq) {
        a.own = ibs_side(q, ldq, B, ids, log_q, mask, row_max, row_logsum, 0);
        a.seg[0] = ibs_side(v, ldv, B, ids, log_q, mask, nullptr, nullptr, 1);
        if (ex) { a.seg[1] = *ex; a.nseg = 2; }
        a.dout = dq; a.ldd = lddq;
        const int lrc = ex ? ibs_launch<1, 1>(a, st) : ibs_launch<1, 0>(a, st);
        if (lrc != RECNOW_OK) return lrc;
        a.seg[1] = IbSide{};                     // dv and de stream one segment: nothing of dq's second one stays behind
        a.nseg = 1;
    }
    if (dv) {
        a.own = ibs_side(v, ldv, B, ids, log_q, mask, nullptr, nullptr, 0);
        a.seg[0] = ibs_side(q, ldq, B, ids, nullptr, mask, row_max, row_logsum, 1);
        a.dout = dv; a.ldd = lddv;
        const int lrc = ibs_launch<2, 0>(a, st);
        if (lrc != RECNOW_OK) return lrc;
    }
    if (ex && de) {
        a.own = *ex;
        a.seg[0] = ibs_side(q, ldq, B, ids, nullptr, mask, row_max, row_logsum, 0);
        a.dout = de; a.ldd = ldde;
        const int lrc = ibs_launch<2, 1>(a, st);
        if (lrc != RECNOW_OK) return lrc;
    }
    return RECNOW_OK;
}

extern "C" int recnow_ibs_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                              const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, float* row_max, float* row_logsum,
                              float* row_pos, float* row_loss, float* loss, float* n_rows, void* ws, size_t ws_bytes, void* stream) {
    const int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    return ibs_fwd(q, ldq, v, ldv, ids, log_q, mask, nullptr, B, D, inv_tau, remove_hits, row_max, row_logsum, row_pos, row_loss, loss, n_rows,
                   ws, ws_bytes, stream);
}

extern "C" int recnow_ibs_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                              const uint8_t* mask, int64_t B, int D, float inv_tau, int remove_hits, const float* row_max,
                              const float* row_logsum, const float* n_rows, const float* gout, float* dq, int64_t lddq, float* dv,
                              int64_t lddv, void* ws, size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    const int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    return ibs_bwd(q, ldq, v, ldv, ids, log_q, mask, nullptr, B, D, inv_tau, remove_hits, row_max, row_logsum, n_rows, gout, dq, lddq, dv, lddv,
                   nullptr, 0, stream);
}

extern "C" int recnow_ibs_extra_fwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                                    const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                                    const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                                    float* row_max, float* row_logsum, float* row_pos, float* row_loss, float* loss, float* n_rows, void* ws,
                                    size_t ws_bytes, void* stream) {
    int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc == RECNOW_OK) rc = ibs_check_extra(extra, ld_extra, ids, extra_ids, N, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    const IbSide ex = ibs_side(extra, ld_extra, N, extra_ids, extra_log_q, extra_mask, nullptr, nullptr, 0);
    return ibs_fwd(q, ldq, v, ldv, ids, log_q, mask, N > 0 ? &ex : nullptr, B, D, inv_tau, remove_hits, row_max, row_logsum, row_pos, row_loss,
                   loss, n_rows, ws, ws_bytes, stream);
}

extern "C" int recnow_ibs_extra_bwd(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                                    const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                                    const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                                    const float* row_max, const float* row_logsum, const float* n_rows, const float* gout, float* dq,
                                    int64_t lddq, float* dv, int64_t lddv, float* de, int64_t ldde, void* ws, size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc == RECNOW_OK) rc = ibs_check_extra(extra, ld_extra, ids, extra_ids, N, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    const IbSide ex = ibs_side(extra, ld_extra, N, extra_ids, extra_log_q, extra_mask, nullptr, nullptr, 0);
    return ibs_bwd(q, ldq, v, ldv, ids, log_q, mask, N > 0 ? &ex : nullptr, B, D, inv_tau, remove_hits, row_max, row_logsum, n_rows, gout, dq,
                   lddq, dv, lddv, de, ldde, stream);
}


// Ranks of the positives: MODE 3 over the items (walked as candidates, or read by the two tiles ahead of the walk alone) and the extras.
extern "C" int recnow_ibs_rank(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                               const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                               const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                               int batch_candidates, int64_t* n_greater, int64_t* n_equal, int64_t* n_candidates, float* row_pos,
                               void* stream) {
    int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc == RECNOW_OK) rc = ibs_check_extra(extra, ld_extra, ids, extra_ids, N, D);
    if (rc != RECNOW_OK) return rc;
    if (B == 0) return RECNOW_OK;
    if (!n_greater || !n_equal || !n_candidates || !row_pos || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    IbArgs a = {};
    a.own = ibs_side(q, ldq, B, ids, log_q, mask, nullptr, nullptr, 0);
    a.seg[0] = ibs_side(v, ldv, B, ids, log_q, mask, nullptr, nullptr, 1);
    a.nseg = 1;
    if (N > 0) { a.seg[1] = ibs_side(extra, ld_extra, N, extra_ids, extra_log_q, extra_mask, nullptr, nullptr, 0); a.nseg = 2; }
    a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits;
    a.row_pos = row_pos; a.n_greater = n_greater; a.n_equal = n_equal; a.n_cand = n_candidates; a.walk_diag = batch_candidates ? 1 : 0;
    return ibs_launch<3, 1>(a, (hipStream_t)stream);
}

// The K first candidates of every row: MODE 4 over the items (walked as candidates, or not at all) and the extras.
extern "C" int recnow_ibs_topk(const float* q, int64_t ldq, const float* v, int64_t ldv, const int64_t* ids, const float* log_q,
                               const uint8_t* mask, int64_t B, int D, const float* extra, int64_t ld_extra, const int64_t* extra_ids,
                               const float* extra_log_q, const uint8_t* extra_mask, int64_t N, float inv_tau, int remove_hits,
                               int batch_candidates, int K, float* scores, int64_t ld_scores, int64_t* indices, int64_t ld_indices,
                               int64_t* n_candidates, void* stream) {
    int rc = ibs_check(q, ldq, v, ldv, B, D);
    if (rc == RECNOW_OK) rc = ibs_check_extra(extra, ld_extra, ids, extra_ids, N, D);
    if (rc != RECNOW_OK) return rc;
    if (K < 1) return RECNOW_EINVAL;
    if (K > IB_TOPK_MAX_K) return RECNOW_EUNSUPPORTED;
    if (B == 0) return RECNOW_OK;
    if (!scores || !indices || !n_candidates || ld_scores < K || ld_indices < K || !(inv_tau > 0.f)) return RECNOW_EINVAL;
    IbArgs a = {};
    a.own = ibs_side(q, ldq, B, ids, log_q, mask, nullptr, nullptr, 0);
    a.seg[0] = ibs_side(v, ldv, B, ids, log_q, mask, nullptr, nullptr, 1);
    a.nseg = 1;
    if (N > 0) { a.seg[1] = ibs_side(extra, ld_extra, N, extra_ids, extra_log_q, extra_mask, nullptr, nullptr, 0); a.nseg = 2; }
    a.D = D; a.inv_tau = inv_tau; a.remove_hits = remove_hits;
    a.n_cand = n_candidates; a.walk_diag = batch_candidates ? 1 : 0;
    a.K = K; a.top_s = scores; a.ld_top_s = ld_scores; a.top_i = indices; a.ld_top_i = ld_indices;
    return ibs_launch<4, 1>(a, (hipStream_t)stream);
}
