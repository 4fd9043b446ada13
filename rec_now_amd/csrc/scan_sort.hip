// Grouping machinery (integer path): canonical keys, stable LSD radix sort of row indices, device-wide scans,
// segment detection.  Replaces the reference's dense (B,B) same-group mask
// (/root/reference/rec_now/rec_block/pairwise_loss_from_batch.py:16-40,43-74) and tf.unique_with_counts
// (/root/reference/rec_now/rec_block/listwise_loss_from_batch.py:109).
//
// HBM-bound integer work on <= a few MB: everything here is about few launches, coalesced 4-B streams and
// LDS-resident counters, not MFMA.
// The one-launch routes for what fits one workgroup or one co-resident grid, and the driver the consumers call, are in grouping.hip.
#include "common.hpp"
#include "scan.hpp"
#include "grouping.hpp"

// ------------------------------------------------------------------------------------------------
// keys
// ------------------------------------------------------------------------------------------------
// inf_equal (RECNOW_KEY_INF_EQUAL, the listwise callers): tf.unique equality -- equal infinities are one group, only NaN rows are solo
__global__ void k_keys_f32(const float* __restrict__ g, int64_t B, uint32_t* __restrict__ w0, uint8_t* __restrict__ solo, int inf_equal) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float v = g[i];
    uint32_t u = __float_as_uint(v);
    if (v == 0.0f) u = 0u;                       // -0.0 == +0.0
    if (inf_equal ? v != v : !(fabsf(v) < INFINITY)) solo[i] = 1;      // NaN, +-inf: v - v is NaN -> equals nothing
    w0[i] = u;
}
__global__ void k_keys_f64(const double* __restrict__ g, int64_t B, uint32_t* __restrict__ w, uint8_t* __restrict__ solo, int inf_equal) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    double v = g[i];
    uint64_t u = (uint64_t)__double_as_longlong(v);
    if (v == 0.0) u = 0ull;
    if (inf_equal ? v != v : !(fabs(v) < (double)INFINITY)) solo[i] = 1;
    w[i] = (uint32_t)(u >> 32);
    w[B + i] = (uint32_t)u;
}
__global__ void k_keys_i32(const int32_t* __restrict__ g, int64_t B, uint32_t* __restrict__ w0) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) w0[i] = (uint32_t)g[i];
}
__global__ void k_keys_i64(const int64_t* __restrict__ g, int64_t B, uint32_t* __restrict__ w) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    uint64_t u = (uint64_t)g[i];
    w[i] = (uint32_t)(u >> 32);
    w[B + i] = (uint32_t)u;
}

extern "C" int recnow_key_words(int dtype) {
    switch (dtype & ~RECNOW_KEY_INF_EQUAL) {
        case RECNOW_KEY_F32: case RECNOW_KEY_I32: return 1;
        case RECNOW_KEY_F64: case RECNOW_KEY_I64: return 2;
        default: return RECNOW_EINVAL;
    }
}

extern "C" int recnow_group_keys(const void* group, int dtype, int64_t B, uint32_t* words, uint8_t* solo, void* stream) {
    if (B < 0 || recnow_key_words(dtype) < 0) return RECNOW_EINVAL;
    if (B == 0) return RECNOW_OK;
    if (!group || !words || !solo) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int T = 256, G = rn_cdiv(B, T);
    const int inf_equal = (dtype & RECNOW_KEY_INF_EQUAL) ? 1 : 0;
    switch (dtype & ~RECNOW_KEY_INF_EQUAL) {
        case RECNOW_KEY_F32: hipLaunchKernelGGL(k_keys_f32, G, T, 0, st, (const float*)group, B, words, solo, inf_equal); break;
        case RECNOW_KEY_F64: hipLaunchKernelGGL(k_keys_f64, G, T, 0, st, (const double*)group, B, words, solo, inf_equal); break;
        case RECNOW_KEY_I32: hipLaunchKernelGGL(k_keys_i32, G, T, 0, st, (const int32_t*)group, B, words); break;
        case RECNOW_KEY_I64: hipLaunchKernelGGL(k_keys_i64, G, T, 0, st, (const int64_t*)group, B, words); break;
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// ------------------------------------------------------------------------------------------------
// radix sort of row indices by n_words x 32-bit keys, 8-bit digits, LSD, stable.
// The index array is permuted, and beside it the values of the key word being sorted travel in the same order, so that
// only the first pass on a word gathers it through the index (for millions of keys every gathered 4-byte word costs a
// 64-byte sector; the first pass of all reads through the identity order, i.e. coalesced).
// Passes whose digit is constant over all rows are skipped on the device (plan), so float-encoded small ids
// cost 2-3 passes instead of 4.
// ------------------------------------------------------------------------------------------------
// (RN_MAX_WORDS, RN_TILE = keys per block per pass, and the pass plan `SortPlan`: grouping.hpp)

// Which digits vary over the batch?  A pass is skippable iff its digit is the same in every key, i.e. iff no bit of that
// byte is 1 in some key and 0 in another: mix[w] = OR of the keys' word w, mix[n_words + w] = OR of its complement; the
// bits set in both are the varying ones.  (Full 256-bin histograms of every digit answered the same question with eight
// LDS atomics per key -- 0.15 ms for 6.5 M ids whose hot values serialise on one bin.)  Also writes the identity order.
__global__ void __launch_bounds__(256)
k_sort_ghist(const uint32_t* __restrict__ words, int64_t B, int n_words, unsigned* __restrict__ mix, int32_t* __restrict__ idx0) {
    __shared__ unsigned part[4][2 * RN_MAX_WORDS];
    unsigned o[RN_MAX_WORDS], z[RN_MAX_WORDS];
#pragma unroll
    for (int w = 0; w < RN_MAX_WORDS; ++w) o[w] = z[w] = 0u;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (int64_t)gridDim.x * blockDim.x) {
        idx0[i] = (int32_t)i;                   // the identity order the first pass starts from
#pragma unroll
        for (int w = 0; w < RN_MAX_WORDS; ++w)
            if (w < n_words) {
                const uint32_t k = words[(int64_t)w * B + i];
                o[w] |= k;
                z[w] |= ~k;
            }
    }
#pragma unroll
    for (int w = 0; w < RN_MAX_WORDS; ++w)
        if (w < n_words) {
            unsigned a = o[w], c = z[w];
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                a |= __shfl_xor(a, s, 64);
                c |= __shfl_xor(c, s, 64);
            }
            if ((threadIdx.x & 63) == 0) {
                part[threadIdx.x >> 6][w] = a;
                part[threadIdx.x >> 6][RN_MAX_WORDS + w] = c;
            }
        }
    __syncthreads();
    // one pair of atomics per word and WORKGROUP: thousands of atomics on the same few addresses serialise in the L2
    if ((int)threadIdx.x < 2 * n_words) {
        const int w = threadIdx.x % n_words, half = threadIdx.x / n_words;
        const int col = half * RN_MAX_WORDS + w;
        atomicOr(&mix[half * n_words + w], part[0][col] | part[1][col] | part[2][col] | part[3][col]);
    }
}

// pass p sorts by word w = n_words-1 - p/4, digit d = p%4 (LSD overall)
__global__ void k_sort_plan(const unsigned* __restrict__ mix, int64_t B, int n_words, SortPlan* plan) {
    __shared__ int triv[RN_MAX_PASS];
    const int np = n_words * 4;
    if (threadIdx.x < RN_MAX_PASS) triv[threadIdx.x] = 0;
    __syncthreads();
    if ((int)threadIdx.x < np) {
        const int p = threadIdx.x, w = n_words - 1 - p / 4, d = p % 4;
        triv[p] = (((mix[w] & mix[n_words + w]) >> (8 * d)) & 255u) == 0u;           // no bit of the byte differs between keys
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int cur = 0, word_in_buf = -1;
        for (int p = 0; p < np; ++p) {
            const int w = n_words - 1 - p / 4;
            plan->trivial[p] = triv[p];
            plan->src[p] = cur;
            plan->carried[p] = word_in_buf == w;
            if (!triv[p]) {                      // the scatter of pass p leaves word w beside the permuted indices
                cur ^= 1;
                word_in_buf = w;
            }
        }
        plan->final_buf = cur;
        plan->final_word = word_in_buf;
        for (int w = 0; w < n_words; ++w) {
            int c = 1;
            for (int d = 0; d < 4; ++d) c &= triv[(n_words - 1 - w) * 4 + d];
            plan->word_const[w] = c;
        }
    }
}

__global__ void __launch_bounds__(256)
k_sort_blockhist(const uint32_t* __restrict__ words, int64_t B, int n_words, int pass, const SortPlan* __restrict__ plan,
                 const int32_t* __restrict__ idx0, const int32_t* __restrict__ idx1, const uint32_t* __restrict__ key0,
                 const uint32_t* __restrict__ key1, unsigned* __restrict__ blockhist, int nblk) {
    if (plan->trivial[pass]) return;
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int32_t* src = plan->src[pass] ? idx1 : idx0;
    const uint32_t* ksrc = plan->src[pass] ? key1 : key0;
    const bool carried = plan->carried[pass];
    const uint32_t* wk = words + (int64_t)(n_words - 1 - pass / 4) * B;
    const int shift = 8 * (pass % 4);
    const int64_t base = (int64_t)blockIdx.x * RN_TILE;
    // One LDS atomic per DISTINCT digit of a wave's 64 keys (the lanes that share a digit are found with eight ballots, the lowest of them adds
    // their count): heavy-tailed keys -- pooled embedding ids, where one id owns a quarter of the entries -- put most lanes of every wave on ONE
    // bin, and 64 atomics on one LDS address serialise (round 5: 38 -> ~20 us per pass at 6.5 M ids; uniform digits cost the ballots, ~1 us).
    const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
    uint32_t kv[RN_TILE / 256];
#pragma unroll
    for (int r = 0; r < RN_TILE / 256; ++r) {           // all loads of the tile in flight before the first ballot
        const int64_t e = base + r * 256 + threadIdx.x;
        kv[r] = e < B ? (carried ? ksrc[e] : wk[src[e]]) : 0u;
    }
#pragma unroll
    for (int r = 0; r < RN_TILE / 256; ++r) {
        const int64_t e = base + r * 256 + threadIdx.x;
        const bool ok = e < B;
        const unsigned d = (kv[r] >> shift) & 255u;
        unsigned long long peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        if (ok && (peers & lt) == 0ull) atomicAdd(&h[d], (unsigned)__popcll(peers));
    }
    __syncthreads();
    blockhist[(int64_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];   // digit-major
}

// stable scatter: wave w of the block owns RN_TILE/4 consecutive keys, 8 rounds of 64 consecutive keys.
__global__ void __launch_bounds__(256)
k_sort_scatter(const uint32_t* __restrict__ words, int64_t B, int n_words, int pass, const SortPlan* __restrict__ plan,
               int32_t* __restrict__ idx0, int32_t* __restrict__ idx1, uint32_t* __restrict__ key0, uint32_t* __restrict__ key1,
               const unsigned* __restrict__ blockoff, int nblk, int scan_here) {
    if (plan->trivial[pass]) return;
    __shared__ unsigned wcnt[4][256];
    __shared__ unsigned boff[256];          // scan_here: this block's first output position of every digit
    __shared__ unsigned wtot[4];
    for (int t = threadIdx.x; t < 1024; t += 256) (&wcnt[0][0])[t] = 0;
    if (scan_here) {
        // `blockoff` holds the RAW digit-major counts [256][nblk]: thread d adds up digit d's row (the part before this block
        // separately), then the 256 row totals are scanned -- one launch less per pass than a separate scan kernel, which
        // matters because a grouping call is a chain of ~30 few-microsecond launches
        const unsigned* row = blockoff + (int64_t)threadIdx.x * nblk;
        unsigned before = 0, total = 0;
        for (int b = 0; b < nblk; ++b) {
            const unsigned v = row[b];
            before += b < (int)blockIdx.x ? v : 0u;
            total += v;
        }
        const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
        unsigned inc = total;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (ln >= o) inc += t;
        }
        if (ln == 63) wtot[wv] = inc;
        __syncthreads();
        unsigned woff = 0;
        for (int i = 0; i < wv; ++i) woff += wtot[i];
        boff[threadIdx.x] = woff + inc - total + before;
    }
    __syncthreads();
    const int sb = plan->src[pass];
    const int32_t* src = sb ? idx1 : idx0;
    int32_t* dst = sb ? idx0 : idx1;
    const uint32_t* ksrc = sb ? key1 : key0;
    uint32_t* kdst = sb ? key0 : key1;
    const bool carried = plan->carried[pass];
    const uint32_t* wk = words + (int64_t)(n_words - 1 - pass / 4) * B;
    const int shift = 8 * (pass % 4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wbase = (int64_t)blockIdx.x * RN_TILE + w * (RN_TILE / 4);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int32_t my_idx[RN_TILE / 256];
    uint32_t my_key[RN_TILE / 256];
    unsigned my_dr[RN_TILE / 256];        // digit | (rank_in_wave << 8)
#pragma unroll
    for (int r = 0; r < RN_TILE / 256; ++r) {
        const int64_t e = wbase + r * 64 + lane;
        const bool ok = e < B;
        int32_t id = ok ? src[e] : 0;
        const uint32_t kv = ok ? (carried ? ksrc[e] : wk[id]) : 0u;
        unsigned d = (kv >> shift) & 255u;
        unsigned long long peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        unsigned prior = ok ? wcnt[w][d] : 0u;                 // every lane reads before any leader adds
        const unsigned rank = prior + (unsigned)__popcll(peers & lt);
        if (ok && (peers & lt) == 0ull) wcnt[w][d] = prior + (unsigned)__popcll(peers);   // leader = lowest peer
        my_idx[r] = id;
        my_key[r] = kv;
        my_dr[r] = d | (rank << 8);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RN_TILE / 256; ++r) {
        const int64_t e = wbase + r * 64 + lane;
        if (e < B) {
            const unsigned d = my_dr[r] & 255u, rank = my_dr[r] >> 8;
            unsigned off = (scan_here ? boff[d] : blockoff[(int64_t)d * nblk + blockIdx.x]) + rank;
            for (int pw = 0; pw < w; ++pw) off += wcnt[pw][d];
            dst[off] = my_idx[r];
            kdst[off] = my_key[r];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// segments
// ------------------------------------------------------------------------------------------------
__global__ void k_seg_heads(const uint32_t* __restrict__ words, const uint8_t* __restrict__ solo, int64_t B, int n_words,
                            int n_words_first, const SortPlan* __restrict__ plan, const int32_t* __restrict__ idx0,
                            const int32_t* __restrict__ idx1, const uint32_t* __restrict__ key0, const uint32_t* __restrict__ key1,
                            int32_t* __restrict__ order, int32_t* __restrict__ head, int32_t* __restrict__ shead) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    const int32_t* fin = plan->final_buf ? idx1 : idx0;
    const uint32_t* kfin = plan->final_buf ? key1 : key0;       // values of word plan->final_word in sorted order
    const int32_t i = fin[k];
    order[k] = i;
    int h = 1, sh = 1;
    if (k > 0) {
        const int32_t j = fin[k - 1];
        const bool s = solo[i] | solo[j];
        bool diff_first = false, diff_any = false;
        for (int w = 0; w < n_words; ++w) {
            if (plan->word_const[w]) continue;                   // one value over the batch: neighbours cannot differ in it
            const bool d = w == plan->final_word ? kfin[k] != kfin[k - 1]
                                                 : words[(int64_t)w * B + i] != words[(int64_t)w * B + j];
            diff_any |= d;
            if (w < n_words_first) diff_first |= d;
        }
        h = (s || diff_any) ? 1 : 0;
        sh = (s || diff_first) ? 1 : 0;
    }
    head[k] = h;
    shead[k] = sh;
}

__global__ void k_seg_finish(const int32_t* __restrict__ head, const int32_t* __restrict__ seg_incl,
                             const int32_t* __restrict__ super_incl, int64_t B, int32_t* __restrict__ seg_id,
                             int32_t* __restrict__ seg_first, int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B) return;
    const int32_t g = seg_incl[k] - 1;
    seg_id[k] = g;
    super_id[k] = super_incl[k] - 1;
    if (head[k]) seg_first[g] = (int32_t)k;
    if (k == B - 1) {
        seg_first[g + 1] = (int32_t)B;
        n_seg[0] = g + 1;
        n_seg[1] = super_incl[k];
    }
}

__global__ void k_seg_empty(int32_t* seg_first, int32_t* n_seg) {
    seg_first[0] = 0;
    n_seg[0] = 0;
    n_seg[1] = 0;
}


extern "C" int recnow_group_segments(const uint32_t* words, const uint8_t* solo, int64_t B, int n_words, int n_words_first,
                                     int32_t* order, int32_t* seg_id, int32_t* seg_first, int32_t* super_id, int32_t* n_seg,
                                     void* ws, size_t ws_bytes, void* stream) {
    if (B < 0 || B > 0x7fffff00ll || n_words < 1 || n_words > RN_MAX_WORDS || n_words_first < 1 || n_words_first > n_words)
        return RECNOW_EINVAL;
    if (!seg_first || !n_seg) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {
        hipLaunchKernelGGL(k_seg_empty, 1, 1, 0, st, seg_first, n_seg);
        RN_LAUNCH_CHECK();
        return RECNOW_OK;
    }
    if (!words || !solo || !order || !seg_id || !super_id || !ws) return RECNOW_EINVAL;
    if (ws_bytes < recnow_group_segments_workspace_bytes(B, n_words)) return RECNOW_EWORKSPACE;
    // one launch where one fits (grouping.hip: one workgroup, or the cooperative launch); else the chain below
    const int rc0 = rn_group_words(words, solo, B, n_words, n_words_first, order, seg_id, seg_first, super_id, n_seg, ws, st);
    if (rc0 != RECNOW_EUNSUPPORTED) return rc0;
    const int nblk = rn_cdiv(B, RN_TILE);
    const RnGroupWs w = rn_group_ws(ws, B, n_words);
    RN_HIP(hipMemsetAsync(w.mix, 0, (size_t)2 * n_words * sizeof(unsigned), st));
    const int T = 256, G = rn_cdiv(B, T);
    {
        int gh = rn_cdiv(B, 256 * 8);
        if (gh > 1024) gh = 1024;
        hipLaunchKernelGGL(k_sort_ghist, gh, 256, 0, st, words, B, n_words, w.mix, w.idx0);
    }
    hipLaunchKernelGGL(k_sort_plan, 1, 256, 0, st, w.mix, B, n_words, w.plan);
    for (int p = 0; p < n_words * 4; ++p) {
        hipLaunchKernelGGL(k_sort_blockhist, nblk, 256, 0, st, words, B, n_words, p, w.plan, w.idx0, w.idx1, w.key0, w.key1, w.blockhist, nblk);
        const int scan_here = nblk <= 128;      // few blocks: every scatter workgroup scans the raw counts itself
        if (!scan_here) {   // millions of keys (pooled embedding ids): device-wide scan, in place (a skipped pass scans stale counts, unused)
            int rc2 = rn_scan<unsigned, unsigned, 0>(w.blockhist, w.blockhist, 256 * (int64_t)nblk, 0, w.scan, w.scan_bytes, st);
            if (rc2) return rc2;
        }
        hipLaunchKernelGGL(k_sort_scatter, nblk, 256, 0, st, words, B, n_words, p, w.plan, w.idx0, w.idx1, w.key0, w.key1, w.blockhist, nblk, scan_here);
    }
    hipLaunchKernelGGL(k_seg_heads, G, T, 0, st, words, solo, B, n_words, n_words_first, w.plan, w.idx0, w.idx1, w.key0, w.key1, order, w.head, w.shead);
    RN_LAUNCH_CHECK();
    int rc = rn_inclusive_scan_i32(w.head, w.seg_incl, B, w.scan, w.scan_bytes, st);
    if (rc) return rc;
    // every word belongs to groups[0] (the pooled lookup's ids, any single id tensor): a super-segment IS a segment -- k_seg_heads wrote equal flags --
    // and the second device-wide scan (37 us of the 6.5 M ids of the pooled lookup's backward) is the first one
    const bool same = n_words_first == n_words;
    if (!same) {
        rc = rn_inclusive_scan_i32(w.shead, w.super_incl, B, w.scan, w.scan_bytes, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_seg_finish, G, T, 0, st, w.head, w.seg_incl, same ? w.seg_incl : w.super_incl, B, seg_id, seg_first, super_id, n_seg);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
