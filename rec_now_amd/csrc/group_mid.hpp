// Device code of the cooperative single-launch grouping (k_group_mid / k_front_mid, grouping.hip): the counterpart of group_small.hpp.
#pragma once
#include "common.hpp"
#include "group_small.hpp"
#include "grouping.hpp"
#ifndef GM_STAMP      // grouping.hip defines the stamps of the -DRN_GS_TRACE build in front of this header
#define GM_STAMP() do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Mid-size batches (8192 < B <= 524288, or several key words): the whole grouping in ONE cooperative launch.
// The general path (scan_sort.hip) is a chain of ~35 launches (per digit: histogram, scan, scatter; then heads, two device-wide scans,
// finish) of a few microseconds of work each -- at BASELINE config 3 (B = 65536) 0.38 ms of kernel time stretched over the side
// stream.  Here G = ceil(B / 2048) <= 256 workgroups (all co-resident: at most one per CU) walk the same phases separated by a
// grid barrier: identity order + varying-bit words | per digit: local histogram | offsets + stable scatter | segment heads + local
// counts | ids.  2 + 2 * (non-trivial digits) barriers of ~5 us each (MI355X_MICROARCH.md, barrier-counter row).
// Barrier = the guide's R1 hand-off: every wave drains its stores, workgroup barrier, lane 0: agent-scope release, arrive on one
// monotonic counter, relaxed agent-scope poll, agent-scope acquire, workgroup barrier, plain loads.  The poll is bounded (2 s):
// on a timeout the error word is set, every later barrier returns at once, the kernel leaves the identity grouping (every row
// its own group: consumers stay in bounds) and n_seg = -1 -- the grid always drains.  The host only takes this route when
// `gm_max_coresident()` says all workgroups fit on the device at once.
// ------------------------------------------------------------------------------------------------
// One flat arrival counter.  Tried and retired (phase stamps of tools/gs_trace.py): arrivals spread over eight counters with a second hop
// (262 144 rows 63.2 -> 62.2 us, but 65 536 rows 41.8 -> 45.3 us and 16 384 rows 22.5 -> 24.8 us: the hop costs more than the contention it removes).
struct GroupMidCtl {          // 128 bytes, zeroed by the host before the launch
    unsigned bar;
    int err;
    unsigned mix[2 * RN_MAX_WORDS];
    unsigned imix[2];         // one key word: OR of the keys' small-integer images and OR of their complements (see gs_int_key)
    unsigned notint;          // != 0: some key has no small-integer image (the keys are sorted as they are)
    unsigned anysolo;         // != 0: some row carries a solo flag (NaN / +-inf id): the heads phase gathers the flags only then
    unsigned pad[10];
};

// Returns false (to every thread of the workgroup) once the error word is set: the caller then leaves through GM_BAIL -- what the other
// workgroups have published so far may be stale, and offsets derived from it could scatter out of bounds.
__device__ __forceinline__ bool gm_barrier(GroupMidCtl* ctl, unsigned target) {
    __shared__ int s_err;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(&ctl->bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(&ctl->bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (__hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            if (wall_clock64() - t0 > 200000000LL) {          // 2 s of the 100 MHz clock
                __hip_atomic_store(&ctl->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_err = __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_err == 0;
}
// A barrier timed out (the workgroups were not co-resident: the host gates this route on the occupancy query, so this is a last line of
// defence; RECNOW_DEBUG_GROUP_TIMEOUT=1 forces it for the tests): this workgroup leaves the identity grouping in ITS ranges -- every row its own
// group -- so that whatever the other workgroups have written or still write, every index in the arrays stays in [0, B] (in-bounds walks for
// every consumer; NOT necessarily a consistent grouping when only some workgroups bail), and n_seg = -1, which `Segments.num_segments()` /
// `recnow_group_segments_status` report and which makes the one-call losses return NaN (k_pair_norm_grad, k_step_dscore, k_lw_norm).  Workgroup 0
// publishes the segment count last and re-reads the error word before it does (end of the kernel).
#define GM_BAR() gm_barrier(ctl, (++nbar) * G)
#define GM_BAIL()                                                                                                    \
    do {                                                                                                             \
        for (int q_ = 0; q_ < TILE / 256; ++q_) {                                                                 \
            const int64_t k_ = (int64_t)g * TILE + q_ * 256 + threadIdx.x;                                      \
            if (k_ < B) { order[k_] = (int32_t)k_; seg_id[k_] = (int32_t)k_; seg_first[k_] = (int32_t)k_; super_id[k_] = (int32_t)k_; } \
        }                                                                                                            \
        if (g == 0 && threadIdx.x == 0) { seg_first[B] = (int32_t)B; n_seg[0] = -1; n_seg[1] = -1; }              \
        return;                                                                                                      \
    } while (0)

// TILE keys per workgroup (256 threads x TILE / 256): 2048, or 4096 from GM_TILE4096_FROM rows on (the host, grouping.hip).
// RAW = 0: canonical key words + solo flags from recnow_group_keys.  RAW = 1 / 2 (round 5, one float32 / int32 id tensor, n_words = 1: the GROUP phase
// of recnow_dcn_mix_step above 8192 rows): `words` IS the id tensor -- every read of it forms the canonical key (-0.0 -> +0.0) on the way, and phase 0
// writes the solo flags (NaN, +-inf) itself, one grid barrier before anybody gathers them: the fill of `solo` and the key kernel in front of this launch go.
template <int RAW>
__device__ __forceinline__ uint32_t gm_canon(uint32_t k) {
    if (RAW == 1) return __uint_as_float(k) == 0.0f ? 0u : k;
    return k;
}
template <int TILE, int RAW>
__device__ __forceinline__ void
group_mid_body(const uint32_t* __restrict__ words, uint8_t* __restrict__ solo, int64_t B, int n_words, int n_words_first,
               GroupMidCtl* __restrict__ ctl, int32_t* __restrict__ idx0, int32_t* __restrict__ idx1, uint32_t* __restrict__ key0,
               uint32_t* __restrict__ key1, unsigned* __restrict__ blockhist, int* __restrict__ headcnt, int32_t* __restrict__ order,
               int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first, int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg,
               const int G, const int g, const int inf_equal) {      // inf_equal (RAW = 1): only NaN ids are solo (the listwise callers: tf.unique equality)
    __shared__ unsigned h[256];
    __shared__ unsigned wcnt[4][256];
    __shared__ unsigned boff[256];
    __shared__ unsigned wtot[4];
    __shared__ unsigned part[4][2 * RN_MAX_WORDS];
    __shared__ unsigned ipart[4][3];
    __shared__ int s_useint, s_anysolo, s_spec;
    __shared__ int s_triv[RN_MAX_PASS], s_src[RN_MAX_PASS], s_carried[RN_MAX_PASS], s_wconst[RN_MAX_WORDS], s_final[2];
    __shared__ int s_cnt[4][2];
    __shared__ int s_red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;      // G workgroups take part, this one is g
    const int Gp = (G + 3) & ~3;
    const int64_t base = (int64_t)g * TILE;
    unsigned nbar = 0;
#ifdef RN_GS_TRACE
    int gm_n = 0;
#endif
    GM_STAMP();
    // ---- phase 0: identity order, bits that vary over the batch ----------------------------------------------------------
    // (round 5) ... and, for one key word, the histogram of the FIRST digit pass on the guess that every key has a small-integer image and that its lowest
    // byte varies (float ids 0 .. 2^24: the usual batch): when the plan behind the barrier agrees (s_spec), pass 0 starts at its offsets -- one grid
    // barrier and one histogram phase less (~8 us of 66 at 262 144 rows).  A wrong guess costs the 2048 LDS atomics; the pass then counts as before.
    h[tid] = 0;
    __syncthreads();
    {
        unsigned o[RN_MAX_WORDS], z[RN_MAX_WORDS];
        unsigned io = 0u, iz = 0u, bad = 0u;                 // small-integer images of the keys (one key word only)
        unsigned anys = 0u;                                   // this thread saw a solo row
#pragma unroll
        for (int w = 0; w < RN_MAX_WORDS; ++w) o[w] = z[w] = 0u;
        // loads from clamped indices, masked afterwards: no load sits under a lane condition (each would end in an `s_waitcnt vmcnt(0)`
        // at its merge, i.e. the eight rounds of a thread would be eight round trips in series)
        for (int w = 0; w < n_words; ++w) {                   // block-uniform trip count
            uint32_t kk[TILE / 256];
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const int64_t i = base + r * 256 + tid;
                kk[r] = gm_canon<RAW>(words[(int64_t)w * B + (i < B ? i : B - 1)]);
            }
            if (RAW == 1) {                                   // the solo flags of this workgroup's keys (read by others only behind a grid barrier)
#pragma unroll
                for (int r = 0; r < TILE / 256; ++r) {
                    const int64_t i = base + r * 256 + tid;
                    const float v = __uint_as_float(kk[r]);
                    const bool fl = inf_equal ? v != v : !(fabsf(v) < INFINITY);
                    if (i < B) solo[i] = fl ? 1 : 0;
                    anys |= (i < B && fl) ? 1u : 0u;
                }
            } else if (RAW == 2) {
#pragma unroll
                for (int r = 0; r < TILE / 256; ++r) {
                    const int64_t i = base + r * 256 + tid;
                    if (i < B) solo[i] = 0;
                }
            }
            unsigned oo = 0u, zz = 0u;
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const bool ok = base + r * 256 + tid < B;
                oo |= ok ? kk[r] : 0u;
                zz |= ok ? ~kk[r] : 0u;
                uint32_t im;
                const bool isint = gs_int_key(kk[r], &im);
                io |= ok ? im : 0u;
                iz |= ok ? ~im : 0u;
                bad |= (ok && !isint) ? 1u : 0u;
                if (ok && n_words == 1) atomicAdd(&h[im & 255u], 1u);
            }
#pragma unroll
            for (int q = 0; q < RN_MAX_WORDS; ++q)
                if (q == w) { o[q] = oo; z[q] = zz; }
        }
        if (RAW == 0) {
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const int64_t i = base + r * 256 + tid;
                anys |= (solo[i < B ? i : B - 1] != 0) ? 1u : 0u;
            }
        }
        if (__ballot(anys != 0u) != 0ull && lane == 0) atomicOr(&ctl->anysolo, 1u);
#pragma unroll
        for (int r = 0; r < TILE / 256; ++r) {
            const int64_t i = base + r * 256 + tid;
            if (i < B) idx0[i] = (int32_t)i;
        }
#pragma unroll
        for (int w = 0; w < RN_MAX_WORDS; ++w)
            if (w < n_words) {
                unsigned a = o[w], c = z[w];
#pragma unroll
                for (int sft = 32; sft > 0; sft >>= 1) {
                    a |= __shfl_xor(a, sft, 64);
                    c |= __shfl_xor(c, sft, 64);
                }
                if (lane == 0) { part[wv][w] = a; part[wv][RN_MAX_WORDS + w] = c; }
            }
        if (n_words == 1) {                                   // block-uniform
#pragma unroll
            for (int sft = 32; sft > 0; sft >>= 1) {
                io |= __shfl_xor(io, sft, 64);
                iz |= __shfl_xor(iz, sft, 64);
                bad |= __shfl_xor(bad, sft, 64);
            }
            if (lane == 0) { ipart[wv][0] = io; ipart[wv][1] = iz; ipart[wv][2] = bad; }
        }
        __syncthreads();
        if (tid < 2 * n_words) {
            const int w = tid % n_words, half = tid / n_words, col = half * RN_MAX_WORDS + w;
            atomicOr(&ctl->mix[half * n_words + w], part[0][col] | part[1][col] | part[2][col] | part[3][col]);
        }
        if (n_words == 1 && tid >= 64 && tid < 67) {
            const int c = tid - 64;
            const unsigned v = ipart[0][c] | ipart[1][c] | ipart[2][c] | ipart[3][c];
            atomicOr(c == 2 ? &ctl->notint : &ctl->imix[c], v);
        }
        if (n_words == 1) blockhist[(int64_t)tid * Gp + g] = h[tid];      // (behind the barrier above: the histogram is complete)
    }
    GM_STAMP();
    if (!GM_BAR()) GM_BAIL();
    GM_STAMP();
    const int np = n_words * 4;
    if (tid == 0) {          // the pass plan, as k_sort_plan builds it (every workgroup derives the same one)
        int cur = 0, word_in_buf = -1;
        const bool useint = n_words == 1 && __hip_atomic_load(&ctl->notint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
        s_useint = useint ? 1 : 0;
        s_anysolo = __hip_atomic_load(&ctl->anysolo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ? 1 : 0;
        for (int p = 0; p < np; ++p) {
            const int w = n_words - 1 - p / 4, d = p % 4;
            const unsigned both = useint ? (__hip_atomic_load(&ctl->imix[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                                            __hip_atomic_load(&ctl->imix[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                         : (__hip_atomic_load(&ctl->mix[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
                                            __hip_atomic_load(&ctl->mix[n_words + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const int tv = ((both >> (8 * d)) & 255u) == 0u;
            s_triv[p] = tv;
            s_src[p] = cur;
            s_carried[p] = word_in_buf == w;
            if (!tv) { cur ^= 1; word_in_buf = w; }
        }
        s_final[0] = cur;
        s_final[1] = word_in_buf;
        s_spec = (useint && !s_triv[0]) ? 1 : 0;             // phase 0 guessed pass 0: integer images, lowest byte
        for (int w = 0; w < n_words; ++w) {
            int c = 1;
            for (int d = 0; d < 4; ++d) c &= s_triv[(n_words - 1 - w) * 4 + d];
            s_wconst[w] = c;
        }
    }
    __syncthreads();
    // ---- digits ---------------------------------------------------------------------------------------------------------------
    for (int p = 0; p < np; ++p) {
        if (s_triv[p]) continue;                              // block-uniform (and the same in every workgroup)
        const int sb = s_src[p];
        const int32_t* src = sb ? idx1 : idx0;
        int32_t* dst = sb ? idx0 : idx1;
        const uint32_t* ksrc = sb ? key1 : key0;
        uint32_t* kdst = sb ? key0 : key1;
        const bool carried = s_carried[p];
        const uint32_t* wk = words + (int64_t)(n_words - 1 - p / 4) * B;
        const int shift = 8 * (p % 4);
        // this tile's keys (kept in registers for the scatter) and its digit histogram
        int32_t my_idx[TILE / 256];
        uint32_t my_key[TILE / 256];
        const bool spec = p == 0 && s_spec != 0;                // block-uniform: blockhist already holds this pass's counts (phase 0)
        h[tid] = 0;
        for (int t = tid; t < 1024; t += 256) (&wcnt[0][0])[t] = 0;
        __syncthreads();
        const int64_t wbase = base + wv * (TILE / 4);
        // all eight rounds' loads in flight together (clamped indices; the block-uniform `carried` chooses between two straight-line
        // load sequences instead of sitting inside every round): two dependent round trips per pass, not sixteen
        if (carried) {
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const int64_t e = wbase + r * 64 + lane, ec = e < B ? e : B - 1;
                my_idx[r] = src[ec];
                my_key[r] = ksrc[ec];
            }
        } else {
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) {
                const int64_t e = wbase + r * 64 + lane;
                my_idx[r] = src[e < B ? e : B - 1];
            }
#pragma unroll
            for (int r = 0; r < TILE / 256; ++r) my_key[r] = gm_canon<RAW>(wk[my_idx[r]]);
            if (s_useint) {                                   // block-uniform: the keys' small-integer images are what is sorted (and carried)
#pragma unroll
                for (int r = 0; r < TILE / 256; ++r) my_key[r] = (uint32_t)__uint_as_float(my_key[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < TILE / 256; ++r) {
            const bool ok = wbase + r * 64 + lane < B;
            my_idx[r] = ok ? my_idx[r] : 0;
            my_key[r] = ok ? my_key[r] : 0u;
            if (ok && !spec) atomicAdd(&h[(my_key[r] >> shift) & 255u], 1u);
        }
        if (!spec) {
            __syncthreads();
            blockhist[(int64_t)tid * Gp + g] = h[tid];        // digit-major, rows of Gp = G rounded up to 4 entries (16-byte row reads below)
            GM_STAMP();
            if (!GM_BAR()) GM_BAIL();
            GM_STAMP();
        }
        {   // first output position of every digit for this workgroup: counts of the workgroups before it + the digits below
            // (round 5: the row is read as 16-byte pieces, sixteen in flight -- one entry per iteration was a chain of G dependent waits: 9.6 us of a
            // pass at G = 128, phase stamps of tools/gs_trace.py; the pad entries of a row are never written and are masked here)
            const uint4* row4 = reinterpret_cast<const uint4*>(blockhist + (int64_t)tid * Gp);
            const int n4 = Gp >> 2;
            unsigned before = 0, total = 0;
            for (int c0 = 0; c0 < n4; c0 += 16) {
                uint4 v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) v[j] = row4[c0 + j < n4 ? c0 + j : n4 - 1];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int b = (c0 + j) * 4;
                    const unsigned e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        total += (c0 + j < n4 && b + q < G) ? e[q] : 0u;
                        before += (c0 + j < n4 && b + q < g) ? e[q] : 0u;
                    }
                }
            }
            unsigned inc = total;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (lane == 63) wtot[wv] = inc;
            __syncthreads();
            unsigned woff = 0;
            for (int i = 0; i < wv; ++i) woff += wtot[i];
            boff[tid] = woff + inc - total + before;
        }
        __syncthreads();
        GM_STAMP();
        // stable ranks: wave w owns TILE / 4 consecutive keys, 8 rounds of 64 consecutive keys (as k_sort_scatter)
        const unsigned long long lt = (1ull << lane) - 1ull;
        unsigned my_dr[TILE / 256];
#pragma unroll
        for (int r = 0; r < TILE / 256; ++r) {
            const int64_t e = wbase + r * 64 + lane;
            const bool ok = e < B;
            const unsigned d = (my_key[r] >> shift) & 255u;
            unsigned long long peers = __ballot(ok);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const unsigned long long m = __ballot(bit);
                peers &= bit ? m : ~m;
            }
            const unsigned prior = ok ? wcnt[wv][d] : 0u;
            const unsigned rank = prior + (unsigned)__popcll(peers & lt);
            if (ok && (peers & lt) == 0ull) wcnt[wv][d] = prior + (unsigned)__popcll(peers);
            my_dr[r] = d | (rank << 8);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < TILE / 256; ++r) {
            const int64_t e = wbase + r * 64 + lane;
            if (e < B) {
                const unsigned d = my_dr[r] & 255u, rank = my_dr[r] >> 8;
                unsigned off = boff[d] + rank;
                for (int pw = 0; pw < wv; ++pw) off += wcnt[pw][d];
                // plain stores (merged in L2, written back by the barrier's release fence): written through (sc1) these RANDOM 4-byte stores become
                // partial writes to memory -- scatter phase 5.7 -> 11.9 us, the launch 62 -> 72-74 us at 262 144 rows
                dst[off] = my_idx[r];
                kdst[off] = my_key[r];
            }
        }
        GM_STAMP();
        if (!GM_BAR()) GM_BAIL();
        GM_STAMP();
    }
    // ---- segments: heads of this tile's sorted positions ------------------------------------------------------------------------------------
    // Round 5: thread (round r, tid) owns position base + r * 256 + tid, so every array access of this phase is coalesced (with TILE / 256 CONSECUTIVE
    // positions per thread a wave instruction read 64 pieces 32-64 bytes apart: 9.4 us of 74 at 262 144 rows, phase stamps of tools/gs_trace.py).  A
    // position's predecessor is the lane below; across waves and rounds the edge values go through LDS, the block's own predecessor is a uniform load.
    // The solo flags are gathered only when the batch has any (ctl->anysolo, set in phase 0).
    const int32_t* fin = s_final[0] ? idx1 : idx0;
    const uint32_t* kfin = s_final[0] ? key1 : key0;
    const int final_word = s_final[1];
    constexpr int R = TILE / 256;
    __shared__ uint32_t s_edge[R][4];                         // the value of lane 63 of (round, wave)
    __shared__ int s_hc[R][4], s_sc[R][4];                    // heads of (round, wave); then their exclusive prefix in (round, wave) order
    const unsigned long long ltm = (1ull << lane) - 1ull;
    const int64_t kprev = base > 0 ? base - 1 : 0;            // the block's predecessor (position 0 has none: it is a head by definition)
    int32_t f[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t k = base + r * 256 + tid;
        f[r] = fin[k < B ? k : B - 1];
    }
    const int32_t fprev = fin[kprev];
    // pv[r] = the value of position k - 1 for this thread's position of round r (vb: the value in front of the block)
    auto prev_of = [&](const uint32_t (&v)[R], uint32_t vb, uint32_t (&pv)[R]) {
        if (lane == 63) {
#pragma unroll
            for (int r = 0; r < R; ++r) s_edge[r][wv] = v[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t pr = __shfl_up(v[r], 1, 64);
            if (lane == 0) pr = wv > 0 ? s_edge[r][wv - 1] : (r > 0 ? s_edge[r > 0 ? r - 1 : 0][3] : vb);
            pv[r] = pr;
        }
        __syncthreads();
    };
    unsigned dany = 0u, dfirst = 0u, sob = 0u;                // bit r: position k and k - 1 differ in some / in a groups[0] word; one of them is solo
    if (s_anysolo) {                                          // block-uniform (and the same in every workgroup)
        uint32_t sv[R], sp[R];
#pragma unroll
        for (int r = 0; r < R; ++r) sv[r] = solo[f[r]];
        const uint32_t vb = solo[fprev];
        prev_of(sv, vb, sp);
#pragma unroll
        for (int r = 0; r < R; ++r) sob |= ((sv[r] | sp[r]) != 0u ? 1u : 0u) << r;
    }
    for (int w = 0; w < n_words; ++w) {                       // block-uniform
        if (s_wconst[w]) continue;
        uint32_t v[R], pv[R], vb;
        if (w == final_word) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t k = base + r * 256 + tid;
                v[r] = kfin[k < B ? k : B - 1];
            }
            vb = kfin[kprev];
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) v[r] = gm_canon<RAW>(words[(int64_t)w * B + f[r]]);
            vb = gm_canon<RAW>(words[(int64_t)w * B + fprev]);
        }
        prev_of(v, vb, pv);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned df = v[r] != pv[r] ? 1u : 0u;
            dany |= df << r;
            if (w < n_words_first) dfirst |= df << r;
        }
    }
    unsigned hb = 0, sbm = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t k = base + r * 256 + tid;
        const bool valid = k < B;
        const bool so = (sob >> r) & 1u;
        const bool hd = valid && (k == 0 || so || ((dany >> r) & 1u));
        const bool sh = valid && (k == 0 || so || ((dfirst >> r) & 1u));
        hb |= (hd ? 1u : 0u) << r;
        sbm |= (sh ? 1u : 0u) << r;
        const unsigned long long mh = __ballot(hd), ms = __ballot(sh);
        if (lane == 0) { s_hc[r][wv] = (int)__popcll(mh); s_sc[r][wv] = (int)__popcll(ms); }
        if (valid) order[k] = f[r];
    }
    __syncthreads();
    if (wv == 0) {                                            // exclusive prefix of the 4 R <= 64 counts in (round, wave) order
        int* hc = &s_hc[0][0];
        int* sc = &s_sc[0][0];
        const int a = lane < 4 * R ? hc[lane] : 0, c = lane < 4 * R ? sc[lane] : 0;
        int ia = a, ic = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t1 = __shfl_up(ia, o, 64), t2 = __shfl_up(ic, o, 64);
            if (lane >= o) { ia += t1; ic += t2; }
        }
        if (lane < 4 * R) { hc[lane] = ia - a; sc[lane] = ic - c; }
        if (lane == 63) { s_cnt[0][0] = ia; s_cnt[0][1] = ic; }
    }
    __syncthreads();
    if (tid == 0) { headcnt[2 * g] = s_cnt[0][0]; headcnt[2 * g + 1] = s_cnt[0][1]; }
    GM_STAMP();
    if (!GM_BAR()) GM_BAIL();
    GM_STAMP();
    int preh = 0, pres = 0, allh = 0, alls = 0;              // heads in the workgroups before this one / in all of them
    {   // thread b reads workgroup b's pair (G <= 256 = the block), block reduction (round 5: every thread walked all G pairs: 9 us at G = 128)
        const int bc = tid < G ? tid : G - 1;
        const int a0 = headcnt[2 * bc], c0 = headcnt[2 * bc + 1];
        int r4[4] = {tid < g ? a0 : 0, tid < g ? c0 : 0, tid < G ? a0 : 0, tid < G ? c0 : 0};
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r4[q] += __shfl_xor(r4[q], o, 64);
        }
        if (lane == 0) { s_red[wv][0] = r4[0]; s_red[wv][1] = r4[1]; s_red[wv][2] = r4[2]; s_red[wv][3] = r4[3]; }
        __syncthreads();
        for (int i = 0; i < 4; ++i) { preh += s_red[i][0]; pres += s_red[i][1]; allh += s_red[i][2]; alls += s_red[i][3]; }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t k = base + r * 256 + tid;
        const bool hd = (hb >> r) & 1u, sh = (sbm >> r) & 1u;
        const unsigned long long mh = __ballot(hd), ms = __ballot(sh);
        const int eh = preh + s_hc[r][wv] + (int)__popcll(mh & ltm);      // heads in front of position k
        const int es = pres + s_sc[r][wv] + (int)__popcll(ms & ltm);
        if (k < B) {
            if (hd) seg_first[eh] = (int32_t)k;
            seg_id[k] = hd ? eh : eh - 1;
            super_id[k] = sh ? es : es - 1;
        }
    }
    if (g == 0 && tid == 0) {
        // a workgroup can time out at the LAST barrier and set ctl->err just as the last arrival completes the count; its peers
        // may have read err before that and passed.  The bailing workgroup then rewrites ITS ranges with the identity grouping while the others
        // write real segments -- every value stays in [0, B] (walks stay in bounds), but the arrays are not a grouping.  So the error word is
        // read once more here, after this workgroup's own writes, and the count is published as -1 (every consumer poisons its result on
        // n_seg < 0) whenever any workgroup has reported a time-out by now.
        const int late = __hip_atomic_load(&ctl->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seg_first[allh] = (int32_t)B;
        n_seg[0] = late ? -1 : allh;
        n_seg[1] = late ? -1 : alls;
    }
    GM_STAMP();
}
