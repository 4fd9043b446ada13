// The grouping front end: the one-launch kernels (one workgroup: group_small.hpp; cooperative: group_mid.hpp), the workspace layout, and the one
// driver every consumer calls (grouping.hpp).  Key formation and the multi-launch chain for what fits no single launch are in scan_sort.hip.
#include "common.hpp"
#include "scan.hpp"
#include "grouping.hpp"
#include "group_small.hpp"
#include "dcnmix_tile.hpp"
#define RN_FRONT_PACK_WGS 255      // pack workgroups of the step's front kernels (k_front_small / k_front_mid)
// diagnostic build (tools/build_variant.py gstrace -DRN_GS_TRACE, tools/gs_trace.py): wall-clock stamps (100 MHz) of thread 0
#ifdef RN_GS_TRACE
__device__ long long g_gs_trace[16];
#define GS_STAMP(i) do { if (threadIdx.x == 0) g_gs_trace[(i)] = wall_clock64(); } while (0)
__device__ long long g_gm_trace[64];
__device__ int g_gm_n;
#define GM_STAMP() do { if (g == GM_TRACE_WG && threadIdx.x == 0) { g_gm_trace[gm_n < 63 ? gm_n : 63] = wall_clock64(); ++gm_n; g_gm_n = gm_n; } } while (0)
#ifndef GM_TRACE_WG
#define GM_TRACE_WG 0
#endif
extern "C" int recnow_debug_gm_trace(long long* out) { int n = 0; hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_gm_n), sizeof(int)); hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gm_trace), sizeof(long long) * 64); return n; }
extern "C" int recnow_debug_gs_trace(long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gs_trace), sizeof(long long) * 16); }
#else
#define GS_STAMP(i) do { } while (0)
#define GM_STAMP() do { } while (0)
#endif
#include "group_mid.hpp"

// ------------------------------------------------------------------------------------------------
// Small batches (B <= 8192, one 32-bit key word): the whole grouping -- stable LSD radix sort, segment heads, segment ids --
// in ONE workgroup on LDS-resident keys.  The general path (scan_sort.hip) is ~24 launches of a few microseconds each, which is all
// of the time at BASELINE config 2 (B = 8192: 0.24 ms per loss, launch-latency bound).
//   1024 threads, thread t owns the 8 consecutive positions [8t, 8t+8) of the current order (so ranks are stable);
//   4-bit digits: a thread's 16 digit counters (each <= 8) pack into one 64-bit register; passes whose digit is constant
//   over the batch are skipped (OR/AND of all keys); counters [16][1024] u16 are scanned block-wide in digit-major order.
// ------------------------------------------------------------------------------------------------
// RAW = 0: canonical key words + solo flags from recnow_group_keys (the C ABI's two-call form).  RAW = 1 / 2 (round 5, the step's GROUP phase at
// shard sizes): `words` IS the caller's float32 / int32 id tensor -- the canonical key (-0.0 -> +0.0) and the solo flag (NaN, +-inf) of
// k_keys_f32 are formed here and the flags live in an LDS bit set, so that the phase is ONE launch instead of a fill, a key kernel and this one
// (kernel trace at 8192 rows: 5.2 + 5.0 + 31.8 us in front of the forward launch).
template <int RAW>
__device__ __forceinline__ void
group_small_body(const uint32_t* __restrict__ words, const uint8_t* __restrict__ solo, int B, int32_t* __restrict__ order,
                 int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first, int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
    uint32_t* key0 = reinterpret_cast<uint32_t*>(gs_lds);
    uint32_t* key1 = key0 + GS_MAXB;
    uint16_t* idx0 = reinterpret_cast<uint16_t*>(key1 + GS_MAXB);
    uint16_t* idx1 = idx0 + GS_MAXB;
    uint16_t* cnt = idx1 + GS_MAXB;                       // [16][GS_T]
    unsigned* wsum = reinterpret_cast<unsigned*>(cnt + 16 * GS_T);   // [16] + 2
    __shared__ unsigned s_solo[GS_MAXB / 32];             // RAW: bit i = row i pairs with nobody
    const int tid = threadIdx.x;
    GS_STAMP(0);
    if (RAW == 1) {
        for (int i = tid; i < GS_MAXB / 32; i += GS_T) s_solo[i] = 0u;
        __syncthreads();
    }
    auto is_solo = [&](int row) -> bool { return RAW == 0 ? solo[row] != 0 : RAW == 1 ? ((s_solo[row >> 5] >> (row & 31)) & 1u) != 0u : false; };
    unsigned vor = 0, vand = 0xffffffffu, ior = 0, iand = 0xffffffffu, bad = 0;
    for (int i = tid; i < B; i += GS_T) {
        uint32_t k = words[i];
        if (RAW == 1) {
            const float v = __uint_as_float(k);
            if (v == 0.0f) k = 0u;                        // -0.0 == +0.0
            if (!(fabsf(v) < INFINITY)) atomicOr(&s_solo[i >> 5], 1u << (i & 31));
        }
        key0[i] = k;
        idx0[i] = (uint16_t)i;
        vor |= k;
        vand &= k;
        uint32_t im;
        bad |= gs_int_key(k, &im) ? 0u : 1u;
        ior |= im;
        iand &= im;
    }
    GS_STAMP(1);
    const unsigned varying = gs_varying_bits(key0, B, vor, vand, ior, iand, bad, wsum);      // (keys rewritten to their small-integer images when all have one)
    GS_STAMP(2);
    uint32_t* ka = key0; uint32_t* kb = key1;
    uint16_t* ia = idx0; uint16_t* ib = idx1;
    const int lo = tid * GS_KPT, hi = min(B, lo + GS_KPT);
    gs_radix_sort_lds(ka, kb, ia, ib, cnt, wsum, B, varying);
    GS_STAMP(3);
    // segment heads over the sorted order; solo rows (NaN / inf ids) are segments of their own
    unsigned heads = 0, nh = 0;
    for (int i = lo; i < hi; ++i) {
        bool h = true;
        if (i > 0) h = (ka[i] != ka[i - 1]) || is_solo(ia[i]) || is_solo(ia[i - 1]);
        heads |= (h ? 1u : 0u) << (i - lo);
        nh += h ? 1u : 0u;
    }
    unsigned total = 0;
    unsigned g = gs_block_exclusive_scan(nh, wsum, &total);
    GS_STAMP(4);
    for (int i = lo; i < hi; ++i) {
        const bool h = (heads >> (i - lo)) & 1u;
        if (h) { seg_first[g] = i; ++g; }
        order[i] = (int32_t)ia[i];
        seg_id[i] = (int32_t)g - 1;
        super_id[i] = (int32_t)g - 1;
    }
    if (tid == 0) {
        seg_first[total] = B;
        n_seg[0] = (int32_t)total;
        n_seg[1] = (int32_t)total;
    }
    GS_STAMP(5);
#ifdef RN_GS_TRACE
    if (threadIdx.x == 0) g_gs_trace[6] = (long long)varying;
#endif
}
template <int RAW>
__global__ void __launch_bounds__(GS_T)
k_group_small(const uint32_t* __restrict__ words, const uint8_t* __restrict__ solo, int B, int32_t* __restrict__ order,
              int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first, int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg) {
    group_small_body<RAW>(words, solo, B, order, seg_id, seg_first, super_id, n_seg);
}
// Front kernel of recnow_dcn_mix_step at shard sizes (round 5): workgroup 0 groups the batch, the others write the weight packs of the row-block
// kernels (dcnmix_tile.hpp) -- two launches that depend on nothing but the step's inputs, one of which keeps ONE compute unit busy for ~20 us.
template <int RAW>
__global__ void __launch_bounds__(GS_T)
k_front_small(const uint32_t* __restrict__ words, int B, int32_t* __restrict__ order, int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first,
              int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg, const RnTileFwd pack, unsigned long long* __restrict__ zero1) {
    if (blockIdx.x == 0) {
        if (zero1 && threadIdx.x == 0) *zero1 = 0ull;      // the step's pair counter (its loss stage adds into it: dcnmix.hip)
        group_small_body<RAW>(words, nullptr, B, order, seg_id, seg_first, super_id, n_seg);
        return;
    }
    tl_pack_range(pack, (int64_t)(blockIdx.x - 1) * GS_T + threadIdx.x, (int64_t)(gridDim.x - 1) * GS_T);
}

// ---- the cooperative launch (device code: group_mid.hpp) ------------------------------------------------------------------------------
template <int TILE, int RAW = 0>
__global__ void __launch_bounds__(256)
k_group_mid(const uint32_t* __restrict__ words, uint8_t* __restrict__ solo, int64_t B, int n_words, int n_words_first,
            GroupMidCtl* __restrict__ ctl, int32_t* __restrict__ idx0, int32_t* __restrict__ idx1, uint32_t* __restrict__ key0,
            uint32_t* __restrict__ key1, unsigned* __restrict__ blockhist, int* __restrict__ headcnt, int32_t* __restrict__ order,
            int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first, int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg, int inf_equal) {
    group_mid_body<TILE, RAW>(words, solo, B, n_words, n_words_first, ctl, idx0, idx1, key0, key1, blockhist, headcnt, order, seg_id, seg_first, super_id,
                              n_seg, (int)gridDim.x, (int)blockIdx.x, inf_equal);
}
// Front kernel of recnow_dcn_mix_step above GS_MAXB rows: the first G workgroups (dispatched first: co-resident as before) group the batch, the others
// write the weight packs of the row-block kernels (see k_front_small).
template <int RAW>
__global__ void __launch_bounds__(256)
k_front_mid(const uint32_t* __restrict__ words, uint8_t* __restrict__ solo, int64_t B, GroupMidCtl* __restrict__ ctl, int32_t* __restrict__ idx0,
            int32_t* __restrict__ idx1, uint32_t* __restrict__ key0, uint32_t* __restrict__ key1, unsigned* __restrict__ blockhist,
            int* __restrict__ headcnt, int32_t* __restrict__ order, int32_t* __restrict__ seg_id, int32_t* __restrict__ seg_first,
            int32_t* __restrict__ super_id, int32_t* __restrict__ n_seg, const int G, const RnTileFwd pack, unsigned long long* __restrict__ zero1) {
    if (zero1 && blockIdx.x == 0 && threadIdx.x == 0) *zero1 = 0ull;
    if ((int)blockIdx.x < G) {
        group_mid_body<RN_TILE, RAW>(words, solo, B, 1, 1, ctl, idx0, idx1, key0, key1, blockhist, headcnt, order, seg_id, seg_first, super_id, n_seg, G,
                                     (int)blockIdx.x, 0);
        return;
    }
    tl_pack_range(pack, (int64_t)((int)blockIdx.x - G) * 256 + threadIdx.x, (int64_t)((int)gridDim.x - G) * 256);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// Largest grid of k_group_mid whose workgroups are all resident at once on the CURRENT device: occupancy x compute units, queried
// once per device (a CU mask, a smaller partition (CPX) or a register-hungrier build all show up here).  The hand-rolled grid
// barrier is only correct below it; anything larger takes the multi-launch chain.
static int gm_max_coresident() {
    static int cached[64];
    static bool have[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!have[dev]) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_group_mid<2048>, 256, 0) != hipSuccess) per_cu = 0;
        // ... and of the front kernels, which carry the same barrier among their first G workgroups (their pack workgroups never wait: they end
        // without looking at the barrier, so residency of the G grouping workgroups is all the barrier needs)
        int f1 = 0, f2 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&f1, (const void*)k_front_mid<1>, 256, 0) != hipSuccess) f1 = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&f2, (const void*)k_front_mid<2>, 256, 0) != hipSuccess) f2 = 0;
        if (f1 < 1 || f2 < 1) per_cu = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        // one workgroup per CU is what the route counts on (the step's GEMMs hold the other slots)
        cached[dev] = per_cu > 0 ? cus : 0;
        have[dev] = true;
    }
    return cached[dev];
}

RnGroupWs rn_group_ws(void* ws, int64_t B, int n_words) {
    RnGroupWs w;
    RnCarver c(ws, 0);
    const int nblk = rn_cdiv(B > 0 ? B : 1, RN_TILE);
    w.plan = c.take<SortPlan>(1);
    w.mix = c.take<unsigned>((size_t)n_words * 4 * 256);
    w.idx0 = c.take<int32_t>(B + 1);
    w.idx1 = c.take<int32_t>(B + 1);
    w.key0 = c.take<uint32_t>(B + 1);
    w.key1 = c.take<uint32_t>(B + 1);
    w.blockhist = c.take<unsigned>((size_t)256 * (nblk > GM_MAXG ? nblk : GM_MAXG));      // (the cooperative route runs up to GM_MAXG tiles)
    w.head = c.take<int32_t>(B + 1);
    w.shead = c.take<int32_t>(B + 1);
    w.seg_incl = c.take<int32_t>(B + 1);
    w.super_incl = c.take<int32_t>(B + 1);
    w.scan_bytes = rn_scan_ws_bytes(B);
    w.scan = c.take<char>(w.scan_bytes);
    w.ctl = c.take<GroupMidCtl>(1);
    w.headcnt = c.take<int>((size_t)2 * GM_MAXG);
    w.total = c.off;
    return w;
}
extern "C" size_t recnow_group_segments_workspace_bytes(int64_t B, int n_words) {
    if (B < 0 || n_words < 1 || n_words > RN_MAX_WORDS) return 0;
    return rn_group_ws(nullptr, B, n_words).total;
}

// The one-workgroup kernels need gs_lds_bytes() of dynamic LDS: their limit is raised on every device they run on (not a stream operation: a first call
// outside a stream capture does it, every later call and every capture finds it done).
static int gs_raise_lds_limit() {
    const void* const kernels[5] = {(const void*)k_group_small<0>, (const void*)k_group_small<1>, (const void*)k_group_small<2>,
                                    (const void*)k_front_small<1>, (const void*)k_front_small<2>};
    for (const void* k : kernels) RN_HIP(rn_lds_grant(k, gs_lds_bytes()));
    return RECNOW_OK;
}

// batches from this size on run 4096 keys per workgroup: half the workgroups at every grid barrier and in every histogram row (phase stamps, tools/gs_trace.py, one box:
// 262 144 rows 79.0 -> 74.6 us, 65 536 rows 44.5 -> 52.8 us -- the phases of a workgroup take longer than what the cheaper barriers save there)
#define GM_TILE4096_FROM 262144ll
typedef void (*GmKernel)(const uint32_t*, uint8_t*, int64_t, int, int, GroupMidCtl*, int32_t*, int32_t*, uint32_t*, uint32_t*, unsigned*, int*, int32_t*, int32_t*,
                         int32_t*, int32_t*, int32_t*, int);
static const GmKernel gm_kernels[2][3] = {{k_group_mid<2048, 0>, k_group_mid<2048, 1>, k_group_mid<2048, 2>},       // [4096 keys per workgroup][raw]
                                          {k_group_mid<4096, 0>, k_group_mid<4096, 1>, k_group_mid<4096, 2>}};

// The cooperative route (one launch, all workgroups co-resident: <= one per CU) over the workspace of recnow_group_segments; RECNOW_EUNSUPPORTED when the
// batch does not fit it (the caller then takes the multi-launch chain).  raw = 0: canonical key words + solo flags; raw = 1 / 2: `words` is a float32 / int32
// id tensor (n_words = 1), the kernel forms keys and solo flags itself (`solo` is written, not read, by the caller's side).  front (raw only): the front
// kernels also write the weight packs and clear one 64-bit word for the caller and say so; the other forms leave front->zeroed / packed alone.  inf_equal
// (raw = 1 without packs): the flags the kernel forms mark NaN ids only (RECNOW_KEY_INF_EQUAL); it travels as a kernel argument, not as another instantiation.
static int rn_group_coop(int raw, int inf_equal, const uint32_t* words, uint8_t* solo, int64_t B, int n_words, int n_words_first, int32_t* order, int32_t* seg_id,
                         int32_t* seg_first, int32_t* super_id, int32_t* n_seg, void* ws, hipStream_t st, RnGroupFront* front = nullptr) {
    // Keys per workgroup: 2048, or 4096 (RECNOW_GROUP_TILE = 2048 / 4096 forces one).  Smaller tiles (more workgroups, less per-key work between two grid
    // barriers) were tried and retired: B = 65 536 on 128 workgroups of 512 keys 114 us against 89 us on 32 of 2048, B = 262 144 on 256 of 1024 keys 207
    // against 147 us per fused loss -- every digit pass makes each thread scan one histogram row over ALL workgroups, and a barrier costs more the more arrive.
    const int maxg = gm_max_coresident() < GM_MAXG ? gm_max_coresident() : GM_MAXG;
    static const int tile_env = rn_env_int("RECNOW_GROUP_TILE", 0);
    const int tile = (tile_env == 4096 || (tile_env == 0 && B >= GM_TILE4096_FROM)) ? 4096 : RN_TILE;
    if (rn_cdiv(B, tile) > maxg) return RECNOW_EUNSUPPORTED;
    const RnGroupWs w = rn_group_ws(ws, B, n_words);
    RN_HIP(hipMemsetAsync(w.ctl, 0, sizeof(GroupMidCtl), st));
    static const bool dbg_timeout = rn_env_int("RECNOW_DEBUG_GROUP_TIMEOUT", 0) == 1;
    if (dbg_timeout) RN_HIP(hipMemsetAsync(&w.ctl->err, 1, sizeof(int), st));      // tests: every barrier reports the time-out at once
    const int g = rn_cdiv(B, tile);
    if (raw && front && front->pack && tile == RN_TILE) {      // + the weight packs on workgroups behind the grouping's
        hipLaunchKernelGGL(raw == 1 ? k_front_mid<1> : k_front_mid<2>, g + RN_FRONT_PACK_WGS, 256, 0, st, words, solo, B, w.ctl, w.idx0, w.idx1, w.key0, w.key1,
                           w.blockhist, w.headcnt, order, seg_id, seg_first, super_id, n_seg, g, *front->pack, front->zero1);
        front->zeroed = front->zero1 ? 1 : 0;
        front->packed = 1;
    } else {
        hipLaunchKernelGGL(gm_kernels[tile == 4096][raw], g, 256, 0, st, words, solo, B, n_words, n_words_first, w.ctl, w.idx0, w.idx1, w.key0, w.key1, w.blockhist,
                           w.headcnt, order, seg_id, seg_first, super_id, n_seg, inf_equal);
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

int rn_group_words(const uint32_t* words, const uint8_t* solo, int64_t B, int n_words, int n_words_first, int32_t* order, int32_t* seg_id,
                   int32_t* seg_first, int32_t* super_id, int32_t* n_seg, void* ws, hipStream_t st) {
    if (B <= GS_MAXB && n_words == 1) {           // small batch, one key word: everything in one workgroup
        int rc = gs_raise_lds_limit();
        if (rc) return rc;
        hipLaunchKernelGGL(k_group_small<0>, 1, GS_T, gs_lds_bytes(), st, words, solo, (int)B, order, seg_id, seg_first, super_id, n_seg);
        RN_LAUNCH_CHECK();
        return RECNOW_OK;
    }
    return rn_group_coop(0, 0, words, const_cast<uint8_t*>(solo), B, n_words, n_words_first, order, seg_id, seg_first, super_id, n_seg, ws, st);
}

int rn_group_rows(const void* groups, int key_dtype, int64_t B, const RnGroupBufs& b, void* grp_ws, size_t grp_ws_bytes, hipStream_t st, RnGroupFront* front) {
    const int dt = key_dtype & ~RECNOW_KEY_INF_EQUAL, inf_equal = dt != key_dtype ? 1 : 0;
    const bool raw = dt == RECNOW_KEY_F32 || dt == RECNOW_KEY_I32;      // ONE id tensor whose keys and solo flags the one-launch kernels form themselves
    const RnTileFwd* pack = front ? front->pack : nullptr;
    if (front) front->zeroed = front->packed = 0;
    int rc = RECNOW_EUNSUPPORTED;
    if (raw && front && !inf_equal && B <= GS_MAXB) {      // the step's shard sizes: one workgroup
        if ((rc = gs_raise_lds_limit())) return rc;
        if (pack) {      // + one pack workgroup per remaining compute unit (every workgroup of this kernel holds 112 KB of LDS)
            hipLaunchKernelGGL(dt == RECNOW_KEY_F32 ? k_front_small<1> : k_front_small<2>, 1 + RN_FRONT_PACK_WGS, GS_T, gs_lds_bytes(), st, (const uint32_t*)groups,
                               (int)B, b.order, b.seg_id, b.seg_first, b.super_id, b.n_seg, *pack, front->zero1);
            front->zeroed = front->zero1 ? 1 : 0;
            front->packed = 1;
        } else {
            hipLaunchKernelGGL(dt == RECNOW_KEY_F32 ? k_group_small<1> : k_group_small<2>, 1, GS_T, gs_lds_bytes(), st, (const uint32_t*)groups,
                               (const uint8_t*)nullptr, (int)B, b.order, b.seg_id, b.seg_first, b.super_id, b.n_seg);
        }
        RN_LAUNCH_CHECK();
        return RECNOW_OK;
    }
    if (raw && B > GS_MAXB && b.solo && grp_ws && !(inf_equal && pack)) {      // no fill of `solo`, no key kernel (the front kernels know only the pairwise rule)
        if (grp_ws_bytes < recnow_group_segments_workspace_bytes(B, 1)) return RECNOW_EWORKSPACE;
        rc = rn_group_coop(dt == RECNOW_KEY_F32 ? 1 : 2, inf_equal, (const uint32_t*)groups, b.solo, B, 1, 1, b.order, b.seg_id, b.seg_first, b.super_id, b.n_seg, grp_ws,
                           st, front);
    }
    if (rc != RECNOW_EUNSUPPORTED) return rc;      // (a batch beyond the co-resident grid goes on)
    RN_HIP(hipMemsetAsync(b.solo, 0, (size_t)B, st));
    if ((rc = recnow_group_keys(groups, key_dtype, B, b.words, b.solo, (void*)st))) return rc;
    return recnow_group_segments(b.words, b.solo, B, b.n_words, b.n_words, b.order, b.seg_id, b.seg_first, b.super_id, b.n_seg, grp_ws, grp_ws_bytes, (void*)st);
}
