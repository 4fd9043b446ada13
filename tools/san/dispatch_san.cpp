// TEST INFRASTRUCTURE: the host-only dispatch logic of the MFMA GEMM (rec_now_amd/csrc/gemm_dispatch.hpp: tile family, 64-row small-M rule, K split, slab
// workspace and the whole launch plan, rn_gemm_plan) swept over descriptors on the CPU under -fsanitize=address,undefined (sanitizer
// build; `make -C tools/san`, run by tests/test_oracle_golden.py).  Checked for every shape: the K slices tile [0, K) exactly (k-chunks are multiples of
// 32, the last slice is not empty), the grid's z extent fits a launch, the slab size never overflows size_t arithmetic for the sizes the layers use, the
// 64-row choice is only made for row counts it divides, and the split of the hot-path products is what DESIGN.md says it is.  Checked for every
// descriptor of the plan sweep (shapes x layouts x operand modes x side product / rank-R update / second output x workspace x ready planes x slot
// target x precision x pointer alignment; the pointers are synthetic addresses, never dereferenced): the plan refuses with one of the documented
// codes or names a kernel that the instantiation lists hold, the tag is the planned family's, lean kernels and paired loads get aligned operands only,
// and slabs and planes lie inside what the workspace query reserves.
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include "../../rec_now_amd/csrc/gemm_dispatch.hpp"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 50) printf("FAILED %s:%d: %s  (M %d N %d K %d batch %d sp_r %d)\n", __FILE__, __LINE__, #c, d.M, d.N, d.K, d.batch, d.sp_r); ++fails; } } while (0)

static void one(int M, int N, int K, int batch, int sp_r, int c2_mode, const RnDispatchEnv& env, int* out_bm = nullptr, int* out_s = nullptr, int slots = 512) {
    recnow_gemm_desc d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.N = N; d.K = K; d.batch = batch; d.sp_r = sp_r; d.c2_mode = c2_mode;
    const GemmCfg c = pick_cfg(&d, env);
    CHECK(c.BM == 64 || c.BM == 128 || c.BM == 256);
    CHECK(c.BN == 32 || c.BN == 64 || c.BN == 128 || c.BN == 160);
    if (c.BM == 64) CHECK(M % 64 == 0 && N == 128 && sp_r >= 1 && sp_r <= 2 && env.precision == 0 && batch == 1);
    int s = 0, kc = 0;
    pick_split(&d, c, &s, &kc, slots);
    CHECK(s >= 1 && kc >= 32 && kc % 32 == 0);
    CHECK(rnd_slab_bytes(&d, s, 256) <= rnd_slab_bytes_any(&d, c, 256));      // what the workspace query reserves holds either slot target
    CHECK((long long)(s - 1) * kc < K);                    // the last slice starts inside K
    CHECK((long long)s * kc >= K);                         // the slices cover K
    if (c2_mode) CHECK(s == 1);                            // fused second outputs need the whole K in one workgroup
    CHECK((long long)batch * s <= 65535 || K > (1 << 24)); // gridDim.z
    const size_t slab = rnd_slab_bytes(&d, s, 256);
    CHECK((s > 1) == (slab > 0));
    if (s > 1) CHECK(slab >= (size_t)s * batch * M * N * sizeof(float) && slab % 256 == 0);
    if (out_bm) *out_bm = c.BM;
    if (out_s) *out_s = s;
}

// ---- the plan sweep ----------------------------------------------------------------------------------------------------------------------
// synthetic device addresses: region i starts at (i + 1) << 32, `skew` bytes further on
static const float* addr(int region, int skew) { return (const float*)(uintptr_t)(((uint64_t)(region + 1) << 32) + (uint64_t)skew); }

enum Feature { F_NONE, F_SP2, F_SP4, F_EU2, F_C2_1, F_C2_2, F_AS_OUT, F_COUNT };
static recnow_gemm_desc make_desc(int M, int N, int K, int batch, int ta, int tb, int a_mode, int b_mode, int feat, int skew) {
    recnow_gemm_desc d;
    memset(&d, 0, sizeof(d));
    d.M = M; d.N = N; d.K = K; d.batch = batch;
    d.a_trans = ta; d.b_trans = tb; d.a_mode = a_mode; d.b_mode = b_mode;
    d.lda = ta ? M : K; d.ldb = tb ? K : N; d.ldc = N; d.lde = N;
    d.a_batch_stride = (int64_t)M * K; d.b_batch_stride = (int64_t)K * N; d.c_batch_stride = (int64_t)M * N;
    d.A = addr(0, skew); d.B = addr(1, skew); d.C = (float*)addr(2, skew);
    if (a_mode) d.A2 = addr(3, skew);
    if (b_mode) d.B2 = addr(4, skew);
    if (a_mode == RECNOW_OPMODE_OUTER) { d.a_hq = 4; d.a_ld2 = 64; }
    if (b_mode == RECNOW_OPMODE_OUTER) { d.b_hq = 4; d.b_ld2 = 64; }
    if (feat == F_SP2 || feat == F_SP4 || feat == F_AS_OUT) {
        d.sp_r = feat == F_SP4 ? 4 : 2;
        d.sp_bx = addr(5, 0); d.sp_cx = (float*)addr(6, 0); d.sp_bx_ks = d.sp_r; d.sp_bx_rs = 1; d.sp_cx_ms = d.sp_r; d.sp_cx_rs = 1;
    }
    if (feat == F_AS_OUT) { d.as_in = addr(7, skew); d.as_out = (float*)addr(8, skew); }
    if (feat == F_EU2) { d.eu_r = 2; d.eu_p = addr(5, 0); d.eu_q = addr(6, 0); d.eu_pms = 2; d.eu_qrs = N; d.eu_qns = 1; }
    if (feat == F_C2_1 || feat == F_C2_2) {
        d.c2_mode = feat == F_C2_1 ? 1 : 2;
        d.C2 = (float*)addr(7, skew); d.ldc2 = N; d.E2 = addr(8, skew); d.lde2 = N;
    }
    return d;
}

static long long plans = 0, planned[6] = {0, 0, 0, 0, 0, 0};
static void check_plan(const recnow_gemm_desc& d, const RnGemmOpts& o, bool has_ws, size_t ws_bytes, const RnDispatchEnv& env, RnGemmPlan* out = nullptr) {
    RnGemmPlan p;
    const int rc = rn_gemm_plan(&d, o, has_ws, ws_bytes, env, &p);
    ++plans;
    if (out) *out = p;
    CHECK(rc == RECNOW_OK || rc == RECNOW_EINVAL || rc == RECNOW_EWORKSPACE || rc == RECNOW_EUNSUPPORTED);
    if (rc != RECNOW_OK) return;
    CHECK(p.family >= RN_GF_NONE && p.family <= RN_GF_S3);
    ++planned[p.family];
    if (p.family == RN_GF_NONE) { CHECK(d.M == 0 || d.N == 0 || d.batch == 0); return; }
    const size_t query = rnd_ws_bytes(&d, env);
    const bool a_skew = ((uintptr_t)d.A & 15) != 0;
    // the K slices tile [0, K) as before; the slabs fit what the query reserves and what the caller handed over
    CHECK(p.splitk >= 1 && p.kchunk >= 32 && p.kchunk % 32 == 0 && (long long)(p.splitk - 1) * p.kchunk < d.K && (long long)p.splitk * p.kchunk >= d.K);
    CHECK((p.splitk > 1) == (p.slab_bytes > 0) && p.slab_bytes <= query);
    if (p.splitk > 1) CHECK(has_ws && p.slab_bytes <= ws_bytes && p.reduce_blocks >= 1 && p.reduce_variant >= 0 && p.reduce_variant <= 2 && (p.reduce_variant == 0 || d.N % 4 == 0));
    CHECK(p.grid_x >= 1 && p.grid_y >= 1 && p.grid_z == d.batch * p.splitk && p.grid_z <= 65535);
    CHECK(p.tail_pairs >= 1 && p.tail_pairs <= 8 && p.xcd_remap >= 0 && p.xcd_remap <= 2);
    // planes the launch splits first lie in the workspace, behind the slabs, inside the query
    CHECK(p.planes >= 0 && p.planes <= 2 && (p.planes == 2) <= (o.planes_ready != nullptr));
    if (p.planes == 1) CHECK(has_ws && p.planes_off == p.slab_bytes && p.planes_off + rnd_planes_bytes(d.K, d.N) <= ws_bytes && p.planes_off + rnd_planes_bytes(d.K, d.N) <= query);
    if (env.precision == 0) CHECK(p.family == RN_GF_GEMM || p.family == RN_GF_SHORTK);
    switch (p.family) {
        case RN_GF_GEMM: {
            CHECK(rnd_has_kgemm(p));      // a combination the lists hold
            const int fam = (p.BM == 256 && p.BN == 32) ? RN_TAG_GEMM_256x32 : (p.BM == 256) ? RN_TAG_GEMM_256x64 : (p.BN == 160) ? RN_TAG_GEMM_128x160
                          : (p.BM == 64) ? RN_TAG_GEMM_64x128 : RN_TAG_GEMM_128x128;
            CHECK(p.tag == (p.xf == 25 ? RN_TAG_GEMM_MIDF : fam));
            CHECK(p.grid_x == rnd_cdiv(d.M, p.BM) && p.grid_y == rnd_cdiv(d.N, p.BN) && p.planes == 0);
            if (!p.edge) CHECK(!a_skew && d.M % p.BM == 0 && d.N % p.BN == 0 && d.K % p.BK == 0 && p.kchunk % p.BK == 0 && p.a2k == d.a_mode && p.b2k == d.b_mode);
            if (p.edge) CHECK(d.sp_r == 0 && d.eu_r == 0 && !d.as_out && !d.c2_mode);
            CHECK(((p.xf & 1) != 0) == (d.sp_r > 0) && ((p.xf & 2) != 0) == (d.eu_r > 0) && ((p.xf & 4) != 0) == (d.as_out != nullptr));
            if (p.xf & 8) CHECK(d.sp_r <= 2 && p.BK == 32);
            if (p.xf & 32) CHECK(env.staging == 1);
            break;
        }
        case RN_GF_SHORTK:
        case RN_GF_SHORTK_SPLIT:
            CHECK(p.tag == RN_TAG_GEMM_SHORTK && !a_skew && p.splitk == 1 && d.K % 16 == 0 && d.K <= 512 && d.M % 128 == 0 && d.N % 128 == 0 && !d.a_trans);
            if (p.family == RN_GF_SHORTK) CHECK(rnd_has_shortk(d.K, p.b_kc != 0, p.ep, p.c2_mode) && p.planes == 0);
            else CHECK(rnd_has_shortk_split(p.b_kc != 0, p.ep, p.c2_mode) && d.K == 144 && p.planes >= 1 && p.planes_off == 0 && env.split_shortk != 0);
            break;
        default:
            CHECK(p.tag == RN_TAG_GEMM_SPLIT && !a_skew && env.split_longk != 0 && d.N == 128 && p.grid_y == 1 && d.sp_r > 0 && d.K % 32 == 0 && d.M % 128 == 0);
            CHECK(p.a2k == d.a_mode && (p.a2k == 0 || p.a2k == RECNOW_OPMODE_MUL));
            if (p.family == RN_GF_SPLIT) CHECK(rnd_has_split(p.a_kc != 0, p.a2k, p.bp) && (p.bp == 2) == (p.planes == 1) && p.planes != 2 && !p.pair);
            else CHECK(p.planes >= 1 && env.split_lean != 0 && d.sp_r <= 2 && p.kchunk <= RND_S3_MAXK && d.K % p.kchunk == 0 && (p.a_kc || env.split_lean == 2));
            if (p.pair) CHECK(p.a_kc && env.s3_pair != 0 && ((uintptr_t)d.A & 127) == 0 && (!d.a_mode || ((uintptr_t)d.A2 & 127) == 0) && p.kchunk % 64 == 0);
    }
}

static void sweep_plan(const RnDispatchEnv& env, bool all_axes) {
    const int Ms[] = {1, 7, 64, 100, 128, 192, 256, 1000, 1024, 4096, 8192, 16384, 32768, 65536, 262144, 2097152};
    const int Ns[] = {1, 8, 32, 33, 64, 65, 128, 130, 144, 160, 161, 256, 1024, 4096, 8192};
    const int Ks[] = {1, 31, 32, 33, 130, 144, 256, 512, 1000, 1024, 4096, 8192, 16384, 32768, 65536, 262144};
    const int modes[][2] = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {0, 2}, {0, 3}, {0, 1}};
    const void* const ready = addr(9, 0);
    for (int M : Ms)
        for (int N : Ns)
            for (int K : Ks)
                for (int batch : {1, 3})
                    for (int feat = 0; feat < F_COUNT; ++feat) {
                        if (feat != F_NONE && batch != 1) continue;
                        for (int lay = 0; lay < 4; ++lay)
                            for (const auto& m : modes)
                                for (int skew : {0, 4, 128}) {       // aligned (to 256 bytes and more), off by one float, on a 128-byte line only
                                    if (!all_axes && skew == 128) continue;
                                    const recnow_gemm_desc d = make_desc(M, N, K, batch, lay & 1, lay >> 1, m[0], m[1], feat, skew);
                                    const size_t q = rnd_ws_bytes(&d, env);
                                    for (int slots : {512, 256})
                                        for (int rdy = 0; rdy < 2; ++rdy) {
                                            if (!all_axes && (rdy || slots == 256)) continue;
                                            const RnGemmOpts o{slots, rdy ? ready : nullptr};
                                            check_plan(d, o, true, q, env);
                                            if (all_axes && skew == 0) check_plan(d, o, false, 0, env);      // no workspace
                                        }
                                }
                    }
}

static bool is_kgemm(const RnGemmPlan& p, int bm, int bn, int bk, int a_kc, int b_kc, int a2k, int b2k, int xf) {
    return p.family == RN_GF_GEMM && p.BM == bm && p.BN == bn && p.BK == bk && p.a_kc == a_kc && p.b_kc == b_kc && !p.edge && p.a2k == a2k && p.b2k == b2k && p.xf == xf;
}

int main(void) {
    const RnDispatchEnv envs[] = {{256, -1, 0}, {0, -1, 0}, {64, 0, 0}, {256, 1, 0}, {256, -1, 1}};
    const int Ms[] = {1, 7, 64, 100, 128, 192, 256, 1000, 1024, 4096, 8192, 16384, 32768, 65536, 262144, 2097152};
    const int Ns[] = {1, 8, 32, 33, 64, 65, 128, 130, 144, 160, 161, 256, 1024, 4096, 8192};
    const int Ks[] = {1, 31, 32, 33, 130, 144, 256, 512, 1000, 1024, 4096, 8192, 16384, 32768, 65536, 262144};
    for (const RnDispatchEnv& env : envs)
        for (int M : Ms)
            for (int N : Ns)
                for (int K : Ks)
                    for (int batch : {1, 3})
                        for (int sp_r : {0, 2, 4})
                            for (int c2 : {0, 1}) {
                                if (sp_r && batch != 1) continue;
                                one(M, N, K, batch, sp_r, c2, env);
                                one(M, N, K, batch, sp_r, c2, env, nullptr, nullptr, 256);      // products launched as concurrent pairs (dcnmix_bwd_tile)
                            }
    // the whole plan: both precisions at the default switches over every axis; the switches' other settings over shapes, layouts and operand kinds
    RnDispatchEnv def = {256, -1, 0}, spl = {256, -1, 1};
    sweep_plan(def, true);
    sweep_plan(spl, true);
    for (int v = 0; v < 6; ++v) {
        RnDispatchEnv e = v == 0 ? def : spl;
        if (v == 0) e.staging = 1;
        if (v == 1) e.split_longk = 0;
        if (v == 2) e.split_shortk = 0;
        if (v == 3) e.split_lean = 0;
        if (v == 4) e.split_lean = 2;
        if (v == 5) e.s3_pair = 0;
        sweep_plan(e, false);
    }
    for (int f = RN_GF_GEMM; f <= RN_GF_S3; ++f)
        if (!planned[f]) { printf("FAILED: the sweep planned no launch of family %d\n", f); ++fails; }
    // the hot-path products, as DESIGN.md 5g / 5h state them (default switches), with the kernel each is planned on
    int bm = 0, s = 0;
    recnow_gemm_desc d;
    RnGemmPlan p;
    const RnGemmOpts o512, o256{256, nullptr};
    auto hot = [&](int M, int N, int K, int ta, int tb, int feat, const RnGemmOpts& o) {
        d = make_desc(M, N, K, 1, ta, tb, 0, 0, feat, 0);
        one(M, N, K, 1, d.sp_r, 0, def, &bm, &s, o.slots ? o.slots : 512);
        check_plan(d, o, true, rnd_ws_bytes(&d, def), def, &p);
        CHECK(p.splitk == s && p.BM == bm);
    };
    hot(65536, 128, 1024, 0, 0, F_SP2, o512); CHECK(bm == 128 && s == 1 && is_kgemm(p, 128, 128, 32, 1, 0, 0, 0, 9));      // GEMM1 at the metric's batch: 512 tiles, no split
    hot(1024, 128, 65536, 1, 0, F_SP2, o512); CHECK(bm == 128 && s == 64 && is_kgemm(p, 128, 128, 32, 0, 0, 0, 0, 9) && p.xcd_remap == 1);      // dU / dW: 8 tiles x 64 slabs
    hot(8192, 128, 1024, 0, 0, F_SP2, o512); CHECK(bm == 64 && s == 4 && is_kgemm(p, 64, 128, 32, 1, 0, 0, 0, 9));        // the 8-GPU shard: 128 tiles x 4
    hot(1024, 128, 8192, 1, 0, F_SP2, o512); CHECK(bm == 64 && s == 32 && is_kgemm(p, 64, 128, 32, 0, 0, 0, 0, 9));
    hot(1024, 128, 8192, 1, 0, F_SP2, o256); CHECK(bm == 64 && s == 16 && is_kgemm(p, 64, 128, 32, 0, 0, 0, 0, 9));       // ... as one of a concurrent pair: 16 tiles x 16 slices
    hot(16384, 128, 1024, 0, 0, F_SP2, o512); CHECK(bm == 64 && s == 2 && is_kgemm(p, 64, 128, 32, 1, 0, 0, 0, 9));
    hot(32768, 128, 1024, 0, 0, F_SP2, o512); CHECK(bm == 64 && s == 1 && is_kgemm(p, 64, 128, 32, 1, 0, 0, 0, 9));
    hot(32768, 4096, 512, 0, 0, F_NONE, o512); CHECK(bm == 128 && s == 1 && is_kgemm(p, 128, 128, 32, 1, 0, 0, 0, 0) && p.xcd_remap == 2);      // PLE expert layer
    hot(512, 4096, 32768, 1, 0, F_NONE, o512); CHECK(bm == 128 && s == 4 && is_kgemm(p, 128, 128, 32, 0, 0, 0, 0, 0) && p.reduce_variant == 1);      // its weight gradient: slabs of 8192 terms (accuracy)
    // split precision: GEMM1 on the caller's planes runs k_gemm_s3 with paired loads, the K = B products k_gemm_split
    d = make_desc(65536, 128, 1024, 1, 0, 0, 0, 0, F_SP2, 0);
    check_plan(d, RnGemmOpts{0, addr(9, 0)}, true, rnd_ws_bytes(&d, spl), spl, &p);
    CHECK(p.family == RN_GF_S3 && p.planes == 2 && p.pair && p.a_kc && p.tag == RN_TAG_GEMM_SPLIT);
    d = make_desc(1024, 128, 65536, 1, 1, 0, 0, 0, F_SP2, 0);
    check_plan(d, o512, true, rnd_ws_bytes(&d, spl), spl, &p);
    CHECK(p.family == RN_GF_SPLIT && p.bp == 0 && !p.a_kc && p.splitk == 64);
    // a side product over two column tiles has no split kernel: the fp32 kernel runs and the tag says so
    d = make_desc(128, 256, 512, 1, 0, 0, 0, 0, F_SP2, 0);
    check_plan(d, o512, true, rnd_ws_bytes(&d, spl), spl, &p);
    CHECK(is_kgemm(p, 128, 128, 32, 1, 0, 0, 0, 9) && p.tag == RN_TAG_GEMM_128x128);
    if (fails) { printf("dispatch sanitizer driver: %d check(s) failed\n", fails); return 1; }
    printf("dispatch sanitizer driver ok (%lld plans: %lld k_gemm, %lld short-K, %lld short-K split, %lld k_gemm_split, %lld k_gemm_s3)\n", plans,
           planned[1], planned[2], planned[3], planned[4], planned[5]);
    return 0;
}
