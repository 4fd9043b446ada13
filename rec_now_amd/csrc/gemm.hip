// Exact-fp32 MFMA GEMM for gfx950: C = epilogue(opA(A) x opB(B)), batched, optional split-K.
//
// Why this shape: the reference's contractions (multi_dense_layer.py:90, dcn_mix_layer.py:135-141, MMoE/PLE experts)
// must match TF's fp32 matmul to 1e-5 relative, so bf16 MFMA is out; gfx950's v_mfma_f32_32x32x2_f32 is an exact fp32
// fma chain at 64 FLOP/clk/SIMD (157 TFLOP/s).  At that rate a 128x128x32 block tile needs 16 KB + 16 KB of LDS per
// 4096 MFMA-cycles per wave, so LDS bandwidth and even ds_read_b32 fragment loads are far from binding; what matters
// is (1) fragment reads that are bank-conflict-free, (2) global loads of the next k-tile in flight under the MFMAs of
// the current one (register-staged double buffering, one barrier per k-tile), (3) enough workgroups (split-K for the
// K = batch-rows weight-gradient GEMMs, reduced deterministically from slabs -- no float atomics).
//
// LDS images are k-major: As[k][m], Bs[k][n].  A wave64 MFMA 32x32x2 fragment read is then 32 consecutive floats for
// lanes 0-31 (k) and 32 consecutive floats for lanes 32-63 (k+1): conflict-free ds_read_b32 with no padding tricks.
// An operand that is k-contiguous in memory ([m][k]) is loaded as float4 along k (coalesced 128-B rows) and transposed
// on the LDS write; its row stride is ROWS+1 floats so those 4-B writes are conflict-free too.
#include <atomic>
#include "gemm_kernel.hpp"
#include "prof.hpp"

// sum the split-K slabs in slice order (deterministic) and apply the epilogue.  float4 per thread along N (the slabs
// are [M][N] with N % 4 == 0 whenever VEC), four slabs in flight per thread.
// Deterministic slab reduction of the split-K products.  QUAD: four adjacent lanes share one float4 of the output, each sums a
// quarter of the slabs (a contiguous range, in order), and the four partial sums are combined as (q0 + q1) + (q2 + q3): four times
// the threads and loads in flight -- an output of 1024 x 132 floats is 33 792 float4, i.e. 132 workgroups of threads that each walk
// 64 slabs with four loads in flight (10.5 us for 35 MB that the product has just left in the memory-side cache).
template <bool VEC, bool QUAD>
__device__ __forceinline__ void splitk_reduce_body(const GemmK& p, const int bid, const int nblk) {
    constexpr int W = VEC ? 4 : 1;
    constexpr int NQ = QUAD ? 4 : 1;
    const int64_t MN = (int64_t)p.M * p.npart;          // one slab
    const int64_t total = MN * p.batch / W;
    const int q = QUAD ? (threadIdx.x & 3) : 0;
    const int per = (p.splitk + NQ - 1) / NQ, k_lo = q * per, k_hi = min(p.splitk, k_lo + per);
    // QUAD: every lane of a quad runs the loop for the quad's element (whole quads are in or out: total is rounded up by the caller's grid)
    for (int64_t i = ((int64_t)bid * 256 + threadIdx.x) / NQ; i < total; i += (int64_t)nblk * 256 / NQ) {
        const int64_t e0 = i * W;
        const int b = (int)(e0 / MN);
        const int64_t mn = e0 % MN;
        const int row = (int)(mn / p.npart), col = (int)(mn % p.npart);
        const float* P = p.partial + ((int64_t)b * p.splitk) * MN + mn;
        // the slabs are summed in fp64 (the kernel is bound by reading them; 64 double adds per output are free): the K = B weight
        // gradients then carry only the fp32 accumulation INSIDE a slab (K / splitk deep), not another 64-term fp32 sum on top --
        // at K = 32 768 the full-size PLE parity test sat at 1.0e-5 of its bound with fp32 slab sums
        double s[W];
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] = 0.0;
        int k = k_lo;
        if (VEC) {
            // eight slabs in flight per lane (the loop is bound by the latency of its loads: 4 in flight read 2.7 TB/s); the sums keep
            // the sequential order
            for (; k + 8 <= k_hi; k += 8) {
                float4 a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const float4*>(P + (int64_t)(k + u) * MN);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    s[0] += a[u].x;
                    s[1 % W] += a[u].y;
                    s[2 % W] += a[u].z;
                    s[3 % W] += a[u].w;
                }
            }
            for (; k + 4 <= k_hi; k += 4) {
                const float4 a0 = *reinterpret_cast<const float4*>(P + (int64_t)(k + 0) * MN);
                const float4 a1 = *reinterpret_cast<const float4*>(P + (int64_t)(k + 1) * MN);
                const float4 a2 = *reinterpret_cast<const float4*>(P + (int64_t)(k + 2) * MN);
                const float4 a3 = *reinterpret_cast<const float4*>(P + (int64_t)(k + 3) * MN);
                s[0] = (((s[0] + a0.x) + a1.x) + a2.x) + a3.x;
                s[1 % W] = (((s[1 % W] + a0.y) + a1.y) + a2.y) + a3.y;
                s[2 % W] = (((s[2 % W] + a0.z) + a1.z) + a2.z) + a3.z;
                s[3 % W] = (((s[3 % W] + a0.w) + a1.w) + a2.w) + a3.w;
            }
        }
        for (; k < k_hi; ++k) {
#pragma unroll
            for (int e = 0; e < W; ++e) s[e] += P[(int64_t)k * MN + e];
        }
        if (QUAD) {
#pragma unroll
            for (int e = 0; e < W; ++e) {
                s[e] += __shfl_xor(s[e], 1, 64);         // q0 + q1 | q2 + q3 (both lanes of a pair hold the same sum)
                s[e] += __shfl_xor(s[e], 2, 64);         // (q0 + q1) + (q2 + q3)
            }
            if (q != 0) continue;
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float v = (float)s[e];
            const int c = col + e;
            if (c >= p.N) {                      // side-product columns ride behind the N main columns of a slab row
                if (c - p.N < p.sp_r) p.cx[(int64_t)row * p.cx_ms + (int64_t)(c - p.N) * p.cx_rs] = v;
                continue;
            }
            if (p.bias) v += p.bias[(int64_t)b * p.sBias + c];
            if (c < p.act_cols) v = rn_act(v, p.act);
            if (p.emul) {
                const float ev = p.emul[(int64_t)b * p.sE + (int64_t)row * p.lde + c];
                v *= (p.e_mode == RECNOW_OPMODE_ACTGRAD) ? rn_act_grad_from_out(ev, p.e_act) : ev;
            }
            float* dst = p.C + (int64_t)b * p.sC + (p.c_trans ? ((int64_t)c * p.ldc + row) : ((int64_t)row * p.ldc + c));
            if (p.perm_s > 0) dst = p.C + ((int64_t)(c / p.perm_s) * p.M + row) * p.perm_s + (c % p.perm_s);      // [N/s][M][s] layout
            if (p.accumulate) v += *dst;
            *dst = v;
        }
    }
}
template <bool VEC, bool QUAD>
__global__ void __launch_bounds__(256)
k_gemm_splitk_reduce(const GemmK p) {
    splitk_reduce_body<VEC, QUAD>(p, blockIdx.x, gridDim.x);
}

// One launch at the end of a DCN-v2 cross layer's backward: the slab reductions of its two K = B weight-gradient products (dW with
// dbias riding as side columns, dU with dgate) and the sum of the sub-space kernel's per-workgroup dV partials -- three launches of a
// few microseconds each otherwise.  Blocks [0, na) run reduction a, [na, na + nb) reduction b, the rest the dV sum (64 columns per
// block: 4 strided groups of partials, fixed order, then a 4-term LDS sum).
__device__ __forceinline__ void reduce_variant(const GemmK& p, int variant, int bid, int nblk) {
    if (variant == 2) splitk_reduce_body<true, true>(p, bid, nblk);
    else if (variant == 1) splitk_reduce_body<true, false>(p, bid, nblk);
    else splitk_reduce_body<false, false>(p, bid, nblk);
}
__global__ void __launch_bounds__(256)
k_layer_end_reduce(const GemmK pa, int va, int na, const GemmK pb, int vb, int nb, const float* __restrict__ dv_part, int dv_nparts, int dv_total,
                   float* __restrict__ dV) {
    const int bid = blockIdx.x;
    if (bid < na) { reduce_variant(pa, va, bid, na); return; }
    if (bid < na + nb) { reduce_variant(pb, vb, bid - na, nb); return; }
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = (bid - na - nb) * 64 + e;
    float s[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] = 0.f;
    if (i < dv_total) {
        int g = q;
        for (; g + 4 * 7 < dv_nparts; g += 4 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] += dv_part[(int64_t)(g + 4 * u) * dv_total + i];
        }
        for (; g < dv_nparts; g += 4) s[0] += dv_part[(int64_t)g * dv_total + i];
    }
    red[q][e] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (q == 0 && i < dv_total) dV[i] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// ---- host dispatch -------------------------------------------------------------------------------------
// The route of a launch is planned on the host (gemm_dispatch.hpp rn_gemm_plan: host-only, so that it also builds under the CPU sanitizers); what
// follows reads the process's switches, fills the kernel arguments and launches what the plan names.
#include "gemm_split.hpp"

static std::atomic<int> g_gemm_staging{rn_env_int("RECNOW_GEMM_GLDS", 0) == 1 ? 1 : 0};      // recnow_set_gemm_staging
static int g_gemm_precision = []() {
    const char* e = getenv("RECNOW_GEMM_PRECISION");
    return (e && (!strcmp(e, "bf16x3") || !strcmp(e, "1"))) ? 1 : 0;
}();
int rn_gemm_precision() { return g_gemm_precision; }
int rn_gemm_set_precision(int mode) {
    if (mode != 0 && mode != 1) return RECNOW_EINVAL;
    g_gemm_precision = mode;
    return RECNOW_OK;
}
static inline RnDispatchEnv dispatch_env() {
    static const int bm64 = rn_env_int("RECNOW_GEMM_BM64", 256);        // A/B: 0 = off, N = tile bound
    static const int kb = rn_env_int("RECNOW_GEMM_BM64_KB", -1);       // A/B: 0 = only to fill the chip, 1 = always
    static const int longk = rn_env_int("RECNOW_SPLIT_LONGK", 1), shortk = rn_env_int("RECNOW_SPLIT_SHORTK", 1);      // A/B switches (RnDispatchEnv)
    static const int lean = rn_env_int("RECNOW_SPLIT_LEAN", 1), pair = rn_env_int("RECNOW_S3_PAIR", 1);
    RnDispatchEnv e{bm64, kb, g_gemm_precision};
    e.staging = g_gemm_staging.load(std::memory_order_relaxed);
    e.split_longk = longk; e.split_shortk = shortk; e.split_lean = lean; e.s3_pair = pair;
    return e;
}

size_t rn_gemm_ws_bytes(const recnow_gemm_desc* d) { return rnd_ws_bytes(d, dispatch_env()); }
size_t rn_gemm_split_planes_bytes(int K, int N) { return rnd_planes_bytes(K, N); }

static_assert(sizeof(GemmK) <= sizeof(((RnDeferredReduce*)nullptr)->k), "RnDeferredReduce::k holds a GemmK");

// the kernel arguments of a planned launch
static GemmK gemm_args(const recnow_gemm_desc* d, const RnGemmPlan& p, void* ws) {
    GemmK k;
    k.A = d->A; k.A2 = d->a_mode ? d->A2 : nullptr; k.B = d->B; k.B2 = d->b_mode ? d->B2 : nullptr;
    k.bias = d->bias; k.emul = d->emul; k.C = d->C; k.partial = p.splitk > 1 ? (float*)ws : nullptr;
    k.lda = d->lda; k.ldb = d->ldb; k.ldc = d->ldc; k.lde = d->lde;
    k.sA = d->a_batch_stride; k.sB = d->b_batch_stride; k.sC = d->c_batch_stride;
    k.sBias = d->bias_batch_stride; k.sE = d->e_batch_stride;
    k.M = d->M; k.N = d->N; k.K = d->K; k.batch = d->batch;
    k.a_mode = d->a_mode; k.a_act = d->a_act; k.b_mode = d->b_mode; k.b_act = d->b_act;
    k.act = d->act; k.act_cols = d->act_cols > 0 ? d->act_cols : d->N; k.e_mode = d->e_mode; k.e_act = d->e_act;
    k.accumulate = d->accumulate; k.c_trans = d->c_trans;
    k.a_hq = d->a_hq > 0 ? d->a_hq : 1; k.b_hq = d->b_hq > 0 ? d->b_hq : 1; k.a_ld2 = d->a_ld2; k.b_ld2 = d->b_ld2;
    k.bx = d->sp_bx; k.cx = d->sp_cx; k.bx_ks = d->sp_bx_ks; k.bx_rs = d->sp_bx_rs; k.cx_ms = d->sp_cx_ms; k.cx_rs = d->sp_cx_rs;
    k.sp_r = d->sp_r;
    k.eu_p = d->eu_p; k.eu_q = d->eu_q; k.eu_pms = d->eu_pms; k.eu_qrs = d->eu_qrs; k.eu_qns = d->eu_qns; k.eu_r = d->eu_r;
    k.npart = d->N + (d->sp_r > 0 ? 4 : 0);
    k.splitk = p.splitk; k.kchunk = p.kchunk;
    k.perm_s = d->c_perm_s > 0 ? d->c_perm_s : 0;       // the permuted store lives in the split-K reduce
    k.trace = nullptr;
    k.tail_pairs = p.tail_pairs;
    k.prio = 0;
    k.direct_store = 1;
    k.C2 = d->C2; k.E2 = d->E2; k.ldc2 = d->ldc2; k.lde2 = d->lde2;
    k.as_in = d->as_in; k.as_out = d->as_out;
    k.E4 = d->E4; k.E5 = d->E5; k.E6 = d->E6;
    k.A_hi = nullptr; k.planes_hi = nullptr;      // (rn_gemm_dx_once_split only)
    k.E3 = d->E3; k.lde3 = d->lde3; k.rv = d->rv; k.cv = d->cv; k.hv = d->hv; k.hp = d->hp; k.hp_ld = d->hp_ld;
    k.mid_V = d->mid_V; k.mid_T1 = d->mid_T1; k.mid_T2 = d->mid_T2; k.mid_T2g = d->mid_T2g; k.mid_ld = d->mid_ld; k.mid_act_outer = d->mid_act_outer;
#ifdef RN_GEMM_TRACE
    if (const char* t = getenv("RECNOW_GEMM_TRACE")) k.trace = (long long*)strtoull(t, nullptr, 10);
#endif
    k.xcd_remap = p.xcd_remap;
    return k;
}

// the planned k_gemm instantiation: lean kernels for the (layout, operand-kind) combos the layers use, the general (EDGE) kernel of the same tile
// family for anything else
static int launch_kgemm(const GemmK& k, const RnGemmPlan& p, dim3 grid, hipStream_t st) {
    if (p.edge) return rn_gemm_launch_edge(k, p.BM, p.BN, p.a_kc, p.b_kc, grid, st);
    if (p.BM == 64) return rn_gemm_launch_lean64x(k, p.a_kc, p.b_kc, p.a2k, p.b2k, p.xf, grid, st);
    if (p.BM == 256) return rn_gemm_launch_lean64(k, p.a_kc, p.b_kc, p.a2k, p.b2k, grid, st);
    if (p.xf) return rn_gemm_launch_lean128x(k, p.a_kc, p.b_kc, p.BK, p.a2k, p.b2k, p.xf, grid, st);
    return p.BN == 160 ? rn_gemm_launch_lean160(k, p.a_kc, p.b_kc, p.BK, p.a2k, p.b2k, grid, st)
                       : rn_gemm_launch_lean128(k, p.a_kc, p.b_kc, p.BK, p.a2k, p.b2k, grid, st);
}

static int rn_gemm_impl(const recnow_gemm_desc* d, void* ws, size_t ws_bytes, hipStream_t st, RnDeferredReduce* defer, const RnGemmOpts& o) {
    if (defer) defer->valid = 0;
    RnGemmPlan p;
    int rc = rn_gemm_plan(d, o, ws != nullptr, ws_bytes, dispatch_env(), &p);
    if (rc || p.family == RN_GF_NONE) return rc;
    const GemmK k = gemm_args(d, p, ws);
    RnProfRecord* pr = nullptr;
    if (rn_prof_on()) {
        // algorithmic HBM bytes: every operand read once, every output written once (read-modify-write outputs count twice)
        const double mk = (double)d->M * d->K, kn = (double)d->K * d->N, mn = (double)d->M * d->N;
        const double elems = mk * (1 + (d->a_mode && d->a_mode != RECNOW_OPMODE_OUTER ? 1 : 0)) + kn * (1 + (d->b_mode && d->b_mode != RECNOW_OPMODE_OUTER ? 1 : 0)) +
                             mn * (1 + (d->emul ? 1 : 0) + (d->accumulate ? 1 : 0)) +
                             (d->c2_mode == 1 ? mn : d->c2_mode == 2 ? 3 * mn : d->c2_mode == 3 ? 0.0 : d->c2_mode == 4 ? 3 * mn : d->c2_mode == 5 ? 5 * mn : d->c2_mode == 6 ? 3 * mn : 0.0) +
                             (d->as_out ? 2 * mk : 0.0);
        pr = rn_prof_begin(p.tag, d->prof_flops > 0.0 ? d->prof_flops : 2.0 * d->M * d->N * (double)d->K * d->batch, 4.0 * elems * d->batch, st);
    }
    char* const planes = p.planes == 2 ? (char*)o.planes_ready : p.planes == 1 ? (char*)ws + p.planes_off : nullptr;
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
    switch (p.family) {
        case RN_GF_GEMM: rc = launch_kgemm(k, p, grid, st); break;
        case RN_GF_SHORTK: rc = rn_gemm_launch_shortk(k, p.b_kc, p.ep, p.c2_mode, st); break;
        case RN_GF_SHORTK_SPLIT: rc = rn_gemm_launch_shortk_split(k, p.b_kc, p.ep, p.c2_mode, planes, p.planes == 1, st); break;
        default: rc = rn_gemm_launch_split(k, p, planes, grid, st); break;
    }
    rn_prof_end(pr, st);
    if (rc) return rc;
    if (p.splitk > 1) {
        if (defer) {             // the caller runs the reduction (rn_layer_end_reduce)
            memcpy(defer->k, &k, sizeof(GemmK));
            defer->variant = p.reduce_variant;
            defer->blocks = p.reduce_blocks;
            defer->valid = 1;
            return RECNOW_OK;
        }
        if (p.reduce_variant == 2) hipLaunchKernelGGL((k_gemm_splitk_reduce<true, true>), p.reduce_blocks, 256, 0, st, k);
        else if (p.reduce_variant == 1) hipLaunchKernelGGL((k_gemm_splitk_reduce<true, false>), p.reduce_blocks, 256, 0, st, k);
        else hipLaunchKernelGGL((k_gemm_splitk_reduce<false, false>), p.reduce_blocks, 256, 0, st, k);
        RN_LAUNCH_CHECK();
    }
    return RECNOW_OK;
}
int rn_gemm(const recnow_gemm_desc* d, void* ws, size_t ws_bytes, hipStream_t st, const RnGemmOpts& o) { return rn_gemm_impl(d, ws, ws_bytes, st, nullptr, o); }
int rn_gemm_deferred(const recnow_gemm_desc* d, void* ws, size_t ws_bytes, hipStream_t st, RnDeferredReduce* out, const RnGemmOpts& o) {
    if (!out) return RECNOW_EINVAL;
    return rn_gemm_impl(d, ws, ws_bytes, st, out, o);
}
// c2_mode 7 / 8 of the short-K kernel (gemm.hpp: RnDxOnce).  The caller owns the shape rules; what a wrong call could turn into an access out of
// bounds or a misaligned 16-byte access is checked here.
int rn_gemm_dx_once_split(const RnDxOnce& q, hipStream_t st) {
    if (!q.A_lo || !q.A_hi || !q.planes_lo || !q.planes_hi || !q.E2 || !q.E3 || !q.C || (q.E4 != nullptr) != (q.E5 != nullptr)) return RECNOW_EINVAL;
    if (q.M <= 0 || q.N <= 0 || q.M % 128 || q.N % 128 || q.lda < 144 || q.ld < q.N || (int64_t)128 * q.lda >= (1ll << 29) || (int64_t)128 * q.ld >= (1ll << 29))
        return RECNOW_EUNSUPPORTED;
    if (!rnd_aligned(q.A_lo, q.lda, 0) || !rnd_aligned(q.A_hi, q.lda, 0) || !rnd_aligned(q.C, q.ld, 0) || !rnd_aligned(q.E2, q.ld, 0) ||
        !rnd_aligned(q.E3, q.ld, 0) || (q.E4 && (!rnd_aligned(q.E4, q.ld, 0) || !rnd_aligned(q.E5, q.ld, 0))) || ((uintptr_t)q.planes_lo & 15) ||
        ((uintptr_t)q.planes_hi & 15))
        return RECNOW_EUNSUPPORTED;
    GemmK k;
    memset(&k, 0, sizeof(k));
    k.A = q.A_lo; k.A_hi = q.A_hi; k.lda = q.lda; k.planes_hi = (const char*)q.planes_hi;
    k.C = q.C; k.ldc = q.ld;
    k.E2 = q.E2; k.E3 = q.E3; k.E4 = q.E4; k.E5 = q.E5; k.lde2 = k.lde3 = q.ld;
    k.M = q.M; k.N = q.N; k.K = 288; k.batch = 1; k.splitk = 1; k.kchunk = 288; k.tail_pairs = 8; k.direct_store = 1;
    RnProfRecord* pr = nullptr;
    if (rn_prof_on()) {      // algorithmic HBM bytes: both A halves and the planes read once, 2 / 4 (M, N) tensors read, C written
        const double mn = (double)q.M * q.N;
        pr = rn_prof_begin(RN_TAG_GEMM_SHORTK, 2.0 * mn * 288.0, 4.0 * (2.0 * q.M * 144.0 + 2.0 * 144.0 * q.N + mn * (q.E4 ? 5 : 3)), st);
    }
    const int rc = rn_gemm_launch_shortk_split2(k, q.E4 ? 7 : 8, q.planes_lo, st);
    rn_prof_end(pr, st);
    return rc;
}
void rn_deferred_slabs(const RnDeferredReduce* r, const float** partial, int* nsplit, int* ld, int64_t* stride) {
    GemmK k;
    memcpy(&k, r->k, sizeof(GemmK));
    *partial = k.partial;
    *nsplit = k.splitk;
    *ld = k.npart;
    *stride = (int64_t)k.M * k.npart;
}
int rn_layer_end_reduce(const RnDeferredReduce* a, const RnDeferredReduce* b, const float* dv_part, int dv_nparts, int dv_total, float* dV,
                        hipStream_t st) {
    GemmK ka, kb;
    memset(&ka, 0, sizeof(ka));
    memset(&kb, 0, sizeof(kb));
    const int na = (a && a->valid) ? a->blocks : 0, nb = (b && b->valid) ? b->blocks : 0;
    if (na) memcpy(&ka, a->k, sizeof(GemmK));
    if (nb) memcpy(&kb, b->k, sizeof(GemmK));
    const int nv = (dv_part && dV && dv_nparts > 0 && dv_total > 0) ? rn_cdiv(dv_total, 64) : 0;
    if (na + nb + nv == 0) return RECNOW_OK;
    hipLaunchKernelGGL(k_layer_end_reduce, na + nb + nv, 256, 0, st, ka, na ? a->variant : 0, na, kb, nb ? b->variant : 0, nb, dv_part, dv_nparts,
                       dv_total, dV);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// ---- deterministic column sum (bias gradients) -----------------------------------------------------------
#define CS_ROWS_PER_BLOCK 512
#define CS_MIN_ROWS 16
// rows per workgroup: 512 for tall matrices, fewer when that would leave most of the 256 CUs idle
static inline int cs_rows(int64_t M, int64_t N) {
    const int64_t colblk = (N + 255) / 256;
    int64_t r = CS_ROWS_PER_BLOCK;
    while (r > CS_MIN_ROWS && ((M + r - 1) / r) * colblk < 512) r /= 2;
    return (int)r;
}
__device__ __forceinline__ float cs_term(const float* __restrict__ X, const float* __restrict__ X2, int mode, int act, int64_t i) {
    float v = X[i];
    if (mode == RECNOW_OPMODE_MUL) v *= X2[i];
    else if (mode == RECNOW_OPMODE_ACTGRAD) v *= rn_act_grad_from_out(X2[i], act);
    return v;
}
__global__ void __launch_bounds__(256)
k_colsum_partial(const float* __restrict__ X, const float* __restrict__ X2, int mode, int act, int64_t M, int64_t N, int64_t ld,
                 float* __restrict__ part, int rows, int cw, int64_t x_bs, int64_t part_bs) {
    // blockIdx.z: one of a batch of equally shaped matrices (rn_colsum_batched: the bias gradients of all experts of a layer in ONE launch -- a
    // single (32 768 x 512) matrix is 128 workgroups, half the chip; round 5)
    X += (int64_t)blockIdx.z * x_bs;
    if (X2) X2 += (int64_t)blockIdx.z * x_bs;
    part += (int64_t)blockIdx.z * part_bs;
    // block (bx, by): columns bx*cw + (tid % cw), rows by*rows .. ; the 256/cw row lanes of a column take rows rl apart
    // (cw = 64 or 128 for matrices narrower than 256 columns: all 256 threads load), four loads in flight each, and are
    // summed in a fixed order through LDS
    // fp64 accumulators (the kernel is bound by its loads; a bias gradient is a sum of up to 512 rows per workgroup here and of the slabs
    // after it, with cancellation: summed in fp32 the full-size PLE + listwise test sat at 1.08e-5 of its 1e-5 bound)
    __shared__ double red[256];
    const int c = threadIdx.x % cw, rlane = threadIdx.x / cw, rl = 256 / cw;
    const int64_t col = (int64_t)blockIdx.x * cw + c;
    const int64_t r0 = (int64_t)blockIdx.y * rows;
    const int64_t r1 = min(M, r0 + rows);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (col < N) {
        int64_t r = r0 + rlane;
        for (; r + 3 * rl < r1; r += 4 * rl) {
            s0 += cs_term(X, X2, mode, act, r * ld + col);
            s1 += cs_term(X, X2, mode, act, (r + rl) * ld + col);
            s2 += cs_term(X, X2, mode, act, (r + 2 * rl) * ld + col);
            s3 += cs_term(X, X2, mode, act, (r + 3 * rl) * ld + col);
        }
        for (; r < r1; r += rl) s0 += cs_term(X, X2, mode, act, r * ld + col);
    }
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (rlane == 0 && col < N) {
        double t = red[c];
        for (int u = 1; u < rl; ++u) t += red[u * cw + c];
        part[(int64_t)blockIdx.y * N + col] = (float)t;
    }
}
// out[col] = sum over slabs, fixed order: 64 columns x 16 strided slab groups per workgroup, then a 16-term LDS sum (a
// column-per-thread loop over hundreds of slabs is a chain of dependent-latency loads: 84 us for 512 slabs, measured)
__global__ void __launch_bounds__(1024)
k_colsum_final(const float* __restrict__ part, int nslab, int64_t N, float* __restrict__ out, int accumulate, int64_t part_bs, int64_t out_bs) {
    __shared__ double red[16][64];
    part += (int64_t)blockIdx.y * part_bs;
    out += (int64_t)blockIdx.y * out_bs;
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t col = (int64_t)blockIdx.x * 64 + e;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < N) {
        int i = q;
        for (; i + 48 < nslab; i += 64) {
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += part[(int64_t)(i + 16 * u) * N + col];
        }
        for (; i < nslab; i += 16) s[0] += part[(int64_t)i * N + col];
    }
    red[q][e] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (q == 0 && col < N) {
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) t += red[u][e];
        out[col] = accumulate ? (float)((double)out[col] + t) : (float)t;
    }
}

// narrow matrices (N < 64): one workgroup column-strip per (column, row-chunk), all 256 threads walk the rows
#define CS_NARROW_ROWS 8192
__global__ void __launch_bounds__(256)
k_colsum_narrow(const float* __restrict__ X, const float* __restrict__ X2, int mode, int act, int64_t M, int64_t N, int64_t ld,
                float* __restrict__ part) {
    __shared__ double red[16];
    const int64_t col = blockIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * CS_NARROW_ROWS, r1 = min(M, r0 + CS_NARROW_ROWS);
    double s = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        float v = X[r * ld + col];
        if (mode == RECNOW_OPMODE_MUL) v *= X2[r * ld + col];
        else if (mode == RECNOW_OPMODE_ACTGRAD) v *= rn_act_grad_from_out(X2[r * ld + col], act);
        s += v;
    }
    s = block_sum<double>(s, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * N + col] = (float)s;
}

size_t rn_colsum_ws_bytes(int64_t M, int64_t N) {
    // upper bound valid for every row count <= M (callers size the workspace for an upper bound of M): rows per
    // workgroup are halved only while slabs * colblk < 512, so slabs <= max(ceil(M/512), 1024/colblk + 2)
    const int64_t m = M > 0 ? M : 1, n = N > 0 ? N : 1;
    const int64_t colblk = (n + 255) / 256;
    int64_t slabs = rn_cdiv(m, CS_ROWS_PER_BLOCK);
    const int64_t alt = 1024 / colblk + 2;
    if (alt > slabs) slabs = alt;
    return rn_align((size_t)(slabs + 1) * (size_t)n * sizeof(float));
}

int rn_colsum(const float* X, const float* X2, int mode, int act, int64_t M, int64_t N, int64_t ld, float* out,
              int accumulate, void* ws, size_t ws_bytes, hipStream_t st) {
    if (M < 0 || N < 0) return RECNOW_EINVAL;
    if (N == 0) return RECNOW_OK;
    if (!out) return RECNOW_EINVAL;
    if (M == 0) {
        if (!accumulate) RN_HIP(hipMemsetAsync(out, 0, (size_t)N * sizeof(float), st));
        return RECNOW_OK;
    }
    if (!X || (mode && !X2) || !ws) return RECNOW_EINVAL;
    if (ws_bytes < rn_colsum_ws_bytes(M, N)) return RECNOW_EWORKSPACE;
    const int rows = cs_rows(M, N);
    int nslab = rn_cdiv(M, rows);
    if (N < 64) {
        nslab = rn_cdiv(M, CS_NARROW_ROWS);
        dim3 gn((unsigned)N, nslab);
        hipLaunchKernelGGL(k_colsum_narrow, gn, 256, 0, st, X, X2, mode, act, M, N, ld, (float*)ws);
    } else {
        const int cw = N <= 64 ? 64 : N <= 128 ? 128 : 256;
        dim3 g1(rn_cdiv(N, cw), nslab);
        hipLaunchKernelGGL(k_colsum_partial, g1, 256, 0, st, X, X2, mode, act, M, N, ld, (float*)ws, rows, cw, (int64_t)0, (int64_t)0);
    }
    hipLaunchKernelGGL(k_colsum_final, rn_cdiv(N, 64), 1024, 0, st, (const float*)ws, nslab, N, out, accumulate, (int64_t)0, (int64_t)0);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// `batch` matrices of one shape, x_bs floats apart (X2 likewise), out[b * out_bs + col]: two launches for all of them.  N >= 64 columns (narrower
// ones: one rn_colsum per matrix).  ws: batch * rn_colsum_ws_bytes(M, N).  The sums of a matrix are those of rn_colsum, term for term.
int rn_colsum_batched(const float* X, const float* X2, int mode, int act, int64_t M, int64_t N, int64_t ld, int batch, int64_t x_bs, float* out,
                      int64_t out_bs, void* ws, size_t ws_bytes, hipStream_t st) {
    if (M < 1 || N < 64 || batch < 1 || batch > 65535) return RECNOW_EUNSUPPORTED;
    if (!X || (mode && !X2) || !ws || !out) return RECNOW_EINVAL;
    const size_t one = rn_colsum_ws_bytes(M, N);
    if (ws_bytes < one * (size_t)batch) return RECNOW_EWORKSPACE;
    const int rows = cs_rows(M, N);
    const int nslab = rn_cdiv(M, rows);
    const int cw = N <= 64 ? 64 : N <= 128 ? 128 : 256;
    const int64_t part_bs = (int64_t)(one / sizeof(float));
    dim3 g1(rn_cdiv(N, cw), nslab, batch);
    hipLaunchKernelGGL(k_colsum_partial, g1, 256, 0, st, X, X2, mode, act, M, N, ld, (float*)ws, rows, cw, x_bs, part_bs);
    dim3 g2(rn_cdiv(N, 64), batch);
    hipLaunchKernelGGL(k_colsum_final, g2, 1024, 0, st, (const float*)ws, nslab, N, out, 0, part_bs, out_bs);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_set_gemm_precision(int mode) { return rn_gemm_set_precision(mode); }
extern "C" int recnow_set_gemm_staging(int mode) {
    if (mode != 0 && mode != 1) return RECNOW_EINVAL;
    g_gemm_staging.store(mode, std::memory_order_relaxed);
    return RECNOW_OK;
}
extern "C" int recnow_get_gemm_staging(void) { return g_gemm_staging.load(std::memory_order_relaxed); }
extern "C" int recnow_get_gemm_precision(void) { return rn_gemm_precision(); }
extern "C" size_t recnow_gemm_workspace_bytes(const recnow_gemm_desc* desc_host) {
    return desc_host ? rn_gemm_ws_bytes(desc_host) : 0;
}
extern "C" int recnow_gemm(const recnow_gemm_desc* desc_host, void* ws, size_t ws_bytes, void* stream) {
    return rn_gemm(desc_host, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int recnow_gemm_route(const recnow_gemm_desc* desc_host, size_t ws_bytes, recnow_gemm_route_info* out) {
    if (!out) return RECNOW_EINVAL;
    RnGemmPlan p;
    const int rc = rn_gemm_plan(desc_host, RnGemmOpts(), ws_bytes > 0, ws_bytes, dispatch_env(), &p);
    *out = recnow_gemm_route_info{p.family, p.BM, p.BN, p.BK, p.a_kc, p.b_kc, p.edge, p.a2k, p.b2k, p.xf, p.bp, p.pair, p.ep, p.c2_mode, p.planes,
                                  p.splitk, p.kchunk, p.grid_x, p.grid_y, p.grid_z, p.xcd_remap, p.tail_pairs, p.reduce_variant, p.reduce_blocks, p.tag};
    return rc;
}
