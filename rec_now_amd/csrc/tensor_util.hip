// Tensor plumbing of three reference modules, each an HBM-bound copy or reduction with no arithmetic to speak of:
//   rec_now/layers/pooling_layer.py                 PoolingLayer (reduce_sum / mean / max / min)   -> k_reduce_* / k_reduce_bwd_*
//   rec_now/layers/fix_length_layer.py              pad_or_truncate, FixLengthLayer                -> k_pad_axis (its own backward)
//   rec_now/rec_block/embedding_wise_weight.py      gather_embedding_element_wise_weight           -> k_elw_fwd / k_elw_bwd (+ the fused multiply)
// Every contiguous input is viewed as (O, R, I): outer, the axis worked on, inner; the host folds the shape and no kernel sees a rank.
// No floating-point atomics: every sum adds in an order fixed by the shape alone, so the same input gives the same bits on every run.
// Tensors a launch touches once go through non-temporal float4 (16-byte) accesses where the sizes and bases allow, scalar ones otherwise.
#include "common.hpp"
#include <math.h>

typedef uint32_t tu_u4 __attribute__((ext_vector_type(4)));
typedef int tu_i4 __attribute__((ext_vector_type(4)));

#define TU_ROW_WAVE_MAX 4096        // a single row (O == 1, I == 1) up to this length is one wave's work; longer rows take the two-stage path
#define TU_FLAT_BLOCKS 1024         // most workgroups (= partials in the workspace) of the two-stage path
#define TU_ELW_LDS 4096             // floats of LDS a workgroup stages weights in: rows of E <= TU_ELW_LDS weights are staged, wider ones are
                                    // read through the cache (16 KB keeps eight workgroups per CU resident; an E beyond it is no embedding count)

static inline bool tu_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- reduce over R ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tu_init(int op) { return op <= RECNOW_REDUCE_MEAN ? 0.f : (op == RECNOW_REDUCE_MAX ? -INFINITY : INFINITY); }
__device__ __forceinline__ float tu_comb(float a, float b, int op) {
    return op <= RECNOW_REDUCE_MEAN ? a + b : (op == RECNOW_REDUCE_MAX ? fmaxf(a, b) : fminf(a, b));
}
__device__ __forceinline__ rn_f4 tu_comb(rn_f4 a, rn_f4 b, int op) {
    return rn_f4{tu_comb(a.x, b.x, op), tu_comb(a.y, b.y, op), tu_comb(a.z, b.z, op), tu_comb(a.w, b.w, op)};
}
template <typename T> __device__ __forceinline__ T tu_splat(float v);
template <> __device__ __forceinline__ float tu_splat<float>(float v) { return v; }
template <> __device__ __forceinline__ rn_f4 tu_splat<rn_f4>(float v) { return rn_f4{v, v, v, v}; }

// Splits of R a workgroup of the column kernels makes: none when the columns alone fill the chip (or R is short), 4 or 16 otherwise.
static int tu_col_splits(int64_t NC, int64_t R) {
    if (NC >= 65536 || R < 8) return 1;
    return (NC < 16384 && R >= 64) ? 16 : 4;
}

// I >= 2.  A column is one float4 (V4) or one float of the inner axis of one outer index: NC = O * Iv of them.  A workgroup is S splits x CW = 256 / S
// columns: lanes run along I, thread (s, c) walks the s-th contiguous piece of R, and split 0 adds the S partials in ascending s through LDS.
template <typename T>
__global__ void __launch_bounds__(256)
k_reduce_cols(const float* __restrict__ x, int64_t NC, int64_t R, int64_t I, int64_t Iv, int S, int op, float* __restrict__ out) {
    constexpr int W = sizeof(T) / 4;
    __shared__ T part[256];
    const int CW = 256 / S, ci = threadIdx.x % CW, s = threadIdx.x / CW;
    const int64_t c = (int64_t)blockIdx.x * CW + ci;
    const int64_t ch = (R + S - 1) / S;
    const int64_t r0 = min(R, s * ch), r1 = min(R, r0 + ch);
    T acc = tu_splat<T>(tu_init(op));
    if (c < NC) {
        const int64_t o = c / Iv, iv = c - o * Iv;
        const float* const p = x + o * R * I + iv * W;
#pragma unroll 4
        for (int64_t r = r0; r < r1; ++r) acc = tu_comb(acc, RN_LD_STREAM(reinterpret_cast<const T*>(p + r * I)), op);
    }
    if (S > 1) {
        part[threadIdx.x] = acc;
        __syncthreads();
        if (s == 0)
            for (int k = 1; k < S; ++k) acc = tu_comb(acc, part[k * CW + ci], op);
    }
    if (s == 0 && c < NC) {
        if (op == RECNOW_REDUCE_MEAN) acc = acc / tu_splat<T>((float)R);
        RN_ST_STREAM(reinterpret_cast<T*>(out + c * W), acc);
    }
}

// I == 1.  A group of GS lanes (a power of two <= 64, the first that covers R) owns one row, so 64 / GS rows share a wave; the group's lanes run
// along R and the partials meet in a butterfly within the group.
__global__ void __launch_bounds__(256)
k_reduce_rows(const float* __restrict__ x, int64_t O, int64_t R, int GS, int op, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, G = 64 / GS, grp = lane / GS, gl = lane % GS;
    for (int64_t row0 = ((int64_t)blockIdx.x * 4 + w) * G; row0 < O; row0 += (int64_t)gridDim.x * 4 * G) {      // wave-uniform: every lane shuffles
        const int64_t row = row0 + grp;
        float acc = tu_init(op);
        if (row < O)
            for (int64_t r = gl; r < R; r += GS) acc = tu_comb(acc, RN_LD_STREAM(x + row * R + r), op);
        for (int o = GS >> 1; o > 0; o >>= 1) acc = tu_comb(acc, __shfl_xor(acc, o, 64), op);
        if (row < O && gl == 0) out[row] = op == RECNOW_REDUCE_MEAN ? acc / (float)R : acc;
    }
}

// the workgroup's 256 values -> one, in a fixed order, in every thread (one use per kernel: `red` is not fenced for a second)
__device__ __forceinline__ float tu_block_comb(float acc, int op, float* red) {
    for (int o = 32; o > 0; o >>= 1) acc = tu_comb(acc, __shfl_xor(acc, o, 64), op);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return tu_comb(tu_comb(red[0], red[1], op), tu_comb(red[2], red[3], op), op);
}

// O == 1, I == 1, a long row: workgroup k reduces elements [k * chunk, (k + 1) * chunk) into partial[k] (chunk is a multiple of 4) ...
template <bool V4>
__global__ void __launch_bounds__(256)
k_reduce_flat1(const float* __restrict__ x, int64_t R, int64_t chunk, int op, float* __restrict__ partial) {
    __shared__ float red[4];
    const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(R, b0 + chunk);
    float acc = tu_init(op);
    if (V4) {
        const int64_t v1 = b0 + ((b1 - b0) & ~(int64_t)3);
        rn_f4 a4 = tu_splat<rn_f4>(tu_init(op));
        for (int64_t i = b0 + 4 * (int64_t)threadIdx.x; i < v1; i += 1024) a4 = tu_comb(a4, RN_LD_STREAM(reinterpret_cast<const rn_f4*>(x + i)), op);
        acc = tu_comb(tu_comb(a4.x, a4.y, op), tu_comb(a4.z, a4.w, op), op);
        if (v1 + threadIdx.x < b1) acc = tu_comb(acc, x[v1 + threadIdx.x], op);
    } else {
        for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) acc = tu_comb(acc, RN_LD_STREAM(x + i), op);
    }
    acc = tu_block_comb(acc, op, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// ... and one workgroup combines the NB partials.
__global__ void __launch_bounds__(256)
k_reduce_flat2(const float* __restrict__ partial, int NB, int64_t R, int op, float* __restrict__ out) {
    __shared__ float red[4];
    float acc = tu_init(op);
    for (int i = threadIdx.x; i < NB; i += 256) acc = tu_comb(acc, partial[i], op);
    acc = tu_block_comb(acc, op, red);
    if (threadIdx.x == 0) out[0] = op == RECNOW_REDUCE_MEAN ? acc / (float)R : acc;
}

static bool tu_flat(int64_t O, int64_t R, int64_t I) { return O == 1 && I == 1 && R > TU_ROW_WAVE_MAX; }
static void tu_flat_plan(int64_t R, int* NB, int64_t* chunk) {
    int64_t nb = (R + 4095) / 4096;
    if (nb > TU_FLAT_BLOCKS) nb = TU_FLAT_BLOCKS;
    int64_t ch = (R + nb - 1) / nb;
    ch = (ch + 1023) / 1024 * 1024;
    *chunk = ch;
    *NB = (int)((R + ch - 1) / ch);
}
static int tu_group(int64_t R) {
    int gs = 1;
    while (gs < 64 && gs < R) gs <<= 1;
    return gs;
}
static bool tu_op_ok(int op) { return op >= RECNOW_REDUCE_SUM && op <= RECNOW_REDUCE_MIN; }

extern "C" size_t recnow_reduce_axis_workspace_bytes(int64_t O, int64_t R, int64_t I) {
    return tu_flat(O, R, I) ? TU_FLAT_BLOCKS * sizeof(float) : 0;
}

extern "C" int recnow_reduce_axis_fwd(const float* x, int64_t O, int64_t R, int64_t I, int op, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (O < 0 || R < 0 || I < 0 || !tu_op_ok(op)) return RECNOW_EINVAL;
    if (O == 0 || I == 0) return RECNOW_OK;
    if (R == 0 || !x || !out) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (tu_flat(O, R, I)) {
        if (!ws || ws_bytes < recnow_reduce_axis_workspace_bytes(O, R, I)) return RECNOW_EWORKSPACE;
        int NB;
        int64_t chunk;
        tu_flat_plan(R, &NB, &chunk);
        float* const partial = (float*)ws;
        if (tu_al16(x)) hipLaunchKernelGGL(k_reduce_flat1<true>, NB, 256, 0, st, x, R, chunk, op, partial);
        else hipLaunchKernelGGL(k_reduce_flat1<false>, NB, 256, 0, st, x, R, chunk, op, partial);
        hipLaunchKernelGGL(k_reduce_flat2, 1, 256, 0, st, partial, NB, R, op, out);
    } else if (I == 1) {
        const int GS = tu_group(R);
        int64_t g = (O + 4 * (64 / GS) - 1) / (4 * (64 / GS));
        if (g > 16384) g = 16384;
        hipLaunchKernelGGL(k_reduce_rows, (int)g, 256, 0, st, x, O, R, GS, op, out);
    } else {
        const bool v4 = I % 4 == 0 && tu_al16(x) && tu_al16(out);
        const int64_t Iv = v4 ? I / 4 : I, NC = O * Iv;
        const int S = tu_col_splits(NC, R);
        const int64_t g = (NC + 256 / S - 1) / (256 / S);
        if (g > 0x7fffffffll) return RECNOW_EUNSUPPORTED;
        if (v4) hipLaunchKernelGGL(k_reduce_cols<rn_f4>, (int)g, 256, 0, st, x, NC, R, I, Iv, S, op, out);
        else hipLaunchKernelGGL(k_reduce_cols<float>, (int)g, 256, 0, st, x, NC, R, I, Iv, S, op, out);
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// ---- gradient of the reduction ----------------------------------------------------------------------------------------------------------------
// sum: dx = g broadcast along R; mean: g * (1 / R); max / min (TensorFlow's rule): every position equal to the result y gets g / count, count = the
// number of equal positions of that run of R.  One launch: the owner(s) of a run count, then write.  The thread layouts are the forward's.
__device__ __forceinline__ float tu_pick(float x, float y, float gv) { return x == y ? gv : 0.f; }
__device__ __forceinline__ rn_f4 tu_pick(rn_f4 x, rn_f4 y, rn_f4 gv) {
    return rn_f4{tu_pick(x.x, y.x, gv.x), tu_pick(x.y, y.y, gv.y), tu_pick(x.z, y.z, gv.z), tu_pick(x.w, y.w, gv.w)};
}
__device__ __forceinline__ void tu_count(float& n, float x, float y) { n += x == y ? 1.f : 0.f; }          // exact in fp32 up to 2^24 per thread
__device__ __forceinline__ void tu_count(rn_f4& n, rn_f4 x, rn_f4 y) {
    n = n + rn_f4{x.x == y.x ? 1.f : 0.f, x.y == y.y ? 1.f : 0.f, x.z == y.z ? 1.f : 0.f, x.w == y.w ? 1.f : 0.f};
}

template <typename T>
__global__ void __launch_bounds__(256)
k_reduce_bwd_cols(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, int64_t NC, int64_t R, int64_t I, int64_t Iv,
                  int S, int op, float inv_r, float* __restrict__ dx) {
    constexpr int W = sizeof(T) / 4;
    __shared__ T part[256];
    const int CW = 256 / S, ci = threadIdx.x % CW, s = threadIdx.x / CW;
    const int64_t c = (int64_t)blockIdx.x * CW + ci;
    const bool live = c < NC;
    const int64_t ch = (R + S - 1) / S;
    const int64_t r0 = min(R, s * ch), r1 = min(R, r0 + ch);
    const int64_t o = live ? c / Iv : 0, iv = live ? c - o * Iv : 0;
    const int64_t base = o * R * I + iv * W;
    T gv = tu_splat<T>(0.f), yv = tu_splat<T>(0.f);
    if (live) gv = *reinterpret_cast<const T*>(g + c * W);
    if (op >= RECNOW_REDUCE_MAX) {
        if (live) yv = *reinterpret_cast<const T*>(y + c * W);
        T n = tu_splat<T>(0.f);
        if (live)
            for (int64_t r = r0; r < r1; ++r) tu_count(n, *reinterpret_cast<const T*>(x + base + r * I), yv);      // plain load: read again below
        if (S > 1) {
            part[threadIdx.x] = n;
            __syncthreads();
            n = part[ci];
            for (int k = 1; k < S; ++k) n = n + part[k * CW + ci];          // counts: whole numbers, exact
        }
        gv = gv / n;                                                        // n >= 1 wherever a position is equal (0 / 0 lanes write nothing)
    } else if (op == RECNOW_REDUCE_MEAN) {
        gv = gv * tu_splat<T>(inv_r);
    }
    if (!live) return;
    if (op >= RECNOW_REDUCE_MAX) {
        for (int64_t r = r0; r < r1; ++r)
            RN_ST_STREAM(reinterpret_cast<T*>(dx + base + r * I), tu_pick(RN_LD_STREAM(reinterpret_cast<const T*>(x + base + r * I)), yv, gv));
    } else {
        for (int64_t r = r0; r < r1; ++r) RN_ST_STREAM(reinterpret_cast<T*>(dx + base + r * I), gv);
    }
}

__global__ void __launch_bounds__(256)
k_reduce_bwd_rows(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, int64_t O, int64_t R, int GS, int op, float inv_r,
                  float* __restrict__ dx) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, G = 64 / GS, grp = lane / GS, gl = lane % GS;
    for (int64_t row0 = ((int64_t)blockIdx.x * 4 + w) * G; row0 < O; row0 += (int64_t)gridDim.x * 4 * G) {
        const int64_t row = row0 + grp;
        const bool live = row < O;
        float gv = live ? g[row] : 0.f;
        if (op >= RECNOW_REDUCE_MAX) {
            const float yv = live ? y[row] : 0.f;
            float n = 0.f;
            if (live)
                for (int64_t r = gl; r < R; r += GS) tu_count(n, x[row * R + r], yv);
            for (int o = GS >> 1; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
            gv = gv / n;
            if (live)
                for (int64_t r = gl; r < R; r += GS) RN_ST_STREAM(dx + row * R + r, tu_pick(RN_LD_STREAM(x + row * R + r), yv, gv));
        } else {
            if (op == RECNOW_REDUCE_MEAN) gv *= inv_r;
            if (live)
                for (int64_t r = gl; r < R; r += GS) RN_ST_STREAM(dx + row * R + r, gv);
        }
    }
}

// One long row: every workgroup counts the whole row (it comes from the cache for all but the first; whole numbers, so any order gives the same count)
// and writes its own piece.
__global__ void __launch_bounds__(256)
k_reduce_bwd_flat(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, int64_t R, int64_t chunk, int op, float inv_r,
                  float* __restrict__ dx) {
    __shared__ float red[4];
    const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(R, b0 + chunk);
    float gv = g[0];
    if (op >= RECNOW_REDUCE_MAX) {
        const float yv = y[0];
        float n = 0.f;                                                      // <= R / 256 + 1 per thread, and R < 2^31: exact
        for (int64_t i = threadIdx.x; i < R; i += 256) tu_count(n, x[i], yv);
        n = tu_block_comb(n, RECNOW_REDUCE_SUM, red);                       // whole numbers: exact below 2^24 equal positions, in any order
        gv = gv / n;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) RN_ST_STREAM(dx + i, tu_pick(x[i], yv, gv));
    } else {
        if (op == RECNOW_REDUCE_MEAN) gv *= inv_r;
        for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) RN_ST_STREAM(dx + i, gv);
    }
}

extern "C" int recnow_reduce_axis_bwd(const float* x, const float* y, const float* g, int64_t O, int64_t R, int64_t I, int op, float* dx, void* stream) {
    if (O < 0 || R < 0 || I < 0 || !tu_op_ok(op)) return RECNOW_EINVAL;
    if (O == 0 || I == 0 || R == 0) return RECNOW_OK;
    if (!g || !dx || (op >= RECNOW_REDUCE_MAX && (!x || !y))) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const float inv_r = 1.f / (float)R;
    if (tu_flat(O, R, I)) {
        int64_t nb = (R + 16383) / 16384;                                   // max / min reads the row once per workgroup: few, large pieces
        if (nb > 256) nb = 256;
        const int64_t chunk = (R + nb - 1) / nb;
        hipLaunchKernelGGL(k_reduce_bwd_flat, (int)((R + chunk - 1) / chunk), 256, 0, st, x, y, g, R, chunk, op, inv_r, dx);
    } else if (I == 1) {
        const int GS = tu_group(R);
        int64_t gr = (O + 4 * (64 / GS) - 1) / (4 * (64 / GS));
        if (gr > 16384) gr = 16384;
        hipLaunchKernelGGL(k_reduce_bwd_rows, (int)gr, 256, 0, st, x, y, g, O, R, GS, op, inv_r, dx);
    } else {
        const bool v4 = I % 4 == 0 && tu_al16(dx) && tu_al16(g) && (op < RECNOW_REDUCE_MAX || (tu_al16(x) && tu_al16(y)));
        const int64_t Iv = v4 ? I / 4 : I, NC = O * Iv;
        const int S = tu_col_splits(NC, R);
        const int64_t gr = (NC + 256 / S - 1) / (256 / S);
        if (gr > 0x7fffffffll) return RECNOW_EUNSUPPORTED;
        if (v4) hipLaunchKernelGGL(k_reduce_bwd_cols<rn_f4>, (int)gr, 256, 0, st, x, y, g, NC, R, I, Iv, S, op, inv_r, dx);
        else hipLaunchKernelGGL(k_reduce_bwd_cols<float>, (int)gr, 256, 0, st, x, y, g, NC, R, I, Iv, S, op, inv_r, dx);
    }
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// ---- pad or truncate --------------------------------------------------------------------------------------------------------------------------
// (O, L_in, I) -> (O, L_out, I).  Within one outer index the input run (L_in * I) is a prefix of the output run (L_out * I) or the other way round, so in
// units U of 4, 8 or 16 bytes the op is out[o][j] = j < Win ? in[o][j] : fill for j < Wout (16 bytes where both runs are whole multiples of them and
// both bases aligned: every I * elt that is one, and e.g. a (B, 80) int64 matrix cut to 50 columns).  IDX = 32-bit indices while both tensors stay below 2^31 units.
template <typename U, typename IDX>
__global__ void __launch_bounds__(256)
k_pad_axis(const U* __restrict__ x, IDX Win, IDX Wout, IDX N, U fill, U* __restrict__ out) {
    for (IDX i = (IDX)blockIdx.x * 256 + threadIdx.x; i < N; i += (IDX)gridDim.x * 256) {
        const IDX o = i / Wout, j = i - o * Wout;
        U v = fill;
        if (j < Win) v = RN_LD_STREAM(x + (o * Win + j));
        RN_ST_STREAM(out + i, v);
    }
}

template <typename U>
static int tu_pad_launch(const void* x, int64_t O, int64_t Win, int64_t Wout, U fill, void* out, hipStream_t st) {
    const int64_t N = O * Wout;
    int64_t g = (N + 255) / 256;
    if (g > 32768) g = 32768;
    if (N < 0x7fffffffll - 32768 * 256 && O * Win < 0x7fffffffll)
        hipLaunchKernelGGL((k_pad_axis<U, uint32_t>), (int)g, 256, 0, st, (const U*)x, (uint32_t)Win, (uint32_t)Wout, (uint32_t)N, fill, (U*)out);
    else
        hipLaunchKernelGGL((k_pad_axis<U, int64_t>), (int)g, 256, 0, st, (const U*)x, Win, Wout, N, fill, (U*)out);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

extern "C" int recnow_pad_axis(const void* x, int elt_bytes, int64_t O, int64_t L_in, int64_t L_out, int64_t I, int64_t fill_bits, void* out, void* stream) {
    if (O < 0 || L_in < 0 || L_out < 0 || I < 0 || (elt_bytes != 4 && elt_bytes != 8)) return RECNOW_EINVAL;
    if (O == 0 || I == 0 || L_out == 0) return RECNOW_OK;
    if (!out || (L_in > 0 && !x)) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t lo = (uint32_t)(uint64_t)fill_bits, hi = (uint32_t)((uint64_t)fill_bits >> 32);
    const int64_t in_bytes = L_in * I * elt_bytes, out_bytes = L_out * I * elt_bytes;      // of one outer index: where the runs and the fill begin
    if (in_bytes % 16 == 0 && out_bytes % 16 == 0 && tu_al16(out) && (L_in == 0 || tu_al16(x))) {
        const tu_u4 f = elt_bytes == 8 ? tu_u4{lo, hi, lo, hi} : tu_u4{lo, lo, lo, lo};
        return tu_pad_launch<tu_u4>(x, O, in_bytes / 16, out_bytes / 16, f, out, st);
    }
    if (elt_bytes == 8) return tu_pad_launch<uint64_t>(x, O, L_in * I, L_out * I, (uint64_t)fill_bits, out, st);
    return tu_pad_launch<uint32_t>(x, O, L_in * I, L_out * I, lo, out, st);
}

// ---- element-wise weights ---------------------------------------------------------------------------------------------------------------------
// out[b][p] = w[b][pos[p]] (gather), times x[b][p] when x is given (apply: the (B, P) weight tensor is never written).  A workgroup takes RB rows at a
// time: their RB * E weights are one contiguous piece of w, staged in LDS (LDS = true, E <= TU_ELW_LDS) or read through the cache (wider rows), and its
// RB * P outputs are one contiguous piece of out, written coalesced in float4 where P % 4 == 0 and the bases allow.
template <bool V4, bool LDS>
__global__ void __launch_bounds__(256)
k_elw_fwd(const float* __restrict__ w, const int32_t* __restrict__ pos, const float* __restrict__ x, int64_t B, int E, int P, int RB, float* __restrict__ out) {
    __shared__ float sw[LDS ? TU_ELW_LDS : 1];
    const int Pv = V4 ? P / 4 : P;
    for (int64_t b0 = (int64_t)blockIdx.x * RB; b0 < B; b0 += (int64_t)gridDim.x * RB) {
        const int nr = (int)min((int64_t)RB, B - b0);
        if (LDS) {
            __syncthreads();                                                // the readers of the previous rows are done
            for (int j = threadIdx.x; j < nr * E; j += 256) sw[j] = RN_LD_STREAM(w + b0 * E + j);
            __syncthreads();
        }
        for (int j = threadIdx.x; j < nr * Pv; j += 256) {
            const int r = j / Pv, pv = j - r * Pv;
            if (V4) {
                const tu_i4 q = reinterpret_cast<const tu_i4*>(pos)[pv];
                rn_f4 v;
                if (LDS) {
                    const float* const row = sw + r * E;
                    v = rn_f4{row[q.x], row[q.y], row[q.z], row[q.w]};
                } else {
                    const float* const row = w + (b0 + r) * E;
                    v = rn_f4{row[q.x], row[q.y], row[q.z], row[q.w]};
                }
                if (x) v = v * RN_LD_STREAM(reinterpret_cast<const rn_f4*>(x + b0 * P) + j);
                RN_ST_STREAM(reinterpret_cast<rn_f4*>(out + b0 * P) + j, v);
            } else {
                float v = LDS ? sw[r * E + pos[pv]] : w[(b0 + r) * E + pos[pv]];
                if (x) v *= RN_LD_STREAM(x + b0 * P + j);
                RN_ST_STREAM(out + b0 * P + j, v);
            }
        }
    }
}

static bool tu_elw_args(int64_t B, int E, int P) { return B >= 0 && E >= 0 && P >= 0 && P <= (1 << 24); }

extern "C" int recnow_elem_weight_fwd(const float* w, const int32_t* pos, const float* x, int64_t B, int E, int P, float* out, void* stream) {
    if (!tu_elw_args(B, E, P)) return RECNOW_EINVAL;
    if (B == 0 || P == 0) return RECNOW_OK;
    if (E == 0 || !w || !pos || !out) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = P % 4 == 0 && tu_al16(pos) && tu_al16(out) && (!x || tu_al16(x));
    const bool lds = E <= TU_ELW_LDS;
    int RB = lds ? TU_ELW_LDS / E : 8;
    if (RB > 64) RB = 64;
    int64_t g = (B + RB - 1) / RB;
    if (g > 8192) g = 8192;
    if (v4 && lds) hipLaunchKernelGGL((k_elw_fwd<true, true>), (int)g, 256, 0, st, w, pos, x, B, E, P, RB, out);
    else if (v4) hipLaunchKernelGGL((k_elw_fwd<true, false>), (int)g, 256, 0, st, w, pos, x, B, E, P, RB, out);
    else if (lds) hipLaunchKernelGGL((k_elw_fwd<false, true>), (int)g, 256, 0, st, w, pos, x, B, E, P, RB, out);
    else hipLaunchKernelGGL((k_elw_fwd<false, false>), (int)g, 256, 0, st, w, pos, x, B, E, P, RB, out);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// dw[b][e] = sum over the positions p of embedding e, in ascending p, of g[b][p] (* x[b][p]): off (E + 1) / idx (P) are the inverse of pos as a CSR
// table.  One thread owns one (b, e): no atomics.  dx[b][p] = g[b][p] * w[b][pos[p]] in the same launch (apply only), by the same workgroup on the
// same RB rows, so the second read of g comes from the cache.
template <bool V4>
__global__ void __launch_bounds__(256)
k_elw_bwd(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ w, const int32_t* __restrict__ pos,
          const int32_t* __restrict__ off, const int32_t* __restrict__ idx, int64_t B, int E, int P, int RB, float* __restrict__ dw, float* __restrict__ dx) {
    const int Pv = V4 ? P / 4 : P;
    for (int64_t b0 = (int64_t)blockIdx.x * RB; b0 < B; b0 += (int64_t)gridDim.x * RB) {
        const int nr = (int)min((int64_t)RB, B - b0);
        if (dw) {
            for (int j = threadIdx.x; j < nr * E; j += 256) {
                const int r = j / E, e = j - r * E;
                const float* const gr = g + (b0 + r) * P;
                const float* const xr = x ? x + (b0 + r) * P : nullptr;
                float s = 0.f;
                for (int k = off[e]; k < off[e + 1]; ++k) {
                    const int p = idx[k];
                    s += xr ? gr[p] * xr[p] : gr[p];
                }
                dw[b0 * E + j] = s;
            }
        }
        if (dx) {
            for (int j = threadIdx.x; j < nr * Pv; j += 256) {
                const int r = j / Pv, pv = j - r * Pv;
                const float* const row = w + (b0 + r) * E;
                if (V4) {
                    const tu_i4 q = reinterpret_cast<const tu_i4*>(pos)[pv];
                    const rn_f4 v = rn_f4{row[q.x], row[q.y], row[q.z], row[q.w]} * reinterpret_cast<const rn_f4*>(g + b0 * P)[j];
                    RN_ST_STREAM(reinterpret_cast<rn_f4*>(dx + b0 * P) + j, v);
                } else {
                    RN_ST_STREAM(dx + b0 * P + j, row[pos[pv]] * g[b0 * P + j]);
                }
            }
        }
    }
}

extern "C" int recnow_elem_weight_bwd(const float* g, const float* x, const float* w, const int32_t* pos, const int32_t* off, const int32_t* idx, int64_t B,
                                      int E, int P, float* dw, float* dx, void* stream) {
    if (!tu_elw_args(B, E, P)) return RECNOW_EINVAL;
    if (B == 0 || (!dw && !dx) || (P == 0 && E == 0)) return RECNOW_OK;
    if ((P > 0 && !g) || (dw && (!off || (P > 0 && !idx))) || (dx && (!w || !pos || E == 0))) return RECNOW_EINVAL;
    if (E > (1 << 24)) return RECNOW_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = P % 4 == 0 && tu_al16(g) && (!dx || (tu_al16(dx) && tu_al16(pos)));
    const int RB = 16;
    int64_t gr = (B + RB - 1) / RB;
    if (gr > 16384) gr = 16384;
    if (v4) hipLaunchKernelGGL(k_elw_bwd<true>, (int)gr, 256, 0, st, g, x, w, pos, off, idx, B, E, P, RB, dw, dx);
    else hipLaunchKernelGGL(k_elw_bwd<false>, (int)gr, 256, 0, st, g, x, w, pos, off, idx, B, E, P, RB, dw, dx);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
