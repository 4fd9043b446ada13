// What the hash + gather kernels share (hash_embed.hip: integer ids and bucket numbers; cross_hash.hip: crossed ids): the kernel arguments,
// the 16-byte / scalar output element, the gather of one id's rows and the body of the forward after the buckets of a tile are in LDS.
// How the buckets of one id get there is the one thing that differs, and is handed in as `hash_one(idx, col)`.
#pragma once
#include "common.hpp"
#include "hash64.hpp"

#define HE_TILE 256

static int he_check(const int64_t* salts, int num_hash, int64_t num_bins) {
    if (num_hash < 1 || num_hash > RN_HASH_MAX_NUM_HASH || num_bins < 1 || !salts) return RECNOW_EINVAL;
    for (int h = 0; h < num_hash; ++h)
        if (salts[h] < 0) return RECNOW_EINVAL;
    return RECNOW_OK;
}

struct HeHash {
    uint64_t salts[RN_HASH_MAX_NUM_HASH];
    int num_hash, first_unsalted;
    uint64_t num_bins;
};
struct HeTables {
    const float* t[RN_HASH_MAX_NUM_HASH];
};

static void he_fill(HeHash* hp, const int64_t* salts, int num_hash, int first_unsalted, int64_t num_bins) {
    for (int h = 0; h < RN_HASH_MAX_NUM_HASH; ++h) hp->salts[h] = h < num_hash ? (uint64_t)salts[h] : 0ull;
    hp->num_hash = num_hash;
    hp->first_unsalted = first_unsalted ? 1 : 0;
    hp->num_bins = (uint64_t)num_bins;
}

__device__ __forceinline__ int64_t he_load_id(const void* __restrict__ ids, int id_dtype, int64_t i) {
    return id_dtype == RECNOW_KEY_I32 ? (int64_t)RN_LD_STREAM((const int32_t*)ids + i) : RN_LD_STREAM((const int64_t*)ids + i);
}

// One element of the output: a float (any D) or 16 bytes (D % 4 == 0, aligned tables and output).
template <bool VEC> struct HeElem;
template <> struct HeElem<false> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T load(const float* row, int u) { return row[u]; }
    static __device__ __forceinline__ void store(float* row, int u, T v) { RN_ST_STREAM(row + u, v); }
};
template <> struct HeElem<true> {
    typedef rn_f4 T;
    static __device__ __forceinline__ T zero() { return rn_f4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ T load(const float* row, int u) { return *reinterpret_cast<const rn_f4*>(row + 4 * u); }      // table rows are re-read: plain loads
    static __device__ __forceinline__ void store(float* row, int u, T v) { RN_ST_STREAM(reinterpret_cast<rn_f4*>(row + 4 * u), v); }
};

// element u of sum_h table_h[bucket_h(i)]: the rows of up to four hash functions in flight, added in hash order
template <bool VEC>
__device__ __forceinline__ typename HeElem<VEC>::T he_sum_rows(const HeTables& tb, const int32_t* bkt, int i, int nh, int D, int u) {
    typedef HeElem<VEC> E;
    typename E::T acc = E::zero();
    for (int h0 = 0; h0 < nh; h0 += 4) {
        typename E::T v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int h = h0 + k;
            const int b = h < nh ? bkt[h * HE_TILE + i] : -1;
            v[k] = b >= 0 ? E::load(tb.t[h < nh ? h : 0] + (int64_t)b * D, u) : E::zero();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (h0 + k < nh) acc = h0 + k == 0 ? v[k] : acc + v[k];
    }
    return acc;
}

struct HeFwd {
    const void* ids;             // (n) int32 / int64 ids, or (n, num_hash) int64 bucket numbers (id_dtype RECNOW_HASH_BUCKETS)
    int id_dtype, D, mode;
    int64_t B, L;                // n = B * L ids
    const float* weights;        // pooled: (B, L) or NULL
    float* out;
    int64_t* keys;               // (n, num_hash) h * num_bins + bucket, or NULL
    int32_t* keys32;             // the same as int32, or NULL
};

// The forward of one workgroup.  he_lds: [nh][HE_TILE] int32 buckets, [HE_TILE] weights, [HE_TILE] partial sums (pooled only).
// hash_one(idx, col) leaves the buckets of id `idx` in column `col` of the bucket tile and writes the keys of the backward.
template <bool VEC, class FILL>
__device__ __forceinline__ void he_fwd_body(const HeFwd& p, const HeHash& hp, const HeTables& tb, unsigned char* he_lds, FILL& hash_one) {
    typedef HeElem<VEC> E;
    const int nh = hp.num_hash, D = p.D, U = VEC ? D / 4 : D;
    int32_t* bkt = reinterpret_cast<int32_t*>(he_lds);                                   // [nh][HE_TILE]
    float* s_w = reinterpret_cast<float*>(he_lds + (size_t)nh * HE_TILE * 4);            // [HE_TILE]
    typename E::T* s_part = reinterpret_cast<typename E::T*>(he_lds + (size_t)(nh + 1) * HE_TILE * 4);      // [HE_TILE], pooled only
    const int tid = threadIdx.x;
    const int64_t n = p.B * p.L;

    if (p.mode != RECNOW_HASH_POOLED) {
        const int64_t ntile = (n + HE_TILE - 1) / HE_TILE;
        const float scale = p.mode == RECNOW_HASH_MEAN ? 1.0f / (float)nh : 1.f;
        for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
            const int64_t i0 = tile * HE_TILE;
            const int cnt = (int)min((int64_t)HE_TILE, n - i0);
            __syncthreads();
            if (tid < cnt) hash_one(i0 + tid, tid);
            __syncthreads();
            if (p.mode == RECNOW_HASH_ROWS) {            // out (n, nh, D): pure copies of table rows
                const int per = nh * U, items = cnt * per;
                for (int j = tid; j < items; j += 256) {
                    const int i = j / per, r = j - i * per, h = r / U, u = r - h * U;
                    const int b = bkt[h * HE_TILE + i];
                    const typename E::T v = b >= 0 ? E::load(tb.t[h] + (int64_t)b * D, u) : E::zero();
                    E::store(p.out + ((i0 + i) * nh + h) * (int64_t)D, u, v);
                }
            } else {                                     // out (n, D)
                const int items = cnt * U;
                for (int j = tid; j < items; j += 256) {
                    const int i = j / U, u = j - i * U;
                    typename E::T v = he_sum_rows<VEC>(tb, bkt, i, nh, D, u);
                    if (p.mode == RECNOW_HASH_MEAN) v = v * scale;
                    E::store(p.out + (i0 + i) * (int64_t)D, u, v);
                }
            }
        }
        return;
    }

    // pooled: out[b] = sum_l w[b][l] * sum_h table_h[bucket_h(ids[b][l])].  RB batch rows per tile, L in pieces of Lc ids; lane
    // (rb, ls, u) adds the ids l = ls, ls + LS, ... of its row, the LS slices are added in slice order at the end.
    const int Lc = (int)min((int64_t)HE_TILE, p.L);
    const int RB = max(1, min(HE_TILE / Lc, HE_TILE / U));
    const int LS = max(1, min(Lc, HE_TILE / (RB * U)));
    const int rb = tid / (LS * U), ls = (tid / U) % LS, u = tid % U;
    const bool lane_on = tid < RB * LS * U;
    const int64_t ntile = (p.B + RB - 1) / RB;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t b0 = tile * RB;
        typename E::T acc = E::zero();
        for (int64_t l0 = 0; l0 < p.L; l0 += Lc) {
            const int pl = (int)min((int64_t)Lc, p.L - l0);              // ids of this piece per row
            __syncthreads();
            if (tid < RB * Lc) {
                const int r = tid / Lc, l = tid - r * Lc;
                if (b0 + r < p.B && l < pl) {
                    const int64_t idx = (b0 + r) * p.L + l0 + l;
                    hash_one(idx, tid);
                    s_w[tid] = p.weights ? RN_LD_STREAM(p.weights + idx) : 1.f;
                }
            }
            __syncthreads();
            if (lane_on && b0 + rb < p.B)
                for (int l = ls; l < pl; l += LS) {
                    const typename E::T s = he_sum_rows<VEC>(tb, bkt, rb * Lc + l, nh, D, u);
                    acc = p.weights ? acc + s * s_w[rb * Lc + l] : acc + s;
                }
        }
        __syncthreads();
        if (lane_on) s_part[tid] = acc;
        __syncthreads();
        if (lane_on && ls == 0 && b0 + rb < p.B) {
            typename E::T s = s_part[tid];
            for (int k = 1; k < LS; ++k) s = s + s_part[tid + k * U];
            E::store(p.out + (b0 + rb) * (int64_t)D, u, s);
        }
    }
}

static bool he_vec(const float* const* tables, int num_hash, int D, const void* a, const void* b) {
    uintptr_t m = (uintptr_t)a | (uintptr_t)b;
    for (int h = 0; h < num_hash; ++h) m |= (uintptr_t)tables[h];
    return D % 4 == 0 && (m & 15) == 0;
}

// bytes of LDS he_fwd_body uses
static size_t he_fwd_lds(int num_hash, int mode, bool vec) {
    return (size_t)(num_hash + 1) * HE_TILE * 4 + (mode == RECNOW_HASH_POOLED ? (size_t)HE_TILE * (vec ? 16 : 4) : 0);
}
