// MultiHashLayer / FastMultiHashLayer (rec_now/layers/multi_hash_layer.py): an id is hashed by num_hash differently salted hash functions
// into num_bins buckets, each bucket selects a row of an embedding table, the rows are summed.  The reference hashes on the host
// (integer ids through tf.strings.as_string) and copies a (B, L, num_hash) index tensor over every step; here the id tensor is all that
// crosses:
//   recnow_hash_ids_host / recnow_hash_bytes_host : the hash functions of hash64.hpp on the host, no GPU call (the CPU suite holds the very
//                             code the kernels compile; string inputs are hashed here and enter the gather kernel as buckets)
//   k_hash_ids              : bucket numbers only (embedding_dim <= 0)
//   k_hash_embed_fwd        : a workgroup takes a tile of 256 ids: one lane hashes one id with all num_hash functions (the salts are
//                             wave-uniform) and leaves the buckets in LDS; then the lanes are dealt out again over the tile's OUTPUT
//                             elements (D / 4 lanes of 16 bytes per row) and gather.  Per-id sum / mean -> (n, D); per-id per-hash rows ->
//                             (n, num_hash, D); pooled -> (B, D) = sum over L of weights * sum over hashes, L split over lane slices that
//                             are added in slice order.  No index tensor and no (B, L, D) temporary; no atomics, fixed summation order.
//   k_hash_embed_bwd_weights: d weights of the pooled mode, the rows re-gathered from the saved keys
// The table gradient is the sorted-segment reduction of embed.hip with key = h * num_bins + bucket (recnow_embed_rows_bwd_direct).
// Integer and gather work, HBM / latency bound; nothing here wants the MFMA pipe.
#include <vector>
#include "common.hpp"
#include "hash64.hpp"

#define HE_TILE 256

static int he_check(const int64_t* salts, int num_hash, int64_t num_bins) {
    if (num_hash < 1 || num_hash > RN_HASH_MAX_NUM_HASH || num_bins < 1 || !salts) return RECNOW_EINVAL;
    for (int h = 0; h < num_hash; ++h)
        if (salts[h] < 0) return RECNOW_EINVAL;
    return RECNOW_OK;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
extern "C" int recnow_hash_ids_host(const void* ids, int id_dtype, int64_t n, const int64_t* salts, int num_hash, int first_unsalted,
                                    int64_t num_bins, int64_t* out) {
    if (n < 0 || (id_dtype != RECNOW_KEY_I32 && id_dtype != RECNOW_KEY_I64)) return RECNOW_EINVAL;
    const int rc = he_check(salts, num_hash, num_bins);
    if (rc) return rc;
    if (n == 0) return RECNOW_OK;
    if (!ids || !out) return RECNOW_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = id_dtype == RECNOW_KEY_I32 ? (int64_t)((const int32_t*)ids)[i] : ((const int64_t*)ids)[i];
        const RnText t = rn_int_text(id);
        for (int h = 0; h < num_hash; ++h)
            out[i * num_hash + h] = rn_hash_bucket_text(t, first_unsalted && h == 0, (uint64_t)salts[h], (uint64_t)num_bins);
    }
    return RECNOW_OK;
}

extern "C" int recnow_hash_bytes_host(const unsigned char* bytes, const int64_t* offsets, int64_t n, const int64_t* salts, int num_hash,
                                      int first_unsalted, int64_t num_bins, int64_t* out) {
    if (n < 0) return RECNOW_EINVAL;
    const int rc = he_check(salts, num_hash, num_bins);
    if (rc) return rc;
    if (n == 0) return RECNOW_OK;
    if (!offsets || !out) return RECNOW_EINVAL;
    std::vector<uint64_t> w;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 0 || (len > 0 && !bytes)) return RECNOW_EINVAL;
        if (first_unsalted && len > RN_HASH_MAX_FP_LEN) return RECNOW_EUNSUPPORTED;      // never a wrong bucket
        w.assign((size_t)(len / 8 + 1 < 4 ? 4 : len / 8 + 1), 0ull);
        for (int64_t p = 0; p < len; ++p) w[(size_t)(p >> 3)] |= (uint64_t)bytes[offsets[i] + p] << ((p & 7) * 8);
        RnText t;
        t.w0 = w[0]; t.w1 = w[1]; t.w2 = w[2]; t.w3 = w[3];
        t.len = (int)(len > RN_HASH_MAX_FP_LEN ? 0 : len);
        for (int h = 0; h < num_hash; ++h) {
            const uint64_t s = (uint64_t)salts[h];
            const uint64_t v = (first_unsalted && h == 0) ? rn_fingerprint64_text(t) : rn_siphash24_words(s, s, w.data(), (uint64_t)len);
            out[i * num_hash + h] = (int64_t)(v % (uint64_t)num_bins);
        }
    }
    return RECNOW_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
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

__global__ void __launch_bounds__(256)
k_hash_ids(const void* __restrict__ ids, int id_dtype, int64_t n, HeHash hp, int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const RnText t = rn_int_text(he_load_id(ids, id_dtype, i));
        for (int h = 0; h < hp.num_hash; ++h)
            out[i * hp.num_hash + h] = rn_hash_bucket_text(t, hp.first_unsalted && h == 0, hp.salts[h], hp.num_bins);
    }
}

extern "C" int recnow_hash_ids(const void* ids, int id_dtype, int64_t n, const int64_t* salts_host, int num_hash, int first_unsalted,
                               int64_t num_bins, int64_t* out, void* stream) {
    if (n < 0 || (id_dtype != RECNOW_KEY_I32 && id_dtype != RECNOW_KEY_I64)) return RECNOW_EINVAL;
    const int rc = he_check(salts_host, num_hash, num_bins);
    if (rc) return rc;
    if (n == 0) return RECNOW_OK;
    if (!ids || !out) return RECNOW_EINVAL;
    HeHash hp;
    he_fill(&hp, salts_host, num_hash, first_unsalted, num_bins);
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_hash_ids, (int)g, 256, 0, (hipStream_t)stream, ids, id_dtype, n, hp, out);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
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

template <bool VEC>
__global__ void __launch_bounds__(256)
k_hash_embed_fwd(HeFwd p, HeHash hp, HeTables tb) {
    typedef HeElem<VEC> E;
    extern __shared__ __attribute__((aligned(16))) unsigned char he_lds[];
    const int nh = hp.num_hash, D = p.D, U = VEC ? D / 4 : D;
    int32_t* bkt = reinterpret_cast<int32_t*>(he_lds);                                   // [nh][HE_TILE]
    float* s_w = reinterpret_cast<float*>(he_lds + (size_t)nh * HE_TILE * 4);            // [HE_TILE]
    typename E::T* s_part = reinterpret_cast<typename E::T*>(he_lds + (size_t)(nh + 1) * HE_TILE * 4);      // [HE_TILE], pooled only
    const int tid = threadIdx.x;
    const int64_t n = p.B * p.L;

    // the buckets of id `idx` into column `col` of the LDS tile (and the keys of the backward)
    auto hash_one = [&](int64_t idx, int col) {
        if (p.id_dtype == RECNOW_HASH_BUCKETS) {
            for (int h = 0; h < nh; ++h) {
                const int64_t b = RN_LD_STREAM((const int64_t*)p.ids + idx * nh + h);
                const bool in = b >= 0 && (uint64_t)b < hp.num_bins;
                bkt[h * HE_TILE + col] = in ? (int32_t)b : -1;
                const int64_t key = in ? (int64_t)h * (int64_t)hp.num_bins + b : -1;
                if (p.keys) p.keys[idx * nh + h] = key;
                if (p.keys32) p.keys32[idx * nh + h] = (int32_t)key;
            }
        } else {
            const RnText t = rn_int_text(he_load_id(p.ids, p.id_dtype, idx));
            for (int h = 0; h < nh; ++h) {
                const int64_t b = rn_hash_bucket_text(t, hp.first_unsalted && h == 0, hp.salts[h], hp.num_bins);
                bkt[h * HE_TILE + col] = (int32_t)b;
                const int64_t key = (int64_t)h * (int64_t)hp.num_bins + b;
                if (p.keys) p.keys[idx * nh + h] = key;
                if (p.keys32) p.keys32[idx * nh + h] = (int32_t)key;
            }
        }
    };

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

extern "C" int recnow_hash_embed_fwd(const void* ids, int id_dtype, int64_t B, int64_t L, const int64_t* salts_host, int num_hash,
                                     int first_unsalted, int64_t num_bins, const float* const* tables_host, int D, const float* weights,
                                     int mode, float* out, int64_t* keys, int32_t* keys32, void* stream) {
    if (B < 0 || L < 0 || D < 1 || mode < RECNOW_HASH_SUM || mode > RECNOW_HASH_POOLED) return RECNOW_EINVAL;
    if (id_dtype != RECNOW_KEY_I32 && id_dtype != RECNOW_KEY_I64 && id_dtype != RECNOW_HASH_BUCKETS) return RECNOW_EINVAL;
    const int rc = he_check(salts_host, num_hash, num_bins);
    if (rc) return rc;
    if (weights && mode != RECNOW_HASH_POOLED) return RECNOW_EINVAL;
    // rows are addressed by a 32-bit bucket, and the sort of the backward by a 32-bit entry index
    if (num_bins > 0x7fffffffll / num_hash || (B > 0 && L > 0x7fffffffll / num_hash / B)) return RECNOW_EUNSUPPORTED;
    if (B == 0 || (L == 0 && mode != RECNOW_HASH_POOLED)) return RECNOW_OK;
    if (!out || !tables_host) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (L == 0) {                                                        // pooled over nothing
        RN_HIP(hipMemsetAsync(out, 0, (size_t)B * D * sizeof(float), st));
        return RECNOW_OK;
    }
    if (!ids) return RECNOW_EINVAL;
    HeHash hp;
    he_fill(&hp, salts_host, num_hash, first_unsalted, num_bins);
    HeTables tb;
    for (int h = 0; h < RN_HASH_MAX_NUM_HASH; ++h) {
        tb.t[h] = h < num_hash ? tables_host[h] : nullptr;
        if (h < num_hash && !tables_host[h]) return RECNOW_EINVAL;
    }
    const bool vec = he_vec(tables_host, num_hash, D, out, nullptr);
    const int U = vec ? D / 4 : D;
    int64_t ntile;
    if (mode == RECNOW_HASH_POOLED) {
        if (U > HE_TILE) return RECNOW_EUNSUPPORTED;
        const int Lc = (int)(L < HE_TILE ? L : HE_TILE);
        int RB = HE_TILE / Lc < HE_TILE / U ? HE_TILE / Lc : HE_TILE / U;
        if (RB < 1) RB = 1;
        ntile = (B + RB - 1) / RB;
    } else {
        ntile = (B * L + HE_TILE - 1) / HE_TILE;
    }
    const int64_t g = ntile < 8192 ? ntile : 8192;
    const size_t lds = (size_t)(num_hash + 1) * HE_TILE * 4 + (mode == RECNOW_HASH_POOLED ? (size_t)HE_TILE * (vec ? 16 : 4) : 0);
    HeFwd p;
    p.ids = ids; p.id_dtype = id_dtype; p.D = D; p.mode = mode; p.B = B; p.L = L; p.weights = weights; p.out = out; p.keys = keys; p.keys32 = keys32;
    if (vec) hipLaunchKernelGGL(k_hash_embed_fwd<true>, (int)g, 256, lds, st, p, hp, tb);
    else hipLaunchKernelGGL(k_hash_embed_fwd<false>, (int)g, 256, lds, st, p, hp, tb);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// dweights[b][l] = <dout[b][:], sum_h table_h[bucket_h(ids[b][l])][:]>, the rows re-gathered from the saved keys (no saved (B, L, D)).
// LPE lanes per id (pow2 >= min(D, 64)).
__global__ void __launch_bounds__(256)
k_hash_embed_bwd_weights(const int64_t* __restrict__ keys, HeTables tb, int nh, int64_t num_bins, int D, const float* __restrict__ dout,
                         int64_t n, int64_t L, int LPE, float* __restrict__ dweights) {
    const int gl = threadIdx.x % LPE;
    const int64_t per = 256 / LPE;
    for (int64_t e0 = (int64_t)blockIdx.x * per; e0 < n; e0 += (int64_t)gridDim.x * per) {
        const int64_t e = e0 + threadIdx.x / LPE;
        float pr = 0.f;
        if (e < n) {
            const float* g = dout + (e / L) * (int64_t)D;
            for (int d = gl; d < D; d += LPE) {
                float s = 0.f;
                for (int h = 0; h < nh; ++h) {
                    const int64_t b = keys[e * nh + h] - (int64_t)h * num_bins;
                    const float v = (b >= 0 && b < num_bins) ? tb.t[h][b * D + d] : 0.f;
                    s = h == 0 ? v : s + v;
                }
                pr += g[d] * s;
            }
        }
        for (int o = LPE >> 1; o > 0; o >>= 1) pr += __shfl_xor(pr, o, 64);
        if (e < n && gl == 0) dweights[e] = pr;
    }
}

extern "C" int recnow_hash_embed_bwd_weights(const int64_t* keys, const float* const* tables_host, int num_hash, int64_t num_bins, int D,
                                             const float* dout, int64_t B, int64_t L, float* dweights, void* stream) {
    if (B < 0 || L < 0 || D < 1 || num_hash < 1 || num_hash > RN_HASH_MAX_NUM_HASH || num_bins < 1) return RECNOW_EINVAL;
    const int64_t n = B * L;
    if (n == 0) return RECNOW_OK;
    if (!keys || !tables_host || !dout || !dweights) return RECNOW_EINVAL;
    HeTables tb;
    for (int h = 0; h < RN_HASH_MAX_NUM_HASH; ++h) {
        tb.t[h] = h < num_hash ? tables_host[h] : nullptr;
        if (h < num_hash && !tables_host[h]) return RECNOW_EINVAL;
    }
    const int LPE = D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
    int64_t g = (n + 256 / LPE - 1) / (256 / LPE);
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(k_hash_embed_bwd_weights, (int)g, 256, 0, (hipStream_t)stream, keys, tb, num_hash, num_bins, D, dout, n, L, LPE, dweights);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
