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
// What the forward does once the buckets are in LDS lives in hash_embed.hpp, shared with the crossed-id kernels of cross_hash.hip.
#include <vector>
#include "hash_embed.hpp"

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

template <bool VEC>
__global__ void __launch_bounds__(256)
k_hash_embed_fwd(HeFwd p, HeHash hp, HeTables tb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char he_lds[];
    const int nh = hp.num_hash;
    int32_t* bkt = reinterpret_cast<int32_t*>(he_lds);                                   // [nh][HE_TILE]

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
    he_fwd_body<VEC>(p, hp, tb, he_lds, hash_one);
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
    const size_t lds = he_fwd_lds(num_hash, mode, vec);
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
