// CartesianProductLayer feeding MultiHashLayer / FastMultiHashLayer (rec_now/layers/cartesian_product_layer.py): the reference turns ids into
// strings, joins them as "a-b-c" per element of the (B, L1 * L2 * ..) cross and hashes the strings.  Here the (B, L1 + L2 + ..) input ids are all
// that is read: every lane composes the text of its element on chip (hash64.hpp: rn_cross_compose, into its own slice of LDS), decides the
// invalid patterns on it (rn_cross_match) and hashes it; the text never reaches memory.
//   recnow_cross_text_host / recnow_cross_hash_ids_host : the same code on the host, no GPU call
//   k_cross_text            : the texts themselves, (B, P, W) bytes and (B, P) lengths, for CrossedIds.text_bytes() / .numpy()
//   k_cross_hash_ids        : bucket numbers only (embedding_dim <= 0)
//   k_cross_hash_embed_fwd  : the forward of hash_embed.hpp with the buckets of a tile filled from composed texts; it writes the same keys, so the
//                             backward kernels of hash_embed.hip / embed.hip serve unchanged.  No atomics, fixed summation order.
// LDS: a lane's text takes RN_CROSS_WORDS = 15 words.  15 is odd, so the 64-bit accesses of consecutive lanes fall on different banks.
#include "hash_embed.hpp"

#define CX_LANE_BYTES (RN_CROSS_WORDS * 8)

static int cx_worst_text(const recnow_cross_desc& d) {
    int worst = 0;
    for (int k = 0; k < d.n_inputs; ++k) worst += (d.dtype[k] == RECNOW_KEY_I32 ? 11 : 20) + (k ? d.sep_len : 0);
    return worst;
}

// P (the elements per row) through *P; RECNOW_EINVAL for a descriptor beyond the limits of include/recnow.h
static int cx_check(const recnow_cross_desc& d, int64_t B, int64_t* P) {
    if (B < 0 || d.n_inputs < 1 || d.n_inputs > RECNOW_CROSS_MAX_INPUTS || d.sep_len < 0 || d.sep_len > RECNOW_CROSS_MAX_SEP) return RECNOW_EINVAL;
    if (d.sep_len < 4 && (d.sep_word >> (8 * d.sep_len)) != 0u) return RECNOW_EINVAL;
    if (d.default_len < 0 || d.default_len > RECNOW_CROSS_MAX_TEXT) return RECNOW_EINVAL;
    int64_t prod = 1;
    for (int k = 0; k < d.n_inputs; ++k) {
        if ((d.dtype[k] != RECNOW_KEY_I32 && d.dtype[k] != RECNOW_KEY_I64) || d.len[k] < 0) return RECNOW_EINVAL;
        if (d.n_alt[k] < 0 || d.n_alt[k] > RECNOW_CROSS_MAX_ALTS) return RECNOW_EINVAL;
        for (int a = 0; a < d.n_alt[k]; ++a)
            if (d.lit_len[k][a] < 0 || d.lit_len[k][a] > RECNOW_CROSS_MAX_LIT) return RECNOW_EINVAL;
        prod *= d.len[k];
        if (prod > 0x7fffffffll) return RECNOW_EUNSUPPORTED;
    }
    for (int k = d.n_inputs; k < RECNOW_CROSS_MAX_INPUTS; ++k)
        if (d.n_alt[k] != 0) return RECNOW_EINVAL;
    if (cx_worst_text(d) > RECNOW_CROSS_MAX_TEXT) return RECNOW_EINVAL;
    if (B > 0 && prod > 0)
        for (int k = 0; k < d.n_inputs; ++k)
            if (!d.ids[k]) return RECNOW_EINVAL;
    *P = prod;
    return RECNOW_OK;
}

// the hash entry points: the hash parameters, Fingerprint64's 32 bytes, the default buckets inside the tables
static int cx_check_hash(const recnow_cross_desc& d, int64_t B, int64_t P, const int64_t* salts, int num_hash, int first_unsalted, int64_t num_bins) {
    const int rc = he_check(salts, num_hash, num_bins);
    if (rc) return rc;
    const bool pat = rn_cross_has_patterns(d);
    if (first_unsalted && (cx_worst_text(d) > RN_HASH_MAX_FP_LEN || (pat && d.default_len > RN_HASH_MAX_FP_LEN))) return RECNOW_EUNSUPPORTED;
    if (B > 0 && P > 0x7fffffffll / num_hash / B) return RECNOW_EUNSUPPORTED;
    if (pat)
        for (int h = 0; h < num_hash; ++h)
            if (d.default_buckets[h] < 0 || d.default_buckets[h] >= num_bins) return RECNOW_EINVAL;
    return RECNOW_OK;
}

// ---- one element, host and device ------------------------------------------------------------------------------------------------------
// composes the text of element (b, j) into w; *matched: an invalid pattern matches it
RN_HD int cx_element(const recnow_cross_desc& d, bool pat, int64_t b, uint32_t j, uint64_t* w, bool* matched) {
    const int len = rn_cross_compose(d, b, j, w);
    *matched = pat && rn_cross_match(d, w, len);
    return len;
}
// word k of what element's text reads as after the replacement
RN_HD uint64_t cx_text_word(const recnow_cross_desc& d, const uint64_t* w, bool matched, int k) {
    return k >= RECNOW_CROSS_MAX_TEXT / 8 ? 0ull : matched ? d.default_words[k] : w[k];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
extern "C" int recnow_cross_text_host(recnow_cross_desc d, int64_t B, int W, unsigned char* text, int32_t* lens) {
    int64_t P;
    const int rc = cx_check(d, B, &P);
    if (rc) return rc;
    const bool pat = rn_cross_has_patterns(d);
    if (W < 8 || W % 8 || W < cx_worst_text(d) || (pat && W < d.default_len)) return RECNOW_EINVAL;
    if (B * P == 0) return RECNOW_OK;
    if (!text || !lens) return RECNOW_EINVAL;
    uint64_t w[RN_CROSS_WORDS];
    for (int64_t b = 0; b < B; ++b)
        for (int64_t j = 0; j < P; ++j) {
            bool matched;
            const int len = cx_element(d, pat, b, (uint32_t)j, w, &matched);
            unsigned char* o = text + (b * P + j) * W;
            for (int k = 0; k < W / 8; ++k) {
                const uint64_t v = cx_text_word(d, w, matched, k);
                for (int q = 0; q < 8; ++q) o[8 * k + q] = (unsigned char)(v >> (8 * q));
            }
            lens[b * P + j] = matched ? d.default_len : len;
        }
    return RECNOW_OK;
}

extern "C" int recnow_cross_hash_ids_host(recnow_cross_desc d, int64_t B, const int64_t* salts, int num_hash, int first_unsalted,
                                          int64_t num_bins, int64_t* out) {
    int64_t P;
    int rc = cx_check(d, B, &P);
    if (rc) return rc;
    rc = cx_check_hash(d, B, P, salts, num_hash, first_unsalted, num_bins);
    if (rc) return rc;
    if (B * P == 0) return RECNOW_OK;
    if (!out) return RECNOW_EINVAL;
    const bool pat = rn_cross_has_patterns(d);
    uint64_t w[RN_CROSS_WORDS];
    for (int64_t b = 0; b < B; ++b)
        for (int64_t j = 0; j < P; ++j) {
            bool matched;
            const int len = cx_element(d, pat, b, (uint32_t)j, w, &matched);
            for (int h = 0; h < num_hash; ++h)
                out[(b * P + j) * num_hash + h] = matched ? d.default_buckets[h]
                                                          : rn_cross_bucket(w, len, first_unsalted && h == 0, (uint64_t)salts[h], (uint64_t)num_bins);
        }
    return RECNOW_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_cross_text(recnow_cross_desc d, int64_t n, uint32_t P, int W8, uint64_t* __restrict__ text, int32_t* __restrict__ lens) {
    __shared__ uint64_t s_txt[256 * RN_CROSS_WORDS];
    uint64_t* w = s_txt + threadIdx.x * RN_CROSS_WORDS;
    const bool pat = rn_cross_has_patterns(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / P;
        bool matched;
        const int len = cx_element(d, pat, b, (uint32_t)(i - b * P), w, &matched);
        for (int k = 0; k < W8; ++k) text[i * W8 + k] = cx_text_word(d, w, matched, k);
        lens[i] = matched ? d.default_len : len;
    }
}

extern "C" int recnow_cross_text(recnow_cross_desc d, int64_t B, int W, unsigned char* text, int32_t* lens, void* stream) {
    int64_t P;
    const int rc = cx_check(d, B, &P);
    if (rc) return rc;
    if (W < 8 || W % 8 || W < cx_worst_text(d) || (rn_cross_has_patterns(d) && W < d.default_len)) return RECNOW_EINVAL;
    const int64_t n = B * P;
    if (n == 0) return RECNOW_OK;
    if (!text || !lens || ((uintptr_t)text & 7)) return RECNOW_EINVAL;
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_cross_text, (int)g, 256, 0, (hipStream_t)stream, d, n, (uint32_t)P, W / 8, (uint64_t*)text, lens);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

__global__ void __launch_bounds__(256)
k_cross_hash_ids(recnow_cross_desc d, int64_t n, uint32_t P, HeHash hp, int64_t* __restrict__ out) {
    __shared__ uint64_t s_txt[256 * RN_CROSS_WORDS];
    uint64_t* w = s_txt + threadIdx.x * RN_CROSS_WORDS;
    const bool pat = rn_cross_has_patterns(d);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)i / P;                          // n * num_hash < 2^31
        bool matched;
        const int len = cx_element(d, pat, (int64_t)b, (uint32_t)i - b * P, w, &matched);
        for (int h = 0; h < hp.num_hash; ++h)
            out[i * hp.num_hash + h] = matched ? d.default_buckets[h] : rn_cross_bucket(w, len, hp.first_unsalted && h == 0, hp.salts[h], hp.num_bins);
    }
}

extern "C" int recnow_cross_hash_ids(recnow_cross_desc d, int64_t B, const int64_t* salts_host, int num_hash, int first_unsalted,
                                     int64_t num_bins, int64_t* out, void* stream) {
    int64_t P;
    int rc = cx_check(d, B, &P);
    if (rc) return rc;
    rc = cx_check_hash(d, B, P, salts_host, num_hash, first_unsalted, num_bins);
    if (rc) return rc;
    const int64_t n = B * P;
    if (n == 0) return RECNOW_OK;
    if (!out) return RECNOW_EINVAL;
    HeHash hp;
    he_fill(&hp, salts_host, num_hash, first_unsalted, num_bins);
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_cross_hash_ids, (int)g, 256, 0, (hipStream_t)stream, d, n, (uint32_t)P, hp, out);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// he_lds: what he_fwd_body uses (lds_body bytes, a multiple of 8), then 256 lanes' texts
template <bool VEC>
__global__ void __launch_bounds__(256)
k_cross_hash_embed_fwd(HeFwd p, HeHash hp, HeTables tb, recnow_cross_desc d, int lds_body) {
    extern __shared__ __attribute__((aligned(16))) unsigned char he_lds[];
    const int nh = hp.num_hash;
    int32_t* bkt = reinterpret_cast<int32_t*>(he_lds);                                   // [nh][HE_TILE]
    uint64_t* w = reinterpret_cast<uint64_t*>(he_lds + lds_body) + threadIdx.x * RN_CROSS_WORDS;
    const bool pat = rn_cross_has_patterns(d);
    const uint32_t P = (uint32_t)p.L;

    auto hash_one = [&](int64_t idx, int col) {
        const uint32_t b = (uint32_t)idx / P;                            // B * L * num_hash < 2^31
        bool matched;
        const int len = cx_element(d, pat, (int64_t)b, (uint32_t)idx - b * P, w, &matched);
        for (int h = 0; h < nh; ++h) {
            const int64_t bk = matched ? d.default_buckets[h] : rn_cross_bucket(w, len, hp.first_unsalted && h == 0, hp.salts[h], hp.num_bins);
            bkt[h * HE_TILE + col] = (int32_t)bk;
            const int64_t key = (int64_t)h * (int64_t)hp.num_bins + bk;
            if (p.keys) p.keys[idx * nh + h] = key;
            if (p.keys32) p.keys32[idx * nh + h] = (int32_t)key;
        }
    };
    he_fwd_body<VEC>(p, hp, tb, he_lds, hash_one);
}

extern "C" int recnow_cross_hash_embed_fwd(recnow_cross_desc d, int64_t B, const int64_t* salts_host, int num_hash, int first_unsalted,
                                           int64_t num_bins, const float* const* tables_host, int D, const float* weights, int mode, float* out,
                                           int64_t* keys, int32_t* keys32, void* stream) {
    if (D < 1 || mode < RECNOW_HASH_SUM || mode > RECNOW_HASH_POOLED) return RECNOW_EINVAL;
    int64_t L;
    int rc = cx_check(d, B, &L);
    if (rc) return rc;
    rc = cx_check_hash(d, B, L, salts_host, num_hash, first_unsalted, num_bins);
    if (rc) return rc;
    if (weights && mode != RECNOW_HASH_POOLED) return RECNOW_EINVAL;
    if (num_bins > 0x7fffffffll / num_hash) return RECNOW_EUNSUPPORTED;
    if (B == 0 || (L == 0 && mode != RECNOW_HASH_POOLED)) return RECNOW_OK;
    if (!out || !tables_host) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (L == 0) {                                                        // pooled over nothing
        RN_HIP(hipMemsetAsync(out, 0, (size_t)B * D * sizeof(float), st));
        return RECNOW_OK;
    }
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
    const size_t lds_body = he_fwd_lds(num_hash, mode, vec);             // a multiple of 1024
    const size_t lds = lds_body + (size_t)256 * CX_LANE_BYTES;
    HeFwd p;
    p.ids = nullptr; p.id_dtype = RECNOW_KEY_I64; p.D = D; p.mode = mode; p.B = B; p.L = L; p.weights = weights; p.out = out; p.keys = keys; p.keys32 = keys32;
    if (vec) hipLaunchKernelGGL(k_cross_hash_embed_fwd<true>, (int)g, 256, lds, st, p, hp, tb, d, (int)lds_body);
    else hipLaunchKernelGGL(k_cross_hash_embed_fwd<false>, (int)g, 256, lds, st, p, hp, tb, d, (int)lds_body);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
