// The two string hashes behind keras.layers.Hashing, for host and device from one source (MultiHashLayer / FastMultiHashLayer):
//   salt = None      FarmHash Fingerprint64 (farmhashna::Hash64) of the bytes              -- lengths 0..32 here
//   salt = (k0, k1)  SipHash-2-4 with the 128-bit key (k0, k1)                               -- any length
// and bucket = hash % num_bins as an unsigned 64-bit remainder (the plain `%`: exact for every num_bins in 1..2^63).
// An integer id is hashed as its decimal text ("%lld": minus sign, no padding), at most 20 bytes.  The text never exists as a byte
// array: it is built straight into little-endian 64-bit words (byte p of the text is bits 8 (p % 8) of word p / 8, zero padded), the
// form both hashes fetch from; RnText holds four such words, enough for the 32 bytes Fingerprint64 is implemented for.
// Everything is plain 64-bit integer C++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ __forceinline__
#else
#define RN_HD inline
#endif

#define RN_HASH_MAX_FP_LEN 32          // Fingerprint64: the 0..16 and 17..32 byte branches
#define RN_HASH_MAX_NUM_HASH 16        // hash functions per layer (kernel argument arrays)

struct RnText {
    uint64_t w0, w1, w2, w3;
    int len;
};

RN_HD uint64_t rn_rotr64(uint64_t v, int s) { return (v >> s) | (v << (64 - s)); }      // 0 < s < 64
RN_HD uint64_t rn_rotl64(uint64_t v, int s) { return (v << s) | (v >> (64 - s)); }

// word i of the text (selects, so that the four words stay in registers on the device)
RN_HD uint64_t rn_text_word(const RnText& t, int i) { return i == 0 ? t.w0 : i == 1 ? t.w1 : i == 2 ? t.w2 : i == 3 ? t.w3 : 0ull; }
// the 8 bytes at byte offset `off` (0 <= off <= 24) as a little-endian word; bytes past the text read as zero
RN_HD uint64_t rn_text_fetch64(const RnText& t, int off) {
    const int i = off >> 3, r = (off & 7) * 8;
    const uint64_t lo = rn_text_word(t, i), hi = rn_text_word(t, i + 1);
    return r == 0 ? lo : (lo >> r) | (hi << (64 - r));
}
RN_HD uint32_t rn_text_fetch32(const RnText& t, int off) { return (uint32_t)rn_text_fetch64(t, off); }
RN_HD uint32_t rn_text_byte(const RnText& t, int p) { return (uint32_t)(rn_text_word(t, p >> 3) >> ((p & 7) * 8)) & 0xffu; }
RN_HD void rn_text_or(RnText& t, int p, uint64_t byte) {
    const uint64_t v = byte << ((p & 7) * 8);
    const int i = p >> 3;
    t.w0 |= i == 0 ? v : 0ull;
    t.w1 |= i == 1 ? v : 0ull;
    t.w2 |= i == 2 ? v : 0ull;
    t.w3 |= i == 3 ? v : 0ull;
}

// ---- integer -> decimal text ---------------------------------------------------------------------------------------------------
RN_HD int rn_digits_u32(uint32_t v) {
    return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7
         : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
// writes the `nd` low decimal digits of v (zero filled) so that the last one lands on byte position `last`
RN_HD void rn_put_digits(RnText& t, uint32_t v, int nd, int last) {
    for (int k = 0; k < nd; ++k) {
        const uint32_t q = v / 10u;
        rn_text_or(t, last - k, (uint64_t)(0x30u + (v - q * 10u)));
        v = q;
    }
}
RN_HD RnText rn_int_text(int64_t id) {
    RnText t;
    t.w0 = t.w1 = t.w2 = t.w3 = 0ull;
    const int neg = id < 0 ? 1 : 0;
    const uint64_t u = neg ? 0ull - (uint64_t)id : (uint64_t)id;      // |INT64_MIN| = 2^63 fits
    if (neg) t.w0 = 0x2dull;                                          // '-'
    if (u < 1000000000ull) {                                          // the usual case: no 64-bit division at all
        const int nd = rn_digits_u32((uint32_t)u);
        t.len = neg + nd;
        rn_put_digits(t, (uint32_t)u, nd, t.len - 1);
        return t;
    }
    // three pieces of at most nine digits: u = (hi * 10^9 + mid) * 10^9 + lo
    const uint64_t q = u / 1000000000ull;
    const uint32_t lo = (uint32_t)(u - q * 1000000000ull);
    const uint32_t hi = (uint32_t)(q / 1000000000ull), mid = (uint32_t)(q - (uint64_t)hi * 1000000000ull);
    if (hi == 0u) {
        const int nd = rn_digits_u32(mid);
        t.len = neg + nd + 9;
        rn_put_digits(t, mid, nd, neg + nd - 1);
    } else {
        const int nd = rn_digits_u32(hi);                             // hi <= 18
        t.len = neg + nd + 18;
        rn_put_digits(t, hi, nd, neg + nd - 1);
        rn_put_digits(t, mid, 9, neg + nd + 8);
    }
    rn_put_digits(t, lo, 9, t.len - 1);
    return t;
}

// ---- SipHash-2-4 ---------------------------------------------------------------------------------------------------------------
struct RnSip {
    uint64_t v0, v1, v2, v3;
};
RN_HD void rn_sip_round(RnSip& s) {
    s.v0 += s.v1; s.v1 = rn_rotl64(s.v1, 13); s.v1 ^= s.v0; s.v0 = rn_rotl64(s.v0, 32);
    s.v2 += s.v3; s.v3 = rn_rotl64(s.v3, 16); s.v3 ^= s.v2;
    s.v0 += s.v3; s.v3 = rn_rotl64(s.v3, 21); s.v3 ^= s.v0;
    s.v2 += s.v1; s.v1 = rn_rotl64(s.v1, 17); s.v1 ^= s.v2; s.v2 = rn_rotl64(s.v2, 32);
}
RN_HD RnSip rn_sip_init(uint64_t k0, uint64_t k1) {
    RnSip s;
    s.v0 = k0 ^ 0x736f6d6570736575ull;
    s.v1 = k1 ^ 0x646f72616e646f6dull;
    s.v2 = k0 ^ 0x6c7967656e657261ull;
    s.v3 = k1 ^ 0x7465646279746573ull;
    return s;
}
RN_HD void rn_sip_block(RnSip& s, uint64_t m) {
    s.v3 ^= m;
    rn_sip_round(s);
    rn_sip_round(s);
    s.v0 ^= m;
}
// `tail`: the len % 8 bytes after the last whole block, zero padded
RN_HD uint64_t rn_sip_finish(RnSip& s, uint64_t tail, uint64_t len) {
    rn_sip_block(s, tail | (len << 56));
    s.v2 ^= 0xffull;
    rn_sip_round(s);
    rn_sip_round(s);
    rn_sip_round(s);
    rn_sip_round(s);
    return s.v0 ^ s.v1 ^ s.v2 ^ s.v3;
}
// any length, from zero-padded little-endian words (len / 8 + 1 of them are read)
RN_HD uint64_t rn_siphash24_words(uint64_t k0, uint64_t k1, const uint64_t* w, uint64_t len) {
    RnSip s = rn_sip_init(k0, k1);
    const uint64_t nb = len >> 3;
    for (uint64_t i = 0; i < nb; ++i) rn_sip_block(s, w[i]);
    return rn_sip_finish(s, w[nb], len);
}
// a text of at most 31 bytes, words in registers
RN_HD uint64_t rn_siphash24_text(uint64_t k0, uint64_t k1, const RnText& t) {
    RnSip s = rn_sip_init(k0, k1);
    const int nb = t.len >> 3;
    if (nb > 0) rn_sip_block(s, t.w0);
    if (nb > 1) rn_sip_block(s, t.w1);
    if (nb > 2) rn_sip_block(s, t.w2);
    return rn_sip_finish(s, rn_text_word(t, nb), (uint64_t)t.len);
}

// ---- FarmHash Fingerprint64 (farmhashna::Hash64), lengths 0..32 ------------------------------------------------------------------
#define RN_FARM_K0 0xc3a5c85c97cb3127ull
#define RN_FARM_K1 0xb492b66fbe98f273ull
#define RN_FARM_K2 0x9ae16a3b2f90404full
RN_HD uint64_t rn_farm_len16(uint64_t u, uint64_t v, uint64_t mul) {
    uint64_t a = (u ^ v) * mul;
    a ^= a >> 47;
    uint64_t b = (v ^ a) * mul;
    b ^= b >> 47;
    return b * mul;
}
// t.len <= RN_HASH_MAX_FP_LEN (the caller checks)
RN_HD uint64_t rn_fingerprint64_text(const RnText& t) {
    const int len = t.len;
    const uint64_t mul = RN_FARM_K2 + (uint64_t)len * 2ull;
    if (len > 16) {
        const uint64_t a = rn_text_fetch64(t, 0) * RN_FARM_K1, b = rn_text_fetch64(t, 8);
        const uint64_t c = rn_text_fetch64(t, len - 8) * mul, d = rn_text_fetch64(t, len - 16) * RN_FARM_K2;
        return rn_farm_len16(rn_rotr64(a + b, 43) + rn_rotr64(c, 30) + d, a + rn_rotr64(b + RN_FARM_K2, 18) + c, mul);
    }
    if (len >= 8) {
        const uint64_t a = rn_text_fetch64(t, 0) + RN_FARM_K2, b = rn_text_fetch64(t, len - 8);
        const uint64_t c = rn_rotr64(b, 37) * mul + a, d = (rn_rotr64(a, 25) + b) * mul;
        return rn_farm_len16(c, d, mul);
    }
    if (len >= 4) {
        const uint64_t a = rn_text_fetch32(t, 0);
        return rn_farm_len16((uint64_t)len + (a << 3), rn_text_fetch32(t, len - 4), mul);
    }
    if (len > 0) {
        const uint32_t a = rn_text_byte(t, 0), b = rn_text_byte(t, len >> 1), c = rn_text_byte(t, len - 1);
        const uint32_t y = a + (b << 8), z = (uint32_t)len + (c << 2);
        const uint64_t m = ((uint64_t)y * RN_FARM_K2) ^ ((uint64_t)z * RN_FARM_K0);
        return (m ^ (m >> 47)) * RN_FARM_K2;
    }
    return RN_FARM_K2;
}

// bucket of one text under hash function h of a layer: `unsalted` selects Fingerprint64, else SipHash keyed (salt, salt)
RN_HD int64_t rn_hash_bucket_text(const RnText& t, int unsalted, uint64_t salt, uint64_t num_bins) {
    const uint64_t h = unsalted ? rn_fingerprint64_text(t) : rn_siphash24_text(salt, salt, t);
    return (int64_t)(h % num_bins);
}

// ---- crossed ids (CartesianProductLayer feeding the hash layers) ------------------------------------------------------------------------
// The text of one element of a cross, "a-b-c", is composed out of rn_int_text pieces and the separator into zero-padded little-endian words
// that the caller owns: RN_CROSS_WORDS of them, the 12 of the longest text plus 3, since an append stores the four words from the one it
// starts in.  The word a piece lands in is a run-time number, so on the device the storage is the lane's own slice of LDS (a per-lane
// register array indexed that way would live in scratch memory); on the host it is a local array.
#include "../../include/recnow.h"
#define RN_CROSS_WORDS (RECNOW_CROSS_MAX_TEXT / 8 + 3)

// the 8 bytes at byte offset `off` (0 <= off <= 96)
RN_HD uint64_t rn_words_fetch64(const uint64_t* w, int off) {
    const int i = off >> 3, r = (off & 7) * 8;
    const uint64_t lo = w[i];
    return r == 0 ? lo : (lo >> r) | (w[i + 1] << (64 - r));
}
// appends the `plen` <= 24 bytes held in x0, x1, x2 (zero padded) at byte `len`; words past the piece are left zero
RN_HD void rn_cross_append(uint64_t* w, int& len, uint64_t x0, uint64_t x1, uint64_t x2, int plen) {
    const int i = len >> 3, r = (len & 7) * 8;
    w[i] |= x0 << r;
    w[i + 1] = r ? (x0 >> (64 - r)) | (x1 << r) : x1;
    w[i + 2] = r ? (x1 >> (64 - r)) | (x2 << r) : x2;
    w[i + 3] = r ? x2 >> (64 - r) : 0ull;
    len += plen;
}
RN_HD int64_t rn_cross_load(const recnow_cross_desc& d, int k, int64_t b, uint32_t j) {
    const int64_t at = (d.batch1[k] ? 0 : b * (int64_t)d.len[k]) + (int64_t)j;
    return d.dtype[k] == RECNOW_KEY_I32 ? (int64_t)((const int32_t*)d.ids[k])[at] : ((const int64_t*)d.ids[k])[at];
}
// the text of element (b, j), j < P row-major with the last input fastest; returns its length (<= the worst case the entry points check)
RN_HD int rn_cross_compose(const recnow_cross_desc& d, int64_t b, uint32_t j, uint64_t* w) {
    uint32_t jk[RECNOW_CROSS_MAX_INPUTS];
#pragma unroll
    for (int k = RECNOW_CROSS_MAX_INPUTS - 1; k >= 0; --k) {
        jk[k] = 0u;
        if (k < d.n_inputs) {
            const uint32_t L = (uint32_t)d.len[k], q = j / L;
            jk[k] = j - q * L;
            j = q;
        }
    }
    for (int k = 0; k < RN_CROSS_WORDS; ++k) w[k] = 0ull;
    int len = 0;
#pragma unroll
    for (int k = 0; k < RECNOW_CROSS_MAX_INPUTS; ++k)
        if (k < d.n_inputs) {
            if (k > 0 && d.sep_len > 0) rn_cross_append(w, len, (uint64_t)d.sep_word, 0ull, 0ull, d.sep_len);
            const RnText t = rn_int_text(rn_cross_load(d, k, b, jk[k]));
            rn_cross_append(w, len, t.w0, t.w1, t.w2, t.len);
        }
    return len;
}

// Does the reference's regular expression of some input's pattern match the joined text?  For input i with the literals s_a the expression is
// ^.*SEP ... (s_a|s_b|..) ... SEP.*$ with the group in position i of n, so the text T matches iff for some literal s and position p
//   T[p : p + |s|] == s,   T[: p] in (.*SEP){i},   T[p + |s| :] in (SEP.*){n - 1 - i}.
// T[: p] is in (.*SEP){i}, i > 0, iff it ends with SEP and what is before that holds i - 1 non-overlapping SEPs, that is iff it reaches at
// least to e_{i-1}, the end of the (i - 1)-th SEP found greedily from the left (the shortest prefix that holds so many); symmetrically with
// b_k from the right.  This is the expression's own match, not a comparison per field: "5--1" matches ^.*-(1)$.
RN_HD bool rn_cross_sep_at(const uint64_t* w, int len, int p, uint32_t sep_word, int sl) {
    if (p < 0 || p + sl > len) return false;
    if (sl == 0) return true;
    const uint32_t mask = sl >= 4 ? 0xffffffffu : (1u << (8 * sl)) - 1u;
    return ((uint32_t)rn_words_fetch64(w, p) & mask) == sep_word;
}
RN_HD bool rn_cross_lit_at(const uint64_t* w, int p, const uint64_t* lit, int n) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < RECNOW_CROSS_MAX_LIT / 8; ++k) {
        const int nb = n - 8 * k;
        if (nb > 0) {
            const uint64_t mask = nb >= 8 ? ~0ull : (1ull << (8 * nb)) - 1ull;
            eq = eq && (rn_words_fetch64(w, p + 8 * k) & mask) == lit[k];
        }
    }
    return eq;
}
RN_HD bool rn_cross_match(const recnow_cross_desc& d, const uint64_t* w, int len) {
    const int n = d.n_inputs, sl = d.sep_len, never = 1 << 20;
    const uint32_t sep = d.sep_word;
    // e1, e2: ends of the first and second SEP from the left; b1, b2: starts of the last and the last but one from the right
    int e1 = sl ? never : 0, e2 = e1, b1 = sl ? -never : len, b2 = b1;
    if (sl) {
        int k = 0;
        for (int p = 0; p + sl <= len && k < 2;) {
            if (rn_cross_sep_at(w, len, p, sep, sl)) {
                p += sl;
                if (k == 0) e1 = p; else e2 = p;
                ++k;
            } else ++p;
        }
        k = 0;
        for (int p = len - sl; p >= 0 && k < 2;) {
            if (rn_cross_sep_at(w, len, p, sep, sl)) {
                if (k == 0) b1 = p; else b2 = p;
                p -= sl;
                ++k;
            } else --p;
        }
    }
    bool hit = false;
#pragma unroll
    for (int i = 0; i < RECNOW_CROSS_MAX_INPUTS; ++i) {
        if (i >= n || d.n_alt[i] <= 0) continue;
        const int after = n - 1 - i;                                                    // fields behind the group
        const int emin = i <= 1 ? 0 : i == 2 ? e1 : e2;                                 // T[: p - sl] must reach e_{i-1}
        const int bmax = after <= 1 ? len : after == 2 ? b1 : b2;                       // T[q + sl :] must start by b_{after-1}
        for (int a = 0; a < d.n_alt[i]; ++a) {
            const int L = d.lit_len[i][a];
            const uint64_t* lit = d.lit_words[i][a];
            const int p_lo = i == 0 ? 0 : emin + sl, p_hi = i == 0 ? 0 : len - L;
            for (int p = p_lo; p <= p_hi && p + L <= len; ++p) {
                if (i > 0 && !rn_cross_sep_at(w, len, p - sl, sep, sl)) continue;
                const int q = p + L;
                if (after == 0 ? q != len : !(rn_cross_sep_at(w, len, q, sep, sl) && q + sl <= bmax)) continue;
                if (rn_cross_lit_at(w, p, lit, L)) hit = true;
            }
        }
    }
    return hit;
}
RN_HD bool rn_cross_has_patterns(const recnow_cross_desc& d) {
    return (d.n_alt[0] | d.n_alt[1] | d.n_alt[2] | d.n_alt[3]) != 0;
}
// bucket of a composed text under hash function h (the caller has checked len <= 32 where `unsalted` can be set)
RN_HD int64_t rn_cross_bucket(const uint64_t* w, int len, int unsalted, uint64_t salt, uint64_t num_bins) {
    uint64_t v;
    if (unsalted) {
        RnText t;
        t.w0 = w[0]; t.w1 = w[1]; t.w2 = w[2]; t.w3 = w[3];
        t.len = len;
        v = rn_fingerprint64_text(t);
    } else {
        v = rn_siphash24_words(salt, salt, w, (uint64_t)len);
    }
    return (int64_t)(v % num_bins);
}
