// Single-slot fetch, sequence embedding and slot pooling of a slot-format batch (slots, ids, weights: each (B, C)):
//   rec_now/rec_block/embedding_util.py:531-584  fetch_single_slot      -> k_slot_fetch (+ k_slot_max_count for ncols=None)
//   rec_now/rec_block/embedding_util.py:327-416  embedding_single_slot  -> k_slot_embed_fwd
//   rec_now/rec_block/embedding_util.py:419-489  pool_slots             -> k_slot_pool_fwd / k_slot_pool_bwd
// The reference compacts the batch with boolean_mask, runs tf.unique, gathers and pads the ragged result: several passes over (B, C),
// two data-dependent sizes and an (n_selected, D) temporary.  Here one wave owns one batch row: its lanes read 64 columns of `slots`
// per pass, a 64-bit __ballot of the match plus the count of set bits below the lane gives every selected entry its output position
// (the running base carries across passes, any C), and the wave writes the row's (ncols) outputs -- selected entries, then defaults --
// so every output element is written exactly once and nothing is allocated but the outputs.
// All of it is HBM-bound copy / gather work: no MFMA, no float atomics, vector stores only.
#include "common.hpp"

#define SF_SENTINEL ((int64_t)0x8000000000000000ull)      // EMB_SENTINEL of embed.hip: the sort key of "no table row" when no V is given

// element i of an int32 (wide == 0) or int64 (wide != 0) array; the flag is uniform over the launch
__device__ __forceinline__ int64_t sf_ld(const void* __restrict__ p, int wide, int64_t i) {
    return wide ? reinterpret_cast<const int64_t*>(p)[i] : (int64_t) reinterpret_cast<const int32_t*>(p)[i];
}
// number of set bits of `bal` below this lane = the rank of a selected lane among the selected lanes of the pass
__device__ __forceinline__ int sf_rank(unsigned long long bal) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// max over the rows of the number of entries whose slot is `target` (ncols=None: RaggedTensor.to_tensor's bounding shape)
__global__ void __launch_bounds__(256)
k_slot_max_count(const void* __restrict__ slots, int s_wide, int64_t target, int64_t B, int C, int32_t* __restrict__ max_count) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int best = 0;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < B; b += (int64_t)gridDim.x * nw) {
        int n = 0;
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int cl = c0 + lane;
            const bool m = cl < C && sf_ld(slots, s_wide, b * C + cl) == target;
            n += __popcll(__ballot(m));
        }
        best = max(best, n);
    }
    if (lane == 0 && best > 0) atomicMax(max_count, best);                  // integer maximum: the same in any order
}

extern "C" int recnow_slot_max_count(const void* slots, int slot_dtype, int64_t target, int64_t B, int C, int32_t* max_count, void* stream) {
    if (B < 0 || C < 0 || (slot_dtype != RECNOW_KEY_I32 && slot_dtype != RECNOW_KEY_I64) || !max_count) return RECNOW_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    RN_HIP(hipMemsetAsync(max_count, 0, sizeof(int32_t), st));
    if (B == 0 || C == 0) return RECNOW_OK;
    if (!slots) return RECNOW_EINVAL;
    int64_t g = (B + 3) / 4;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_slot_max_count, (int)g, 256, 0, st, slots, slot_dtype == RECNOW_KEY_I64, target, B, C, max_count);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// Row b of every output = the entries of row b whose slot is `target`, in column order, cut to ncols or filled up with the defaults.
// src[b][j] = the source column of output position j, -1 for a filled-up one.  Every output pointer is optional.
__global__ void __launch_bounds__(256)
k_slot_fetch(const void* __restrict__ slots, int s_wide, int64_t target, const void* __restrict__ ids, int i_wide, const float* __restrict__ weights,
             int64_t B, int C, int ncols, int64_t default_id, float default_weight, void* __restrict__ out_ids, float* __restrict__ out_w,
             uint8_t* __restrict__ mask, int32_t* __restrict__ src) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t* const o64 = reinterpret_cast<int64_t*>(out_ids);
    int32_t* const o32 = reinterpret_cast<int32_t*>(out_ids);
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < B; b += (int64_t)gridDim.x * nw) {
        const int64_t in0 = b * C, out0 = b * ncols;
        int base = 0;                                                       // selected entries before this pass (wave-uniform)
        for (int c0 = 0; c0 < C && base < ncols; c0 += 64) {                // a full row needs no more passes
            const int cl = c0 + lane;
            const bool m = cl < C && sf_ld(slots, s_wide, in0 + cl) == target;
            const unsigned long long bal = __ballot(m);
            const int pos = base + sf_rank(bal);
            if (m && pos < ncols) {
                if (out_ids) {
                    if (i_wide) o64[out0 + pos] = reinterpret_cast<const int64_t*>(ids)[in0 + cl];
                    else o32[out0 + pos] = reinterpret_cast<const int32_t*>(ids)[in0 + cl];
                }
                if (out_w) out_w[out0 + pos] = weights[in0 + cl];
                if (mask) mask[out0 + pos] = 1;
                if (src) src[out0 + pos] = cl;
            }
            base += __popcll(bal);
        }
        for (int j = min(base, ncols) + lane; j < ncols; j += 64) {
            if (out_ids) {
                if (i_wide) o64[out0 + j] = default_id;
                else o32[out0 + j] = (int32_t)default_id;
            }
            if (out_w) out_w[out0 + j] = default_weight;
            if (mask) mask[out0 + j] = 0;
            if (src) src[out0 + j] = -1;
        }
    }
}

static bool sf_key_dtype(int dt) { return dt == RECNOW_KEY_I32 || dt == RECNOW_KEY_I64; }

extern "C" int recnow_slot_fetch(const void* slots, int slot_dtype, int64_t target, const void* ids, int id_dtype, const float* weights,
                                 int64_t B, int C, int ncols, int64_t default_id, float default_weight, void* out_ids, float* out_weights,
                                 uint8_t* mask, int32_t* src, void* stream) {
    if (B < 0 || C < 0 || ncols < 0 || !sf_key_dtype(slot_dtype)) return RECNOW_EINVAL;
    if ((out_ids && !sf_key_dtype(id_dtype)) || (out_ids && C > 0 && !ids) || (out_weights && C > 0 && !weights)) return RECNOW_EINVAL;
    if (B == 0 || ncols == 0) return RECNOW_OK;
    if (C > 0 && !slots) return RECNOW_EINVAL;
    int64_t g = (B + 3) / 4;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_slot_fetch, (int)g, 256, 0, (hipStream_t)stream, slots, slot_dtype == RECNOW_KEY_I64, target, ids, id_dtype == RECNOW_KEY_I64,
                       weights, B, C, ncols, default_id, default_weight, out_ids, out_weights, mask, src);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// dweights[b][c] = dout[b][j] where src[b][j] == c, 0 elsewhere.  A source column feeds at most one position, so the row is cleared and
// then filled by the same wave: no atomics.
__global__ void __launch_bounds__(256)
k_slot_fetch_bwd(const int32_t* __restrict__ src, const float* __restrict__ dout, int64_t B, int C, int ncols, float* __restrict__ dweights) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < B; b += (int64_t)gridDim.x * nw) {
        for (int c = lane; c < C; c += 64) dweights[b * C + c] = 0.f;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // the zeros have landed before another lane overwrites one of them
        for (int j = lane; j < ncols; j += 64) {
            const int s = src[b * ncols + j];
            if (s >= 0 && s < C) dweights[b * C + s] = dout[b * ncols + j];
        }
    }
}

extern "C" int recnow_slot_fetch_bwd(const int32_t* src, const float* dout, int64_t B, int C, int ncols, float* dweights, void* stream) {
    if (B < 0 || C < 0 || ncols < 0) return RECNOW_EINVAL;
    if (B == 0 || C == 0) return RECNOW_OK;
    if (!dweights || (ncols > 0 && (!src || !dout))) return RECNOW_EINVAL;
    int64_t g = (B + 3) / 4;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_slot_fetch_bwd, (int)g, 256, 0, (hipStream_t)stream, src, dout, B, C, ncols, dweights);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// The selection of k_slot_fetch fused with the gather: out[b][j][:] = table[rows[b][c_j]][:] for the j-th selected column c_j of row b, zero rows
// behind the last one.  The rows of the selected entries of a pass are compacted into lanes 0 .. n-1 with ONE permute (selected lanes go to
// their rank, the others behind them: a bijection), then a group of GS lanes copies one table row per step -- GS = the number of 16-byte
// (V4) or 4-byte pieces of a row rounded up to a power of two, so at D = 8 a wave moves 32 rows per step and at D = 32 eight.
// key / key32 (optional): per output position the table row, or pad_key for filled-up positions and rows outside [0, V) -- the sort key of the
// table gradient (recnow_embed_rows_bwd_direct over the B * ncols positions).
template <bool V4>
__global__ void __launch_bounds__(256)
k_slot_embed_fwd(const float* __restrict__ table, int D, int64_t V, const void* __restrict__ slots, int s_wide, int64_t target,
                 const void* __restrict__ rows, int r_wide, const float* __restrict__ weights, int64_t B, int C, int ncols, float default_weight,
                 float* __restrict__ out, float* __restrict__ out_w, uint8_t* __restrict__ mask, int32_t* __restrict__ src, int64_t* __restrict__ key,
                 int32_t* __restrict__ key32, int64_t pad_key, int GS) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int NV = V4 ? D / 4 : D;                                          // pieces per table row
    const int G = 64 / GS, grp = lane / GS, gl = lane % GS;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < B; b += (int64_t)gridDim.x * nw) {
        const int64_t in0 = b * C, out0 = b * ncols;
        int base = 0;
        for (int c0 = 0; c0 < C && base < ncols; c0 += 64) {
            const int cl = c0 + lane;
            const bool m = cl < C && sf_ld(slots, s_wide, in0 + cl) == target;
            int64_t r = m ? sf_ld(rows, r_wide, in0 + cl) : -1;
            if (r < 0 || r >= V) r = -1;                                    // outside the table: a zero row, as recnow_embed_pool_fwd
            const unsigned long long bal = __ballot(m);
            const int rank = sf_rank(bal), n = __popcll(bal), pos = base + rank;
            if (m && pos < ncols) {
                if (out_w) out_w[out0 + pos] = weights[in0 + cl];
                if (mask) mask[out0 + pos] = 1;
                if (src) src[out0 + pos] = cl;
                if (key) key[out0 + pos] = r >= 0 ? r : pad_key;
                if (key32) key32[out0 + pos] = (int32_t)(r >= 0 ? r : pad_key);
            }
            const int dest = (m ? rank : n + lane - rank) * 4;              // selected lanes first, in order
            const int lo = __builtin_amdgcn_ds_permute(dest, (int)r), hi = __builtin_amdgcn_ds_permute(dest, (int)(r >> 32));
            const int64_t crow = (int64_t)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
            const int take = min(n, ncols - base);                          // entries of this pass that fit (wave-uniform)
            for (int k0 = 0; k0 < take; k0 += G) {
                const int i = k0 + grp;
                const int64_t ri = __shfl(crow, min(i, 63), 64);            // by every lane; used by the groups that have an entry
                if (i < take) {
                    float* const o = out + (out0 + base + i) * (int64_t)D;
                    if (V4) {
                        for (int v = gl; v < NV; v += GS) {
                            const rn_f4 x = ri >= 0 ? *reinterpret_cast<const rn_f4*>(table + ri * (int64_t)D + 4 * v) : rn_f4{0.f, 0.f, 0.f, 0.f};
                            RN_ST_STREAM(reinterpret_cast<rn_f4*>(o + 4 * v), x);
                        }
                    } else {
                        for (int v = gl; v < NV; v += GS) RN_ST_STREAM(o + v, ri >= 0 ? table[ri * (int64_t)D + v] : 0.f);
                    }
                }
            }
            base += n;
        }
        const int first = min(base, ncols);
        for (int j = first + lane; j < ncols; j += 64) {
            if (out_w) out_w[out0 + j] = default_weight;
            if (mask) mask[out0 + j] = 0;
            if (src) src[out0 + j] = -1;
            if (key) key[out0 + j] = pad_key;
            if (key32) key32[out0 + j] = (int32_t)pad_key;
        }
        float* const z = out + (out0 + first) * (int64_t)D;                 // the zero rows are one contiguous range
        const int64_t nz = (int64_t)(ncols - first) * D;
        if (V4) {
            for (int64_t e = 4 * (int64_t)lane; e < nz; e += 256) RN_ST_STREAM(reinterpret_cast<rn_f4*>(z + e), (rn_f4{0.f, 0.f, 0.f, 0.f}));
        } else {
            for (int64_t e = lane; e < nz; e += 64) RN_ST_STREAM(z + e, 0.f);
        }
    }
}

extern "C" int recnow_slot_embed_fwd(const float* table, int D, int64_t V, const void* slots, int slot_dtype, int64_t target, const void* rows,
                                     int row_dtype, const float* weights, int64_t B, int C, int ncols, float default_weight, float* out,
                                     float* out_weights, uint8_t* mask, int32_t* src, int64_t* key, int32_t* key32, int64_t key_limit, void* stream) {
    if (B < 0 || C < 0 || ncols < 0 || D < 1 || V < 0 || !sf_key_dtype(slot_dtype) || !sf_key_dtype(row_dtype)) return RECNOW_EINVAL;
    if (key_limit < 0 || (key32 && (key_limit <= 0 || key_limit >= 0x7fffffffll)) || (out_weights && C > 0 && !weights)) return RECNOW_EINVAL;
    if (B == 0 || ncols == 0) return RECNOW_OK;
    if (!out || (C > 0 && (!slots || !rows)) || (V > 0 && !table)) return RECNOW_EINVAL;
    const int64_t pad_key = key_limit > 0 ? key_limit : SF_SENTINEL;
    const bool v4 = D % 4 == 0 && (((uintptr_t)table | (uintptr_t)out) & 15) == 0;
    const int nv = v4 ? D / 4 : D;
    int GS = 1;
    while (GS < nv && GS < 64) GS <<= 1;
    int64_t g = (B + 3) / 4;
    if (g > 8192) g = 8192;
    hipStream_t st = (hipStream_t)stream;
    const int sw = slot_dtype == RECNOW_KEY_I64, rw = row_dtype == RECNOW_KEY_I64;
    if (v4) hipLaunchKernelGGL(k_slot_embed_fwd<true>, (int)g, 256, 0, st, table, D, V, slots, sw, target, rows, rw, weights, B, C, ncols, default_weight, out, out_weights, mask, src, key, key32, pad_key, GS);
    else hipLaunchKernelGGL(k_slot_embed_fwd<false>, (int)g, 256, 0, st, table, D, V, slots, sw, target, rows, rw, weights, B, C, ncols, default_weight, out, out_weights, mask, src, key, key32, pad_key, GS);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// pool_slots: per row and target t the minimum id, the sum (mean) of the weights and the number of kept entries of the columns whose seg is t.
// Lane l of the wave owns target t0 + l; the row's columns come in 64 at a time and the kept ones are handed to the owners one by one in
// ascending column order (readlane with a wave-uniform index), so a sum always adds in column order: no atomics, no LDS.  More than 64 targets
// walk the row once per 64 (seg comes from the cache).  drop: an entry is dropped when the column immediately before it has the same seg
// (first_occurance_in_row(need_sort=False) applied to the segment ids, as the reference does).
__global__ void __launch_bounds__(256)
k_slot_pool_fwd(const int32_t* __restrict__ seg, const void* __restrict__ ids, int i_wide, const float* __restrict__ weights, int64_t B, int C, int T,
                int mean, int drop, void* __restrict__ out_ids, float* __restrict__ out_w, float* __restrict__ cnt_out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int64_t id_max = i_wide ? INT64_MAX : (int64_t)INT32_MAX;
    for (int64_t b = (int64_t)blockIdx.x * nw + w; b < B; b += (int64_t)gridDim.x * nw) {
        const int64_t in0 = b * C;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            int64_t mn = id_max;
            float sum = 0.f;
            int n = 0;
            int prev = -2;                                                  // seg of the column before this pass (none before column 0)
            for (int c0 = 0; c0 < C; c0 += 64) {
                const int cl = c0 + lane;
                const int s = cl < C ? seg[in0 + cl] : -1;
                int before = __shfl_up(s, 1, 64);
                if (lane == 0) before = prev;
                prev = __shfl(s, 63, 64);
                const bool kept = s >= t0 && s < t0 + 64 && !(drop && before == s);
                int64_t id = 0;
                float wv = 0.f;
                if (kept) {
                    if (ids) id = sf_ld(ids, i_wide, in0 + cl);
                    if (weights) wv = weights[in0 + cl];
                }
                unsigned long long todo = __ballot(kept);
                while (todo) {
                    const int j = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    const int sj = __builtin_amdgcn_readlane(s, j);
                    const int lo = __builtin_amdgcn_readlane((int)id, j), hi = __builtin_amdgcn_readlane((int)(id >> 32), j);
                    const float wj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), j));
                    if (sj == t) {
                        const int64_t idj = (int64_t)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
                        mn = idj < mn ? idj : mn;
                        sum += wj;
                        ++n;
                    }
                }
            }
            if (t < T) {
                const int64_t o = b * T + t;
                if (out_ids) {
                    const int64_t v = (n == 0 || mn == id_max) ? 0 : mn;    // 'min0': tf.where(results != dtype.max, results, 0)
                    if (i_wide) reinterpret_cast<int64_t*>(out_ids)[o] = v;
                    else reinterpret_cast<int32_t*>(out_ids)[o] = (int32_t)v;
                }
                if (out_w) out_w[o] = (mean && n > 0) ? sum / (float)n : sum;
                if (cnt_out) cnt_out[o] = (float)n;
            }
        }
    }
}

extern "C" int recnow_slot_pool_fwd(const int32_t* seg, const void* ids, int id_dtype, const float* weights, int64_t B, int C, int T, int mean,
                                    int drop_duplicate, void* out_ids, float* out_weights, float* cnt, void* stream) {
    if (B < 0 || C < 0 || T < 0) return RECNOW_EINVAL;
    if ((out_ids && !sf_key_dtype(id_dtype)) || (out_ids && C > 0 && !ids) || (out_weights && C > 0 && !weights)) return RECNOW_EINVAL;
    if (B == 0 || T == 0) return RECNOW_OK;
    if (C > 0 && !seg) return RECNOW_EINVAL;
    int64_t g = (B + 3) / 4;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(k_slot_pool_fwd, (int)g, 256, 0, (hipStream_t)stream, seg, out_ids ? ids : nullptr, id_dtype == RECNOW_KEY_I64,
                       out_weights ? weights : nullptr, B, C, T, mean, drop_duplicate, out_ids, out_weights, cnt);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}

// dweights[b][c] = dout[b][seg[b][c]] (/ cnt for 'mean') for kept entries, 0 otherwise
__global__ void __launch_bounds__(256)
k_slot_pool_bwd(const int32_t* __restrict__ seg, const float* __restrict__ cnt, const float* __restrict__ dout, int64_t N, int C, int T, int mean,
                int drop, float* __restrict__ dweights) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / C;
        const int c = (int)(i - b * C);
        const int s = seg[i];
        float g = 0.f;
        if (s >= 0 && !(drop && c > 0 && seg[i - 1] == s)) {
            g = dout[b * T + s];
            if (mean) g /= cnt[b * T + s];                                  // a kept entry makes its count >= 1
        }
        dweights[i] = g;
    }
}

extern "C" int recnow_slot_pool_bwd(const int32_t* seg, const float* cnt, const float* dout, int64_t B, int C, int T, int mean, int drop_duplicate,
                                    float* dweights, void* stream) {
    if (B < 0 || C < 0 || T < 0) return RECNOW_EINVAL;
    const int64_t N = B * C;
    if (N == 0) return RECNOW_OK;
    if (!seg || !dweights || (T > 0 && !dout) || (mean && !cnt)) return RECNOW_EINVAL;
    int64_t g = (N + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(k_slot_pool_bwd, (int)g, 256, 0, (hipStream_t)stream, seg, cnt, dout, N, C, T, mean, drop_duplicate, dweights);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
