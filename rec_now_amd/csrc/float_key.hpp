// The order-preserving uint32 image of a float, shared by the entries that sort rows by a float with recnow_group_segments
// (pairwise_auc_sort.hip: by score; listmle.hip: by label, descending through the complement).
#pragma once
#include "common.hpp"

#define RN_FLOAT_KEY_NAN 0xffffffffu       // the key of every NaN: above the key of +inf (0xff800000)

// a < b <=> key(a) < key(b), -0.0 and +0.0 share a key, every NaN has the one largest key
__device__ __forceinline__ uint32_t rn_float_key(float v) {
    if (v != v) return RN_FLOAT_KEY_NAN;
    if (v == 0.f) return 0x80000000u;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
