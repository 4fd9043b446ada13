// Weight-gradient partials of the per-sample layer kernels (afm.hip, autoint.hip, bilinear.hip): every workgroup (or row chunk) of a backward
// launch sums its samples in fp32 into its own slab of the workspace; rn_part_reduce (partials.hip) adds the slabs in fp64 in a fixed tree.
// Included after common.hpp.
#pragma once

#define RN_PART_BYTES (32u << 20)               // the slabs of one launch at the most

// Slabs of a launch over B samples: one per rows_min samples, at most maxg, inside RN_PART_BYTES, at least one.
static inline int rn_part_groups(int64_t B, int rows_min, int maxg, int64_t slab_floats) {
    int64_t g = (B + rows_min - 1) / rows_min;
    const int64_t cap = (int64_t)RN_PART_BYTES / (4 * slab_floats);
    if (g > cap) g = cap;
    if (g > maxg) g = maxg;
    return g < 1 ? 1 : (int)g;
}

// Where the n reduced elements go: element e belongs to the first segment with e < end[i] and lands at dst[i][e - end[i - 1]].  The ends do
// not decrease; a segment that is not used ends where the one before it does.
struct RnPartDst {
    float* dst[4];
    int64_t end[4];
};

// Element e < n is the sum of the S * G terms  part[chunk * gstride + slot * sstride + e],  term t = (slot t / G, chunk t % G).  64 threads per
// element: thread c adds the terms c, c + 64, .. in fp64 in that order, then one thread adds the 64 sums in lane order -- a fixed tree.
int rn_part_reduce(const float* part, int64_t n, int S, int G, int64_t gstride, int64_t sstride, const RnPartDst& d, hipStream_t st);
