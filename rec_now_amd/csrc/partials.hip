// The fixed fp64 tree over weight-gradient partials (partials.hpp).
#include "common.hpp"
#include "partials.hpp"

// One output element per group of 64 threads (4 per workgroup), grid-stride over the elements.
__global__ void __launch_bounds__(256)
k_part_reduce(const float* __restrict__ part, RnPartDst d, int64_t n, int S, int G, int64_t gstride, int64_t sstride) {
    __shared__ double red[256];
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int nterm = S * G;
    for (int64_t e0 = (int64_t)blockIdx.x * 4; e0 < n; e0 += (int64_t)gridDim.x * 4) {
        const int64_t e = e0 + sub;
        double acc = 0.0;
        if (e < n)
            for (int t = c; t < nterm; t += 64) {
                const int slot = S > 1 ? t / G : 0;
                acc += (double)part[(int64_t)(t - slot * G) * gstride + slot * sstride + e];
            }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (c == 0 && e < n) {
            double tot = 0.0;
            for (int t = 0; t < 64; ++t) tot += red[sub * 64 + t];
            float* o = d.dst[0];
            int64_t first = 0;
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (e >= d.end[i - 1]) { o = d.dst[i]; first = d.end[i - 1]; }
            o[e - first] = (float)tot;
        }
        __syncthreads();
    }
}

int rn_part_reduce(const float* part, int64_t n, int S, int G, int64_t gstride, int64_t sstride, const RnPartDst& d, hipStream_t st) {
    int64_t g = (n + 3) / 4;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(k_part_reduce, (int)g, 256, 0, st, part, d, n, S, G, gstride, sstride);
    RN_LAUNCH_CHECK();
    return RECNOW_OK;
}
