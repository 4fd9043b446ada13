// Shared by the two routes of the in-batch GAUC (pairwise_auc.hip: the compare-only walk; pairwise_auc_sort.hip: sort and per-class prefix counts): the
// record both routes leave per sorted row, and the two kernels that turn the records into per-list sums and the metric.
//
// The record: int4 {n_i, c_i, t_i, takes part (0 / 1)} at the row's position k in the CALLER's sorted order (`order`, `seg_id`, `seg_first`), [B] of them.
// k_pa_segsum: a workgroup per segment (grid-stride over the segments), 256 threads striding the segment, int64 block sums of n, c, t and the row count;
//   no atomics.  k_pa_metric (one workgroup): the fp64 weighted sum and weight sum in fixed order, their float32 ratio and the int64 number of lists counted.
#pragma once
#include "common.hpp"

static __global__ void __launch_bounds__(256)
k_pa_segsum(const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first, int64_t B, const int4* __restrict__ nct,
            long long* __restrict__ list_n, long long* __restrict__ list_c, long long* __restrict__ list_t, long long* __restrict__ list_rows) {
    __shared__ long long red[16];
    const int nseg = seg_id[B - 1] + 1;
    for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
        const int s = seg_first[g], e = seg_first[g + 1];
        long long n = 0, c = 0, t = 0, r = 0;
        for (int i = s + threadIdx.x; i < e; i += 256) {
            const int4 v = nct[i];
            n += v.x;
            c += v.y;
            t += v.z;
            r += v.w;
        }
        n = block_sum<long long>(n, red);
        c = block_sum<long long>(c, red);
        t = block_sum<long long>(t, red);
        r = block_sum<long long>(r, red);
        if (threadIdx.x == 0) {
            list_n[g] = n;
            list_c[g] = c;
            list_t[g] = t;
            list_rows[g] = r;
        }
    }
}

static __global__ void __launch_bounds__(1024)
k_pa_metric(const int32_t* __restrict__ seg_id, int64_t B, const long long* __restrict__ list_n, const long long* __restrict__ list_c,
            const long long* __restrict__ list_t, const long long* __restrict__ list_rows, int weight_kind, float* __restrict__ auc,
            double* __restrict__ weighted_sum, double* __restrict__ weight_sum, long long* __restrict__ n_lists) {
    __shared__ double red[16];
    __shared__ long long redc[16];
    const int nseg = seg_id[B - 1] + 1;
    double num = 0.0, den = 0.0;
    long long cnt = 0;
    for (int g = threadIdx.x; g < nseg; g += 1024) {                // fixed order per thread, fixed tree
        const long long n = list_n[g];
        if (n > 0) {
            const double a = (double)(2 * list_c[g] + list_t[g]) / (double)(2 * n);
            const double w = weight_kind == RECNOW_AUC_WEIGHT_ROWS ? (double)list_rows[g] : weight_kind == RECNOW_AUC_WEIGHT_PAIRS ? (double)n : 1.0;
            num += w * a;
            den += w;
            cnt += 1;
        }
    }
    num = block_sum<double>(num, red);
    den = block_sum<double>(den, red);
    cnt = block_sum<long long>(cnt, redc);
    if (threadIdx.x == 0) {
        if (auc) *auc = den > 0.0 ? (float)(num / den) : 0.f;
        if (weighted_sum) *weighted_sum = num;
        if (weight_sum) *weight_sum = den;
        if (n_lists) *n_lists = cnt;
    }
}

// The tail of both entries: per-list sums into the caller's arrays (or the workspace's where one is not asked for), then the metric when any of it is.
static inline void pa_launch_sums(const int32_t* seg_id, const int32_t* seg_first, int64_t B, const int4* nct, long long* ln, long long* lc, long long* lt,
                                  long long* lr, int weight_kind, float* auc, double* weighted_sum, double* weight_sum, int64_t* n_lists, hipStream_t st) {
    const int GS = B < 4096 ? (int)B : 4096;                        // a workgroup per segment, grid-stride: there are at most B segments
    hipLaunchKernelGGL(k_pa_segsum, GS, 256, 0, st, seg_id, seg_first, B, nct, ln, lc, lt, lr);
    if (auc || weighted_sum || weight_sum || n_lists)
        hipLaunchKernelGGL(k_pa_metric, 1, 1024, 0, st, seg_id, B, (const long long*)ln, (const long long*)lc, (const long long*)lt,
                           (const long long*)lr, weight_kind, auc, weighted_sum, weight_sum, (long long*)n_lists);
}
