// Shared by the table walks of pairwise_table.hip (BPR), pairwise_kind.hip (hinge, squared hinge, margin-logistic) and pairwise_lambda.hip: the class id kept in
// Member.valid, the K x K weight table in LDS and the direction weights of one candidate.  The packing, flag and finalize kernels stay in
// pairwise_table.hip; pairwise_kind.hip launches them through the two host helpers declared at the end.
#pragma once
#include "common.hpp"
#include "pairwise_walk.hpp"

#define PT_MAXV 16
#define PT_BAD 256
#define PT_CLS(v) (((v) >> 1) & 15)

// tw[0..256): W reduced to "> 0 else 0", row-major with a stride of 16; tw[256..512): its transpose.  The caller synchronises.
__device__ __forceinline__ void pt_load_table(const float* __restrict__ W, int nv, float* tw) {
    for (int i = threadIdx.x; i < PT_MAXV * PT_MAXV; i += blockDim.x) {
        const int a = i >> 4, b = i & 15;
        float w = (a < nv && b < nv) ? W[a * nv + b] : 0.f;
        w = w > 0.f ? w : 0.f;                                                     // zero, negative and NaN drop the pair; +inf keeps it
        tw[i] = w;
        tw[PT_MAXV * PT_MAXV + ((b << 4) | a)] = w;
    }
}

// Weights of the two directions of one candidate: wf of (me, o), wb of (o, me); 0 where that direction is no pair.  trow / tcol: row
// class(me) of the table and of its transpose.  The wrong-order rule ANDs in per direction (reference :197-203).
template <int WRONG>
__device__ __forceinline__ void pt_dirs(const Member& me, const Member& o, bool other, const float* trow, const float* tcol, float& wf, float& wb) {
    const int oc = PT_CLS(o.valid);
    const bool both = other && ((me.valid & o.valid & 1) != 0);
    bool okf = both, okb = both;
    if (WRONG) {
        okf = okf && (me.score < o.score);
        okb = okb && (o.score < me.score);
    }
    const float f = trow[oc], b = tcol[oc];
    wf = okf ? f : 0.f;
    wb = okb ? b : 0.f;
}

// the unknown-label flag lives in the spare member record mem[B] of the pairwise workspace
static inline unsigned* pt_bad_flag(const PairWs& pw, int64_t B) { return reinterpret_cast<unsigned*>(pw.mem + B); }

// k_pt_pack + k_pt_flag: members with class ids into pw.mem, the unknown-label flag raised or cleared (no counter is touched)
int rn_pt_pack_members(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, int64_t B, const float* label_values,
                       int n_values, const PairWs& pw, hipStream_t st);
// k_pt_finalize: the n per-workgroup fp64 loss partials summed in fixed order, divided by P + 1e-10 when reduce_mean
int rn_pt_finalize(const double* part, int n, const int64_t* n_pair, int reduce_mean, float* loss, hipStream_t st);
