// Shared by the pair walks of pairwise.hip, pairwise_table.hip, pairwise_kind.hip and pairwise_lambda.hip: the 16-byte member record of a sorted row, the LDS
// staging of a workgroup's member range, the walk loops, the layout of the pairwise workspace (recnow_pairwise_workspace_bytes) and, at the end, the pair terms
// of the kinds other than BPR (pk_f, pk_term, pk_dirs).
#pragma once
#include "common.hpp"

struct __attribute__((aligned(16))) Member {   // one sorted row
    float label;
    float score;
    int32_t row;      // original row index
    int32_t valid;    // sample mask (1 = takes part)
};

struct __attribute__((aligned(8))) PairAux {   // beside a member, for the NDCG pair weight (pairwise_lambda.hip)
    float discount;   // D(position of the row in its list by score); 0 for a row that does not take part
    float gain;       // G(label)
};

__device__ __forceinline__ Member load_member(const float* __restrict__ scores, const float* __restrict__ labels,
                                              const uint8_t* __restrict__ mask, const int32_t* __restrict__ order, int64_t k) {
    Member m;
    m.row = order[k];
    m.label = labels[m.row];
    m.score = scores[m.row];
    m.valid = mask ? (mask[m.row] != 0) : 1;
    return m;
}

// Where a walk's member records come from: the packed array (k_pack_members), or -- UNP, the step's loss stage since round 5 -- straight from the loss's
// inputs through the sorted order (three dependent gathers instead of one 16-byte load: used to FILL the LDS stage of a workgroup, which is what the walks
// read; a walk that cannot be staged -- a group of more than 2048 rows -- pays the gathers per member).  Saves the pack launch in front of the walk.
template <bool UNP>
struct MemberSrc {
    const Member* __restrict__ mem;
    const float* __restrict__ scores;
    const float* __restrict__ labels;
    const uint8_t* __restrict__ mask;
    const int32_t* __restrict__ order;
    __device__ __forceinline__ Member operator[](int64_t k) const {
        if constexpr (UNP) return load_member(scores, labels, mask, order, k);
        else return mem[k];
    }
};

// The rows of a workgroup are 256 consecutive sorted positions, so the members they walk form ONE contiguous range of the
// member array: [first row's segment start, last row's segment end).  When it fits (<= PW_STAGE members, 32 KB) it is staged
// in LDS once, coalesced, and every per-row walk reads LDS (a walk is a chain of dependent 16-byte loads otherwise: ~0.4 us
// per member from L1/L2).  Block-uniform decision; oversize ranges (one huge group) fall back to global loads.
#define PW_STAGE 2048
template <typename SRC>
__device__ __forceinline__ bool stage_members(const SRC mem, const int32_t* __restrict__ seg_id,
                                              const int32_t* __restrict__ seg_first, int64_t B, Member* lds, int* base, int rows_per_block = 0) {
    *base = 0;
    const int64_t rpb = rows_per_block > 0 ? rows_per_block : (int64_t)blockDim.x;
    const int64_t k0 = (int64_t)blockIdx.x * rpb;
    if (k0 >= B) return false;
    const int64_t k1 = min(B, k0 + rpb) - 1;
    const int lo = seg_first[seg_id[k0]], hi = seg_first[seg_id[k1] + 1];
    if (hi - lo > PW_STAGE) return false;
    for (int i = threadIdx.x; i < hi - lo; i += blockDim.x) lds[i] = mem[lo + i];
    __syncthreads();
    *base = lo;
    return true;
}
// The second records of the range stage_members has just staged (it returned true), at the same indices.  The caller synchronises.
template <typename T>
__device__ __forceinline__ void stage_beside(const T* __restrict__ aux, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
                                             int64_t B, T* lds) {
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x;
    const int64_t k1 = min(B, k0 + (int64_t)blockDim.x) - 1;
    const int lo = seg_first[seg_id[k0]], hi = seg_first[seg_id[k1] + 1];
    for (int i = threadIdx.x; i < hi - lo; i += blockDim.x) lds[i] = aux[lo + i];
}
// A row's walk over its segment, from LDS when the block's range was staged, else from global memory.  Two loops, so each
// reads through a pointer of a known address space (one generic pointer made every read a flat_load that waits on both
// counters), unrolled by four so that four member reads are in flight instead of one per ~40-instruction body.
#define PW_WALK(IN_LDS, STAGED, SBASE, MEM, S, E, J, O, BODY)            \
    do {                                                                  \
        if (IN_LDS) {                                                     \
            _Pragma("unroll 4") for (int J = (S); J < (E); ++J) {        \
                const Member O = (STAGED)[J - (SBASE)];                   \
                BODY                                                      \
            }                                                             \
        } else {                                                          \
            _Pragma("unroll 4") for (int J = (S); J < (E); ++J) {        \
                const Member O = (MEM)[J];                                \
                BODY                                                      \
            }                                                             \
        }                                                                 \
    } while (0)

// the same two loops with a stride of one wave: lanes of a wave share the walk of ONE row (k_pair_long)
#define PW_WALK_STRIDED(IN_LDS, STAGED, SBASE, MEM, S, E, J, O, BODY)    \
    do {                                                                  \
        if (IN_LDS) {                                                     \
            _Pragma("unroll 4") for (int J = (S); J < (E); J += 64) {    \
                const Member O = (STAGED)[J - (SBASE)];                   \
                BODY                                                      \
            }                                                             \
        } else {                                                          \
            _Pragma("unroll 4") for (int J = (S); J < (E); J += 64) {    \
                const Member O = (MEM)[J];                                \
                BODY                                                      \
            }                                                             \
        }                                                                 \
    } while (0)

// The walks above with a second record per member read beside it (pairwise_lambda.hip: the {discount, gain} record of the NDCG pair weight):
// SAUX is staged like STAGED, AUX is indexed like MEM.  STEP is 1 (a thread per row) or 64 (a wave per row); the members go through the
// loops above, so there is one place where a walk's bounds are written.
#define PW_WALK_AUX(IN_LDS, STAGED, SAUX, SBASE, MEM, AUX, S, E, STEP, J, O, OA, BODY)                \
    do {                                                                                               \
        if ((STEP) == 1) {                                                                             \
            PW_WALK(IN_LDS, STAGED, SBASE, MEM, S, E, J, O, {                                          \
                const PairAux OA = (IN_LDS) ? (SAUX)[J - (SBASE)] : (AUX)[J];                          \
                BODY                                                                                   \
            });                                                                                        \
        } else {                                                                                       \
            PW_WALK_STRIDED(IN_LDS, STAGED, SBASE, MEM, S, E, J, O, {                                  \
                const PairAux OA = (IN_LDS) ? (SAUX)[J - (SBASE)] : (AUX)[J];                          \
                BODY                                                                                   \
            });                                                                                        \
        }                                                                                              \
    } while (0)

// segments longer than this are walked by a wave per row (k_pair_long, k_pair_all; the table walks of pairwise_table.hip, the kind walks of pairwise_kind.hip)
#define PW_LONG 512

#define RN_PW_T 256
#define RN_PW_LPR 4        // lanes per row of the quad form of k_pair_all
#define RN_VEC_BLOCKS 1024

// workspace layout: members (B + 1) | per-block loss partials | long-row counts | long-row loss terms | long-row gradient terms
struct PairWs {
    Member* mem;
    double* part;
    int32_t* long_cnt;
    float *long_la, *long_ga;
};
static inline PairWs pair_ws(void* ws, size_t ws_bytes, int64_t B) {
    RnCarver c(ws, ws_bytes);
    PairWs p;
    p.mem = c.take<Member>(B + 1);
    const int G = 2 * rn_cdiv(B, RN_PW_T / RN_PW_LPR);
    p.part = c.take<double>(G > RN_VEC_BLOCKS ? G : RN_VEC_BLOCKS);
    p.long_cnt = c.take<int32_t>(B);
    p.long_la = c.take<float>(B);
    p.long_ga = c.take<float>(B);
    return p;
}

// ---- the pair terms of pairwise_kind.hip and pairwise_lambda.hip -----------------------------------------------------------------------
// f(u) and f'(u) of one direction.  relu as `u < 0 ? 0 : u`, so that a NaN score of a taking-part row reaches the loss as it does in torch.relu.
template <int KIND>
__device__ __forceinline__ void pk_f(float u, float& f, float& df) {
    if (KIND == RECNOW_PAIR_KIND_HINGE) {
        f = u < 0.f ? 0.f : u;
        df = u > 0.f ? 1.f : 0.f;
    } else if (KIND == RECNOW_PAIR_KIND_SQUARED_HINGE) {
        const float h = u < 0.f ? 0.f : u;
        f = h * h;
        df = h + h;
    } else {                                                                       // hardware exp2 / log2 / rcp, as bpr_term (pairwise.hip)
        const float ex = __builtin_amdgcn_exp2f(-1.44269504f * fabsf(u));          // in (0, 1]: 1 + ex is never denormal
        const float inv = __builtin_amdgcn_rcpf(1.f + ex);
        f = fmaxf(u, 0.f) + 0.69314718f * __builtin_amdgcn_logf(1.f + ex);         // softplus(u)
        df = u >= 0.f ? inv : ex * inv;                                            // sigma(u)
    }
}

// One candidate, both directions.  The loss term of the backward direction is the other row's forward term: only its derivative is used here
// (the compiler drops the unused log2).
template <int KIND>
__device__ __forceinline__ void pk_term(const Member& me, const Member& o, float wf, float wb, float factor, float margin, float& la, float& ga) {
    const float d = factor * (me.score - o.score);
    float ff, dff, fb, dfb;
    pk_f<KIND>(margin - d, ff, dff);
    pk_f<KIND>(margin + d, fb, dfb);
    la += wf > 0.f ? wf * ff : 0.f;
    ga += (wb > 0.f ? wb * dfb : 0.f) - (wf > 0.f ? wf * dff : 0.f);
}

// Direction weights of one candidate under the default rule label_i > label_j (weight 1); Member.valid is 0 / 1 here.
template <int WRONG>
__device__ __forceinline__ void pk_dirs(const Member& me, const Member& o, bool other, float& wf, float& wb) {
    const bool both = other && ((me.valid & o.valid & 1) != 0);
    bool okf = both && (me.label > o.label), okb = both && (o.label > me.label);
    if (WRONG) {
        okf = okf && (me.score < o.score);
        okb = okb && (o.score < me.score);
    }
    wf = okf ? 1.f : 0.f;
    wb = okb ? 1.f : 0.f;
}
