// Shared by the pair walks of pairwise.hip, pairwise_table.hip, pairwise_kind.hip and pairwise_lambda.hip: the 16-byte member record of a sorted row, the LDS
// staging of a workgroup's member range, the walk loops, the two route skeletons every family's kernels are instantiations of (pw_wave_rows: a wave per row of
// a long segment; pw_thread_rows: a thread per row) with the row epilogue of the forward+backward kernels, the layout of the pairwise workspace
// (recnow_pairwise_workspace_bytes) and, at the end, the pair terms of the kinds other than BPR (pk_f, pk_term, pk_dirs).
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
// A row's walk over its segment, from LDS when the block's range was staged, else from global memory.  Two loops, so each
// reads through a pointer of a known address space (one generic pointer made every read a flat_load that waits on both
// counters), unrolled by four so that four member reads are in flight instead of one per ~40-instruction body.
// Bounds of a walk: a row walks [seg_first[g], seg_first[g + 1]) of its own segment; staged reads stay inside the staged range [SBASE, SBASE + PW_STAGE),
// which contains the segment of every row that walks it; unstaged reads stay inside the B member records.
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

// the same two loops with a stride of one wave: lanes of a wave share the walk of ONE row (pw_wave_rows, k_pair_all)
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

// segments longer than this are walked by a wave per row (pw_wave_rows; the long-row workgroups of k_pair_all)
#define PW_LONG 512

#define RN_PW_T 256
#define RN_PW_LPR 4        // lanes per row of the quad form of k_pair_all
#define RN_VEC_BLOCKS 1024
static_assert(RN_PW_T == 256, "pw_thread_rows strides by RN_PW_T; its kernels are compiled for and launched with 256 threads");

// ---- the two route skeletons ---------------------------------------------------------------------------------------------------------------
// Every walk of the four families but the one-call walk (k_pair_all, pairwise.hip) is one of these two functions over a policy P, a small struct
// built in the __global__ wrapper from the kernel's arguments and its __shared__ arrays:
//   void P::once()                            once per workgroup in front of the first stage: the table load, or nothing (the skeleton synchronises)
//   void P::stage(int i, int k)               the second record of sorted position k into slot i of its own LDS stage, or nothing
//   Row  P::begin(me, k, wave)                the accumulators of row k, and what the row keeps for its candidates (wave: called by pw_wave_rows, whose
//                                             rows are parked, not finished)
//   void P::candidate(row, me, o, other, in_lds, i, j)    one candidate: member o of sorted position j (slot i = j - base of the stage when in_lds),
//                                             other = (j != k); a policy with second records reads o's from its stage (in_lds) or from global memory
//   void P::park(row, k, lane)                pw_wave_rows: the wave reduction and the lane-0 stores per sorted position
//   Out  P::finish(row, me, k, is_long)       pw_thread_rows: the row's stores (a long row first fetches what park left); returns the row's block-sum term
struct PwPlain {      // a policy without a table and without second records
    __device__ __forceinline__ void once() const {}
    __device__ __forceinline__ void stage(int, int) const {}
};

// Long segments: a wave per row.  One thread per row makes the time of a call the latency of the longest walk: a 2048-row group (the Zipf-skewed
// batches of SURVEY 8d) is 2048 dependent iterations per lane whatever the rest of the batch looks like.  Rows of segments longer than PW_LONG are
// therefore walked by a whole wave each -- lanes stride over the members (coalesced 16-byte reads), partial sums are joined by the fixed butterfly
// of wave_sum, so results stay bitwise reproducible -- and parked per sorted position for the thread-per-row kernels, which skip the walk of such
// rows.  A workgroup owns 64 consecutive sorted rows; a segment lying strictly inside them is shorter than 64 rows, so only the first and the last
// row's segment can be long, and looking at those two decides block-uniformly whether there is anything to do: batches without long groups pay one
// empty launch.
template <typename P>
__device__ __forceinline__ void pw_wave_rows(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id, const int32_t* __restrict__ seg_first,
                                             int64_t B, Member* staged, const P& p) {
    const int64_t k0 = (int64_t)blockIdx.x * 64;
    if (k0 >= B) return;
    const int64_t kl = min(B, k0 + 64) - 1;
    const int g0 = seg_id[k0], g1 = seg_id[kl];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool first = true;
    for (int phase = 0; phase < 2; ++phase) {                       // only the first and the last row's segment can be long (block-uniform)
        if (phase == 1 && g1 == g0) break;
        const int g = phase == 0 ? g0 : g1;
        const int s = seg_first[g], e = seg_first[g + 1];
        if (e - s <= PW_LONG) continue;
        // members of the segment through LDS when they fit (32 KB): lanes then read consecutive 16-byte records at LDS speed and
        // the walk is bound by its ~25 VALU instructions per candidate; from global memory it was bound by the read latency
        const bool in_lds = e - s <= PW_STAGE;
        __syncthreads();                                            // every wave is done with the previous segment's stage
        if (first) p.once();
        first = false;
        if (in_lds)
            for (int i = threadIdx.x; i < e - s; i += 256) {
                staged[i] = mem[s + i];
                p.stage(i, s + i);
            }
        __syncthreads();
        const int64_t ka = k0 > s ? k0 : (int64_t)s, kb = kl < (int64_t)e - 1 ? kl : (int64_t)e - 1;
        for (int64_t k = ka + w; k <= kb; k += 4) {                 // waves take the segment's rows of this block in turn
            const Member me = mem[k];
            auto row = p.begin(me, k, true);
            PW_WALK_STRIDED(in_lds, staged, s, mem, s + lane, e, j, o, { p.candidate(row, me, o, j != (int)k, in_lds, j - s, j); });
            p.park(row, k, lane);
        }
    }
}

// A thread per row: RN_PW_T consecutive sorted rows per workgroup of RN_PW_T threads, their member range staged when it fits.  One barrier
// covers the table, the second records and the stage.  A row of a long segment walks nothing (is_long: pw_wave_rows has parked its sums).
// Returns the row's term of the kernel's block sum, Out() for a thread beyond B.  Its kernels carry __launch_bounds__(256) and MUST be launched
// with RN_PW_T threads and rn_cdiv(B, RN_PW_T) workgroups, B > 0 (as pw_wave_rows must with 256 threads and rn_cdiv(B, 64) workgroups).
template <typename P>
__device__ __forceinline__ typename P::Out pw_thread_rows(const Member* __restrict__ mem, const int32_t* __restrict__ seg_id,
                                                          const int32_t* __restrict__ seg_first, int64_t B, Member* staged, const P& p) {
    p.once();
    // the block's member range as stage_members (the one-call walk's) forms it, with the second records beside the members; clamped into the
    // batch instead of branched on (the grid has no block beyond B; a branch in front of the first loads costs their latency once more)
    const int64_t k0 = min((int64_t)blockIdx.x * RN_PW_T, B - 1), k1 = min(k0 + RN_PW_T, B) - 1;
    // even lanes look up the first row's segment start, odd lanes the last row's segment end: one vector load per level (as four scalar loads the
    // lookups were waited on one after the other, a load latency more than the parent's in front of every walk)
    const int odd = threadIdx.x & 1;
    const int f = seg_first[seg_id[odd ? k1 : k0] + odd];
    const int sbase = __builtin_amdgcn_readlane(f, 0), n = __builtin_amdgcn_readlane(f, 1) - sbase;
    const bool in_lds = n <= PW_STAGE;
    if (in_lds)
        for (int i = threadIdx.x; i < n; i += RN_PW_T) {
            staged[i] = mem[sbase + i];
            p.stage(i, sbase + i);
        }
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * RN_PW_T + threadIdx.x;
    typename P::Out out = typename P::Out();
    if (k < B) {
        const Member me = mem[k];
        const int g = seg_id[k];
        const int s = seg_first[g], e = seg_first[g + 1];
        const bool is_long = e - s > PW_LONG;
        auto row = p.begin(me, k, false);
        PW_WALK(in_lds, staged, sbase, mem, (is_long ? e : s), e, j, o, { p.candidate(row, me, o, j != (int)k, in_lds, j - sbase, j); });
        out = p.finish(row, me, k, is_long);
    }
    return out;
}

// what park / finish do with a pair count, and with the loss and gradient sums of a forward+backward row
__device__ __forceinline__ void pw_park_count(int cc, int64_t k, int lane, int32_t* __restrict__ long_cnt) {
    cc = wave_sum(cc);
    if (lane == 0) long_cnt[k] = cc;
}
__device__ __forceinline__ void pw_park_sums(float la, float ga, int64_t k, int lane, float* __restrict__ long_la, float* __restrict__ long_ga) {
    la = wave_sum(la);
    ga = wave_sum(ga);
    if (lane == 0) {
        long_la[k] = la;
        long_ga[k] = ga;
    }
}
struct PwCountOut {   // where a counting row leaves its count
    const int32_t* long_cnt;
    int32_t* cnt_row;
    const int32_t* super_id;
    unsigned long long* cnt_super;
    __device__ __forceinline__ long long finish(int cc, const Member& me, int64_t k, bool is_long) const {
        if (is_long) cc = long_cnt[k];
        cnt_row[me.row] = cc;
        if (cc) atomicAdd(&cnt_super[super_id[k]], (unsigned long long)cc);   // integer atomics: order-independent
        return cc;
    }
};
__device__ __forceinline__ void pw_add_pairs(long long c, long long* red, unsigned long long* __restrict__ n_pair) {
    c = block_sum<long long>(c, red);
    if (threadIdx.x == 0 && c) atomicAdd(n_pair, (unsigned long long)c);
}

// The row epilogue of the forward+backward kernels.  The occurrence weight cnt_super[super] ** power (and inv, the 1 / IDCG of the NDCG weight, with
// SCALED) is uniform within a segment (a segment lies inside one main group), so it multiplies the row's sums of both directions.  weight() runs in
// front of the walk, so that its dependent loads and the powf wait under the walk and not behind it; finish() behind it.  POISON: *bad != 0 (a
// taking-part row with a label outside the table's values) puts NaN into every gradient entry and loss partial.
template <bool POISON, bool SCALED>
struct PwRowEnd {
    const int32_t* super_id;
    const unsigned long long *cnt_super, *n_pair;
    const float* inv;
    float factor, power;
    int reduce_mean;
    const unsigned* bad;
    const float *long_la, *long_ga;
    float* dscores;
    __device__ __forceinline__ float weight(int64_t k) const {
        float w = 1.f;
        if (power != 0.f) {
            const float cnt = (float)cnt_super[super_id[k]];
            // cnt == 0: no pair of this main group survived, the weight is never used (avoid 0**negative = inf -> inf*0)
            w = (cnt == 0.f) ? 1.f : ((power == 1.f) ? cnt : powf(cnt, power));
        }
        if (SCALED) w *= inv[k];
        return w;
    }
    // read with weight(), in front of the walk and behind the skeleton's barrier, where its latency is hidden
    __device__ __forceinline__ bool poison() const { return POISON && *bad != 0u; }
    __device__ __forceinline__ double finish(const Member& me, int64_t k, bool is_long, float w, float la, float ga, bool poisoned) const {
        if (is_long) {
            la = long_la[k];
            ga = long_ga[k];
        }
        const float qnan = __int_as_float(0x7fc00000);
        const float denom = reduce_mean ? ((float)(*n_pair) + 1.0e-10f) : 1.f;
        dscores[me.row] = poisoned ? qnan : w * factor * ga / denom;
        return poisoned ? (double)qnan : (double)(w * la);
    }
};
__device__ __forceinline__ void pw_store_block_loss(double lsum, double* red, double* __restrict__ block_loss) {
    lsum = block_sum<double>(lsum, red);
    if (threadIdx.x == 0) block_loss[blockIdx.x] = lsum;
}

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

// pairwise.hip, for the other three files: k_pack_members without counters (members of the default rule: valid is 0 / 1), and k_loss_finalize on the
// device's pair count (the n per-workgroup fp64 loss partials summed in fixed order, divided by P + 1e-10 when reduce_mean)
int rn_pack_members(const float* scores, const float* labels, const uint8_t* mask, const int32_t* order, int64_t B, Member* mem, hipStream_t st,
                    int64_t* zero_b = nullptr, int64_t* zero_1 = nullptr);
int rn_loss_finalize(const double* part, int n, const int64_t* n_pair, int reduce_mean, float* loss, hipStream_t st);

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
