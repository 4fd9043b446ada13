// "Group these rows": the library-internal front end of every loss, metric and pooled-lookup backward -- ids -> keys -> stable radix sort -> segments.
// The one declaration of what grouping.hip and scan_sort.hip define for each other and for the one-call consumers (pairwise.hip, listwise.hip,
// dcnmix.hip); the C ABI's entries (recnow_group_keys, recnow_group_segments, ...) are in include/recnow.h.
#pragma once
#include "common.hpp"

struct RnTileFwd;         // the weight packs of the step's row-block kernels (dcnmix_tile.hpp)
struct GroupMidCtl;       // control block of the cooperative launch (group_mid.hpp)

#define RN_MAX_WORDS 8
#define RN_MAX_PASS (4 * RN_MAX_WORDS)
#define RN_TILE 2048          // keys per block per pass (256 threads x 8)
#define GM_MAXG 256           // most workgroups of the cooperative launch

struct SortPlan {
    int trivial[RN_MAX_PASS];
    int src[RN_MAX_PASS];     // which index buffer (0/1) pass p reads
    int carried[RN_MAX_PASS]; // the key buffer beside that index buffer already holds pass p's word in that order
    int final_buf;            // buffer holding the sorted order after the last pass
    int final_word;           // key word whose values lie beside that order in the key buffer (-1: none)
    int word_const[RN_MAX_WORDS];   // word w has one value over the whole batch (all four digits trivial)
    int pad[2];
};

// The workspace of recnow_group_segments, in this order (every piece 256-byte aligned).  A null `ws` gives the size in `total`.
struct RnGroupWs {
    SortPlan* plan;                             // the chain's pass plan
    unsigned* mix;                              // the chain's varying-bit words (2 per key word; sized n_words * 4 * 256 as ever)
    int32_t *idx0, *idx1;                       // B + 1 each: the two index buffers of the sort
    uint32_t *key0, *key1;                      // B + 1 each: the key word that travels beside them
    unsigned* blockhist;                        // 256 x max(blocks of RN_TILE keys, GM_MAXG)
    int32_t *head, *shead, *seg_incl, *super_incl;      // B + 1 each: the chain's head flags and their scans
    void* scan; size_t scan_bytes;              // device-wide scans of the chain (rn_scan_ws_bytes(B))
    GroupMidCtl* ctl;                           // cooperative launch: control block
    int* headcnt;                               // cooperative launch: 2 x GM_MAXG head counts
    size_t total;
};
RnGroupWs rn_group_ws(void* ws, int64_t B, int n_words);

// The one-launch routes over canonical key words (recnow_group_segments; arguments checked by the caller): one workgroup up to GS_MAXB rows of one key
// word, else the cooperative launch.  RECNOW_EUNSUPPORTED: the batch is beyond the co-resident grid -- scan_sort.hip then runs the multi-launch chain.
int rn_group_words(const uint32_t* words, const uint8_t* solo, int64_t B, int n_words, int n_words_first, int32_t* order, int32_t* seg_id,
                   int32_t* seg_first, int32_t* super_id, int32_t* n_seg, void* ws, hipStream_t st);

struct RnGroupBufs {
    int32_t *order, *seg_id, *seg_first, *super_id, *n_seg;      // outputs, as recnow_group_segments writes them
    uint32_t* words;          // scratch of the fallback: n_words x B canonical key words
    uint8_t* solo;            // B solo flags (written by the raw cooperative launch, filled and read by the fallback)
    int n_words;
};
// The step's front (recnow_dcn_mix_step only): the grouping launch may also write the weight packs on further workgroups and clear one 64-bit word
// (the step's pair counter).  zeroed / packed are set only where a launch really did so: a grouping launch without them must not mark the packs current.
struct RnGroupFront {
    const RnTileFwd* pack;            // NULL: no packs wanted
    unsigned long long* zero1;        // NULL: nothing to clear
    int zeroed, packed;               // out
};
// Groups the B > 0 rows of ONE id tensor.  The ladder, once:
//   [front != NULL: one workgroup straight from float32 / int32 ids, B <= GS_MAXB]   the step only: the pairwise loss has its own packed small route in front,
//                                                                                    and the route knows nothing of RECNOW_KEY_INF_EQUAL (the listwise loss)
//   -> one cooperative launch straight from float32 / int32 ids above GS_MAXB rows   (RECNOW_KEY_INF_EQUAL travels in key_dtype; never with packs)
//   -> fill of `solo`, recnow_group_keys, recnow_group_segments                      (every id type and size)
int rn_group_rows(const void* groups, int key_dtype, int64_t B, const RnGroupBufs& b, void* grp_ws, size_t grp_ws_bytes, hipStream_t st, RnGroupFront* front);
